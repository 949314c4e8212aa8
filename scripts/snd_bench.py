#!/usr/bin/env python3
"""The ACK side and the retransmit on the device, timed: lvlip_snd_dev and
lvlip_rtx_dev against the composed alternatives they replace.

ACK side: RECORDS pure-ACK records (status NO_DATA, ACK set) in random flow
order over FLOWS flows (1024, 65536); every flow owns a write queue of 16
frames of 536 payload bytes, built in HBM by lvlip_tso_dev, and every ack_seq
lies on a random segment boundary of its flow's queue.

  a  lvlip_snd_dev (device events)
  c  the path it replaces, wall time: the records copied to pinned host
     memory, a synchronise, lvlip_snd_cpu there over a host copy of the ring
     (made beforehand, not timed)
  one_flow: form a again with every record of flow 0 (the wave's reduction)

Retransmit: SLOTS live slots over SLOTS / 16 flows, every flow's queue of 16
frames of 1460 payload bytes (stride 1536) re-sent, rcv_nxt and the window
changed.

  a  lvlip_rtx_dev (device events)
  b  composed on the device (device events): a header patch (two strided
     torch copies into bytes 42-45 and 48-49 of every frame), then
     lvlip_tx_checksum_dev over the same frames

Before anything is timed, the device's results are checked equal, byte for
byte, to the host form's (and the composed retransmit's frames to the fused
one's).

    python scripts/snd_bench.py [--records N] [--flows N ...] [--slots N] [--warmup W] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "level-ip_amd"))

import torch  # noqa: E402

import lvlip  # noqa: E402
from lro_advance_bench import _dev, spread, wall_ms  # noqa: E402
from tso_bench import template, timed  # noqa: E402

M32 = 0xFFFFFFFF


def flows_and_sends(nflows: int, segs: int, mss: int, stride: int):
    """(reverse flows, sends): flow k's frames go out from port k; the reverse
    plan keeps that order (the key ends in the port, in network order)."""
    data = np.tile(np.frombuffer(template(mss), dtype=np.uint8), (nflows, 1))
    k = np.arange(nflows)
    data[:, 34], data[:, 35] = k >> 8, k & 0xFF
    una = (0xFFFF0000 + 7919 * k) & M32
    data[:, 38:42] = una.astype(">u4").view(np.uint8).reshape(-1, 4)
    sends = np.zeros(nflows, dtype=lvlip.TsoSend)
    sends["payload_off"], sends["out_off"] = 0, k.astype(np.uint64) * (segs * stride)
    sends["len"], sends["mss"], sends["stride"], sends["hdr"] = segs * mss, mss, stride, data
    flows = np.zeros(nflows, dtype=lvlip.LRO_FLOW_DTYPE)
    flows["saddr"], flows["daddr"] = data[:, 30:34].copy().view("<u4")[:, 0], data[:, 26:30].copy().view("<u4")[:, 0]
    flows["sport"], flows["dport"] = data[:, 36:38].copy().view("<u2")[:, 0], data[:, 34:36].copy().view("<u2")[:, 0]
    flows["rcv_nxt"], flows["rcv_wnd"], flows["out_off"], flows["user"] = 0x01020304, 1, k, k
    lvlip.lro_plan(flows)
    if flows["user"].tolist() != list(range(nflows)):
        raise SystemExit("the plan reordered the flows")
    snd = np.zeros(nflows, dtype=lvlip.SND_FLOW_DTYPE)
    snd["snd_una"], snd["snd_nxt"] = una, (una + segs * mss) & M32
    snd["nseg"], snd["rtx"], snd["win"] = segs, 1, 4321
    return flows, sends, snd


class Ring:
    def __init__(self, nflows, segs, mss, stride, dev):
        self.dev, self.nflows = dev, nflows
        self.flows, sends, self.snd = flows_and_sends(nflows, segs, mss, stride)
        nseg, ring_bytes = lvlip.tso_plan(sends)
        self.snd["seg0"] = sends["seg0"]
        self.nslots, _ = lvlip.snd_plan(self.snd)
        gen = torch.Generator(device=dev).manual_seed(1)
        payload = torch.randint(0, 256, (segs * mss,), dtype=torch.uint8, device=dev, generator=gen)
        self.ring = torch.zeros(ring_bytes + 64, dtype=torch.uint8, device=dev)
        self.fd = torch.zeros(16 * nseg, dtype=torch.uint8, device=dev)
        lvlip.tso_dev(payload, _dev(sends, dev), nseg, self.ring, self.fd)
        self.flow_t, self.snd_t = _dev(self.flows, dev), _dev(self.snd, dev)
        torch.cuda.synchronize(dev)


class AckSide(Ring):
    def __init__(self, nflows, n, dev, one_flow=False, segs=16, mss=536):
        super().__init__(nflows, segs, mss, 592, dev)
        rng = np.random.default_rng(nflows)
        rec = np.zeros(n, dtype=lvlip.LRO_REC_DTYPE)
        rec["flow"] = 0 if one_flow else rng.integers(0, nflows, n)
        rec["status"], rec["tcp_flags"] = lvlip.LRO_NO_DATA, 0x10
        acked = rng.integers(0, segs + 1, n).astype(np.uint64) * np.uint64(mss)
        rec["ack_seq"] = (self.snd["snd_una"][rec["flow"]].astype(np.uint64) + acked) & np.uint64(M32)
        self.n, self.rec = n, rec
        self.rec_t = _dev(rec, dev)
        self.res_t = torch.zeros(32 * nflows, dtype=torch.uint8, device=dev)
        self.pinned = torch.empty(16 * n, dtype=torch.uint8).pin_memory()
        self.ring_h, self.fd_h = self.ring.cpu().numpy(), self.fd.cpu().numpy().view(lvlip.FRAME_DESC_DTYPE)
        self.res_h = np.zeros(nflows, dtype=lvlip.SND_RESULT_DTYPE)

    def a(self):
        lvlip.snd_dev(self.flow_t, self.snd_t, self.rec_t, self.ring, self.fd, self.res_t)

    def c(self):
        self.pinned.copy_(self.rec_t, non_blocking=True)
        torch.cuda.synchronize(self.dev)
        rc = lvlip.lib().lvlip_snd_cpu(self.flows.ctypes.data, self.snd.ctypes.data, self.nflows, self.pinned.data_ptr(),
                                       self.n, self.ring_h.ctypes.data, self.fd_h.ctypes.data, self.res_h.ctypes.data)
        if rc != lvlip.OK:
            raise SystemExit(f"lvlip_snd_cpu: {rc}")

    def check(self):
        self.a()
        self.c()
        torch.cuda.synchronize(self.dev)
        if self.res_t.cpu().numpy().tobytes() != self.res_h.tobytes():
            raise SystemExit(f"{self.nflows} flows: the device's results differ from the host form's")
        return {"popped": int(self.res_h["popped"].sum()), "n_new": int(self.res_h["n_new"].sum())}


class Retransmit(Ring):
    """SLOTS live slots over SLOTS / per flows (at most LVLIP_LRO_MAX_FLOWS):
    `per` frames per queue, all of them re-sent."""

    def __init__(self, nslots, dev, mss=1460, stride=1536, per=16):
        nflows = nslots // per
        super().__init__(nflows, per, mss, stride, dev)
        self.stride = stride
        self.snd["rtx"] = per
        self.nslots, _ = lvlip.snd_plan(self.snd)
        self.snd_t = _dev(self.snd, dev)
        lro = np.zeros(nflows, dtype=lvlip.LRO_RESULT_DTYPE)
        lro["delivered"] = 0x1000 + np.arange(nflows)
        self.lro_t = _dev(lro, dev)
        self.out_t = torch.zeros(16 * self.nslots, dtype=torch.uint8, device=dev)
        ack = np.repeat((self.flows["rcv_nxt"].astype(np.uint64) + lro["delivered"]) & M32, per)
        self.ack_t = _dev(ack.astype(">u4"), dev).view(self.nslots, 4)
        self.win_t = _dev(np.repeat(self.snd["win"], per).astype(">u2"), dev).view(self.nslots, 2)
        self.ring2 = self.ring.clone()  # the composed form's ring
        self.frames2 = self.ring2[:self.nslots * stride].view(self.nslots, stride)
        torch.cuda.synchronize(dev)

    def a(self):
        lvlip.rtx_dev(self.flow_t, self.lro_t, self.snd_t, None, self.nslots, self.ring, self.fd, self.out_t)

    def b(self):
        self.frames2[:, 42:46] = self.ack_t
        self.frames2[:, 48:50] = self.win_t
        s = torch.cuda.current_stream(self.dev)
        rc = lvlip.lib().lvlip_tx_checksum_dev(self.ring2.data_ptr(), self.fd.data_ptr(), self.nslots, None, None,
                                               s.cuda_stream)
        if rc != lvlip.OK:
            raise SystemExit(f"lvlip_tx_checksum_dev: {rc}")

    def check(self):
        self.a()
        self.b()
        torch.cuda.synchronize(self.dev)
        if not torch.equal(self.ring, self.ring2):
            raise SystemExit("the composed retransmit's frames differ from the fused one's")
        host = self.ring[:4 * self.stride + 64].cpu().numpy().copy()
        return {"frame_bytes": int(self.nslots) * (54 + 1460), "first_frames_hash": int(host.astype(np.uint64).sum())}


def time_forms(obj, forms, warmup, repeats, dev):
    stream = torch.cuda.current_stream(dev)
    t = {k: [] for k in forms}
    for r in range(warmup + repeats):
        for k, wall in forms.items():  # alternating, one process
            torch.cuda.synchronize(dev)
            ms = wall_ms(getattr(obj, k)) if wall else timed(getattr(obj, k), stream)
            if r >= warmup:
                t[k].append(ms)
    return {k: spread(v) for k, v in t.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--flows", type=int, nargs="*", default=[1024, 65536])
    ap.add_argument("--slots", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        raise SystemExit("snd_bench needs a HIP device (nothing is timed on the CPU)")
    dev = torch.device("cuda", 0)
    snd = {}
    for nflows in args.flows:
        x = AckSide(nflows, args.records, dev)
        made = x.check()
        t = time_forms(x, {"a": False, "c": True}, args.warmup, args.repeats, dev)
        del x
        torch.cuda.empty_cache()
        one = AckSide(nflows, args.records, dev, one_flow=True)
        one.check()
        t["one_flow"] = time_forms(one, {"a": False}, args.warmup, args.repeats, dev)["a"]
        del one
        torch.cuda.empty_cache()
        snd[str(nflows)] = {"records": args.records, **made, "equal_to_host_form": True, "ms": t,
                            "ratio_c_over_a": round(t["c"]["median"] / t["a"]["median"], 2)}
    r = Retransmit(args.slots, dev)
    made = r.check()
    t = time_forms(r, {"a": False, "b": False}, args.warmup, args.repeats, dev)
    rtx = {"slots": r.nslots, **made, "equal_to_composed": True, "ms": t,
           "ratio_b_over_a": round(t["b"]["median"] / t["a"]["median"], 2)}
    res = {"script": "scripts/snd_bench.py", "device": torch.cuda.get_device_name(dev), "build_id": lvlip.BUILD_ID,
           "warmup": args.warmup, "repeats": args.repeats,
           "forms": {"snd.a": "lvlip_snd_dev (device events)",
                     "snd.c": "records to pinned host memory, synchronise, lvlip_snd_cpu over a host copy of the ring (wall)",
                     "snd.one_flow": "lvlip_snd_dev, every record of flow 0 (device events)",
                     "rtx.a": "lvlip_rtx_dev (device events)",
                     "rtx.b": "two strided torch copies into the headers, then lvlip_tx_checksum_dev (device events)"},
           "snd": snd, "rtx": rtx}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
