#!/usr/bin/env python3
"""The acknowledgement step of receive coalescing on the device, timed:
lvlip_ack_dev against the host path it replaces.

Batch shapes, FLOWS flows (256, 4096, 65536) with frames of MSS (536) payload
bytes, built in HBM by lvlip_tso_dev:

  all_ack     one in-order frame per flow: every flow gets a 54-byte ACK
  sack_heavy  segments 0, 2, 4, 6, 8 of nine per flow: a prefix and four
              islands, every flow gets a 90-byte ACK with four SACK blocks

Forms, alternating in one process after warm-up rounds (median, min, max):

  a  lvlip_ack_dev alone (device events)
  b  lvlip_lro_dev with LVLIP_RX_VERIFY_L4, lvlip_lro_advance_dev and
     lvlip_ack_dev inside one pair of device events
  c  the path a replaces, wall time from the end of the advance step: the
     results copied to pinned host memory, a synchronise, lvlip_ack_cpu into
     pinned memory, the frames copied back to the device

Before anything is timed at a size, the device's frames and fd are checked
equal, byte for byte, to the host form's on the same results.

    python scripts/ack_bench.py [--flows N ...] [--warmup W] [--repeats R] [--out FILE]
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

MSS, STRIDE = 536, 592
SHAPES = {"all_ack": (1, (0,)), "sack_heavy": (9, (0, 2, 4, 6, 8))}


def headers(nflows: int):
    """(data headers, ACK headers), nflows x 54: the peers differ in their
    source port, and the stack answers each from the reversed addresses."""
    data = np.tile(np.frombuffer(template(MSS), dtype=np.uint8), (nflows, 1))
    k = np.arange(nflows)
    data[:, 34], data[:, 35] = k >> 8, k & 0xFF
    ack = data.copy()
    ack[:, 0:6], ack[:, 6:12] = data[:, 6:12], data[:, 0:6]
    ack[:, 26:30], ack[:, 30:34] = data[:, 30:34], data[:, 26:30]
    ack[:, 34:36], ack[:, 36:38] = data[:, 36:38], data[:, 34:36]
    ack[:, 38:42], ack[:, 42:46] = data[:, 42:46], 0  # seq = the peer's ack_seq
    ack[:, 47] = 0x10
    return data, ack


class Loop:
    """The receive loop of nflows flows in HBM, up to the ACK frames."""

    def __init__(self, nflows: int, segs: int, keep, dev):
        self.dev, self.nflows = dev, nflows
        data, ack = headers(nflows)
        k = np.arange(nflows, dtype=np.uint64)
        sends = np.zeros(nflows, dtype=lvlip.TsoSend)
        sends["payload_off"], sends["out_off"] = k * (segs * MSS), k * (segs * STRIDE)
        sends["len"], sends["mss"], sends["stride"], sends["hdr"] = segs * MSS, MSS, STRIDE, data
        nseg, ring_bytes = lvlip.tso_plan(sends)
        gen = torch.Generator(device=dev).manual_seed(1)
        payload = torch.randint(0, 256, (nflows * segs * MSS,), dtype=torch.uint8, device=dev, generator=gen)
        self.ring = torch.zeros(ring_bytes + 32, dtype=torch.uint8, device=dev)
        fd = torch.zeros(16 * nseg, dtype=torch.uint8, device=dev)
        lvlip.tso_dev(payload, _dev(sends, dev), nseg, self.ring, fd)
        rng = np.random.default_rng(nflows)
        arrive = (np.arange(nflows)[:, None] * segs + np.asarray(keep)[None, :]).reshape(-1)
        arrive = arrive[rng.permutation(arrive.size)]  # the network's order
        self.fd = fd.view(nseg, 16)[torch.from_numpy(arrive).to(dev)].contiguous().view(-1)
        self.n = arrive.size

        flows = np.zeros(nflows, dtype=lvlip.LRO_FLOW_DTYPE)
        flows["saddr"], flows["daddr"] = data[:, 26:30].copy().view("<u4")[:, 0], data[:, 30:34].copy().view("<u4")[:, 0]
        flows["sport"], flows["dport"] = data[:, 34:36].copy().view("<u2")[:, 0], data[:, 36:38].copy().view("<u2")[:, 0]
        flows["rcv_nxt"], flows["rcv_wnd"], flows["out_off"], flows["user"] = 0xFFFFFF00, segs * MSS, k * (segs * MSS), k
        lvlip.lro_plan(flows)
        self.flows = flows
        self.tmpl = np.zeros(nflows, dtype=lvlip.ACK_TMPL_DTYPE)
        self.tmpl["hdr"] = ack[flows["user"].astype(np.int64)]  # the plan reordered the flows
        self.tmpl["out_off"], self.tmpl["max_sack"] = np.arange(nflows) * lvlip.ACK_MAX_FRAME, 4
        self.ack_bytes = lvlip.ack_plan(self.tmpl, flows)

        self.flow_t, self.tmpl_t = _dev(flows, dev), _dev(self.tmpl, dev)
        self.stream_t = torch.zeros(nflows * segs * MSS, dtype=torch.uint8, device=dev)
        self.rec_t = torch.zeros(16 * self.n, dtype=torch.uint8, device=dev)
        self.res_t = torch.zeros(48 * nflows, dtype=torch.uint8, device=dev)
        self.ws_t = torch.empty(lvlip.lro_advance_workspace_bytes(self.n, nflows), dtype=torch.uint8, device=dev)
        self.ack_t = torch.zeros(self.ack_bytes, dtype=torch.uint8, device=dev)
        self.afd_t = torch.zeros(16 * nflows, dtype=torch.uint8, device=dev)
        self.ack_c_t = torch.zeros(self.ack_bytes, dtype=torch.uint8, device=dev)
        self.res_pin = torch.empty(48 * nflows, dtype=torch.uint8).pin_memory()
        self.ack_pin = torch.zeros(self.ack_bytes, dtype=torch.uint8).pin_memory()
        self.afd_host = np.zeros(nflows, dtype=lvlip.FRAME_DESC_DTYPE)
        self.receive_and_advance()
        torch.cuda.synchronize(dev)

    def receive_and_advance(self):
        lvlip.lro_dev(self.ring, self.fd, self.flow_t, lvlip.RX_VERIFY_L4, self.stream_t, self.rec_t)
        lvlip.lro_advance_dev(self.flow_t, self.rec_t, self.res_t, self.ws_t)

    def a(self):
        lvlip.ack_dev(self.tmpl_t, self.flow_t, self.res_t, 0, self.ack_t, self.afd_t)

    def b(self):
        self.receive_and_advance()
        self.a()

    def c(self):
        self.res_pin.copy_(self.res_t, non_blocking=True)
        torch.cuda.synchronize(self.dev)
        rc = lvlip.lib().lvlip_ack_cpu(self.tmpl.ctypes.data, self.flows.ctypes.data, self.res_pin.data_ptr(),
                                       self.nflows, 0, self.ack_pin.data_ptr(), self.afd_host.ctypes.data)
        if rc != lvlip.OK:
            raise SystemExit(f"lvlip_ack_cpu: {rc}")
        self.ack_c_t.copy_(self.ack_pin, non_blocking=True)
        torch.cuda.synchronize(self.dev)

    def check(self) -> dict:
        self.ack_t.fill_(0x5A)
        self.ack_pin.fill_(0x5A)
        self.a()
        self.c()
        torch.cuda.synchronize(self.dev)
        lens = self.afd_host["len"]
        if not (torch.equal(self.ack_t, self.ack_c_t)
                and self.afd_t.cpu().numpy().tobytes() == self.afd_host.tobytes()):
            raise SystemExit(f"{self.nflows} flows: the device's frames differ from the host form's")
        return {"frames": int((lens > 0).sum()), "frame_bytes": int(lens.sum())}

    def time(self, warmup: int, repeats: int) -> dict:
        stream = torch.cuda.current_stream(self.dev)
        t = {k: [] for k in "abc"}
        for r in range(warmup + repeats):
            for k in "abc":  # alternating, one process
                torch.cuda.synchronize(self.dev)
                ms = timed(getattr(self, k), stream) if k in "ab" else wall_ms(self.c)
                if r >= warmup:
                    t[k].append(ms)
        return {k: spread(v) for k, v in t.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, nargs="*", default=[256, 4096, 65536])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=31)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        raise SystemExit("ack_bench needs a HIP device (nothing is timed on the CPU)")
    dev = torch.device("cuda", 0)
    shapes = {}
    for name, (segs, keep) in SHAPES.items():
        shapes[name] = {}
        for nflows in args.flows:
            loop = Loop(nflows, segs, keep, dev)
            made = loop.check()
            t = loop.time(args.warmup, args.repeats)
            shapes[name][str(nflows)] = {"records": loop.n, **made, "equal_to_host_form": True, "ms": t,
                                         "ratio_c_over_a": round(t["c"]["median"] / t["a"]["median"], 2)}
            del loop
            torch.cuda.empty_cache()
    res = {"script": "scripts/ack_bench.py", "device": torch.cuda.get_device_name(dev), "build_id": lvlip.BUILD_ID,
           "mss": MSS, "warmup": args.warmup, "repeats": args.repeats,
           "forms": {"a": "lvlip_ack_dev (device events)",
                     "b": "lvlip_lro_dev + lvlip_lro_advance_dev + lvlip_ack_dev (one pair of device events)",
                     "c": "results to pinned host memory, synchronise, lvlip_ack_cpu into pinned memory, frames back "
                          "to the device (wall)"},
           "shapes": shapes}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
