#!/usr/bin/env python3
"""The scoreboard and the selective retransmit on the device, timed:
lvlip_sack_dev against the host path it replaces, and lvlip_rtx_sack_dev
against lvlip_rtx_dev.

Scoreboard: RECORDS ACK frames (90-byte slots of 96, NOP NOP SACK with 1-4
blocks, status NO_DATA, ACK set) in random flow order over FLOWS flows (1024,
65536); every flow owns a write queue of 16 frames of 536 payload bytes, built
in HBM by lvlip_tso_dev, and block j of a frame covers 1-3 whole segments from
segment 1 + 4 j of its flow's queue.  one_flow: every record of flow 0, whose
queue holds 65 536 frames, each block 1-3 segments anywhere in it.

  a  lvlip_sack_dev (device events); the scoreboard keeps its marks between
     repeats, and every repeat stores the same ones again
  c  the path it replaces, wall time: records and ACK frames copied to pinned
     host memory, a synchronise, lvlip_sack_cpu there over a host copy of the
     ring (made beforehand, not timed), the scoreboard copied back to the
     device, a synchronise

Retransmit: 65 536 flows, queues of 16 frames of 1460 payload bytes (stride
1536), rtx 4 or 16 slots a flow.

  rtx        lvlip_rtx_dev (device events)
  parent     lvlip_rtx_dev of the library given by --parent-lib (the commit
             before lvlip_rtx_sack_*: k_rtx without the pick argument)
  sack0      lvlip_rtx_sack_dev, no mark set: the same frames as rtx
  sack6of8   lvlip_rtx_sack_dev, entries 0-5 of every 8 marked (rtx 4 only:
             the four free entries 6, 7, 14, 15 are re-sent)

Before anything is timed the device's res and scoreboard are checked equal,
byte for byte, to the host form's, sack0's ring, fd_out and the parent's ring
to rtx's, and sack6of8's pick and fd_out to lvlip_rtx_sack_cpu's.

    python scripts/sack_bench.py [--records N] [--flows N ...] [--parent-lib SO] [--warmup W] [--repeats R] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "level-ip_amd"))

import torch  # noqa: E402

import lvlip  # noqa: E402
from lro_advance_bench import _dev  # noqa: E402
from snd_bench import M32, Ring, time_forms  # noqa: E402

SLOT = 96  # bytes per ACK frame slot


def ack_frames(snd, flow, segs, mss, rng, anywhere):
    """n ACK frames of 54 + 4 + 8 b bytes in slots of SLOT; returns (bytes, fd)."""
    n = flow.size
    b = rng.integers(1, 5, n)
    fr = np.zeros((n, SLOT), dtype=np.uint8)
    fr[:, 12:14] = (8, 0)
    fr[:, 14] = 0x45
    fr[:, 23] = 6
    fr[:, 46] = (5 + 1 + 2 * b) << 4
    fr[:, 47] = 0x10
    fr[:, 54:57] = (1, 1, 5)
    fr[:, 57] = 2 + 8 * b
    una = snd["snd_una"][flow].astype(np.uint64)
    for j in range(4):
        start = rng.integers(0, segs - 3, n) if anywhere else np.full(n, 1 + 4 * j)
        left = (una + start.astype(np.uint64) * mss) & M32
        right = (left + rng.integers(1, 4, n).astype(np.uint64) * mss) & M32
        blk = np.concatenate([left.astype(">u4").view(np.uint8).reshape(n, 4), right.astype(">u4").view(np.uint8).reshape(n, 4)], 1)
        fr[:, 58 + 8 * j:66 + 8 * j] = np.where((b > j)[:, None], blk, 0)
    fd = np.zeros(n, dtype=lvlip.FRAME_DESC_DTYPE)
    fd["offset"], fd["len"] = np.arange(n, dtype=np.uint64) * SLOT, 58 + 8 * b
    return fr.reshape(-1), fd


class Scoreboard(Ring):
    def __init__(self, nflows, n, dev, segs=16, mss=536, one_flow=False):
        super().__init__(nflows, segs, mss, 592, dev)
        rng = np.random.default_rng(nflows + segs)
        rec = np.zeros(n, dtype=lvlip.LRO_REC_DTYPE)
        rec["flow"] = 0 if one_flow else rng.integers(0, nflows, n)
        rec["status"], rec["tcp_flags"] = lvlip.LRO_NO_DATA, 0x10
        rec["ack_seq"] = self.snd["snd_una"][rec["flow"]]
        acks, afd = ack_frames(self.snd, rec["flow"], segs, mss, rng, anywhere=one_flow)
        self.n, self.nfd = n, nflows * segs
        self.rec_t, self.acks_t, self.afd_t = _dev(rec, dev), _dev(acks, dev), _dev(afd, dev)
        self.afd_h = afd
        self.board_t = torch.zeros(self.nfd, dtype=torch.uint8, device=dev)
        self.res_t = torch.zeros(16 * nflows, dtype=torch.uint8, device=dev)
        self.ws_t = torch.empty(lvlip.sack_workspace_bytes(n, nflows), dtype=torch.uint8, device=dev)
        self.pin_rec = torch.empty(16 * n, dtype=torch.uint8).pin_memory()
        self.pin_acks = torch.empty(acks.size, dtype=torch.uint8).pin_memory()
        self.pin_board = torch.zeros(self.nfd, dtype=torch.uint8).pin_memory()
        self.board2_t = torch.zeros(self.nfd, dtype=torch.uint8, device=dev)
        self.ring_h, self.fd_h = self.ring.cpu().numpy(), self.fd.cpu().numpy().view(lvlip.FRAME_DESC_DTYPE)
        self.res_h = np.zeros(nflows, dtype=lvlip.SACK_RESULT_DTYPE)

    def a(self):
        lvlip.sack_dev(self.flow_t, self.snd_t, self.rec_t, self.acks_t, self.afd_t, self.ring, self.fd, self.board_t,
                       self.res_t, workspace_t=self.ws_t)

    def c(self):
        self.pin_rec.copy_(self.rec_t, non_blocking=True)
        self.pin_acks.copy_(self.acks_t, non_blocking=True)
        torch.cuda.synchronize(self.dev)
        rc = lvlip.lib().lvlip_sack_cpu(self.flows.ctypes.data, self.snd.ctypes.data, self.nflows, self.pin_rec.data_ptr(),
                                        self.pin_acks.data_ptr(), self.afd_h.ctypes.data, self.n, self.ring_h.ctypes.data,
                                        self.fd_h.ctypes.data, self.pin_board.data_ptr(), self.res_h.ctypes.data)
        if rc != lvlip.OK:
            raise SystemExit(f"lvlip_sack_cpu: {rc}")
        self.board2_t.copy_(self.pin_board, non_blocking=True)
        torch.cuda.synchronize(self.dev)

    def check(self):
        self.a()
        self.c()
        torch.cuda.synchronize(self.dev)
        if self.res_t.cpu().numpy().tobytes() != self.res_h.tobytes() or not torch.equal(self.board_t, self.board2_t):
            raise SystemExit(f"{self.nflows} flows: the device's scoreboard or results differ from the host form's")
        return {"n_blocks": int(self.res_h["n_blocks"].sum()), "n_valid": int(self.res_h["n_valid"].sum()),
                "n_sacked": int(self.res_h["n_sacked"].sum()), "entries": self.nfd}


class Selective(Ring):
    def __init__(self, nflows, rtx, dev, parent, mss=1460, stride=1536, per=16):
        super().__init__(nflows, per, mss, stride, dev)
        self.snd["rtx"] = rtx
        self.nslots, _ = lvlip.snd_plan(self.snd)
        self.snd_t = _dev(self.snd, dev)
        self.lro = np.zeros(nflows, dtype=lvlip.LRO_RESULT_DTYPE)
        self.lro["delivered"] = 0x1000 + np.arange(nflows)
        self.lro_t = _dev(self.lro, dev)
        self.out_t = torch.zeros(16 * self.nslots, dtype=torch.uint8, device=dev)
        self.out2_t = torch.zeros(16 * self.nslots, dtype=torch.uint8, device=dev)
        self.pick_t = torch.zeros(4 * self.nslots, dtype=torch.uint8, device=dev)
        self.none_t = torch.zeros(nflows * per, dtype=torch.uint8, device=dev)
        self.marks = np.tile(np.array([1] * 6 + [0] * 2, dtype=np.uint8), nflows * per // 8)
        self.marks_t = _dev(self.marks, dev)
        self.parent_lib = parent
        torch.cuda.synchronize(dev)

    def rtx(self):
        lvlip.rtx_dev(self.flow_t, self.lro_t, self.snd_t, None, self.nslots, self.ring, self.fd, self.out_t)

    def parent(self):
        s = torch.cuda.current_stream(self.dev)
        rc = self.parent_lib.lvlip_rtx_dev(self.flow_t.data_ptr(), self.lro_t.data_ptr(), self.snd_t.data_ptr(), None,
                                           self.nflows, self.nslots, self.ring.data_ptr(), self.fd.data_ptr(),
                                           self.out2_t.data_ptr(), s.cuda_stream)
        if rc != lvlip.OK:
            raise SystemExit(f"the parent's lvlip_rtx_dev: {rc}")

    def sack0(self):
        lvlip.rtx_sack_dev(self.flow_t, self.lro_t, self.snd_t, None, self.none_t, self.nslots, self.ring, self.fd,
                           self.out2_t, self.pick_t)

    def sack6of8(self):
        lvlip.rtx_sack_dev(self.flow_t, self.lro_t, self.snd_t, None, self.marks_t, self.nslots, self.ring, self.fd,
                           self.out2_t, self.pick_t)

    def check(self, forms):
        self.rtx()
        torch.cuda.synchronize(self.dev)
        want = self.ring.clone()
        for name in ("parent", "sack0"):
            if name not in forms:
                continue
            self.ring.copy_(self.fresh)
            getattr(self, name)()
            torch.cuda.synchronize(self.dev)
            if not torch.equal(self.ring, want) or not torch.equal(self.out_t, self.out2_t):
                raise SystemExit(f"{name}: ring or fd_out differ from lvlip_rtx_dev's")
        if "sack6of8" in forms:
            self.sack6of8()
            torch.cuda.synchronize(self.dev)
            ring_h = self.fresh.cpu().numpy()
            fd_h = self.fd.cpu().numpy().view(lvlip.FRAME_DESC_DTYPE)
            fd_out, pick = lvlip.rtx_sack_cpu(self.flows, self.lro, self.snd, None, self.marks, ring_h, fd_h)
            if self.pick_t.cpu().numpy().tobytes() != pick.tobytes() or self.out2_t.cpu().numpy().tobytes() != fd_out.tobytes():
                raise SystemExit("sack6of8: pick or fd_out differ from lvlip_rtx_sack_cpu's")
            if sorted(set((pick.reshape(-1, 4) % 16).reshape(-1).tolist())) != [6, 7, 14, 15]:
                raise SystemExit("sack6of8: the picked entries are not 6, 7, 14, 15 of every queue")
        return {"slots": self.nslots, "frame_bytes": int(self.nslots) * (54 + 1460)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--flows", type=int, nargs="*", default=[1024, 65536])
    ap.add_argument("--long-queue", type=int, default=65536)
    ap.add_argument("--rtx-flows", type=int, default=65536)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        raise SystemExit("sack_bench needs a HIP device (nothing is timed on the CPU)")
    dev = torch.device("cuda", 0)
    sack = {}
    cases = [(str(nf), dict(nflows=nf)) for nf in args.flows] + [("one_flow", dict(nflows=1, segs=args.long_queue, one_flow=True))]
    for name, kw in cases:
        x = Scoreboard(n=args.records, dev=dev, **kw)
        made = x.check()
        t = time_forms(x, {"a": False, "c": True}, args.warmup, args.repeats, dev)
        sack[name] = {"records": args.records, **made, "equal_to_host_form": True, "ms": t,
                      "ratio_c_over_a": round(t["c"]["median"] / t["a"]["median"], 2)}
        del x
        torch.cuda.empty_cache()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.lvlip_rtx_dev.restype = ctypes.c_int
        parent.lvlip_rtx_dev.argtypes = lvlip.SIGNATURES["lvlip_rtx_dev"][1]
    rtx = {}
    for per_flow in (4, 16):
        forms = ["rtx", "sack0"] + (["parent"] if parent is not None else []) + (["sack6of8"] if per_flow == 4 else [])
        r = Selective(args.rtx_flows, per_flow, dev, parent)
        r.fresh = r.ring.clone()
        made = r.check(forms)
        del r.fresh
        torch.cuda.empty_cache()
        t = time_forms(r, {k: False for k in forms}, args.warmup, args.repeats, dev)
        rtx[f"rtx{per_flow}"] = {**made, "equal": True, "ms": t,
                                 "sack0_minus_rtx_ms": round(t["sack0"]["median"] - t["rtx"]["median"], 4),
                                 **({"rtx_over_parent": round(t["rtx"]["median"] / t["parent"]["median"], 3)}
                                    if parent is not None else {})}
        del r
        torch.cuda.empty_cache()
    res = {"script": "scripts/sack_bench.py", "device": torch.cuda.get_device_name(dev), "build_id": lvlip.BUILD_ID,
           "warmup": args.warmup, "repeats": args.repeats,
           "forms": {"sack.a": "lvlip_sack_dev (device events)",
                     "sack.c": "records and ACK frames to pinned host memory, synchronise, lvlip_sack_cpu over a host copy "
                               "of the ring, scoreboard back to the device, synchronise (wall)",
                     "rtx.rtx": "lvlip_rtx_dev (device events)",
                     "rtx.parent": "lvlip_rtx_dev of the parent commit's library (device events)",
                     "rtx.sack0": "lvlip_rtx_sack_dev, no marks (device events)",
                     "rtx.sack6of8": "lvlip_rtx_sack_dev, 6 of every 8 entries marked (device events)"},
           "sack": sack, "rtx": rtx}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
