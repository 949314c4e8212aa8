#!/usr/bin/env python3
"""The advance step of receive coalescing on the device, timed:
lvlip_lro_advance_dev against the host path it replaces.

Batch shapes, FRAMES frames (default 1 048 576) of MSS (1460) payload bytes each:

  in_order    scripts/lro_bench.py's batch: as few flows as a 2^30 window allows
              (two), one after the other, each in order
  shuffled    the same number of frames over FLOWS (4096) flows, in shuffled
              arrival order, 1 % of them arriving a second time

Forms, alternating in one process after warm-up rounds (median, min, max):

  a  lvlip_lro_advance_dev alone (device events)
  b  lvlip_lro_dev with LVLIP_RX_VERIFY_L4, then lvlip_lro_advance_dev, inside
     one pair of device events
  c  the path this replaces, wall time from the end of the receive kernel: the
     records copied to pinned host memory, then lvlip_lro_advance there
  d  lvlip_lro_advance alone on the host (wall time)

and a and c again on small batches (256, 4096, 65536 records written by numpy
in the shuffled shape, 256 records per flow), to see where the device form
starts to win.  Before anything is timed, the device results are checked equal,
byte for byte, to the host form's on the same records at that size.

    python scripts/lro_advance_bench.py [--frames N] [--flows F] [--warmup W] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "level-ip_amd"))

import torch  # noqa: E402

import lvlip  # noqa: E402
from tso_bench import template, timed  # noqa: E402

MSS, STRIDE = 1460, 1536
LRO_BENCH_FUSED_MS = 0.985  # DESIGN.md §9b, profiles/lro_1460.json: lvlip_lro_dev alone on the in_order batch


def _dev(a: np.ndarray, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


class Advance:
    """The four forms over one record array on the device."""

    def __init__(self, flows: np.ndarray, rec_t, n: int, dev, receive=None):
        self.flows, self.n, self.dev, self.receive = flows, n, dev, receive
        self.flow_t = _dev(flows, dev)
        self.rec_t = rec_t
        self.res_t = torch.zeros(48 * flows.size, dtype=torch.uint8, device=dev)
        self.ws_bytes = lvlip.lro_advance_workspace_bytes(n, flows.size)
        self.ws_t = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.pinned = torch.empty(16 * n, dtype=torch.uint8).pin_memory()
        self.host_rec = self.pinned.numpy().view(lvlip.LRO_REC_DTYPE)

    def a(self):
        lvlip.lro_advance_dev(self.flow_t, self.rec_t, self.res_t, self.ws_t)

    def b(self):
        self.receive()
        self.a()

    def c(self):
        self.pinned.copy_(self.rec_t[:16 * self.n], non_blocking=True)
        torch.cuda.synchronize(self.dev)
        return lvlip.lro_advance(self.flows, self.host_rec)

    def d(self):
        return lvlip.lro_advance(self.flows, self.host_rec)

    def check(self) -> bool:
        self.res_t.fill_(0x5A)
        self.a()
        torch.cuda.synchronize(self.dev)
        want = self.c()
        return self.res_t.cpu().numpy().tobytes() == want.tobytes()

    def time(self, warmup: int, repeats: int) -> dict:
        stream = torch.cuda.current_stream(self.dev)
        forms = ["a", "c", "d"] + (["b"] if self.receive else [])
        t = {k: [] for k in forms}
        for r in range(warmup + repeats):
            for k in forms:  # alternating, one process
                torch.cuda.synchronize(self.dev)
                ms = timed(getattr(self, k), stream) if k in "ab" else wall_ms(getattr(self, k))
                if r >= warmup:
                    t[k].append(ms)
        return {k: spread(v) for k, v in t.items()}


def frames_batch(n: int, nflows: int, shuffle: bool, dev):
    """n TSO-built frames over nflows flows in HBM -> (flows, receive, rec_t,
    records in the batch): receive() is the lvlip_lro_dev call that writes rec_t."""
    per = n // nflows
    hdrs = [bytearray(template(MSS)) for _ in range(nflows)]
    for k, h in enumerate(hdrs):
        h[34:36] = (1024 + k).to_bytes(2, "big")
    sends = np.concatenate([lvlip.tso_send(bytes(h), k * per * MSS, per * MSS, MSS, out_off=k * per * STRIDE,
                                           stride=STRIDE) for k, h in enumerate(hdrs)])
    nseg, _ = lvlip.tso_plan(sends)
    assert nseg == n
    gen = torch.Generator(device=dev).manual_seed(1)
    payload = torch.randint(0, 256, (n * MSS,), dtype=torch.uint8, device=dev, generator=gen)
    ring = torch.zeros(n * STRIDE + 16, dtype=torch.uint8, device=dev)
    fd = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    lvlip.tso_dev(payload, _dev(sends, dev), nseg, ring, fd)
    if shuffle:
        rng = np.random.default_rng(2)
        order = rng.permutation(n)
        order = np.concatenate([order, order[:n // 100]])  # 1 % arrive twice
        order = order[rng.permutation(order.size)]
        fd = fd.view(n, 16)[torch.from_numpy(order).to(dev)].contiguous().view(-1)
    m = fd.numel() // 16
    flows = np.concatenate([lvlip.lro_flow(h[26:30], h[30:34], 1024 + k, 8000, 0xFFFFFF00, per * MSS,
                                           out_off=k * per * MSS) for k, h in enumerate(hdrs)])
    lvlip.lro_plan(flows)
    flow_t = _dev(flows, dev)
    out = torch.zeros(n * MSS, dtype=torch.uint8, device=dev)
    rec_t = torch.zeros(16 * m, dtype=torch.uint8, device=dev)

    def receive():
        lvlip.lro_dev(ring, fd, flow_t, lvlip.RX_VERIFY_L4, out, rec_t)

    receive()
    torch.cuda.synchronize(dev)
    if not torch.equal(out, payload):
        raise SystemExit("the received stream is not the payload")
    return flows, receive, rec_t, m


def numpy_batch(n: int, dev):
    """n PLACED records in the shuffled shape, 256 per flow, 1 % twice."""
    nflows = max(1, n // 256)
    rng = np.random.default_rng(n)
    flows = np.concatenate([lvlip.lro_flow(bytes((10, 0, 0, 4)), bytes((10, 0, 0, 5)), 1024 + k, 8000, 0xFFFFFF00,
                                           1 << 20, out_off=k << 20) for k in range(nflows)])
    lvlip.lro_plan(flows)
    ids = rng.permutation(n - n // 100)
    ids = np.concatenate([ids, ids[:n // 100]])
    ids = ids[rng.permutation(n)]
    rec = np.zeros(n, dtype=lvlip.LRO_REC_DTYPE)
    rec["flow"], rec["rel"] = ids % nflows, (ids // nflows) * MSS
    rec["dlen"], rec["status"], rec["tcp_flags"] = MSS, lvlip.LRO_PLACED, 0x10
    return flows, _dev(rec, dev)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--flows", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--small", type=int, nargs="*", default=[256, 4096, 65536])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        raise SystemExit("lro_advance_bench needs a HIP device (nothing is timed on the CPU)")
    dev = torch.device("cuda", 0)
    n = args.frames
    few = -(-n * MSS // (1 << 30))
    if n % few or n % args.flows:
        raise SystemExit(f"{n} frames do not split evenly over {few} and {args.flows} flows")

    shapes = {}
    for name, nflows, shuffle in (("in_order", few, False), ("shuffled", args.flows, True)):
        flows, receive, rec_t, m = frames_batch(n, nflows, shuffle, dev)
        adv = Advance(flows, rec_t, m, dev, receive)
        if not adv.check():
            raise SystemExit(f"{name}: the device results differ from the host form's")
        t = adv.time(args.warmup, args.repeats)
        shapes[name] = {"records": m, "flows": nflows, "workspace_bytes": adv.ws_bytes, "equal_to_host_form": True,
                        "ms": t, "ratio_c_over_a": round(t["c"]["median"] / t["a"]["median"], 1),
                        "b_minus_lro_bench_fused_ms": round(t["b"]["median"] - LRO_BENCH_FUSED_MS, 4)}
        del adv, receive, rec_t
        torch.cuda.empty_cache()

    small = {}
    for m in args.small:
        flows, rec_t = numpy_batch(m, dev)
        adv = Advance(flows, rec_t, m, dev)
        if not adv.check():
            raise SystemExit(f"{m} records: the device results differ from the host form's")
        t = adv.time(args.warmup, args.repeats)
        small[str(m)] = {"flows": int(flows.size), "workspace_bytes": adv.ws_bytes, "equal_to_host_form": True,
                         "ms": {k: t[k] for k in "ac"}, "ratio_c_over_a": round(t["c"]["median"] / t["a"]["median"], 2)}
    wins = [int(m) for m, v in small.items() if v["ratio_c_over_a"] > 1.0]
    res = {"script": "scripts/lro_advance_bench.py", "device": torch.cuda.get_device_name(dev),
           "build_id": lvlip.BUILD_ID, "frames": n, "mss": MSS, "warmup": args.warmup, "repeats": args.repeats,
           "forms": {"a": "lvlip_lro_advance_dev (device events)",
                     "b": "lvlip_lro_dev + lvlip_lro_advance_dev (one pair of device events)",
                     "c": "records to pinned host memory + lvlip_lro_advance (wall)",
                     "d": "lvlip_lro_advance on the host (wall)"},
           "lro_bench_fused_ms": LRO_BENCH_FUSED_MS, "shapes": shapes, "small": small,
           "smallest_size_where_a_beats_c": min(wins) if wins else None}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
