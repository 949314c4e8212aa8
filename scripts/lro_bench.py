#!/usr/bin/env python3
"""Receive coalescing on the device, timed: lvlip_lro_dev against the
composition the library offered before it, on the same buffers (DESIGN.md
§9b).

Workload: FRAMES frames (default 1 048 576) of MSS (1460) payload bytes in
slots of STRIDE (1536) bytes, in order: about 3.1 GB of frames and stream, far
beyond the 256 MB Infinity Cache.  A flow's window is at most 2^30 bytes, so
the frames belong to as few flows as that allows (two at the default size),
one after the other, each in order.

  fused       lvlip_lro_dev with LVLIP_RX_VERIFY_L4: frames -> verified stream
              bytes and records, one launch
  unfused     lvlip_rx_verify_dev with LVLIP_RX_VERIFY_L4, then a torch strided
              copy_ of the payload columns (all an in-order, one-flow,
              equal-length batch needs; it cannot place anything else)
  one pass    lvlip_lro_dev with flags 0 against the strided copy alone

Device events around each form, the forms alternating in one process after
warm-up rounds; median, min and max of the repeats.  Before timing, the
outputs are checked equal: both streams are the payload, every record is
PLACED at its place, every verdict is OK.

    python scripts/lro_bench.py [--frames N] [--mss M] [--stride S] [--warmup W] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "level-ip_amd"))

import torch  # noqa: E402

import lvlip  # noqa: E402
from tso_bench import template, timed  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--mss", type=int, default=1460)
    ap.add_argument("--stride", type=int, default=1536)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        raise SystemExit("lro_bench needs a HIP device (nothing is timed on the CPU)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    n, mss, stride = args.frames, args.mss, args.stride
    length = n * mss
    nflows = -(-length // (1 << 30))
    if n % nflows:
        raise SystemExit(f"{n} frames do not split evenly over {nflows} flows")
    per = n // nflows  # frames of one flow

    # the frames: the segmentation kernel's, RFC-clean addresses (10.0.0.4 -> 10.0.0.5 loses no carry)
    hdrs = [bytearray(template(mss)) for _ in range(nflows)]
    for k, h in enumerate(hdrs):
        h[34:36] = (40001 + k).to_bytes(2, "big")
    sends = np.concatenate([lvlip.tso_send(bytes(h), k * per * mss, per * mss, mss, out_off=k * per * stride,
                                           stride=stride) for k, h in enumerate(hdrs)])
    nseg, _ = lvlip.tso_plan(sends)
    assert nseg == n
    gen = torch.Generator(device=dev).manual_seed(1)
    payload = torch.randint(0, 256, (length,), dtype=torch.uint8, device=dev, generator=gen)
    sends_t = torch.from_numpy(sends.view(np.uint8).reshape(-1).copy()).to(dev)
    ring = torch.zeros(n * stride + 16, dtype=torch.uint8, device=dev)
    fd = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    lvlip.tso_dev(payload, sends_t, nseg, ring, fd)
    flow = np.concatenate([lvlip.lro_flow(h[26:30], h[30:34], 40001 + k, 8000, 0xFFFFFF00, per * mss,
                                          out_off=k * per * mss) for k, h in enumerate(hdrs)])
    lvlip.lro_plan(flow)
    flow_t = torch.from_numpy(flow.view(np.uint8).reshape(-1).copy()).to(dev)
    out_f = torch.zeros(length, dtype=torch.uint8, device=dev)
    out_u = torch.zeros(length, dtype=torch.uint8, device=dev)
    rec = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    slots = ring[:n * stride].view(n, stride)
    L4 = lvlip.RX_VERIFY_L4

    def fused():
        lvlip.lro_dev(ring, fd, flow_t, L4, out_f, rec)

    def one_pass():
        lvlip.lro_dev(ring, fd, flow_t, 0, out_f, rec)

    verdicts = []

    def verify():
        verdicts[:] = [lvlip.rx_verify_dev(ring, fd, L4)]

    def copy():
        out_u.view(n, mss).copy_(slots[:, 54:54 + mss])

    # ---- the outputs, before anything is timed
    checked = {}
    for name, fn in (("fused", fused), ("one_pass", one_pass)):
        out_f.zero_()
        fn()
        torch.cuda.synchronize(dev)
        r = rec.cpu().numpy().view(lvlip.LRO_REC_DTYPE)
        checked[name + "_stream_is_payload"] = bool(torch.equal(out_f, payload))
        checked[name + "_records_placed_in_order"] = bool(
            (r["status"] == lvlip.LRO_PLACED).all() and (r["rel"] == np.tile(np.arange(per, dtype=np.uint64) * mss, nflows)).all())
    verify()
    copy()
    torch.cuda.synchronize(dev)
    checked["unfused_stream_is_payload"] = bool(torch.equal(out_u, payload))
    checked["unfused_verdicts_ok"] = bool((verdicts[0] == lvlip.RX_OK).all())
    if not all(checked.values()):
        raise SystemExit(f"outputs differ at this size: {checked}")

    steps = {"fused": fused, "verify": verify, "copy": copy, "one_pass": one_pass}
    for _ in range(args.warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize(dev)
    t = {k: [] for k in steps}
    t["unfused_chain"] = []
    for _ in range(args.repeats):  # alternating, one process
        for k, fn in steps.items():
            t[k].append(timed(fn, stream))
        t["unfused_chain"].append(timed(lambda: (verify(), copy()), stream))
    med = {k: statistics.median(v) for k, v in t.items()}
    unfused = med["verify"] + med["copy"]
    frames_bytes = n * (54 + mss)
    algo = frames_bytes + length + 16 * n + 16 * n  # frames read, stream written, descriptors read, records written
    res = {
        "script": "scripts/lro_bench.py", "device": torch.cuda.get_device_name(dev), "build_id": lvlip.BUILD_ID,
        "frames": n, "flows": nflows, "mss": mss, "stride": stride, "stream_bytes": length, "algorithmic_bytes": algo,
        "warmup": args.warmup, "repeats": args.repeats, "checked": checked,
        "median_ms": {k: round(v, 4) for k, v in med.items()},
        "min_ms": {k: round(min(v), 4) for k, v in t.items()},
        "max_ms": {k: round(max(v), 4) for k, v in t.items()},
        "fused_ms": round(med["fused"], 4), "unfused_ms": round(unfused, 4),
        "fused_GBps": round(algo / med["fused"] / 1e6, 1),
        "ratio_unfused_over_fused": round(unfused / med["fused"], 3),
        "ratio_chain_over_fused": round(med["unfused_chain"] / med["fused"], 3),
        "one_pass_GBps": round(algo / med["one_pass"] / 1e6, 1),
        "ratio_copy_over_one_pass": round(med["copy"] / med["one_pass"], 3),
    }
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
