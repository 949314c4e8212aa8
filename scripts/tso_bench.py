#!/usr/bin/env python3
"""Segmentation on the device, timed: lvlip_tso_dev against the unfused
composition the library offered before it, on the same buffers (DESIGN.md,
"Segmentation on the device").

Workload: one send of SEGS x MSS payload bytes (default 1 048 576 x 1460) into
frame slots of STRIDE bytes (1536): about 3.1 GB of payload plus frames, far
beyond the 256 MB Infinity Cache.

  fused     lvlip_tso_dev: payload -> finished frames, one launch
  unfused   (a) a strided device copy of the payload into the frames' payload
                places (hipMemcpy2DAsync, and torch's strided copy_; the faster
                one counts),
            (b) a broadcast of the 54 header bytes into every slot,
            (c) lvlip_tx_checksum_dev over the frames (reads every byte again)

Both are timed with device events around each call, alternating fused and
unfused in one process after warm-up rounds; the median of the repeats is
reported.  Algorithmic bytes = len + sum of frame lengths + 96 n + 16 nseg
(payload read, frames written, the sends read, the descriptors written); GB/s
is over those bytes for both forms, the fraction of peak against 8 TB/s.

Before timing, the fused output is checked at this size: every payload slice
equals its source, and lvlip_tx_checksum_dev (an independent kernel) reports
every frame filled and leaves the buffer unchanged.

    python scripts/tso_bench.py [--segs N] [--mss M] [--stride S] [--warmup W] [--repeats R] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "level-ip_amd"))

import torch  # noqa: E402

import lvlip  # noqa: E402

PEAK = 8.0e12  # HBM3E, bytes/s (spec)


def template(mss: int) -> bytes:
    eth = bytes.fromhex("0a1b2c3d4e5f000c296d5025") + b"\x08\x00"
    ip = struct.pack("!BBHHHBBH4s4s", 0x45, 0, 40 + mss, 0, 0x4000, 64, 6, 0, bytes((10, 0, 0, 4)),
                     bytes((10, 0, 0, 5)))
    tcp = struct.pack("!HHIIBBHHH", 40001, 8000, 0xFFFFFF00, 0x01020304, 0x50, 0x18, 0xADBD, 0, 0)
    return eth + ip + tcp


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)  # ms


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--segs", type=int, default=1 << 20)
    ap.add_argument("--mss", type=int, default=1460)
    ap.add_argument("--stride", type=int, default=1536)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        raise SystemExit("tso_bench needs a HIP device (nothing is timed on the CPU)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    segs, mss, stride = args.segs, args.mss, args.stride
    length = segs * mss

    hdr = template(mss)
    sends = lvlip.tso_send(hdr, 0, length, mss, out_off=0, stride=stride)
    nseg, out_bytes = lvlip.tso_plan(sends)
    assert nseg == segs
    gen = torch.Generator(device=dev).manual_seed(1)
    payload = torch.randint(0, 256, (length,), dtype=torch.uint8, device=dev, generator=gen)
    sends_t = torch.from_numpy(sends.view(np.uint8).reshape(-1).copy()).to(dev)
    out = torch.zeros(segs * stride, dtype=torch.uint8, device=dev)
    fd = torch.zeros(16 * nseg, dtype=torch.uint8, device=dev)
    hdr_t = torch.frombuffer(bytearray(hdr), dtype=torch.uint8).to(dev)
    slots = out.view(segs, stride)

    def fused():
        lvlip.tso_dev(payload, sends_t, nseg, out, fd)

    # the HIP runtime this process already uses (PyTorch's own copy, as lvlip loads it)
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = ctypes.CDLL(cand if os.path.exists(cand) else "libamdhip64.so")
    hip.hipMemcpy2DAsync.restype = ctypes.c_int
    hip.hipMemcpy2DAsync.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]

    def copy_2d():
        rc = hip.hipMemcpy2DAsync(out.data_ptr() + 54, stride, payload.data_ptr(), mss, mss, segs, 3,
                                  stream.cuda_stream)  # 3: device to device
        if rc != 0:
            raise RuntimeError(f"hipMemcpy2DAsync: {rc}")

    def copy_torch():
        slots[:, 54:54 + mss].copy_(payload.view(segs, mss))

    def header():
        slots[:, :54] = hdr_t

    def checksum():
        lvlip.tx_checksum_dev(out, fd)

    # ---- the fused output at this size, before anything is timed
    fused()
    torch.cuda.synchronize(dev)
    payload_ok = bool(torch.equal(slots[:, 54:54 + mss], payload.view(segs, mss)))
    before = out.clone()
    status = lvlip.tx_checksum_dev(out, fd)
    torch.cuda.synchronize(dev)
    filled = int(status.sum())
    unchanged = bool(torch.equal(out, before))
    del before
    if not (payload_ok and filled == nseg and unchanged):
        raise SystemExit(f"fused output wrong at this size: payload_ok={payload_ok} filled={filled}/{nseg} "
                         f"unchanged={unchanged}")

    steps = {"fused": fused, "copy_2d": copy_2d, "copy_torch": copy_torch, "header": header,
             "checksum": checksum}
    try:
        copy_2d()
        torch.cuda.synchronize(dev)
    except RuntimeError as e:  # the runtime refuses the shape: torch's copy is the baseline's
        print(f"copy_2d left out: {e}", file=sys.stderr)
        del steps["copy_2d"]
    for _ in range(args.warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize(dev)
    t = {k: [] for k in steps}
    for _ in range(args.repeats):  # alternating, one process
        for k, fn in steps.items():
            t[k].append(timed(fn, stream))
    med = {k: statistics.median(v) for k, v in t.items()}
    copy_key = "copy_2d" if "copy_2d" in med and med["copy_2d"] <= med["copy_torch"] else "copy_torch"
    unfused = med[copy_key] + med["header"] + med["checksum"]
    # the same three calls back to back inside one pair of events (launch gaps included once)
    chain = []
    for _ in range(args.repeats):
        chain.append(timed(lambda: (steps[copy_key](), header(), checksum()), stream))
    unfused_chain = statistics.median(chain)

    algo = length + nseg * (54 + mss) + 96 * 1 + 16 * nseg
    res = {
        "script": "scripts/tso_bench.py", "device": torch.cuda.get_device_name(dev), "build_id": lvlip.BUILD_ID,
        "segs": segs, "mss": mss, "stride": stride, "payload_bytes": length, "out_bytes": out_bytes,
        "algorithmic_bytes": algo, "warmup": args.warmup, "repeats": args.repeats,
        "checked": {"payload_slices_equal": payload_ok, "tx_checksum_dev_filled": filled,
                    "tx_checksum_dev_left_unchanged": unchanged},
        "median_ms": {k: round(v, 4) for k, v in med.items()},
        "min_ms": {k: round(min(v), 4) for k, v in t.items()},
        "max_ms": {k: round(max(v), 4) for k, v in t.items()},
        "unfused_copy": copy_key,
        "fused_ms": round(med["fused"], 4),
        "unfused_ms": round(unfused, 4),
        "unfused_chain_ms": round(unfused_chain, 4),
        "fused_GBps": round(algo / med["fused"] / 1e6, 1),
        "fused_fraction_of_8TBps": round(algo / (med["fused"] * 1e-3) / PEAK, 4),
        "unfused_GBps": round(algo / unfused / 1e6, 1),
        "ratio_unfused_over_fused": round(unfused / med["fused"], 3),
        "ratio_chain_over_fused": round(unfused_chain / med["fused"], 3),
        "fused_wins": bool(med["fused"] < min(unfused, unfused_chain)),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
