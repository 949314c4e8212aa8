#!/usr/bin/env python3
"""The persist timer on the device, timed.

lvlip_persist_dev at 1 024 and 65 536 flows with none, a quarter and all of
the flows firing (every flow is stalled with its timer armed; a flow that does
not fire waits, so it still loads its words and stores its state and results).

Each is set against the host alternative the earlier sections use: what the
CPU form reads (f, s, w, t, p) goes to pinned memory on the stream, one
synchronise, lvlip_persist_cpu, and p, res, fd_out and the frames go back.

Method: warm-up rounds, then REPEATS timed rounds, device form and host
alternative alternating in one process; device events around the device call,
wall clock around the host alternative; median and range.  The state the call
changes is restored from a pristine copy before every round, outside the
timing.  Before timing, every output byte of the device form is checked
against the CPU form at the size that is timed.

    python scripts/persist_bench.py [--warmup W] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "level-ip_amd"))

import torch  # noqa: E402

import lvlip  # noqa: E402

NOW = 1_000_000


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)  # ms


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def summary(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), rounds=len(ms))


def t_of(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def pinned(nbytes):
    return torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()


def case(nflows, share, rng):
    """Every flow stalled and armed; the first `share` of each four has a timer that ran out."""
    f = np.zeros(nflows, dtype=lvlip.LRO_FLOW_DTYPE)
    f["rcv_nxt"], f["rcv_wnd"] = rng.integers(0, 1 << 32, nflows, dtype=np.uint64), 1
    s = np.zeros(nflows, dtype=lvlip.SND_FLOW_DTYPE)
    s["snd_una"] = s["snd_nxt"] = rng.integers(0, 1 << 32, nflows, dtype=np.uint64)
    s["win"] = 29200
    w = np.zeros(nflows, dtype=lvlip.PUSH_FLOW_DTYPE)
    w["unsent"], w["mss"], w["wnd"] = 1 << 20, 1460, 0
    hdr = bytes(12) + b"\x08\x00" + struct.pack("!BBHHHBBH4s4s", 0x45, 0, 0, 7, 0x4000, 64, 6, 0, bytes([10, 0, 0, 4]),
                                                bytes([10, 0, 0, 5])) + \
        struct.pack("!HHIIBBHHH", 40000, 8000, 0, 0, 0x50, 0x18, 0, 0, 0)
    w["hdr"] = np.frombuffer(hdr, dtype=np.uint8)
    w["hdr"][:, 34:36] = (np.arange(nflows) & 0xFFFF).astype(">u2").view(np.uint8).reshape(nflows, 2)
    t = lvlip.rto_flows(nflows)
    p = lvlip.persist_flows(nflows)
    p["armed"], p["interval"], p["probes"] = 1, 1000, 1
    p["expires"] = np.where(np.arange(nflows) % 4 < share, NOW - 1, NOW + 500)
    return f, s, w, t, p


def bench(nflows, share, a, dev, stream, rng):
    f, s, w, t, p = case(nflows, share, rng)
    d = {k: t_of(v, dev) for k, v in dict(f=f, s=s, w=w, t0=t, p0=p).items()}
    d["t"], d["p"] = d["t0"].clone(), d["p0"].clone()
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
    out, fd, res = z(64 * nflows), z(16 * nflows), z(16 * nflows)
    run = lambda: lvlip.persist_dev(d["f"], None, d["s"], d["w"], d["t"], d["p"], NOW, out, fd, res, stream=stream)  # noqa: E731
    run()
    stream.synchronize()
    ht, hp = t.copy(), p.copy()
    hout, hfd, hres = lvlip.persist_cpu(f, None, s, w, ht, hp, NOW)
    for name, got, want in (("t", d["t"], ht), ("p", d["p"], hp), ("out", out, hout), ("fd_out", fd, hfd), ("res", res, hres)):
        if got.cpu().numpy().tobytes() != want.tobytes():
            raise SystemExit(f"persist_bench: {name} differs from lvlip_persist_cpu")
    fired = int(hres["fired"].sum())
    if fired != sum(1 for k in range(nflows) if k % 4 < share):
        raise SystemExit("persist_bench: the wrong flows fired")
    pin = {k: pinned(d[k].numel()) for k in ("f", "s", "w", "t", "p")}
    dt = dict(f=lvlip.LRO_FLOW_DTYPE, s=lvlip.SND_FLOW_DTYPE, w=lvlip.PUSH_FLOW_DTYPE, t=lvlip.RTO_FLOW_DTYPE,
              p=lvlip.PERSIST_FLOW_DTYPE)
    p_out = pinned(64 * nflows)

    def host():
        for k in pin:
            pin[k].copy_(d[k], non_blocking=True)
        stream.synchronize()
        h = {k: pin[k].numpy().view(dt[k]) for k in pin}
        _, xfd, xres = lvlip.persist_cpu(h["f"], None, h["s"], h["w"], h["t"], h["p"], NOW, p_out.numpy())
        d["p"].copy_(pin["p"], non_blocking=True), d["t"].copy_(pin["t"], non_blocking=True)
        out.copy_(p_out, non_blocking=True)
        fd.copy_(torch.from_numpy(xfd.view(np.uint8)), non_blocking=True)
        res.copy_(torch.from_numpy(xres.view(np.uint8)), non_blocking=True)
        stream.synchronize()

    t_dev, t_host = [], []
    for r in range(a.warmup + a.repeats):
        d["t"].copy_(d["t0"]), d["p"].copy_(d["p0"])
        x = timed(run, stream)
        d["t"].copy_(d["t0"]), d["p"].copy_(d["p0"])
        stream.synchronize()
        y = wall(host)
        if r >= a.warmup:
            t_dev.append(x), t_host.append(y)
    row = dict(nflows=nflows, fired=fired, dev=summary(t_dev), host=summary(t_host))
    row["ratio_host_over_dev"] = row["host"]["median_ms"] / row["dev"]["median_ms"]
    return row


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        raise SystemExit("persist_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream(dev)
    out = dict(device=torch.cuda.get_device_name(dev), build_id=lvlip.BUILD_ID, persist=[])
    for nflows in (1024, 65536):
        for share in (0, 1, 4):
            out["persist"].append(bench(nflows, share, a, dev, stream, rng))
            print(json.dumps(out["persist"][-1]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
