#!/usr/bin/env python3
"""The congestion window on the device, timed.

lvlip_cc_dev at 1 024 and 65 536 flows with queues of 8 and of 4 096 entries
and at one flow with a queue of 2^20 entries, a quarter of the entries marked;
and at 65 536 flows x 4 096 entries with no entry and with every entry marked,
the two ends of the descriptor traffic.

Each is set against the host alternative the earlier sections use: what the
CPU form reads (s, snd, prev, c, t, the queue's descriptors and the scoreboard)
goes to pinned memory on the stream, one synchronise, lvlip_cc_cpu, and c and t
go back.

For the two largest shapes the bytes the device form has to move (1 B per queue
entry and 16 B per marked entry, as whole 64-B sectors) are set against the
rate of liblvlip_lab's contiguous read probe over 1 GiB, measured in the same
process.

Method: warm-up rounds, then REPEATS timed rounds, device form and host
alternative alternating in one process; device events around the device call,
wall clock around the host alternative; median and range.  c and t are restored
from a pristine copy before every round, outside the timing.  Before timing,
every output byte of the device form is checked against the CPU form at the
size that is timed.

    python scripts/cc_bench.py [--warmup W] [--repeats R] [--out FILE]
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

PROBE_BYTES = 1 << 30


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
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)


def pinned(nbytes):
    return torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()


def sectors(marks: np.ndarray) -> int:
    """Bytes of whole 64-B sectors behind 1 B per entry and 16 B per marked
    entry: the scoreboard's sectors, and the descriptor sectors (four entries
    each) that hold a marked entry."""
    n = marks.size
    pad = np.zeros(-n % 4, dtype=marks.dtype)
    touched = np.concatenate([marks, pad]).reshape(-1, 4).any(axis=1)
    return 64 * ((n + 63) // 64) + 64 * int(touched.sum())


def case(nflows, queue, marked, rng):
    s = np.zeros(nflows, dtype=lvlip.SND_FLOW_DTYPE)
    s["nseg"], s["seg0"] = queue, np.arange(nflows, dtype=np.uint64) * queue
    s["snd_una"] = rng.integers(0, 1 << 32, nflows, dtype=np.uint64)
    s["snd_nxt"] = (s["snd_una"].astype(np.uint64) + np.uint64(8 * 536)) & np.uint64(0xFFFFFFFF)
    snd = np.zeros(nflows, dtype=lvlip.SND_RESULT_DTYPE)
    snd["n_new"], snd["acked"], snd["popped"] = 2, 1072, min(2, queue)
    prev = np.zeros(nflows, dtype=lvlip.RTO_RESULT_DTYPE)
    prev["fired"], prev["backoff"] = rng.integers(0, 3, nflows), 1
    c, t = lvlip.cc_init(536, nflows=nflows), lvlip.rto_flows(nflows)
    nfd = nflows * queue
    fd = np.zeros(nfd, dtype=lvlip.FRAME_DESC_DTYPE)
    fd["offset"], fd["len"] = np.arange(nfd, dtype=np.uint64) * 592, 590
    sacked = (rng.random(nfd) < marked).astype(np.uint8)
    return s, snd, prev, c, t, fd, sacked


def bench(nflows, queue, marked, a, dev, stream, rng):
    s, snd, prev, c, t, fd, sacked = case(nflows, queue, marked, rng)
    d = {k: t_of(v, dev) for k, v in dict(s=s, snd=snd, prev=prev, c0=c, t0=t, fd=fd, sacked=sacked).items()}
    d["c"], d["t"] = d["c0"].clone(), d["t0"].clone()
    res = torch.zeros(16 * nflows, dtype=torch.uint8, device=dev)
    run = lambda: lvlip.cc_dev(d["s"], d["snd"], d["prev"], d["c"], d["t"], d["fd"], d["sacked"], res, stream=stream)  # noqa: E731
    run()
    stream.synchronize()
    hc, ht = c.copy(), t.copy()
    hres = lvlip.cc_cpu(s, snd, prev, hc, ht, fd, sacked)
    for name, got, want in (("res", res, hres), ("c", d["c"], hc), ("t", d["t"], ht)):
        if got.cpu().numpy().tobytes() != want.tobytes():
            raise SystemExit(f"cc_bench: {name} differs from lvlip_cc_cpu at {nflows} x {queue}")
    p = {k: pinned(d[k].numel()) for k in ("s", "snd", "prev", "c", "t", "fd", "sacked")}

    def host():
        for k in p:
            p[k].copy_(d[k], non_blocking=True)
        stream.synchronize()
        lvlip.cc_cpu(p["s"].numpy().view(lvlip.SND_FLOW_DTYPE), p["snd"].numpy().view(lvlip.SND_RESULT_DTYPE),
                     p["prev"].numpy().view(lvlip.RTO_RESULT_DTYPE), p["c"].numpy().view(lvlip.CC_FLOW_DTYPE),
                     p["t"].numpy().view(lvlip.RTO_FLOW_DTYPE), p["fd"].numpy().view(lvlip.FRAME_DESC_DTYPE),
                     p["sacked"].numpy())
        d["c"].copy_(p["c"], non_blocking=True), d["t"].copy_(p["t"], non_blocking=True)
        stream.synchronize()

    t_dev, t_host = [], []
    for r in range(a.warmup + a.repeats):
        d["c"].copy_(d["c0"]), d["t"].copy_(d["t0"])
        x = timed(run, stream)
        d["c"].copy_(d["c0"]), d["t"].copy_(d["t0"])
        stream.synchronize()
        y = wall(host)
        if r >= a.warmup:
            t_dev.append(x), t_host.append(y)
    row = dict(nflows=nflows, queue=queue, marked=marked, entries=nflows * queue, n_sacked=int(hres["n_sacked"].sum()),
               sector_bytes=sectors(sacked), dev=summary(t_dev), host=summary(t_host))
    row["ratio_host_over_dev"] = row["host"]["median_ms"] / row["dev"]["median_ms"]
    return row


def read_probe(a, dev, stream):
    """GB/s of the lab's contiguous nontemporal read over PROBE_BYTES, median of the timed rounds."""
    lab = lvlip.lab()
    buf = torch.empty(PROBE_BYTES, dtype=torch.uint8, device=dev).fill_(1)
    sink = torch.zeros(1, dtype=torch.int32, device=dev)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def run():
        if lab.lvlip_lab_probe(buf.data_ptr(), PROBE_BYTES, sink.data_ptr(), 1, 8, 1, cus * 2, stream.cuda_stream):
            raise SystemExit("cc_bench: the read probe failed")

    ms = [timed(run, stream) for _ in range(a.warmup + a.repeats)][a.warmup:]
    out = summary(ms)
    out["bytes"], out["gb_per_s"] = PROBE_BYTES, PROBE_BYTES / out["median_ms"] / 1e6
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        raise SystemExit("cc_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream(dev)
    out = dict(device=torch.cuda.get_device_name(dev), build_id=lvlip.BUILD_ID, probe=read_probe(a, dev, stream), cc=[])
    print(json.dumps(out["probe"]), flush=True)
    shapes = ((1024, 8, .25), (1024, 4096, .25), (65536, 8, .25), (65536, 4096, .25), (1, 1 << 20, .25),
              (65536, 4096, 0.), (65536, 4096, 1.))
    for nflows, queue, marked in shapes:
        row = bench(nflows, queue, marked, a, dev, stream, rng)
        if row["entries"] >= 1 << 28:  # the largest shapes: bytes moved against the read probe
            row["gb_per_s"] = row["sector_bytes"] / row["dev"]["median_ms"] / 1e6
            row["fraction_of_probe"] = row["gb_per_s"] / out["probe"]["gb_per_s"]
        out["cc"].append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
