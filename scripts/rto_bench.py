#!/usr/bin/env python3
"""The timer and the peer's window on the device, timed.

  (a) lvlip_wnd_dev over N ACK records (54-byte frames) at 1 024 flows, at
      65 536 flows and with every record of one flow.
  (b) lvlip_rto_dev at 1 024 and 65 536 flows with queues of 8 and of 4 096
      entries, every flow timing out (so every queue's scoreboard range is
      cleared).

Each is set against the host alternative the earlier sections use: what the
CPU form reads goes to pinned memory on the stream, one synchronise, the _cpu
call, and the state it changed goes back (t and w for the window; t, the gate
and the scoreboard for the timer).

Method: warm-up rounds, then REPEATS timed rounds, device form and host
alternative alternating in one process; device events around the device call,
wall clock around the host alternative; median and range.  The state a call
changes is restored from a pristine copy before every round, outside the
timing.  Before timing, every output byte of the device form is checked
against the CPU form at the size that is timed.

    python scripts/rto_bench.py [--records N] [--warmup W] [--repeats R] [--out FILE]
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


def wnd_case(n, nflows, one_flow, rng):
    f = np.zeros(nflows, dtype=lvlip.LRO_FLOW_DTYPE)
    f["rcv_wnd"] = 1
    s = np.zeros(nflows, dtype=lvlip.SND_FLOW_DTYPE)
    s["snd_una"] = rng.integers(0, 1 << 32, nflows, dtype=np.uint64)
    s["snd_nxt"] = (s["snd_una"].astype(np.uint64) + np.uint64(1 << 20)) & np.uint64(0xFFFFFFFF)
    t = lvlip.rto_flows(nflows, wscale=7, wnd_cap=1 << 22)
    w = np.zeros(nflows, dtype=lvlip.PUSH_FLOW_DTYPE)
    rec = np.zeros(n, dtype=lvlip.LRO_REC_DTYPE)
    rec["flow"] = 0 if one_flow else rng.integers(0, nflows, n)
    rec["status"], rec["tcp_flags"] = 20, 0x10
    d = rng.integers(0, (1 << 20) + 1, n).astype(np.uint64)
    rec["ack_seq"] = (s["snd_una"][rec["flow"]].astype(np.uint64) + d) & np.uint64(0xFFFFFFFF)
    hdr = bytes(12) + b"\x08\x00" + struct.pack("!BBHHHBBH4s4s", 0x45, 0, 40, 0, 0x4000, 64, 6, 0, bytes(4), bytes(4)) + \
        struct.pack("!HHIIBBHHH", 8000, 40000, 0, 0, 0x50, 0x10, 0, 0, 0)
    frames = np.tile(np.frombuffer(hdr, dtype=np.uint8), (n, 1))
    frames[:, 48:50] = rng.integers(0, 65536, n).astype(">u2").view(np.uint8).reshape(n, 2)
    buf = np.concatenate([np.zeros(1, dtype=np.uint8), frames.reshape(-1), np.zeros(16, dtype=np.uint8)])  # odd addresses
    fd = np.zeros(n, dtype=lvlip.FRAME_DESC_DTYPE)
    fd["offset"], fd["len"] = 1 + 54 * np.arange(n, dtype=np.uint64), 54
    return f, s, t, w, rec, buf, fd


def bench_wnd(n, nflows, one_flow, a, dev, stream, rng):
    f, s, t, w, rec, buf, fd = wnd_case(n, nflows, one_flow, rng)
    d = {k: t_of(v, dev) for k, v in dict(f=f, s=s, t0=t, w0=w, rec=rec, buf=buf, fd=fd).items()}
    d["t"], d["w"], res = d["t0"].clone(), d["w0"].clone(), torch.zeros(16 * nflows, dtype=torch.uint8, device=dev)
    run = lambda: lvlip.wnd_dev(d["f"], d["s"], d["t"], d["w"], d["rec"], d["buf"], d["fd"], lvlip.WND_APPLY, res,  # noqa: E731
                                stream=stream)
    run()
    stream.synchronize()
    ht, hw = t.copy(), w.copy()
    hres = lvlip.wnd_cpu(f, s, ht, hw, rec, buf, fd, lvlip.WND_APPLY)
    for name, got, want in (("res", res, hres), ("t", d["t"], ht), ("w", d["w"], hw)):
        if got.cpu().numpy().tobytes() != want.tobytes():
            raise SystemExit(f"rto_bench: wnd {name} differs from lvlip_wnd_cpu")
    p_rec, p_buf, p_fd = pinned(rec.nbytes), pinned(buf.nbytes), pinned(fd.nbytes)

    def host():
        p_rec.copy_(d["rec"], non_blocking=True), p_buf.copy_(d["buf"], non_blocking=True)
        p_fd.copy_(d["fd"], non_blocking=True)
        stream.synchronize()
        xt, xw = t.copy(), w.copy()
        lvlip.wnd_cpu(f, s, xt, xw, p_rec.numpy().view(lvlip.LRO_REC_DTYPE), p_buf.numpy(),
                      p_fd.numpy().view(lvlip.FRAME_DESC_DTYPE), lvlip.WND_APPLY)
        d["t"].copy_(torch.from_numpy(xt.view(np.uint8)), non_blocking=True)
        d["w"].copy_(torch.from_numpy(xw.view(np.uint8).reshape(-1)), non_blocking=True)
        stream.synchronize()

    t_dev, t_host = [], []
    for r in range(a.warmup + a.repeats):
        d["t"].copy_(d["t0"]), d["w"].copy_(d["w0"])
        x = timed(run, stream)
        d["t"].copy_(d["t0"]), d["w"].copy_(d["w0"])
        stream.synchronize()
        y = wall(host)
        if r >= a.warmup:
            t_dev.append(x), t_host.append(y)
    row = dict(records=n, nflows=nflows, one_flow=one_flow, dev=summary(t_dev), host=summary(t_host))
    row["ratio_host_over_dev"] = row["host"]["median_ms"] / row["dev"]["median_ms"]
    return row


def bench_rto(nflows, queue, a, dev, stream):
    s = np.zeros(nflows, dtype=lvlip.SND_FLOW_DTYPE)
    s["nseg"], s["seg0"] = queue, 1 + np.arange(nflows, dtype=np.uint64) * (queue + 1)
    t = lvlip.rto_flows(nflows)
    t["armed"], t["expires"] = 1, 500
    sres = np.zeros(nflows, dtype=lvlip.SND_RESULT_DTYPE)
    pres = np.zeros(nflows, dtype=lvlip.PUSH_RESULT_DTYPE)
    nfd = 1 + nflows * (queue + 1)
    d = {k: t_of(v, dev) for k, v in dict(s=s, sres=sres, pres=pres, t0=t).items()}
    d["t"] = d["t0"].clone()
    sacked = torch.ones(nfd, dtype=torch.uint8, device=dev)
    gate, res = torch.zeros(32 * nflows, dtype=torch.uint8, device=dev), torch.zeros(16 * nflows, dtype=torch.uint8, device=dev)
    run = lambda: lvlip.rto_dev(d["s"], d["sres"], d["pres"], d["t"], 501, 0, sacked, gate, res, stream=stream)  # noqa: E731
    run()
    stream.synchronize()
    ht, hk = t.copy(), np.ones(nfd, dtype=np.uint8)
    hgate, hres = lvlip.rto_cpu(s, sres, pres, ht, 501, 0, hk)
    for name, got, want in (("t", d["t"], ht), ("gate", gate, hgate), ("res", res, hres), ("sacked", sacked, hk)):
        if got.cpu().numpy().tobytes() != want.tobytes():
            raise SystemExit(f"rto_bench: rto {name} differs from lvlip_rto_cpu")
    if not (hres["fired"] == 1).all():
        raise SystemExit("rto_bench: not every flow timed out")
    p = {k: pinned(d[k].numel()) for k in ("s", "sres", "pres", "t")}
    p_k = pinned(nfd)

    def host():
        for k in p:
            p[k].copy_(d[k], non_blocking=True)
        p_k.copy_(sacked, non_blocking=True)
        stream.synchronize()
        g, _ = lvlip.rto_cpu(p["s"].numpy().view(lvlip.SND_FLOW_DTYPE), p["sres"].numpy().view(lvlip.SND_RESULT_DTYPE),
                             p["pres"].numpy().view(lvlip.PUSH_RESULT_DTYPE), p["t"].numpy().view(lvlip.RTO_FLOW_DTYPE),
                             501, 0, p_k.numpy())
        d["t"].copy_(p["t"], non_blocking=True), sacked.copy_(p_k, non_blocking=True)
        gate.copy_(torch.from_numpy(g.view(np.uint8)), non_blocking=True)
        stream.synchronize()

    t_dev, t_host = [], []
    for r in range(a.warmup + a.repeats):
        d["t"].copy_(d["t0"]), sacked.fill_(1)
        x = timed(run, stream)
        d["t"].copy_(d["t0"]), sacked.fill_(1)
        stream.synchronize()
        y = wall(host)
        if r >= a.warmup:
            t_dev.append(x), t_host.append(y)
    row = dict(nflows=nflows, queue=queue, bytes_cleared=nflows * queue, dev=summary(t_dev), host=summary(t_host))
    row["ratio_host_over_dev"] = row["host"]["median_ms"] / row["dev"]["median_ms"]
    return row


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        raise SystemExit("rto_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream(dev)
    out = dict(device=torch.cuda.get_device_name(dev), build_id=lvlip.BUILD_ID, records=a.records, wnd=[], rto=[])
    for nflows, one in ((1024, False), (65536, False), (1024, True)):
        out["wnd"].append(bench_wnd(a.records, nflows, one, a, dev, stream, rng))
        print(json.dumps(out["wnd"][-1]), flush=True)
        torch.cuda.empty_cache()
    for nflows in (1024, 65536):
        for queue in (8, 4096):
            out["rto"].append(bench_rto(nflows, queue, a, dev, stream))
            print(json.dumps(out["rto"][-1]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
