#!/usr/bin/env python3
"""The write queue on the device, timed.

  (a) lvlip_push_dev with SLOTS live slots of MSS-byte segments over 1 024 and
      over 65 536 flows, against lvlip_tso_dev building the same segments into
      the same slots: the push is TSO's kernel body between two small launches.
  (b) the compaction alone: push 0, every flow's queue of 8 or of 4 096 entries
      moved down by one entry.

Method: warm-up rounds, then REPEATS timed rounds with device events around
each call, the forms alternating in one process; the median and the range are
reported.  The state a push changes (s, w) is copied back from a pristine copy
before every round, outside the events.  Before timing, the device results are
checked: at a sixteenth of the size every output byte against lvlip_push_cpu,
and at full size the ring lvlip_push_dev leaves against the ring lvlip_tso_dev
leaves for sends with the same header fields (TSO itself is checked against
the CPU form by the tests).

    python scripts/push_bench.py [--slots N] [--mss M] [--warmup W] [--repeats R] [--out FILE]
"""
import argparse
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

ISS, IRS, WIN = 0xFFFFF000, 0x01020304, 29200


def template(k: int = 0, seq: int = 0, ack: int = 0, win: int = 0) -> bytes:
    eth = bytes.fromhex("0a1b2c3d4e5f000c296d5025") + b"\x08\x00"
    ip = struct.pack("!BBHHHBBH4s4s", 0x45, 0, 0, 0, 0x4000, 64, 6, 0, bytes((10, 0, 0, 4)), bytes((10, 0, 0, 5)))
    return eth + ip + struct.pack("!HHIIBBHHH", 40000 + k % 20000, 8000, seq, ack, 0x50, 0x18, win, 0, 0)


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)  # ms


def summary(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), rounds=len(ms))


def build(nflows: int, per: int, mss: int, queue: int = 0, push=None):
    """nflows flows with `per` ring slots and `per` unsent segments each (the
    last one short), a queue of `queue` entries one above q0."""
    k = np.arange(nflows, dtype=np.uint64)
    stride, cap = 54 + mss + 3, per + queue + 1
    unsent = per * mss - (mss // 3 if per else 0)
    w = np.zeros(nflows, dtype=lvlip.PUSH_FLOW_DTYPE)
    w["hdr"][:] = np.frombuffer(template(), dtype=np.uint8)
    w["pay_off"], w["ring_off"], w["q0"] = 5 + k * (unsent + 1), 3 + k * cap * stride, k * cap
    w["unsent"], w["stride"], w["cap"], w["push"], w["wnd"], w["mss"] = unsent, stride, cap, per if push is None else push, \
        lvlip.PUSH_NO_LIMIT, mss
    w["slot_nxt"] = queue % cap
    s = np.zeros(nflows, dtype=lvlip.SND_FLOW_DTYPE)
    s["snd_una"] = s["snd_nxt"] = (ISS + 7919 * k) & 0xFFFFFFFF
    s["seg0"], s["nseg"], s["win"] = w["q0"] + (1 if queue else 0), queue, WIN
    f = np.zeros(nflows, dtype=lvlip.LRO_FLOW_DTYPE)
    f["rcv_nxt"] = IRS
    nslots, ring_bytes, nfd = lvlip.push_plan(w, s)
    # the same segments as sends: header fields as the push sets them, frames into the same slots
    sends = np.zeros(nflows, dtype=lvlip.TsoSend)
    hdr = np.tile(np.frombuffer(template(0, 0, IRS, WIN), dtype=np.uint8), (nflows, 1))
    hdr[:, 38:42] = s["snd_nxt"].astype(">u4").view(np.uint8).reshape(nflows, 4)
    sends["hdr"] = hdr
    sends["payload_off"], sends["out_off"], sends["len"], sends["stride"], sends["mss"] = \
        w["pay_off"], w["ring_off"] + np.uint64(queue % cap) * np.uint64(stride), np.maximum(unsent, 1), stride, mss
    nseg = lvlip.tso_plan(sends)[0]
    return dict(f=f, s=s, w=w, sends=sends, nslots=nslots, nseg=nseg, ring_bytes=ring_bytes, nfd=nfd,
                pay_bytes=int(5 + nflows * (unsent + 1) + 64))


def to_dev(c, dev, rng):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d = dict(f=t(c["f"]), s0=t(c["s"]), w0=t(c["w"]), sends=t(c["sends"]))
    d["s"], d["w"] = d["s0"].clone(), d["w0"].clone()
    d["pay"] = torch.randint(0, 256, (c["pay_bytes"],), dtype=torch.uint8, device=dev)
    d["ring"] = torch.full((c["ring_bytes"] + 64,), 0xA5, dtype=torch.uint8, device=dev)
    fd = np.zeros(c["nfd"], dtype=lvlip.FRAME_DESC_DTYPE)
    fd["offset"], fd["len"] = np.arange(c["nfd"]), 60
    d["fd0"] = t(fd)
    d["fd"], d["sacked"] = d["fd0"].clone(), torch.zeros(c["nfd"], dtype=torch.uint8, device=dev)
    d["fd_out"] = torch.zeros(16 * max(c["nslots"], 1), dtype=torch.uint8, device=dev)
    d["res"] = torch.zeros(16 * c["f"].size, dtype=torch.uint8, device=dev)
    return d


def push(c, d, stream):
    return lvlip.push_dev(d["f"], None, d["s"], d["w"], c["nslots"], d["pay"], d["ring"], d["fd"], d["sacked"], d["fd_out"],
                          d["res"], stream=stream)


def reset(d):
    d["s"].copy_(d["s0"]), d["w"].copy_(d["w0"]), d["fd"].copy_(d["fd0"])


def check_against_cpu(c, dev, rng):
    d = to_dev(c, dev, rng)
    s = torch.cuda.current_stream(dev)
    push(c, d, s)
    s.synchronize()
    hs, hw = c["s"].copy(), c["w"].copy()
    ring = np.full(c["ring_bytes"] + 64, 0xA5, dtype=np.uint8)
    fd = d["fd0"].cpu().numpy().view(lvlip.FRAME_DESC_DTYPE).copy()
    sk = np.zeros(c["nfd"], dtype=np.uint8)
    fd_out, res = lvlip.push_cpu(c["f"], None, hs, hw, d["pay"].cpu().numpy(), ring, fd, sk)
    for name, got, want in (("ring", d["ring"], ring), ("fd", d["fd"], fd), ("sacked", d["sacked"], sk), ("s", d["s"], hs),
                            ("w", d["w"], hw), ("res", d["res"], res), ("fd_out", d["fd_out"][:16 * c["nslots"]], fd_out)):
        if got.cpu().numpy().tobytes() != np.ascontiguousarray(want).tobytes():
            raise SystemExit(f"push_bench: {name} differs from lvlip_push_cpu")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1 << 20)
    ap.add_argument("--mss", type=int, default=1460)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        raise SystemExit("push_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream(dev)
    out = dict(device=torch.cuda.get_device_name(dev), build_id=lvlip.BUILD_ID, slots=a.slots, mss=a.mss, push_vs_tso=[],
               compaction=[])

    for nflows in (1024, 65536):
        per = a.slots // nflows
        check_against_cpu(build(nflows, max(per // 16, 1), a.mss, queue=3), dev, rng)
        c = build(nflows, per, a.mss)
        d = to_dev(c, dev, rng)
        push(c, d, stream)
        stream.synchronize()
        got = d["ring"].clone()
        d["ring"].fill_(0xA5)
        lvlip.tso_dev(d["pay"], d["sends"], c["nseg"], d["ring"], None, stream=stream)
        stream.synchronize()
        if c["nseg"] != c["nslots"] or not torch.equal(got, d["ring"]):
            raise SystemExit("push_bench: lvlip_push_dev's ring is not lvlip_tso_dev's")
        del got
        t_push, t_tso = [], []
        for r in range(a.warmup + a.repeats):
            reset(d)
            p = timed(lambda: push(c, d, stream), stream)
            t = timed(lambda: lvlip.tso_dev(d["pay"], d["sends"], c["nseg"], d["ring"], None, stream=stream), stream)
            if r >= a.warmup:
                t_push.append(p), t_tso.append(t)
        row = dict(nflows=nflows, slots=c["nslots"], push=summary(t_push), tso=summary(t_tso))
        row["ratio_push_over_tso"] = row["push"]["median_ms"] / row["tso"]["median_ms"]
        out["push_vs_tso"].append(row)
        print(json.dumps(row), flush=True)
        del d
        torch.cuda.empty_cache()

    for nflows, queue in ((1024, 8), (65536, 8), (1024, 4096)):
        c = build(nflows, 0, 8, queue=queue, push=0)
        check_against_cpu(c, dev, rng)
        d = to_dev(c, dev, rng)
        ts = []
        for r in range(a.warmup + a.repeats):
            reset(d)
            t = timed(lambda: push(c, d, stream), stream)
            if r >= a.warmup:
                ts.append(t)
        row = dict(nflows=nflows, queue=queue, entries_moved=nflows * queue, **summary(ts))
        out["compaction"].append(row)
        print(json.dumps(row), flush=True)

    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
