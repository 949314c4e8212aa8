#!/usr/bin/env python3
"""The end of a connection on the device, timed.

lvlip_fin_dev at 1 024 and 65 536 flows over 1 048 576 records, one in
sixteen of them a FIN of which half stand at their flow's stream end.  A
quarter of the flows are in FIN_WAIT_1 with a timer that ran out (they re-send
their FIN), a quarter are ESTABLISHED and close now (they send it), the rest
are ESTABLISHED and only watch for the peer's FIN.

Each is set against the host alternative the earlier sections use: what the
CPU form reads (f, gin, rec, s, w, t, x, close) goes to pinned memory on the
stream, one synchronise, lvlip_fin_cpu, and f, s, x, gate, res, fd_out and the
frames go back.

Method: scripts/persist_bench.py's.  Warm-up rounds, then REPEATS timed rounds,
device form and host alternative alternating in one process; device events
around the device call, wall clock around the host alternative; median and
range.  The state the call changes is restored from a pristine copy before
every round, outside the timing.  Before timing, every output byte of the
device form is checked against the CPU form at the size that is timed.

    python scripts/fin_bench.py [--warmup W] [--repeats R] [--records N] [--out FILE]
"""
import argparse
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "level-ip_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import lvlip  # noqa: E402
from persist_bench import pinned, summary, t_of, timed, wall  # noqa: E402

NOW = 1_000_000


def case(nflows, nrec, rng):
    f = np.zeros(nflows, dtype=lvlip.LRO_FLOW_DTYPE)
    f["rcv_nxt"], f["rcv_wnd"] = rng.integers(0, 1 << 32, nflows, dtype=np.uint64), 1 << 16
    gin = np.zeros(nflows, dtype=lvlip.LRO_RESULT_DTYPE)
    gin["delivered"] = rng.integers(0, 3000, nflows)
    s = np.zeros(nflows, dtype=lvlip.SND_FLOW_DTYPE)
    s["snd_una"] = s["snd_nxt"] = rng.integers(0, 1 << 32, nflows, dtype=np.uint64)
    s["win"] = 29200
    w = np.zeros(nflows, dtype=lvlip.PUSH_FLOW_DTYPE)
    w["mss"] = 1460
    hdr = bytes(12) + b"\x08\x00" + struct.pack("!BBHHHBBH4s4s", 0x45, 0, 0, 7, 0x4000, 64, 6, 0, bytes([10, 0, 0, 4]),
                                                bytes([10, 0, 0, 5])) + \
        struct.pack("!HHIIBBHHH", 40000, 8000, 0, 0, 0x50, 0x18, 0, 0, 0)
    w["hdr"] = np.frombuffer(hdr, dtype=np.uint8)
    w["hdr"][:, 34:36] = (np.arange(nflows) & 0xFFFF).astype(">u2").view(np.uint8).reshape(nflows, 2)
    t = lvlip.rto_flows(nflows)
    x = lvlip.fin_flows(f)
    kind = np.arange(nflows) % 4
    x["state"][kind == 0] = lvlip.TCP_FIN_WAIT_1
    x["interval"], x["expires"] = 1000, NOW - 1
    x["fin_seq"] = s["snd_nxt"] - np.uint32(1)
    s["snd_una"][kind == 0] -= np.uint32(1)
    close = (kind == 1).astype(np.uint8)
    rec = np.zeros(nrec, dtype=lvlip.LRO_REC_DTYPE)
    rec["flow"] = rng.integers(0, nflows, nrec)
    rec["dlen"] = np.where(rng.random(nrec) < .5, 0, 1460)
    fin = rng.random(nrec) < 1 / 16
    at_end = rng.random(nrec) < .5
    rec["rel"] = np.where(at_end, gin["delivered"][rec["flow"]] - rec["dlen"].astype(np.uint32), rng.integers(0, 60000, nrec))
    rec["status"] = np.where(rec["dlen"] == 0, lvlip.LRO_NO_DATA, lvlip.LRO_PLACED)
    rec["tcp_flags"] = np.where(fin, 0x11, 0x10)
    rec["ack_seq"] = rng.integers(0, 1 << 32, nrec)
    return f, gin, rec, s, w, t, x, close


def bench(nflows, nrec, a, dev, stream, rng):
    f, gin, rec, s, w, t, x, close = case(nflows, nrec, rng)
    d = {k: t_of(v, dev) for k, v in dict(f0=f, gin=gin, rec=rec, s0=s, w=w, t=t, x0=x, close=close).items()}
    for k in ("f", "s", "x"):
        d[k] = d[k + "0"].clone()
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
    out, fd, res, gate = z(64 * nflows), z(16 * nflows), z(16 * nflows), z(48 * nflows)
    ws = z(lvlip.fin_workspace_bytes(nflows))

    def restore():
        for k in ("f", "s", "x"):
            d[k].copy_(d[k + "0"])

    run = lambda: lvlip.fin_dev(d["f"], d["gin"], d["rec"], d["s"], d["w"], d["t"], d["x"], d["close"], NOW, out, gate,  # noqa: E731
                                ws, fd, res, stream=stream)
    run()
    stream.synchronize()
    hf, hs, hx = f.copy(), s.copy(), x.copy()
    hout, hfd, hgate, hres = lvlip.fin_cpu(hf, gin, rec, hs, w, t, hx, close, NOW)
    for name, got, want in (("f", d["f"], hf), ("s", d["s"], hs), ("x", d["x"], hx), ("out", out, hout), ("fd_out", fd, hfd),
                            ("gate", gate, hgate), ("res", res, hres)):
        if got.cpu().numpy().tobytes() != want.tobytes():
            raise SystemExit(f"fin_bench: {name} differs from lvlip_fin_cpu")
    ev = hres["events"]
    frames = int(((ev & (lvlip.FIN_EV_SENT | lvlip.FIN_EV_RESENT)) != 0).sum())
    fins = int(((ev & lvlip.FIN_EV_PEER_FIN) != 0).sum())
    if frames != sum(1 for k in range(nflows) if k % 4 < 2) or (nrec and not fins):
        raise SystemExit("fin_bench: the wrong flows sent, or no FIN was taken")
    names = ("f", "gin", "rec", "s", "w", "t", "x", "close")
    pin = {k: pinned(d[k].numel()) for k in names}
    dt = dict(f=lvlip.LRO_FLOW_DTYPE, gin=lvlip.LRO_RESULT_DTYPE, rec=lvlip.LRO_REC_DTYPE, s=lvlip.SND_FLOW_DTYPE,
              w=lvlip.PUSH_FLOW_DTYPE, t=lvlip.RTO_FLOW_DTYPE, x=lvlip.FIN_FLOW_DTYPE, close=np.uint8)
    p_out = pinned(64 * nflows)

    def host():
        for k in names:
            pin[k][:d[k].numel()].copy_(d[k], non_blocking=True)
        stream.synchronize()
        h = {k: pin[k].numpy()[:d[k].numel()].view(dt[k]) for k in names}
        _, xfd, xgate, xres = lvlip.fin_cpu(h["f"], h["gin"], h["rec"], h["s"], h["w"], h["t"], h["x"], h["close"], NOW,
                                            p_out.numpy())
        for k in ("f", "s", "x"):
            d[k].copy_(pin[k][:d[k].numel()], non_blocking=True)
        out.copy_(p_out, non_blocking=True)
        for dst, src in ((fd, xfd), (gate, xgate), (res, xres)):
            dst.copy_(torch.from_numpy(src.view(np.uint8)), non_blocking=True)
        stream.synchronize()

    t_dev, t_host = [], []
    for r in range(a.warmup + a.repeats):
        restore()
        v = timed(run, stream)
        restore()
        stream.synchronize()
        y = wall(host)
        if r >= a.warmup:
            t_dev.append(v), t_host.append(y)
    row = dict(nflows=nflows, records=nrec, frames=frames, peer_fins=fins, dev=summary(t_dev), host=summary(t_host))
    row["ratio_host_over_dev"] = row["host"]["median_ms"] / row["dev"]["median_ms"]
    return row


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        raise SystemExit("fin_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    stream = torch.cuda.current_stream(dev)
    out = dict(device=torch.cuda.get_device_name(dev), build_id=lvlip.BUILD_ID, fin=[])
    for nflows in (1024, 65536):
        for nrec in (0, a.records):
            out["fin"].append(bench(nflows, nrec, a, dev, stream, rng))
            print(json.dumps(out["fin"][-1]), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
