"""What tests/test_persist_cpu.py and tests/test_persist_gpu.py share: a plain
restatement of lvlip_persist_*'s steps 0-4 and of the probe frame from the
header's text (include/lvlip_skb.h, "the persist timer"), which never calls
the library, and the random states both files run through it."""
import struct

import numpy as np

import lvlip
import pyoracle
from tcp_model import lost_carry_seed

M32 = 0xFFFFFFFF
CANARY = 0x5A
MAX_MS = 60000
ETH = bytes.fromhex("0a1b2c3d4e5f000c296d5025") + b"\x08\x00"
BRANCHES = ("dead", "open", "open_armed", "arm", "wait", "fire")


def template(saddr: bytes, daddr: bytes, sport: int, dport: int, flags: int = 0x18, ident: int = 0x1234) -> bytes:
    """A 54-byte header template: seq, ack_seq, window and both checksums hold
    bytes the calls must replace."""
    ip = struct.pack("!BBHHHBBH4s4s", 0x45, 0, 0xEEEE, ident, 0x4000, 64, 6, 0xEEEE, saddr, daddr)
    tcp = struct.pack("!HHIIBBHHH", sport, dport, 0xEEEEEEEE, 0xEEEEEEEE, 0x50, flags, 0xEEEE, 0xEEEE, 0)
    return ETH + ip + tcp


def model_step(p: dict, dead: int, nseg: int, unsent: int, wnd: int, mss: int, rto: int, now: int):
    """Steps 0-4 on the dict p (expires, interval, probes, armed, reserved).
    Returns (p', fired, (interval, probes) of the result, clear, branch)."""
    if dead:
        return p, 0, (0, 0), 0, "dead"
    stalled = nseg == 0 and unsent > 0 and wnd < min(unsent, mss)
    if not stalled:
        if p["armed"]:
            return dict(expires=0, interval=0, probes=0, armed=0, reserved=(0, 0, 0)), 0, (0, 0), 1, "open_armed"
        return p, 0, (0, 0), 0, "open"
    q = dict(p)
    if not p["armed"]:
        q["armed"], q["probes"] = 1, 0
        q["interval"] = max(1, min(rto, MAX_MS))
        q["expires"] = (now + q["interval"]) & M32
        return q, 0, (q["interval"], 0), 0, "arm"
    if p["expires"] < now:
        q["probes"] = min(p["probes"] + 1, M32)
        q["interval"] = min(2 * p["interval"], MAX_MS)
        q["expires"] = (now + q["interval"]) & M32
        return q, 1, (q["interval"], q["probes"]), 0, "fire"
    return q, 0, (p["interval"], p["probes"]), 0, "wait"


def model_probe(hdr: bytes, snd_una: int, ack: int, win: int, seed_fn=lost_carry_seed) -> bytes:
    """The probe of one flow from the header's text."""
    ip = bytearray(hdr[14:34])
    ip[2:4] = struct.pack("!H", 40)
    ip[10:12] = b"\x00\x00"
    ip[10:12] = struct.pack("<H", pyoracle.checksum(bytes(ip), 20, 0))
    tcp = bytearray(hdr[34:54])
    tcp[4:8] = struct.pack("!I", (snd_una - 1) & M32)
    tcp[8:12] = struct.pack("!I", ack & M32)
    tcp[13] &= 0xFF ^ 0x09
    tcp[14:16] = struct.pack("!H", win)
    tcp[16:18] = b"\x00\x00"
    tcp[16:18] = struct.pack("<H", pyoracle.checksum(bytes(tcp), 20, seed_fn(hdr[26:30], hdr[30:34], 20)))
    return bytes(hdr[:14]) + bytes(ip) + bytes(tcp)


def model_run(f, lro, s, w, t, p, now: int, out: np.ndarray):
    """The whole call on copies: (t', p', out', fd_out, res, branches)."""
    n = s.size
    t, p, out = t.copy(), p.copy(), out.copy()
    fd = np.zeros(n, dtype=lvlip.FRAME_DESC_DTYPE)
    res = np.zeros(n, dtype=lvlip.PERSIST_RESULT_DTYPE)
    branches = []
    for k in range(n):
        pk = dict(expires=int(p["expires"][k]), interval=int(p["interval"][k]), probes=int(p["probes"][k]),
                  armed=int(p["armed"][k]), reserved=tuple(int(x) for x in p["reserved"][k]))
        q, fired, (iv, pr), clear, br = model_step(pk, int(t["dead"][k]), int(s["nseg"][k]), int(w["unsent"][k]),
                                                   int(w["wnd"][k]), int(w["mss"][k]), int(t["rto"][k]), now & M32)
        branches.append(br)
        p[k] = (q["expires"], q["interval"], q["probes"], q["armed"], q["reserved"])
        if clear:
            t["dupacks"][k] = 0
        una = int(s["snd_una"][k])
        res[k] = (fired, iv, pr, (una - 1) & M32 if fired else 0)
        fd[k] = (64 * k, 54 if fired else 0, 0)
        if fired:
            ack = int(f["rcv_nxt"][k]) + (int(lro["delivered"][k]) if lro is not None else 0)
            fr = model_probe(w["hdr"][k].tobytes(), una, ack, int(s["win"][k]))
            out[64 * k:64 * k + 54] = np.frombuffer(fr, dtype=np.uint8)
    return t, p, out, fd, res, branches


def make_sides(n: int, saddr: bytes = bytes([10, 0, 0, 4]), daddr: bytes = bytes([10, 0, 0, 5]), flags: int = 0x18):
    """n flows' reverse-plan receive sides f, send sides s and write sides w
    (all of one address pair, distinct by source port, in plan order), and the
    peer's plan of the same connections, which receives the probes."""
    rng = np.random.default_rng(n)
    f = np.concatenate([lvlip.lro_flow(daddr, saddr, 80, 1000 + k, int(rng.integers(0, 1 << 32)), 1 << 16, k << 16)
                        for k in range(n)])
    s = np.zeros(n, dtype=lvlip.SND_FLOW_DTYPE)
    s["snd_una"] = rng.integers(0, 1 << 32, n)
    s["snd_nxt"] = s["snd_una"]
    s["win"] = rng.integers(0, 1 << 16, n)
    w = np.concatenate([lvlip.push_flow(template(saddr, daddr, 1000 + k, 80, flags, ident=k & 0xFFFF), 0, 0, 536,
                                        k * 4 * 590, 4, k * 4, 4) for k in range(n)])
    peer = np.concatenate([lvlip.lro_flow(saddr, daddr, 1000 + k, 80, int(s["snd_una"][k]), 1 << 16, k << 16)
                           for k in range(n)])
    lvlip.lro_plan(f), lvlip.lro_plan(peer)  # both are in plan order already
    return f, s, w, peer


def random_case(n: int, seed: int, mix=(.1, .25, .2)):
    """States that mix the five branches: (f, lro, s, w, t, p, now).  mix =
    the shares of dead, open and unarmed flows."""
    rng = np.random.default_rng(seed)
    f, s, w, _ = make_sides(n)
    lro = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
    lro["delivered"] = rng.integers(0, 5000, n)
    now = int(rng.choice([1_000_000, 5, M32 - 3]))
    mss = rng.choice([1, 2, 536, 1460, 65495], n)
    w["mss"] = mss
    w["stride"] = 54 + mss
    unsent = np.where(rng.random(n) < .5, rng.integers(1, 3 * mss + 1), rng.integers(0, mss + 1))
    w["unsent"] = unsent
    first = np.minimum(unsent, mss)
    pick = rng.integers(0, 6, n)
    wnd = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4],
                    [0, np.minimum(1, mss - 1), mss - 1, mss, np.maximum(first, 1) - 1], 1 << 30)
    w["wnd"] = wnd
    s["nseg"] = rng.random(n) < .2
    open_ = rng.random(n) < mix[1]
    w["wnd"][open_] = 1 << 30
    t = lvlip.rto_flows(n)
    t["dead"] = rng.random(n) < mix[0]
    t["rto"] = rng.choice([0, 1, 200, 1000, 59999, 60000, 60001, 120000, M32], n)
    t["dupacks"] = rng.integers(0, 6, n)
    t["expires"], t["armed"] = rng.integers(0, 1 << 32, n), rng.random(n) < .5
    p = lvlip.persist_flows(n)
    armed = rng.random(n) > mix[2]
    p["armed"] = armed
    p["interval"] = np.where(armed, rng.choice([1, 200, 1000, 30000, 30001, 59999, 60000], n), 0)
    p["probes"] = np.where(armed, rng.choice([0, 1, 7, M32 - 1, M32], n), 0)
    p["expires"] = np.where(armed, (now + rng.integers(-3, 4, n)) & M32, 0)
    return f, lro, s, w, t, p, now
