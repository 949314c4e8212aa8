"""What tests/test_fin_cpu.py and tests/test_fin_gpu.py share: a plain
restatement of lvlip_fin_*'s steps 0-6 and of the FIN frame from the header's
text (include/lvlip_skb.h, "the end of a connection"), which never calls the
library, and the random states and records both files run through it."""
import struct

import numpy as np

import lvlip
import pyoracle
from persist_model import CANARY, M32, make_sides  # noqa: F401  (re-exported)
from tcp_model import lost_carry_seed

EST, FW1, FW2, CLOSED, CW, CLOSING, LAST_ACK, TW = 3, 4, 5, 6, 7, 8, 9, 10
STATES = (EST, FW1, FW2, CLOSED, CW, CLOSING, LAST_ACK, TW)
PEER_FIN, ACK_OWED, SENT, RESENT, ACKED, TW_DONE, LATE_WRITE = 1, 2, 4, 8, 16, 32, 64
EVENTS = (PEER_FIN, ACK_OWED, SENT, RESENT, ACKED, TW_DONE, LATE_WRITE)
MAX_MS = MSL2 = 60000
BRANCHES = ("dead", "closed", "acked_fw1", "acked_closing", "acked_last", "hit_est", "hit_fw1", "hit_fw2", "hit_ignored",
            "again", "again_tw", "again_ignored", "req", "send_est", "send_cw", "send_waits", "hold", "resend", "wait",
            "tw_done", "tw_wait", "late")
PLACED, NO_DATA, OOW = lvlip.LRO_PLACED, lvlip.LRO_NO_DATA, lvlip.LRO_OUT_OF_WINDOW


def model_step(x: dict, dead, rcv_nxt, una, nxt, nseg, unsent, rto, hit, again, close, now):
    """Steps 0 and 2-6 on the dict x (base, fin_seq, expires, interval, retries,
    state, flags).  Returns (x', events, frame, rcv_nxt', snd_nxt', interval of
    the result, branches)."""
    x = dict(x)
    x["base"] = rcv_nxt
    if dead or x["state"] == CLOSED:
        return x, 0, 0, rcv_nxt, nxt, 0, {"dead" if dead else "closed"}
    br, ev, frame, st = set(), 0, 0, x["state"]

    def time_wait():
        x["interval"], x["expires"] = MSL2, (now + MSL2) & M32

    if st in (FW1, CLOSING, LAST_ACK) and una == (x["fin_seq"] + 1) & M32:
        ev |= ACKED
        br.add({FW1: "acked_fw1", CLOSING: "acked_closing", LAST_ACK: "acked_last"}[st])
        if st == CLOSING:
            time_wait()
        st = {FW1: FW2, CLOSING: TW, LAST_ACK: CLOSED}[st]
    if hit:
        if st in (EST, FW1, FW2):
            rcv_nxt = (rcv_nxt + 1) & M32
            ev |= PEER_FIN | ACK_OWED
            br.add({EST: "hit_est", FW1: "hit_fw1", FW2: "hit_fw2"}[st])
            if st == FW2:
                time_wait()
            st = {EST: CW, FW1: CLOSING, FW2: TW}[st]
        else:
            br.add("hit_ignored")
    if again:
        if st in (CW, CLOSING, LAST_ACK, TW):
            ev |= ACK_OWED
            br.add("again_tw" if st == TW else "again")
            if st == TW:
                time_wait()
        else:
            br.add("again_ignored")
    x["base"] = rcv_nxt
    if close:
        x["flags"] |= 1
        br.add("req")
    if x["flags"] & 1 and st in (EST, CW) and unsent == 0:
        br.add("send_est" if st == EST else "send_cw")
        x["fin_seq"], nxt = nxt, (nxt + 1) & M32
        st = FW1 if st == EST else LAST_ACK
        x["interval"] = max(1, min(rto, MAX_MS))
        x["expires"], x["retries"] = (now + x["interval"]) & M32, 0
        ev |= SENT
        frame = 1
    elif st in (FW1, CLOSING, LAST_ACK):
        if nseg > 0:
            x["expires"] = (now + x["interval"]) & M32
            br.add("hold")
        elif x["expires"] < now:
            x["retries"] = min(x["retries"] + 1, M32)
            x["interval"] = min(2 * x["interval"], MAX_MS)
            x["expires"] = (now + x["interval"]) & M32
            ev |= RESENT
            frame = 1
            br.add("resend")
        else:
            br.add("wait")
    elif st == TW:
        if x["expires"] < now:
            st = CLOSED
            ev |= TW_DONE
            br.add("tw_done")
        else:
            br.add("tw_wait")
    elif x["flags"] & 1 and st in (EST, CW):
        br.add("send_waits")
    if st in (FW1, FW2, CLOSING, LAST_ACK, TW) and unsent > 0:
        ev |= LATE_WRITE
        br.add("late")
    x["state"] = st
    return x, ev, frame, rcv_nxt, nxt, x["interval"], br


def model_frame(hdr: bytes, fin_seq: int, ack: int, win: int, seed_fn=lost_carry_seed) -> bytes:
    """The FIN of one flow from the header's text."""
    ip = bytearray(hdr[14:34])
    ip[2:4] = struct.pack("!H", 40)
    ip[10:12] = b"\x00\x00"
    ip[10:12] = struct.pack("<H", pyoracle.checksum(bytes(ip), 20, 0))
    tcp = bytearray(hdr[34:54])
    tcp[4:8] = struct.pack("!I", fin_seq & M32)
    tcp[8:12] = struct.pack("!I", ack & M32)
    tcp[13] = (tcp[13] & (0xFF ^ 0x08)) | 0x11
    tcp[14:16] = struct.pack("!H", win)
    tcp[16:18] = b"\x00\x00"
    tcp[16:18] = struct.pack("<H", pyoracle.checksum(bytes(tcp), 20, seed_fn(hdr[26:30], hdr[30:34], 20)))
    return bytes(hdr[:14]) + bytes(ip) + bytes(tcp)


def model_scan(f, gin, rec, x):
    """Step 1: (hit, again) per flow."""
    n = f.size
    hit, again = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for r in (rec if rec is not None else ()):
        k = int(r["flow"])
        if k >= n or not int(r["tcp_flags"]) & 1 or int(r["status"]) not in (PLACED, NO_DATA):
            continue
        key = (int(r["rel"]) + int(r["dlen"])) & M32
        target = (int(f["rcv_nxt"][k]) + int(gin["delivered"][k]) - int(x["base"][k])) & M32
        hit[k] |= key == target
        again[k] |= key == (target - 1) & M32
    return hit, again


def model_run(f, gin, rec, s, w, t, x, close, now: int, out: np.ndarray):
    """The whole call on copies: (f', s', x', out', fd_out, gate, res, branches)."""
    n = s.size
    f, s, x, out = f.copy(), s.copy(), x.copy(), out.copy()
    fd = np.zeros(n, dtype=lvlip.FRAME_DESC_DTYPE)
    res = np.zeros(n, dtype=lvlip.FIN_RESULT_DTYPE)
    gate = gin.copy()
    hit, again = model_scan(f, gin, rec, x)
    branches = []
    for k in range(n):
        xk = {name: int(x[name][k]) for name in ("base", "fin_seq", "expires", "interval", "retries", "state", "flags")}
        q, ev, frame, rn, sn, iv, br = model_step(
            xk, int(t["dead"][k]), int(f["rcv_nxt"][k]), int(s["snd_una"][k]), int(s["snd_nxt"][k]), int(s["nseg"][k]),
            int(w["unsent"][k]), int(t["rto"][k]), bool(hit[k]), bool(again[k]),
            0 if close is None else int(close[k]), now & M32)
        branches.append(br)
        for name, v in q.items():
            x[name][k] = v
        f["rcv_nxt"][k], s["snd_nxt"][k] = rn, sn
        if ev & ACK_OWED and gin["placed"][k] == 0:
            gate["placed"][k] = 1
        res[k] = (ev, q["state"], q["fin_seq"] if frame else 0, iv)
        fd[k] = (64 * k, 54 if frame else 0, 0)
        if frame:
            fr = model_frame(w["hdr"][k].tobytes(), q["fin_seq"], rn + int(gin["delivered"][k]), int(s["win"][k]))
            out[64 * k:64 * k + 54] = np.frombuffer(fr, dtype=np.uint8)
    return f, s, x, out, fd, gate, res, branches


def random_case(n: int, seed: int, nrec: int = None, with_close: bool = True):
    """States and records that mix every branch: (f, gin, rec, s, w, t, x,
    close, now).  The receive side is as lvlip_lro_next_* left it for some
    flows (delivered 0, base behind rcv_nxt) and as it stood before for
    others."""
    rng = np.random.default_rng(seed)
    f, s, w, _ = make_sides(n)
    now = int(rng.choice([1_000_000, 5, M32 - 3]))
    f["rcv_nxt"][rng.random(n) < .1] = M32  # the FIN's rcv_nxt + 1 wraps
    gin = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
    gin["delivered"] = np.where(rng.random(n) < .5, 0, rng.integers(0, 5000, n))
    gin["placed"] = np.where(rng.random(n) < .6, 0, rng.integers(1, 9, n))
    gin["nsack"] = rng.integers(0, 5, n)
    gin["reserved"] = 0
    gin["sack"] = rng.integers(0, 1 << 32, (n, 4, 2))
    x = lvlip.fin_flows(f)
    x["base"] = f["rcv_nxt"] - np.where(rng.random(n) < .5, 0, rng.integers(0, 3000, n)).astype(np.uint32)
    x["state"] = rng.choice(STATES, n)
    x["flags"] = rng.random(n) < .35
    x["interval"] = rng.choice([0, 1, 200, 1000, 30000, 30001, 59999, 60000], n)
    x["retries"] = rng.choice([0, 1, 7, M32 - 1, M32], n)
    x["expires"] = (now + rng.integers(-3, 4, n)) & M32
    s["snd_nxt"][rng.random(n) < .1] = M32  # our FIN's snd_nxt + 1 wraps
    x["fin_seq"] = s["snd_nxt"] - 1
    sent = np.isin(x["state"], (FW1, FW2, CLOSING, LAST_ACK, TW))
    acked = rng.random(n) < .5
    s["nseg"] = np.where(rng.random(n) < .25, rng.integers(1, 4, n), 0)
    back = np.where(sent & acked, 0, np.where(s["nseg"] > 0, 1 + 536 * s["nseg"], sent.astype(np.int64)))
    s["snd_una"] = s["snd_nxt"] - back.astype(np.uint32)
    w["unsent"] = np.where(rng.random(n) < .25, rng.integers(1, 3000, n), 0)
    t = lvlip.rto_flows(n)
    t["dead"] = rng.random(n) < .08
    t["rto"] = rng.choice([0, 1, 200, 1000, 59999, 60000, 60001, M32], n)
    close = (rng.random(n) < .3).astype(np.uint8) * rng.choice([1, 2, 255], n).astype(np.uint8) if with_close else None
    # the round's records: FINs at, one before and around the stream's end, bare and with data, among others
    nrec = 3 * n if nrec is None else nrec
    rec = np.zeros(nrec, dtype=lvlip.LRO_REC_DTYPE)
    rec["flow"] = rng.integers(0, n, nrec)
    odd = rng.random(nrec) < .05
    rec["flow"][odd] = rng.choice([n, n + 7, M32], int(odd.sum()))
    k = np.minimum(rec["flow"], n - 1)
    target = f["rcv_nxt"][k] + gin["delivered"][k] - x["base"][k]
    rec["dlen"] = np.where(rng.random(nrec) < .5, 0, rng.integers(1, 1461, nrec))
    key = target + rng.choice([0, 0, M32, 1, 5, M32 - 1], nrec).astype(np.uint32)
    rec["rel"] = key - rec["dlen"]
    rec["status"] = np.where(rec["dlen"] == 0, NO_DATA, PLACED)
    other = rng.random(nrec) < .15
    rec["status"][other] = rng.choice([OOW, lvlip.LRO_CONTROL, lvlip.LRO_NO_FLOW, 2], int(other.sum()))
    rec["tcp_flags"] = np.where(rng.random(nrec) < .45, 0x11, rng.choice([0x10, 0x18, 0x19, 0x01], nrec))
    rec["ack_seq"] = rng.integers(0, 1 << 32, nrec)
    return f, gin, rec, s, w, t, x, close, now
