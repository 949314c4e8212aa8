"""The end of a connection on the calling thread (fin_cpu.c, include/lvlip_skb.h
"the end of a connection"): lvlip_fin_cpu against a plain restatement of its
steps and of the FIN frame (tests/fin_model.py, which never calls the
library); the FIN, the ACK of the peer's FIN and the states against what the
reference's own stack sent and passed through (tests/golden/fin_ref.json); the
refusals; gate against gin; the wraps of rcv_nxt, snd_nxt and the clock; and
the loop of tests/test_rto_cpu.py with both sides closing, a lost FIN on every
second flow and a lost ACK of a FIN: all 16 endpoints reach CLOSED with the
call and none leaves ESTABLISHED without it."""
import functools
import json
import os
import struct

import numpy as np
import pytest

import lvlip
from fin_model import (ACK_OWED, ACKED, BRANCHES, CANARY, CLOSED, CLOSING, CW, EST, EVENTS, FW1, FW2, LAST_ACK,
                       LATE_WRITE, M32, PEER_FIN, RESENT, SENT, STATES, TW, TW_DONE, make_sides, model_frame,
                       model_run, random_case)
from test_rto_cpu import TICK, RtoLoop  # imported, never edited

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, R, FD, G = lvlip.FIN_FLOW_DTYPE, lvlip.FIN_RESULT_DTYPE, lvlip.FRAME_DESC_DTYPE, lvlip.LRO_RESULT_DTYPE
NAMES = ("f", "s", "x", "out", "fd_out", "gate", "res")


def test_layout_and_symbols():
    assert X.itemsize == 32 and [X.fields[k][1] for k in ("base", "fin_seq", "expires", "interval", "retries", "state",
                                                          "flags", "reserved")] == [0, 4, 8, 12, 16, 20, 21, 22]
    assert R.itemsize == 16 and [R.fields[k][1] for k in ("events", "state", "seq", "interval")] == [0, 4, 8, 12]
    assert (lvlip.TCP_ESTABLISHED, lvlip.TCP_FIN_WAIT_1, lvlip.TCP_FIN_WAIT_2, lvlip.TCP_CLOSED, lvlip.TCP_CLOSE_WAIT,
            lvlip.TCP_CLOSING, lvlip.TCP_LAST_ACK, lvlip.TCP_TIME_WAIT) == STATES
    assert (lvlip.FIN_EV_PEER_FIN, lvlip.FIN_EV_ACK_OWED, lvlip.FIN_EV_SENT, lvlip.FIN_EV_RESENT, lvlip.FIN_EV_ACKED,
            lvlip.FIN_EV_TW_DONE, lvlip.FIN_EV_LATE_WRITE) == EVENTS
    for name in ("lvlip_fin_check", "lvlip_fin_cpu", "lvlip_fin_workspace_bytes", "lvlip_fin_dev"):
        assert hasattr(lvlip.lib(), name)
    src = open(os.path.join(ROOT, "level-ip_amd", "BUILD_SOURCES")).read()
    assert "csrc/fin_cpu.c" in src and "csrc/fin_kernels.hip" in src
    assert len(lvlip.SIGNATURES["lvlip_fin_cpu"][1]) == 15 and len(lvlip.SIGNATURES["lvlip_fin_dev"][1]) == 17
    hdr = open(os.path.join(ROOT, "include", "lvlip_skb.h")).read()
    for name, v in (("ESTABLISHED", 3), ("FIN_WAIT_1", 4), ("FIN_WAIT_2", 5), ("CLOSED", 6), ("CLOSE_WAIT", 7),
                    ("CLOSING", 8), ("LAST_ACK", 9), ("TIME_WAIT", 10)):
        assert f"#define LVLIP_TCP_{name}" in hdr and getattr(lvlip, "TCP_" + name) == v
    assert [lvlip.fin_workspace_bytes(n) for n in (0, 1, 8, 9, 65536)] == [16, 16, 16, 32, 131072]


def run_cpu(f, gin, rec, s, w, t, x, close, now, out=None):
    """The call on copies, from a buffer of canary bytes: (f', s', x', out, fd_out, gate, res)."""
    f, s, x = f.copy(), s.copy(), x.copy()
    out = np.full(64 * s.size + 7, CANARY, dtype=np.uint8) if out is None else out.copy()
    out, fd, gate, res = lvlip.fin_cpu(f, gin, rec, s, w, t, x, close, now, out)
    return f, s, x, out, fd, gate, res


# ------------------------------------------------------------ against the model --

def test_cpu_equals_the_model_on_every_state_event_and_branch():
    seen, events, before, after = set(), 0, set(), set()
    for seed in range(16):
        case = random_case(97, seed, with_close=seed != 3)
        out0 = np.full(64 * 97 + 7, CANARY, dtype=np.uint8)
        want = model_run(*case, out0)
        got = run_cpu(*case, out0)
        for name, a, b in zip(NAMES, got, want):
            assert a.tobytes() == b.tobytes(), (seed, name)
        for br in want[7]:
            seen |= br
        events |= int(np.bitwise_or.reduce(want[6]["events"]))
        before |= set(case[6]["state"].tolist())
        after |= set(want[2]["state"].tolist())
    assert seen == set(BRANCHES), set(BRANCHES) ^ seen
    assert events == sum(EVENTS) and before == set(STATES) == after


def test_records_without_a_fin_and_no_records_change_nothing_of_the_receive_side():
    f, gin, rec, s, w, t, x, close, now = random_case(33, 5)
    rec["tcp_flags"] &= 0xFE
    for r in (rec, rec[:0], None):
        got = run_cpu(f, gin, r, s, w, t, x, close, now)
        assert got[0]["rcv_nxt"].tobytes() == f["rcv_nxt"].tobytes()
        assert not (got[6]["events"] & (PEER_FIN | ACK_OWED)).any() and got[5].tobytes() == gin.tobytes()
        assert (got[2]["base"] == f["rcv_nxt"]).all()


def one(state=EST, flags=0, close=0, hit=False, again=False, now=1000, una=None, nxt=5000, fin_seq=None, nseg=0,
        unsent=0, rto=1000, expires=0, interval=0, retries=0, rcv_nxt=None, dead=0, delivered=0, placed=0):
    """One flow through the call; returns (f', s', x', out, fd, gate, res)."""
    f, s, w, _ = make_sides(1)
    if rcv_nxt is not None:
        f["rcv_nxt"] = rcv_nxt
    s["snd_nxt"], s["snd_una"], s["nseg"] = nxt, nxt if una is None else una, nseg
    w["unsent"] = unsent
    t = lvlip.rto_flows(1, rto=rto)
    t["dead"] = dead
    x = lvlip.fin_flows(f)
    x["state"], x["flags"], x["expires"], x["interval"], x["retries"] = state, flags, expires, interval, retries
    x["fin_seq"] = (nxt - 1) & M32 if fin_seq is None else fin_seq
    gin = np.zeros(1, dtype=G)
    gin["delivered"], gin["placed"] = delivered, placed
    rec = np.zeros(2, dtype=lvlip.LRO_REC_DTYPE)
    rec["flow"], rec["status"], rec["tcp_flags"] = (0, M32), lvlip.LRO_NO_DATA, 0x11
    rec["rel"][0] = (delivered if hit else delivered - 1 if again else delivered + 9) & M32
    return run_cpu(f, gin, rec, s, w, t, x, np.array([close], dtype=np.uint8), now)


def test_every_transition_of_rfc_793():
    """RFC 793 figure 6 from ESTABLISHED down, and the one call that takes
    FIN_WAIT_1 to TIME_WAIT (src/tcp_input.c:441-449)."""
    table = (
        (dict(state=EST, close=1), FW1, SENT),
        (dict(state=EST, hit=True), CW, PEER_FIN | ACK_OWED),
        (dict(state=EST, hit=True, close=1), LAST_ACK, PEER_FIN | ACK_OWED | SENT),
        (dict(state=CW, close=1), LAST_ACK, SENT),
        (dict(state=CW, flags=1), LAST_ACK, SENT),
        (dict(state=FW1, expires=5000), FW2, ACKED),
        (dict(state=FW1, una=4999, expires=5000, hit=True), CLOSING, PEER_FIN | ACK_OWED),
        (dict(state=FW1, expires=5000, hit=True), TW, ACKED | PEER_FIN | ACK_OWED),
        (dict(state=FW2, hit=True), TW, PEER_FIN | ACK_OWED),
        (dict(state=CLOSING, expires=5000), TW, ACKED),
        (dict(state=CLOSING, una=4999, expires=5000, again=True), CLOSING, ACK_OWED),
        (dict(state=LAST_ACK, expires=5000), CLOSED, ACKED),
        (dict(state=LAST_ACK, una=4999, expires=5000, again=True), LAST_ACK, ACK_OWED),
        (dict(state=TW, expires=5000, again=True), TW, ACK_OWED),
        (dict(state=TW, expires=999), CLOSED, TW_DONE),
        (dict(state=TW, expires=1000), TW, 0),
        (dict(state=CW, again=True), CW, ACK_OWED),
        (dict(state=CW, hit=True), CW, 0),
        (dict(state=EST, again=True), EST, 0),
        (dict(state=FW2, again=True), FW2, 0),
        (dict(state=EST, close=1, unsent=1), EST, 0),
        (dict(state=FW2, unsent=1), FW2, LATE_WRITE),
        (dict(state=CLOSED, hit=True, close=1), CLOSED, 0),
        (dict(state=EST, hit=True, close=1, dead=1), EST, 0),
    )
    for kw, state, events in table:
        f, s, x, out, fd, gate, res = one(**kw)
        assert (int(x["state"][0]), int(res["events"][0]), int(res["state"][0])) == (state, events, state), kw
        assert int(fd["len"][0]) == (54 if events & (SENT | RESENT) else 0)
        assert int(gate["placed"][0]) == (1 if events & ACK_OWED else 0)
        if state == TW and kw["state"] != TW or kw.get("again") and state == TW:
            assert (int(x["interval"][0]), int(x["expires"][0])) == (60000, 61000), "TCP_2MSL from now"


def test_the_fin_timer_doubles_holds_and_saturates():
    f, s, x, out, fd, gate, res = one(close=1, rto=700, now=100)
    assert (int(x["interval"][0]), int(x["expires"][0]), int(x["retries"][0]), int(res["seq"][0])) == (700, 800, 0, 5000)
    assert int(s["snd_nxt"][0]) == 5001 and int(x["fin_seq"][0]) == 5000 and x["flags"][0] == 1
    seen = []
    for i in range(9):
        kw = dict(state=FW1, flags=1, nxt=5001, una=5000, fin_seq=5000, interval=int(x["interval"][0]), retries=i)
        now = int(x["expires"][0])
        assert one(expires=now, now=now, **kw)[6]["events"][0] == 0, "the test is strict"
        held = one(expires=now, now=now + 1, nseg=2, **dict(kw, una=3000))
        assert held[6]["events"][0] == 0 and int(held[2]["expires"][0]) == now + 1 + kw["interval"], "data in flight"
        f, s, x, out, fd, gate, res = one(expires=now, now=now + 1, **kw)
        assert res["events"][0] == RESENT and fd["len"][0] == 54 and x["retries"][0] == i + 1 and res["seq"][0] == 5000
        assert int(x["expires"][0]) == now + 1 + int(x["interval"][0]) and int(s["snd_nxt"][0]) == 5001
        seen.append(int(res["interval"][0]))
    assert seen == [1400, 2800, 5600, 11200, 22400, 44800, 60000, 60000, 60000]
    assert one(state=LAST_ACK, una=4999, expires=5, now=6, interval=1, retries=M32)[2]["retries"][0] == M32
    for rto, iv in ((0, 1), (1, 1), (60000, 60000), (60001, 60000), (M32, 60000)):
        assert int(one(close=1, rto=rto)[2]["interval"][0]) == iv


def test_wraps_of_rcv_nxt_snd_nxt_and_the_clock():
    f, s, x, out, fd, gate, res = one(hit=True, rcv_nxt=M32, close=1, nxt=M32, now=M32 - 10, delivered=7)
    assert (int(f["rcv_nxt"][0]), int(x["base"][0]), int(s["snd_nxt"][0]), int(x["fin_seq"][0])) == (0, 0, 0, M32)
    assert int(x["expires"][0]) == (M32 - 10 + 1000) & M32 == 989
    assert out[38:42].tolist() == [255] * 4 and out[42:46].tolist() == [0, 0, 0, 7], "seq 2^32 - 1, ack_seq 0 + 7"
    assert one(state=FW1, nxt=0, una=0, fin_seq=M32)[6]["events"][0] == ACKED, "snd_una == fin_seq + 1 mod 2^32"
    for expires, now in ((M32 - 1, M32), (M32, M32), (M32, 0), (0, 1), (5, 4), (0x80000000, 0x7FFFFFFF), (0, M32)):
        ev = one(state=FW1, una=4999, expires=expires, interval=10, now=now)[6]["events"][0]
        tw = one(state=TW, expires=expires, interval=60000, now=now)[6]["events"][0]
        assert (int(ev), int(tw)) == ((RESENT, TW_DONE) if expires < now else (0, 0)), (expires, now)
    # target across the wrap: base in front of it, rcv_nxt behind it
    f, s, w, _ = make_sides(1)
    f["rcv_nxt"] = 3
    x = lvlip.fin_flows(f)
    x["base"] = M32 - 5  # lvlip_lro_next_* moved rcv_nxt on by 9
    rec = np.zeros(1, dtype=lvlip.LRO_REC_DTYPE)
    rec["rel"], rec["dlen"], rec["status"], rec["tcp_flags"] = 2, 7, lvlip.LRO_PLACED, 0x19
    got = run_cpu(f, np.zeros(1, dtype=G), rec, s, w, lvlip.rto_flows(1), x, None, 5)
    assert got[6]["events"][0] == PEER_FIN | ACK_OWED and got[0]["rcv_nxt"][0] == 4 and got[2]["state"][0] == CW


def test_a_fin_in_front_of_a_hole_is_ignored_and_one_whose_hole_the_batch_fills_is_taken():
    f, s, w, _ = make_sides(1)
    rec = np.zeros(1, dtype=lvlip.LRO_REC_DTYPE)
    rec["rel"], rec["dlen"], rec["status"], rec["tcp_flags"] = 536, 100, lvlip.LRO_PLACED, 0x19
    gin = np.zeros(1, dtype=G)
    for delivered, taken in ((0, False), (536, False), (636, True)):
        gin["delivered"], gin["placed"] = delivered, 1
        got = run_cpu(f, gin, rec, s, w, lvlip.rto_flows(1), lvlip.fin_flows(f), None, 5)
        assert bool(got[6]["events"][0] & PEER_FIN) == taken
        assert int(got[0]["rcv_nxt"][0]) == (int(f["rcv_nxt"][0]) + taken) & M32
        assert got[5]["placed"][0] == 1, "an ACK that was owed anyway keeps its count"


# ------------------------------------------------------------------- the golden --

@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "fin_ref.json")) as fh:
        return json.load(fh)


class RefPeer:
    """One connection of the reference's stack as this library sees it: the
    stack's header template, its receive side and its send side."""

    def __init__(self, ep):
        first = ep["steps"][0]
        hdr = bytes.fromhex(ep["template"])
        sport, dport = struct.unpack("!HH", hdr[34:38])
        self.f = lvlip.lro_flow(hdr[30:34], hdr[26:30], dport, sport, first["rcv_nxt"], 65535)
        lvlip.lro_plan(self.f)
        self.s = np.zeros(1, dtype=lvlip.SND_FLOW_DTYPE)
        self.s["snd_una"], self.s["snd_nxt"] = first["snd_una"], first["snd_nxt"]
        self.s["win"] = int.from_bytes(hdr[48:50], "big")
        self.w = lvlip.push_flow(hdr, 0, 0, 536, 0, 1, 0, 1)
        self.tmpl = lvlip.ack_tmpl(hdr, max_sack=0)
        self.t, self.x = lvlip.rto_flows(1), lvlip.fin_flows(self.f)
        self.res = np.zeros(1, dtype=G)
        self.now = 0

    def step(self, fed, close):
        """One round: the frame fed (or none) through the receive path, the ACK
        side, lvlip_fin_cpu and lvlip_ack_cpu without LVLIP_ACK_ALL.  Returns
        the frames sent, the FIN first."""
        self.now += TICK
        rec = np.zeros(0, dtype=lvlip.LRO_REC_DTYPE)
        if fed:
            buf = np.frombuffer(fed, dtype=np.uint8)
            fd = np.zeros(1, dtype=FD)
            fd["len"] = len(fed)
            _, rec = lvlip.lro_cpu(buf, fd, self.f, lvlip.RX_VERIFY_L4)
            sres = lvlip.snd_cpu(self.f, self.s, rec, np.zeros(64, dtype=np.uint8), np.zeros(1, dtype=FD))
            lvlip.snd_next_cpu(self.s, sres)
        lvlip.lro_advance_carry(self.f, rec, self.res, self.res)
        lvlip.lro_next_cpu(self.f, self.res)
        out, fd, gate, res = lvlip.fin_cpu(self.f, self.res, rec, self.s, self.w, self.t, self.x,
                                           np.array([close], dtype=np.uint8), self.now)
        lvlip.fin_check(self.x, self.f)
        self.tmpl["hdr"][0, 38:42] = np.frombuffer(struct.pack("!I", int(self.s["snd_nxt"][0])), dtype=np.uint8)
        ack, afd = lvlip.ack_cpu(self.tmpl, self.f, gate, 0)
        sent = [out[:54].tobytes()] if fd["len"][0] else []
        if afd["len"][0]:
            sent.append(ack[int(afd["offset"][0]):int(afd["offset"][0]) + int(afd["len"][0])].tobytes())
        return sent, res


@pytest.mark.parametrize("name", ("active", "passive", "simultaneous", "fin_ack"))
def test_frames_and_states_of_the_reference_stack(name):
    """Every frame the reference emitted while closing, byte for byte, from
    lvlip_fin_cpu (the FIN) and the unchanged lvlip_ack_cpu on its gate (the
    ACK of the peer's FIN), and sk->state, rcv_nxt and snd_nxt after each step.
    One departure is pinned: tcp_close leaves a CLOSE_WAIT socket in CLOSE_WAIT
    (src/tcp.c:278-282) and an ACK of its FIN changes nothing; here the states
    are RFC 793's LAST_ACK and CLOSED."""
    ep = next(e for e in golden()["episodes"] if e["name"] == name)
    peer = RefPeer(ep)
    closed = 0
    for st in ep["steps"][1:]:
        closed |= st["op"] == "close"
        sent, res = peer.step(bytes.fromhex(st["fed"]) if st["fed"] else None, closed)
        assert [x.hex() for x in sent] == st["emitted"], (name, st["op"])
        state = st["state"]
        if name == "passive" and st["op"] != "peer_fin":
            assert state == CW, "the reference's CLOSE_WAIT after close and after the ACK of its FIN"
            state = LAST_ACK if st["op"] == "close" else CLOSED
        assert int(peer.x["state"][0]) == state == int(res["state"][0]), (name, st["op"])
        assert (int(peer.f["rcv_nxt"][0]), int(peer.s["snd_nxt"][0]), int(peer.s["snd_una"][0])) == \
            (st["rcv_nxt"], st["snd_nxt"], st["snd_una"]), (name, st["op"])
        if st["op"] == "close":
            fin = bytes.fromhex(st["emitted"][0])
            assert fin[47] == 0x11, "FIN and ACK, no PSH: what tcp_queue_fin leaves in byte 13"
            assert sent[0] == model_frame(bytes.fromhex(ep["template"]), st["snd_nxt"] - 1, st["rcv_nxt"],
                                          int(peer.s["win"][0]))


# ------------------------------------------------------------------- refusals --

def test_refusals_write_nothing_and_noops():
    L = lvlip.lib()
    f, gin, rec, s, w, t, x, close, now = random_case(4, 3)
    x["interval"] = 1000
    out = np.full(64 * 4, CANARY, dtype=np.uint8)
    fd, res = np.full(64, CANARY, dtype=np.uint8).view(FD), np.full(64, CANARY, dtype=np.uint8).view(R)
    gate, ws = np.full(48 * 4, CANARY, dtype=np.uint8).view(G), np.zeros(64, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data  # noqa: E731
    ok = [ptr(f), ptr(gin), ptr(rec), rec.size, ptr(s), ptr(w), ptr(t), ptr(x), 4, ptr(close), now, ptr(out), ptr(fd),
          ptr(gate), ptr(res)]
    arrays = (f, s, x, out, fd, gate, res)
    keep = [a.tobytes() for a in arrays]

    def untouched():
        return [a.tobytes() for a in arrays] == keep

    def both(args):
        return L.lvlip_fin_cpu(*args), L.lvlip_fin_dev(*args, ptr(ws), None)

    for i in (0, 1, 2, 4, 5, 6, 7, 11, 12, 13, 14):
        bad = list(ok)
        bad[i] = None
        assert both(bad) == (lvlip.EINVAL, lvlip.EINVAL), i
    for i, v in ((8, lvlip.LRO_MAX_FLOWS + 1), (3, 0xFFFFFFF1), (13, ptr(gin))):
        bad = list(ok)
        bad[i] = v
        assert both(bad) == (lvlip.EINVAL, lvlip.EINVAL), i
    assert L.lvlip_fin_dev(*ok, None, None) == lvlip.EINVAL, "no workspace"
    assert untouched()
    fresh = lvlip.fin_flows(f)
    for field, v in (("state", 0), ("state", 2), ("state", 11), ("state", 255), ("reserved", (0,) * 9 + (1,)),
                     ("reserved", (1,) + (0,) * 9), ("interval", 60001), ("base", int(f["rcv_nxt"][3]) ^ 1)):
        q = fresh.copy()
        q[field][3] = v
        assert L.lvlip_fin_check(ptr(q), ptr(f), 4) == lvlip.EINVAL and L.lvlip_fin_check(ptr(q), ptr(f), 3) == lvlip.OK
        with pytest.raises(ValueError):
            lvlip.fin_check(q, f)
        bad = list(ok)
        bad[7] = ptr(q)
        qb = q.tobytes()
        want = lvlip.OK if field == "base" else lvlip.EINVAL  # inside a round rcv_nxt has moved on
        assert L.lvlip_fin_cpu(*bad) == want and q.tobytes() == (qb if want else q.tobytes())
        assert untouched() or field == "base"
        for a, b in zip(arrays, keep):
            if a is not x:
                a[...] = np.frombuffer(b, dtype=a.dtype).reshape(a.shape)
    assert untouched()
    lvlip.fin_check(fresh, f)
    for state in STATES:
        q = fresh.copy()
        q["state"], q["interval"], q["flags"] = state, 60000, 1
        assert L.lvlip_fin_check(ptr(q), ptr(f), 4) == lvlip.OK
    assert L.lvlip_fin_check(None, ptr(f), 1) == lvlip.EINVAL and L.lvlip_fin_check(ptr(fresh), None, 1) == lvlip.EINVAL
    assert L.lvlip_fin_check(None, None, 0) == lvlip.OK
    assert L.lvlip_fin_check(ptr(fresh), ptr(f), lvlip.LRO_MAX_FLOWS + 1) == lvlip.EINVAL
    # nflows == 0 is a no-op, whatever else is passed; n == 0 takes a NULL rec; close may be NULL
    bad = list(ok)
    bad[8] = 0
    nothing = [None, None, None, 9, None, None, None, None, 0, None, 5, None, None, None, None]
    assert both(bad) == (lvlip.OK, lvlip.OK) and L.lvlip_fin_cpu(*nothing) == lvlip.OK and untouched()
    # the device form refuses a misaligned pointer before any HIP call
    for i, off in ((0, 4), (1, 8), (2, 8), (4, 4), (5, 4), (6, 4), (7, 4), (12, 8), (13, 8), (14, 8)):
        bad = list(ok)
        bad[i] += off
        assert L.lvlip_fin_dev(*bad, ptr(ws), None) == lvlip.EINVAL, i
    assert L.lvlip_fin_dev(*ok, ptr(ws) + 8, None) == lvlip.EINVAL and untouched()
    for args in (ok[:2] + [None, 0] + ok[4:], ok[:9] + [None] + ok[10:]):
        assert L.lvlip_fin_cpu(*args) == lvlip.OK and not untouched()
    with pytest.raises(ValueError):
        lvlip.fin_cpu(f, gin, rec, s, w, t, lvlip.fin_flows(f)[:3], close, 5)
    with pytest.raises(ValueError):
        lvlip.fin_cpu(f, gin, rec, s, w, t, x, close, 5, out=np.zeros(64 * 4 - 1, dtype=np.uint8))


# --------------------------------------------------------------- gate and gin --

def test_gate_is_gin_with_placed_raised_only_for_an_owed_ack():
    raised = kept = 0
    for seed in range(4):
        case = random_case(97, 30 + seed)
        gin = case[1]
        got = run_cpu(*case)
        gate, res = got[5], got[6]
        owed = (res["events"] & ACK_OWED) != 0
        up = owed & (gin["placed"] == 0)
        want = gin.copy()
        want["placed"][up] = 1
        assert gate.tobytes() == want.tobytes() and gin["sack"].any()
        raised, kept = raised + int(up.sum()), kept + int((owed & ~up).sum())
        assert case[1].tobytes() == gin.tobytes(), "gin is only read"
    assert raised and kept


# ------------------------------------------------------------- the whole loop --

CLOSE_AT = 3         # the round from which the applications have closed
FIN_ACK_LOST = 2     # the flow whose first ACK of a FIN (from B) never arrives
ACKS_ON = (lvlip.LRO_PLACED, lvlip.LRO_NO_DATA, lvlip.LRO_OUT_OF_WINDOW)


class FinLoop(RtoLoop):
    """RtoLoop (8 flows x 40 x 536 B, every fifth first transmission lost):
    endpoint A sends the data, endpoint B receives it; both have a receive
    side, a send side, a write side, a timer and a close state.  From round
    CLOSE_AT on A's application has closed every flow (its FIN waits for
    `unsent` to reach 0 and then follows data still in flight), B's has closed
    the even flows at once (so it sits in FIN_WAIT while it still receives) and
    closes an odd flow once it has seen A's FIN.  A's first FIN of every second
    flow is lost; so is B's first ACK of A's FIN on flow FIN_ACK_LOST.  A sends
    ACKs only where its gate says one is owed."""

    def run(self, fin: bool, rounds=None):
        p = self.p
        b, n = p.base, p.n
        L = b.link
        fb, fa, snd, w, tmpl = b.fb.copy(), L.fa.copy(), p.snd.copy(), p.w.copy(), L.tmpl.copy()
        ring = np.full(p.ring_bytes, CANARY, dtype=np.uint8)
        fd, sacked = np.zeros(p.nfd, dtype=FD), np.zeros(p.nfd, dtype=np.uint8)
        stream = np.full(L.stream.size, CANARY, dtype=np.uint8)
        res, ares = np.zeros(n, dtype=G), np.zeros(n, dtype=G)
        sres = np.zeros(n, dtype=lvlip.SND_RESULT_DTYPE)
        sent = np.zeros(n * p.segs, dtype=np.int32)
        t = lvlip.rto_flows(n, snd_wnd=b.wnd)
        w["wnd"] = b.wnd
        # A's ACKs of B's FIN; B's send side, write side (its ACK template's header) and timer
        tmpl_a = np.concatenate([lvlip.ack_tmpl(w["hdr"][k].tobytes(), out_off=5 + 91 * k, max_sack=0) for k in range(n)])
        tmpl_a["hdr"][:, 47] = 0x10
        snd_b = np.zeros(n, dtype=lvlip.SND_FLOW_DTYPE)
        snd_b["snd_una"] = snd_b["snd_nxt"] = fa["rcv_nxt"]
        snd_b["seg0"] = np.arange(n)
        w_b = np.concatenate([lvlip.push_flow(tmpl["hdr"][k].tobytes(), 0, 0, p.mss, 0, 1, k, 1) for k in range(n)])
        t_b = lvlip.rto_flows(n)
        xa, xb = lvlip.fin_flows(fa), lvlip.fin_flows(fb)
        fin_a, fin_b = np.full(64 * n, CANARY, dtype=np.uint8), np.full(64 * n, CANARY, dtype=np.uint8)
        none = np.zeros(n, dtype=FD)
        none["offset"] = 64 * np.arange(n)
        arec = np.zeros(0, dtype=lvlip.LRO_REC_DTYPE)
        log = dict(xa=[], xb=[], ea=[], eb=[], nxt=[], drop_fin=[], drop_ack=[], close_b=[], ra=[], rb=[], wnd=[], drop=[],
                   nseg=[])
        ack_a_bytes = lvlip.ack_plan(tmpl_a, fa)
        now = done = 0
        while rounds is None or done < rounds:
            now += TICK
            closing = done >= CLOSE_AT
            pfd, pres = lvlip.push_cpu(fa, None, snd, w, L.payload, ring, fd, sacked)
            gate, rres = lvlip.rto_cpu(snd, sres, pres, t, now, lvlip.RTO_FAST, sacked)
            afd_a, ffd_a, ea = none, none, np.zeros(n, dtype=R)
            nseg = snd["nseg"].copy()  # A's queues as lvlip_fin_* finds them
            ack_a = np.full(ack_a_bytes, CANARY, dtype=np.uint8)
            if fin:
                lvlip.lro_advance_carry(fa, arec, ares, ares)
                lvlip.lro_next_cpu(fa, ares)
                _, ffd_a, gate_a, ea = lvlip.fin_cpu(fa, ares, arec, snd, w, t, xa, np.full(n, closing, dtype=np.uint8),
                                                     now, fin_a)
                lvlip.fin_check(xa, fa)
                tmpl_a["hdr"][:, 38:42] = snd["snd_nxt"].astype(">u4").view(np.uint8).reshape(n, 4)
                _, afd_a = lvlip.ack_cpu(tmpl_a, fa, gate_a, 0, out=ack_a)
                assert ((afd_a["len"] > 0) == ((ea["events"] & ACK_OWED) != 0)).all(), "an ACK exactly where one is owed"
            fd_out, _ = lvlip.rtx_sack_cpu(fa, None, snd, gate, sacked, ring, fd)
            wire = self.wire(pfd, fd_out, ring, sent)
            # the network: A's first FIN of every second flow is lost
            ffd_a = ffd_a.copy()
            first = ((ea["events"] & SENT) != 0) & (np.arange(n) % 2 == 1)
            ffd_a["len"][first] = 0
            # B: the ring's frames, A's FINs and A's ACKs, one record array
            _, rec = lvlip.lro_cpu(ring, wire, fb, lvlip.RX_VERIFY_L4, out=stream)
            _, frec = lvlip.lro_cpu(fin_a, ffd_a, fb, lvlip.RX_VERIFY_L4, out=stream)
            _, krec = lvlip.lro_cpu(ack_a, afd_a, fb, lvlip.RX_VERIFY_L4, out=stream)
            rec = np.concatenate([rec, frec, krec])
            lvlip.lro_advance_carry(fb, rec, res, res)
            wnd = np.minimum(b.wnd, b.end - fb["out_off"] - res["delivered"]).astype(np.uint32)
            tmpl["hdr"][:, 48], tmpl["hdr"][:, 49] = wnd >> 8, wnd & 0xFF
            snd_b["win"] = wnd
            bres = lvlip.snd_cpu(fb, snd_b, rec, np.zeros(64, dtype=np.uint8), np.zeros(n, dtype=FD))
            lvlip.snd_next_cpu(snd_b, bres)
            ffd_b, eb, gate_b = none, np.zeros(n, dtype=R), res
            close_b = closing & ((np.arange(n) % 2 == 0) | (xb["state"] == CW))
            if fin:
                lvlip.lro_next_cpu(fb, res)
                _, ffd_b, gate_b, eb = lvlip.fin_cpu(fb, res, rec, snd_b, w_b, t_b, xb, close_b.astype(np.uint8), now, fin_b)
                lvlip.fin_check(xb, fb)
                tmpl["hdr"][:, 38:42] = snd_b["snd_nxt"].astype(">u4").view(np.uint8).reshape(n, 4)
            ack, afd = lvlip.ack_cpu(tmpl, fb, gate_b, lvlip.ACK_ALL, out=np.full(L.ack_bytes, CANARY, dtype=np.uint8))
            lvlip.lro_next_cpu(fb, res)
            fb["rcv_wnd"] = wnd
            # B acknowledges only a round in which a frame of the flow arrived (tests/test_persist_cpu.py's
            # receiver); the network: B's first ACK of A's FIN on one flow is lost
            got = np.zeros(n, dtype=bool)
            got[rec["flow"][np.isin(rec["status"], ACKS_ON)]] = True
            drop_ack = ((eb["events"] & PEER_FIN) != 0) & (np.arange(n) == FIN_ACK_LOST)
            afd["len"][drop_ack | ~got] = 0
            # A: B's ACKs and B's FINs, one buffer and one record array
            both = np.concatenate([ack, fin_b])
            both_fd = np.concatenate([afd, ffd_b])
            both_fd["offset"][n:] += ack.size
            _, arec = lvlip.lro_cpu(both, both_fd, fa, lvlip.RX_VERIFY_L4, out=np.zeros(n + 64, dtype=np.uint8))
            sres = lvlip.snd_cpu(fa, snd, arec, ring, fd)
            lvlip.sack_cpu(fa, snd, arec, both, both_fd, ring, fd, sacked)
            lvlip.wnd_cpu(fa, snd, t, w, arec, both, both_fd, lvlip.WND_APPLY)
            lvlip.snd_next_cpu(snd, sres)
            for k, v in (("xa", xa["state"]), ("xb", xb["state"]), ("ea", ea["events"]), ("eb", eb["events"]),
                         ("nxt", snd["snd_nxt"]), ("drop_fin", first), ("drop_ack", drop_ack), ("close_b", close_b),
                         ("ra", ea), ("rb", eb), ("wnd", wnd), ("drop", drop_ack | ~got), ("nseg", nseg)):
                log[k].append(np.array(v).copy())
            done += 1
            if rounds is None and (xa["state"] == CLOSED).all() and (xb["state"] == CLOSED).all():
                break
            assert done < 1500, "the loop does not end"
        return dict(stream=stream, fb=fb, fa=fa, snd=snd, snd_b=snd_b, w=w, res=res, ares=ares, sres=sres, ring=ring,
                    fd=fd, sacked=sacked, sent=sent, t=t, xa=xa, xb=xb, fin_a=fin_a, fin_b=fin_b, rounds=done,
                    log={k: np.array(v) for k, v in log.items()})


@functools.lru_cache(maxsize=None)
def fin_loop_cpu():
    loop = FinLoop()
    return loop, loop.run(True)


def test_the_loop_never_closes_without_the_call():
    loop = FinLoop()
    got = loop.run(False, rounds=120)
    p = loop.p
    assert np.array_equal(got["stream"], p.base.link.payload), "the transfer itself ends"
    assert (got["log"]["xa"] == EST).all() and (got["log"]["xb"] == EST).all(), "no flow ever leaves ESTABLISHED"
    last = (p.iss + p.segs * p.mss) & M32
    assert (((last - got["log"]["nxt"].astype(np.int64)) & M32) <= p.segs * p.mss).all(), "snd_nxt never passes the data"
    assert (got["snd"]["snd_nxt"] == last).all() and (got["snd_b"]["snd_nxt"] == got["snd_b"]["snd_una"]).all()


def test_the_loop_closes_all_sixteen_endpoints_with_the_call():
    loop, got = fin_loop_cpu()
    p, log = loop.p, got["log"]
    n = p.n
    assert np.array_equal(got["stream"], p.base.link.payload), "the streams are not the payloads"
    assert (got["xa"]["state"] == CLOSED).all() and (got["xb"]["state"] == CLOSED).all()
    last = (p.iss + p.segs * p.mss) & M32
    assert (got["snd"]["snd_nxt"] == (last + 1) & M32).all() and (got["snd"]["snd_una"] == got["snd"]["snd_nxt"]).all()
    assert (got["fb"]["rcv_nxt"] == got["snd"]["snd_nxt"]).all() and (got["fa"]["rcv_nxt"] == got["snd_b"]["snd_nxt"]).all()
    assert (got["snd_b"]["snd_una"] == got["snd_b"]["snd_nxt"]).all() and not got["snd"]["nseg"].any()
    assert (got["xa"]["fin_seq"] == last).all() and not got["t"]["dead"].any()
    assert log["drop_fin"].sum(0).tolist() == [k % 2 for k in range(n)] and log["drop_ack"].sum() == 1
    ev_a, ev_b = np.bitwise_or.reduce(log["ea"], 0), np.bitwise_or.reduce(log["eb"], 0)
    assert (ev_a[1::2] & RESENT).all(), "a lost FIN goes out again"
    assert ev_a[FIN_ACK_LOST] & RESENT and ((log["eb"][:, FIN_ACK_LOST] & ACK_OWED) != 0).sum() >= 2, \
        "the FIN whose ACK was lost goes out again and is acknowledged again"
    for side, ev in ((log["xa"], ev_a), (log["xb"], ev_b)):
        assert (ev & (SENT | ACKED | PEER_FIN)).tolist() == [SENT | ACKED | PEER_FIN] * n
        assert not (ev & LATE_WRITE).any()
        for k in range(n):
            seq = [int(v) for i, v in enumerate(side[:, k]) if i == 0 or v != side[i - 1, k]]
            assert seq[-1] == CLOSED and all((a, b) in ((EST, FW1), (EST, CW), (FW1, FW2), (FW1, CLOSING), (FW1, TW),
                                                        (FW2, TW), (CLOSING, TW), (CW, LAST_ACK), (TW, CLOSED),
                                                        (LAST_ACK, CLOSED), (EST, LAST_ACK)) for a, b in zip(seq, seq[1:])), seq
    paths = {tuple(int(v) for i, v in enumerate(side[:, k]) if i == 0 or v != side[i - 1, k])
             for side in (log["xa"], log["xb"]) for k in range(n)}
    assert any(TW in q for q in paths) and any(LAST_ACK in q for q in paths), paths
    assert ((log["ea"] & TW_DONE) != 0).sum() + ((log["eb"] & TW_DONE) != 0).sum() >= 1
    assert (((log["ea"] & SENT) != 0) & (log["nseg"] > 0)).any(), "on some flow A's FIN leaves while data is in flight"
    assert got["rounds"] > 200, "TIME_WAIT lasts 2 MSL of the loop's clock"
