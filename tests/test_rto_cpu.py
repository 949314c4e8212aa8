"""The retransmission timer on the calling thread (rto_cpu.c, include/lvlip_skb.h
"the timer and the peer's window"): lvlip_rto_cpu against the reference's own
tcp_rtt and timer handler (tests/golden/rto_ref.json, every step bit for bit),
the order of its four steps, the gate, dead flows, the scoreboard clear, the
refusals, and the gate in front of lvlip_rtx_sack_cpu; the loop with a clock;
the example."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import lvlip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
NONE = 0xFFFFFFFF
T, SR, PR, S = lvlip.RTO_FLOW_DTYPE, lvlip.SND_RESULT_DTYPE, lvlip.PUSH_RESULT_DTYPE, lvlip.SND_FLOW_DTYPE


def flows(n=1, **kw):
    t = lvlip.rto_flows(n)
    for k, v in kw.items():
        t[k] = v
    return t


def call(t, nseg, now, n_new=0, n_dup=0, pushed=0, flags=0, sacked=None, seg0=None):
    """One lvlip_rto_cpu call on arrays built from scalars or lists."""
    n = t.size
    s = np.zeros(n, dtype=S)
    s["nseg"] = nseg
    s["seg0"] = np.arange(n) * 1000 if seg0 is None else seg0
    sres, pres = np.zeros(n, dtype=SR), np.zeros(n, dtype=PR)
    sres["n_new"], sres["n_dup"], pres["pushed"] = n_new, n_dup, pushed
    sres["snd_una"], sres["inflight"] = 77, s["nseg"]  # the gate must not copy them
    return lvlip.rto_cpu(s, sres, pres, t, now, flags, sacked)


def state(t, k=0):
    return dict(srtt=int(t["srtt"][k]), rttvar=int(t["rttvar"][k]), rto=int(t["rto"][k]), backoff=int(t["backoff"][k]),
                armed=int(t["armed"][k]))


def test_layout_and_symbols():
    assert T.itemsize == 32 and [T.fields[k][1] for k in ("rto", "wnd_cap", "armed", "wscale")] == [8, 24, 28, 31]
    for name in ("lvlip_rto_check", "lvlip_rto_cpu", "lvlip_rto_dev", "lvlip_wnd_cpu", "lvlip_wnd_dev"):
        assert hasattr(lvlip.lib(), name)
    src = open(os.path.join(ROOT, "level-ip_amd", "BUILD_SOURCES")).read()
    assert "csrc/rto_cpu.c" in src and "csrc/rto_kernels.hip" in src


# ------------------------------------------------------- the reference's steps --

@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "rto_ref.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ("backoff", "samples", "large"))
def test_every_golden_step_bit_for_bit(name):
    """One flow carried through a whole session of the reference by
    lvlip_rto_cpu alone; only the clock is set per step.  In a sample step the
    timer expires at the top of the clock's range, so that step 3 (an unsigned
    comparison, as src/timer.c:71 is) never fires inside it: the reference's
    tcp_rtt was called on its own."""
    steps = next(s["steps"] for s in golden()["sessions"] if s["name"] == name)
    t = flows()
    nseg, clock, seen = 0, 5000, set()
    for i, st in enumerate(steps):
        op = st["op"]
        seen.add(op)
        if op == "push":
            clock += 17
            nseg = 1
            _, res = call(t, nseg, clock, pushed=1)
            assert int(t["expires"][0]) == (clock + st["expires_minus_now"]) & M32 and res["fired"][0] == 0
        elif op in ("rtt", "rtt_backoff", "rtt_unarmed", "ack_all"):
            if t["armed"][0]:
                t["expires"] = M32
            now = (int(t["expires"][0]) - int(t["rto"][0]) + st["r"]) & M32
            if op == "ack_all":
                nseg = 0
            took = op in ("rtt", "ack_all") and st["r"] >= 0 and t["backoff"][0] == 0 and t["armed"][0]
            gate, res = call(t, nseg, now, n_new=1)
            assert res["fired"][0] == 0 and gate["popped"][0] == nseg
            assert res["sample"][0] == (st["r"] if took else NONE), (i, st)
        elif op == "timeout":
            t["expires"] = clock = clock + 1000 * i  # wherever a sample step left it
            clock += 1
            gate, res = call(t, nseg, clock)
            assert res["fired"][0] == lvlip.RTO_TIMEOUT and gate["popped"][0] == 0
            assert int(t["dead"][0]) == st["dead"]
            if not st["dead"]:
                assert int(t["expires"][0]) == (clock + int(t["rto"][0])) & M32
        else:
            raise AssertionError(op)
        assert state(t) == st["after"], (name, i, st, state(t))
        assert res["rto"][0] == st["after"]["rto"] and res["backoff"][0] == st["after"]["backoff"]
    assert seen >= {"backoff": {"push", "timeout", "rtt_backoff"}, "samples": {"rtt", "rtt_unarmed", "ack_all", "push"},
                    "large": {"rtt"}}[name]


def test_integer_estimator_equals_double_arithmetic():
    """The header's claim, on random state: (3 v + |s - r|) / 4 and (7 s + r) / 8
    truncated equal the reference's double expressions (src/tcp.c:442-443)."""
    rng = np.random.default_rng(3)
    n = 2000
    srtt = rng.integers(1, 1 << 24, n)
    rttvar = rng.integers(0, 1 << 24, n)
    r = rng.integers(0, 1 << 24, n)
    t = flows(n, srtt=srtt, rttvar=rttvar, armed=1, expires=M32, rto=1000)
    now = (M32 - 1000 + r) & M32
    for k in range(n):  # one clock per call
        tk = t[k:k + 1]
        call(tk, 1, int(now[k]), n_new=1)
        v = int(0.75 * int(rttvar[k]) + 0.25 * abs(int(srtt[k]) - int(r[k])))
        s = int(0.875 * int(srtt[k]) + 0.125 * int(r[k]))
        assert (int(tk["rttvar"][0]), int(tk["srtt"][0]), int(tk["rto"][0])) == (v, s, s + max(4 * v, 200))


# ----------------------------------------------------------- order and outputs --

def test_order_of_the_steps():
    # 1 before 2: the ACK that empties the queue stops the timer, the push in the same round arms it afresh
    t = flows(armed=1, expires=9000, backoff=2, rto=4000)
    gate, res = call(t, 3, 6000, n_new=1, pushed=3)
    assert (t["armed"][0], t["backoff"][0], t["expires"][0]) == (1, 0, 10000) and res["sample"][0] == NONE
    # ... while a queue that still held entries keeps its timer and its backoff
    t = flows(armed=1, expires=9000, backoff=2, rto=4000)
    call(t, 4, 6000, n_new=1, pushed=3)
    assert (t["armed"][0], t["backoff"][0], t["expires"][0]) == (1, 2, 9000)
    # 1 before 3: the sample is taken with the rto the timer was armed with, then the timer fires on the NEW rto
    t = flows(armed=1, expires=2000, rto=1000)
    gate, res = call(t, 2, 2001, n_new=1)
    assert res["sample"][0] == 1001 and res["fired"][0] == 1
    assert (t["srtt"][0], t["rttvar"][0]) == (1001, 500) and t["rto"][0] == 2 * (1001 + 2000) and t["backoff"][0] == 1
    assert t["expires"][0] == 2001 + t["rto"][0] and gate["popped"][0] == 0
    # 2 before 3: a timer armed in this call expires in the future
    t = flows()
    gate, res = call(t, 1, 123456, pushed=1)
    assert res["fired"][0] == 0 and t["expires"][0] == 124456 and gate["popped"][0] == 1
    # 3: strict; the empty queue disarms without firing
    t = flows(armed=1, expires=500)
    assert call(t, 1, 500)[1]["fired"][0] == 0 and call(t, 1, 501)[1]["fired"][0] == 1
    t = flows(armed=1, expires=500, backoff=3)
    gate, res = call(t, 0, 501)
    assert res["fired"][0] == 0 and (t["armed"][0], t["backoff"][0]) == (0, 0) and gate["popped"][0] == 0
    # 3 before 4: a timeout is not also a fast retransmit
    t = flows(armed=1, expires=500, dupacks=2)
    assert call(t, 1, 501, n_dup=1, flags=lvlip.RTO_FAST)[1]["fired"][0] == lvlip.RTO_TIMEOUT
    # r < 0 returns
    t = flows(armed=1, expires=5000, rto=1000)
    assert call(t, 1, 3999, n_new=1)[1]["sample"][0] == NONE and state(t)["srtt"] == 0
    assert call(t, 1, 4000, n_new=1)[1]["sample"][0] == 0


def test_fast_retransmit():
    t = flows(armed=1, expires=M32)
    for now, n_dup, want in ((10, 1, 0), (20, 1, 0), (30, 1, 2), (40, 1, 0), (50, 5, 0)):
        before = t.copy()
        gate, res = call(t, 4, now, n_dup=n_dup, flags=lvlip.RTO_FAST)
        assert res["fired"][0] == want and gate["popped"][0] == (0 if want else 4)
        before["dupacks"] += n_dup
        assert t.tobytes() == before.tobytes(), "a fast retransmit changes no timer state"
    assert call(t, 4, 60, n_new=1, n_dup=9, flags=lvlip.RTO_FAST)[1]["fired"][0] == 0 and t["dupacks"][0] == 0
    # crossing 3 in one batch; not without the flag; not with an empty queue
    t = flows(dupacks=1)
    assert call(t, 4, 10, n_dup=7, flags=lvlip.RTO_FAST)[1]["fired"][0] == 2
    t = flows(dupacks=1)
    assert call(t, 4, 10, n_dup=7)[1]["fired"][0] == 0 and t["dupacks"][0] == 8
    t = flows(dupacks=1)
    assert call(t, 0, 10, n_dup=7, flags=lvlip.RTO_FAST)[1]["fired"][0] == 0


def test_gate_is_a_whole_result_and_dead_flows_are_inert():
    t = flows(4, armed=[1, 1, 1, 0], expires=[100, 100, 900, 0], rto=[1000, 70000, 1000, 1000], dead=[0, 0, 0, 1],
              backoff=[0, 6, 0, 3], dupacks=[0, 0, 0, 2])
    keep = t[3:4].copy()
    sacked = np.full(4000, 1, dtype=np.uint8)
    gate, res = call(t, [5, 6, 7, 8], 200, n_new=[0, 0, 0, 1], n_dup=[0, 0, 0, 5], pushed=[0, 0, 0, 8],
                     flags=lvlip.RTO_FAST, sacked=sacked)
    assert res["fired"].tolist() == [1, 1, 0, 0] and gate["popped"].tolist() == [0, 0, 7, 8]
    for k in SR.names:
        if k != "popped":
            assert not gate[k].any(), k
    assert t["dead"].tolist() == [0, 1, 0, 1] and t["armed"].tolist() == [1, 0, 1, 0]
    assert t["rto"].tolist() == [2000, 70000, 1000, 1000] and t["backoff"].tolist() == [1, 0, 0, 3]
    assert t[3:4].tobytes() == keep.tobytes() and list(res[3].tolist()) == [0, NONE, 1000, 3]
    # the flow that died fired once (the head goes out first there too) and never again
    gate, res = call(t, [5, 6, 7, 8], 10 ** 6, n_dup=9, flags=lvlip.RTO_FAST)
    assert res["fired"].tolist() == [1, 0, 1, 0] and gate["popped"].tolist() == [0, 6, 0, 8]


def test_scoreboard_is_cleared_only_inside_timed_out_queues():
    rng = np.random.default_rng(1)
    nseg = np.array([0, 1, 63, 64, 65, 200, 9, 9])
    seg0 = np.array([3, 11, 101, 301, 501, 701, 1001, 1101])
    t = flows(8, armed=1, expires=100)
    t["armed"][6] = 0                      # silent
    t["dupacks"][7], t["armed"][7] = 2, 0  # fast: keeps its marks
    sacked = rng.integers(1, 4, 1200).astype(np.uint8)
    want = sacked.copy()
    for k in range(6):
        want[seg0[k]:seg0[k] + nseg[k]] = 0
    gate, res = call(t, nseg, 101, n_dup=[0] * 7 + [1], flags=lvlip.RTO_FAST, sacked=sacked, seg0=seg0)
    assert res["fired"].tolist() == [0, 1, 1, 1, 1, 1, 0, 2]
    assert sacked.tobytes() == want.tobytes() and sacked[seg0[2] - 1] and sacked[seg0[2] + 63]


def test_refusals_and_noops():
    L = lvlip.lib()
    t, s = flows(2), np.zeros(2, dtype=S)
    gate, res = np.zeros(2, dtype=SR), np.zeros(2, dtype=lvlip.RTO_RESULT_DTYPE)
    p = lambda a: a.ctypes.data  # noqa: E731
    ok = (p(s), None, None, p(t), 2, 5, 0, None, p(gate), p(res))
    assert L.lvlip_rto_cpu(*ok) == lvlip.OK
    assert L.lvlip_rto_cpu(None, None, None, None, 0, 5, 0, None, None, None) == lvlip.OK
    keep = t.tobytes()
    for i in (0, 3, 8, 9):
        bad = list(ok)
        bad[i] = None
        assert L.lvlip_rto_cpu(*bad) == lvlip.EINVAL
    bad = list(ok)
    bad[6] = 2
    assert L.lvlip_rto_cpu(*bad) == lvlip.EINVAL
    bad[6], bad[4] = 0, lvlip.LRO_MAX_FLOWS + 1
    assert L.lvlip_rto_cpu(*bad) == lvlip.EINVAL
    assert t.tobytes() == keep
    for field, v in (("wscale", 15), ("armed", 2), ("dead", 2), ("snd_wnd", (1 << 30) + 1), ("wnd_cap", (1 << 30) + 1)):
        u = flows(2)
        u[field][1] = v
        assert L.lvlip_rto_check(p(u), 2) == lvlip.EINVAL and L.lvlip_rto_check(p(u), 1) == lvlip.OK
        with pytest.raises(ValueError):
            lvlip.rto_check(u)
        assert L.lvlip_rto_cpu(p(s), None, None, p(u), 2, 5, 0, None, p(gate), p(res)) == lvlip.EINVAL
    assert L.lvlip_rto_check(None, 1) == lvlip.EINVAL and L.lvlip_rto_check(None, 0) == lvlip.OK
    # the device form: the same refusals and a misaligned pointer before any HIP call
    dok = ok + (None,)
    for i, v in ((0, None), (3, None), (8, None), (9, None), (6, 2), (0, p(s) + 4), (3, p(t) + 4), (8, p(gate) + 8),
                 (9, p(res) + 8), (1, p(gate) + 8), (2, p(res) + 4)):
        bad = list(dok)
        bad[i] = v
        assert L.lvlip_rto_dev(*bad) == lvlip.EINVAL, i
    assert L.lvlip_rto_dev(None, None, None, None, 0, 5, 0, None, None, None, None) == lvlip.OK
    with pytest.raises(ValueError):
        lvlip.rto_cpu(s, None, None, flows(3), 5)
    with pytest.raises(ValueError):
        s2 = s.copy()
        s2["nseg"] = 5
        lvlip.rto_cpu(s2, None, None, t, 5, sacked=np.zeros(3, dtype=np.uint8))
    # pushed beyond the queue is clamped; NULL results mean no ACK and no push
    u = flows(1)
    s1 = np.zeros(1, dtype=S)
    s1["nseg"] = 2
    pres = np.zeros(1, dtype=PR)
    pres["pushed"] = 9
    lvlip.rto_cpu(s1, None, pres, u, 50)
    assert u["armed"][0] == 1 and u["expires"][0] == 1050
    u = flows(1, dupacks=2)
    assert lvlip.rto_cpu(s1, None, None, u, 50, lvlip.RTO_FAST)[1]["fired"][0] == 0


# ------------------------------------------------------ the gate and the retransmit --

def test_the_gate_resends_exactly_the_fired_flows():
    from test_push_cpu import PushLoop

    loop = PushLoop()
    L, n = loop.base.link, loop.n
    fa, snd, w = L.fa.copy(), loop.snd.copy(), loop.w.copy()
    ring = np.zeros(loop.ring_bytes, dtype=np.uint8)
    fd, sacked = np.zeros(loop.nfd, dtype=lvlip.FRAME_DESC_DTYPE), np.zeros(loop.nfd, dtype=np.uint8)
    _, pres = lvlip.push_cpu(fa, None, snd, w, L.payload, ring, fd, sacked)
    t = flows(n)
    gate, res = lvlip.rto_cpu(snd, None, pres, t, 1000, 0, sacked)
    assert not res["fired"].any() and t["armed"].all() and (gate["popped"] == snd["nseg"]).all()
    fd_out, pick = lvlip.rtx_sack_cpu(fa, None, snd, gate, sacked, ring.copy(), fd)
    assert not fd_out["len"].any() and (pick == NONE).all()
    t["expires"][[1, 4, 6]] = 1500  # three flows time out, one with marks on its queue
    sacked[snd["seg0"][4]:snd["seg0"][4] + 3] = 1
    gate, res = lvlip.rto_cpu(snd, None, None, t, 1501, 0, sacked)
    assert np.flatnonzero(res["fired"]).tolist() == [1, 4, 6] and not sacked.any()
    ungated, _ = lvlip.rtx_sack_cpu(fa, None, snd, None, sacked, ring.copy(), fd)
    fd_out, pick = lvlip.rtx_sack_cpu(fa, None, snd, gate, sacked, ring, fd)
    live = (fd_out["len"] > 0).reshape(n, loop.rtx)
    assert live.all(axis=1).tolist() == [k in (1, 4, 6) for k in range(n)] and int(live.sum()) == 3 * loop.rtx
    for k in (1, 4, 6):
        sl = slice(k * loop.rtx, (k + 1) * loop.rtx)
        assert fd_out[sl].tobytes() == ungated[sl].tobytes()
    assert (ungated["len"] > 0).all()


# ------------------------------------------------------------- the whole loop --

TICK = 300  # ms of the caller's clock per round


class RtoLoop:
    """tests/test_push_cpu.py's PushLoop (8 flows x 40 x 536 B, every fifth
    first transmission lost, 16 slots) with a clock, the peer's window and the
    timer: new segments go out once, as lvlip_push_* built them; what
    lvlip_rtx_sack_* sends is gated by lvlip_rto_* (`gated`) or, for the count
    to compare with, every unmarked head entry every round.  The receiver
    writes its real window into the ACK template each round, and lvlip_wnd_*
    hands it to lvlip_push_*."""

    def __init__(self):
        from test_push_cpu import PushLoop

        self.p = PushLoop()

    def wire(self, pfd, fd_out, ring, sent):
        both = np.concatenate([pfd, fd_out])
        live = both["len"] > 0
        off = both["offset"].astype(np.int64)
        seq = np.zeros(both.size, dtype=np.int64)
        for j in range(4):
            seq = (seq << 8) | ring[off + 38 + j]
        p = self.p
        flow = np.concatenate([np.arange(pfd.size) // p.rtx, np.arange(fd_out.size) // p.rtx])
        seg = np.clip(((seq - p.iss[flow]) & M32) // p.mss, 0, p.segs - 1)
        idx = flow * p.segs + seg
        first = np.zeros(both.size, dtype=bool)
        first[:pfd.size] = True  # a first transmission is one lvlip_push_* built this round
        lost = live & first & (seg % 5 == 4)
        np.add.at(sent, idx, live.astype(np.int32))
        out = both.copy()
        out["len"][lost] = 0
        return out

    def run_cpu(self, gated: bool, rounds=None):
        p = self.p
        b, n = p.base, p.n
        L = b.link
        fb, fa, snd, w, tmpl = b.fb.copy(), L.fa.copy(), p.snd.copy(), p.w.copy(), L.tmpl.copy()
        ring = np.full(p.ring_bytes, 0x5A, dtype=np.uint8)
        fd, sacked = np.zeros(p.nfd, dtype=lvlip.FRAME_DESC_DTYPE), np.zeros(p.nfd, dtype=np.uint8)
        stream = np.full(L.stream.size, 0x5A, dtype=np.uint8)
        res = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
        sres = np.zeros(n, dtype=SR)
        sent = np.zeros(n * p.segs, dtype=np.int32)
        t = lvlip.rto_flows(n, snd_wnd=b.wnd)
        w["wnd"] = b.wnd
        resent, now, done = 0, 0, 0
        while rounds is None or done < rounds:
            now += TICK
            pfd, pres = lvlip.push_cpu(fa, None, snd, w, L.payload, ring, fd, sacked)
            gate, rres = lvlip.rto_cpu(snd, sres, pres, t, now, lvlip.RTO_FAST, sacked)
            fd_out, _ = lvlip.rtx_sack_cpu(fa, None, snd, gate if gated else None, sacked, ring, fd)
            resent += int((fd_out["len"] > 0).sum())
            wire = self.wire(pfd, fd_out, ring, sent)
            _, rec = lvlip.lro_cpu(ring, wire, fb, lvlip.RX_VERIFY_L4, out=stream)
            lvlip.lro_advance_carry(fb, rec, res, res)
            wnd = np.minimum(b.wnd, b.end - fb["out_off"] - res["delivered"]).astype(np.uint32)  # as it will reopen
            tmpl["hdr"][:, 48], tmpl["hdr"][:, 49] = wnd >> 8, wnd & 0xFF
            ack, afd = lvlip.ack_cpu(tmpl, fb, res, lvlip.ACK_ALL, out=np.full(L.ack_bytes, 0x5A, dtype=np.uint8))
            lvlip.lro_next_cpu(fb, res)
            fb["rcv_wnd"] = wnd
            _, arec = lvlip.lro_cpu(ack, afd, fa, lvlip.RX_VERIFY_L4, out=np.zeros(n + 64, dtype=np.uint8))
            sres = lvlip.snd_cpu(fa, snd, arec, ring, fd)
            lvlip.sack_cpu(fa, snd, arec, ack, afd, ring, fd, sacked)
            wres = lvlip.wnd_cpu(fa, snd, t, w, arec, ack, afd, lvlip.WND_APPLY)
            lvlip.snd_next_cpu(snd, sres)
            done += 1
            if rounds is None and not snd["nseg"].any() and not w["unsent"].any():
                break
            assert done < 2000, "the loop does not end"
        return dict(stream=stream, fb=fb, snd=snd, w=w, res=res, sres=sres, ring=ring, fd=fd, sacked=sacked, sent=sent,
                    t=t, wres=wres, rres=rres, gate=gate, resent=resent, rounds=done)

    def check_done(self, got: dict):
        p = self.p
        L = p.base.link
        assert np.array_equal(got["stream"], L.payload), "the streams are not the payloads"
        assert not got["snd"]["nseg"].any() and (got["snd"]["snd_una"] == got["snd"]["snd_nxt"]).all()
        assert not got["w"]["unsent"].any() and (got["fb"]["rcv_nxt"] == got["snd"]["snd_nxt"]).all()
        assert ((got["snd"]["snd_nxt"].astype(np.int64) - p.iss) & M32 == p.segs * p.mss).all()
        assert (got["sent"].reshape(p.n, p.segs)[:, 4::5] >= 2).all(), "every lost frame went out again"
        assert not got["t"]["dead"].any()


@functools.lru_cache(maxsize=None)
def rto_loop_cpu():
    loop = RtoLoop()
    return loop, loop.run_cpu(True), loop.run_cpu(False)


def test_the_loop_with_a_clock_on_the_cpu_forms():
    loop, gated, ungated = rto_loop_cpu()
    loop.check_done(gated)
    loop.check_done(ungated)
    assert 0 < gated["resent"] <= ungated["resent"], (gated["resent"], ungated["resent"])
    n, segs = loop.p.n, loop.p.segs
    assert gated["resent"] >= n * segs // 5  # every lost frame at least
    assert (gated["t"]["srtt"] > 0).all() and (gated["t"]["snd_wnd"] <= loop.p.base.wnd).all()


# ------------------------------------------------------ example and sanitizers --

C_SRCS = ("rto_cpu.c", "push_cpu.c", "sack_cpu.c", "snd_cpu.c", "ack_cpu.c", "rcv_cpu.c", "seg_cpu.c", "csum_cpu.c")


def test_example_runs_to_its_own_check():
    exe = os.path.join(ROOT, "examples", "build", "rto_loop")
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rto_loop ok" in r.stdout, r.stdout + r.stderr


def _sanitized(tmp_path, main_c, exe_name):
    exe = tmp_path / exe_name
    src = [main_c] + [os.path.join(ROOT, "level-ip_amd", "csrc", f) for f in C_SRCS]
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "include"), *src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    return r.stdout


def test_example_under_sanitizers(tmp_path):
    assert "rto_loop ok" in _sanitized(tmp_path, os.path.join(ROOT, "examples", "rto_loop.c"), "rto_loop_san")


def test_hostile_records_and_frames_under_sanitizers(tmp_path):
    """tests/sanitize/rto_hostile.c, a stand-alone main: lvlip_wnd_cpu and
    lvlip_rto_cpu on crafted records, frames malloc'd at exactly their length
    and extreme timer state, under ASan + UBSan."""
    assert "rto_hostile ok" in _sanitized(tmp_path, os.path.join(ROOT, "tests", "sanitize", "rto_hostile.c"),
                                          "rto_hostile_san")


def test_ctypes_signatures_take_the_documented_arguments():
    assert len(lvlip.SIGNATURES["lvlip_rto_cpu"][1]) == 10 and len(lvlip.SIGNATURES["lvlip_rto_dev"][1]) == 11
    assert len(lvlip.SIGNATURES["lvlip_wnd_cpu"][1]) == 11 and len(lvlip.SIGNATURES["lvlip_wnd_dev"][1]) == 12
