"""The congestion window on the calling thread (cc_cpu.c, include/lvlip_skb.h
"the congestion window"): the layout, lvlip_cc_cpu against a plain restatement
of the header's four steps over random state in every branch, scripted sessions
with hand-checked numbers at mss 536, the pipe, the refusals, the loop of
tests/test_rto_cpu.py with the call in every round, the example and the
sanitizer builds."""
import functools
import os
import subprocess

import numpy as np
import pytest

import lvlip
from test_rto_cpu import TICK, RtoLoop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
MAXW = 1 << 30
C, R, T = lvlip.CC_FLOW_DTYPE, lvlip.CC_RESULT_DTYPE, lvlip.RTO_FLOW_DTYPE
S, SR, RR, FD = lvlip.SND_FLOW_DTYPE, lvlip.SND_RESULT_DTYPE, lvlip.RTO_RESULT_DTYPE, lvlip.FRAME_DESC_DTYPE
EV_TIMEOUT, EV_ENTER, EV_EXIT, EV_SLOWSTART, EV_AVOID = 1, 2, 4, 8, 16
QUEUES = (0, 1, 63, 64, 65, 200)


def test_layout_and_symbols():
    assert C.itemsize == 32 and R.itemsize == 16 and lvlip.CC_FLOW is C and lvlip.CC_RESULT is R
    assert [C.fields[k][1] for k in ("cwnd", "ssthresh", "recover", "acc", "cwnd_max", "mss", "in_rec", "reserved",
                                     "reserved2")] == [0, 4, 8, 12, 16, 20, 22, 23, 24]
    assert [R.fields[k][1] for k in ("cwnd", "sacked_bytes", "n_sacked", "event")] == [0, 4, 8, 12]
    for name in ("lvlip_cc_check", "lvlip_cc_cpu", "lvlip_cc_dev"):
        assert hasattr(lvlip.lib(), name)
    src = open(os.path.join(ROOT, "level-ip_amd", "BUILD_SOURCES")).read()
    assert "csrc/cc_cpu.c" in src and "csrc/cc_kernels.hip" in src
    assert (lvlip.CC_MAX_WND, lvlip.CC_EV_TIMEOUT, lvlip.CC_EV_ENTER, lvlip.CC_EV_EXIT, lvlip.CC_EV_SLOWSTART,
            lvlip.CC_EV_AVOID) == (MAXW, EV_TIMEOUT, EV_ENTER, EV_EXIT, EV_SLOWSTART, EV_AVOID)
    assert len(lvlip.SIGNATURES["lvlip_cc_cpu"][1]) == 9 and len(lvlip.SIGNATURES["lvlip_cc_dev"][1]) == 10


def test_cc_init_is_the_rfc_5681_initial_window():
    c = lvlip.cc_init([536, 1095, 1460, 2190, 2191, 9000, 1], 1 << 20)
    assert c["cwnd"].tolist() == [2144, 4380, 4380, 4380, 4382, 18000, 4]
    assert (c["ssthresh"] == MAXW).all() and (c["cwnd_max"] == 1 << 20).all() and not c["in_rec"].any()
    lvlip.cc_check(c)
    assert lvlip.cc_init(536, 1000, nflows=3)["cwnd"].tolist() == [1000] * 3  # held to the ceiling


# ------------------------------------------------------ an independent model --

def model(s, snd, prev, c, t, fd, sacked):
    """The header's four steps with plain ints.  Returns (c, wnd_cap, res) as
    new arrays; nothing is modified."""
    c, cap = c.copy(), t["wnd_cap"].copy()
    res = np.zeros(s.size, dtype=R)
    for k in range(s.size):
        x = {f: int(c[f][k]) for f in ("cwnd", "ssthresh", "recover", "acc", "cwnd_max", "mss", "in_rec")}
        if t["dead"][k]:
            res[k] = (x["cwnd"], 0, 0, 0)
            continue
        mss, una, nxt = x["mss"], int(s["snd_una"][k]), int(s["snd_nxt"][k])
        flight = (nxt - una) & M32
        a, n_new = (int(snd["acked"][k]), int(snd["n_new"][k])) if snd is not None else (0, 0)
        fired, bo = (int(prev["fired"][k]), int(prev["backoff"][k])) if prev is not None else (0, 0)
        half = max(flight // 2, 2 * mss)
        event = 0
        if fired == 1:
            if bo == 1:
                x["ssthresh"] = half
            x.update(cwnd=mss, acc=0, in_rec=0, recover=nxt)
            event |= EV_TIMEOUT
        elif fired == 2 and x["in_rec"] == 0:
            x.update(ssthresh=half, cwnd=half, acc=0, in_rec=1, recover=nxt)
            event |= EV_ENTER
        if n_new > 0 and a > 0:
            if x["in_rec"] == 1:
                if a >= (x["recover"] - una) & M32:
                    x.update(in_rec=0, cwnd=x["ssthresh"], acc=0)
                    event |= EV_EXIT
            elif x["cwnd"] < x["ssthresh"]:
                x["cwnd"] += min(a, n_new * mss)
                event |= EV_SLOWSTART
            else:
                x["acc"] += a
                if x["acc"] >= x["cwnd"]:
                    x["acc"] -= x["cwnd"]
                    x["cwnd"] += mss
                    event |= EV_AVOID
                x["acc"] = min(x["acc"], x["cwnd"])
            x["cwnd"] = min(x["cwnd"], x["cwnd_max"])
        n_sacked = nbytes = 0
        if sacked is not None:
            nseg = int(s["nseg"][k])
            p = min(int(snd["popped"][k]), nseg) if snd is not None else 0
            for q in range(int(s["seg0"][k]) + p, int(s["seg0"][k]) + nseg):
                if sacked[q]:
                    n_sacked += 1
                    if fd["len"][q] >= 54:
                        nbytes += int(fd["len"][q]) - 54
            nbytes = min(nbytes, MAXW)
        for f, v in x.items():
            c[f][k] = v
        cap[k] = min(x["cwnd"] + nbytes, MAXW)
        res[k] = (x["cwnd"], nbytes, n_sacked, event)
    return c, cap, res


def random_case(nflows: int, seed: int, queues=QUEUES):
    """State in every branch of the four steps; queues of `queues` entries at
    odd seg0 with gaps, a third of the entries marked (1 or 0xFF), some
    descriptors shorter than a header."""
    rng = np.random.default_rng(seed)
    pick = lambda v: rng.choice(np.array(v, dtype=np.int64), nflows)  # noqa: E731
    mss = pick([1, 536, 536, 1460, 9000, 65495])
    c = lvlip.cc_init(mss, MAXW)
    c["cwnd_max"] = np.maximum(mss, pick([MAXW, MAXW, 1 << 20, 20000, 4000]))
    c["cwnd"] = np.clip(pick([0, 2144, 4288, 30000, 1 << 20, MAXW]), mss, c["cwnd_max"])
    c["cwnd"][rng.random(nflows) < .1] = MAXW  # above a small ceiling: legal, step 1 leaves such a state
    c["ssthresh"] = pick([0, 2144, 4288, 10000, 1 << 20, MAXW, MAXW])
    low = rng.random(nflows) < .4  # congestion avoidance
    c["ssthresh"][low] = np.minimum(c["ssthresh"][low], c["cwnd"][low])
    c["acc"] = np.minimum(pick([0, 0, 1000, 4287, MAXW]), c["cwnd"])
    c["in_rec"] = rng.random(nflows) < .4
    s = np.zeros(nflows, dtype=S)
    s["snd_una"] = pick([0, 5, 0x7FFFFFF0, 0xFFFFF000, 0xFFFFFFFF])
    flight = pick([0, 536, 2144, 8040, 100001, MAXW])
    s["snd_nxt"] = (s["snd_una"].astype(np.int64) + flight) & M32
    c["recover"] = (s["snd_una"].astype(np.int64) + pick([-5000, 0, 1000, 4288, 100001])) & M32
    s["nseg"] = rng.choice(queues, nflows)
    s["seg0"] = 1 + 2 * np.cumsum(np.concatenate([[0], (s["nseg"][:-1] + 3) // 2 + 1]))
    snd = np.zeros(nflows, dtype=SR)
    snd["n_new"] = pick([0, 0, 1, 3, 100, M32])
    snd["acked"] = pick([0, 1, 536, 1000, 4288, 8040, 100001, MAXW])
    snd["popped"] = np.where(rng.random(nflows) < .3, 0, pick([1, 63, 64, 200, 500, M32]))
    full =rng.random(nflows) < .2
    snd["popped"][full] = s["nseg"][full]
    snd["snd_una"], snd["n_dup"], snd["inflight"] = 77, 5, 9  # not read
    prev = np.zeros(nflows, dtype=RR)
    prev["fired"] = pick([0, 0, 1, 2])
    prev["backoff"] = pick([0, 1, 1, 2, 255])
    prev["sample"], prev["rto"] = 123, 1000  # not read
    t = lvlip.rto_flows(nflows)
    t["dead"] = rng.random(nflows) < .1
    t["wnd_cap"], t["srtt"], t["dupacks"] = 4242, 17, 2
    nfd = int(s["seg0"][-1] + s["nseg"][-1]) + 7
    fd = np.zeros(nfd, dtype=FD)
    fd["offset"] = rng.integers(0, 1 << 40, nfd)
    fd["len"] = rng.choice(np.array([0, 53, 54, 55, 590, 590, 1514, 65549], dtype=np.int64), nfd)
    sacked = rng.choice(np.array([0, 0, 0, 0, 1, 0xFF], dtype=np.uint8), nfd)
    return s, snd, prev, c, t, fd, sacked


def run_cpu(s, snd, prev, c, t, fd, sacked):
    """lvlip_cc_cpu on copies; asserts that what is only read keeps its bytes
    and that only wnd_cap of t changed.  Returns (c, t, res)."""
    ins = [None if a is None else a.copy() for a in (s, snd, prev, fd, sacked)]
    cc, tc = c.copy(), t.copy()
    res = lvlip.cc_cpu(s, snd, prev, cc, tc, fd, sacked)
    for a, b, name in zip((s, snd, prev, fd, sacked), ins, ("s", "snd", "prev", "fd", "sacked")):
        assert a is None or a.tobytes() == b.tobytes(), name + " is only read"
    back = tc.copy()
    back["wnd_cap"] = t["wnd_cap"]
    assert back.tobytes() == t.tobytes(), "of t, only wnd_cap is written"
    return cc, tc, res


def test_cpu_form_equals_the_model_in_every_branch():
    case = random_case(2000, 7)
    s, snd, prev, c, t, fd, sacked = case
    lvlip.cc_check(c)
    cc, tc, res = run_cpu(*case)
    mc, mcap, mres = model(*case)
    assert cc.tobytes() == mc.tobytes() and tc["wnd_cap"].tobytes() == mcap.tobytes() and res.tobytes() == mres.tobytes()
    live = t["dead"] == 0
    seen = set(res["event"][live].tolist())
    for bit in (EV_TIMEOUT, EV_ENTER, EV_EXIT, EV_SLOWSTART, EV_AVOID):
        assert any(e & bit for e in seen), bit
    assert {EV_TIMEOUT | EV_SLOWSTART, EV_ENTER | EV_EXIT, 0} <= seen  # two steps in one call, and none
    dead = ~live
    assert dead.any() and cc[dead].tobytes() == c[dead].tobytes() and (tc["wnd_cap"][dead] == 4242).all()
    assert (res["cwnd"][dead] == c["cwnd"][dead]).all() and not res["event"][dead].any() and not res["n_sacked"][dead].any()
    # branches the events do not name: a partial ACK, a repeated timeout, FASTRTX inside recovery, every clamp
    part = live & (c["in_rec"] == 1) & (prev["fired"] == 0) & (snd["n_new"] > 0) & (snd["acked"] > 0) & (res["event"] == 0)
    under = part & (c["cwnd"] <= c["cwnd_max"])  # step 2's last line holds cwnd to the ceiling even then
    assert under.any() and cc[under].tobytes() == c[under].tobytes()
    assert (part & ~under).any() and (cc["cwnd"][part & ~under] == c["cwnd_max"][part & ~under]).all()
    again = live & (prev["fired"] == 1) & (prev["backoff"] != 1)
    assert again.any() and (cc["ssthresh"][again] == c["ssthresh"][again]).all()
    assert (live & (prev["fired"] == 2) & (c["in_rec"] == 1) & (res["event"] & EV_ENTER == 0)).any()
    grew = live & (res["event"] & (EV_SLOWSTART | EV_AVOID) != 0)
    assert (grew & (cc["cwnd"] == cc["cwnd_max"])).any() and (tc["wnd_cap"][live] == MAXW).any()
    assert (live & (snd["popped"] > s["nseg"]) & (s["nseg"] > 0)).any() and (res["n_sacked"] > 0).any()
    # with every optional argument NULL in turn
    for drop in (1, 2, 6):
        alt = list(case)
        alt[drop] = None
        if drop == 6:
            alt[5] = None
        got, want = run_cpu(*alt), model(*alt)
        assert got[0].tobytes() == want[0].tobytes() and got[1]["wnd_cap"].tobytes() == want[1].tobytes()
        assert got[2].tobytes() == want[2].tobytes()


# ---------------------------------------- scripted sessions, by hand, mss 536 --

def step(c, t, una=1000, flight=0, a=0, n_new=0, fired=0, bo=0):
    s, snd, prev = np.zeros(1, dtype=S), np.zeros(1, dtype=SR), np.zeros(1, dtype=RR)
    s["snd_una"], s["snd_nxt"] = una, (una + flight) & M32
    snd["acked"], snd["n_new"], prev["fired"], prev["backoff"] = a, n_new, fired, bo
    res = lvlip.cc_cpu(s, snd, prev, c, t)
    assert res["cwnd"][0] == c["cwnd"][0] == t["wnd_cap"][0] and res["n_sacked"][0] == 0
    return int(res["event"][0])


def test_slow_start_doubles_per_round_until_ssthresh():
    c, t = lvlip.cc_init(536), lvlip.rto_flows(1)
    assert c["cwnd"][0] == 2144
    c["ssthresh"] = 8576
    assert step(c, t, flight=2144, a=2144, n_new=4) == EV_SLOWSTART and c["cwnd"][0] == 4288
    assert step(c, t, flight=4288, a=4288, n_new=8) == EV_SLOWSTART and c["cwnd"][0] == 8576
    assert step(c, t, flight=8576, a=8576, n_new=16) == EV_AVOID and c["cwnd"][0] == 9112 and c["acc"][0] == 0
    # RFC 3465: one ACK for the whole flight grows the window by one mss, no ACK or no bytes by nothing
    c = lvlip.cc_init(536)
    assert step(c, t, flight=2144, a=2144, n_new=1) == EV_SLOWSTART and c["cwnd"][0] == 2680
    assert step(c, t, flight=2144, a=0, n_new=3) == 0 and step(c, t, flight=2144, a=500, n_new=0) == 0
    assert step(c, t, flight=2144, a=100, n_new=2) == EV_SLOWSTART and c["cwnd"][0] == 2780


def test_avoidance_adds_one_mss_per_cwnd_of_acknowledged_bytes_and_one_per_call():
    c, t = lvlip.cc_init(536), lvlip.rto_flows(1)
    c["cwnd"] = c["ssthresh"] = 8576
    assert step(c, t, a=4000, n_new=1) == 0 and (c["cwnd"][0], c["acc"][0]) == (8576, 4000)
    assert step(c, t, a=4000, n_new=1) == 0 and (c["cwnd"][0], c["acc"][0]) == (8576, 8000)
    assert step(c, t, a=4000, n_new=1) == EV_AVOID and (c["cwnd"][0], c["acc"][0]) == (9112, 3424)
    c["acc"] = 0
    assert step(c, t, a=30000, n_new=50) == EV_AVOID and (c["cwnd"][0], c["acc"][0]) == (9648, 9648)  # 20888, held
    assert step(c, t, a=1, n_new=1) == EV_AVOID and (c["cwnd"][0], c["acc"][0]) == (10184, 1)


def test_timeouts_fast_recovery_and_the_ceiling():
    c, t = lvlip.cc_init(536), lvlip.rto_flows(1)
    c["cwnd"], c["acc"] = 9000, 77
    assert step(c, t, flight=8040, fired=1, bo=1) == EV_TIMEOUT
    assert (c["ssthresh"][0], c["cwnd"][0], c["acc"][0], c["in_rec"][0], c["recover"][0]) == (4020, 536, 0, 0, 9040)
    assert step(c, t, flight=2000, fired=1, bo=2) == EV_TIMEOUT and (c["ssthresh"][0], c["cwnd"][0]) == (4020, 536)
    assert step(c, t, flight=536, fired=1, bo=1) == EV_TIMEOUT and c["ssthresh"][0] == 1072  # never below two segments
    # the third duplicate ACK: ssthresh and cwnd are half the flight, recover is snd_nxt
    c = lvlip.cc_init(536)
    c["cwnd"], c["acc"] = 9000, 77
    assert step(c, t, una=0xFFFFF000, flight=8040, fired=2, bo=0) == EV_ENTER
    recover = (0xFFFFF000 + 8040) & M32
    assert (c["ssthresh"][0], c["cwnd"][0], c["acc"][0], c["in_rec"][0], c["recover"][0]) == (4020, 4020, 0, 1, recover)
    keep = c.tobytes()
    assert step(c, t, una=0xFFFFF000, flight=8040, fired=2) == 0 and c.tobytes() == keep  # FASTRTX inside recovery
    assert step(c, t, una=0xFFFFF000, flight=8040, a=1000, n_new=2) == 0 and c.tobytes() == keep  # a partial ACK
    assert step(c, t, una=0xFFFFF000 + 1000, flight=9000, a=7039, n_new=9) == 0 and c.tobytes() == keep
    assert step(c, t, una=0xFFFFF000 + 1000, flight=9000, a=7040, n_new=9) == EV_EXIT  # reaches recover, across the wrap
    assert (c["cwnd"][0], c["in_rec"][0], c["acc"][0], c["ssthresh"][0]) == (4020, 0, 0, 4020)
    # a timeout inside recovery leaves it; entering and the full ACK in one call
    c["in_rec"] = 1
    assert step(c, t, flight=8040, fired=1, bo=1) == EV_TIMEOUT and c["in_rec"][0] == 0
    assert step(c, t, flight=8040, a=8040, n_new=1, fired=2) == EV_ENTER | EV_EXIT and c["cwnd"][0] == 4020
    # cwnd_max holds both kinds of growth
    c = lvlip.cc_init(536, 3000)
    assert step(c, t, a=2144, n_new=4) == EV_SLOWSTART and c["cwnd"][0] == 3000
    c["ssthresh"] = 3000
    assert step(c, t, a=3000, n_new=4) == EV_AVOID and (c["cwnd"][0], c["acc"][0]) == (3000, 0)


# ------------------------------------------------------------------ the pipe --

def pipe(nseg, seg0, popped, lens, marks, cwnd=2144, snd_none=False):
    c, t = lvlip.cc_init(536), lvlip.rto_flows(1)
    c["cwnd"] = cwnd
    s, snd = np.zeros(1, dtype=S), np.zeros(1, dtype=SR)
    s["seg0"], s["nseg"], snd["popped"] = seg0, nseg, popped
    fd = np.zeros(len(lens), dtype=FD)
    fd["len"] = lens
    sacked = None if marks is None else np.array(marks, dtype=np.uint8)
    cc, tc, res = run_cpu(s, None if snd_none else snd, None, c, t, fd, sacked)
    assert cc.tobytes() == c.tobytes() and res["cwnd"][0] == cwnd and res["event"][0] == 0
    return int(res["n_sacked"][0]), int(res["sacked_bytes"][0]), int(tc["wnd_cap"][0])


def test_pipe_counts_marked_unpopped_entries():
    lens = [590, 590, 53, 54, 55, 590, 1514, 0, 590, 590]
    marks = [9, 1, 1, 0xFF, 1, 0, 0xFF, 1, 0, 7]  # entries 0 and 9 lie outside the queue [1, 9)
    assert pipe(8, 1, 0, lens, marks) == (6, 536 + 0 + 0 + 1 + 1460 + 0, 2144 + 1997)
    assert pipe(8, 1, 2, lens, marks) == (4, 0 + 1 + 1460, 2144 + 1461)  # entries 1 and 2 are popped
    assert pipe(8, 1, 8, lens, marks) == (0, 0, 2144) and pipe(8, 1, 9, lens, marks) == (0, 0, 2144)
    assert pipe(8, 1, M32, lens, marks) == (0, 0, 2144)  # popped beyond the queue is clamped
    assert pipe(8, 1, 5, lens, marks, snd_none=True) == (6, 1997, 2144 + 1997)  # NULL snd: nothing popped
    assert pipe(8, 1, 0, lens, None) == (0, 0, 2144) and pipe(0, 1, 0, lens, marks) == (0, 0, 2144)
    # saturation: of the output, and of the sum itself
    assert pipe(8, 1, 0, lens, marks, cwnd=MAXW - 100) == (6, 1997, MAXW)
    assert pipe(3, 0, 0, [M32, M32, 600], [1, 1, 1]) == (3, MAXW, MAXW)


# ---------------------------------------------------------------- refusals --

def test_refusals_write_nothing():
    L = lvlip.lib()
    p = lambda a: a.ctypes.data  # noqa: E731
    n = 3
    s, snd, prev = np.zeros(n, dtype=S), np.zeros(n, dtype=SR), np.zeros(n, dtype=RR)
    s["nseg"], s["seg0"] = 2, [0, 2, 4]
    fd, sacked = np.zeros(6, dtype=FD), np.ones(6, dtype=np.uint8)
    fresh = lambda: (lvlip.cc_init(536, nflows=n), lvlip.rto_flows(n), np.full(16 * n, 0x5A, dtype=np.uint8).view(R))  # noqa: E731
    c, t, res = fresh()
    canary = res.tobytes()
    ok = [p(s), p(snd), p(prev), p(c), p(t), n, p(fd), p(sacked), p(res)]
    keep = (c.tobytes(), t.tobytes())

    def refused(fn, args):
        assert fn(*args) == lvlip.EINVAL, args
        assert (c.tobytes(), t.tobytes()) == keep and res.tobytes() == canary, "a refusal wrote"

    for i in (0, 3, 4, 8, 6):  # NULL s, c, t, res; NULL fd with a scoreboard
        bad = list(ok)
        bad[i] = None
        refused(L.lvlip_cc_cpu, bad)
        refused(L.lvlip_cc_dev, bad + [None])
    bad = list(ok)
    bad[5] = lvlip.LRO_MAX_FLOWS + 1
    refused(L.lvlip_cc_cpu, bad)
    refused(L.lvlip_cc_dev, bad + [None])
    for i, off in ((0, 4), (3, 4), (4, 4), (1, 8), (2, 8), (6, 8), (8, 8)):  # the device form's alignment, before any HIP call
        bad = list(ok) + [None]
        bad[i] += off
        refused(L.lvlip_cc_dev, bad)
    assert L.lvlip_cc_cpu(*[None] * 5, 0, None, None, None) == lvlip.OK  # nflows == 0
    assert L.lvlip_cc_dev(*[None] * 5, 0, None, None, None, None) == lvlip.OK
    assert L.lvlip_cc_check(None, 0) == lvlip.OK and L.lvlip_cc_check(None, 1) == lvlip.EINVAL
    assert L.lvlip_cc_check(p(c), lvlip.LRO_MAX_FLOWS + 1) == lvlip.EINVAL
    # every state the check names, in the last flow: the check, the wrapper and the call
    states = (("mss", 0), ("mss", 65496), ("cwnd", 535), ("cwnd", MAXW + 1), ("cwnd_max", 535), ("cwnd_max", MAXW + 1),
              ("ssthresh", MAXW + 1), ("in_rec", 2), ("reserved", 1), ("reserved2", (1, 0)), ("reserved2", (0, 1)))
    for field, v in states:
        c, t, res = fresh()
        c[field][n - 1] = v
        keep = (c.tobytes(), t.tobytes())
        assert L.lvlip_cc_check(p(c), n) == lvlip.EINVAL and L.lvlip_cc_check(p(c), n - 1) == lvlip.OK, field
        with pytest.raises(ValueError):
            lvlip.cc_check(c)
        refused(L.lvlip_cc_cpu, [p(s), p(snd), p(prev), p(c), p(t), n, p(fd), p(sacked), p(res)])
    # the limits themselves pass
    c, t, res = fresh()
    c["mss"], c["cwnd"], c["cwnd_max"], c["ssthresh"] = [1, 65495, 536], [1, MAXW, 536], [MAXW, MAXW, 536], [0, MAXW, 5]
    lvlip.cc_check(c)
    with pytest.raises(ValueError):
        lvlip.cc_cpu(s, snd, prev, lvlip.cc_init(536, nflows=2), t)
    with pytest.raises(ValueError):
        lvlip.cc_cpu(s, snd, prev, c, t, fd[:5], sacked)
    with pytest.raises(TypeError):
        lvlip.cc_cpu(s, snd, prev, c, t, None, sacked)


# ------------------------------------------------------------- the whole loop --

IW = 2144  # lvlip.cc_init(536)


class CcLoop:
    """tests/test_rto_cpu.py's RtoLoop.run_cpu(gated=True) with lvlip_cc_cpu in
    every round, after lvlip_sack_cpu and before lvlip_wnd_cpu.  A flow's first
    push runs before the first call, so w.wnd starts at the initial window."""

    def __init__(self):
        self.rto = RtoLoop()
        self.p = self.rto.p

    def run_cpu(self, rounds=None):
        p = self.p
        b, n = p.base, p.n
        L = b.link
        fb, fa, snd, w, tmpl = b.fb.copy(), L.fa.copy(), p.snd.copy(), p.w.copy(), L.tmpl.copy()
        ring = np.full(p.ring_bytes, 0x5A, dtype=np.uint8)
        fd, sacked = np.zeros(p.nfd, dtype=FD), np.zeros(p.nfd, dtype=np.uint8)
        stream = np.full(L.stream.size, 0x5A, dtype=np.uint8)
        res = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
        sres = np.zeros(n, dtype=SR)
        sent = np.zeros(n * p.segs, dtype=np.int32)
        c = lvlip.cc_init(p.mss, nflows=n)
        t = lvlip.rto_flows(n, snd_wnd=b.wnd, wnd_cap=IW)
        w["wnd"] = min(b.wnd, IW)
        resent, now, done, cres, flight, caps = 0, 0, 0, [], [], []
        while rounds is None or done < rounds:
            now += TICK
            caps.append(t["wnd_cap"].copy())
            pfd, pres = lvlip.push_cpu(fa, None, snd, w, L.payload, ring, fd, sacked)
            flight.append((snd["snd_nxt"] - snd["snd_una"]).astype(np.int64) & M32)
            gate, rres = lvlip.rto_cpu(snd, sres, pres, t, now, lvlip.RTO_FAST, sacked)
            fd_out, _ = lvlip.rtx_sack_cpu(fa, None, snd, gate, sacked, ring, fd)
            resent += int((fd_out["len"] > 0).sum())
            wire = self.rto.wire(pfd, fd_out, ring, sent)
            _, rec = lvlip.lro_cpu(ring, wire, fb, lvlip.RX_VERIFY_L4, out=stream)
            lvlip.lro_advance_carry(fb, rec, res, res)
            wnd = np.minimum(b.wnd, b.end - fb["out_off"] - res["delivered"]).astype(np.uint32)
            tmpl["hdr"][:, 48], tmpl["hdr"][:, 49] = wnd >> 8, wnd & 0xFF
            ack, afd = lvlip.ack_cpu(tmpl, fb, res, lvlip.ACK_ALL, out=np.full(L.ack_bytes, 0x5A, dtype=np.uint8))
            lvlip.lro_next_cpu(fb, res)
            fb["rcv_wnd"] = wnd
            _, arec = lvlip.lro_cpu(ack, afd, fa, lvlip.RX_VERIFY_L4, out=np.zeros(n + 64, dtype=np.uint8))
            sres = lvlip.snd_cpu(fa, snd, arec, ring, fd)
            lvlip.sack_cpu(fa, snd, arec, ack, afd, ring, fd, sacked)
            cres.append(lvlip.cc_cpu(snd, sres, rres, c, t, fd, sacked))
            wres = lvlip.wnd_cpu(fa, snd, t, w, arec, ack, afd, lvlip.WND_APPLY)
            lvlip.snd_next_cpu(snd, sres)
            done += 1
            if rounds is None and not snd["nseg"].any() and not w["unsent"].any():
                break
            assert done < 2000, "the loop does not end"
        return dict(stream=stream, fb=fb, snd=snd, w=w, res=res, sres=sres, ring=ring, fd=fd, sacked=sacked, sent=sent,
                    t=t, c=c, wres=wres, rres=rres, gate=gate, resent=resent, rounds=done, cres=np.stack(cres),
                    flight=np.stack(flight), caps=np.stack(caps))


# What the CPU loop takes with the call in every round (the gated loop of tests/test_rto_cpu.py takes 19 without
# it): measured, and the device loop's round count too (tests/test_cc_gpu.py).
CC_ROUNDS = 20


@functools.lru_cache(maxsize=None)
def cc_loop_cpu():
    loop = CcLoop()
    return loop, loop.run_cpu()


def test_the_loop_with_a_congestion_window_on_the_cpu_forms():
    loop, got = cc_loop_cpu()
    loop.rto.check_done(got)
    assert got["rounds"] == CC_ROUNDS
    assert (got["flight"] <= got["caps"]).all(), "a flow ran past its round's wnd_cap"
    assert (got["flight"][0] <= IW).all() and (got["flight"][0] > 0).all()
    ev = np.bitwise_or.reduce(got["cres"]["event"].reshape(-1))
    assert ev & EV_SLOWSTART and ev & (EV_TIMEOUT | EV_ENTER), hex(ev)
    assert (got["cres"]["cwnd"] >= loop.p.mss).all() and got["cres"]["n_sacked"].any()
    lvlip.cc_check(got["c"])


# ------------------------------------------------------ example and sanitizers --

C_SRCS = ("cc_cpu.c", "rto_cpu.c", "push_cpu.c", "sack_cpu.c", "snd_cpu.c", "ack_cpu.c", "rcv_cpu.c", "seg_cpu.c",
          "csum_cpu.c")


def test_example_runs_to_its_own_check():
    exe = os.path.join(ROOT, "examples", "build", "cc_loop")
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("cc_loop ok"), r.stdout + r.stderr
    assert "with lvlip_cc_cpu" in r.stdout and "without lvlip_cc_cpu" in r.stdout


def _sanitized(tmp_path, main_c, exe_name):
    """tests/test_rto_cpu.py's recipe: a stand-alone program from the *_cpu.c
    sources under ASan + UBSan; nothing is loaded into Python."""
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
    assert "cc_loop ok" in _sanitized(tmp_path, os.path.join(ROOT, "examples", "cc_loop.c"), "cc_loop_san")


def test_hostile_state_and_descriptors_under_sanitizers(tmp_path):
    """tests/sanitize/cc_hostile.c, a stand-alone main: lvlip_cc_cpu on extreme
    state, popped beyond the queue, descriptors shorter than a header and of
    2^32 - 1 bytes, a recover behind snd_una, every array malloc'd at exactly
    its size, under ASan + UBSan."""
    assert "cc_hostile ok" in _sanitized(tmp_path, os.path.join(ROOT, "tests", "sanitize", "cc_hostile.c"),
                                         "cc_hostile_san")
