"""lvlip_rbuf_plan / _check / _cpu (include/lvlip_skb.h, "f1: the
receive buffer") without a GPU: the CPU form against tests/rbuf_model.py's
plain restatement, byte for byte, over random cases that take every branch;
every refusal and every broken invariant; the reference's own stream
(tests/golden/lro_ref.json) read through the call in chunks; and the loop,
tests/test_rto_cpu.py's transfer into receive buffers of 8 segments with an
application that reads a scripted amount each round, which stalls at `cap`
bytes when the call is left out."""
import functools

import numpy as np
import pytest

import lvlip
from rbuf_model import ALL_BRANCHES, M32, branches, model, random_case
from test_rto_cpu import TICK, RtoLoop

P, R = lvlip.RBUF_FLOW_DTYPE, lvlip.RBUF_RESULT_DTYPE
CASES = [(n, seed) for n in (1, 7, 33) for seed in (0, 1, 2)]


def test_layout_and_symbols():
    assert P.itemsize == 48 and P.itemsize % 16 == 0 and R.itemsize == 32
    assert [P.fields[k][1] for k in ("base_off", "sink_off", "cap", "head", "adv_edge", "piece0", "mss", "wscale",
                                     "reserved")] == [0, 8, 16, 20, 24, 28, 32, 34, 35]
    for name in ("lvlip_rbuf_plan", "lvlip_rbuf_check", "lvlip_rbuf_cpu"):
        assert hasattr(lvlip.lib(), name)


def run_cpu(f, res, p, t, nread, out, sink):
    f, p, t, out = f.copy(), p.copy(), t.copy(), out.copy()
    sink = None if sink is None else sink.copy()
    gate, rres = lvlip.rbuf_cpu(f, res, p, t, nread, out, sink)
    return f, p, t, gate, rres, out, sink


def same(got, want):
    for name, a, b in zip(("f", "p", "t", "gate", "rres", "out", "sink"), got, want):
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), name


# ------------------------------------------------------------------ the model --

def test_cpu_equals_the_model_and_every_branch_is_taken():
    seen = set()
    for n, seed in CASES:
        case = random_case(n, seed, max_cap=80000 if seed == 2 else 3000, shift=seed)
        res0 = case[1].copy()
        got = run_cpu(*case)
        same(got, model(*case))
        assert case[1].tobytes() == res0.tobytes(), "res is only read"
        lvlip.rbuf_check(got[1], got[0])  # every call leaves a state the check takes
        seen |= branches(got[4], case[1], case[4])
    assert seen == ALL_BRANCHES, ALL_BRANCHES - seen


def test_no_sink_and_no_reads():
    f, res, p, t, nread, out, sink = random_case(33, 5)
    same(run_cpu(f, res, p, t, nread, out, None), model(f, res, p, t, nread, out, None))
    got = run_cpu(f, res, p, t, None, out, sink)
    same(got, model(f, res, p, t, None, out, sink))
    assert not got[4]["read"].any() and got[6].tobytes() == sink.tobytes()


def test_touching_ranges_and_the_first_flow_that_stays():
    """live == head: the move's source starts where its destination ends;
    live == head + 1 does not move."""
    f, res, p, t, nread, out, sink = random_case(2, 3)  # rebuilt: 100 read bytes and 100 / 101 unread ones
    at = 5
    for k, unread in ((0, 100), (1, 101)):
        p["base_off"][k], p["cap"][k], p["head"][k] = at, 400, 100
        f["out_off"][k], f["rcv_wnd"][k] = at + 100 + unread, 400 - 100 - unread
        p["adv_edge"][k] = (int(f["rcv_nxt"][k]) + int(f["rcv_wnd"][k])) & M32
        at += 400
    res["nsack"], nread[:] = 0, 0
    out = np.arange(at + 64, dtype=np.uint32).astype(np.uint8)
    lvlip.rbuf_plan(p, f)
    got = run_cpu(f, res, p, t, nread, out, sink)
    same(got, model(f, res, p, t, nread, out, sink))
    assert got[4]["flags"][0] & lvlip.RBUF_MOVED and got[4]["moved"][0] == 100
    assert not got[4]["flags"][1] & lvlip.RBUF_MOVED and got[4]["head"][1] == 100
    assert got[5][5:105].tobytes() == out[105:205].tobytes() and got[5][105:].tobytes() == out[105:].tobytes()


# ------------------------------------------------------- refusals and the check --

def fresh(n=3, cap=1000):
    f = np.zeros(n, dtype=lvlip.LRO_FLOW_DTYPE)
    f["sport"], f["rcv_nxt"], f["rcv_wnd"], f["out_off"] = np.arange(n), 1000, cap, np.arange(n) * cap
    p = lvlip.rbuf_flows(f, 536)
    assert lvlip.rbuf_plan(p, f) == n * -(-cap // lvlip.RBUF_PIECE)
    return f, p


def test_a_fresh_flow_and_the_plans_pieces():
    f, p = fresh(3, 40000)
    assert p["piece0"].tolist() == [0, 3, 6] and (p["head"] == 0).all()
    assert (p["adv_edge"] == 41000).all() and (p["base_off"] == f["out_off"]).all() and (p["cap"] == 40000).all()
    lvlip.rbuf_check(p, f)
    assert lvlip.lib().lvlip_rbuf_plan(None, None, 0, None) == 0
    assert lvlip.lib().lvlip_rbuf_check(None, None, 0) == lvlip.OK


BROKEN = {
    "base_off beyond out_off": lambda f, p: p["base_off"].__setitem__(1, 1001),
    "region does not end with the buffer": lambda f, p: f["rcv_wnd"].__setitem__(1, 999),
    "head beyond used": lambda f, p: p["head"].__setitem__(1, 1),
    "cap 0": lambda f, p: (p["cap"].__setitem__(1, 0), f["rcv_wnd"].__setitem__(1, 0)),
    "cap above 2^30": lambda f, p: (p["cap"].__setitem__(2, (1 << 30) + 1), f["rcv_wnd"].__setitem__(2, (1 << 30) + 1)),
    "mss 0": lambda f, p: p["mss"].__setitem__(0, 0),
    "wscale 15": lambda f, p: p["wscale"].__setitem__(0, 15),
    "reserved": lambda f, p: p["reserved"][2].__setitem__(12, 1),
    "overlapping buffers": lambda f, p: (p["base_off"].__setitem__(1, 999), f["out_off"].__setitem__(1, 999)),
    "base_off + cap wraps": lambda f, p: (p["base_off"].__setitem__(2, (1 << 64) - 10),
                                          f["out_off"].__setitem__(2, (1 << 64) - 10)),
}


@pytest.mark.parametrize("what", sorted(BROKEN))
def test_each_broken_invariant_is_refused(what):
    f, p = fresh()
    BROKEN[what](f, p)
    f0, p0 = f.copy(), p.copy()
    with pytest.raises(ValueError):
        lvlip.rbuf_plan(p, f)
    with pytest.raises(ValueError):
        lvlip.rbuf_check(p, f)
    res, t = np.zeros(3, dtype=lvlip.LRO_RESULT_DTYPE), np.zeros(3, dtype=lvlip.ACK_TMPL_DTYPE)
    out = np.zeros(4000, dtype=np.uint8)
    with pytest.raises(lvlip.LvlipError) as e:
        lvlip.rbuf_cpu(f, res, p, t, None, out, None)
    assert e.value.rc == lvlip.EINVAL
    assert f.tobytes() == f0.tobytes() and p.tobytes() == p0.tobytes() and not out.any() and not t.view(np.uint8).any()


def test_the_check_wants_the_plans_piece0_and_the_plan_writes_nothing_when_it_refuses():
    f, p = fresh(3, 40000)
    p["piece0"][2] = 5
    with pytest.raises(ValueError):
        lvlip.rbuf_check(p, f)
    assert lvlip.rbuf_plan(p, f) == 9 and p["piece0"][2] == 6
    p["piece0"], p["mss"][2] = 77, 0
    with pytest.raises(ValueError):
        lvlip.rbuf_plan(p, f)
    assert (p["piece0"] == 77).all()
    # more than 2^31 pieces
    n = 40000
    f = np.zeros(n, dtype=lvlip.LRO_FLOW_DTYPE)
    f["rcv_wnd"], f["out_off"] = 1 << 30, np.arange(n, dtype=np.uint64) << 30
    with pytest.raises(ValueError):
        lvlip.rbuf_plan(lvlip.rbuf_flows(f, 536), f)


def test_refusals_and_noops():
    L = lvlip.lib()
    f, p = fresh()
    res, gate = np.zeros(3, dtype=lvlip.LRO_RESULT_DTYPE), np.zeros(3, dtype=lvlip.LRO_RESULT_DTYPE)
    t, rres = np.zeros(3, dtype=lvlip.ACK_TMPL_DTYPE), np.full(3, 7, dtype="<u4").repeat(8).view(R)
    out = np.zeros(4000, dtype=np.uint8)
    arrays = (f, res, p, t, out, gate, rres)
    before = [a.tobytes() for a in arrays]
    q = lambda a: a.ctypes.data  # noqa: E731
    ok = [q(f), q(res), q(p), q(t), 3, None, q(out), None, q(gate), q(rres)]
    for i in (0, 1, 2, 3, 6, 8, 9):
        bad = list(ok)
        bad[i] = None
        assert L.lvlip_rbuf_cpu(*bad) == lvlip.EINVAL, i
    bad = list(ok)
    bad[8] = q(res)
    assert L.lvlip_rbuf_cpu(*bad) == lvlip.EINVAL, "gate == res"
    bad = list(ok)
    bad[4] = lvlip.LRO_MAX_FLOWS + 1
    assert L.lvlip_rbuf_cpu(*bad) == lvlip.EINVAL
    assert L.lvlip_rbuf_check(None, q(f), 3) == lvlip.EINVAL and L.lvlip_rbuf_check(q(p), None, 3) == lvlip.EINVAL
    assert L.lvlip_rbuf_check(q(p), q(f), lvlip.LRO_MAX_FLOWS + 1) == lvlip.EINVAL
    assert L.lvlip_rbuf_plan(None, q(f), 3, None) == 0xFFFFFFFF
    assert L.lvlip_rbuf_plan(q(p), q(f), lvlip.LRO_MAX_FLOWS + 1, None) == 0xFFFFFFFF
    assert L.lvlip_rbuf_cpu(None, None, None, None, 0, None, None, None, None, None) == lvlip.OK
    assert [a.tobytes() for a in arrays] == before, "a refusal writes nothing"


# ------------------------------------------------- reading the reference's stream --

@pytest.mark.parametrize("chunk", (1, 100, 1 << 20))
def test_sink_holds_what_the_references_tcp_data_dequeue_returned(chunk):
    """The frames the unmodified stack received go through lvlip_lro_cpu ->
    advance -> next -> lvlip_rbuf_cpu with a sink; the fixture records the
    bytes of all its tcp_data_dequeue calls as one string, so the sink's bytes
    are compared with their concatenation."""
    from test_lro_cpu import fixture_inputs

    fx, buf, fd, flow = fixture_inputs()
    want = bytes.fromhex(fx["dequeued_hex"])
    out, rec = lvlip.lro_cpu(buf, fd, flow, lvlip.RX_VERIFY_L4)
    res = lvlip.lro_advance(flow, rec)
    p = lvlip.rbuf_flows(flow, fx["seg"], sink_off=5)
    lvlip.rbuf_plan(p, flow)
    lvlip.lro_next_cpu(flow, res)
    t = np.zeros(1, dtype=lvlip.ACK_TMPL_DTYPE)
    sink = np.full(len(want) + 64, 0xA5, dtype=np.uint8)
    got = 0
    for _ in range(len(want) // chunk + 2):
        _, rres = lvlip.rbuf_cpu(flow, res, p, t, np.array([chunk], dtype=np.uint32), out, sink)
        got += int(rres["read"][0])
    assert got == len(want) == fx["count"] and int(p["sink_off"][0]) == 5 + got
    assert sink[5:5 + got].tobytes() == want and (sink[:5] == 0xA5).all() and (sink[5 + got:] == 0xA5).all()


# ------------------------------------------------------------- the whole loop --

class RbufLoop:
    """tests/test_rto_cpu.py's RtoLoop (8 flows x 40 x 536 B, every fifth first
    transmission lost) into receive buffers of cap = 8 x 536 bytes at odd
    offsets of a small `out`, read by an application that takes a scripted
    0 .. cap bytes per flow and round into a sink.  The window in B's ACKs is
    what lvlip_rbuf_* writes; ACKs are built without LVLIP_ACK_ALL from its
    gate.  with_call False leaves the call out: the template keeps the window
    the host wrote and nothing empties the buffers."""

    MAX_ROUNDS = 400

    def __init__(self):
        self.rto = RtoLoop()
        p = self.rto.p
        b = p.base
        self.n, self.cap, self.total = p.n, b.wnd, p.segs * p.mss
        assert self.cap == 8 * 536
        self.fb = b.fb.copy()
        self.fb["out_off"] = 7 + np.arange(self.n) * (self.cap + 5)
        self.fb["rcv_wnd"] = self.cap
        self.out_bytes = int(self.fb["out_off"][-1]) + self.cap + 9
        self.irs = self.fb["rcv_nxt"].copy()
        self.rb = lvlip.rbuf_flows(self.fb, p.mss, sink_off=np.arange(self.n) * self.total)
        lvlip.rbuf_plan(self.rb, self.fb)
        rng = np.random.default_rng(11)
        self.nread = rng.integers(0, self.cap + 1, (self.MAX_ROUNDS, self.n)).astype(np.uint32)
        self.nread[rng.random((self.MAX_ROUNDS, self.n)) < 0.3] = 0
        self.nread[5:9] = 0  # the application is away for a few rounds: the buffers fill

    def run_cpu(self, with_call: bool = True, rounds=None):
        R_, p = self.rto, self.rto.p
        b, n = p.base, p.n
        L = b.link
        fb, fa, snd, w, tmpl, rb = self.fb.copy(), L.fa.copy(), p.snd.copy(), p.w.copy(), L.tmpl.copy(), self.rb.copy()
        tmpl["hdr"][:, 48], tmpl["hdr"][:, 49] = self.cap >> 8, self.cap & 0xFF
        ring = np.full(p.ring_bytes, 0x5A, dtype=np.uint8)
        fd, sacked = np.zeros(p.nfd, dtype=lvlip.FRAME_DESC_DTYPE), np.zeros(p.nfd, dtype=np.uint8)
        out = np.full(self.out_bytes, 0x5A, dtype=np.uint8)
        sink = np.full(n * self.total, 0x5A, dtype=np.uint8)
        res = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
        sres = np.zeros(n, dtype=lvlip.SND_RESULT_DTYPE)
        sent = np.zeros(n * p.segs, dtype=np.int32)
        t = lvlip.rto_flows(n, snd_wnd=self.cap)
        w["wnd"] = self.cap
        log, edges, now, done = [], [], 0, 0
        while True:
            now += TICK
            pfd, pres = lvlip.push_cpu(fa, None, snd, w, L.payload, ring, fd, sacked)
            gate_a, rres_a = lvlip.rto_cpu(snd, sres, pres, t, now, lvlip.RTO_FAST, sacked)
            fd_out, _ = lvlip.rtx_sack_cpu(fa, None, snd, gate_a, sacked, ring, fd)
            wire = R_.wire(pfd, fd_out, ring, sent)
            _, rec = lvlip.lro_cpu(ring, wire, fb, lvlip.RX_VERIFY_L4, out=out)
            lvlip.lro_advance_carry(fb, rec, res, res)
            lvlip.lro_next_cpu(fb, res)
            if with_call:
                gate, rr = lvlip.rbuf_cpu(fb, res, rb, tmpl, self.nread[done], out, sink)
                log.append(rr)
                edges.append(rb["adv_edge"].copy())
            else:
                gate = res
            ack, afd = lvlip.ack_cpu(tmpl, fb, gate, 0, out=np.full(L.ack_bytes, 0x5A, dtype=np.uint8))
            _, arec = lvlip.lro_cpu(ack, afd, fa, lvlip.RX_VERIFY_L4, out=np.zeros(n + 64, dtype=np.uint8))
            sres = lvlip.snd_cpu(fa, snd, arec, ring, fd)
            lvlip.sack_cpu(fa, snd, arec, ack, afd, ring, fd, sacked)
            lvlip.wnd_cpu(fa, snd, t, w, arec, ack, afd, lvlip.WND_APPLY)
            lvlip.snd_next_cpu(snd, sres)
            done += 1
            if rounds is not None:
                if done == rounds:
                    break
            elif not snd["nseg"].any() and not w["unsent"].any() and not (fb["out_off"] - rb["base_off"] - rb["head"]).any():
                break
            assert done < self.MAX_ROUNDS, "the loop does not end"
        return dict(out=out, sink=sink, fb=fb, rb=rb, tmpl=tmpl, snd=snd, w=w, res=res, t=t, sent=sent, rounds=done,
                    log=np.array(log).view(R).reshape(-1, n) if log else None, edges=np.array(edges), gate=gate)


@functools.lru_cache(maxsize=None)
def rbuf_loop_cpu():
    loop = RbufLoop()
    return loop, loop.run_cpu(True)


def test_the_loop_delivers_every_byte_through_buffers_of_eight_segments():
    loop, got = rbuf_loop_cpu()
    L = loop.rto.p.base.link
    assert loop.total > 4 * loop.cap
    assert np.array_equal(got["sink"], L.payload), "the sink is not the payloads, in order"
    assert ((got["fb"]["rcv_nxt"].astype(np.int64) - loop.irs) & M32 == loop.total).all()
    assert (got["rb"]["sink_off"] == (np.arange(loop.n) + 1) * loop.total).all()
    assert not got["t"]["dead"].any()
    # no flow's advertised right edge ever moves left
    e = got["edges"].astype(np.int64)
    assert (((e[1:] - e[:-1]) & M32) < (1 << 31)).all()
    log = got["log"]
    assert ((log["flags"] & lvlip.RBUF_MOVED) != 0).any(axis=0).all(), "every flow reuses its buffer"
    assert ((log["flags"] & lvlip.RBUF_UPDATE) != 0).any(axis=0).all(), "every flow owes a window update once"
    assert (log["moved"].sum(axis=0) <= log["read"].sum(axis=0)).all(), "at most one more copy per stream byte"
    assert (log["read"].sum(axis=0) == loop.total).all()
    lvlip.rbuf_check(got["rb"], got["fb"])


def test_without_the_call_the_flows_stop_at_cap_bytes():
    loop, want = rbuf_loop_cpu()
    stalled = loop.run_cpu(False, rounds=want["rounds"])
    after = loop.run_cpu(False, rounds=want["rounds"] + 50)
    for got in (stalled, after):
        assert ((got["fb"]["rcv_nxt"].astype(np.int64) - loop.irs) & M32 == loop.cap).all()
        assert not got["fb"]["rcv_wnd"].any()
    assert after["fb"].tobytes() == stalled["fb"].tobytes(), "50 further rounds change nothing"
