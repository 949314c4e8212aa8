"""The zero-window persist timer on the calling thread (persist_cpu.c,
include/lvlip_skb.h "the persist timer"): lvlip_persist_cpu against a plain
restatement of its steps and of the probe frame (tests/persist_model.py, which
never calls the library), the doubling and its ceiling, the clock's wrap, the
probe as the peer's receive path sees it, the one store into the
retransmission timer and why it is there, the refusals, and the loop of
tests/test_rto_cpu.py with a receiver that stops reading and a lost window
update: it hangs without the call and ends with it.  The reference has no
persist timer, so there is no golden file."""
import functools
import os
import subprocess

import numpy as np
import pytest

import lvlip
import pyoracle
from persist_model import BRANCHES, CANARY, M32, make_sides, model_probe, model_run, random_case
from tcp_model import lost_carry_seed
from test_rto_cpu import TICK, RtoLoop  # imported, never edited

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R, FD = lvlip.PERSIST_FLOW_DTYPE, lvlip.PERSIST_RESULT_DTYPE, lvlip.FRAME_DESC_DTYPE


def test_layout_and_symbols():
    assert P.itemsize == 16 and [P.fields[k][1] for k in ("expires", "interval", "probes", "armed", "reserved")] == \
        [0, 4, 8, 12, 13]
    assert R.itemsize == 16 and [R.fields[k][1] for k in ("fired", "interval", "probes", "seq")] == [0, 4, 8, 12]
    assert (lvlip.PERSIST_MAX_MS, lvlip.PERSIST_SLOT) == (60000, 64)
    for name in ("lvlip_persist_check", "lvlip_persist_cpu", "lvlip_persist_dev"):
        assert hasattr(lvlip.lib(), name)
    src = open(os.path.join(ROOT, "level-ip_amd", "BUILD_SOURCES")).read()
    assert "csrc/persist_cpu.c" in src and "csrc/persist_kernels.hip" in src
    assert len(lvlip.SIGNATURES["lvlip_persist_cpu"][1]) == 11 and len(lvlip.SIGNATURES["lvlip_persist_dev"][1]) == 12


def run_cpu(f, lro, s, w, t, p, now, out=None):
    """The call on copies, from a buffer of canary bytes: (t', p', out, fd_out, res)."""
    t, p = t.copy(), p.copy()
    out = np.full(64 * s.size + 7, CANARY, dtype=np.uint8) if out is None else out.copy()
    out, fd, res = lvlip.persist_cpu(f, lro, s, w, t, p, now, out)
    return t, p, out, fd, res


def one(p=None, t=None, nseg=0, unsent=5000, wnd=0, mss=536, now=1000, una=None):
    """One flow through the call; returns (t', p', out, fd, res)."""
    f, s, w, _ = make_sides(1)
    s["nseg"], w["unsent"], w["wnd"], w["mss"] = nseg, unsent, wnd, mss
    if una is not None:
        s["snd_una"] = s["snd_nxt"] = una
    return run_cpu(f, None, s, w, lvlip.rto_flows(1) if t is None else t, lvlip.persist_flows(1) if p is None else p, now)


def armed(expires, interval=1000, probes=0):
    p = lvlip.persist_flows(1)
    p["armed"], p["expires"], p["interval"], p["probes"] = 1, expires, interval, probes
    return p


# ------------------------------------------------------------ against the model --

def test_cpu_equals_the_model_on_every_branch():
    seen, wnds, short, nsegs = set(), set(), 0, set()
    for seed in range(12):
        f, lro, s, w, t, p, now = random_case(97, seed)
        out0 = np.full(64 * 97 + 7, CANARY, dtype=np.uint8)
        want = model_run(f, lro, s, w, t, p, now, out0)
        got = run_cpu(f, lro, s, w, t, p, now, out0)
        for name, a, b in zip(("t", "p", "out", "fd_out", "res"), got, want):
            assert a.tobytes() == b.tobytes(), (seed, name)
        seen |= set(want[5])
        for k in range(97):
            mss, wnd, unsent = int(w["mss"][k]), int(w["wnd"][k]), int(w["unsent"][k])
            wnds |= {name for name, v in (("0", 0), ("1", 1), ("mss-1", mss - 1), ("mss", mss)) if wnd == v and mss > 2}
            short += 0 < unsent < mss and wnd < unsent and want[5][k] in ("arm", "wait", "fire")
        nsegs |= set(s["nseg"].tolist())
    assert seen == set(BRANCHES), seen
    assert wnds == {"0", "1", "mss-1", "mss"} and short > 0 and nsegs == {0, 1}
    # lro == NULL: delivered counts as 0
    f, lro, s, w, t, p, now = random_case(33, 99)
    want = model_run(f, None, s, w, t, p, now, np.full(64 * 33 + 7, CANARY, dtype=np.uint8))
    got = run_cpu(f, None, s, w, t, p, now)
    assert got[2].tobytes() == want[2].tobytes() and want[4]["fired"].any()


def test_the_stalled_test_at_its_edges():
    for nseg, unsent, wnd, mss, stalled in ((0, 5000, 0, 536, 1), (0, 5000, 1, 536, 1), (0, 5000, 535, 536, 1),
                                            (0, 5000, 536, 536, 0), (0, 100, 99, 536, 1), (0, 100, 100, 536, 0),
                                            (0, 0, 0, 536, 0), (1, 5000, 0, 536, 0), (0, 1, 0, 1, 1)):
        _, p, _, fd, res = one(nseg=nseg, unsent=unsent, wnd=wnd, mss=mss)
        assert int(p["armed"][0]) == stalled and int(res["interval"][0]) == (1000 if stalled else 0)
        assert res["fired"][0] == 0 and fd["len"][0] == 0


def test_doubling_stops_at_the_ceiling_and_arming_never_fires():
    t = lvlip.rto_flows(1, rto=1000)
    now = 5000
    _, p, out, fd, res = one(t=t, now=now)
    assert list(res[0].tolist()) == [0, 1000, 0, 0] and (p["armed"][0], p["expires"][0]) == (1, 6000)
    assert (out == CANARY).all() and fd["len"][0] == 0, "arming sends nothing"
    seen = []
    for i in range(9):
        now = int(p["expires"][0])
        assert one(t=t, p=p, now=now)[4]["fired"][0] == 0, "the test is strict"
        before, now = now, now + 1
        _, p, _, fd, res = one(t=t, p=p, now=now)
        assert res["fired"][0] == 1 and res["probes"][0] == p["probes"][0] == i + 1 and fd["len"][0] == 54
        assert int(p["expires"][0]) == now + int(p["interval"][0]) and before < now
        seen.append(int(res["interval"][0]))
    assert seen == [2000, 4000, 8000, 16000, 32000, 60000, 60000, 60000, 60000]
    # the intervals the probes were sent after: 1000, 2000, .. 32000, 60000, 60000
    assert [1000] + seen[:-1] == [1000, 2000, 4000, 8000, 16000, 32000, 60000, 60000, 60000]
    # an expired timer of an unarmed flow: the call arms and does not fire
    stale = lvlip.persist_flows(1)
    stale["expires"] = 1
    _, p, _, fd, res = one(p=stale, now=5000)
    assert res["fired"][0] == 0 and p["armed"][0] == 1 and fd["len"][0] == 0


@pytest.mark.parametrize("rto, interval", ((0, 1), (1, 1), (999, 999), (60000, 60000), (60001, 60000),
                                           (120000, 60000), (M32, 60000)))
def test_interval_at_arming(rto, interval):
    _, p, _, _, res = one(t=lvlip.rto_flows(1, rto=rto), now=77)
    assert (int(p["interval"][0]), int(p["expires"][0]), int(res["interval"][0])) == (interval, 77 + interval, interval)


def test_probes_saturate():
    _, p, _, _, res = one(p=armed(10, probes=M32 - 1), now=11)
    assert res["probes"][0] == p["probes"][0] == M32
    _, p, _, _, res = one(p=p, now=int(p["expires"][0]) + 1)
    assert res["fired"][0] == 1 and res["probes"][0] == p["probes"][0] == M32


def test_the_clock_wraps_as_the_retransmission_timer_does():
    """expires < now, unsigned and strict, at the same clock values as
    lvlip_rto_cpu's step 3: both timers share one convention."""
    S = lvlip.SND_FLOW_DTYPE
    for expires, now in ((M32 - 1, M32), (M32, M32), (M32, 0), (0, 1), (5, 4), (0x80000000, 0x7FFFFFFF),
                         (0x7FFFFFFF, 0x80000000), (0, M32)):
        fired = one(p=armed(expires), now=now)[4]["fired"][0]
        t = lvlip.rto_flows(1)
        t["armed"], t["expires"] = 1, expires
        s = np.zeros(1, dtype=S)
        s["nseg"] = 1
        rto_fired = lvlip.rto_cpu(s, None, None, t, now)[1]["fired"][0]
        assert int(fired) == int(expires < now) == int(rto_fired != 0), (expires, now)
    # arming across the wrap; the new timer is then far in the "past" of an unsigned clock and fires next round
    _, p, _, _, _ = one(now=M32 - 10)
    assert int(p["expires"][0]) == (M32 - 10 + 1000) & M32 == 989
    assert one(p=p, now=M32 - 9)[4]["fired"][0] == 1
    # firing across it
    _, p, _, _, res = one(p=armed(M32 - 1, 40000), now=M32)
    assert res["fired"][0] == 1 and int(p["expires"][0]) == (M32 + 60000) & M32


# --------------------------------------------------------------------- the probe --

def check_probes(f, lro, s, w, peer, out, fd, res, seed_fn=lost_carry_seed, l4=lvlip.RX_VERIFY_L4):
    n = s.size
    fired = np.flatnonzero(res["fired"])
    assert fired.size
    slots = out[:64 * n].reshape(n, 64)
    assert (slots[:, 54:] == CANARY).all() and (out[64 * n:] == CANARY).all()
    assert (slots[res["fired"] == 0] == CANARY).all(), "a silent flow's slot"
    assert fd["offset"].tolist() == [64 * k for k in range(n)] and not fd["reserved"].any()
    assert fd["len"].tolist() == [54 if x else 0 for x in res["fired"]]
    frames = [bytearray(slots[k, :54].tobytes()) for k in fired]
    assert (lvlip.rx_verify_cpu(frames, l4) == lvlip.RX_OK).all()
    _, rec = lvlip.lro_cpu(out, fd, peer, l4, out=np.zeros(n << 16, dtype=np.uint8))
    for k in fired:
        fr = bytes(frames[list(fired).index(k)])
        ack = (int(f["rcv_nxt"][k]) + (int(lro["delivered"][k]) if lro is not None else 0)) & M32
        assert (rec["flow"][k], rec["status"][k], rec["rel"][k], rec["dlen"][k]) == (k, lvlip.LRO_NO_DATA, M32, 0)
        assert rec["ack_seq"][k] == ack and not rec["tcp_flags"][k] & 0x09 and rec["tcp_flags"][k] & 0x10
        assert int(res["seq"][k]) == (int(s["snd_una"][k]) - 1) & M32 == int.from_bytes(fr[38:42], "big")
        hdr = w["hdr"][k].tobytes()
        ip = bytearray(fr[14:34])
        ip[10:12] = b"\0\0"
        assert int.from_bytes(fr[24:26], "little") == pyoracle.checksum(bytes(ip), 20, 0)
        tcp = bytearray(fr[34:54])
        tcp[16:18] = b"\0\0"
        assert int.from_bytes(fr[50:52], "little") == pyoracle.checksum(bytes(tcp), 20, seed_fn(hdr[26:30], hdr[30:34], 20))
        assert fr[16:18] == b"\x00\x28" and fr[18:20] == hdr[18:20] and fr[:14] == hdr[:14], "length, id, Ethernet"
        assert int.from_bytes(fr[48:50], "big") == int(s["win"][k]) and fr[47] == hdr[47] & ~0x09 & 0xFF
        assert fr == model_probe(hdr, int(s["snd_una"][k]), ack, int(s["win"][k]))
    for k in np.flatnonzero(res["fired"] == 0):
        assert rec["status"][k] not in (lvlip.LRO_PLACED, lvlip.LRO_NO_DATA) and res["seq"][k] == 0


def all_fire(n, **kw):
    f, s, w, peer = make_sides(n, **kw)
    w["unsent"], w["wnd"] = 5000, np.arange(n) % 536
    p = lvlip.persist_flows(n)
    p["armed"], p["interval"], p["expires"] = 1, 1000, 10
    lro = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
    lro["delivered"] = np.arange(n) * 7
    return f, lro, s, w, lvlip.rto_flows(n), p, peer


def test_every_probe_is_a_frame_the_peer_takes():
    f, lro, s, w, t, p, peer = all_fire(40)
    p["armed"][::5] = 0  # silent flows between them: they arm
    s["snd_una"][3] = s["snd_nxt"][3] = 0
    peer["rcv_nxt"][3] = 0
    _, _, out, fd, res = run_cpu(f, lro, s, w, t, p, 11)
    check_probes(f, lro, s, w, peer, out, fd, res)
    assert res["seq"][3] == M32 and out[64 * 3 + 38:64 * 3 + 42].tolist() == [255] * 4
    assert res["fired"].tolist() == [int(k % 5 != 0) for k in range(40)]
    # the template's PSH and FIN never reach the wire; its other flag bits do
    f, lro, s, w, t, p, peer = all_fire(3, flags=0x19 | 0x40)
    _, _, out, fd, res = run_cpu(f, None, s, w, t, p, 11)
    check_probes(f, None, s, w, peer, out, fd, res)
    assert out[47] == 0x50


def test_checksums_with_a_pseudo_header_sum_that_loses_its_carry():
    """250.x + 250.y as little-endian words pass 2^32: the seed wraps as the
    reference's does (src/tcp.c:92-95), so the field is not the RFC's and only
    the IPv4 header is verified here."""
    sa, da = bytes([10, 0, 0, 250]), bytes([10, 0, 0, 251])
    assert int.from_bytes(sa, "little") + int.from_bytes(da, "little") > M32
    f, lro, s, w, t, p, peer = all_fire(5, saddr=sa, daddr=da)
    _, _, out, fd, res = run_cpu(f, lro, s, w, t, p, 11)
    check_probes(f, lro, s, w, peer, out, fd, res, l4=0)
    assert (lvlip.rx_verify_cpu([bytearray(out[:54].tobytes())], lvlip.RX_VERIFY_L4) == lvlip.RX_BAD_L4).all()


# ----------------------------------------------------------- the store into t --

def test_only_dupacks_is_written_and_only_on_the_edge():
    for seed in range(6):
        f, lro, s, w, t, p, now = random_case(97, 50 + seed)
        t2, p2, _, _, _ = run_cpu(f, lro, s, w, t, p, now)
        edge = (p["armed"] != 0) & (p2["armed"] == 0) & (t["dead"] == 0)
        assert edge.any() and (t["dupacks"] > 0).any()
        want = t.copy()
        want["dupacks"][edge] = 0
        assert t2.tobytes() == want.tobytes()
        assert not p2[edge].view(np.uint8).any(), "p is all zero after the edge"


def episode(clear: bool):
    """Three answered probes, then the window reopens, four segments go out and
    the first is lost: the fired values of lvlip_rto_cpu over the three
    duplicate ACKs that follow.  clear False: the same script with the store
    into dupacks left out."""
    S, SR, PR = lvlip.SND_FLOW_DTYPE, lvlip.SND_RESULT_DTYPE, lvlip.PUSH_RESULT_DTYPE
    f, s, w, _ = make_sides(1)
    w["unsent"], w["wnd"] = 5000, 0
    t, p = lvlip.rto_flows(1), lvlip.persist_flows(1)
    sres, pres = np.zeros(1, dtype=SR), np.zeros(1, dtype=PR)
    now, probes = 100, 0

    def round_(n_dup=0, pushed=0):
        nonlocal t, p
        sres["n_dup"], pres["pushed"] = n_dup, pushed
        _, rres = lvlip.rto_cpu(s, sres, pres, t, now, lvlip.RTO_FAST)
        keep = t["dupacks"].copy()
        t, p, _, _, res = run_cpu(f, None, s, w, t, p, now)
        if not clear:
            t["dupacks"] = keep
        return int(rres["fired"][0]), int(res["fired"][0])

    assert round_() == (0, 0) and p["armed"][0] == 1
    answered = 0
    while probes < 3:
        now = int(p["expires"][0]) + 1
        fired = round_(n_dup=answered)  # last round's probe was answered by one duplicate ACK
        assert fired == (0, 1)
        probes, answered = probes + 1, 1
    now += 10
    assert round_(n_dup=1) == (0, 0) and t["dupacks"][0] >= 3
    # the window reopens (that ACK is one more duplicate); four segments go out
    w["wnd"], s["nseg"] = 5000, 4
    s["snd_nxt"] = s["snd_una"] + 4 * 536
    now += 10
    assert round_(n_dup=1, pushed=4) == (0, 0) and p["armed"][0] == 0
    got = []
    for _ in range(3):  # the first segment is lost: the other three raise a duplicate ACK each
        now += 10
        got.append(round_(n_dup=1)[0])
    return got, int(t["dupacks"][0])


def test_the_clear_is_what_lets_the_first_loss_after_the_stall_fire_fast():
    assert episode(True) == ([0, 0, lvlip.RTO_FASTRTX], 3)
    got, dupacks = episode(False)
    assert got == [0, 0, 0] and dupacks >= 7, "without the clear step 4 never sees dupacks cross 3"


# ------------------------------------------------------------------- refusals --

def test_refusals_write_nothing_and_noops():
    L = lvlip.lib()
    f, lro, s, w, t, p, now = random_case(4, 3)
    out = np.full(64 * 4, CANARY, dtype=np.uint8)
    fd, res = np.full(4, CANARY, dtype=np.uint8).repeat(16).view(FD), np.full(64, CANARY, dtype=np.uint8).view(R)
    ptr = lambda a: a.ctypes.data  # noqa: E731
    ok = [ptr(f), ptr(lro), ptr(s), ptr(w), ptr(t), ptr(p), 4, now, ptr(out), ptr(fd), ptr(res)]
    keep = [a.tobytes() for a in (t, p, out, fd, res)]

    def untouched():
        return [a.tobytes() for a in (t, p, out, fd, res)] == keep

    for i in (0, 2, 3, 4, 5, 8, 9, 10):
        bad = list(ok)
        bad[i] = None
        assert L.lvlip_persist_cpu(*bad) == lvlip.EINVAL and L.lvlip_persist_dev(*bad, None) == lvlip.EINVAL, i
    bad = list(ok)
    bad[6] = lvlip.LRO_MAX_FLOWS + 1
    assert L.lvlip_persist_cpu(*bad) == lvlip.EINVAL and L.lvlip_persist_dev(*bad, None) == lvlip.EINVAL
    assert untouched()
    for field, v, arm in (("armed", 2, None), ("reserved", (0, 0, 1), None), ("reserved", (1, 0, 0), None),
                          ("interval", 60001, 0), ("interval", 60001, 1), ("interval", 0, 1)):
        q = lvlip.persist_flows(4)
        q["armed"][3], q["interval"][3] = 1, 1000
        if arm is not None:
            q["armed"][3] = arm
        q[field][3] = v
        assert L.lvlip_persist_check(ptr(q), 4) == lvlip.EINVAL and L.lvlip_persist_check(ptr(q), 3) == lvlip.OK
        with pytest.raises(ValueError):
            lvlip.persist_check(q)
        bad = list(ok)
        bad[5] = ptr(q)
        qb = q.tobytes()
        assert L.lvlip_persist_cpu(*bad) == lvlip.EINVAL and untouched() and q.tobytes() == qb
    q = lvlip.persist_flows(2)
    q["interval"] = 60000  # not armed: the call never reads it
    assert L.lvlip_persist_check(ptr(q), 2) == lvlip.OK
    assert L.lvlip_persist_check(None, 1) == lvlip.EINVAL and L.lvlip_persist_check(None, 0) == lvlip.OK
    assert L.lvlip_persist_check(ptr(q), lvlip.LRO_MAX_FLOWS + 1) == lvlip.EINVAL
    # nflows == 0 is a no-op, whatever else is passed
    bad = list(ok)
    bad[6] = 0
    assert L.lvlip_persist_cpu(*bad) == lvlip.OK and L.lvlip_persist_dev(*bad, None) == lvlip.OK
    assert L.lvlip_persist_cpu(*([None] * 6), 0, 5, None, None, None) == lvlip.OK and untouched()
    # the device form refuses a misaligned pointer before any HIP call
    for i, off in ((0, 4), (1, 8), (2, 4), (3, 4), (4, 4), (5, 4), (9, 8), (10, 8)):
        bad = list(ok)
        bad[i] += off
        assert L.lvlip_persist_dev(*bad, None) == lvlip.EINVAL, i
    assert untouched()
    assert L.lvlip_persist_cpu(*ok) == lvlip.OK and not untouched()
    with pytest.raises(ValueError):
        lvlip.persist_cpu(f, None, s, w, t, lvlip.persist_flows(3), 5)
    with pytest.raises(ValueError):
        lvlip.persist_cpu(f, None, s, w, t, p, 5, out=np.zeros(64 * 4 - 1, dtype=np.uint8))


# ------------------------------------------------------------- the whole loop --

CLOSE0, CLOSE1 = 3, 45  # the receiving application reads nothing in rounds [CLOSE0, CLOSE1)
ACKS_ON = (lvlip.LRO_PLACED, lvlip.LRO_NO_DATA, lvlip.LRO_OUT_OF_WINDOW)


class PersistLoop(RtoLoop):
    """RtoLoop (8 flows x 40 x 536 B, every fifth first transmission lost)
    with a receiver that stops reading for a stretch of rounds, so that its
    window closes; that acknowledges only a round in which a frame of the flow
    arrived; and whose window update, the ACK of the round it reads again,
    is lost for every flow.  lvlip_persist_cpu runs behind lvlip_rto_cpu, its
    probes go to the receiver beside the ring's frames."""

    def run(self, persist: bool, rounds=None):
        p = self.p
        b, n = p.base, p.n
        L = b.link
        fb, fa, snd, w, tmpl = b.fb.copy(), L.fa.copy(), p.snd.copy(), p.w.copy(), L.tmpl.copy()
        ring = np.full(p.ring_bytes, CANARY, dtype=np.uint8)
        fd, sacked = np.zeros(p.nfd, dtype=FD), np.zeros(p.nfd, dtype=np.uint8)
        stream = np.full(L.stream.size, CANARY, dtype=np.uint8)
        res = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
        sres = np.zeros(n, dtype=lvlip.SND_RESULT_DTYPE)
        sent = np.zeros(n * p.segs, dtype=np.int32)
        t, pst = lvlip.rto_flows(n, snd_wnd=b.wnd), lvlip.persist_flows(n)
        w["wnd"] = b.wnd
        probe = np.full(64 * n, CANARY, dtype=np.uint8)
        no_probe = np.zeros(n, dtype=FD)
        no_probe["offset"] = 64 * np.arange(n)
        log = dict(wnd=[], drop=[], pres=[], stalled=[], frames=[], una=[], nxt=[], unsent=[])
        resent = now = done = 0
        while rounds is None or done < rounds:
            now += TICK
            pfd, pres = lvlip.push_cpu(fa, None, snd, w, L.payload, ring, fd, sacked)
            gate, rres = lvlip.rto_cpu(snd, sres, pres, t, now, lvlip.RTO_FAST, sacked)
            stalled = (snd["nseg"] == 0) & (w["unsent"] > 0) & (w["wnd"] < np.minimum(w["unsent"], w["mss"]))
            bfd, bres = no_probe, np.zeros(n, dtype=R)
            if persist:
                _, bfd, bres = lvlip.persist_cpu(fa, None, snd, w, t, pst, now, probe)
                assert not (bres["fired"] & (snd["nseg"] > 0)).any(), "a probe from a flow with data in flight"
            fd_out, _ = lvlip.rtx_sack_cpu(fa, None, snd, gate, sacked, ring, fd)
            resent += int((fd_out["len"] > 0).sum())
            wire = self.wire(pfd, fd_out, ring, sent)
            _, rec = lvlip.lro_cpu(ring, wire, fb, lvlip.RX_VERIFY_L4, out=stream)
            _, brec = lvlip.lro_cpu(probe, bfd, fb, lvlip.RX_VERIFY_L4, out=stream)
            assert (brec["status"][bres["fired"] == 1] == lvlip.LRO_NO_DATA).all()
            rec = np.concatenate([rec, brec])
            lvlip.lro_advance_carry(fb, rec, res, res)
            if CLOSE0 <= done < CLOSE1:  # nothing is read: the window is what lvlip_lro_next_* leaves of it
                wnd = fb["rcv_wnd"] - np.minimum(res["delivered"], fb["rcv_wnd"])
            else:
                wnd = np.minimum(b.wnd, b.end - fb["out_off"] - res["delivered"]).astype(np.uint32)
            tmpl["hdr"][:, 48], tmpl["hdr"][:, 49] = wnd >> 8, wnd & 0xFF
            ack, afd = lvlip.ack_cpu(tmpl, fb, res, lvlip.ACK_ALL, out=np.full(L.ack_bytes, CANARY, dtype=np.uint8))
            lvlip.lro_next_cpu(fb, res)
            fb["rcv_wnd"] = wnd
            got = np.zeros(n, dtype=bool)
            got[rec["flow"][np.isin(rec["status"], ACKS_ON)]] = True
            drop = ~got | (done == CLOSE1)  # no ACK without a frame; the window update is lost
            afd["len"][drop] = 0
            _, arec = lvlip.lro_cpu(ack, afd, fa, lvlip.RX_VERIFY_L4, out=np.zeros(n + 64, dtype=np.uint8))
            sres = lvlip.snd_cpu(fa, snd, arec, ring, fd)
            lvlip.sack_cpu(fa, snd, arec, ack, afd, ring, fd, sacked)
            wres = lvlip.wnd_cpu(fa, snd, t, w, arec, ack, afd, lvlip.WND_APPLY)
            lvlip.snd_next_cpu(snd, sres)
            frames = (pfd["len"] > 0).reshape(n, -1).sum(1) + (fd_out["len"] > 0).reshape(n, -1).sum(1) + bres["fired"]
            for k, v in (("wnd", wnd), ("drop", drop), ("pres", bres), ("stalled", stalled), ("frames", frames),
                         ("una", snd["snd_una"]), ("nxt", snd["snd_nxt"]), ("unsent", w["unsent"])):
                log[k].append(np.array(v).copy())
            done += 1
            if rounds is None and not snd["nseg"].any() and not w["unsent"].any():
                break
            assert done < 2000, "the loop does not end"
        return dict(stream=stream, fb=fb, snd=snd, w=w, res=res, sres=sres, ring=ring, fd=fd, sacked=sacked, sent=sent,
                    t=t, pst=pst, wres=wres, rres=rres, gate=gate, resent=resent, rounds=done, probe=probe,
                    log={k: np.array(v) for k, v in log.items()})


@functools.lru_cache(maxsize=None)
def persist_loop_cpu():
    loop = PersistLoop()
    return loop, loop.run(True)


def test_the_loop_hangs_without_the_call():
    loop = PersistLoop()
    got = loop.run(False, rounds=CLOSE1 + 10 + 50)["log"]
    assert (got["wnd"][CLOSE1 - 1] == 0).all(), "the window closed"
    a, z = CLOSE1 + 10, CLOSE1 + 10 + 50
    same = (got["una"][a - 1] == got["una"][z - 1]) & (got["nxt"][a - 1] == got["nxt"][z - 1]) & \
        (got["unsent"][a - 1] == got["unsent"][z - 1]) & (got["frames"][a:z].sum(0) == 0) & (got["unsent"][z - 1] > 0)
    assert same.any(), "every flow got over the lost window update by itself"
    assert (got["stalled"][z - 1] == same).all()


def test_the_loop_ends_with_the_call():
    loop, got = persist_loop_cpu()
    loop.check_done(got)
    log = got["log"]
    assert (log["wnd"][CLOSE1 - 1] == 0).all() and got["rounds"] > CLOSE1
    ever = log["stalled"].any(0)
    probes = log["pres"]["fired"].sum(0)
    assert ever.any() and (probes[ever] >= 1).all() and not probes[~ever].any()
    assert log["pres"]["probes"].max() >= 3, "the stretch is long enough for the interval to double"
    assert not got["pst"].view(np.uint8).any(), "p is all zero at the end"
    assert not (log["pres"]["fired"].astype(bool) & ~log["stalled"]).any()


# ------------------------------------------------------ example and sanitizers --

C_SRCS = ("persist_cpu.c", "rto_cpu.c", "push_cpu.c", "sack_cpu.c", "snd_cpu.c", "ack_cpu.c", "rcv_cpu.c", "seg_cpu.c",
          "csum_cpu.c")


def test_example_runs_to_its_own_check():
    exe = os.path.join(ROOT, "examples", "build", "persist_loop")
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "persist_loop ok" in r.stdout, r.stdout + r.stderr


def _sanitized(tmp_path, main_c, exe_name):
    """A stand-alone program of its own process: the main and the library's C
    sources as strict C99 under ASan + UBSan."""
    exe = tmp_path / exe_name
    csrc = os.path.join(ROOT, "level-ip_amd", "csrc")
    src = [main_c] + [os.path.join(csrc, f) for f in C_SRCS]
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "include"), "-I", csrc, *src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    return r.stdout


def test_example_under_sanitizers(tmp_path):
    assert "persist_loop ok" in _sanitized(tmp_path, os.path.join(ROOT, "examples", "persist_loop.c"), "persist_loop_san")


def test_hostile_state_under_sanitizers(tmp_path):
    """tests/sanitize/persist_hostile.c, a stand-alone main: lvlip_persist_check
    and lvlip_persist_cpu on a NULL mix, nflows at the limit and garbage
    intervals, and flow_persist_step on boundary states, under ASan + UBSan."""
    assert "persist_hostile ok" in _sanitized(tmp_path, os.path.join(ROOT, "tests", "sanitize", "persist_hostile.c"),
                                              "persist_hostile_san")
