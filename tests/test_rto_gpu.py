"""The retransmission timer on the MI355X (k_rto, rto_kernels.hip): every byte
of t, gate, res and the scoreboard of lvlip_rto_dev against lvlip_rto_cpu, at
the flow counts around a workgroup's four waves and a wave's 64 lanes, with
queues around the clear's 64-byte step at odd seg0; the golden sessions; and
the whole loop with a clock, both new calls in every round, queued on one
stream with one synchronise."""
import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import CANARY, _t, guarded, unguard
from test_rto_cpu import TICK, rto_loop_cpu

pytestmark = pytest.mark.gpu
M32 = 0xFFFFFFFF
QUEUES = (0, 1, 63, 64, 65, 200)


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


def random_case(nflows: int, seed: int):
    """States in every branch of the four steps; queues of QUEUES entries at odd seg0."""
    rng = np.random.default_rng(seed)
    s = np.zeros(nflows, dtype=lvlip.SND_FLOW_DTYPE)
    s["nseg"] = rng.choice(QUEUES, nflows)
    s["seg0"] = 1 + 2 * np.cumsum(np.concatenate([[0], (s["nseg"][:-1] + 3) // 2 + 1]))  # odd, with gaps
    t = lvlip.rto_flows(nflows)
    now = 1_000_000
    t["armed"] = rng.random(nflows) < .7
    t["dead"] = rng.random(nflows) < .1
    t["backoff"] = rng.choice([0, 0, 0, 1, 5, 255], nflows)
    t["rto"] = rng.choice([200, 1000, 1000, 59999, 60000, 60001, 64000, 0x80000000], nflows)
    t["expires"] = (now + rng.integers(-1200, 1200, nflows)) & M32
    t["expires"][rng.random(nflows) < .2] = now  # not yet: the test is strict
    t["srtt"] = rng.choice([0, 0, 1, 120, 6329, 1 << 20], nflows)
    t["rttvar"] = rng.choice([0, 60, 49, 51, 1 << 19], nflows)
    t["dupacks"] = rng.integers(0, 5, nflows)
    sres = np.zeros(nflows, dtype=lvlip.SND_RESULT_DTYPE)
    sres["n_new"] = rng.choice([0, 0, 1, 3], nflows)
    sres["n_dup"] = rng.choice([0, 1, 2, 4], nflows)
    sres["snd_una"], sres["n_old"] = 77, 5  # must not reach the gate
    pres = np.zeros(nflows, dtype=lvlip.PUSH_RESULT_DTYPE)
    pres["pushed"] = np.where(rng.random(nflows) < .5, 0, np.minimum(s["nseg"], rng.choice([1, 64, 500], nflows)))
    sacked = rng.integers(1, 3, int(s["seg0"][-1] + s["nseg"][-1]) + 7).astype(np.uint8)
    return s, sres, pres, t, now, sacked


def run_both(dev, s, sres, pres, t, now, sacked, flags):
    tc, kc = t.copy(), None if sacked is None else sacked.copy()
    gate, res = lvlip.rto_cpu(s, sres, pres, tc, now, flags, kc)
    n = s.size
    s_t = _t(s, dev)
    sres_t = None if sres is None else _t(sres, dev)
    pres_t = None if pres is None else _t(pres, dev)
    t_t = torch.cat([_t(t, dev), guarded(0, dev)])
    k_t = None if sacked is None else torch.cat([_t(sacked, dev), guarded(0, dev)])
    gate_t, res_t = guarded(32 * n, dev), guarded(16 * n, dev)
    torch.cuda.synchronize(dev)
    lvlip.rto_dev(s_t, sres_t, pres_t, t_t, now, flags, k_t, gate_t, res_t)
    torch.cuda.synchronize(dev)
    assert np.array_equal(s_t.cpu().numpy(), s.view(np.uint8).reshape(-1)), "s is only read"
    assert unguard(t_t, t.nbytes, lvlip.RTO_FLOW_DTYPE).tobytes() == tc.tobytes(), "t"
    assert unguard(gate_t, 32 * n, lvlip.SND_RESULT_DTYPE).tobytes() == gate.tobytes(), "gate"
    assert unguard(res_t, 16 * n, lvlip.RTO_RESULT_DTYPE).tobytes() == res.tobytes(), "res"
    if sacked is not None:
        assert unguard(k_t, sacked.size, np.uint8).tobytes() == kc.tobytes(), "sacked"
    return tc, gate, res, kc


@pytest.mark.parametrize("nflows", (1, 3, 4, 5, 63, 64, 65, 257))
def test_dev_equals_cpu(nflows, dev):
    for seed, flags in ((0, 0), (1, lvlip.RTO_FAST)):
        case = random_case(nflows, seed + 10 * nflows)
        run_both(dev, *case, flags)


def test_every_queue_length_times_out_and_only_its_range_is_cleared(dev):
    """All of QUEUES time out at odd seg0: the bytes on both sides of every
    range keep their marks (checked against the CPU form, which the CPU tests
    hold to a plain restatement), and a fast retransmit keeps its own."""
    n = len(QUEUES) + 1
    s = np.zeros(n, dtype=lvlip.SND_FLOW_DTYPE)
    s["nseg"] = QUEUES + (65,)
    s["seg0"] = [1, 3, 7, 73, 141, 209, 411]
    t = lvlip.rto_flows(n)
    t["armed"], t["expires"] = 1, 500
    t["armed"][-1], t["dupacks"][-1] = 0, 2
    sres = np.zeros(n, dtype=lvlip.SND_RESULT_DTYPE)
    sres["n_dup"][-1] = 1
    sacked = np.full(480, 1, dtype=np.uint8)
    tc, gate, res, kc = run_both(dev, s, sres, None, t, 501, sacked, lvlip.RTO_FAST)
    assert res["fired"].tolist() == [0, 1, 1, 1, 1, 1, 2]
    assert int((kc == 0).sum()) == sum(QUEUES) and kc[6] == 1 and kc[70] == 1 and kc[72] == 1 and kc[411:476].all()
    run_both(dev, s, None, None, t, 501, None, 0)  # NULL snd, push and sacked


def test_the_golden_sessions_on_the_device(dev):
    """The three sessions of tests/golden/rto_ref.json side by side as three
    flows would not share a clock; so each session's states before every step
    (from the CPU replay) go through the device in one call per step kind."""
    from test_rto_cpu import golden

    for sess in golden()["sessions"]:
        t = lvlip.rto_flows(1)
        nseg = 0
        for st in sess["steps"]:
            s = np.zeros(1, dtype=lvlip.SND_FLOW_DTYPE)
            sres = np.zeros(1, dtype=lvlip.SND_RESULT_DTYPE)
            pres = np.zeros(1, dtype=lvlip.PUSH_RESULT_DTYPE)
            if st["op"] == "push":
                nseg, now, pres["pushed"] = 1, 4242, 1
            elif st["op"] == "timeout":
                t["expires"], now = 9000, 9001
            else:
                if t["armed"][0]:
                    t["expires"] = M32
                now = (int(t["expires"][0]) - int(t["rto"][0]) + st["r"]) & M32
                sres["n_new"] = 1
                nseg = 0 if st["op"] == "ack_all" else nseg
            s["nseg"] = nseg
            t = run_both(dev, s, sres, pres, t, now, None, 0)[0]
            assert {k: int(t[k][0]) for k in st["after"]} == st["after"]


def test_misaligned_pointers_are_refused_before_any_launch(dev):
    s, sres, pres, t, now, sacked = random_case(4, 1)
    ten = [_t(a, dev) for a in (s, sres, pres, t)]
    gate, res = torch.zeros(160, dtype=torch.uint8, device=dev), torch.zeros(96, dtype=torch.uint8, device=dev)
    p = [x.data_ptr() for x in ten]
    ok = (p[0], p[1], p[2], p[3], 4, now, 0, None, gate.data_ptr(), res.data_ptr(), None)
    for i, off in ((0, 4), (1, 8), (2, 4), (3, 4), (8, 8), (9, 8)):
        bad = list(ok)
        bad[i] += off
        assert lvlip.lib().lvlip_rto_dev(*bad) == lvlip.EINVAL, i
    torch.cuda.synchronize(dev)
    assert not gate.any().item() and np.array_equal(ten[3].cpu().numpy(), t.view(np.uint8).reshape(-1))


# ------------------------------------------------------------- the whole loop --

def loop_dev(loop, rounds: int, dev) -> dict:
    """RtoLoop.run_cpu(gated=True) through the device forms on ONE stream: no
    copy to the host, no synchronise and no host decision between the first
    launch and the last; the clock is the only value the host supplies per
    round.  The network and the receiver's window are torch operations on the
    same stream."""
    p = loop.p
    b, n = p.base, p.n
    L, nrtx, npush = b.link, p.nslots_rtx, p.nslots
    fb, fa, snd, tmpl, pay = (_t(a, dev) for a in (b.fb, L.fa, p.snd, L.tmpl, L.payload))
    w0 = p.w.copy()
    w0["wnd"] = b.wnd
    w, t = _t(w0, dev), _t(lvlip.rto_flows(n, snd_wnd=b.wnd), dev)
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
    ring = torch.full((p.ring_bytes + 64,), CANARY, dtype=torch.uint8, device=dev)
    fd, sacked = guarded(16 * p.nfd, dev), guarded(p.nfd, dev)
    fd[:16 * p.nfd] = 0
    sacked[:p.nfd] = 0
    stream_t = torch.full((L.stream.size,), CANARY, dtype=torch.uint8, device=dev)
    res, sres, kres, pres, wres, rres, gate = z(48 * n), z(32 * n), z(16 * n), z(16 * n), z(16 * n), z(16 * n), z(32 * n)
    sent = torch.zeros(n * p.segs, dtype=torch.int32, device=dev)
    nw = npush + nrtx
    rec, arec, afd = guarded(16 * nw, dev), z(16 * n), z(16 * n)
    pfd, fd_out, pick, wire = z(16 * npush), z(16 * nrtx), z(4 * nrtx), z(16 * nw)
    ack, sink = z(L.ack_bytes), z(n + 64)
    ws = torch.empty(lvlip.lro_advance_carry_workspace_bytes(nw, n), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(max(lvlip.sack_workspace_bytes(n, n), 256), dtype=torch.uint8, device=dev)
    end_lo = torch.from_numpy((b.end & 0xFFFFFFFF).astype(np.int64)).to(dev)
    fb32 = fb.view(torch.int32).view(n, 12)   # rcv_wnd is word 4, out_off's low word 6
    res32 = res.view(torch.int32).view(n, 12)  # delivered is word 0
    tm = tmpl.view(n, 64)                      # hdr at byte 8: the window at 8 + 48
    iss = torch.from_numpy(p.iss).to(dev)
    flow = torch.cat([torch.arange(npush, device=dev) // p.rtx, torch.arange(nrtx, device=dev) // p.rtx])
    first = torch.arange(nw, device=dev) < npush
    four = torch.arange(4, device=dev)
    resent = torch.zeros((), dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        for r in range(rounds):
            now = (r + 1) * TICK
            lvlip.push_dev(fa, None, snd, w, npush, pay, ring, fd[:16 * p.nfd], sacked[:p.nfd], pfd, pres, stream=s)
            lvlip.rto_dev(snd, sres, pres, t, now, lvlip.RTO_FAST, sacked[:p.nfd], gate, rres, stream=s)
            lvlip.rtx_sack_dev(fa, None, snd, gate, sacked[:p.nfd], nrtx, ring, fd[:16 * p.nfd], fd_out, pick, stream=s)
            resent += ((fd_out.view(torch.int64).view(nrtx, 2)[:, 1] & 0xFFFFFFFF) > 0).sum()
            # the network: stream segment 4 mod 5 of a flow is lost when lvlip_push_* sends it
            wire[:16 * npush] = pfd
            wire[16 * npush:] = fd_out
            fo = wire.view(torch.int64).view(nw, 2)
            live = (fo[:, 1] & 0xFFFFFFFF) > 0
            by = ring[fo[:, 0:1] + 38 + four].to(torch.int64)
            seq = (by[:, 0] << 24) | (by[:, 1] << 16) | (by[:, 2] << 8) | by[:, 3]
            seg = (((seq - iss[flow]) & 0xFFFFFFFF) // p.mss).clamp(0, p.segs - 1)
            idx = flow * p.segs + seg
            lost = live & first & (seg % 5 == 4)
            sent.index_put_((idx,), live.to(torch.int32), accumulate=True)
            w32 = wire.view(torch.int32).view(nw, 4)
            w32[:, 2] = torch.where(lost, torch.zeros_like(w32[:, 2]), w32[:, 2])
            # B
            lvlip.lro_dev(ring, wire, fb, lvlip.RX_VERIFY_L4, stream_t, rec[:16 * nw], stream=s)
            lvlip.lro_advance_carry_dev(fb, rec[:16 * nw], res, res, ws, stream=s)
            wnd = torch.minimum(torch.full_like(end_lo, b.wnd), end_lo - fb32[:, 6] - res32[:, 0])
            tm[:, 56], tm[:, 57] = (wnd >> 8).to(torch.uint8), (wnd & 0xFF).to(torch.uint8)
            lvlip.ack_dev(tmpl, fb, res, lvlip.ACK_ALL, ack, afd, stream=s)
            lvlip.lro_next_dev(fb, res, stream=s)
            fb32[:, 4] = wnd.to(torch.int32)
            # A
            lvlip.lro_dev(ack, afd, fa, lvlip.RX_VERIFY_L4, sink, arec, stream=s)
            lvlip.snd_dev(fa, snd, arec, ring, fd[:16 * p.nfd], sres, stream=s)
            lvlip.sack_dev(fa, snd, arec, ack, afd, ring, fd[:16 * p.nfd], sacked[:p.nfd], kres, ws2, stream=s)
            lvlip.wnd_dev(fa, snd, t, w, arec, ack, afd, lvlip.WND_APPLY, wres, stream=s)
            lvlip.snd_next_dev(snd, sres, stream=s)
    s.synchronize()  # the only one
    assert (rec[16 * nw:] == CANARY).all(), "written behind one round's records"
    assert (ring[p.ring_bytes:] == CANARY).all(), "written behind the ring"
    h = lambda x, dt=np.uint8: x.cpu().numpy().view(dt)  # noqa: E731
    return dict(stream=h(stream_t), fb=h(fb, lvlip.LRO_FLOW_DTYPE), snd=h(snd, lvlip.SND_FLOW_DTYPE),
                w=h(w, lvlip.PUSH_FLOW_DTYPE), res=h(res, lvlip.LRO_RESULT_DTYPE), sres=h(sres, lvlip.SND_RESULT_DTYPE),
                ring=h(ring)[:p.ring_bytes], fd=unguard(fd, 16 * p.nfd, lvlip.FRAME_DESC_DTYPE),
                sacked=unguard(sacked, p.nfd, np.uint8), sent=h(sent, np.int32), t=h(t, lvlip.RTO_FLOW_DTYPE),
                wres=h(wres, lvlip.WND_RESULT_DTYPE), rres=h(rres, lvlip.RTO_RESULT_DTYPE),
                gate=h(gate, lvlip.SND_RESULT_DTYPE), resent=int(resent.item()))


def test_the_loop_with_a_clock_on_one_stream(dev):
    """8 flows x 40 x 536 B through 16 slots, every fifth first transmission
    lost, lvlip_wnd_dev and lvlip_rto_dev in every round: as many rounds as the
    CPU loop needed, one synchronise.  Every byte is delivered; the final state
    and the stream equal the CPU loop's byte for byte; the gate re-sent no more
    frames than the ungated loop (both counts from the CPU forms, here)."""
    loop, want, ungated = rto_loop_cpu()
    got = loop_dev(loop, want["rounds"], dev)
    loop.check_done(got)
    for k in ("stream", "fb", "snd", "w", "res", "sres", "ring", "fd", "sacked", "sent", "t", "wres", "rres", "gate"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["resent"] == want["resent"] <= ungated["resent"]
