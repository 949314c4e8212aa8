"""The congestion window on the MI355X (k_cc_sum and k_cc_fin, cc_kernels.hip):
every byte of c, t and res of lvlip_cc_dev against lvlip_cc_cpu, at flow counts
around a workgroup's four waves, with queues around a wave's 64 entries at odd
seg0; queues that span many waves and workgroups; the scoreboard at every
alignment; the refusals; and the loop of tests/test_rto_gpu.py with the call in
every round, queued on one stream with one synchronise.  Every pointer handed
to the device is valid for the ranges the contract names."""
import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import CANARY, _t, guarded, unguard
from test_cc_cpu import IW, QUEUES, cc_loop_cpu, random_case
from test_rto_cpu import TICK

pytestmark = pytest.mark.gpu
C, R, T = lvlip.CC_FLOW_DTYPE, lvlip.CC_RESULT_DTYPE, lvlip.RTO_FLOW_DTYPE


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


def run_both(dev, s, snd, prev, c, t, fd, sacked, shift: int = 0):
    """lvlip_cc_cpu and lvlip_cc_dev on copies of one case; c, t and res byte
    for byte, canaries behind every written array, the inputs unchanged.  The
    scoreboard starts `shift` bytes into its allocation."""
    cc, tc = c.copy(), t.copy()
    res = lvlip.cc_cpu(s, snd, prev, cc, tc, fd, sacked)
    n = s.size
    s_t = _t(s, dev)
    snd_t = None if snd is None else _t(snd, dev)
    prev_t = None if prev is None else _t(prev, dev)
    fd_t = None if fd is None else _t(fd, dev)
    k_t = None if sacked is None else torch.cat([guarded(0, dev)[:shift], _t(sacked, dev)])
    c_t, t_t = torch.cat([_t(c, dev), guarded(0, dev)]), torch.cat([_t(t, dev), guarded(0, dev)])
    res_t = guarded(16 * n, dev)
    torch.cuda.synchronize(dev)
    lvlip.cc_dev(s_t, snd_t, prev_t, c_t, t_t, fd_t, None if k_t is None else k_t[shift:], res_t)
    torch.cuda.synchronize(dev)
    assert unguard(c_t, c.nbytes, C).tobytes() == cc.tobytes(), "c"
    assert unguard(t_t, t.nbytes, T).tobytes() == tc.tobytes(), "t"
    assert unguard(res_t, 16 * n, R).tobytes() == res.tobytes(), "res"
    for a, a_t, name in ((s, s_t, "s"), (snd, snd_t, "snd"), (prev, prev_t, "prev"), (fd, fd_t, "fd")):
        assert a is None or np.array_equal(a_t.cpu().numpy(), a.view(np.uint8).reshape(-1)), name + " is only read"
    if sacked is not None:
        assert np.array_equal(k_t.cpu().numpy()[shift:], sacked) and (k_t.cpu().numpy()[:shift] == CANARY).all()
    return cc, tc, res


@pytest.mark.parametrize("nflows", (1, 3, 5, 257))
def test_dev_equals_cpu(nflows, dev):
    case = random_case(nflows, 100 + nflows)
    _, t, res = run_both(dev, *case)
    if nflows == 257:  # what the case is for: every queue length, marks, dead flows, every fired value, short frames
        s, snd, prev = case[0], case[1], case[2]
        assert set(s["nseg"].tolist()) == set(QUEUES) and set(prev["fired"].tolist()) == {0, 1, 2}
        assert case[4]["dead"].any() and res["n_sacked"].any() and (case[5]["len"] < 54).any()
        assert (snd["popped"] == 0).any() and (snd["popped"] == s["nseg"]).any() and (snd["popped"] > s["nseg"]).any()
        assert np.bitwise_or.reduce(res["event"]) == 0x1F
    for drop in (1, 2, 6):  # snd, prev and sacked NULL in turn
        alt = list(random_case(nflows, 200 + nflows))
        alt[drop] = None
        run_both(dev, *alt)
    alt = list(case)
    alt[5] = alt[6] = None  # no scoreboard and no descriptors
    run_both(dev, *alt)


@pytest.mark.parametrize("nflows,nseg", ((1, 70_000), (3, 20_000)))
def test_one_long_queue_spans_many_waves(nflows, nseg, dev):
    s, snd, prev, c, t, fd, sacked = random_case(nflows, 300 + nflows, queues=(nseg,))
    t["dead"] = 0
    snd["popped"] = [0, 12_345, 7][:nflows]
    _, _, res = run_both(dev, s, snd, prev, c, t, fd, sacked)
    assert (res["n_sacked"] > nseg // 8).all() and (res["sacked_bytes"] > 0).all()
    want = [int((sacked[int(a) + int(p):int(a) + nseg] != 0).sum()) for a, p in zip(s["seg0"], snd["popped"])]
    assert res["n_sacked"].tolist() == want


@pytest.mark.parametrize("shift", (0, 1, 3, 7))
def test_the_scoreboard_at_any_alignment(shift, dev):
    run_both(dev, *random_case(5, 400), shift=shift)


def test_misaligned_pointers_are_refused_before_any_launch(dev):
    s, snd, prev, c, t, fd, sacked = random_case(4, 1)
    ten = [_t(a, dev) for a in (s, snd, prev, c, t, fd, sacked)]
    pad = lambda x: torch.cat([x, guarded(0, dev)])  # noqa: E731  a misaligned start stays inside the allocation
    ten = [pad(x) for x in ten]
    res = guarded(16 * 4 + 16, dev)
    p = [x.data_ptr() for x in ten]
    ok = (p[0], p[1], p[2], p[3], p[4], 4, p[5], p[6], res.data_ptr(), None)
    for i, off in ((0, 4), (1, 8), (2, 8), (3, 4), (4, 4), (6, 8), (8, 8)):
        bad = list(ok)
        bad[i] += off
        assert lvlip.lib().lvlip_cc_dev(*bad) == lvlip.EINVAL, i
    torch.cuda.synchronize(dev)
    assert (res == CANARY).all().item(), "a refused call wrote res"
    assert unguard(ten[3], c.nbytes, C).tobytes() == c.tobytes() and unguard(ten[4], t.nbytes, T).tobytes() == t.tobytes()


# ------------------------------------------------------------- the whole loop --

def loop_dev(loop, rounds: int, dev) -> dict:
    """CcLoop.run_cpu through the device forms on ONE stream, as
    tests/test_rto_gpu.py's loop_dev with lvlip_cc_dev between lvlip_sack_dev
    and lvlip_wnd_dev: no copy to the host, no synchronise and no host decision
    between the first launch and the last.  Every round's lvlip_cc_result is
    kept, on the device."""
    p = loop.p
    b, n = p.base, p.n
    L, nrtx, npush = b.link, p.nslots_rtx, p.nslots
    fb, fa, snd, tmpl, pay = (_t(a, dev) for a in (b.fb, L.fa, p.snd, L.tmpl, L.payload))
    w0 = p.w.copy()
    w0["wnd"] = min(b.wnd, IW)
    w, t = _t(w0, dev), _t(lvlip.rto_flows(n, snd_wnd=b.wnd, wnd_cap=IW), dev)
    c = torch.cat([_t(lvlip.cc_init(p.mss, nflows=n), dev), guarded(0, dev)])
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
    ring = torch.full((p.ring_bytes + 64,), CANARY, dtype=torch.uint8, device=dev)
    fd, sacked = guarded(16 * p.nfd, dev), guarded(p.nfd, dev)
    fd[:16 * p.nfd] = 0
    sacked[:p.nfd] = 0
    stream_t = torch.full((L.stream.size,), CANARY, dtype=torch.uint8, device=dev)
    res, sres, kres, pres, wres, rres, gate = z(48 * n), z(32 * n), z(16 * n), z(16 * n), z(16 * n), z(16 * n), z(32 * n)
    cres = guarded(16 * n * rounds, dev)
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
            lvlip.cc_dev(snd, sres, rres, c, t, fd[:16 * p.nfd], sacked[:p.nfd], cres[16 * n * r:16 * n * (r + 1)], stream=s)
            lvlip.wnd_dev(fa, snd, t, w, arec, ack, afd, lvlip.WND_APPLY, wres, stream=s)
            lvlip.snd_next_dev(snd, sres, stream=s)
    s.synchronize()  # the only one
    assert (rec[16 * nw:] == CANARY).all(), "written behind one round's records"
    assert (ring[p.ring_bytes:] == CANARY).all(), "written behind the ring"
    h = lambda x, dt=np.uint8: x.cpu().numpy().view(dt)  # noqa: E731
    return dict(stream=h(stream_t), fb=h(fb, lvlip.LRO_FLOW_DTYPE), snd=h(snd, lvlip.SND_FLOW_DTYPE),
                w=h(w, lvlip.PUSH_FLOW_DTYPE), res=h(res, lvlip.LRO_RESULT_DTYPE), sres=h(sres, lvlip.SND_RESULT_DTYPE),
                ring=h(ring)[:p.ring_bytes], fd=unguard(fd, 16 * p.nfd, lvlip.FRAME_DESC_DTYPE),
                sacked=unguard(sacked, p.nfd, np.uint8), sent=h(sent, np.int32), t=h(t, T),
                c=unguard(c, 32 * n, C), cres=unguard(cres, 16 * n * rounds, R).reshape(rounds, n),
                wres=h(wres, lvlip.WND_RESULT_DTYPE), rres=h(rres, lvlip.RTO_RESULT_DTYPE),
                gate=h(gate, lvlip.SND_RESULT_DTYPE), resent=int(resent.item()))


def test_the_loop_with_a_congestion_window_on_one_stream(dev):
    """8 flows x 40 x 536 B through 16 slots, every fifth first transmission
    lost, lvlip_cc_dev in every round: as many rounds as the CPU loop needed,
    one synchronise.  Every byte is delivered; state, stream and every round's
    lvlip_cc_result equal the CPU loop's byte for byte."""
    loop, want = cc_loop_cpu()
    got = loop_dev(loop, want["rounds"], dev)
    loop.rto.check_done(got)
    for k in ("stream", "fb", "snd", "w", "res", "sres", "ring", "fd", "sacked", "sent", "t", "c", "cres", "wres", "rres",
              "gate"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["resent"] == want["resent"]
