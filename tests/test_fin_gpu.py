"""The end of a connection on the MI355X (k_fin_scan and k_fin,
fin_kernels.hip): every byte of f, s, x, gate, res, fd_out and out of
lvlip_fin_dev against lvlip_fin_cpu (which tests/test_fin_cpu.py holds to a
plain restatement and to the reference's own frames), at the flow counts around
a lane group's eight flows per wave and 32 per workgroup, at record counts
around a workgroup's 256, with `out` at every address mod 16, with and without
`close`, and every array the call writes between canary bytes."""
import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import CANARY, _t, guarded, unguard
from fin_model import ACK_OWED, CLOSED, EST, FW1, PEER_FIN, RESENT, SENT, random_case

pytestmark = pytest.mark.gpu
X, R, FD, G = lvlip.FIN_FLOW_DTYPE, lvlip.FIN_RESULT_DTYPE, lvlip.FRAME_DESC_DTYPE, lvlip.LRO_RESULT_DTYPE
F, S = lvlip.LRO_FLOW_DTYPE, lvlip.SND_FLOW_DTYPE


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


def run_both(dev, f, gin, rec, s, w, t, x, close, now, shift=0):
    """Both forms from the same bytes; `out` starts `shift` bytes into a 256-B
    aligned buffer of canary bytes, and f, s, x, gate, res, fd_out and the
    workspace have canary bytes behind them.  Returns the CPU form's
    (f, s, x, out, fd, gate, res)."""
    n = s.size
    fc, sc, xc = f.copy(), s.copy(), x.copy()
    out, fd, gate, res = lvlip.fin_cpu(fc, gin, rec, sc, w, t, xc, close, now, np.full(64 * n, CANARY, dtype=np.uint8))
    ins = [_t(a, dev) for a in (gin, w, t)]
    rec_t = _t(rec, dev) if rec is not None and rec.size else None
    close_t = None if close is None else _t(close, dev)
    f_t, s_t, x_t = (torch.cat([_t(a, dev), guarded(0, dev)]) for a in (f, s, x))
    buf = devbuf.guarded_aligned(shift + 64 * n, dev)
    fd_t, res_t, gate_t = guarded(16 * n, dev), guarded(16 * n, dev), guarded(48 * n, dev)
    nws = lvlip.fin_workspace_bytes(n)
    ws_t = guarded(nws, dev)
    torch.cuda.synchronize(dev)
    lvlip.fin_dev(f_t[:f.nbytes], ins[0], rec_t, s_t[:s.nbytes], ins[1], ins[2], x_t[:x.nbytes], close_t, now,
                  buf[shift:], gate_t, ws_t[:nws], fd_t, res_t)
    torch.cuda.synchronize(dev)
    for a, q in zip((gin, w, t), ins):
        assert np.array_equal(q.cpu().numpy(), a.view(np.uint8).reshape(-1)), "gin, w and t are only read"
    if rec_t is not None:
        assert np.array_equal(rec_t.cpu().numpy(), rec.view(np.uint8).reshape(-1)), "rec is only read"
    assert unguard(f_t, f.nbytes, F).tobytes() == fc.tobytes(), "f"
    assert unguard(s_t, s.nbytes, S).tobytes() == sc.tobytes(), "s"
    assert unguard(x_t, x.nbytes, X).tobytes() == xc.tobytes(), "x"
    assert unguard(gate_t, 48 * n, G).tobytes() == gate.tobytes(), "gate"
    assert unguard(res_t, 16 * n, R).tobytes() == res.tobytes(), "res"
    assert unguard(fd_t, 16 * n, FD).tobytes() == fd.tobytes(), "fd_out"
    unguard(ws_t, nws, np.uint8)
    got = buf.cpu().numpy()
    assert (got[:shift] == CANARY).all() and (got[shift + 64 * n:] == CANARY).all(), "written around out"
    assert got[shift:shift + 64 * n].tobytes() == out.tobytes(), "out"
    return fc, sc, xc, out, fd, gate, res


@pytest.mark.parametrize("nflows", (1, 7, 8, 9, 31, 32, 33, 64, 257))
def test_dev_equals_cpu(nflows, dev):
    events = 0
    for seed in (0, 1, 2):
        case = random_case(nflows, seed + 10 * nflows)
        res = run_both(dev, *case, shift=(3 * nflows + 5 * seed) % 16)[6]
        events |= int(np.bitwise_or.reduce(res["events"]))
    if nflows >= 31:
        assert events & SENT and events & RESENT and events & PEER_FIN, "the cases are fixed by their seeds"
    case = random_case(nflows, 7 + nflows, with_close=False)
    assert case[7] is None
    run_both(dev, *case)  # close == NULL


@pytest.mark.parametrize("nrec", (0, 1, 63, 64, 65, 1000))
def test_record_counts_around_a_workgroup(nrec, dev):
    """FIN records among data and ACK records, for 33 flows."""
    for seed in (0, 1):
        case = random_case(33, 100 + seed + nrec, nrec=nrec)
        res = run_both(dev, *case, shift=seed)[6]
        if nrec >= 64:
            assert (res["events"] & PEER_FIN).any() and (res["events"] & ACK_OWED).any()
        if nrec == 0:
            assert not (res["events"] & (PEER_FIN | ACK_OWED)).any()
            run_both(dev, case[0], case[1], None, *case[3:])  # rec == NULL


def all_or_none(n, fire):
    f, gin, rec, s, w, t, x, close, now = random_case(n, 11)
    t["dead"], s["nseg"], w["unsent"] = 0, 0, 0
    x["state"], x["interval"], x["flags"] = FW1, 1000, 1
    s["snd_una"] = s["snd_nxt"] - 1
    x["fin_seq"] = s["snd_una"]
    x["expires"] = now - 1 if fire else now
    return f, gin, rec, s, w, t, x, close, now


def test_out_at_every_address_mod_16(dev):
    """Silent flows between those that re-send, so a store past a frame's 54
    bytes or into a neighbour's slot shows at every offset of the first chunk."""
    case = all_or_none(40, True)
    case[6]["expires"][::3] = case[8]
    for shift in range(16):
        fd = run_both(dev, *case, shift=shift)[4]
        assert (fd["len"] > 0).sum() == 26


def test_all_send_and_none_sends(dev):
    res = run_both(dev, *all_or_none(70, True), shift=9)[6]
    assert ((res["events"] & RESENT) != 0).all()
    _, _, _, out, fd, _, res = run_both(dev, *all_or_none(70, False), shift=9)
    assert not (res["events"] & (SENT | RESENT)).any() and not fd["len"].any() and (out == CANARY).all(), "out untouched"
    f, gin, rec, s, w, t, x, close, now = random_case(70, 12)
    x["state"], t["dead"], w["unsent"] = EST, 0, 0
    res = run_both(dev, f, gin, rec, s, w, t, x, np.ones(70, dtype=np.uint8), now, shift=3)[6]
    assert ((res["events"] & SENT) != 0).all(), "every flow closes at once"
    x["state"] = CLOSED
    _, _, x2, out, _, gate, res = run_both(dev, f, gin, rec, s, w, t, x, np.ones(70, dtype=np.uint8), now, shift=3)
    assert not res["events"].any() and (out == CANARY).all() and gate.tobytes() == gin.tobytes()


def test_two_runs_give_identical_bytes(dev):
    case = random_case(257, 4)
    a = run_both(dev, *case, shift=1)
    b = run_both(dev, *case, shift=1)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


def test_refusals_before_any_launch(dev):
    f, gin, rec, s, w, t, x, close, now = random_case(4, 1)
    ten = [_t(a, dev) for a in (f, gin, rec, s, w, t, x, close)]
    pad = lambda nbytes: torch.zeros(nbytes + 32, dtype=torch.uint8, device=dev)  # noqa: E731
    out, fd, gate, res, ws = pad(256), pad(64), pad(192), pad(64), pad(64)
    q = [a.data_ptr() for a in ten]
    ok = (q[0], q[1], q[2], rec.size, q[3], q[4], q[5], q[6], 4, q[7], now, out.data_ptr(), fd.data_ptr(),
          gate.data_ptr(), res.data_ptr(), ws.data_ptr(), None)
    L = lvlip.lib()
    for i, off in ((0, 4), (1, 8), (2, 8), (4, 4), (5, 4), (6, 4), (7, 4), (12, 8), (13, 8), (14, 8), (15, 8)):
        bad = list(ok)
        bad[i] += off
        assert L.lvlip_fin_dev(*bad) == lvlip.EINVAL, i
    for i in (0, 1, 2, 4, 5, 6, 7, 11, 12, 13, 14, 15):
        bad = list(ok)
        bad[i] = None
        assert L.lvlip_fin_dev(*bad) == lvlip.EINVAL, i
    bad = list(ok)
    bad[13] = q[1]
    assert L.lvlip_fin_dev(*bad) == lvlip.EINVAL, "gate == gin"
    torch.cuda.synchronize(dev)
    assert not any(a.any().item() for a in (out, fd, gate, res, ws))
    for a, b in zip((f, s, x), (ten[0], ten[3], ten[6])):
        assert np.array_equal(b.cpu().numpy(), a.view(np.uint8).reshape(-1))


# ------------------------------------------------------------- the whole loop --

def loop_dev(loop, want: dict, dev) -> dict:
    """FinLoop.run(True) through the device forms on ONE stream: no copy to the
    host, no synchronise and no host decision between the first launch and the
    last.  What the applications and the wire decide per round (when each side
    closes, the window B writes into its ACK template, which FINs and ACKs
    never arrive) is taken from the CPU loop and uploaded beforehand; the
    network's loss of data frames is a torch operation on the same stream, and
    so is copying snd_nxt into the ACK templates."""
    from test_fin_cpu import CLOSE_AT
    from test_rto_cpu import TICK

    p = loop.p
    b, n = p.base, p.n
    L, nrtx, npush = b.link, p.nslots_rtx, p.nslots
    rounds, log = want["rounds"], want["log"]
    fb, fa, snd, tmpl, pay = (_t(a, dev) for a in (b.fb, L.fa, p.snd, L.tmpl, L.payload))
    w0 = p.w.copy()
    w0["wnd"] = b.wnd
    tmpl_a0 = np.concatenate([lvlip.ack_tmpl(w0["hdr"][k].tobytes(), out_off=5 + 91 * k, max_sack=0) for k in range(n)])
    tmpl_a0["hdr"][:, 47] = 0x10
    snd_b0 = np.zeros(n, dtype=S)
    snd_b0["snd_una"] = snd_b0["snd_nxt"] = L.fa["rcv_nxt"]
    snd_b0["seg0"] = np.arange(n)
    w_b0 = np.concatenate([lvlip.push_flow(L.tmpl["hdr"][k].tobytes(), 0, 0, p.mss, 0, 1, k, 1) for k in range(n)])
    ack_a_bytes = lvlip.ack_plan(tmpl_a0, L.fa)
    w, t = _t(w0, dev), _t(lvlip.rto_flows(n, snd_wnd=b.wnd), dev)
    tmpl_a, snd_b, w_b, t_b = _t(tmpl_a0, dev), _t(snd_b0, dev), _t(w_b0, dev), _t(lvlip.rto_flows(n), dev)
    xa, xb = _t(lvlip.fin_flows(L.fa), dev), _t(lvlip.fin_flows(b.fb), dev)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)  # noqa: E731
    wnds, drops, drop_fin = up(log["wnd"], np.int64), up(log["drop"], bool), up(log["drop_fin"], bool)
    close_b = up(log["close_b"], np.uint8)
    close_a = up(np.repeat((np.arange(rounds) >= CLOSE_AT)[:, None], n, 1), np.uint8)
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
    ring = torch.full((p.ring_bytes + 64,), CANARY, dtype=torch.uint8, device=dev)
    fd, sacked = guarded(16 * p.nfd, dev), guarded(p.nfd, dev)
    fd[:16 * p.nfd] = 0
    sacked[:p.nfd] = 0
    stream_t = torch.full((L.stream.size,), CANARY, dtype=torch.uint8, device=dev)
    res, ares, sres, bres = z(48 * n), z(48 * n), z(32 * n), z(32 * n)
    kres, pres, wres, rres, gate = z(16 * n), z(16 * n), z(16 * n), z(16 * n), z(32 * n)
    gate_a, gate_b = guarded(48 * n, dev), guarded(48 * n, dev)
    ra, rb = guarded(16 * n * rounds, dev), guarded(16 * n * rounds, dev)  # every round's lvlip_fin_result
    sent = torch.zeros(n * p.segs, dtype=torch.int32, device=dev)
    nw = npush + nrtx
    rec = guarded(16 * (nw + 2 * n), dev)
    arec = guarded(16 * 2 * n, dev)
    pfd, fd_out, pick, wire = z(16 * npush), z(16 * nrtx), z(4 * nrtx), z(16 * nw)
    fin_a = torch.full((64 * n + 64,), CANARY, dtype=torch.uint8, device=dev)
    ffd_a, afd_a = z(16 * n), z(16 * n)
    ack_a = torch.full((ack_a_bytes,), CANARY, dtype=torch.uint8, device=dev)
    both = torch.full((L.ack_bytes + 64 * n + 64,), CANARY, dtype=torch.uint8, device=dev)  # B's ACKs, then B's FINs
    ack, fin_b = both[:L.ack_bytes], both[L.ack_bytes:L.ack_bytes + 64 * n]
    both_fd = z(16 * 2 * n)
    afd, ffd_b = both_fd[:16 * n], both_fd[16 * n:]
    sink, no_ring, no_fd = z(n + 64), z(64), z(16 * n)
    ws_a = torch.empty(lvlip.lro_advance_carry_workspace_bytes(2 * n, n), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(lvlip.lro_advance_carry_workspace_bytes(nw + 2 * n, n), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(max(lvlip.sack_workspace_bytes(2 * n, n), 256), dtype=torch.uint8, device=dev)
    ws_fa, ws_fb = guarded(lvlip.fin_workspace_bytes(n), dev), guarded(lvlip.fin_workspace_bytes(n), dev)
    nws = lvlip.fin_workspace_bytes(n)
    fb32 = fb.view(torch.int32).view(n, 12)        # rcv_wnd is word 4
    tm, tm_a = tmpl.view(n, 64), tmpl_a.view(n, 64)  # hdr at byte 8: seq at 8 + 38, the window at 8 + 48
    snd8, snd_b8 = snd.view(n, 32), snd_b.view(n, 32)  # snd_nxt is bytes 4 .. 7, win bytes 24 .. 25
    afd32, ffd_a32 = afd.view(torch.int32).view(n, 4), ffd_a.view(torch.int32).view(n, 4)  # len is word 2
    both64 = both_fd.view(torch.int64).view(2 * n, 2)  # offset is word 0
    iss = torch.from_numpy(p.iss).to(dev)
    flow = torch.cat([torch.arange(npush, device=dev) // p.rtx, torch.arange(nrtx, device=dev) // p.rtx])
    first = torch.arange(nw, device=dev) < npush
    four = torch.arange(4, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        for r in range(rounds):
            now = (r + 1) * TICK
            # A
            lvlip.push_dev(fa, None, snd, w, npush, pay, ring, fd[:16 * p.nfd], sacked[:p.nfd], pfd, pres, stream=s)
            lvlip.rto_dev(snd, sres, pres, t, now, lvlip.RTO_FAST, sacked[:p.nfd], gate, rres, stream=s)
            if r:
                lvlip.lro_advance_carry_dev(fa, arec[:32 * n], ares, ares, ws_a, stream=s)
            lvlip.lro_next_dev(fa, ares, stream=s)
            lvlip.fin_dev(fa, ares, arec[:32 * n] if r else None, snd, w, t, xa, close_a[r], now, fin_a[:64 * n],
                          gate_a[:48 * n], ws_fa[:nws], ffd_a, ra[16 * n * r:16 * n * (r + 1)], stream=s)
            tm_a[:, 46:50] = snd8[:, 4:8].flip(1)
            lvlip.ack_dev(tmpl_a, fa, gate_a[:48 * n], 0, ack_a, afd_a, stream=s)
            lvlip.rtx_sack_dev(fa, None, snd, gate, sacked[:p.nfd], nrtx, ring, fd[:16 * p.nfd], fd_out, pick, stream=s)
            # the network: stream segment 4 mod 5 of a flow is lost when lvlip_push_* sends it; a first FIN is lost
            wire[:16 * npush] = pfd
            wire[16 * npush:] = fd_out
            fo = wire.view(torch.int64).view(nw, 2)
            live = (fo[:, 1] & 0xFFFFFFFF) > 0
            by = ring[fo[:, 0:1] + 38 + four].to(torch.int64)
            seq = (by[:, 0] << 24) | (by[:, 1] << 16) | (by[:, 2] << 8) | by[:, 3]
            seg = (((seq - iss[flow]) & 0xFFFFFFFF) // p.mss).clamp(0, p.segs - 1)
            lost = live & first & (seg % 5 == 4)
            sent.index_put_((flow * p.segs + seg,), live.to(torch.int32), accumulate=True)
            w32 = wire.view(torch.int32).view(nw, 4)
            w32[:, 2] = torch.where(lost, torch.zeros_like(w32[:, 2]), w32[:, 2])
            ffd_a32[:, 2] = torch.where(drop_fin[r], torch.zeros_like(ffd_a32[:, 2]), ffd_a32[:, 2])
            # B: the ring's frames, A's FINs and A's ACKs, one record array
            lvlip.lro_dev(ring, wire, fb, lvlip.RX_VERIFY_L4, stream_t, rec[:16 * nw], stream=s)
            lvlip.lro_dev(fin_a, ffd_a, fb, lvlip.RX_VERIFY_L4, stream_t, rec[16 * nw:16 * (nw + n)], stream=s)
            lvlip.lro_dev(ack_a, afd_a, fb, lvlip.RX_VERIFY_L4, stream_t, rec[16 * (nw + n):16 * (nw + 2 * n)], stream=s)
            recs = rec[:16 * (nw + 2 * n)]
            lvlip.lro_advance_carry_dev(fb, recs, res, res, ws_b, stream=s)
            hi, lo = (wnds[r] >> 8).to(torch.uint8), (wnds[r] & 0xFF).to(torch.uint8)
            tm[:, 56], tm[:, 57] = hi, lo
            snd_b8[:, 24], snd_b8[:, 25] = lo, hi
            lvlip.snd_dev(fb, snd_b, recs, no_ring, no_fd, bres, stream=s)
            lvlip.snd_next_dev(snd_b, bres, stream=s)
            lvlip.lro_next_dev(fb, res, stream=s)
            lvlip.fin_dev(fb, res, recs, snd_b, w_b, t_b, xb, close_b[r], now, fin_b, gate_b[:48 * n], ws_fb[:nws], ffd_b,
                          rb[16 * n * r:16 * n * (r + 1)], stream=s)
            tm[:, 46:50] = snd_b8[:, 4:8].flip(1)
            lvlip.ack_dev(tmpl, fb, gate_b[:48 * n], lvlip.ACK_ALL, ack, afd, stream=s)
            fb32[:, 4] = wnds[r].to(torch.int32)
            afd32[:, 2] = torch.where(drops[r], torch.zeros_like(afd32[:, 2]), afd32[:, 2])
            both64[n:, 0] += L.ack_bytes
            # A: B's ACKs and B's FINs, one buffer and one record array
            lvlip.lro_dev(both, both_fd, fa, lvlip.RX_VERIFY_L4, sink, arec[:32 * n], stream=s)
            lvlip.snd_dev(fa, snd, arec[:32 * n], ring, fd[:16 * p.nfd], sres, stream=s)
            lvlip.sack_dev(fa, snd, arec[:32 * n], both, both_fd, ring, fd[:16 * p.nfd], sacked[:p.nfd], kres, ws2, stream=s)
            lvlip.wnd_dev(fa, snd, t, w, arec[:32 * n], both, both_fd, lvlip.WND_APPLY, wres, stream=s)
            lvlip.snd_next_dev(snd, sres, stream=s)
    s.synchronize()  # the only one
    assert (ring[p.ring_bytes:] == CANARY).all(), "written behind the ring"
    assert (fin_a[64 * n:] == CANARY).all() and (both[L.ack_bytes + 64 * n:] == CANARY).all(), "written behind the FINs"
    for g in (rec, arec, gate_a, gate_b, ws_fa, ws_fb):
        assert (g[-devbuf.GUARD:] == CANARY).all(), "written behind a guarded array"
    h = lambda q, dt=np.uint8: q.cpu().numpy().view(dt)  # noqa: E731
    return dict(stream=h(stream_t), fb=h(fb, F), fa=h(fa, F), snd=h(snd, S), snd_b=h(snd_b, S),
                w=h(w, lvlip.PUSH_FLOW_DTYPE), res=h(res, G), ares=h(ares, G), ring=h(ring)[:p.ring_bytes],
                fd=unguard(fd, 16 * p.nfd, FD), sacked=unguard(sacked, p.nfd, np.uint8), sent=h(sent, np.int32),
                t=h(t, lvlip.RTO_FLOW_DTYPE), xa=h(xa, X), xb=h(xb, X), fin_a=h(fin_a)[:64 * n], fin_b=h(fin_b),
                ra=unguard(ra, 16 * n * rounds, R).reshape(rounds, n), rb=unguard(rb, 16 * n * rounds, R).reshape(rounds, n))


def test_the_close_loop_on_one_stream(dev):
    """8 flows x 40 x 536 B with loss, then both sides close, with lost FINs
    and a lost ACK of a FIN: as many rounds as the CPU loop needed, one
    synchronise.  All 16 endpoints are CLOSED; state, stream bytes, the FINs'
    buffers and every round's lvlip_fin_result at both ends equal the CPU
    loop's."""
    from test_fin_cpu import fin_loop_cpu

    loop, want = fin_loop_cpu()
    got = loop_dev(loop, want, dev)
    assert (got["xa"]["state"] == CLOSED).all() and (got["xb"]["state"] == CLOSED).all()
    for k in ("stream", "fb", "fa", "snd", "snd_b", "w", "res", "ares", "ring", "fd", "sacked", "sent", "t", "xa", "xb",
              "fin_a", "fin_b"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["ra"].tobytes() == want["log"]["ra"].tobytes(), "every round's lvlip_fin_result at A"
    assert got["rb"].tobytes() == want["log"]["rb"].tobytes(), "every round's lvlip_fin_result at B"
    assert (got["ra"]["events"] & RESENT).any() and (got["rb"]["events"] & PEER_FIN).any()
