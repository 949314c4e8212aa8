"""The persist timer on the MI355X (k_persist, persist_kernels.hip): every byte
of p, t, res, fd_out and out of lvlip_persist_dev against lvlip_persist_cpu
(which tests/test_persist_cpu.py holds to a plain restatement), at the flow
counts around a lane group's eight flows per wave and 32 per workgroup (the
mapping is k_ack's: eight lanes per flow), with `out` at every address mod 16;
and the loop with a receiver that stops reading, queued on one stream with one
synchronise."""
import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import CANARY, _t, guarded, unguard
from persist_model import random_case
from test_persist_cpu import CLOSE1, persist_loop_cpu
from test_rto_cpu import TICK

pytestmark = pytest.mark.gpu
P, R, FD, T = lvlip.PERSIST_FLOW_DTYPE, lvlip.PERSIST_RESULT_DTYPE, lvlip.FRAME_DESC_DTYPE, lvlip.RTO_FLOW_DTYPE


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


def run_both(dev, f, lro, s, w, t, p, now, shift=0):
    """Both forms from the same bytes; `out` starts `shift` bytes into a 256-B
    aligned buffer of canary bytes.  Returns the CPU form's (t, p, out, fd, res)."""
    n = s.size
    tc, pc = t.copy(), p.copy()
    out, fd, res = lvlip.persist_cpu(f, lro, s, w, tc, pc, now, np.full(64 * n, CANARY, dtype=np.uint8))
    ins = [_t(a, dev) for a in (f, s, w)]
    lro_t = None if lro is None else _t(lro, dev)
    t_t, p_t = torch.cat([_t(t, dev), guarded(0, dev)]), torch.cat([_t(p, dev), guarded(0, dev)])
    buf = devbuf.guarded_aligned(shift + 64 * n, dev)
    fd_t, res_t = guarded(16 * n, dev), guarded(16 * n, dev)
    torch.cuda.synchronize(dev)
    lvlip.persist_dev(ins[0], lro_t, ins[1], ins[2], t_t, p_t, now, buf[shift:], fd_t, res_t)
    torch.cuda.synchronize(dev)
    for a, x in zip((f, s, w), ins):
        assert np.array_equal(x.cpu().numpy(), a.view(np.uint8).reshape(-1)), "f, s and w are only read"
    assert unguard(t_t, t.nbytes, T).tobytes() == tc.tobytes(), "t"
    assert unguard(p_t, p.nbytes, P).tobytes() == pc.tobytes(), "p"
    assert unguard(res_t, 16 * n, R).tobytes() == res.tobytes(), "res"
    assert unguard(fd_t, 16 * n, FD).tobytes() == fd.tobytes(), "fd_out"
    got = buf.cpu().numpy()
    assert (got[:shift] == CANARY).all() and (got[shift + 64 * n:] == CANARY).all(), "written around out"
    assert got[shift:shift + 64 * n].tobytes() == out.tobytes(), "out"
    return tc, pc, out, fd, res


@pytest.mark.parametrize("nflows", (1, 7, 8, 9, 31, 32, 33, 64, 257))
def test_dev_equals_cpu(nflows, dev):
    fired = 0
    for seed in (0, 1):
        case = random_case(nflows, seed + 10 * nflows)
        fired += int(run_both(dev, *case, shift=(3 * nflows + 5 * seed) % 16)[4]["fired"].sum())
    assert fired or nflows == 1, "the cases are fixed by their seeds: flows fire at every count but 1"
    case = random_case(nflows, 7 + nflows)
    run_both(dev, case[0], None, *case[2:])  # lro == NULL


def all_or_none(n, fire):
    f, lro, s, w, t, p, now = random_case(n, 11)
    s["nseg"], t["dead"], w["unsent"], w["wnd"] = 0, 0, 5000, 0
    w["mss"] = 536
    p["armed"], p["interval"], p["probes"] = 1, 1000, 2
    p["expires"] = now - 1 if fire else now
    return f, lro, s, w, t, p, now


def test_out_at_every_address_mod_16(dev):
    """Silent flows between fired ones, so a store past a frame's 54 bytes or
    into a neighbour's slot shows at every offset of the first chunk."""
    case = all_or_none(40, True)
    case[5]["expires"][::3] = case[6]
    for shift in range(16):
        assert run_both(dev, *case, shift=shift)[4]["fired"].sum() == 26


def test_all_fired_and_none_fired(dev):
    res = run_both(dev, *all_or_none(70, True), shift=9)[4]
    assert res["fired"].all() and (res["probes"] == 3).all()
    _, _, out, fd, res = run_both(dev, *all_or_none(70, False), shift=9)
    assert not res["fired"].any() and not fd["len"].any() and (out == CANARY).all(), "out is untouched"


def test_two_runs_give_identical_bytes(dev):
    case = random_case(257, 4)
    a = run_both(dev, *case, shift=1)
    b = run_both(dev, *case, shift=1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_misaligned_pointers_are_refused_before_any_launch(dev):
    f, lro, s, w, t, p, now = random_case(4, 1)
    ten = [_t(a, dev) for a in (f, lro, s, w, t, p)]
    pad = lambda nbytes: torch.zeros(nbytes + 32, dtype=torch.uint8, device=dev)  # noqa: E731
    out, fd, res = pad(256), pad(64), pad(64)
    q = [x.data_ptr() for x in ten]
    ok = (*q, 4, now, out.data_ptr(), fd.data_ptr(), res.data_ptr(), None)
    for i, off in ((0, 4), (1, 8), (2, 4), (3, 4), (4, 4), (5, 4), (9, 8), (10, 8)):
        bad = list(ok)
        bad[i] += off
        assert lvlip.lib().lvlip_persist_dev(*bad) == lvlip.EINVAL, i
    torch.cuda.synchronize(dev)
    assert not out.any().item() and not fd.any().item() and not res.any().item()
    for a, x in zip((t, p), ten[4:]):
        assert np.array_equal(x.cpu().numpy(), a.view(np.uint8).reshape(-1))


# ------------------------------------------------------------- the whole loop --

def loop_dev(loop, want: dict, dev) -> dict:
    """PersistLoop.run(True) through the device forms on ONE stream: no copy to
    the host, no synchronise and no host decision between the first launch and
    the last.  What the receiving application and the wire decide per round
    (the window the receiver writes into its ACK template and which ACKs never
    arrive) is taken from the CPU loop and uploaded beforehand; the network's
    loss of data frames is a torch operation on the same stream."""
    p = loop.p
    b, n = p.base, p.n
    L, nrtx, npush = b.link, p.nslots_rtx, p.nslots
    rounds = want["rounds"]
    fb, fa, snd, tmpl, pay = (_t(a, dev) for a in (b.fb, L.fa, p.snd, L.tmpl, L.payload))
    w0 = p.w.copy()
    w0["wnd"] = b.wnd
    w, t, pst = _t(w0, dev), _t(lvlip.rto_flows(n, snd_wnd=b.wnd), dev), _t(lvlip.persist_flows(n), dev)
    wnds = torch.from_numpy(want["log"]["wnd"].astype(np.int64)).to(dev)  # [rounds, n]
    drops = torch.from_numpy(want["log"]["drop"]).to(dev)
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
    ring = torch.full((p.ring_bytes + 64,), CANARY, dtype=torch.uint8, device=dev)
    probe = guarded(64 * n, dev)
    fd, sacked = guarded(16 * p.nfd, dev), guarded(p.nfd, dev)
    fd[:16 * p.nfd] = 0
    sacked[:p.nfd] = 0
    stream_t = torch.full((L.stream.size,), CANARY, dtype=torch.uint8, device=dev)
    res, sres, kres, pres, wres, rres, gate = z(48 * n), z(32 * n), z(16 * n), z(16 * n), z(16 * n), z(16 * n), z(32 * n)
    bres = guarded(16 * n * rounds, dev)  # every round's lvlip_persist_result
    sent = torch.zeros(n * p.segs, dtype=torch.int32, device=dev)
    nw = npush + nrtx
    rec, arec, afd, bfd = guarded(16 * (nw + n), dev), z(16 * n), z(16 * n), z(16 * n)
    pfd, fd_out, pick, wire = z(16 * npush), z(16 * nrtx), z(4 * nrtx), z(16 * nw)
    ack, sink = z(L.ack_bytes), z(n + 64)
    ws = torch.empty(lvlip.lro_advance_carry_workspace_bytes(nw + n, n), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(max(lvlip.sack_workspace_bytes(n, n), 256), dtype=torch.uint8, device=dev)
    fb32 = fb.view(torch.int32).view(n, 12)  # rcv_wnd is word 4
    tm = tmpl.view(n, 64)                     # hdr at byte 8: the window at 8 + 48
    afd32 = afd.view(torch.int32).view(n, 4)  # len is word 2
    iss = torch.from_numpy(p.iss).to(dev)
    flow = torch.cat([torch.arange(npush, device=dev) // p.rtx, torch.arange(nrtx, device=dev) // p.rtx])
    first = torch.arange(nw, device=dev) < npush
    four = torch.arange(4, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        for r in range(rounds):
            now = (r + 1) * TICK
            lvlip.push_dev(fa, None, snd, w, npush, pay, ring, fd[:16 * p.nfd], sacked[:p.nfd], pfd, pres, stream=s)
            lvlip.rto_dev(snd, sres, pres, t, now, lvlip.RTO_FAST, sacked[:p.nfd], gate, rres, stream=s)
            lvlip.persist_dev(fa, None, snd, w, t, pst, now, probe, bfd, bres[16 * n * r:16 * n * (r + 1)], stream=s)
            lvlip.rtx_sack_dev(fa, None, snd, gate, sacked[:p.nfd], nrtx, ring, fd[:16 * p.nfd], fd_out, pick, stream=s)
            # the network: stream segment 4 mod 5 of a flow is lost when lvlip_push_* sends it
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
            # B: the ring's frames and the probes, one record array
            lvlip.lro_dev(ring, wire, fb, lvlip.RX_VERIFY_L4, stream_t, rec[:16 * nw], stream=s)
            lvlip.lro_dev(probe, bfd, fb, lvlip.RX_VERIFY_L4, stream_t, rec[16 * nw:16 * (nw + n)], stream=s)
            lvlip.lro_advance_carry_dev(fb, rec[:16 * (nw + n)], res, res, ws, stream=s)
            tm[:, 56], tm[:, 57] = (wnds[r] >> 8).to(torch.uint8), (wnds[r] & 0xFF).to(torch.uint8)
            lvlip.ack_dev(tmpl, fb, res, lvlip.ACK_ALL, ack, afd, stream=s)
            lvlip.lro_next_dev(fb, res, stream=s)
            fb32[:, 4] = wnds[r].to(torch.int32)
            afd32[:, 2] = torch.where(drops[r], torch.zeros_like(afd32[:, 2]), afd32[:, 2])
            # A
            lvlip.lro_dev(ack, afd, fa, lvlip.RX_VERIFY_L4, sink, arec, stream=s)
            lvlip.snd_dev(fa, snd, arec, ring, fd[:16 * p.nfd], sres, stream=s)
            lvlip.sack_dev(fa, snd, arec, ack, afd, ring, fd[:16 * p.nfd], sacked[:p.nfd], kres, ws2, stream=s)
            lvlip.wnd_dev(fa, snd, t, w, arec, ack, afd, lvlip.WND_APPLY, wres, stream=s)
            lvlip.snd_next_dev(snd, sres, stream=s)
    s.synchronize()  # the only one
    assert (rec[16 * (nw + n):] == CANARY).all(), "written behind one round's records"
    assert (ring[p.ring_bytes:] == CANARY).all(), "written behind the ring"
    h = lambda x, dt=np.uint8: x.cpu().numpy().view(dt)  # noqa: E731
    return dict(stream=h(stream_t), fb=h(fb, lvlip.LRO_FLOW_DTYPE), snd=h(snd, lvlip.SND_FLOW_DTYPE),
                w=h(w, lvlip.PUSH_FLOW_DTYPE), res=h(res, lvlip.LRO_RESULT_DTYPE), sres=h(sres, lvlip.SND_RESULT_DTYPE),
                ring=h(ring)[:p.ring_bytes], fd=unguard(fd, 16 * p.nfd, FD), sacked=unguard(sacked, p.nfd, np.uint8),
                sent=h(sent, np.int32), t=h(t, T), pst=h(pst, P), wres=h(wres, lvlip.WND_RESULT_DTYPE),
                rres=h(rres, lvlip.RTO_RESULT_DTYPE), gate=h(gate, lvlip.SND_RESULT_DTYPE),
                probe=unguard(probe, 64 * n, np.uint8), bres=unguard(bres, 16 * n * rounds, R).reshape(rounds, n))


def test_the_loop_with_a_closed_window_on_one_stream(dev):
    """8 flows x 40 x 536 B, the receiver reads nothing for a stretch of rounds
    and its window update is lost: as many rounds as the CPU loop needed, one
    synchronise.  Every byte is delivered; state, stream bytes, the probes'
    buffer and every round's lvlip_persist_result equal the CPU loop's."""
    loop, want = persist_loop_cpu()
    assert want["rounds"] > CLOSE1
    got = loop_dev(loop, want, dev)
    loop.check_done(got)
    for k in ("stream", "fb", "snd", "w", "res", "sres", "ring", "fd", "sacked", "sent", "t", "pst", "wres", "rres",
              "gate", "probe"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["bres"].tobytes() == want["log"]["pres"].tobytes(), "every round's lvlip_persist_result"
    assert got["bres"]["fired"].any()
