"""The write queue on the MI355X (push_kernels.hip): lvlip_push_dev against
lvlip_push_cpu in every byte of every output, on the cases of
tests/test_push_cpu.py and on shapes the kernels care about (the compaction's
64-entry chunks, every alignment of ring and payload, a segment of several
sweeps of a row, 65 536 flows); determinism; and the whole loop with a ring of
16 slots per flow queued on one stream with a single synchronise at its end,
against the same loop on the CPU forms."""
import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import CANARY, _t, guarded, unguard
from test_push_cpu import (CASES, FD, NO_LIMIT, PUSH_ROUNDS, PushCase, PushLoop, assert_outputs, make_case, push_loop_cpu,
                           random_specs, run_cpu)
from test_tso_cpu import template

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


def run_dev(c: PushCase, dev, stream=None) -> dict:
    """lvlip_push_dev on copies, canaries behind every output; what is only
    read is compared afterwards."""
    n = c.w.size
    f_t, pay_t = _t(c.f, dev), _t(c.payload, dev)
    lro_t = None if c.lro is None else _t(c.lro, dev)
    sk_t = None if c.sacked is None else torch.cat([_t(c.sacked, dev), guarded(0, dev)])
    s_t, w_t, fd_t = (torch.cat([_t(a, dev), guarded(0, dev)]) for a in (c.snd, c.w, c.fd))
    ring_t = _t(c.ring, dev)
    out_t, res_t = guarded(16 * c.nslots, dev), guarded(16 * n, dev)
    torch.cuda.synchronize(dev)
    lvlip.push_dev(f_t, lro_t, s_t, w_t, c.nslots, pay_t, ring_t, fd_t, sk_t, out_t, res_t, stream=stream)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    assert np.array_equal(f_t.cpu().numpy(), c.f.view(np.uint8).reshape(-1)), "f is only read"
    assert np.array_equal(pay_t.cpu().numpy(), c.payload), "the payload is only read"
    assert c.lro is None or np.array_equal(lro_t.cpu().numpy(), c.lro.view(np.uint8).reshape(-1)), "lro is only read"
    return dict(ring=ring_t.cpu().numpy(), fd=unguard(fd_t, c.fd.nbytes, FD),
                sacked=None if c.sacked is None else unguard(sk_t, c.sacked.size, np.uint8),
                fd_out=unguard(out_t, 16 * c.nslots, FD), snd=unguard(s_t, c.snd.nbytes, lvlip.SND_FLOW_DTYPE),
                w=unguard(w_t, c.w.nbytes, lvlip.PUSH_FLOW_DTYPE), res=unguard(res_t, 16 * n, lvlip.PUSH_RESULT_DTYPE))


@pytest.mark.parametrize("make", CASES)
def test_dev_equals_cpu_on_the_models_cases(make, dev):
    c = make()
    assert_outputs(run_dev(c, dev), run_cpu(c))


def test_300_flows(dev):
    c = make_case(random_specs(300, 7), seed=7)
    want = run_cpu(c)
    assert int((want["res"]["pushed"] > 0).sum()) > 50 and int((want["res"]["moved"] > 0).sum()) > 50
    assert_outputs(run_dev(c, dev), want)


@pytest.mark.parametrize("shift", (1, 64, 70))
def test_compaction_chunk_boundaries(shift, dev):
    """Queues of 63, 64, 65 and 129 entries moved down by less than, exactly
    and more than a chunk: source and destination overlap."""
    specs = [dict(mss=7, cap=200, nseg=q, shift=shift, slot_nxt=199, push=3, unsent=100, span=0, wnd=NO_LIMIT, una=k)
             for k, q in enumerate((63, 64, 65, 129, 0, 1))]
    c = make_case(specs, seed=shift)
    want = run_cpu(c)
    assert want["res"]["moved"].tolist() == [63, 64, 65, 129, 0, 1] and (want["res"]["pushed"] == 3).all()
    assert_outputs(run_dev(c, dev), want)


def test_every_alignment_of_ring_and_payload(dev):
    """All 16 values of ring_off mod 16 and of pay_off mod 16, odd strides."""
    seen_r, seen_p = set(), set()
    for r in range(16):
        specs = [dict(mss=m, cap=5, nseg=1, shift=2, slot_nxt=3, push=4, unsent=3 * m + m // 2 + 1, span=0, wnd=NO_LIMIT,
                      una=r) for m in (536, 1460, 8, 34)]
        c = make_case(specs, seed=r, ring_mod=r, pay_mod=(7 * r + 1) % 16)
        assert (c.w["stride"] % 2 == 1).all()
        seen_r.add(int(c.w["ring_off"][0]) % 16), seen_p.add(int(c.w["pay_off"][0]) % 16)
        assert_outputs(run_dev(c, dev), run_cpu(c), f"ring_off mod 16 = {r}: ")
    assert len(seen_r) == 16 and len(seen_p) == 16


def test_mss_8960(dev):
    """Several sweeps of a row per frame, the last segment short."""
    specs = [dict(mss=8960, cap=5, nseg=1, shift=1, slot_nxt=4, push=5, unsent=3 * 8960 + 100, span=0, wnd=NO_LIMIT, una=1),
             dict(mss=8960, cap=2, nseg=0, shift=0, slot_nxt=1, push=2, unsent=8960, span=0, wnd=NO_LIMIT, una=2)]
    c = make_case(specs, seed=2)
    want = run_cpu(c)
    assert want["res"]["pushed"].tolist() == [4, 1]
    assert_outputs(run_dev(c, dev), want)


def many_flows(n: int = 65536) -> PushCase:
    """n flows with push 1 and mss 8, laid out with array arithmetic."""
    k = np.arange(n, dtype=np.uint64)
    f = np.zeros(n, dtype=lvlip.LRO_FLOW_DTYPE)
    f["rcv_nxt"] = (k * 2654435761) & 0xFFFFFFFF
    snd = np.zeros(n, dtype=lvlip.SND_FLOW_DTYPE)
    w = np.zeros(n, dtype=lvlip.PUSH_FLOW_DTYPE)
    w["hdr"][:] = np.frombuffer(template(), dtype=np.uint8)
    w["mss"], w["cap"], w["push"], w["stride"], w["wnd"] = 8, 2, 1, 63, NO_LIMIT
    w["q0"], w["ring_off"], w["pay_off"] = 2 * k, 3 + 126 * k, 20 * k + 1
    w["unsent"], w["slot_nxt"] = k % 20, k % 2
    snd["snd_una"] = snd["snd_nxt"] = (k * 40503) & 0xFFFFFFFF
    snd["nseg"] = k % 3 % 2          # 0, 1, 0, 0, 1, 0: an entry in a third of the queues
    snd["seg0"] = w["q0"] + (k % 2)  # some of them one above q0
    snd["win"] = k % 65536
    rng = np.random.default_rng(5)
    fd = np.zeros(2 * n, dtype=FD)
    fd["offset"], fd["len"] = np.arange(2 * n) + 7, 62
    return PushCase(f, None, snd, w, rng.integers(0, 256, 20 * n + 32, dtype=np.uint8),
                    np.full(3 + 126 * n + 64, 0xA5, dtype=np.uint8), fd, rng.integers(0, 2, 2 * n, dtype=np.uint8))


def test_65536_flows(dev):
    c = many_flows()
    assert c.nslots == 65536
    want = run_cpu(c)
    assert int(want["res"]["pushed"].sum()) > 50000 and int(want["res"]["moved"].sum()) > 5000
    assert_outputs(run_dev(c, dev), want)


def test_determinism(dev):
    """The same call twice on fresh copies, and with the flows permuted in
    memory (the regions stay where they are; the plan numbers the slots
    afresh): identical bytes."""
    c = make_case(random_specs(17, 2), seed=2)
    a, b = run_dev(c, dev), run_dev(c, dev)
    assert_outputs(b, a)
    perm = np.random.default_rng(0).permutation(17)
    p = c.copy()
    p.f, p.lro, p.snd, p.w = c.f[perm].copy(), c.lro[perm].copy(), c.snd[perm].copy(), c.w[perm].copy()
    p.nslots = lvlip.push_plan(p.w, p.snd)[0]
    got = run_dev(p, dev)
    for k in ("ring", "fd", "sacked"):
        assert got[k].tobytes() == a[k].tobytes(), k
    assert got["res"].tobytes() == a["res"][perm].tobytes() and got["snd"].tobytes() == a["snd"][perm].tobytes()
    back = got["w"].copy()
    back["slot0"] = c.w["slot0"][perm]
    assert back.tobytes() == a["w"][perm].tobytes()
    for k in range(17):  # a flow's slots hold the same descriptors wherever the plan put them
        n, s0, s1 = int(p.w[k]["push"]), int(p.w[k]["slot0"]), int(c.w[perm[k]]["slot0"])
        assert got["fd_out"][s0:s0 + n].tobytes() == a["fd_out"][s1:s1 + n].tobytes()


# ------------------------------------------------------------- the whole loop --

def loop_dev(loop: PushLoop, dev) -> dict:
    """PushLoop.run_cpu's rounds through the device forms on ONE stream: no
    copy to the host, no synchronise and no host decision between the first
    launch and the last.  The network and the application's window update are
    torch operations on the same stream."""
    b, n = loop.base, loop.n
    L, nrtx = b.link, loop.nslots_rtx
    fb, fa, snd, w, tmpl, pay = (_t(a, dev) for a in (b.fb, L.fa, loop.snd, loop.w, L.tmpl, L.payload))
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
    ring = torch.full((loop.ring_bytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
    fd, sacked = guarded(16 * loop.nfd, dev), guarded(loop.nfd, dev)
    fd[:16 * loop.nfd] = 0
    sacked[:loop.nfd] = 0
    stream_t = torch.full((L.stream.size,), 0xA5, dtype=torch.uint8, device=dev)
    res, sres, kres, pres = z(48 * n), z(32 * n), z(16 * n), z(16 * n)
    sent = torch.zeros(n * loop.segs, dtype=torch.int32, device=dev)
    rec, arec, afd = guarded(16 * nrtx, dev), z(16 * n), z(16 * n)
    pfd, fd_out, pick, wire = z(16 * loop.nslots), z(16 * nrtx), z(4 * nrtx), z(16 * nrtx)
    ack, sink = z(L.ack_bytes), z(n + 64)
    ws = torch.empty(lvlip.lro_advance_carry_workspace_bytes(nrtx, n), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(max(lvlip.sack_workspace_bytes(n, n), 256), dtype=torch.uint8, device=dev)
    end_lo = torch.from_numpy((b.end & 0xFFFFFFFF).astype(np.int64)).to(dev)
    fb32 = fb.view(torch.int32).view(n, 12)  # rcv_wnd is word 4, out_off's low word 6 (every offset is below 2^31)
    iss = torch.from_numpy(loop.iss).to(dev)
    flow = torch.arange(nrtx, device=dev) // loop.rtx
    four = torch.arange(4, device=dev)
    pushed = torch.zeros((), dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        for _ in range(PUSH_ROUNDS):
            lvlip.push_dev(fa, None, snd, w, loop.nslots, pay, ring, fd[:16 * loop.nfd], sacked[:loop.nfd], pfd, pres,
                           stream=s)
            pushed += pres.view(torch.int32).view(n, 4)[:, 0].sum()
            lvlip.rtx_sack_dev(fa, None, snd, sres, sacked[:loop.nfd], nrtx, ring, fd[:16 * loop.nfd], fd_out, pick,
                               stream=s)
            # the network: stream segment 4 mod 5 of a flow is lost the first time it goes out
            fo = fd_out.view(torch.int64).view(nrtx, 2)
            live = (fo[:, 1] & 0xFFFFFFFF) > 0
            by = ring[fo[:, 0:1] + 38 + four].to(torch.int64)
            seq = (by[:, 0] << 24) | (by[:, 1] << 16) | (by[:, 2] << 8) | by[:, 3]
            seg = (((seq - iss[flow]) & 0xFFFFFFFF) // loop.mss).clamp(0, loop.segs - 1)
            idx = flow * loop.segs + seg
            lost = live & (sent[idx] == 0) & (seg % 5 == 4)
            sent.index_put_((idx,), live.to(torch.int32), accumulate=True)
            wire.copy_(fd_out)
            w32 = wire.view(torch.int32).view(nrtx, 4)
            w32[:, 2] = torch.where(lost, torch.zeros_like(w32[:, 2]), w32[:, 2])
            # B
            lvlip.lro_dev(ring, wire, fb, lvlip.RX_VERIFY_L4, stream_t, rec[:16 * nrtx], stream=s)
            lvlip.lro_advance_carry_dev(fb, rec[:16 * nrtx], res, res, ws, stream=s)
            lvlip.ack_dev(tmpl, fb, res, lvlip.ACK_ALL, ack, afd, stream=s)
            lvlip.lro_next_dev(fb, res, stream=s)
            fb32[:, 4] = torch.minimum(torch.full_like(end_lo, b.wnd), end_lo - fb32[:, 6]).to(torch.int32)
            # A
            lvlip.lro_dev(ack, afd, fa, lvlip.RX_VERIFY_L4, sink, arec, stream=s)
            lvlip.snd_dev(fa, snd, arec, ring, fd[:16 * loop.nfd], sres, stream=s)
            lvlip.sack_dev(fa, snd, arec, ack, afd, ring, fd[:16 * loop.nfd], sacked[:loop.nfd], kres, ws2, stream=s)
            lvlip.snd_next_dev(snd, sres, stream=s)
    s.synchronize()  # the only one
    assert (rec[16 * nrtx:] == CANARY).all(), "written behind one round's records"
    assert (ring[loop.ring_bytes:] == 0xA5).all(), "written behind the ring of 16 slots per flow"
    h = lambda t, dt=np.uint8: t.cpu().numpy().view(dt)  # noqa: E731
    return dict(stream=h(stream_t), fb=h(fb, lvlip.LRO_FLOW_DTYPE), snd=h(snd, lvlip.SND_FLOW_DTYPE),
                w=h(w, lvlip.PUSH_FLOW_DTYPE), res=h(res, lvlip.LRO_RESULT_DTYPE), sres=h(sres, lvlip.SND_RESULT_DTYPE),
                ring=h(ring)[:loop.ring_bytes], fd=unguard(fd, 16 * loop.nfd, FD), sacked=unguard(sacked, loop.nfd, np.uint8),
                sent=h(sent, np.int32), pres=h(pres, lvlip.PUSH_RESULT_DTYPE), pushed=int(pushed.item()))


def test_the_loop_with_a_ring_of_16_slots_on_one_stream(dev):
    """8 flows x 40 segments through 16 ring slots per flow, every fifth first
    transmission lost: 48 rounds of push, selective retransmit, receive, ACK,
    ACK side and steps queued on one stream, one synchronise.  Afterwards every
    stream holds its payload, every queue is empty, and every byte of the ring,
    the state and the results equals the CPU forms'."""
    loop, want = push_loop_cpu()
    got = loop_dev(loop, dev)
    loop.check_done(got)
    for k in ("stream", "fb", "snd", "w", "res", "sres", "ring", "fd", "sacked", "sent", "pres"):
        assert got[k].tobytes() == want[k].tobytes(), k
