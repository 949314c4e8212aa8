"""State across batches on the MI355X (adv_kernels.hip's carry form,
next_kernels.hip): lvlip_lro_advance_carry_dev, lvlip_lro_next_dev and
lvlip_snd_next_dev against their host twins byte for byte, on the cases of
tests/test_carry_cpu.py; what the calls may write; and the whole loop with loss
on one stream with a single synchronise at its end, against the same loop on
the CPU forms.

The record counts put n + 4 nflows on and beside an edge of adv_kernels.hip's
256-element scan tile (252 + 4 and 253 + 4 with one flow), and 1025 records end
a grid of five tiles on one lane."""
import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import ALIGNED_GUARD as GUARD, CANARY, _t, guarded_aligned as guarded
from test_carry_cpu import (ROUNDS, StreamLoop, assert_same, edge_cases, model_carry, random_case, step_inputs,
                            stream_loop_cpu)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


def carry_dev(flows, rec, prev, dev, in_place=False, stream=None) -> np.ndarray:
    """lvlip_lro_advance_carry_dev with canaries behind res and behind the
    workspace at the size the library asked for; f, rec and prev compared
    afterwards."""
    nflows, n = flows.size, rec.size
    fl_t, rec_t = _t(flows, dev), _t(rec, dev)
    need = lvlip.lro_advance_carry_workspace_bytes(n, nflows)
    assert need > 0 and need % 256 == 0 and need >= lvlip.lro_advance_workspace_bytes(n, nflows)
    ws_t, res_t = guarded(need, dev), guarded(48 * nflows, dev)
    prev_t = None
    if prev is not None:
        prev_t = res_t[:48 * nflows] if in_place else _t(prev, dev)
        if in_place:
            prev_t.copy_(_t(prev, dev))
    torch.cuda.synchronize(dev)
    got = lvlip.lro_advance_carry_dev(fl_t, rec_t if n else None, prev_t, res_t[:48 * nflows], ws_t[:need], stream=stream)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    assert got.data_ptr() == res_t.data_ptr()
    assert (ws_t[need:] == CANARY).all(), "written behind the workspace"
    assert (res_t[48 * nflows:] == CANARY).all(), "written behind res"
    assert np.array_equal(rec_t.cpu().numpy(), rec.view(np.uint8).reshape(-1)), "rec is only read"
    assert np.array_equal(fl_t.cpu().numpy(), flows.view(np.uint8).reshape(-1)), "f is only read"
    if prev is not None and not in_place:
        assert np.array_equal(prev_t.cpu().numpy(), prev.view(np.uint8).reshape(-1)), "prev is only read"
    return res_t[:48 * nflows].cpu().numpy().view(lvlip.LRO_RESULT_DTYPE)


@pytest.mark.parametrize("nflows", (1, 3, 17))
@pytest.mark.parametrize("n", (0, 1, 63, 252, 253, 1025))
def test_carry_dev_equals_host(n, nflows, dev):
    flows, rec, prev = random_case(n, nflows)
    want = lvlip.lro_advance_carry(flows, rec, prev)
    assert_same(want, model_carry(flows, rec, prev), "the host form and the model")
    assert_same(carry_dev(flows, rec, prev, dev), want, f"n {n}, {nflows} flows")
    assert_same(carry_dev(flows, rec, prev, dev, in_place=True), want, f"n {n}, {nflows} flows, prev == res")
    if n:
        assert_same(carry_dev(flows, rec, None, dev), lvlip.lro_advance(flows, rec), f"n {n}, {nflows} flows, no prev")


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_carry_dev_edges(name, dev):
    flows, rec, prev, _ = edge_cases()[name]
    want = lvlip.lro_advance_carry(flows, rec, prev)
    assert_same(carry_dev(flows, rec, prev, dev), want, name)
    assert_same(carry_dev(flows, rec, prev, dev, in_place=True), want, name + ", prev == res")


def test_carry_dev_without_prev_is_the_plain_form(dev):
    """prev == NULL: lvlip_lro_advance_dev's bytes on the crafted records (flow
    0xFFFFFFFF, rel 0xFFFFFFFF, dlen 65535, six islands, every status); without
    a record either, zeros and no workspace."""
    from test_lro_advance_gpu import advance_dev, crafted

    for n in (256, 769):
        flows, rec, _ = crafted(n)
        want = lvlip.lro_advance(flows, rec)
        assert_same(carry_dev(flows, rec, None, dev), want, f"{n} crafted records")
        assert_same(advance_dev(flows, rec, dev), want, "the plain device form")
    res_t = guarded(48 * flows.size, dev)
    got = lvlip.lro_advance_carry_dev(_t(flows, dev), None, None, res_t[:48 * flows.size])
    torch.cuda.synchronize(dev)
    assert not got.cpu().numpy().any() and (res_t[48 * flows.size:] == CANARY).all()


def test_results_do_not_depend_on_the_run_or_the_order(dev):
    flows, rec, prev = random_case(1025, 17)
    first = carry_dev(flows, rec, prev, dev)
    assert carry_dev(flows, rec, prev, dev).tobytes() == first.tobytes()
    assert carry_dev(flows, np.ascontiguousarray(rec[::-1]), prev, dev).tobytes() == first.tobytes()
    perm = np.random.default_rng(3).permutation(rec.size)
    assert carry_dev(flows, np.ascontiguousarray(rec[perm]), prev, dev).tobytes() == first.tobytes()


@pytest.mark.parametrize("with_prev", (True, False))
def test_a_workspace_one_byte_short_is_refused(with_prev, dev):
    flows, rec, prev = random_case(253, 3)
    need = lvlip.lro_advance_carry_workspace_bytes(rec.size, flows.size)
    ws_t = guarded(need, dev)
    res_t = torch.full((48 * flows.size,), CANARY, dtype=torch.uint8, device=dev)
    prev_t = _t(prev, dev) if with_prev else None
    with pytest.raises(lvlip.LvlipError) as e:
        lvlip.lro_advance_carry_dev(_t(flows, dev), _t(rec, dev), prev_t, res_t, ws_t[:need - 1])
    torch.cuda.synchronize(dev)
    assert e.value.rc == lvlip.ERANGE
    assert (res_t == CANARY).all() and (ws_t == CANARY).all()
    lvlip.lro_advance_carry_dev(_t(flows, dev), _t(rec, dev), prev_t, res_t, ws_t[:need])
    torch.cuda.synchronize(dev)
    got = res_t.cpu().numpy().view(lvlip.LRO_RESULT_DTYPE)
    assert_same(got, lvlip.lro_advance_carry(flows, rec, prev if with_prev else None), "the size asked for is enough")
    assert (ws_t[need:] == CANARY).all()


@pytest.mark.parametrize("nflows", (1, 3, 17, 300))
def test_next_dev_equals_cpu(nflows, dev):
    """Both steps, once and twice, into canaries; 300 flows end a grid of two
    workgroups on lane 43."""
    flows, res, snd, sres = step_inputs(nflows)
    want = [a.copy() for a in (flows, res, snd, sres)]
    lvlip.lro_next_cpu(want[0], want[1])
    lvlip.snd_next_cpu(want[2], want[3])
    ts = []
    for a in (flows, res, snd, sres):
        t = guarded(a.nbytes, dev)
        t[:a.nbytes].copy_(_t(a, dev))
        ts.append(t)
    torch.cuda.synchronize(dev)
    for rnd in range(2):
        lvlip.lro_next_dev(ts[0][:48 * nflows], ts[1][:48 * nflows])
        lvlip.snd_next_dev(ts[2][:32 * nflows], ts[3][:32 * nflows])
        torch.cuda.synchronize(dev)
        for t, a, what in zip(ts, want, ("f", "res", "s", "snd res")):
            got = t[:a.nbytes].cpu().numpy().view(a.dtype)
            assert_same(got, a, f"{what}, applied {rnd + 1} times")
            assert (t[a.nbytes:] == CANARY).all(), f"written behind {what}"


def test_next_dev_at_the_flow_limit(dev):
    """65 536 flows: the last workgroup is full, every index below nflows."""
    n = lvlip.LRO_MAX_FLOWS
    rng = np.random.default_rng(1)
    flows = np.zeros(n, dtype=lvlip.LRO_FLOW_DTYPE)
    flows["rcv_nxt"], flows["rcv_wnd"] = rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 30, n)
    flows["out_off"] = rng.integers(0, 1 << 62, n)
    res = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
    res["delivered"], res["nsack"] = rng.integers(0, 1 << 31, n), 3
    wf, wr = flows.copy(), res.copy()
    lvlip.lro_next_cpu(wf, wr)
    f_t, r_t = guarded(flows.nbytes, dev), guarded(res.nbytes, dev)
    f_t[:flows.nbytes].copy_(_t(flows, dev))
    r_t[:res.nbytes].copy_(_t(res, dev))
    lvlip.lro_next_dev(f_t[:flows.nbytes], r_t[:res.nbytes])
    torch.cuda.synchronize(dev)
    assert_same(f_t[:flows.nbytes].cpu().numpy().view(flows.dtype), wf, "f")
    assert_same(r_t[:res.nbytes].cpu().numpy().view(res.dtype), wr, "res")
    assert (f_t[flows.nbytes:] == CANARY).all() and (r_t[res.nbytes:] == CANARY).all()


# ------------------------------------------------------------- the whole loop --

def run_dev(loop: StreamLoop, dev) -> dict:
    """StreamLoop.run_cpu's rounds through the device forms on ONE stream: no
    copy to the host, no synchronise and no host decision between the first
    launch and the last.  The network and the application's window update are
    torch operations on the same stream."""
    L, n, nslots = loop.link, loop.nflows, loop.nslots
    fb, fa, snd, ring, fd, tmpl = (_t(a, dev) for a in (loop.fb, L.fa, L.snd, L.ring, L.fd, L.tmpl))
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
    stream_t = torch.full((L.stream.size,), 0xA5, dtype=torch.uint8, device=dev)
    res, sres, kres = z(48 * n), z(32 * n), z(16 * n)
    sacked, sent = z(L.fd.size), torch.zeros(L.fd.size, dtype=torch.int32, device=dev)
    rec, arec, afd = guarded(16 * nslots, dev), z(16 * n), z(16 * n)  # rec: one round's frames, a canary behind it
    fd_out, pick, wire = z(16 * nslots), z(4 * nslots), z(16 * nslots)
    ack, sink = z(L.ack_bytes), z(n + 64)
    ws = torch.empty(lvlip.lro_advance_carry_workspace_bytes(nslots, n), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(max(lvlip.sack_workspace_bytes(n, n), 256), dtype=torch.uint8, device=dev)
    end_lo = torch.from_numpy((loop.end & 0xFFFFFFFF).astype(np.int64)).to(dev)
    fb32 = fb.view(torch.int32).view(n, 12)  # rcv_wnd is word 4, out_off's low word 6 (every offset is below 2^31)
    assert int(loop.end.max()) < 1 << 31
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        for _ in range(ROUNDS):
            lvlip.rtx_sack_dev(fa, None, snd, sres, sacked, nslots, ring, fd, fd_out, pick, stream=s)
            # the network: an entry 4 mod 5 is lost the first time it goes out
            idx = pick.view(torch.int32).to(torch.int64)
            live = idx >= 0  # a dead slot's pick is 0xFFFFFFFF
            idx = idx.clamp(min=0)
            lost = live & (sent[idx] == 0) & (idx % 5 == 4)
            sent.index_put_((idx,), live.to(torch.int32), accumulate=True)
            wire.copy_(fd_out)
            w32 = wire.view(torch.int32).view(nslots, 4)
            w32[:, 2] = torch.where(lost, torch.zeros_like(w32[:, 2]), w32[:, 2])
            # B
            lvlip.lro_dev(ring, wire, fb, lvlip.RX_VERIFY_L4, stream_t, rec[:16 * nslots], stream=s)
            lvlip.lro_advance_carry_dev(fb, rec[:16 * nslots], res, res, ws, stream=s)
            lvlip.ack_dev(tmpl, fb, res, lvlip.ACK_ALL, ack, afd, stream=s)
            lvlip.lro_next_dev(fb, res, stream=s)
            fb32[:, 4] = torch.minimum(torch.full_like(end_lo, loop.wnd), end_lo - fb32[:, 6]).to(torch.int32)
            # A
            lvlip.lro_dev(ack, afd, fa, lvlip.RX_VERIFY_L4, sink, arec, stream=s)
            lvlip.snd_dev(fa, snd, arec, ring, fd, sres, stream=s)
            lvlip.sack_dev(fa, snd, arec, ack, afd, ring, fd, sacked, kres, ws2, stream=s)
            lvlip.snd_next_dev(snd, sres, stream=s)
    s.synchronize()  # the only one
    assert (rec[16 * nslots:] == CANARY).all(), "written behind one round's records"
    h = lambda t, dt=np.uint8: t.cpu().numpy().view(dt)  # noqa: E731
    return dict(stream=h(stream_t), fb=h(fb, lvlip.LRO_FLOW_DTYPE), snd=h(snd, lvlip.SND_FLOW_DTYPE),
                res=h(res, lvlip.LRO_RESULT_DTYPE), sres=h(sres, lvlip.SND_RESULT_DTYPE), ring=h(ring), sacked=h(sacked),
                sent=h(sent, np.int32), most=nslots)


def test_the_loop_with_loss_on_one_stream(dev):
    """8 flows x 40 segments through windows of 8 segments, every fifth first
    transmission lost, lvlip_rtx_sack_dev re-sending: 40 rounds (the queue's
    length: a round's head retransmit arrives, so the prefix grows by a
    segment a round at least) queued on one stream, one synchronise.  Afterwards
    every stream holds its payload, every queue is empty, the record buffer was
    one round's frames, and every byte of the state equals the CPU forms'."""
    loop, want = stream_loop_cpu()
    got = run_dev(loop, dev)
    loop.check_done(got)
    for k in ("stream", "fb", "snd", "res", "sres", "ring", "sacked", "sent"):
        assert got[k].tobytes() == want[k].tobytes(), k
