"""lvlip_ack_dev on the MI355X (ack_kernels.hip): every byte of the whole out
buffer and of fd against lvlip_ack_cpu on the same inputs (and, for the
hand-written case, against the independent model of tests/test_ack_cpu.py), the
reference's own ACK frames through lvlip_lro_dev -> lvlip_lro_advance_dev ->
lvlip_ack_dev on one stream of the caller's, the frames it wrote through
lvlip_rx_verify_dev, and that two runs give the same bytes.

GROUP and FLOWS are ack_kernels.hip's ACK_GROUP (lanes per flow) and ACK_FLOWS
(flows per workgroup): the flow counts leave a lane group's wave partly filled
(1, 3), fill a workgroup twice less one, exactly, and plus one (63, 64, 65) and
end a grid of many workgroups on a partly filled one (4097)."""
import functools

import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import _t
from test_ack_cpu import (CANARY, assert_same_out, golden_compared, golden_inputs, hand, make_flows, make_tmpl,
                          model_run, random_res)

pytestmark = pytest.mark.gpu

GROUP = 8
FLOWS = 256 // GROUP
NFLOWS = (1, 3, 63, 64, 65, 4097)
assert 63 == 2 * FLOWS - 1 and 4097 % FLOWS == 1
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


@functools.lru_cache(maxsize=None)
def random_case(n: int):
    """(tmpl, flows, res, out_size): slots 90 apart from offset 3, so that
    neighbouring frames touch, with one byte more in front of the second half
    of them: 90 is even, so the first half starts at the odd residues mod 16
    and the second at the even ones.  max_sack cycles 0..4 against nsack's
    0..4 with another period."""
    flows = make_flows(n)
    tmpl = make_tmpl(flows, (np.arange(n) // 5 + 4) % 5, stride=90, first=3)
    tmpl["out_off"][n // 2:] += 1
    res = random_res(n, seed=n)
    if n >= 16:
        assert sorted({int(o) % 16 for o in tmpl["out_off"]}) == list(range(16))
    if n >= 63:
        assert {(min(int(r["nsack"]), 4), int(t["max_sack"])) for r, t in zip(res, tmpl)} >= {
            (a, b) for a in range(5) for b in range(5)}
        assert (res["placed"] == 0).any() and (res["placed"] > 0).any()
    return tmpl, flows, res, lvlip.ack_plan(tmpl, flows) + GUARD


def run_dev(tmpl, flows, res, flags, out_size, dev, stream=None):
    """lvlip_ack_dev into canary bytes, with a canary behind fd; t, f and res
    compared afterwards.  Returns (out, fd) on the host."""
    n = flows.size
    t_t, f_t, r_t = _t(tmpl, dev), _t(flows, dev), _t(res, dev)
    out_t = torch.full((out_size,), CANARY, dtype=torch.uint8, device=dev)
    fd_t = torch.full((16 * n + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    assert out_t.data_ptr() % 16 == 0 and fd_t.data_ptr() % 16 == 0
    torch.cuda.synchronize(dev)
    lvlip.ack_dev(t_t, f_t, r_t, flags, out_t, fd_t[:16 * n], stream=stream)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    assert (fd_t[16 * n:] == CANARY).all(), "written behind fd"
    for name, t, a in (("t", t_t, tmpl), ("f", f_t, flows), ("res", r_t, res)):
        assert np.array_equal(t.cpu().numpy(), a.view(np.uint8).reshape(-1)), f"{name} is only read"
    return out_t.cpu().numpy(), fd_t[:16 * n].cpu().numpy().view(lvlip.FRAME_DESC_DTYPE)


def cpu_form(tmpl, flows, res, flags, out_size):
    return lvlip.ack_cpu(tmpl, flows, res, flags, out=np.full(out_size, CANARY, dtype=np.uint8))


@pytest.mark.parametrize("flags", (0, lvlip.ACK_ALL))
@pytest.mark.parametrize("n", NFLOWS)
def test_ack_dev_equals_cpu_form(n, flags, dev):
    tmpl, flows, res, out_size = random_case(n)
    want_out, want_fd = cpu_form(tmpl, flows, res, flags, out_size)
    got_out, got_fd = run_dev(tmpl, flows, res, flags, out_size, dev)
    assert_same_out(got_out, want_out, tmpl, f"{n} flows, flags {flags}")
    assert np.array_equal(got_fd, want_fd), f"{n} flows, flags {flags}: fd"


@pytest.mark.parametrize("flags", (0, lvlip.ACK_ALL))
def test_ack_dev_equals_model(flags, dev):
    """The hand-written case of the CPU tests (every nsack against every
    max_sack, clamped values, the wraps, a left edge 0, an idle flow, slots 91
    apart) against the independent model, and with fd NULL."""
    h = hand()
    want_out, want_fd = model_run(h.tmpl, h.flows, h.res, flags, h.out_size)
    got_out, got_fd = run_dev(h.tmpl, h.flows, h.res, flags, h.out_size, dev)
    assert_same_out(got_out, want_out, h.tmpl, f"flags {flags}")
    assert np.array_equal(got_fd, want_fd)
    out_t = torch.full((h.out_size,), CANARY, dtype=torch.uint8, device=dev)
    lvlip.ack_dev(_t(h.tmpl, dev), _t(h.flows, dev), _t(h.res, dev), flags, out_t, None)
    torch.cuda.synchronize(dev)
    assert_same_out(out_t.cpu().numpy(), want_out, h.tmpl, f"flags {flags}, no fd")


def test_pipeline_reproduces_the_reference_acks(dev):
    """The golden comparisons of the CPU tests with every step on the device:
    lvlip_lro_dev, lvlip_lro_advance_dev and lvlip_ack_dev on one non-default
    stream, and only the ACK frame read back."""
    fx, buf, fd, flow, tmpl = golden_inputs()
    stream = torch.cuda.Stream(dev)
    buf_t, fl_t, t_t = _t(buf, dev), _t(flow, dev), _t(tmpl, dev)
    for j, want in golden_compared(fx):
        fd_t = _t(fd[:j + 1], dev)
        stream_t = torch.zeros(lvlip.lro_plan(flow) + 32, dtype=torch.uint8, device=dev)
        ack_t = torch.full((5 + 90 + 9,), CANARY, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            rec_t = lvlip.lro_dev(buf_t, fd_t, fl_t, lvlip.RX_VERIFY_L4, stream_t, stream=stream)
            res_t = lvlip.lro_advance_dev(fl_t, rec_t[:16 * (j + 1)], stream=stream)
            lvlip.ack_dev(t_t, fl_t, res_t, 0, ack_t, None, stream=stream)
        stream.synchronize()
        got = ack_t.cpu().numpy()
        assert got[5:5 + len(want)].tobytes().hex() == want.hex(), f"arrival {j}"
        assert (got[:5] == CANARY).all() and (got[5 + len(want):] == CANARY).all(), f"arrival {j}"


def test_the_acks_verify_on_the_device(dev):
    """Closing the loop: lvlip_rx_verify_dev with LVLIP_RX_VERIFY_L4 over the
    frames and the fd lvlip_ack_dev wrote gives LVLIP_RX_OK for every flow that
    got an ACK and LVLIP_RX_SHORT for the len == 0 entries.  The verifier sums
    the RFC's pseudo header, the frames carry the reference's (the carry out of
    the u32 is lost): the test addresses are 10.0.0.x, whose seed does not wrap,
    so the two agree."""
    tmpl, flows, res, out_size = random_case(65)
    n = flows.size
    assert all(h[26] == 10 and h[30] == 10 and h[27] == h[28] == 0 for h in tmpl["hdr"])
    out_t = torch.full((out_size + 15 & ~15,), CANARY, dtype=torch.uint8, device=dev)
    fd_t = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    lvlip.ack_dev(_t(tmpl, dev), _t(flows, dev), _t(res, dev), 0, out_t, fd_t)
    verdict = lvlip.rx_verify_dev(out_t, fd_t, lvlip.RX_VERIFY_L4)
    torch.cuda.synchronize(dev)
    verdict = verdict.cpu().numpy()[:n]
    acked = res["placed"] > 0
    assert acked.any() and not acked.all()
    assert (verdict[acked] == lvlip.RX_OK).all(), verdict[acked]
    assert (verdict[~acked] == lvlip.RX_SHORT).all(), verdict[~acked]
    lens = fd_t.cpu().numpy().view(lvlip.FRAME_DESC_DTYPE)["len"]
    assert (lens[~acked] == 0).all() and (lens[acked] >= 54).all()


def test_two_runs_give_the_same_bytes(dev):
    tmpl, flows, res, out_size = random_case(4097)
    a = run_dev(tmpl, flows, res, lvlip.ACK_ALL, out_size, dev)
    b = run_dev(tmpl, flows, res, lvlip.ACK_ALL, out_size, dev, stream=torch.cuda.Stream(dev))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
