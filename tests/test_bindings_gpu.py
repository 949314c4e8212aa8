"""The nine device wrappers of lvlip.py's f1/f2 part at the smallest shapes at
which their pointer-or-NULL and allocate-or-check code can go wrong: one flow
with nothing to do, one flow with one record, frame or slot, every optional
tensor once given and once None.  Every result is compared byte for byte with
the call's CPU twin.  An output the caller gives is one record larger than
needed and lies in front of canary bytes: the wrapper returns exactly the
records asked for, in the caller's memory, and writes nothing behind them.

Every call here is a valid one."""
import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import CANARY, _t, guarded, guarded_aligned, unguard
from test_ack_cpu import make_flows, make_tmpl, random_res
from test_lro_cpu import case as lro_case
from test_sack_cpu import make_acks
from test_snd_cpu import Case as SndCase
from test_snd_cpu import rtx_inputs
from test_tso_cpu import template as tso_template

pytestmark = pytest.mark.gpu

FD, REC = lvlip.FRAME_DESC_DTYPE, lvlip.LRO_REC_DTYPE
BOTH = (True, False)


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


def opt(a, dev):
    return _t(a, dev) if a is not None else None


def canary(nbytes: int):
    return np.full(nbytes, CANARY, dtype=np.uint8)


def result(call, given: bool, per: int, n: int, dtype, dev, least: int = 1) -> np.ndarray:
    """call(result tensor or None) -> the wrapper's result of n records of per
    bytes, as an array.  A given tensor holds n + 1 records; a new one is
    returned cut to n (or, for a wrapper that returns it whole, holds `least`)."""
    g = guarded(per * (n + 1), dev)
    got = call(g[:per * (n + 1)] if given else None)
    torch.cuda.synchronize(dev)
    assert got.dtype == torch.uint8 and got.is_contiguous()
    if given:
        assert got.numel() == 0 or got.data_ptr() == g.data_ptr(), "the caller's tensor is the result"
        assert got.numel() == per * (n if least == 0 else n + 1)
        return unguard(g, per * n, dtype)
    assert got.numel() == per * max(n, least)
    return got.cpu().numpy()[:per * n].view(dtype)


# ---------------------------------------------------------------------- tso --

@pytest.mark.parametrize("with_fd", BOTH)
@pytest.mark.parametrize("nsend", (0, 1))
def test_tso_dev(nsend, with_fd, dev):
    sends = lvlip.tso_send(tso_template(), 3, 40, 64, out_off=5)[:nsend].copy()
    payload = np.arange(64, dtype=np.uint8)
    nseg, out_bytes = lvlip.tso_plan(sends)
    assert nseg == nsend
    want, want_fd = lvlip.tso_cpu(payload, sends, out=canary(out_bytes + 16))
    out_t = _t(canary(out_bytes + 16), dev)
    g = guarded(16 * (nseg + 1), dev)
    assert lvlip.tso_dev(_t(payload, dev), _t(sends, dev), nseg, out_t, g[:16 * (nseg + 1)] if with_fd else None) is None
    torch.cuda.synchronize(dev)
    assert np.array_equal(out_t.cpu().numpy(), want)
    assert unguard(g, 16 * nseg if with_fd else 0, FD).tobytes() == (want_fd.tobytes() if with_fd else b"")


# ------------------------------------------------------- lro and its advance --

@pytest.mark.parametrize("given", BOTH)
@pytest.mark.parametrize("with_flows", BOTH)
@pytest.mark.parametrize("n", (0, 1))
def test_lro_dev(n, with_flows, given, dev):
    buf, fd, flows, out_size = lro_case(1, 1).laid_out(1, 7)
    fd = fd[:n].copy()
    want, want_rec = lvlip.lro_cpu(buf, fd, flows[:with_flows], lvlip.RX_VERIFY_L4,
                                   out=canary(out_size) if with_flows else None)
    out_t = _t(canary(out_size), dev)
    rec = result(lambda r: lvlip.lro_dev(_t(buf, dev), _t(fd, dev), _t(flows, dev) if with_flows else None,
                                         lvlip.RX_VERIFY_L4, out_t, r), given, 16, n, REC, dev)
    assert rec.tobytes() == want_rec.tobytes()
    assert np.array_equal(out_t.cpu().numpy(), want if with_flows else canary(out_size))


@pytest.mark.parametrize("given", BOTH)
@pytest.mark.parametrize("n", (0, 1))
def test_lro_advance_dev(n, given, dev):
    buf, fd, flows, out_size = lro_case(1, 1).laid_out(1, 7)
    _, rec = lvlip.lro_cpu(buf, fd[:n].copy(), flows, lvlip.RX_VERIFY_L4)
    want = lvlip.lro_advance(flows, rec)
    need = lvlip.lro_advance_workspace_bytes(n, 1)
    ws = guarded_aligned(need, dev)
    rec_t = _t(rec, dev) if n or given else None  # no records: an empty tensor, or None
    res = result(lambda r: lvlip.lro_advance_dev(_t(flows, dev), rec_t, r, ws[:need] if given and need else None),
                 given, 48, 1, lvlip.LRO_RESULT_DTYPE, dev, least=0)
    assert res.tobytes() == want.tobytes()
    assert (ws[need:] == CANARY).all(), "written behind the workspace"


# ---------------------------------------------------------------------- ack --

@pytest.mark.parametrize("with_fd", BOTH)
@pytest.mark.parametrize("placed", (0, 1))
def test_ack_dev(placed, with_fd, dev):
    """placed 0: the flow gets no frame, out stays as it was."""
    flows = make_flows(1)
    tmpl, res = make_tmpl(flows, 4, first=3), random_res(1, seed=1)
    res["placed"] = placed
    out_size = lvlip.ack_plan(tmpl, flows) + 16
    want, want_fd = lvlip.ack_cpu(tmpl, flows, res, 0, out=canary(out_size))
    assert (int(want_fd[0]["len"]) > 0) == bool(placed)
    out_t = _t(canary(out_size), dev)
    g = guarded(32, dev)
    assert lvlip.ack_dev(_t(tmpl, dev), _t(flows, dev), _t(res, dev), 0, out_t, g[:32] if with_fd else None) is None
    torch.cuda.synchronize(dev)
    assert np.array_equal(out_t.cpu().numpy(), want)
    assert unguard(g, 16 if with_fd else 0, FD).tobytes() == (want_fd.tobytes() if with_fd else b"")


# -------------------------------------------------------------- snd and rtx --

def one_queue(rtx: int) -> SndCase:
    """One flow with a queue of three frames of 8, 8 and 1 payload bytes."""
    c = SndCase(nseg=[3], mss=[8], rtx=[rtx], seed=5)
    assert c.nslots == rtx and c.fd.size == 3
    return c


def ack_of(c: SndCase, acked: int, n: int) -> np.ndarray:
    rec = np.zeros(n, dtype=REC)
    rec[:] = (0, 0, 0, lvlip.LRO_NO_DATA, 0x10, (int(c.snd[0]["snd_una"]) + acked) & 0xFFFFFFFF)
    return rec


@pytest.mark.parametrize("given", BOTH)
@pytest.mark.parametrize("n", (0, 1))
def test_snd_dev(n, given, dev):
    c = one_queue(2)
    rec = ack_of(c, 8, n)
    want = lvlip.snd_cpu(c.flows, c.snd, rec, c.ring, c.fd)
    assert int(want[0]["popped"]) == n
    rec_t = _t(rec, dev) if n or given else None
    res = result(lambda r: lvlip.snd_dev(_t(c.flows, dev), _t(c.snd, dev), rec_t, _t(c.ring, dev), _t(c.fd, dev), r),
                 given, 32, 1, lvlip.SND_RESULT_DTYPE, dev, least=0)
    # without a record the C call is a no-op: a new tensor is zeroed, the caller's keeps its bytes
    assert res.tobytes() == (canary(32).tobytes() if given and n == 0 else want.tobytes())


@pytest.mark.parametrize("given", BOTH)
@pytest.mark.parametrize("with_results", BOTH)
@pytest.mark.parametrize("rtx", (0, 1))
def test_rtx_dev(rtx, with_results, given, dev):
    c = one_queue(rtx)
    lro, sres = rtx_inputs(c, 1) if with_results else (None, None)
    want = c.ring.copy()
    want_fd = lvlip.rtx_cpu(c.flows, lro, c.snd, sres, want, c.fd)
    ring_t = _t(c.ring, dev)
    fd_out = result(lambda o: lvlip.rtx_dev(_t(c.flows, dev), opt(lro, dev), _t(c.snd, dev), opt(sres, dev), rtx,
                                            ring_t, _t(c.fd, dev), o), given, 16, rtx, FD, dev, least=0)
    assert fd_out.tobytes() == want_fd.tobytes()
    assert np.array_equal(ring_t.cpu().numpy(), want)


# ------------------------------------------------------- sack and rtx_sack --

@pytest.mark.parametrize("given", BOTH)
@pytest.mark.parametrize("n", (0, 1))
def test_sack_dev(n, given, dev):
    c = one_queue(2)
    rec, aring, afd = make_acks(c, 1, seed=3, blocks_only=True)
    rec, afd = rec[:n].copy(), afd[:n].copy()
    board = np.zeros(3, dtype=np.uint8)
    want = lvlip.sack_cpu(c.flows, c.snd, rec, aring, afd, c.ring, c.fd, board)
    acks = [_t(a, dev) if n or given else None for a in (rec, aring, afd)]  # no records: unused tensors, or None
    need = max(lvlip.sack_workspace_bytes(n, 1), 256)
    ws, board_g = guarded_aligned(need, dev), guarded(3, dev)
    board_g[:3] = 0
    res = result(lambda r: lvlip.sack_dev(_t(c.flows, dev), _t(c.snd, dev), acks[0], acks[1], acks[2], _t(c.ring, dev),
                                          _t(c.fd, dev), board_g[:3], r, ws[:need] if given else None),
                 given, 16, 1, lvlip.SACK_RESULT_DTYPE, dev, least=0)
    # without a record the C call is a no-op: a new tensor is zeroed, the caller's keeps its bytes
    assert res.tobytes() == (canary(16).tobytes() if given and n == 0 else want.tobytes())
    assert np.array_equal(unguard(board_g, 3, np.uint8), board)
    assert (ws[need:] == CANARY).all(), "written behind the workspace"


@pytest.mark.parametrize("given", BOTH)
@pytest.mark.parametrize("with_board", BOTH)
@pytest.mark.parametrize("rtx", (0, 2))
def test_rtx_sack_dev(rtx, with_board, given, dev):
    """The queue's first entry is marked: with the scoreboard the slots pick
    entries 1 and 2, without it 0 and 1."""
    c = one_queue(rtx)
    board = np.array([1, 0, 0], dtype=np.uint8) if with_board else None
    want = c.ring.copy()
    want_fd, want_pick = lvlip.rtx_sack_cpu(c.flows, None, c.snd, None, board, want, c.fd)
    assert want_pick.tolist() == ([1, 2] if with_board else [0, 1])[:rtx]
    ring_t, picks = _t(c.ring, dev), []

    def call(o):
        got = lvlip.rtx_sack_dev(_t(c.flows, dev), None, _t(c.snd, dev), None, opt(board, dev), rtx, ring_t,
                                 _t(c.fd, dev), o, picks[0] if given else None)
        picks.append(got[1])
        return got[0]

    pick_g = guarded(4 * (rtx + 1), dev)
    picks.append(pick_g[:4 * (rtx + 1)])
    fd_out = result(call, given, 16, rtx, FD, dev, least=0)
    assert fd_out.tobytes() == want_fd.tobytes()
    assert picks[1].numel() == 4 * rtx and (not given or rtx == 0 or picks[1].data_ptr() == pick_g.data_ptr())
    assert picks[1].cpu().numpy().view(np.uint32).tolist() == want_pick.tolist()
    assert unguard(pick_g, 4 * rtx if given else 0, np.uint32).tolist() == (want_pick.tolist() if given else [])
    assert np.array_equal(ring_t.cpu().numpy(), want)
