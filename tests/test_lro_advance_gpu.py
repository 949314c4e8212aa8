"""lvlip_lro_advance_dev on the MI355X (adv_kernels.hip): every result's 48
bytes against lvlip_lro_advance on the same records copied to the host, and
through result_tuples against the independent model of tests/test_lro_cpu.py:
behind lvlip_lro_dev on one stream of the caller's, on crafted record arrays
(numpy writes them: every status, flows out of range, duplicates, touching and
nearly touching intervals, a long interval over short ones, six islands, edges
that wrap, rel 0xFFFFFFFF), on a flow whose one island spans many scan tiles
next to a flow that must not inherit its maximum, and what the call may write:
res and its workspace up to the size it asked for, nothing else.

TILE is adv_kernels.hip's ADV_TILE (sorted elements per scan tile), SPINE its
ADV_SPINE (the lanes of the one wave that scans the tile maxima): above
TILE * SPINE records a lane of the spine scans more than one maximum."""
import functools

import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import ALIGNED_GUARD as GUARD, CANARY, _t, guarded_aligned as guarded
from test_lro_cpu import FLOW_COUNTS, N_LIST, case, fixture_inputs, model_advance, plan_flows, result_tuples

pytestmark = pytest.mark.gpu

TILE = 256
SPINE = 64
NFLOWS = 10
SIZES = (1, 255, 256, 257, 3 * TILE + 1, 40000)
assert SIZES[-1] > TILE * SPINE
STATUSES = (0, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 18, 19, 20, 21)  # every value but PLACED


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


def advance_dev(flows: np.ndarray, rec: np.ndarray, dev, stream=None) -> np.ndarray:
    """lvlip_lro_advance_dev with canaries behind res and behind the workspace
    at the size the library asked for; rec and f compared afterwards."""
    nflows, n = flows.size, rec.size
    fl_t, rec_t = _t(flows, dev), _t(rec, dev)
    need = lvlip.lro_advance_workspace_bytes(n, nflows)
    assert (need > 0) == (n > 0)
    ws_t, res_t = guarded(need, dev), guarded(48 * nflows, dev)
    torch.cuda.synchronize(dev)
    got = lvlip.lro_advance_dev(fl_t, rec_t if n else None, res_t[:48 * nflows], ws_t[:need] if need else None,
                                stream=stream)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    assert got.data_ptr() == res_t.data_ptr()
    assert (ws_t[need:] == CANARY).all(), "written behind the workspace"
    assert (res_t[48 * nflows:] == CANARY).all(), "written behind res"
    assert np.array_equal(rec_t.cpu().numpy(), rec.view(np.uint8).reshape(-1)), "rec is only read"
    assert np.array_equal(fl_t.cpu().numpy(), flows.view(np.uint8).reshape(-1)), "f is only read"
    return res_t[:48 * nflows].cpu().numpy().view(lvlip.LRO_RESULT_DTYPE)


def assert_same_results(got: np.ndarray, flows: np.ndarray, rec: np.ndarray, what: str) -> np.ndarray:
    want = lvlip.lro_advance(flows, rec)
    if got.tobytes() != want.tobytes():
        k = int(np.flatnonzero(got != want)[0])
        pytest.fail(f"{what}: flow {k}: device {got[k]}, host form {want[k]}")
    assert result_tuples(got) == model_advance(flows, rec), what
    return want


# --------------------------------------------------- behind lvlip_lro_dev --

@pytest.mark.parametrize("nflows", FLOW_COUNTS)
@pytest.mark.parametrize("n", N_LIST)
def test_pipeline_on_one_stream(n, nflows, dev):
    buf, fd, flows, out_size = case(n, nflows).laid_out(1, 7)
    stream = torch.cuda.Stream(dev)
    buf_t, fd_t, fl_t = _t(buf, dev), _t(fd, dev), _t(flows, dev)
    out_t = torch.zeros(out_size, dtype=torch.uint8, device=dev)
    ws_t = guarded(lvlip.lro_advance_workspace_bytes(n, nflows), dev)
    res_t = guarded(48 * nflows, dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        rec_t = lvlip.lro_dev(buf_t, fd_t, fl_t, lvlip.RX_VERIFY_L4, out_t, stream=stream)
        lvlip.lro_advance_dev(fl_t, rec_t[:16 * n], res_t[:48 * nflows], ws_t[:-GUARD], stream=stream)
    stream.synchronize()
    rec = rec_t.cpu().numpy().view(lvlip.LRO_REC_DTYPE)[:n]
    got = res_t[:48 * nflows].cpu().numpy().view(lvlip.LRO_RESULT_DTYPE)
    assert_same_results(got, flows, rec, f"n {n}, {nflows} flows")
    assert (res_t[48 * nflows:] == CANARY).all() and (ws_t[-GUARD:] == CANARY).all()
    assert n < 15 or (rec["status"] == lvlip.LRO_PLACED).any()


def test_pipeline_reproduces_the_reference_count(dev):
    fx, buf, fd, flow = fixture_inputs()
    stream = torch.cuda.Stream(dev)
    buf_t, fd_t, fl_t = _t(buf, dev), _t(fd, dev), _t(flow, dev)
    out_t = torch.zeros(lvlip.lro_plan(flow) + 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        rec_t = lvlip.lro_dev(buf_t, fd_t, fl_t, lvlip.RX_VERIFY_L4, out_t, stream=stream)
        res_t = lvlip.lro_advance_dev(fl_t, rec_t, stream=stream)
    stream.synchronize()
    rec = rec_t.cpu().numpy().view(lvlip.LRO_REC_DTYPE)[:len(fd)]
    got = res_t.cpu().numpy().view(lvlip.LRO_RESULT_DTYPE)
    assert_same_results(got, flow, rec, "the reference's segments")
    assert fx["count"] == 2680 and int(got[0]["delivered"]) == 2680 and int(got[0]["nsack"]) == 1


# -------------------------------------------------------- crafted records --

def _rec(flow, rel, dlen, status=lvlip.LRO_PLACED, tcp_flags=0x10, ack=0x01020304):
    return (flow, rel, dlen, status, tcp_flags, ack)


@functools.lru_cache(maxsize=None)
def crafted(n: int):
    """(flows, rec, names): NFLOWS flows and n records.  The first records are
    the named cases on flows A-D (A the flow whose rcv_nxt is 0xFFFFFF00);
    flows E and F never get a record; the rest of the n are random intervals,
    other statuses and flows out of range over the four remaining flows."""
    rng = np.random.default_rng(n)
    flows = plan_flows(NFLOWS, 1 << 30, 0)
    A = int(np.flatnonzero(flows["rcv_nxt"] == 0xFFFFFF00)[0])
    B, C, D, E, F = ((A + j) % NFLOWS for j in range(1, 6))
    fill = [k for k in range(NFLOWS) if k not in (A, B, C, D, E, F)]
    P = lvlip.LRO_PLACED
    rows = []
    # A: six islands, none at 0, arriving out of order; the SACK edges wrap
    rows += [_rec(A, 1000 + 300 * k, 100) for k in (5, 1, 4, 0, 3, 2)]
    # B: a prefix from 0 sent twice, an interval that touches it, one a byte further
    rows += [_rec(B, 0, 100), _rec(B, 201, 99), _rec(B, 100, 100), _rec(B, 0, 100)]
    # C: a long interval over short ones with gaps between them, one that touches its end, one beyond
    rows += [_rec(C, 300, 10), _rec(C, 50, 5000), _rec(C, 100, 10), _rec(C, 5062, 8), _rec(C, 200, 10),
             _rec(C, 5050, 10)]
    # D: the largest rel and dlen there are, an empty interval, a prefix
    rows += [_rec(D, 0xFFFFFFFF, 65535), _rec(D, 5000, 0), _rec(D, 0, 10)]
    # PLACED on flows that are not planned: ignored
    rows += [_rec(NFLOWS, 0, 100), _rec(0xFFFFFFFF, 0, 100), _rec(0x10000, 0, 100), _rec(NFLOWS + 5, 7, 100),
             _rec(0xFFFFFFFF, 0xFFFFFFFF, 65535)]
    # every other status on a planned flow, where it would make an island if it counted
    rows += [_rec(B, 50000 + 1000 * j, 100, status=st) for j, st in enumerate(STATUSES)]
    names = dict(A=A, B=B, C=C, D=D, E=E, F=F, special=len(rows))
    rec = np.zeros(max(n, len(rows)), dtype=lvlip.LRO_REC_DTYPE)
    rec[:len(rows)] = rows
    m = rec.size - len(rows)
    if m:
        tail = rec[len(rows):]
        tail["flow"] = rng.choice(fill + [NFLOWS, NFLOWS + 1, 0xFFFFFFFF], m, p=[0.22] * 4 + [0.04] * 3)
        tail["rel"] = 10 * rng.integers(0, 3 * m, m)
        tail["dlen"] = rng.choice((1, 5, 10, 11, 20, 1460), m)
        tail["status"] = np.where(rng.random(m) < 0.85, P, rng.choice(STATUSES, m))
        tail["tcp_flags"], tail["ack_seq"] = 0x10, rng.integers(0, 1 << 32, m)
    return flows, np.ascontiguousarray(rec[:n]), names


def test_crafted_records_hold_every_case():
    """The named cases mean what their comments say (the host form's results)."""
    flows, rec, nm = crafted(SIZES[2])
    assert rec.size == 256 and nm["special"] < 255
    assert set(rec["status"].tolist()) == set(STATUSES) | {lvlip.LRO_PLACED}
    res = lvlip.lro_advance(flows, rec)
    t = result_tuples(res)
    assert t == model_advance(flows, rec)
    nxt = lambda k: int(flows[k]["rcv_nxt"])  # noqa: E731
    w = lambda k, lo, hi: ((nxt(k) + lo) & 0xFFFFFFFF, (nxt(k) + hi) & 0xFFFFFFFF)  # noqa: E731
    A, B, C, D = (nm[x] for x in "ABCD")
    assert t[A] == (0, 6, [w(A, 1000 + 300 * k, 1100 + 300 * k) for k in range(4)])
    assert all(left < 0x1000 for left, _ in t[A][2]), "the edges wrapped"
    assert t[B] == (200, 4, [w(B, 201, 300)])
    assert t[C] == (0, 6, [w(C, 50, 5060), w(C, 5062, 5070)])
    assert t[D] == (10, 3, [w(D, 5000, 5000), w(D, 0xFFFFFFFF, 0xFFFFFFFF + 65535)])
    assert t[nm["E"]] == t[nm["F"]] == (0, 0, [])


@pytest.mark.parametrize("n", SIZES)
def test_crafted_records(n, dev):
    flows, rec, _ = crafted(n)
    assert rec.size == n
    got = advance_dev(flows, rec, dev)
    assert_same_results(got, flows, rec, f"{n} crafted records")


def test_results_do_not_depend_on_the_run_or_the_order(dev):
    """Twice the same bytes; and the records in another order (equal keys then
    meet the sort in another order) give the same results."""
    flows, rec, _ = crafted(SIZES[4])
    first = advance_dev(flows, rec, dev)
    assert advance_dev(flows, rec, dev).tobytes() == first.tobytes()
    again = advance_dev(flows, np.ascontiguousarray(rec[::-1]), dev)
    assert again.tobytes() == first.tobytes()


# ----------------------------------------------- the carry across the tiles --

@pytest.mark.parametrize("m", [2900, 20000])
def test_carry_across_tiles_stays_inside_its_flow(m, dev):
    """Flow k: [0, 60000) at m = 2900, [0, 20 m + 10) at m = 20000, and m
    intervals of 10 B every 20 B inside it: one island over 12 tiles, or over
    79 of about 40 000 records' 157, where every lane of the spine scans three
    tile maxima, so the running maximum must cross tiles and the spine's lanes.
    A record's dlen has 16 bits, so the long interval is records of 60000 B
    that touch, the last one shorter: between two of them it is the carried
    maximum alone that keeps the 3000 small intervals below each one island.
    Flow k + 1: the same small intervals alone, each its own island: flow k's
    maximum must not reach it."""
    long = max(60000, 20 * m + 10)
    assert m > 2 * TILE and 20 * m + 10 <= long < 1 << 20
    assert (m == 2900) == (2 * m + 1 <= TILE * SPINE)
    cover = [_rec(0, c, min(60000, long - c)) for c in range(0, long, 60000)]
    assert len(cover) == (1 if m == 2900 else 7)
    flows = plan_flows(3, 1 << 20, 0)
    rows = cover + [_rec(0, 20 * j, 10) for j in range(m)] + [_rec(1, 20 * j, 10) for j in range(m)]
    rec = np.array(rows, dtype=lvlip.LRO_REC_DTYPE)[np.random.default_rng(3).permutation(len(rows))]
    rec = np.ascontiguousarray(rec)
    got = advance_dev(flows, rec, dev)
    assert_same_results(got, flows, rec, "carry")
    nxt = int(flows[1]["rcv_nxt"])
    assert result_tuples(got) == [(long, m + len(cover), []),
                                  (10, m, [((nxt + 20 * j) & 0xFFFFFFFF, (nxt + 20 * j + 10) & 0xFFFFFFFF)
                                           for j in range(1, 5)]), (0, 0, [])]
    assert int(got[0]["nsack"]) == 0 and int(got[1]["nsack"]) == 4


# ------------------------------------------------------ what may be written --

def test_nothing_else_is_written(dev):
    """advance_dev's canaries and comparisons, on the batch that uses the most
    of the workspace per record (one tile, one bitmap word more than full)."""
    flows, rec, _ = crafted(SIZES[3])
    need = lvlip.lro_advance_workspace_bytes(rec.size, flows.size)
    assert need % 256 == 0 and need >= 20 * rec.size
    got = advance_dev(flows, rec, dev)
    assert_same_results(got, flows, rec, "canaries")


def test_a_workspace_one_byte_short_is_refused(dev):
    flows, rec, _ = crafted(SIZES[3])
    need = lvlip.lro_advance_workspace_bytes(rec.size, flows.size)
    ws_t = guarded(need, dev)
    res_t = torch.full((48 * flows.size,), CANARY, dtype=torch.uint8, device=dev)
    with pytest.raises(lvlip.LvlipError) as e:
        lvlip.lro_advance_dev(_t(flows, dev), _t(rec, dev), res_t, ws_t[:need - 1])
    torch.cuda.synchronize(dev)
    assert e.value.rc == lvlip.ERANGE
    assert (res_t == CANARY).all() and (ws_t == CANARY).all()
    lvlip.lro_advance_dev(_t(flows, dev), _t(rec, dev), res_t, ws_t[:need])
    torch.cuda.synchronize(dev)
    got = res_t.cpu().numpy().view(lvlip.LRO_RESULT_DTYPE)
    assert_same_results(got, flows, rec, "the size asked for is enough")


def test_no_records_zeroes_the_results(dev):
    flows = plan_flows(3, 4096, 0)
    res_t = guarded(48 * 3, dev)
    got = lvlip.lro_advance_dev(_t(flows, dev), None, res_t[:144])
    torch.cuda.synchronize(dev)
    assert not got.cpu().numpy().any() and got.numel() == 144
    assert (res_t[144:] == CANARY).all()
    empty = np.zeros(0, dtype=lvlip.LRO_REC_DTYPE)
    assert_same_results(got.cpu().numpy().view(lvlip.LRO_RESULT_DTYPE), flows, empty, "no records")
