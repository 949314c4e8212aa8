"""State across batches (include/lvlip_skb.h: lvlip_lro_advance_carry,
lvlip_lro_next_cpu, lvlip_snd_next_cpu) without a GPU: the advance step with
carried islands and both steps against an independent model, prev == NULL
against lvlip_lro_advance, batches cut apart against the one batch, the
forgotten fifth island, the edges the header names, what the steps leave of the
frames lvlip_ack_cpu and lvlip_rtx_cpu build, the refusals, the whole loop with
loss on the CPU forms, a sanitizer build of examples/stream_loop.c and the new
kernels' scratch size.  tests/test_carry_gpu.py shares the model and the cases.

The model (model_carry, model_lro_next, model_snd_next) restates the header's
text with Python integers: it uses neither tcp_hdr.h nor interval_union.h."""
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import lvlip
from test_lro_cpu import fixture_inputs, flow_kw, plan_flows, tcp_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
CANARY = 0xA5
P = lvlip.LRO_PLACED
STATUSES = (0, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 18, 19, 20, 21)  # every value but PLACED


# --------------------------------------------------------------- the model --

def carried(flow, prev) -> list:
    """The blocks of prev that count for the flow as it is now: [(l, r)]."""
    nxt, wnd = int(flow["rcv_nxt"]), int(flow["rcv_wnd"])
    out = []
    for j in range(min(int(prev["nsack"]), 4)):
        l, r = ((int(v) - nxt) & M32 for v in prev["sack"][j])
        if l < r <= wnd:
            out.append((l, r))
    return out


def islands(iv) -> list:
    """The union of intervals that touch or overlap, ascending: [[lo, hi]]."""
    merged = []
    for lo, hi in sorted(iv):
        if merged and lo <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], hi)
        else:
            merged.append([lo, hi])
    return merged


def model_carry(flows, rec, prev=None) -> np.ndarray:
    res = np.zeros(flows.size, dtype=lvlip.LRO_RESULT_DTYPE)
    by_flow = [[] for _ in range(flows.size)]
    for r in rec:
        if int(r["status"]) == P and int(r["flow"]) < flows.size:
            by_flow[int(r["flow"])].append((int(r["rel"]), int(r["rel"]) + int(r["dlen"])))
    for k, f in enumerate(flows):
        isl = islands(by_flow[k] + (carried(f, prev[k]) if prev is not None else []))
        res[k]["placed"] = len(by_flow[k])
        if isl and isl[0][0] == 0:
            res[k]["delivered"] = isl[0][1] & M32
            isl = isl[1:]
        res[k]["nsack"] = min(len(isl), 4)
        for j, (lo, hi) in enumerate(isl[:4]):
            res[k]["sack"][j] = ((int(f["rcv_nxt"]) + lo) & M32, (int(f["rcv_nxt"]) + hi) & M32)
    return res


def model_lro_next(flows, res):
    f, r = flows.copy(), res.copy()
    for k in range(f.size):
        d = min(int(r[k]["delivered"]), int(f[k]["rcv_wnd"]))
        f[k]["rcv_nxt"] = (int(f[k]["rcv_nxt"]) + d) & M32
        f[k]["out_off"] = int(f[k]["out_off"]) + d
        f[k]["rcv_wnd"] = int(f[k]["rcv_wnd"]) - d
        r[k]["delivered"] = 0
    return f, r


def model_snd_next(snd, res):
    s, r = snd.copy(), res.copy()
    for k in range(s.size):
        p = min(int(r[k]["popped"]), int(s[k]["nseg"]))
        s[k]["snd_una"] = r[k]["snd_una"]
        s[k]["seg0"] = (int(s[k]["seg0"]) + p) & M32
        s[k]["nseg"] = int(s[k]["nseg"]) - p
        r[k]["popped"], r[k]["acked"], r[k]["inflight"] = 0, 0, s[k]["nseg"]
    return s, r


def assert_same(got: np.ndarray, want: np.ndarray, what: str) -> None:
    if got.tobytes() != want.tobytes():
        k = int(np.flatnonzero(got != want)[0])
        pytest.fail(f"{what}: flow {k}: got {got[k]}, want {want[k]}")


# --------------------------------------------------------------- the cases --

def _rec(flow, rel, dlen, status=P, tcp_flags=0x10, ack=0x01020304):
    return (flow, rel, dlen, status, tcp_flags, ack)


def _prev(flows, k_blocks: dict, nsack=None) -> np.ndarray:
    """A prev array: per flow index the relative blocks [(l, r)] (stored
    absolute, against the flow's rcv_nxt); delivered and placed hold junk,
    which the calls must ignore."""
    prev = np.zeros(flows.size, dtype=lvlip.LRO_RESULT_DTYPE)
    prev["delivered"], prev["placed"], prev["reserved"] = 0xDEADBEEF, 0x12345678, 0x77
    for k, blocks in k_blocks.items():
        for j, (l, r) in enumerate(blocks):
            prev[k]["sack"][j] = ((int(flows[k]["rcv_nxt"]) + l) & M32, (int(flows[k]["rcv_nxt"]) + r) & M32)
        prev[k]["nsack"] = len(blocks)
    for k, v in (nsack or {}).items():
        prev[k]["nsack"] = v
    return prev


@functools.lru_cache(maxsize=None)
def random_case(n: int, nflows: int, seed: int = 0):
    """(flows, rec, prev): n records as the crafted generator's tail makes them
    (random intervals on multiples of 10, other statuses, flows out of range,
    flow 0xFFFFFFFF, dlen 65535 among them) and a prev whose blocks are valid,
    stale, empty, straddling or beyond the window, with nsack up to 7."""
    rng = np.random.default_rng(10007 * n + 31 * nflows + seed)
    wnd = 1 << 20
    flows = plan_flows(nflows, wnd, 0)
    rec = np.zeros(n, dtype=lvlip.LRO_REC_DTYPE)
    if n:
        rec["flow"] = rng.choice(list(range(nflows)) + [nflows, nflows + 1, M32], n,
                                 p=[0.88 / nflows] * nflows + [0.04] * 3)
        rec["rel"] = 10 * rng.integers(0, 3 * n + 30, n)
        rec["dlen"] = rng.choice((1, 5, 10, 11, 20, 1460, 65535), n, p=[0.16] * 6 + [0.04])
        rec["status"] = np.where(rng.random(n) < 0.85, P, rng.choice(STATUSES, n))
        rec["tcp_flags"], rec["ack_seq"] = 0x10, rng.integers(0, 1 << 32, n)
        rec[0] = _rec(M32, M32, 65535)
    prev = np.zeros(nflows, dtype=lvlip.LRO_RESULT_DTYPE)
    prev["delivered"], prev["placed"] = rng.integers(0, 1 << 32, nflows), rng.integers(0, 1 << 32, nflows)
    for k in range(nflows):
        nxt = int(flows[k]["rcv_nxt"])
        prev[k]["nsack"] = int(rng.integers(0, 8))
        for j in range(4):
            kind = int(rng.integers(0, 8))
            l = 10 * int(rng.integers(0, 3 * n + 30))
            r = l + int(rng.choice((5, 10, 30, 70000)))
            if kind == 4:
                l, r = (-500) & M32, (-100) & M32  # stale
            elif kind == 5:
                r = l                              # empty
            elif kind == 6:
                l, r = (-20) & M32, 30             # straddles rcv_nxt
            elif kind == 7:
                l, r = wnd - 5, wnd + 5            # ends beyond the window
            prev[k]["sack"][j] = ((nxt + l) & M32, (nxt + r) & M32)
    prev[0]["nsack"] = 7  # more than sack[] holds: four are read
    prev[0]["sack"][3] = ((int(flows[0]["rcv_nxt"]) + 15) & M32, (int(flows[0]["rcv_nxt"]) + 70015) & M32)
    return flows, rec, prev


def edge_cases():
    """name -> (flows, rec, prev, want): want the per-flow (delivered, placed,
    [(l, r) relative islands]) where the comment says what must happen, or
    None (the model alone decides)."""
    E = {}
    recs = lambda rows: np.array(rows, dtype=lvlip.LRO_REC_DTYPE) if rows else np.zeros(0, lvlip.LRO_REC_DTYPE)  # noqa: E731
    # a carried block longer than a record can be, and one that ends at rcv_wnd = 2^30
    f = plan_flows(2, 1 << 30, 0)
    E["long_blocks"] = (f, recs([_rec(0, 0, 1000), _rec(1, 5, 7)]),
                        _prev(f, {0: [(1000, 71000)], 1: [(100, 70100), ((1 << 30) - 70000, 1 << 30)]}),
                        [(71000, 1, []), (0, 1, [(5, 12), (100, 70100), ((1 << 30) - 70000, 1 << 30)])])
    # one byte beyond 2^30 does not count
    E["beyond_2_30"] = (f, recs([]), _prev(f, {0: [((1 << 30) - 70000, (1 << 30) + 1)]}), [(0, 0, []), (0, 0, [])])
    # a record closes the hole in front of a carried block; records touch a block at both ends
    f = plan_flows(3, 1 << 16, 0)
    E["touching"] = (f, recs([_rec(0, 0, 500), _rec(1, 400, 100), _rec(1, 700, 50), _rec(2, 499, 1), _rec(2, 702, 9)]),
                     _prev(f, {0: [(500, 900)], 1: [(500, 700)], 2: [(501, 701)]}),
                     [(900, 1, []), (0, 2, [(400, 750)]), (0, 2, [(499, 500), (501, 701), (702, 711)])])
    # stale, empty, straddling and beyond-window blocks next to one that counts; nsack 7
    E["ignored_blocks"] = (f, recs([_rec(0, 0, 10)]),
                           _prev(f, {0: [((-300) & M32, (-100) & M32), (50, 50), ((-5) & M32, 40), (60, 70)],
                                     1: [((1 << 16) - 10, (1 << 16) + 1), (20, 30), (80, 70), (1 << 31, (1 << 31) + 5)],
                                     2: [(10, 20), (30, 40), (50, 60), (70, 80)]}, nsack={2: 7}),
                           [(10, 1, [(60, 70)]), (0, 0, [(20, 30)]), (0, 0, [(10, 20), (30, 40), (50, 60), (70, 80)])])
    # nsack says 2: blocks 2 and 3 are not read
    E["nsack_limits"] = (f, recs([]), _prev(f, {1: [(10, 20), (30, 40), (50, 60), (70, 80)]}, nsack={1: 2}),
                         [(0, 0, []), (0, 0, [(10, 20), (30, 40)]), (0, 0, [])])
    # a carry and no record at all; a block at rel 0 is the prefix
    E["no_records"] = (f, recs([]), _prev(f, {0: [(100, 200), (200, 300), (250, 400)], 2: [(0, 64)]}),
                       [(0, 0, [(100, 400)]), (0, 0, []), (64, 0, [])])
    # rcv_nxt 12 bytes below 2^32: the carried edges and the new ones wrap
    f = plan_flows(2, 4096, 0, rcv_nxt0=0xFFFFFFF4)
    k = int(np.flatnonzero(f["rcv_nxt"] == 0xFFFFFFF4)[0])
    E["wrap"] = (f, recs([_rec(k, 0, 8), _rec(k, 40, 8)]), _prev(f, {k: [(8, 20), (30, 40)], 1 - k: [(5, 6)]}),
                 [(20, 2, [(30, 48)]) if j == k else (0, 0, [(5, 6)]) for j in range(2)])
    # more than four islands in one call: the first four, as before
    f = plan_flows(1, 1 << 16, 0)
    E["six_islands"] = (f, recs([_rec(0, 100 * j, 10) for j in (9, 3, 7)]),
                        _prev(f, {0: [(100, 110), (500, 510), (1100, 1110), (200, 210)]}),
                        [(0, 3, [(100, 110), (200, 210), (300, 310), (500, 510)])])
    return E


def want_result(flows, want) -> np.ndarray:
    res = np.zeros(flows.size, dtype=lvlip.LRO_RESULT_DTYPE)
    for k, (d, p, isl) in enumerate(want):
        res[k]["delivered"], res[k]["placed"], res[k]["nsack"] = d, p, len(isl)
        for j, (l, r) in enumerate(isl):
            res[k]["sack"][j] = ((int(flows[k]["rcv_nxt"]) + l) & M32, (int(flows[k]["rcv_nxt"]) + r) & M32)
    return res


# ------------------------------------------------------------ the bindings --

NEW = ("lvlip_lro_advance_carry", "lvlip_lro_advance_carry_workspace_bytes", "lvlip_lro_advance_carry_dev",
       "lvlip_lro_next_cpu", "lvlip_lro_next_dev", "lvlip_snd_next_cpu", "lvlip_snd_next_dev")


def test_symbols_are_exported_and_bound():
    L = lvlip.lib()
    for name in NEW:
        assert name in lvlip.SIGNATURES
        assert getattr(L, name).argtypes == lvlip.SIGNATURES[name][1]
        assert getattr(L, name).restype == lvlip.SIGNATURES[name][0]
        assert callable(getattr(lvlip, name[len("lvlip_"):]))
    hdr = open(os.path.join(ROOT, "include", "lvlip_skb.h")).read()
    for name in NEW:  # the argument counts are the header's
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
        assert len(decl.split(",")) == len(lvlip.SIGNATURES[name][1]), name


# ---------------------------------------------------- the advance with carry --

@pytest.mark.parametrize("n", (1, 255, 256, 257, 769))
def test_without_prev_it_is_lro_advance(n):
    """prev == NULL: all 48 bytes of every result, on the crafted records of
    tests/test_lro_advance_gpu.py (six islands, flows out of range, flow
    0xFFFFFFFF, rel 0xFFFFFFFF, dlen 65535, every status)."""
    from test_lro_advance_gpu import crafted

    flows, rec, _ = crafted(n)
    assert n < 255 or ((rec["flow"] == M32).any() and (rec["dlen"] == 65535).any())  # n == 1 is the first row alone
    want = lvlip.lro_advance(flows, rec)
    assert_same(lvlip.lro_advance_carry(flows, rec), want, "prev NULL")
    assert_same(model_carry(flows, rec), want, "the model without prev")
    # and an all-zero prev carries nothing
    assert_same(lvlip.lro_advance_carry(flows, rec, np.zeros(flows.size, dtype=lvlip.LRO_RESULT_DTYPE)), want, "empty prev")


@pytest.mark.parametrize("nflows", (1, 3, 17))
@pytest.mark.parametrize("n", (0, 1, 63, 252, 253, 1025))
def test_carry_equals_model(n, nflows):
    flows, rec, prev = random_case(n, nflows)
    before = prev.copy()
    got = lvlip.lro_advance_carry(flows, rec, prev)
    assert_same(got, model_carry(flows, rec, prev), f"n {n}, {nflows} flows")
    assert prev.tobytes() == before.tobytes(), "prev is only read"
    assert carried(flows[0], prev[0]) and (prev["nsack"] > 4).any()
    # in place: prev == res
    inplace = prev.copy()
    assert lvlip.lro_advance_carry(flows, rec, inplace, inplace) is inplace
    assert_same(inplace, got, "prev == res")
    # the records' order does not matter
    assert_same(lvlip.lro_advance_carry(flows, np.ascontiguousarray(rec[::-1]), prev), got, "reversed records")


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_edges(name):
    flows, rec, prev, want = edge_cases()[name]
    got = lvlip.lro_advance_carry(flows, rec, prev)
    assert_same(got, model_carry(flows, rec, prev), name)
    assert_same(got, want_result(flows, want), name + ": what the case is about")
    inplace = prev.copy()
    lvlip.lro_advance_carry(flows, rec, inplace, inplace)
    assert_same(inplace, got, name + ": prev == res")


def test_no_records_with_a_carry_is_not_a_zero_fill():
    flows, rec, prev, _ = edge_cases()["no_records"]
    assert rec.size == 0
    got = lvlip.lro_advance_carry(flows, rec, prev)
    assert got["nsack"].tolist() == [1, 0, 0] and got["delivered"].tolist() == [0, 0, 64] and not got["placed"].any()
    assert not lvlip.lro_advance_carry(flows, rec).view(np.uint8).any()


# ----------------------------------------------------------- split and whole --

def run_batches(buf, fd, flows, cuts, out_size, forget_check=None):
    """lro_cpu -> lro_advance_carry -> lro_next_cpu over fd cut at `cuts`.
    Returns (out, delivered per flow, flows at the end, results at the end)."""
    flows = flows.copy()
    out = np.full(out_size, CANARY, dtype=np.uint8)
    res = np.zeros(flows.size, dtype=lvlip.LRO_RESULT_DTYPE)
    total = np.zeros(flows.size, dtype=np.uint64)
    edges = [0, *cuts, fd.size]
    for a, b in zip(edges[:-1], edges[1:]):
        _, rec = lvlip.lro_cpu(buf, fd[a:b], flows, lvlip.RX_VERIFY_L4, out=out)
        lvlip.lro_advance_carry(flows, rec, res, res)
        total += res["delivered"]
        lvlip.lro_next_cpu(flows, res)
    return out, total, flows, res


def islands_at(frames_so_far, flows, flags=lvlip.RX_VERIFY_L4) -> list:
    """Per flow the islands beyond the prefix after these frames, from the
    test's own parse of them (tests/test_lro_cpu.py's model_rec), against the
    flows as they were planned."""
    from test_lro_cpu import model_rec

    iv = [[] for _ in range(flows.size)]
    for fr in frames_so_far:
        k, rel, dlen, st, *_ = model_rec(bytes(fr), flows, flags)
        if st == P:
            iv[k].append((rel, rel + dlen))
    return [[m for m in islands(v) if m[0] != 0] for v in iv]


def cut_qualifies(frames, flows, cuts) -> bool:
    return all(len(isl) <= 4 for c in cuts for isl in islands_at(frames[:c], flows))


def check_split(frames, buf, fd, flows, out_size, cuts, whole):
    out, total, f_end, res = run_batches(buf, fd, flows, cuts, out_size)
    w_out, w_total, w_end, w_res = whole
    assert np.array_equal(out, w_out), f"cuts {cuts}: the out bytes"
    assert total.tolist() == w_total.tolist(), f"cuts {cuts}: the sum of delivered"
    assert f_end["rcv_nxt"].tolist() == w_end["rcv_nxt"].tolist(), f"cuts {cuts}: rcv_nxt"
    assert res["nsack"].tolist() == w_res["nsack"].tolist() and res["sack"].tolist() == w_res["sack"].tolist(), \
        f"cuts {cuts}: sack[]"


def test_the_reference_segments_in_every_split():
    """tests/golden/lro_ref.json: 7 segments arriving as 0, 2, 1, 1, 4, 3, 6
    never leave more than two islands, so every one- and two-cut split
    qualifies and must give what the reference's own stack returned."""
    fx, buf, fd, flow = fixture_inputs()
    frames = [bytes.fromhex(h) for h in fx["frames"]]
    out_size = lvlip.lro_plan(flow.copy()) + 32
    whole = run_batches(buf, fd, flow, (), out_size)
    assert int(whole[1][0]) == fx["count"] == 2680
    assert whole[0][3:3 + 2680].tobytes().hex() == fx["dequeued_hex"]
    assert int(whole[3][0]["nsack"]) == 1 and int(whole[3][0]["sack"][0][0]) == (fx["rcv_nxt"] + 6 * 536) & M32
    splits = [c for r in (1, 2) for c in itertools.combinations(range(1, 7), r)]
    assert len(splits) == 6 + 15
    for cuts in splits:
        assert cut_qualifies(frames, flow, cuts)
        assert max(len(i) for c in range(8) for i in islands_at(frames[:c], flow)) <= 2
        check_split(frames, buf, fd, flow, out_size, cuts, whole)


@functools.lru_cache(maxsize=None)
def split_case(n: int, nflows: int):
    """Segments that share boundaries (every stream cut once into pieces of 1
    .. 1460 bytes), a seventh of them lost and sent again some places later, a
    few lost for good, a fifth sent twice, displaced by up to three places so that holes
    open and close, with a pure ACK and an out-of-window frame per flow
    between them.  Pieces share boundaries because
    a frame that starts below a moved rcv_nxt is OUT_OF_WINDOW by the header's
    rule (rel >= 2^31), in one batch as in many: such a frame would place bytes
    in the one batch that no later batch places."""
    rng = np.random.default_rng(77 * n + nflows)
    wnd = 8192
    flows = plan_flows(nflows, wnd, 0)
    frames = []
    per = max(2, n // nflows)
    for k, f in enumerate(flows):
        kw, nxt = flow_kw(f), int(f["rcv_nxt"])
        stream = rng.integers(0, 256, wnd, dtype=np.uint8)
        pos, mine = 0, []
        while len(mine) < per and pos < wnd - 100:
            dlen = min(int(rng.choice((1, 17, 100, 536, 1460))), wnd - 100 - pos)
            fr = tcp_frame(stream[pos:pos + dlen].tobytes(), nxt + pos, **kw)
            fate = rng.random()  # below 0.06 lost for good; below 0.2 lost, and sent again some places later
            late = float(rng.integers(4, 9)) if fate < 0.2 else 0.0
            if fate >= 0.06:
                mine.append((len(mine) + late + rng.integers(0, 4), fr))
            if rng.random() < 0.2:
                mine.append((len(mine) + rng.integers(0, 4), fr))
            pos += dlen
        mine += [(len(mine) / 2, tcp_frame(b"", nxt + 5, **kw)), (len(mine) / 3, tcp_frame(b"x" * 64, nxt + wnd - 10, **kw))]
        frames += mine
    order = np.argsort([key for key, _ in frames], kind="stable")  # the flows interleaved, each nearly in order
    frames = [frames[int(i)][1] for i in order]
    buf, fd = lvlip.pack_frames(frames, align_mod=16, seed=n)
    return frames, buf, fd, flows


@pytest.mark.parametrize("n,nflows", ((14, 1), (60, 3), (300, 17)))
def test_split_equals_whole(n, nflows):
    """Every 1-, 2- and 3-cut split of the small case and 60 seeded ones of the
    others.  Left out (more than four islands of a flow at a boundary): the
    share is asserted below one half and printed; it is 0 of 240 cuts at n = 14
    and 0 of 60 at n = 60 and at n = 300, while most boundaries have islands
    to carry (asserted too)."""
    frames, buf, fd, flows = split_case(n, nflows)
    m = len(frames)
    out_size = lvlip.lro_plan(flows.copy()) + 32
    whole = run_batches(buf, fd, flows, (), out_size)
    assert whole[1].sum() > 0 and (whole[3]["nsack"] > 0).any()
    if n == 14:
        splits = [c for r in (1, 2, 3) for c in itertools.combinations(range(1, m), r) if r < 3 or c[0] % 3 == 0]
    else:
        rng = np.random.default_rng(n)
        splits = [tuple(sorted(rng.choice(np.arange(1, m), int(rng.integers(1, 4)), replace=False).tolist()))
                  for _ in range(60)]
    used = [c for c in splits if cut_qualifies(frames, flows, c)]
    print(f"n {n}: {len(splits) - len(used)} of {len(splits)} cuts left out")
    assert len(used) > len(splits) / 2
    carrying = sum(any(islands_at(frames[:c], flows)) for cuts in used[:40] for c in cuts)
    assert carrying > sum(len(cuts) for cuts in used[:40]) / 2, "the boundaries carry nothing"
    for cuts in used:
        check_split(frames, buf, fd, flows, out_size, cuts, whole)


def test_a_fifth_island_is_forgotten_and_placed_again():
    """Five islands after the first batch: four are carried.  The second batch
    fills every hole, so the one batch delivers 950 bytes; cut in two, the
    prefix ends at 900, where the forgotten island began, and the peer's
    retransmission of those 50 bytes is placed and delivered by a third."""
    f = plan_flows(1, 4096, 0)
    one = np.array([_rec(0, 100 + 200 * j, 50) for j in range(5)], dtype=lvlip.LRO_REC_DTYPE)
    two = np.array([_rec(0, 0, 100)] + [_rec(0, 150 + 200 * j, 150) for j in range(4)], dtype=lvlip.LRO_REC_DTYPE)
    whole = lvlip.lro_advance_carry(f, np.concatenate([one, two]))
    assert int(whole[0]["delivered"]) == 950 and int(whole[0]["nsack"]) == 0
    res = lvlip.lro_advance_carry(f, one)
    assert int(res[0]["nsack"]) == 4 and int(res[0]["placed"]) == 5
    lvlip.lro_advance_carry(f, two, res, res)
    assert (int(res[0]["delivered"]), int(res[0]["nsack"]), int(res[0]["placed"])) == (900, 0, 5)
    lvlip.lro_next_cpu(f, res)
    again = np.array([_rec(0, 0, 50)], dtype=lvlip.LRO_REC_DTYPE)  # the peer re-sends [900, 950)
    lvlip.lro_advance_carry(f, again, res, res)
    assert int(res[0]["delivered"]) == 50
    lvlip.lro_next_cpu(f, res)
    assert int(f[0]["rcv_nxt"]) == (0xFFFFFF00 + 950) & M32 and int(f[0]["rcv_wnd"]) == 4096 - 950


# ------------------------------------------------------------------ the steps --

def guarded_copy(a: np.ndarray):
    """(bytes with 64 canary bytes on both sides, the array inside them)."""
    raw = np.full(a.nbytes + 128, CANARY, dtype=np.uint8)
    raw[64:64 + a.nbytes] = a.view(np.uint8).reshape(-1)
    return raw, raw[64:64 + a.nbytes].view(a.dtype)


def step_inputs(nflows: int, seed: int = 0):
    """Flows, results, send sides and their results with delivered and popped
    below, at and above rcv_wnd and nseg."""
    rng = np.random.default_rng(nflows + seed)
    flows = plan_flows(nflows, 4096, 0, rcv_nxt0=0xFFFFFFF4)
    res = np.zeros(nflows, dtype=lvlip.LRO_RESULT_DTYPE)
    res["delivered"] = rng.choice((0, 1, 4095, 4096, 4097, M32), nflows)
    res["placed"], res["nsack"] = rng.integers(0, 9, nflows), rng.integers(0, 5, nflows)
    res["sack"] = rng.integers(0, 1 << 32, (nflows, 4, 2))
    res["delivered"][0] = 4096 if nflows == 1 else 12  # the window reaches 0; rcv_nxt reaches 2^32 exactly
    res["delivered"][-1] = 4096 if nflows == 1 else M32
    snd = np.zeros(nflows, dtype=lvlip.SND_FLOW_DTYPE)
    snd["snd_una"] = rng.integers(0, 1 << 32, nflows)
    snd["snd_nxt"] = (snd["snd_una"].astype(np.uint64) + 50000) & M32
    snd["nseg"] = rng.integers(0, 6, nflows)
    snd["seg0"] = np.cumsum(np.concatenate([[7], snd["nseg"][:-1]]))
    snd["rtx"], snd["win"] = 2, 29200
    lvlip.snd_plan(snd)
    sres = np.zeros(nflows, dtype=lvlip.SND_RESULT_DTYPE)
    sres["acked"] = rng.integers(0, 50001, nflows)
    sres["snd_una"] = (snd["snd_una"].astype(np.uint64) + sres["acked"]) & M32
    for c in ("n_new", "n_dup", "n_old", "n_beyond"):
        sres[c] = rng.integers(0, 9, nflows)
    sres["popped"] = np.minimum(rng.integers(0, 8, nflows), 7)
    sres["popped"][-1] = M32
    sres["inflight"] = 0x55
    return flows, res, snd, sres


@pytest.mark.parametrize("nflows", (1, 3, 17, 300))
def test_steps_equal_model_clamp_and_consume(nflows):
    flows, res, snd, sres = step_inputs(nflows)
    assert nflows == 1 or ((res["delivered"] > flows["rcv_wnd"]).any() and (sres["popped"] > snd["nseg"]).any())
    want_f, want_r = model_lro_next(flows, res)
    want_s, want_q = model_snd_next(snd, sres)
    raws = [guarded_copy(a) for a in (flows, res, snd, sres)]
    (_, f), (_, r), (_, s), (_, q) = raws
    lvlip.lro_next_cpu(f, r)
    lvlip.snd_next_cpu(s, q)
    for got, want, what in ((f, want_f, "f"), (r, want_r, "res"), (s, want_s, "s"), (q, want_q, "snd res")):
        assert_same(got, want, what)
    for raw, _ in raws:
        assert (raw[:64] == CANARY).all() and (raw[-64:] == CANARY).all(), "written outside f, s or res"
    assert (f["rcv_wnd"] <= flows["rcv_wnd"]).all() and (s["nseg"] <= snd["nseg"]).all()
    assert (f["out_off"] + f["rcv_wnd"] == flows["out_off"] + flows["rcv_wnd"]).all(), "the range shrinks from its front"
    assert [x.tobytes()[:12] for x in f] == [x.tobytes()[:12] for x in flows] and (f["user"] == flows["user"]).all()
    assert (s["slot0"] == snd["slot0"]).all() and (s["rtx"] == 2).all() and (s["snd_nxt"] == snd["snd_nxt"]).all()
    assert (r["sack"] == res["sack"]).all() and (r["nsack"] == res["nsack"]).all() and (r["placed"] == res["placed"]).all()
    # twice changes nothing
    lvlip.lro_next_cpu(f, r)
    lvlip.snd_next_cpu(s, q)
    for got, want, what in ((f, want_f, "f"), (r, want_r, "res"), (s, want_s, "s"), (q, want_q, "snd res")):
        assert_same(got, want, what + ", applied twice")


def test_steps_leave_the_frames_ack_and_rtx_build():
    """lvlip_ack_cpu and lvlip_rtx_cpu after the steps build the frames they
    built before them, from a round of tests/test_snd_gpu.py's link on the CPU
    forms (frames lost, so there are islands and queue heads to re-send)."""
    from test_snd_gpu import Link

    link = Link(3, 12, 3)
    got = link.round_cpu(link.first_flight(np.random.default_rng(4)))
    res, sres = got["res"].copy(), got["sres"].copy()
    assert (res["delivered"] > 0).any() and (res["nsack"] > 0).any() and (sres["popped"] > 0).any()
    rres = np.zeros(3, dtype=lvlip.LRO_RESULT_DTYPE)  # the reverse direction: one byte of B's delivered
    rres["delivered"], rres["placed"] = 1, 1
    fb, fa, snd = link.fb.copy(), link.fa.copy(), link.snd.copy()

    def frames():
        ack, afd = lvlip.ack_cpu(link.tmpl, fb, res, lvlip.ACK_ALL, out=np.full(link.ack_bytes, CANARY, dtype=np.uint8))
        ring = link.ring.copy()
        fd_out = lvlip.rtx_cpu(fa, rres, snd, sres, ring, link.fd)
        return ack.tobytes(), afd.tobytes(), ring.tobytes(), fd_out.tobytes()

    before = frames()
    lvlip.lro_next_cpu(fb, res)
    lvlip.lro_next_cpu(fa, rres)
    lvlip.snd_next_cpu(snd, sres)
    assert (fb["rcv_nxt"] != link.fb["rcv_nxt"]).any() and (fa["rcv_nxt"] == 0x01020305).all()
    assert (snd["seg0"] != link.snd["seg0"]).any() and not sres["popped"].any()
    assert frames() == before
    assert lvlip.snd_plan(snd.copy())[0] == link.nslots, "the plan's nslots still holds"


def test_a_window_of_zero_places_nothing():
    """delivered == rcv_wnd: the window reaches 0; a data frame on that flow is
    OUT_OF_WINDOW and a pure ACK NO_DATA, and only the plan refuses the flow."""
    f = plan_flows(2, 1000, 0)
    kw, nxt = flow_kw(f[0]), int(f[0]["rcv_nxt"])
    data = bytes(range(250)) * 4
    buf, fd = lvlip.pack_frames([tcp_frame(data, nxt, **kw)], align_mod=16, seed=1)
    out, rec = lvlip.lro_cpu(buf, fd, f)
    res = lvlip.lro_advance_carry(f, rec)
    assert int(res[0]["delivered"]) == 1000
    lvlip.lro_next_cpu(f, res)
    assert int(f[0]["rcv_wnd"]) == 0 and int(f[0]["rcv_nxt"]) == (nxt + 1000) & M32 and int(f[1]["rcv_wnd"]) == 1000
    buf, fd = lvlip.pack_frames([tcp_frame(b"more", nxt + 1000, **kw), tcp_frame(b"", nxt + 1000, **kw)], align_mod=16, seed=2)
    before = out.copy()
    out, rec = lvlip.lro_cpu(buf, fd, f, out=out)
    assert rec["status"].tolist() == [lvlip.LRO_OUT_OF_WINDOW, lvlip.LRO_NO_DATA] and rec["flow"].tolist() == [0, 0]
    assert np.array_equal(out, before)
    lvlip.lro_advance_carry(f, rec, res, res)
    assert not res["delivered"].any() and not res["placed"].any()
    with pytest.raises(ValueError):
        lvlip.lro_plan(f.copy())


def test_refusals_without_gpu():
    """Host memory stands in for the device pointers: a refused call touches
    none of it and makes no HIP call."""
    L = lvlip.lib()
    flows, rec, prev = random_case(16, 3)
    _, res, snd, sres = step_inputs(3)
    keep = [a.copy() for a in (flows, prev, res, snd, sres)]
    out = np.full(3 * 48 + 16, 0x5A, dtype=np.uint8)
    ws = np.zeros(1 << 16, dtype=np.uint8)
    f, r, p, o = flows.ctypes.data, rec.ctypes.data, prev.ctypes.data, out.ctypes.data
    o += -o % 16
    w = ws.ctypes.data
    w += -w % 256
    assert f % 8 == 0 and r % 16 == 0 and p % 16 == 0
    size = 1 << 15
    # the host form: lvlip_lro_advance's refusals
    for args in ((None, 3, r, 16, p, o), (f, 3, r, 16, p, None), (f, 3, None, 16, p, o)):
        assert L.lvlip_lro_advance_carry(*args) == lvlip.EINVAL
    assert L.lvlip_lro_advance_carry(None, 0, None, 0, None, None) == lvlip.OK
    refused = {"NULL f": (None, 3, r, 16, p, o, w, size), "NULL res": (f, 3, r, 16, p, None, w, size),
               "NULL rec": (f, 3, None, 16, p, o, w, size), "n above LVLIP_MAX_BATCH": (f, 3, r, 0xFFFFFFF1, p, o, w, size),
               "nflows above LVLIP_LRO_MAX_FLOWS": (f, 65537, r, 16, p, o, w, size),
               "n + 4 nflows above LVLIP_MAX_BATCH": (f, 3, r, 0xFFFFFFF0 - 11, p, o, w, size),
               "NULL workspace": (f, 3, r, 16, p, o, None, size), "NULL workspace, no records": (f, 3, None, 0, p, o, None, size),
               "NULL workspace, no prev": (f, 3, r, 16, None, o, None, size),
               "workspace at 128 mod 256": (f, 3, r, 16, p, o, w + 128, size),
               "misaligned f": (f + 4, 3, r, 16, p, o, w, size), "misaligned rec": (f, 3, r + 8, 16, p, o, w, size),
               "misaligned res": (f, 3, r, 16, p, o + 8, w, size), "misaligned prev": (f, 3, r, 16, p + 8, o, w, size)}
    for what, args in refused.items():
        assert L.lvlip_lro_advance_carry_dev(*args, None) == lvlip.EINVAL, what
    assert L.lvlip_lro_advance_carry_dev(None, 0, r, 16, p, None, None, 0, None) == lvlip.OK
    assert L.lvlip_lro_advance_carry_workspace_bytes(16, 0) == 0
    assert L.lvlip_lro_advance_carry_workspace_bytes(0xFFFFFFF0 - 11, 3) == 0
    assert L.lvlip_lro_advance_carry_workspace_bytes(16, 65537) == 0
    if lvlip.device_count() == 0:
        assert L.lvlip_lro_advance_carry_workspace_bytes(16, 3) == 0
        assert L.lvlip_lro_advance_carry_dev(f, 3, r, 16, p, o, w, size, None) == lvlip.ENODEV
    # the steps
    s, q, rr = snd.ctypes.data, sres.ctypes.data, res.ctypes.data
    assert rr % 16 == 0 and q % 16 == 0 and s % 8 == 0
    for cpu, dev, a, b in ((L.lvlip_lro_next_cpu, L.lvlip_lro_next_dev, f, rr),
                           (L.lvlip_snd_next_cpu, L.lvlip_snd_next_dev, s, q)):
        for args in ((None, b, 3), (a, None, 3), (a, b, 65537)):
            assert cpu(*args) == lvlip.EINVAL
            assert dev(*args, None) == lvlip.EINVAL
        assert dev(a + 4, b, 3, None) == lvlip.EINVAL and dev(a, b + 8, 3, None) == lvlip.EINVAL
        assert cpu(None, None, 0) == lvlip.OK and dev(None, None, 0, None) == lvlip.OK
    for a, k in zip((flows, prev, res, snd, sres), keep):
        assert a.tobytes() == k.tobytes()
    assert (out == 0x5A).all() and not ws.any()
    with pytest.raises(ValueError):
        lvlip.lro_next_cpu(flows.copy(), res[:2].copy())
    with pytest.raises(TypeError):
        lvlip.snd_next_cpu(snd.view(np.uint8), sres)


# ------------------------------------------------------------- the whole loop --

SEGS, WND_SEGS, ROUNDS = 40, 8, 40


class StreamLoop:
    """tests/test_snd_gpu.py's link, 8 flows x 40 segments of 536 B, run the
    continuous way: B's window is 8 segments and slides, A sends 8 queue entries
    per flow and round through the scoreboard, every record array is one
    round's nslots frames.  The network: an entry whose index is 4 mod 5 is
    lost the first time it is sent; what is sent again arrives.  The window is
    opened again after each round by the application (the caller's step):
    rcv_wnd = min(window, what is left of the region)."""

    def __init__(self, nflows: int = 8):
        from test_snd_gpu import MSS, Link

        self.link = L = Link(nflows, SEGS, WND_SEGS)
        self.mss, self.nflows, self.nslots = MSS, nflows, L.nslots
        self.wnd = WND_SEGS * MSS
        self.end = (L.fb["out_off"] + L.fb["rcv_wnd"]).astype(np.uint64)
        self.fb = L.fb.copy()
        self.fb["rcv_wnd"] = self.wnd
        assert self.nslots == nflows * WND_SEGS and SEGS % 5 == 0

    def run_cpu(self):
        L, n = self.link, self.nflows
        fb, fa, snd, ring = self.fb.copy(), L.fa.copy(), L.snd.copy(), L.ring.copy()
        stream = np.full(L.stream.size, CANARY, dtype=np.uint8)
        res = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
        sres = np.zeros(n, dtype=lvlip.SND_RESULT_DTYPE)
        sacked = np.zeros(L.fd.size, dtype=np.uint8)
        sent = np.zeros(L.fd.size, dtype=np.int32)
        most = 0
        for _ in range(ROUNDS):
            fd_out, pick = lvlip.rtx_sack_cpu(fa, None, snd, sres, sacked, ring, L.fd)
            live = pick != lvlip.SACK_NO_PICK
            idx = np.where(live, pick, 0)
            lost = live & (sent[idx] == 0) & (idx % 5 == 4)
            np.add.at(sent, idx, live.astype(np.int32))
            wire = fd_out.copy()
            wire["len"][lost] = 0
            _, rec = lvlip.lro_cpu(ring, wire, fb, lvlip.RX_VERIFY_L4, out=stream)
            most = max(most, rec.size)
            lvlip.lro_advance_carry(fb, rec, res, res)
            ack, afd = lvlip.ack_cpu(L.tmpl, fb, res, lvlip.ACK_ALL, out=np.full(L.ack_bytes, CANARY, dtype=np.uint8))
            lvlip.lro_next_cpu(fb, res)
            fb["rcv_wnd"] = np.minimum(self.wnd, self.end - fb["out_off"])
            _, arec = lvlip.lro_cpu(ack, afd, fa, lvlip.RX_VERIFY_L4, out=np.zeros(n + 64, dtype=np.uint8))
            sres = lvlip.snd_cpu(fa, snd, arec, ring, L.fd)
            lvlip.sack_cpu(fa, snd, arec, ack, afd, ring, L.fd, sacked)
            lvlip.snd_next_cpu(snd, sres)
        return dict(stream=stream, fb=fb, snd=snd, res=res, sres=sres, ring=ring, sacked=sacked, sent=sent, most=most)

    def check_done(self, got: dict):
        L = self.link
        assert np.array_equal(got["stream"], L.payload), "the streams are not the payloads"
        assert not got["snd"]["nseg"].any() and (got["snd"]["snd_una"] == got["snd"]["snd_nxt"]).all()
        assert (got["fb"]["rcv_nxt"] == got["snd"]["snd_nxt"]).all() and not got["fb"]["rcv_wnd"].any()
        assert (got["fb"]["out_off"] == self.end).all()
        assert not got["sres"]["popped"].any() and not got["sres"]["inflight"].any()
        assert got["most"] == self.nslots, "a round's records are one round's frames"
        assert (got["sent"][np.arange(L.fd.size) % 5 == 4] >= 2).all(), "every lost frame went out again"


@functools.lru_cache(maxsize=None)
def stream_loop_cpu():
    loop = StreamLoop()
    return loop, loop.run_cpu()


def test_the_loop_with_loss_on_the_cpu_forms():
    """40 rounds, the queue's length: every round the head of an unfinished
    queue is sent, and unless that is its first time it arrives, so the prefix
    grows by a segment a round at least."""
    loop, got = stream_loop_cpu()
    loop.check_done(got)


def test_example_under_sanitizers(tmp_path):
    """examples/stream_loop.c (its own main: the transfer of snd_loop.c with
    one round's records, sliding windows and the steps, on the CPU forms, every
    buffer malloc'd at exactly its planned size) compiled with the library's C
    sources under ASan + UBSan, and run as a program."""
    exe = tmp_path / "stream_loop_san"
    src = [os.path.join(ROOT, "examples", "stream_loop.c")] + [
        os.path.join(ROOT, "level-ip_amd", "csrc", f)
        for f in ("sack_cpu.c", "snd_cpu.c", "ack_cpu.c", "rcv_cpu.c", "seg_cpu.c", "csum_cpu.c")]
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "include"), *src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stream_loop ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_new_kernels_use_no_scratch(tmp_path):
    """k_lro_next, k_snd_next, the carry form's key and emit kernels and both
    instantiations of the scan kernels: every private segment is 0."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    found = []
    for name, pat in (("next_kernels", r"k_(?:lro|snd)_next"), ("adv_kernels", r"k_adv_\w+")):
        asm = tmp_path / f"{name}.s"
        subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "-S", "--cuda-device-only", os.path.join(ROOT, "level-ip_amd", "csrc", f"{name}.hip"),
                        "-o", str(asm)], check=True, capture_output=True)
        found += re.findall(r"\.name:\s+(\S*" + pat + r"\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)",
                            asm.read_text())
    names = [name for name, _ in found]
    for want in ("k_lro_next", "k_snd_next", "k_adv_keys_carry", "k_adv_emit_carry"):
        assert any(want in name for name in names), (want, names)
    for tmpl in ("k_adv_reduce", "k_adv_heads"):  # the 2-B and the 4-B lengths
        assert len([name for name in names if tmpl in name]) == 2, (tmpl, names)
    assert all(int(size) == 0 for _, size in found), found
