"""lvlip_sack_dev and lvlip_rtx_sack_dev on the MI355X (sack_kernels.hip,
snd_kernels.hip): every byte of res, of the scoreboard, of pick, of fd_out and
of the ring against lvlip_sack_cpu / lvlip_rtx_sack_cpu on the same inputs,
the inputs only read, canaries around every output; the reference's own ACK
frames (tests/golden/ack_ref.json); the whole chain with the two calls at its
end on one stream with a single synchronise, and a transfer with loss run to
its end through the device calls.

The record counts straddle a wave (63, 64, 65) and k_sack_parse's workgroup of
SACK_TILE = 256 records (255, 256, 257), and 3000 records make a grid of twelve.
The queues of test_sack_cpu.queues() put 63, 64, 65 and 300 entries against
the 64 entries a wave of k_sack_mark and of k_pick handles per step, and its
six flows against their SACK_WAVES = SND_WAVES = 4 flows per workgroup; a queue
of 66 000 entries passes the 64 * SACK_Y = 65 536 entries one sweep of
k_sack_mark's chunks covers, so that a wave takes a second step; with 2100
flows a queue gets SACK_GRID / 525 = 249 chunks, and a queue of 20 000 among
them passes that sweep too."""
import functools

import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import _t
from test_sack_cpu import NO_PICK, ack_frame, golden_check, in_queues, make_acks, marks_case, queues, sack_opt
from test_snd_cpu import CANARY, GUARD, M32, Case, hand
from test_snd_gpu import MSS, Link

pytestmark = pytest.mark.gpu

SACK_TILE, SACK_WAVES, SACK_Y, SACK_Y_MIN, SACK_GRID = 256, 4, 1024, 8, 1 << 17  # sack_kernels.hip


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


def run_sack_dev(c, rec, aring, afd, dev, sacked=None, stream=None):
    """lvlip_sack_dev with canaries around the scoreboard (at an odd address)
    and behind res; the inputs compared afterwards.  Returns (res, board)."""
    n, nfd = c.flows.size, c.fd.size
    inputs = (c.flows, c.snd, rec, aring, afd, c.ring, c.fd)
    ins = [_t(a, dev) for a in inputs]
    res_t = torch.full((16 * n + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    board_t = torch.full((7 + nfd + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    board_t[7:7 + nfd] = 0 if sacked is None else torch.from_numpy(sacked).to(dev)
    torch.cuda.synchronize(dev)
    lvlip.sack_dev(*ins, board_t[7:7 + nfd], res_t[:16 * n], stream=stream)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    board = board_t.cpu().numpy()
    assert (res_t[16 * n:] == CANARY).all(), "written behind res"
    assert (board[:7] == CANARY).all() and (board[7 + nfd:] == CANARY).all(), "written around the scoreboard"
    for name, t, a in zip(("f", "s", "rec", "ack_base", "ack_fd", "base", "fd"), ins, inputs):
        assert np.array_equal(t.cpu().numpy(), a.view(np.uint8).reshape(-1)), f"{name} is only read"
    return res_t[:16 * n].cpu().numpy().view(lvlip.SACK_RESULT_DTYPE), board[7:7 + nfd]


def cpu_sack(c, rec, aring, afd, sacked=None):
    board = np.zeros(c.fd.size, dtype=np.uint8) if sacked is None else sacked.copy()
    return lvlip.sack_cpu(c.flows, c.snd, rec, aring, afd, c.ring, c.fd, board), board


def assert_same(got, want, what):
    (gres, gboard), (wres, wboard) = got, want
    if gres.tobytes() != wres.tobytes():
        k = int(np.flatnonzero(gres != wres)[0])
        pytest.fail(f"{what}: flow {k}: got {gres[k]}, want {wres[k]}; {int((gres != wres).sum())} flows differ")
    if not np.array_equal(gboard, wboard):
        bad = np.flatnonzero(gboard != wboard)
        pytest.fail(f"{what}: {bad.size} scoreboard bytes differ, first at entry {int(bad[0])}: got {int(gboard[bad[0]])}")


# ----------------------------------------------------------- the scoreboard --

@pytest.mark.parametrize("n", (1, 63, 64, 65, SACK_TILE - 1, SACK_TILE, SACK_TILE + 1, 3000))
def test_sack_dev_equals_cpu_by_records(n, dev):
    c = queues()
    rec, aring, afd = make_acks(c, n, seed=n)
    before = (np.random.default_rng(n).integers(0, 8, c.fd.size) == 0).astype(np.uint8) * (1 + n % 2)
    want = cpu_sack(c, rec, aring, afd, before)
    assert_same(run_sack_dev(c, rec, aring, afd, dev, sacked=before), want, f"n {n}")
    if n >= 63:
        assert (want[0]["n_valid"] > 0).any() and ((want[1] == 1) & (before == 0)).any()
        assert ((want[1] == before) | ((want[1] == 1) & in_queues(c))).all()


def test_sack_dev_the_hand_case(dev):
    """snd_una 12 bytes below 2^32, a queue out of sequence order, spans of 0."""
    c = hand()
    rec, aring, afd = make_acks(c, 600, seed=3)
    want = cpu_sack(c, rec, aring, afd)
    assert int(want[0][0]["n_sacked"]) > 0, "blocks that wrap mark entries"
    assert_same(run_sack_dev(c, rec, aring, afd, dev), want, "hand")


def test_sack_dev_every_record_of_one_flow(dev):
    """The wave reduces before its atomics; the same batch permuted."""
    c = queues()
    rec, aring, afd = make_acks(c, 600, seed=5, one_flow=5, blocks_only=True)
    want = cpu_sack(c, rec, aring, afd)
    assert int(want[0][5]["n_blocks"]) >= 600 == int((rec["flow"] == 5).sum()) and int(want[0][5]["n_sacked"]) > 30
    assert_same(run_sack_dev(c, rec, aring, afd, dev), want, "one flow")
    p = np.random.default_rng(0).permutation(600)
    assert_same(run_sack_dev(c, rec[p], aring, afd[p], dev), want, "one flow, permuted")


@functools.lru_cache(maxsize=None)
def many_flows() -> Case:
    k = np.arange(301)
    return Case(nseg=[int(v) for v in (k * 3 + 1) % 5], mss=[int(v) for v in 8 + 8 * (k % 5)], seed=301)


def test_sack_dev_one_record_per_flow(dev):
    """301 flows (76 workgroups of SACK_WAVES, the last with one flow), one
    record each, in a shuffled order."""
    c = many_flows()
    parts = [make_acks(c, 1, seed=k, one_flow=k, blocks_only=True) for k in range(301)]
    order = np.random.default_rng(1).permutation(301)
    rec = np.concatenate([parts[k][0] for k in order])
    afd, rings, off = [], [], 0
    for k in order:
        d = parts[k][2].copy()
        d["offset"] += off
        afd.append(d)
        rings.append(parts[k][1])
        off += parts[k][1].size
    aring, afd = np.concatenate(rings), np.concatenate(afd)
    want = cpu_sack(c, rec, aring, afd)
    assert int((want[0]["n_blocks"] > 0).sum()) == 301 and int(want[0]["n_sacked"].sum()) > 50
    assert_same(run_sack_dev(c, rec, aring, afd, dev), want, "one record per flow")


@functools.lru_cache(maxsize=None)
def long_queue() -> Case:
    return Case(nseg=[66000], mss=[8], rtx=[100], seed=66)


def test_sack_dev_a_queue_beyond_one_sweep(dev):
    """One flow: k_sack_mark's SACK_Y chunks of 64 entries cover 65 536, and
    the queue holds 66 000; 2000 records of one block of 20 entries each."""
    c = long_queue()
    assert int(c.snd[0]["nseg"]) > 64 * SACK_Y
    una, rng = int(c.snd[0]["snd_una"]), np.random.default_rng(8)
    frames = [ack_frame(rng, b"\1\1" + sack_opt([((una + 8 * 33 * j) & M32, (una + 8 * (33 * j + 20)) & M32)]))
              for j in rng.permutation(2000)]  # entries 33 j .. 33 j + 19 of every 33
    aring = np.frombuffer(b"".join(frames), dtype=np.uint8).copy()
    afd = np.array([(66 * i, 66, 0) for i in range(2000)], dtype=lvlip.FRAME_DESC_DTYPE)
    rec = np.array([(0, 0, 0, lvlip.LRO_NO_DATA, 0x10, una)] * 2000, dtype=lvlip.LRO_REC_DTYPE)
    want = cpu_sack(c, rec, aring, afd)
    marked = np.flatnonzero(want[1])
    assert marked.size == 2000 * 20 and marked.max() == 33 * 1999 + 19 >= 64 * SACK_Y, "marks behind the first sweep"
    assert_same(run_sack_dev(c, rec, aring, afd, dev), want, "long queue")


@functools.lru_cache(maxsize=None)
def long_among_many() -> Case:
    return Case(nseg=[20000] + [1] * 2099, mss=[8] * 2100, rtx=[1] * 2100, seed=21)


def test_sack_dev_a_long_queue_among_many_flows(dev):
    """2100 flows make 525 workgroups of SACK_WAVES, so a queue is spread over
    SACK_GRID / 525 = 249 chunks of 64 = 15 936 entries a sweep; flow 0 holds
    20 000, and its waves take a second step."""
    c = long_among_many()
    y = SACK_GRID // -(-2100 // SACK_WAVES)
    assert SACK_Y_MIN <= y < SACK_Y and 64 * y < int(c.snd[0]["nseg"])
    una, rng = int(c.snd[0]["snd_una"]), np.random.default_rng(9)
    frames = [ack_frame(rng, b"\1\1" + sack_opt([((una + 8 * 33 * j) & M32, (una + 8 * (33 * j + 20)) & M32)]))
              for j in rng.permutation(600)]
    rec0 = np.array([(0, 0, 0, lvlip.LRO_NO_DATA, 0x10, una)] * 600, dtype=lvlip.LRO_REC_DTYPE)
    rec1, aring1, afd1 = make_acks(c, 300, seed=4)
    aring = np.concatenate([np.frombuffer(b"".join(frames), dtype=np.uint8), aring1])
    afd = np.concatenate([np.array([(66 * i, 66, 0) for i in range(600)], dtype=lvlip.FRAME_DESC_DTYPE), afd1])
    afd["offset"][600:] += 66 * 600
    rec = np.concatenate([rec0, rec1])
    want = cpu_sack(c, rec, aring, afd)
    q0 = int(c.snd[0]["seg0"])
    marked = np.flatnonzero(want[1][q0:q0 + 20000])
    assert marked.size >= 600 * 20 and marked.max() >= 64 * y, "marks behind the first sweep"
    assert_same(run_sack_dev(c, rec, aring, afd, dev), want, "a long queue among many flows")


def test_sack_dev_accumulates_and_repeats_on_a_stream(dev):
    c = queues()
    rec, aring, afd = make_acks(c, 400, seed=9)
    s = torch.cuda.Stream(dev)
    _, half = cpu_sack(c, rec[:200], aring, afd[:200])
    want = cpu_sack(c, rec[200:], aring, afd[200:], half)
    _, got_half = run_sack_dev(c, rec[:200], aring, afd[:200], dev, stream=s)
    assert np.array_equal(got_half, half)
    assert_same(run_sack_dev(c, rec[200:], aring, afd[200:], dev, sacked=got_half, stream=s), want, "second call")
    assert_same(run_sack_dev(c, rec[200:], aring, afd[200:], dev, sacked=got_half), want, "again, default stream")


def test_sack_dev_workspace_too_small(dev):
    c = queues()
    rec, aring, afd = make_acks(c, 64, seed=1)
    need = lvlip.sack_workspace_bytes(64, c.flows.size)
    assert need >= 96 * 64
    ins = [_t(a, dev) for a in (c.flows, c.snd, rec, aring, afd, c.ring, c.fd)]
    board_t = torch.full((c.fd.size,), CANARY, dtype=torch.uint8, device=dev)
    res_t = torch.full((16 * c.flows.size,), CANARY, dtype=torch.uint8, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    with pytest.raises(lvlip.LvlipError) as e:
        lvlip.sack_dev(*ins, board_t, res_t, workspace_t=ws[:need - 1])
    torch.cuda.synchronize(dev)
    assert e.value.rc == lvlip.ERANGE
    assert (board_t == CANARY).all() and (res_t == CANARY).all(), "nothing written"
    lvlip.sack_dev(*ins, board_t, res_t, workspace_t=ws)  # exactly enough
    torch.cuda.synchronize(dev)
    assert not (res_t == CANARY).all()


def test_sack_dev_marks_what_the_reference_reported(dev):
    def sack(flow, snd, rec, abuf, afd, ring, fd):
        board_t = torch.zeros(fd.size, dtype=torch.uint8, device=dev)
        res_t = lvlip.sack_dev(_t(flow, dev), _t(snd, dev), _t(rec, dev), _t(abuf, dev), _t(afd, dev), _t(ring, dev),
                               _t(fd, dev), board_t)
        torch.cuda.synchronize(dev)
        board = board_t.cpu().numpy()
        cpu = np.zeros(fd.size, dtype=np.uint8)
        cpu_res = lvlip.sack_cpu(flow, snd, rec, abuf, afd, ring, fd, cpu)
        res = res_t.cpu().numpy().view(lvlip.SACK_RESULT_DTYPE)
        assert np.array_equal(board, cpu) and res.tobytes() == cpu_res.tobytes()
        return res, board

    golden_check(sack)


# --------------------------------------------------- the selective retransmit --

def run_rtx_sack_dev(c, lro, sres, sacked, dev):
    """lvlip_rtx_sack_dev on a copy of the ring, canaries behind fd_out and
    pick.  Returns (ring, fd_out, pick) on the host."""
    f_t, s_t, fd_t, ring_t = _t(c.flows, dev), _t(c.snd, dev), _t(c.fd, dev), _t(c.ring, dev)
    board_t = _t(sacked, dev) if sacked is not None else None
    out_t = torch.full((16 * c.nslots + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    pick_t = torch.full((4 * c.nslots + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    lvlip.rtx_sack_dev(f_t, _t(lro, dev) if lro is not None else None, s_t, _t(sres, dev) if sres is not None else None,
                       board_t, c.nslots, ring_t, fd_t, out_t[:16 * c.nslots], pick_t[:4 * c.nslots])
    torch.cuda.synchronize(dev)
    assert (out_t[16 * c.nslots:] == CANARY).all() and (pick_t[4 * c.nslots:] == CANARY).all(), "written behind an output"
    assert np.array_equal(fd_t.cpu().numpy(), c.fd.view(np.uint8).reshape(-1)), "fd is only read"
    if sacked is not None:
        assert np.array_equal(board_t.cpu().numpy(), sacked), "the scoreboard is only read"
    return (ring_t.cpu().numpy(), out_t[:16 * c.nslots].cpu().numpy().view(lvlip.FRAME_DESC_DTYPE),
            pick_t[:4 * c.nslots].cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("seed", (0, 1, None))
def test_rtx_sack_dev_equals_cpu(seed, dev):
    """Queues of 0 .. 300 entries, rtx up to 70, marks on two thirds of the
    entries (None: no scoreboard); flow 4 has one free entry, its last."""
    c, sacked, lro, sres = marks_case(seed or 0)
    if seed is None:
        sacked = None
    want = c.ring.copy()
    want_fd, want_pick = lvlip.rtx_sack_cpu(c.flows, lro, c.snd, sres, sacked, want, c.fd)
    got, got_fd, got_pick = run_rtx_sack_dev(c, lro, sres, sacked, dev)
    assert np.array_equal(got_pick, want_pick) and got_fd.tobytes() == want_fd.tobytes()
    assert np.array_equal(got, want), f"{int((got != want).sum())} ring bytes differ"
    assert (want_pick != NO_PICK).sum() > 10 and (want_pick == NO_PICK).any() and not np.array_equal(want, c.ring)
    if seed is None:
        plain = c.ring.copy()
        plain_fd = lvlip.rtx_cpu(c.flows, lro, c.snd, sres, plain, c.fd)
        assert np.array_equal(got, plain) and got_fd.tobytes() == plain_fd.tobytes(), "without a scoreboard: lvlip_rtx_*"


def test_rtx_sack_dev_a_long_scan(dev):
    """66 000 entries, the first 65 000 marked but every 1000th: the selection
    scans a thousand steps of 64 and still fills its 100 slots in order."""
    c = long_queue()
    sacked = np.zeros(c.fd.size, dtype=np.uint8)
    sacked[:65000] = 1
    sacked[999:65000:1000] = 0
    want = c.ring.copy()
    want_fd, want_pick = lvlip.rtx_sack_cpu(c.flows, None, c.snd, None, sacked, want, c.fd)
    assert want_pick[:66].tolist() == list(range(999, 65000, 1000)) + [65000] and (want_pick != NO_PICK).all()
    got, got_fd, got_pick = run_rtx_sack_dev(c, None, None, sacked, dev)
    assert np.array_equal(got_pick, want_pick) and got_fd.tobytes() == want_fd.tobytes() and np.array_equal(got, want)


# ---------------------------------------------------------------- the chain --

class SackLink(Link):
    """test_snd_gpu.Link with the scoreboard: lvlip_sack_* behind lvlip_snd_*,
    and lvlip_rtx_sack_* in the place of lvlip_rtx_*."""

    def __init__(self, nflows, segs, rtx, dev=None):
        super().__init__(nflows, segs, rtx, dev)
        self.sacked = np.zeros(self.fd.size, dtype=np.uint8)
        if dev is not None:
            self.t["sacked"] = torch.zeros(self.fd.size, dtype=torch.uint8, device=dev)
            self.t["kres"] = torch.zeros(16 * nflows, dtype=torch.uint8, device=dev)
            self.t["pick"] = torch.zeros(4 * self.nslots, dtype=torch.uint8, device=dev)
            self.t["kws"] = torch.empty(lvlip.sack_workspace_bytes(nflows, nflows), dtype=torch.uint8, device=dev)

    def round_cpu(self, wire, use_sack=True):
        _, rec = lvlip.lro_cpu(self.ring, wire, self.fb, lvlip.RX_VERIFY_L4, out=self.stream)
        self.rec = np.concatenate([self.rec, rec])
        res = lvlip.lro_advance(self.fb, self.rec)
        ack, afd = lvlip.ack_cpu(self.tmpl, self.fb, res, lvlip.ACK_ALL, out=np.full(self.ack_bytes, CANARY, dtype=np.uint8))
        _, arec = lvlip.lro_cpu(ack, afd, self.fa, lvlip.RX_VERIFY_L4, out=np.zeros(self.nflows + GUARD, dtype=np.uint8))
        sres = lvlip.snd_cpu(self.fa, self.snd, arec, self.ring, self.fd)
        if not use_sack:
            fd_out = lvlip.rtx_cpu(self.fa, None, self.snd, sres, self.ring, self.fd)
            return dict(res=res, sres=sres, fd_out=fd_out, stream=self.stream.copy())
        kres = lvlip.sack_cpu(self.fa, self.snd, arec, ack, afd, self.ring, self.fd, self.sacked)
        fd_out, pick = lvlip.rtx_sack_cpu(self.fa, None, self.snd, sres, self.sacked, self.ring, self.fd)
        return dict(rec=self.rec.copy(), res=res, ack=ack, afd=afd, arec=arec, sres=sres, kres=kres,
                    sacked=self.sacked.copy(), fd_out=fd_out, pick=pick, ring=self.ring.copy(), stream=self.stream.copy())

    def round_dev(self, wire, stream):
        """The eight calls on `stream`, one synchronise at the end."""
        t, n = self.t, wire.size
        assert self.nrec + n <= self.cap
        wire_t, snd_t = _t(wire, self.dev), _t(self.snd, self.dev)
        t["ack"].fill_(CANARY)
        torch.cuda.synchronize(self.dev)  # the uploads; nothing below waits again
        lvlip.lro_dev(t["ring"], wire_t, t["fb"], lvlip.RX_VERIFY_L4, t["stream"],
                      t["rec"][16 * self.nrec:16 * (self.nrec + n)], stream=stream)
        self.nrec += n
        lvlip.lro_advance_dev(t["fb"], t["rec"][:16 * self.nrec], t["res"], t["ws"], stream=stream)
        lvlip.ack_dev(t["tmpl"], t["fb"], t["res"], lvlip.ACK_ALL, t["ack"], t["afd"], stream=stream)
        lvlip.lro_dev(t["ack"], t["afd"], t["fa"], lvlip.RX_VERIFY_L4, t["sink"], t["arec"], stream=stream)
        lvlip.snd_dev(t["fa"], snd_t, t["arec"], t["ring"], t["fd"], t["sres"], stream=stream)
        lvlip.sack_dev(t["fa"], snd_t, t["arec"], t["ack"], t["afd"], t["ring"], t["fd"], t["sacked"], t["kres"],
                       workspace_t=t["kws"], stream=stream)
        lvlip.rtx_sack_dev(t["fa"], None, snd_t, t["sres"], t["sacked"], self.nslots, t["ring"], t["fd"], t["fd_out"],
                           t["pick"], stream=stream)
        stream.synchronize()
        h = lambda k, dt=np.uint8: t[k].cpu().numpy().view(dt)  # noqa: E731
        return dict(rec=h("rec", lvlip.LRO_REC_DTYPE)[:self.nrec], res=h("res", lvlip.LRO_RESULT_DTYPE), ack=h("ack"),
                    afd=h("afd", lvlip.FRAME_DESC_DTYPE), arec=h("arec", lvlip.LRO_REC_DTYPE),
                    sres=h("sres", lvlip.SND_RESULT_DTYPE), kres=h("kres", lvlip.SACK_RESULT_DTYPE), sacked=h("sacked"),
                    fd_out=h("fd_out", lvlip.FRAME_DESC_DTYPE), pick=h("pick", np.uint32), ring=h("ring"),
                    stream=h("stream"))


def lose(fd_out: np.ndarray, rng) -> np.ndarray:
    live = fd_out[fd_out["len"] > 0]
    live = live[np.arange(live.size) % 5 != 4] if live.size > 1 else live
    return live[rng.permutation(live.size)]


def run_to_the_end(link, round_of, rng):
    """(rounds, frames re-sent); asserts the transfer ends and delivers."""
    wire, resent = link.first_flight(rng), 0
    for rnd in range(40):
        got = round_of(wire)
        if "pick" in got:
            live = got["pick"][got["pick"] != NO_PICK]
            assert not got["sacked"][live].any(), f"round {rnd}: a picked entry is marked"
            assert np.array_equal(got["pick"] != NO_PICK, got["fd_out"]["len"] > 0)
        link.carry_on(got["sres"])
        if not link.snd["nseg"].any():
            break
        resent += int((got["fd_out"]["len"] > 0).sum())
        wire = lose(got["fd_out"], rng)
    assert (got["sres"]["inflight"] == 0).all() and not link.snd["nseg"].any(), f"not done after {rnd + 1} rounds"
    assert (got["res"]["delivered"] == link.segs * MSS).all()
    assert np.array_equal(got["stream"], link.payload), "the streams are not the payloads"
    assert (link.snd["snd_una"] == link.snd["snd_nxt"]).all(), "something is in flight"
    return rnd + 1, resent


def test_the_chain_with_the_scoreboard(dev, capsys):
    """8 flows x 40 segments of 536 B, every fifth frame lost, rtx 8, max_sack
    4.  Round 1 on one stream with one synchronise against the CPU forms, byte
    for byte, and against what the loss pattern says: the ACK of every flow
    acknowledges 4 segments and reports the islands 5-8, 10-13, 15-18 and
    20-23, so the holes 4, 9, 14, 19 and then 24-27 are picked.  Then the
    transfer to its end through the device calls, and the same transfer on the
    CPU forms with and without the scoreboard."""
    host, gpu = SackLink(8, 40, 8), SackLink(8, 40, 8, dev)
    s = torch.cuda.Stream(dev)
    wire = host.first_flight(np.random.default_rng(7))
    want, got = host.round_cpu(wire), gpu.round_dev(wire, s)
    for k in ("rec", "res", "afd", "arec", "sres", "kres", "sacked", "pick", "fd_out", "ack", "ring", "stream"):
        assert got[k].tobytes() == want[k].tobytes(), f"round 1: {k}"
    assert (want["sres"]["popped"] == 4).all()
    for k in range(8):
        q = int(host.snd[k]["seg0"])
        marks = [e for lo in (5, 10, 15, 20) for e in range(lo, lo + 4)]
        assert (np.flatnonzero(want["sacked"][q:q + 40]) == marks).all(), f"flow {k}"
        assert want["pick"][8 * k:8 * k + 8].tolist() == [q + e for e in (4, 9, 14, 19, 24, 25, 26, 27)], f"flow {k}"
    assert (want["kres"]["n_blocks"] == 4).all() and (want["kres"]["n_sacked"] == 16).all()

    totals = {}
    link = SackLink(8, 40, 8, dev)
    totals["device, scoreboard"] = run_to_the_end(link, lambda w: link.round_dev(w, s), np.random.default_rng(7))
    for name, use in (("cpu, scoreboard", True), ("cpu, head of the queue", False)):
        cpu = SackLink(8, 40, 8)
        totals[name] = run_to_the_end(cpu, lambda w, cpu=cpu, use=use: cpu.round_cpu(w, use), np.random.default_rng(7))
    assert totals["device, scoreboard"] == totals["cpu, scoreboard"]
    with capsys.disabled():
        print("\n(rounds, frames re-sent):", totals)
