"""lvlip_snd_dev and lvlip_rtx_dev on the MI355X (snd_kernels.hip): every byte
of res, of the whole ring and of fd_out against lvlip_snd_cpu / lvlip_rtx_cpu
on the same inputs; the whole chain lvlip_lro_dev -> lvlip_lro_advance_dev ->
lvlip_ack_dev -> reverse lvlip_lro_dev -> lvlip_snd_dev -> lvlip_rtx_dev on one
stream of the caller's with a single synchronise, against the CPU forms; a
transfer with loss, run to the end through the device calls; what the
reference's own stack did (tests/golden/snd_ref.json); and the foreign frames
of tests/test_snd_cpu.py (TCP options, bytes behind the segment, a wrapping
pseudo-header sum, the accepted and refused lengths) against the Python model
over the ring's bytes and against the CPU forms.

The record counts leave a wave partly filled, fill it, and spill one record
into the next (63, 64, 65), and end a grid of two workgroups on one lane
(257).  The flow counts do the same to k_snd_fin's four flows per workgroup
and end a large grid on one (4097).  The queue lengths put the end of the
leading run before, on and behind the 64 entries a wave scans per step."""
import functools
import struct

import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import _t
from test_snd_cpu import (CANARY, FOREIGN, GUARD, M32, Case, _rec, check_rtx_foreign, fixture, foreign, foreign_records,
                          golden_resend, golden_ring, golden_snd, head_acks, head_named_check, make_records, model_rtx,
                          model_snd, rtx_inputs)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


@functools.lru_cache(maxsize=None)
def flows_case(nflows: int) -> Case:
    """Queues of 0 .. 4 frames of 8 .. 40 payload bytes per flow."""
    k = np.arange(nflows)
    return Case(nseg=[int(v) for v in (k * 3 + 1) % 5], mss=[int(v) for v in 8 + 8 * (k % 5)], seed=nflows)


def run_snd_dev(c: Case, rec: np.ndarray, dev, fd=None, stream=None) -> np.ndarray:
    """lvlip_snd_dev into canary bytes with a canary behind res; the inputs
    compared afterwards."""
    fd = c.fd if fd is None else fd
    n = c.flows.size
    ins = [_t(a, dev) for a in (c.flows, c.snd, rec, c.ring, fd)]
    res_t = torch.full((32 * n + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    lvlip.snd_dev(ins[0], ins[1], ins[2], ins[3], ins[4], res_t[:32 * n], stream=stream)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    assert (res_t[32 * n:] == CANARY).all(), "written behind res"
    for name, t, a in zip(("f", "s", "rec", "base", "fd"), ins, (c.flows, c.snd, rec, c.ring, fd)):
        assert np.array_equal(t.cpu().numpy(), a.view(np.uint8).reshape(-1)), f"{name} is only read"
    return res_t[:32 * n].cpu().numpy().view(lvlip.SND_RESULT_DTYPE)


def assert_same_res(got, want, what):
    if got.tobytes() != want.tobytes():
        k = int(np.flatnonzero(got != want)[0])
        pytest.fail(f"{what}: flow {k}: got {got[k]}, want {want[k]}; {int((got != want).sum())} flows differ")


# ------------------------------------------------------------ the ACK side --

@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_snd_dev_equals_cpu_by_records(n, dev):
    c = flows_case(33)
    rec = make_records(c, n, seed=n)
    assert_same_res(run_snd_dev(c, rec, dev), lvlip.snd_cpu(c.flows, c.snd, rec, c.ring, c.fd), f"n {n}")


@pytest.mark.parametrize("nflows", (1, 2, 33, 4097))
def test_snd_dev_equals_cpu_by_flows(nflows, dev):
    c = flows_case(nflows)
    rec = make_records(c, 257, seed=nflows)
    want = lvlip.snd_cpu(c.flows, c.snd, rec, c.ring, c.fd)
    assert_same_res(run_snd_dev(c, rec, dev), want, f"nflows {nflows}")
    assert (want["n_new"] > 0).any() and (want["popped"] > 0).any()


def test_snd_dev_every_record_of_one_flow(dev):
    """The wave reduces before its atomics: 257 records of one flow, and the
    same records in another order."""
    c = flows_case(33)
    rec = make_records(c, 257, seed=5, one_flow=6)
    want = lvlip.snd_cpu(c.flows, c.snd, rec, c.ring, c.fd)
    assert int(want[6]["n_new"]) >= 40 and int(want["n_new"].sum()) == int(want[6]["n_new"])
    assert_same_res(run_snd_dev(c, rec, dev), want, "one flow")
    assert_same_res(run_snd_dev(c, rec[np.random.default_rng(0).permutation(257)], dev), want, "one flow, shuffled")


def test_snd_dev_most_flows_without_a_record(dev):
    c = flows_case(4097)
    rec = make_records(c, 257, seed=2, few_flows=True)
    want = lvlip.snd_cpu(c.flows, c.snd, rec, c.ring, c.fd)
    assert int((want["n_new"] + want["n_dup"] + want["n_old"] + want["n_beyond"] > 0).sum()) <= 3
    got = run_snd_dev(c, rec, dev)
    assert_same_res(got, want, "few flows")
    idle = got[3:]
    assert (idle["snd_una"] == c.snd["snd_una"][3:]).all() and (idle["inflight"] == c.snd["nseg"][3:]).all()


@functools.lru_cache(maxsize=None)
def queues_case() -> Case:
    return Case(nseg=[0, 1, 63, 64, 65, 300], mss=[8] * 6, seed=11)


@pytest.mark.parametrize("run", (0, 1, 62, 63, 64, 65, 128, 299, 300))
def test_snd_dev_leading_run(run, dev):
    """Queues of 0, 1, 63, 64, 65 and 300 frames, `run` of them acknowledged
    (and 3 bytes of the next): the scan ends before, on and behind a wave's 64
    entries, in the first step and in later ones."""
    c = queues_case()
    rec = np.concatenate([_rec(k, int(c.snd[k]["snd_una"]) + min(8 * run + 3, c.span(k))) for k in range(6)])
    want = lvlip.snd_cpu(c.flows, c.snd, rec, c.ring, c.fd)
    assert want["popped"].tolist() == [min(run, int(n)) for n in c.snd["nseg"]]
    assert_same_res(run_snd_dev(c, rec, dev), want, f"run {run}")
    if run == 64:  # a frame too short to be one ends the run, wherever it is
        fd = c.fd.copy()
        fd[int(c.snd[5]["seg0"]) + 40]["len"] = 53
        want = lvlip.snd_cpu(c.flows, c.snd, rec, c.ring, fd)
        assert int(want[5]["popped"]) == 40
        assert_same_res(run_snd_dev(c, rec, dev, fd=fd), want, "a short entry")


def test_snd_dev_twice_the_same_on_a_stream(dev):
    c = flows_case(33)
    rec = make_records(c, 257, seed=8)
    s = torch.cuda.Stream(dev)
    a, b = run_snd_dev(c, rec, dev, stream=s), run_snd_dev(c, rec, dev)
    assert a.tobytes() == b.tobytes()


# ----------------------------------------------------------- the retransmit --

def run_rtx_dev(c: Case, lro, sres, dev, ring=None, fd=None):
    """lvlip_rtx_dev on a copy of the ring, canary behind fd_out.  Returns
    (ring, fd_out) on the host."""
    ring = c.ring if ring is None else ring
    fd = c.fd if fd is None else fd
    f_t, s_t, fd_t = _t(c.flows, dev), _t(c.snd, dev), _t(fd, dev)
    ring_t = _t(ring, dev)
    assert ring_t.data_ptr() % 16 == 0
    out_t = torch.full((16 * c.nslots + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    lvlip.rtx_dev(f_t, _t(lro, dev) if lro is not None else None, s_t, _t(sres, dev) if sres is not None else None,
                  c.nslots, ring_t, fd_t, out_t[:16 * c.nslots])
    torch.cuda.synchronize(dev)
    assert (out_t[16 * c.nslots:] == CANARY).all(), "written behind fd_out"
    assert np.array_equal(fd_t.cpu().numpy(), fd.view(np.uint8).reshape(-1)), "fd is only read"
    return ring_t.cpu().numpy(), out_t[:16 * c.nslots].cpu().numpy().view(lvlip.FRAME_DESC_DTYPE)


def assert_same_ring(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        pytest.fail(f"{what}: {bad.size} ring bytes differ, first at {int(bad[0])}: got 0x{int(got[bad[0]]):02x}, "
                    f"want 0x{int(want[bad[0]]):02x}")


@functools.lru_cache(maxsize=None)
def sizes_case() -> Case:
    """17 frames of each payload size, strides of 1 mod 16: every size at
    every frame alignment; the last frame of each queue is shorter."""
    c = Case(nseg=[17] * 6, mss=[1, 2, 3, 536, 1460, 8946], rtx=[17, 18, 17, 17, 17, 17], seed=21)
    for k in range(6):
        q = int(c.snd[k]["seg0"])
        assert sorted(int(o) % 16 for o in c.fd["offset"][q:q + 16]) == list(range(16))
    return c


@pytest.mark.parametrize("with_results", (True, False))
def test_rtx_dev_equals_cpu_every_size_and_alignment(with_results, dev):
    c = sizes_case()
    lro, sres = rtx_inputs(c, 6) if with_results else (None, None)
    if with_results:
        sres["popped"][:3] = (0, 5, 17)  # all live, the tail dead, all dead
    want = c.ring.copy()
    want_fd = lvlip.rtx_cpu(c.flows, lro, c.snd, sres, want, c.fd)
    model, model_fd = model_rtx(c, lro, sres, c.ring)
    assert np.array_equal(want, model) and np.array_equal(want_fd, model_fd)
    got, got_fd = run_rtx_dev(c, lro, sres, dev)
    assert np.array_equal(got_fd, want_fd)
    assert_same_ring(got, want, "sizes")
    assert 0 < int((want_fd["len"] == 0).sum()) < want_fd.size


@pytest.mark.parametrize("nflows", (2, 33, 4097))
def test_rtx_dev_equals_cpu_by_flows(nflows, dev):
    """Slots that end a workgroup of 16 partly filled, flows with rtx 0 in
    front of and behind flows with slots (the search over slot0)."""
    c = flows_case(nflows)
    c = Case(nseg=[int(v) for v in c.snd["nseg"]], mss=[int(v) for v in 8 + 8 * (np.arange(nflows) % 5)],
             rtx=[int(v) for v in (np.arange(nflows) * 7 + 3) % 4 * (np.arange(nflows) % 3 > 0)], seed=nflows)
    lro, sres = rtx_inputs(c, nflows)
    want = c.ring.copy()
    want_fd = lvlip.rtx_cpu(c.flows, lro, c.snd, sres, want, c.fd)
    got, got_fd = run_rtx_dev(c, lro, sres, dev)
    assert np.array_equal(got_fd, want_fd)
    assert_same_ring(got, want, f"nflows {nflows}")


def test_rtx_dev_leaves_frames_it_cannot_rewrite(dev):
    c = Case(nseg=[4], mss=[100], rtx=[4], seed=2)
    ring, fd = c.ring.copy(), c.fd.copy()
    fd[0]["len"] = 53
    ring[int(fd[1]["offset"]) + 14] = 0x46
    ring[int(fd[2]["offset"]) + 17] += 1
    want = ring.copy()
    want_fd = lvlip.rtx_cpu(c.flows, None, c.snd, None, want, fd)
    assert want_fd["len"].tolist() == [0, 0, 0, int(fd[3]["len"])]
    got, got_fd = run_rtx_dev(c, None, None, dev, ring=ring, fd=fd)
    assert np.array_equal(got_fd, want_fd)
    assert_same_ring(got, want, "frames that stay")


# ---------------------------------------------------------- foreign frames --
#
# The queues of test_snd_cpu.foreign (TCP options, bytes behind the segment,
# addresses whose pseudo-header sum wraps, a 0x46 byte 14, zero-length frames,
# the last accepted and first refused lengths; every kind at every residue mod
# 16) through the device forms, against the Python model over the ring's bytes
# AND against the CPU forms.

@pytest.mark.parametrize("name", FOREIGN)
def test_snd_dev_foreign_frames_equal_model_and_cpu(name, dev):
    q = foreign(name)
    rec = foreign_records(q, 3)
    want = model_snd(q.flows, q.snd, rec, q.ring, q.fd)
    got = run_snd_dev(q, rec, dev)
    assert_same_res(got, want, f"{name}: against the model")
    assert_same_res(got, lvlip.snd_cpu(q.flows, q.snd, rec, q.ring, q.fd), f"{name}: against the CPU form")
    assert (want["popped"] > 0).any() and (want["inflight"] > 0).any() and (want["n_new"] > 0).any()


def test_snd_dev_foreign_heads_one_ack_at_a_time(dev):
    """An ACK one byte before, on and one byte behind every end_seq of the
    head queues, each alone in its batch (the inputs uploaded once)."""
    q = foreign("heads")
    n = q.flows.size
    ins = [_t(a, dev) for a in (q.flows, q.snd, q.ring, q.fd)]
    res_t = torch.full((32 * n + GUARD,), CANARY, dtype=torch.uint8, device=dev)
    popped = set()
    for k, a in head_acks(q):
        rec = _rec(k, a)
        lvlip.snd_dev(ins[0], ins[1], _t(rec, dev), ins[2], ins[3], res_t[:32 * n])
        got = res_t.cpu().numpy()
        assert (got[32 * n:] == CANARY).all(), "written behind res"
        got = got[:32 * n].view(lvlip.SND_RESULT_DTYPE)
        assert_same_res(got, model_snd(q.flows, q.snd, rec, q.ring, q.fd), f"flow {k}, ack {a:#x}: against the model")
        assert_same_res(got, lvlip.snd_cpu(q.flows, q.snd, rec, q.ring, q.fd), f"flow {k}, ack {a:#x}: against the CPU form")
        popped.add(int(got[k]["popped"]))
    assert popped == {0, 1, 2, 3, 4}


def test_snd_dev_foreign_heads_named(dev):
    head_named_check(lambda q, rec: run_snd_dev(q, rec, dev))


@pytest.mark.parametrize("with_results", (False, True))
@pytest.mark.parametrize("name", FOREIGN)
def test_rtx_dev_foreign_frames_equal_model_and_cpu(name, with_results, dev):
    def run(q, lro, sres, ring):
        cpu = ring.copy()
        cpu_fd = lvlip.rtx_cpu(q.flows, lro, q.snd, sres, cpu, q.fd)
        got, got_fd = run_rtx_dev(q, lro, sres, dev, ring=ring)
        assert np.array_equal(got_fd, cpu_fd), f"{name}: fd_out against the CPU form"
        assert_same_ring(got, cpu, f"{name}: against the CPU form")
        ring[:] = got
        return got_fd

    check_rtx_foreign(name, with_results, run)


# ---------------------------------------------------------------- the chain --

MSS = 536
IRS = 0x01020304
ETH_AB = bytes.fromhex("000c296d50250a1b2c3d4e5f0800")
ETH_BA = bytes.fromhex("0a1b2c3d4e5f000c296d50250800")
A, B = bytes((10, 0, 0, 4)), bytes((10, 0, 0, 5))


def _hdr(eth, src, dst, sport, dport, seq, ack, flags):
    ip = struct.pack("!BBHHHBBH4s4s", 0x45, 0, 0, 0x1234, 0x4000, 64, 6, 0, src, dst)
    return eth + ip + struct.pack("!HHIIBBHHH", sport, dport, seq & M32, ack & M32, 0x50, flags, 0x7210, 0, 0)


class Link:
    """Side A sends nflows x segs frames of MSS bytes from a TX ring; side B
    coalesces, advances over all records so far and acknowledges; A parses the
    ACKs through the reverse plan, runs the ACK side and re-sends `rtx` frames
    from the head of every queue.  One round of all that on the device
    (round_dev: one stream, no host step) or on the CPU forms (round_cpu)."""

    def __init__(self, nflows: int, segs: int, rtx: int, dev=None):
        self.nflows, self.segs, self.dev = nflows, segs, dev
        length = segs * MSS
        self.iss = [(0xFFFFF000 + 0x01000193 * k) & M32 for k in range(nflows)]
        self.fb = np.concatenate([lvlip.lro_flow(A, B, 40000 + k, 8000, self.iss[k], length, out_off=k * length, user=k)
                                  for k in range(nflows)])
        self.fa = np.concatenate([lvlip.lro_flow(B, A, 8000, 40000 + k, IRS, 1, out_off=k, user=k)
                                  for k in range(nflows)])
        lvlip.lro_plan(self.fb)
        lvlip.lro_plan(self.fa)
        assert self.fa["user"].tolist() == list(range(nflows)) == self.fb["user"].tolist()
        stride = 54 + MSS + 3
        self.sends = np.concatenate([lvlip.tso_send(_hdr(ETH_AB, A, B, 40000 + k, 8000, self.iss[k], IRS, 0x18),
                                                    k * length, length, MSS, out_off=5 + k * segs * stride, stride=stride)
                                     for k in range(nflows)])
        self.payload = np.random.default_rng(nflows).integers(0, 256, nflows * length, dtype=np.uint8)
        self.ring, self.fd = lvlip.tso_cpu(self.payload, self.sends)
        self.ring = np.concatenate([self.ring, np.zeros(GUARD, dtype=np.uint8)])
        self.tmpl = np.concatenate([lvlip.ack_tmpl(_hdr(ETH_BA, B, A, 8000, 40000 + k, IRS, 0, 0x10), out_off=3 + 91 * k)
                                    for k in range(nflows)])
        self.ack_bytes = lvlip.ack_plan(self.tmpl, self.fb) + GUARD
        self.snd = np.zeros(nflows, dtype=lvlip.SND_FLOW_DTYPE)
        self.snd["snd_una"], self.snd["seg0"], self.snd["nseg"] = self.iss, self.sends["seg0"], segs
        self.snd["snd_nxt"] = (self.snd["snd_una"].astype(np.uint64) + length) & M32
        self.snd["rtx"], self.snd["win"] = rtx, 28200  # not the window the frames were built with
        self.nslots, _ = lvlip.snd_plan(self.snd)
        self.stream = np.full(nflows * length, CANARY, dtype=np.uint8)
        self.rec = np.zeros(0, dtype=lvlip.LRO_REC_DTYPE)
        self.cap = nflows * segs * 8  # records B may ever hold
        if dev is not None:
            self.t = {k: _t(getattr(self, k), dev) for k in ("fb", "fa", "ring", "fd", "tmpl", "stream")}
            self.t["rec"] = torch.zeros(16 * self.cap, dtype=torch.uint8, device=dev)
            self.t["res"] = torch.zeros(48 * nflows, dtype=torch.uint8, device=dev)
            self.t["ws"] = torch.empty(lvlip.lro_advance_workspace_bytes(self.cap, nflows), dtype=torch.uint8, device=dev)
            self.t["ack"] = torch.full((self.ack_bytes,), CANARY, dtype=torch.uint8, device=dev)
            self.t["afd"] = torch.zeros(16 * nflows, dtype=torch.uint8, device=dev)
            self.t["arec"] = torch.zeros(16 * nflows, dtype=torch.uint8, device=dev)
            self.t["sink"] = torch.zeros(nflows + GUARD, dtype=torch.uint8, device=dev)
            self.t["sres"] = torch.zeros(32 * nflows, dtype=torch.uint8, device=dev)
            self.t["fd_out"] = torch.zeros(16 * self.nslots, dtype=torch.uint8, device=dev)
            self.nrec = 0

    def round_cpu(self, wire: np.ndarray) -> dict:
        _, rec = lvlip.lro_cpu(self.ring, wire, self.fb, lvlip.RX_VERIFY_L4, out=self.stream)
        self.rec = np.concatenate([self.rec, rec])
        res = lvlip.lro_advance(self.fb, self.rec)
        ack, afd = lvlip.ack_cpu(self.tmpl, self.fb, res, lvlip.ACK_ALL, out=np.full(self.ack_bytes, CANARY, dtype=np.uint8))
        _, arec = lvlip.lro_cpu(ack, afd, self.fa, lvlip.RX_VERIFY_L4, out=np.zeros(self.nflows + GUARD, dtype=np.uint8))
        sres = lvlip.snd_cpu(self.fa, self.snd, arec, self.ring, self.fd)
        fd_out = lvlip.rtx_cpu(self.fa, None, self.snd, sres, self.ring, self.fd)
        return dict(rec=self.rec.copy(), res=res, ack=ack, afd=afd, arec=arec, sres=sres, fd_out=fd_out,
                    ring=self.ring.copy(), stream=self.stream.copy())

    def round_dev(self, wire: np.ndarray, stream) -> dict:
        """The six calls on `stream`, one synchronise at the end."""
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
        lvlip.rtx_dev(t["fa"], None, snd_t, t["sres"], self.nslots, t["ring"], t["fd"], t["fd_out"], stream=stream)
        stream.synchronize()
        h = lambda k, dt=np.uint8: t[k].cpu().numpy().view(dt)  # noqa: E731
        return dict(rec=h("rec", lvlip.LRO_REC_DTYPE)[:self.nrec], res=h("res", lvlip.LRO_RESULT_DTYPE), ack=h("ack"),
                    afd=h("afd", lvlip.FRAME_DESC_DTYPE), arec=h("arec", lvlip.LRO_REC_DTYPE),
                    sres=h("sres", lvlip.SND_RESULT_DTYPE), fd_out=h("fd_out", lvlip.FRAME_DESC_DTYPE), ring=h("ring"),
                    stream=h("stream"))

    def carry_on(self, sres: np.ndarray) -> None:
        self.snd["snd_una"] = sres["snd_una"]
        self.snd["seg0"] += sres["popped"]
        self.snd["nseg"] -= sres["popped"]

    def first_flight(self, rng) -> np.ndarray:
        keep = np.arange(self.fd.size) % 5 != 4  # every fifth frame lost
        return self.fd[keep][rng.permutation(int(keep.sum()))]


def test_the_chain_on_one_stream(dev):
    """Two rounds of the whole loop: the device's six calls on one stream of
    the caller's, one synchronise per round, against the CPU forms: records,
    results, ACK frames, the reverse records, the ACK side's results, the ring
    after the retransmit and fd_out, byte for byte."""
    host, gpu = Link(3, 12, 3), Link(3, 12, 3, dev)
    s = torch.cuda.Stream(dev)
    rng = np.random.default_rng(4)
    wire = host.first_flight(rng)
    for rnd in range(2):
        want, got = host.round_cpu(wire), gpu.round_dev(wire, s)
        for k in ("rec", "res", "afd", "arec", "sres", "fd_out", "ack", "ring", "stream"):
            assert got[k].tobytes() == want[k].tobytes(), f"round {rnd}: {k}"
        assert (want["sres"]["popped"] > 0).any() and (want["fd_out"]["len"] > 0).all()
        assert not np.array_equal(want["ring"][:-GUARD], lvlip.tso_cpu(host.payload, host.sends)[0]), "nothing re-sent"
        host.carry_on(want["sres"])
        gpu.carry_on(got["sres"])
        wire = want["fd_out"][1:]  # the first re-sent frame is lost again


def test_a_transfer_with_loss_ends_on_the_device(dev):
    """8 flows x 40 segments of 536 B, every fifth frame lost in every flight:
    the loop runs through the device calls until every stream byte is
    delivered and nothing is in flight."""
    link = Link(8, 40, 8, dev)
    s = torch.cuda.Stream(dev)
    rng = np.random.default_rng(7)
    wire = link.first_flight(rng)
    for rnd in range(30):
        got = link.round_dev(wire, s)
        link.carry_on(got["sres"])
        assert (got["sres"]["n_old"] == 0).all() and (got["sres"]["n_beyond"] == 0).all()
        if not link.snd["nseg"].any():
            break
        live = got["fd_out"][got["fd_out"]["len"] > 0]
        live = live[np.arange(live.size) % 5 != 4] if live.size > 1 else live
        wire = live[rng.permutation(live.size)]
    assert (got["sres"]["inflight"] == 0).all() and not link.snd["nseg"].any(), f"not done after {rnd + 1} rounds"
    assert (got["res"]["delivered"] == 40 * MSS).all()
    assert np.array_equal(got["stream"], link.payload), "the streams are not the payloads"
    assert (link.snd["snd_una"] == link.snd["snd_nxt"]).all() and rnd >= 2


# ---------------------------------------------------------------- the golden --

def test_snd_dev_reproduces_the_reference_queue(dev):
    """Every ACK the reference's stack was fed, from the state it was in: the
    snd_una and queue length the stack was left with (tests/golden/snd_ref.json)."""
    fx = fixture()
    flow, ring, fd = golden_ring(fx)
    ins = [_t(a, dev) for a in (flow, ring, fd)]
    for c in fx["cases"]:
        res_t = lvlip.snd_dev(ins[0], _t(golden_snd(c["before"]), dev), _t(_rec(0, c["ack_seq"]), dev), ins[1], ins[2])
        torch.cuda.synchronize(dev)
        r = res_t.cpu().numpy().view(lvlip.SND_RESULT_DTYPE)[0]
        assert (int(r["snd_una"]), int(r["inflight"])) == (c["after"]["snd_una"], c["after"]["queue"]), (c["stage"], c["name"])


def test_rtx_dev_reproduces_the_reference_resend(dev):
    """The frame the reference's retransmission timer sent, byte for byte, and
    no other byte of the ring changed."""
    flow, lro, snd, ring, fd, o, want = golden_resend(fixture())
    ring_t = _t(ring, dev)
    out_t = lvlip.rtx_dev(_t(flow, dev), _t(lro, dev), _t(snd, dev), None, 1, ring_t, _t(fd, dev))
    torch.cuda.synchronize(dev)
    got = ring_t.cpu().numpy()
    assert got[o:o + len(want)].tobytes().hex() == want.hex()
    d = out_t.cpu().numpy().view(lvlip.FRAME_DESC_DTYPE)[0]
    assert (int(d["offset"]), int(d["len"])) == (o, len(want))
    changed = np.flatnonzero(got != ring)
    assert changed.size and set(int(v) for v in changed - o) <= set(range(42, 46)) | set(range(48, 52))
