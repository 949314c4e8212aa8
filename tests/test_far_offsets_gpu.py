"""Offsets at and beyond 2^32 through every device call that takes one:
lvlip_frame_desc.offset, lvlip_tso_send.payload_off / out_off,
lvlip_lro_flow.out_off, lvlip_ack_tmpl.out_off and the checksum descriptor's
offset are uint64_t, the kernels rebuild them from two dwords and add chunk
indices to them, and no other device test passes 3 GiB.

One allocation of 4096 + 2^32 + 2 MiB bytes is only address space.  `base`
starts 4096 bytes in; three zones are ever filled, used and read back: the
4096-byte fore-guard, base[0, 1 MiB) and base[2^32 - 1 MiB, 2^32 + 1 MiB).

Placement.  High objects start at 2^32 + x (x from 16 KiB up, below 512 KiB)
or within 2048 bytes below 2^32, so that they straddle it; low objects lie in
[512 KiB, 1 MiB).  Every 32-bit alias of every offset used then lands in a
checked zone that holds canary bytes: truncation to u32 and a 32-bit add that
wraps land in base[0, 512 KiB), which no object ever occupies, and the sign
extension of a straddler's low dword lands in the fore-guard.  A dropped high
dword, an int chunk offset or a wrapping add therefore shows up as a wrong
byte (a store into canary, or canary read as data), never as a fault.  Each
call mixes low and high objects, so the high dword differs from one descriptor
to the next.

Expected bytes come from the CPU form of the same call on a 3 MiB host ring:
the low zone maps to [0, 1 MiB) and the high zone to [1 MiB, 3 MiB), a shift
by 2^32 - 2 MiB, a multiple of 16, so every alignment is the device's.
Offsets in fd, fd_out and the descriptors are mapped back before comparing;
all three zones are compared whole, so a wrong write shows as well as a
missing one."""
import numpy as np
import pytest
import torch

import devbuf
import lvlip
import pyoracle
import workloads
from devbuf import CANARY, _t, guarded, unguard
from test_ack_cpu import make_flows, make_tmpl, random_res
from test_lro_cpu import ME, PEER, tcp_frame
from test_skb_cpu import _rx_cases
from test_skb_gpu import _echo_requests
from test_snd_cpu import Case, make_records, rtx_inputs
from test_tso_cpu import template as tso_template

pytestmark = pytest.mark.gpu

MiB, TOP, FORE = 1 << 20, 1 << 32, 4096
SHIFT = TOP - 2 * MiB         # host offset + SHIFT = device offset, for the high zone
LOW0 = MiB // 2               # low objects from here; [0, LOW0) is where the 32-bit aliases land
HIGH0 = 2 * MiB + (16 << 10)  # host offset of 2^32 + 16 KiB: the first high object that does not straddle
HIGH1 = 2 * MiB + LOW0
SIZES = (1, 2, 3, 536, 1460)


def far(o):
    """Host ring offset(s) -> device offset(s)."""
    o = np.asarray(o, dtype=np.uint64)
    return np.where(o < MiB, o, o + np.uint64(SHIFT))


def near(o):
    o = np.asarray(o, dtype=np.uint64)
    return np.where(o < MiB, o, o - np.uint64(SHIFT))


class Lay:
    """Hands out host offsets: low(), high() (successive objects one residue
    mod 16 further, a canary gap between them) and one straddle(size, before)
    that starts `before` bytes below 2^32."""

    def __init__(self):
        self.lo, self.hi, self.n, self.straddler = LOW0 + 16, HIGH0, 0, None

    def _next(self, cur, size):
        self.n += 1
        o = cur + 1 + ((3 * self.n - cur - 1) % 16)
        return o, o + size

    def low(self, size):
        o, self.lo = self._next(self.lo, size)
        assert self.lo <= MiB - 64
        return o

    def high(self, size):
        o, self.hi = self._next(self.hi, size)
        assert self.hi <= HIGH1
        return o

    def straddle(self, size, before):
        assert self.straddler is None and 0 < before <= 2048 and before < size <= before + (16 << 10) - 64
        self.straddler = 2 * MiB - before
        return self.straddler

    def put(self, where, size, before=None):
        return self.straddle(size, before) if where == "x" else self.low(size) if where == "l" else self.high(size)


def assert_mixed(dev_off, dev_len=None):
    """Low and high offsets both occur; with lengths, one object crosses 2^32."""
    o = np.asarray(dev_off, dtype=np.uint64)
    assert (o < MiB).any() and (o >= TOP).any()
    if dev_len is not None:
        assert ((o < TOP) & (o + np.asarray(dev_len, dtype=np.uint64) > TOP)).any()


class Far:
    def __init__(self, dev):
        free, _ = torch.cuda.mem_get_info(dev)
        assert free > 6e9, f"needs ~4.3 GB of HBM, {free / 1e9:.1f} GB free"
        self.dev = dev
        self.big = torch.empty(FORE + TOP + 2 * MiB, dtype=torch.uint8, device=dev)
        self.base = self.big[FORE:]
        assert self.base.data_ptr() % 16 == 0 and self.base.is_contiguous()

    def load(self, ring: np.ndarray) -> None:
        assert ring.size == 3 * MiB and (ring[:LOW0] == CANARY).all()
        self.big[:FORE] = CANARY
        self.base[:MiB].copy_(torch.from_numpy(ring[:MiB].copy()))
        self.base[TOP - MiB:TOP + MiB].copy_(torch.from_numpy(ring[MiB:].copy()))
        torch.cuda.synchronize(self.dev)

    def check(self, want: np.ndarray, what: str) -> None:
        torch.cuda.synchronize(self.dev)
        fore = self.big[:FORE].cpu().numpy()
        got = np.concatenate([self.base[:MiB].cpu().numpy(), self.base[TOP - MiB:TOP + MiB].cpu().numpy()])
        assert (fore == CANARY).all(), f"{what}: written in front of base, at {int(np.flatnonzero(fore != CANARY)[0]) - FORE}"
        assert (want[:LOW0] == CANARY).all()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            b = int(bad[0])
            pytest.fail(f"{what}: {bad.size} bytes differ, first at device offset {int(far(b)):#x}: got 0x{int(got[b]):02x}, "
                        f"want 0x{int(want[b]):02x}")


@pytest.fixture(scope="module")
def zone():
    z = Far(devbuf.device())
    yield z
    z.base = z.big = None
    torch.cuda.empty_cache()


def blank() -> np.ndarray:
    return np.full(3 * MiB, CANARY, dtype=np.uint8)


def fd_far(fd: np.ndarray) -> np.ndarray:
    d = fd.copy()
    d["offset"] = far(fd["offset"])
    return d


def fd_near(fd: np.ndarray) -> np.ndarray:
    d = fd.copy()
    d["offset"] = near(fd["offset"])
    return d


# ---------------------------------------------------------------- lvlip_tso --

def test_tso_dev(zone):
    """payload_off and out_off low and high, sizes 1, 2, 3, 536 and 1460; the
    last send starts 700 bytes below 2^32 and its second frame crosses it."""
    rng = np.random.default_rng(1)
    lay, ring0, sends = Lay(), blank(), []
    hdr = tso_template()
    plan =[(1, 1, "l", "h"), (5, 2, "h", "l"), (3, 3, "l", "h"), (1100, 536, "h", "l"), (2921, 1460, "l", "h"),
            (1460, 1460, "h", "h"), (3 * 536, 536, "h", "x")]
    for length, mss, pw, ow in plan:
        nseg = -(-length // mss)
        stride = 54 + mss + 3
        po = lay.put(pw, length)
        oo = lay.put(ow, nseg * stride, before=700)
        ring0[po:po + length] = rng.integers(0, 256, length, dtype=np.uint8)
        sends.append(lvlip.tso_send(hdr, po, length, mss, out_off=oo, stride=stride))
    sends = np.concatenate(sends)
    want, want_fd = lvlip.tso_cpu(ring0.copy(), sends, out=ring0.copy())
    far_sends = sends.copy()
    far_sends["payload_off"], far_sends["out_off"] = far(sends["payload_off"]), far(sends["out_off"])
    nseg, out_bytes = lvlip.tso_plan(far_sends)
    assert nseg == want_fd.size and out_bytes > TOP and np.array_equal(far_sends["seg0"], sends["seg0"])
    assert_mixed(far_sends["payload_off"])
    assert_mixed(far(want_fd["offset"]), want_fd["len"])
    assert set(SIZES) <= {int(v) - 54 for v in want_fd["len"]}
    zone.load(ring0)
    fd_t = guarded(16 * nseg, zone.dev)
    lvlip.tso_dev(zone.base, _t(far_sends, zone.dev), nseg, zone.base, fd_t)
    zone.check(want, "lvlip_tso_dev")
    got_fd = unguard(fd_t, 16 * nseg, lvlip.FRAME_DESC_DTYPE)
    assert np.array_equal(got_fd, fd_far(want_fd))
    assert not np.array_equal(want, ring0)


# ---------------------------------------------------------------- lvlip_lro --

@pytest.mark.parametrize("straddler", ("frame", "payload"))
def test_lro_dev(straddler, zone):
    """fd.offset low, high and (frame) straddling 2^32; the flows' out_off low
    and high and (payload) 700 bytes below 2^32, so that a 1460-byte payload
    lands across it."""
    rng = np.random.default_rng(2)
    lay, ring0 = Lay(), blank()
    wnd = 4096
    outs = [lay.low(wnd), lay.high(wnd), lay.put("x" if straddler == "payload" else "h", wnd, before=700)]
    flows = np.concatenate([lvlip.lro_flow(PEER, ME, 40001 + k, 8000, 0xFFFFFF00, wnd, out_off=o, user=k)
                            for k, o in enumerate(outs)])
    lvlip.lro_plan(flows)
    frames, rel = [], [0, 0, 0]
    for i, n in enumerate((1460, 1, 2, 3, 536, 1460, 536, 1, 2, 3, 536, 1460)):
        k = int(flows[i % 3]["user"])
        frames.append((i % 3, tcp_frame(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), 0xFFFFFF00 + rel[i % 3],
                                        sport=40001 + k)))
        rel[i % 3] += n
    fd = np.zeros(len(frames), dtype=lvlip.FRAME_DESC_DTYPE)
    for i, (_, fr) in enumerate(frames):
        where = "x" if straddler == "frame" and i == 5 else "lh"[i % 2]
        o = lay.put(where, len(fr), before=300)
        ring0[o:o + len(fr)] = np.frombuffer(fr, dtype=np.uint8)
        fd[i]["offset"], fd[i]["len"] = o, len(fr)
    want, want_rec = lvlip.lro_cpu(ring0.copy(), fd, flows, lvlip.RX_VERIFY_L4, out=ring0.copy())
    assert (want_rec["status"] == lvlip.LRO_PLACED).all() and not np.array_equal(want, ring0)
    far_flows = flows.copy()
    far_flows["out_off"] = far(flows["out_off"])
    assert_mixed(far(fd["offset"]), fd["len"] if straddler == "frame" else None)
    assert_mixed(far_flows["out_off"])
    if straddler == "payload":
        k = int(np.flatnonzero(far_flows["out_off"] == TOP - 700)[0])
        assert any(int(r["flow"]) == k and int(r["rel"]) < 700 < int(r["rel"]) + int(r["dlen"]) for r in want_rec)
    zone.load(ring0)
    rec_t = guarded(16 * fd.size, zone.dev)
    lvlip.lro_dev(zone.base, _t(fd_far(fd), zone.dev), _t(far_flows, zone.dev), lvlip.RX_VERIFY_L4, zone.base, rec_t)
    zone.check(want, "lvlip_lro_dev")
    assert unguard(rec_t, 16 * fd.size, lvlip.LRO_REC_DTYPE).tobytes() == want_rec.tobytes()


# ---------------------------------------------------------------- lvlip_ack --

def test_ack_dev(zone):
    """Template out_off low and high; one ACK frame starts 30 bytes below 2^32."""
    n = 12
    flows = make_flows(n)
    res = random_res(n, 5)
    tmpl = make_tmpl(flows, 4)
    lay = Lay()
    tmpl["out_off"] = [lay.put("x" if k == 7 else "lh"[k % 2], lvlip.ACK_MAX_FRAME, before=30) for k in range(n)]
    ring0 = blank()
    want, want_fd = lvlip.ack_cpu(tmpl, flows, res, lvlip.ACK_ALL, out=ring0.copy())
    assert (want_fd["len"] >= 54).all() and int(want_fd[7]["len"]) > 30
    far_tmpl = tmpl.copy()
    far_tmpl["out_off"] = far(tmpl["out_off"])
    assert lvlip.ack_plan(far_tmpl, flows) > TOP
    assert_mixed(far(want_fd["offset"]), want_fd["len"])
    zone.load(ring0)
    fd_t = guarded(16 * n, zone.dev)
    lvlip.ack_dev(_t(far_tmpl, zone.dev), _t(flows, zone.dev), _t(res, zone.dev), lvlip.ACK_ALL, zone.base, fd_t)
    zone.check(want, "lvlip_ack_dev")
    assert np.array_equal(unguard(fd_t, 16 * n, lvlip.FRAME_DESC_DTYPE), fd_far(want_fd))


# ------------------------------------------------------ lvlip_snd, lvlip_rtx --

def far_queue(before: int):
    """(case, ring, fd): five queues of three frames of 1, 2, 3, 536 and 1460
    payload bytes (cut by lvlip_tso_cpu), moved frame by frame to low and high
    offsets of a host ring; the 1460-byte head of the last queue starts
    `before` bytes below 2^32."""
    c = Case(nseg=[3] * 5, mss=list(SIZES), rtx=[3] * 5, seed=41)
    lay, ring, fd = Lay(), blank(), c.fd.copy()
    head = int(c.snd[4]["seg0"])
    for i, d in enumerate(c.fd):
        o, n = int(d["offset"]), int(d["len"])
        at = lay.put("x" if i == head else "lh"[i % 2], n, before=before)
        ring[at:at + n] = c.ring[o:o + n]
        fd[i]["offset"] = at
    assert int(fd[head]["len"]) == 1514
    assert_mixed(far(fd["offset"]), fd["len"])
    return c, ring, fd


def test_snd_dev(zone):
    """Queue frames low and high; the 54 header bytes of one cross 2^32 (it
    starts 30 bytes below): ip.len below, seq and hl above."""
    c, ring, fd = far_queue(30)
    rec = np.concatenate([make_records(c, 65, 6, few_flows=True)] + [  # flow 3: one frame and a bit; flow 4: all
        np.array([(k, 0, 0, lvlip.LRO_NO_DATA, 0x10, (int(c.snd[k]["snd_una"]) + d) & 0xFFFFFFFF)],
                 dtype=lvlip.LRO_REC_DTYPE) for k, d in ((3, 546), (4, c.span(4)))])
    want = lvlip.snd_cpu(c.flows, c.snd, rec, ring, fd)
    assert (int(want[3]["popped"]), int(want[3]["inflight"]), int(want[4]["popped"])) == (1, 2, 3)
    zone.load(ring)
    res_t = guarded(32 * 5, zone.dev)
    lvlip.snd_dev(_t(c.flows, zone.dev), _t(c.snd, zone.dev), _t(rec, zone.dev), zone.base, _t(fd_far(fd), zone.dev),
                  res_t[:32 * 5])
    zone.check(ring, "lvlip_snd_dev")
    assert unguard(res_t, 32 * 5, lvlip.SND_RESULT_DTYPE).tobytes() == want.tobytes()


@pytest.mark.parametrize("before", (20, 46, 300), ids=("header_chunks", "stored_bytes", "sweep"))
def test_rtx_dev(before, zone):
    """The same queue; the straddling frame starts 20 bytes below 2^32 (its
    header chunks cross), 46 below (the ten stored bytes 42..51 cross: 42..45
    below, 46..51 above) and 300 below (the sweep over the payload crosses)."""
    c, ring, fd = far_queue(before)
    lro, sres = rtx_inputs(c, 3)
    sres["popped"] = (0, 1, 3, 2, 0)
    want = ring.copy()
    want_fd = lvlip.rtx_cpu(c.flows, lro, c.snd, sres, want, fd)
    live = want_fd["len"] > 0
    assert 0 < int(live.sum()) < live.size and int(want_fd[int(c.snd[4]["slot0"])]["offset"]) == 2 * MiB - before
    assert_mixed(far(want_fd[live]["offset"]), want_fd[live]["len"])
    changed = np.flatnonzero(want != ring)
    assert changed.size and (changed >= 2 * MiB).any() and (changed < MiB).any()
    at = changed - (2 * MiB - before)  # within the straddling frame: only the ten stored bytes, on both sides of 2^32
    at = {int(v) for v in at if 0 <= v < 1514}
    assert at and at <= set(range(42, 46)) | set(range(48, 52))
    if before == 46:
        assert at & set(range(42, 46)) and at & set(range(48, 52))
    zone.load(ring)
    out_t = guarded(16 * c.nslots, zone.dev)
    lvlip.rtx_dev(_t(c.flows, zone.dev), _t(lro, zone.dev), _t(c.snd, zone.dev), _t(sres, zone.dev), c.nslots, zone.base,
                  _t(fd_far(fd), zone.dev), out_t[:16 * c.nslots])
    zone.check(want, "lvlip_rtx_dev")
    assert np.array_equal(fd_near(unguard(out_t, 16 * c.nslots, lvlip.FRAME_DESC_DTYPE)), want_fd)


# ------------------------------------------------------------ the frame calls --

def place_frames(frames, before: int):
    """(ring, fd): the frames low, high and, the longest, `before` bytes below 2^32."""
    lay, ring = Lay(), blank()
    fd = np.zeros(len(frames), dtype=lvlip.FRAME_DESC_DTYPE)
    big = max(range(len(frames)), key=lambda i: len(frames[i]))
    assert len(frames[big]) > before
    for i, f in enumerate(frames):
        o = lay.put("x" if i == big else "lh"[i % 2], len(f), before=before)
        ring[o:o + len(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
        fd[i]["offset"], fd[i]["len"] = o, len(f)
    assert_mixed(far(fd["offset"]), fd["len"])
    return ring, fd


def filled(ring: np.ndarray, fd: np.ndarray, frames) -> np.ndarray:
    want = ring.copy()
    for d, f in zip(fd, frames):
        want[int(d["offset"]):int(d["offset"]) + int(d["len"])] = np.frombuffer(bytes(f), dtype=np.uint8)
    return want


@pytest.mark.parametrize("flags", (0, lvlip.RX_VERIFY_L4))
def test_rx_verify_dev(flags, zone):
    frames = _rx_cases(61)[:24]
    ring, fd = place_frames(frames, 100)
    want = lvlip.rx_verify_cpu([bytearray(f) for f in frames], flags)
    assert (want == lvlip.RX_OK).any() and (want != lvlip.RX_OK).any()
    zone.load(ring)
    got = lvlip.rx_verify_dev(zone.base, _t(fd_far(fd), zone.dev), flags)
    zone.check(ring, "lvlip_rx_verify_dev")
    assert got.cpu().numpy().tolist() == want.tolist()


def test_tx_checksum_dev(zone):
    frames = workloads.frames(12, seed=62, max_l4=1460) + workloads.frames(2, seed=63, max_l4=8900)
    ring, fd = place_frames(frames, 40)
    done = [bytearray(f) for f in frames]
    lvlip.tx_checksum_cpu(done)
    want = filled(ring, fd, done)
    assert not np.array_equal(want, ring)
    zone.load(ring)
    st = lvlip.tx_checksum_dev(zone.base, _t(fd_far(fd), zone.dev))
    zone.check(want, "lvlip_tx_checksum_dev")
    assert st.cpu().numpy().tolist() == [1] * len(frames)


@pytest.mark.parametrize("flags", (0, lvlip.ECHO_FULL))
def test_icmp_echo_reply_dev(flags, zone):
    frames, _ = _echo_requests(np.random.default_rng(64), 12)
    ring, fd = place_frames(frames, 36)
    done = [bytearray(f) for f in frames]
    lvlip.icmp_echo_reply_fill(done)
    want = filled(ring, fd, done)
    assert not np.array_equal(want, ring)
    zone.load(ring)
    st = lvlip.icmp_echo_reply_dev(zone.base, _t(fd_far(fd), zone.dev), flags=flags)
    zone.check(want, "lvlip_icmp_echo_reply_dev")
    assert set(st.cpu().numpy().tolist()) <= {1, 2}


# ------------------------------------------------------------ the checksum batch --

VARIANTS = [(lvlip.KERNEL_AUTO, 0, 0), (lvlip.KERNEL_WAVE, 2, 0), (lvlip.KERNEL_FLAT, 0, 0),
            (lvlip.KERNEL_FLAT, 4 | (2 << 8), 0), (lvlip.KERNEL_WINDOW, 2 | (3 << 8), 0),
            (lvlip.KERNEL_WINDOW, 3 | (1 << 8), 1), (lvlip.KERNEL_WFLAT, 0, 0),
            (lvlip.KERNEL_LANE, 0, 0), (lvlip.KERNEL_LANE, 2 | (4 << 8) | (1 << 16), 0)]  # test_max_int_packet's


@pytest.mark.parametrize("length,before", ((20, 7), (1500, 700), (9000, 2047)))
def test_csum_batch_dev(length, before, zone):
    """Packets of 20, 1500 and 9000 bytes low and high, and one of `length`
    that starts `before` bytes below 2^32, through every kernel variant,
    against the oracle on the host ring."""
    rng = np.random.default_rng(length)
    lay, ring = Lay(), blank()
    off, lens = [], []
    for i, n in enumerate((20, 1500, 9000, 20, 1500, 9000, length)):
        o = lay.put("x" if i == 6 else "lh"[i % 2], n, before=before)  # each length low and high
        ring[o:o + n] = rng.integers(0, 256, n, dtype=np.uint8)
        off.append(o)
        lens.append(n)
    d = np.zeros(len(off), dtype=lvlip.DESC_DTYPE)
    d["offset"], d["len"], d["start_sum"] = off, lens, rng.integers(0, 1 << 32, len(off), dtype=np.uint64)
    want = pyoracle.batch(ring, d)
    far_d = d.copy()
    far_d["offset"] = far(d["offset"])
    assert_mixed(far_d["offset"], far_d["len"])
    zone.load(ring)
    descs = _t(far_d, zone.dev)
    for k, u, w in VARIANTS:
        out = lvlip.batch_torch(zone.base, descs, None, kernel=k, unroll=u, waves_per_cu=w)
        torch.cuda.synchronize(zone.dev)
        assert out.cpu().numpy().view(np.uint16).tolist() == want.tolist(), (k, u, w)
    zone.check(ring, "lvlip_csum_batch_dev")
