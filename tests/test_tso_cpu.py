"""TCP segmentation from a header template (include/lvlip_skb.h, lvlip_tso_*)
without a GPU: the plan, the CPU form against the reference's own tcp_send
frames (tests/golden/tso_ref.json, written by tests/golden/make_tso_golden.py
from the unmodified stack) and against an independent builder over the shape
list, the refusals, and a sanitizer build of examples/tso_frames.c.

The builder (build_expected) assembles frames with numpy and struct from the
semantics in the header; its checksums come from the oracle (pyoracle.checksum,
and the reference's tcp_udp_checksum where oracle/_ref/libref.so is present),
never from the product.  tests/test_tso_gpu.py shares it, with the cases."""
import ctypes
import functools
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import lvlip
import pyoracle
from tcp_model import _bswap16, lost_carry_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tso_ref.json")
CANARY = 0xA5
HDR = 54

MSS_LIST = (1, 2, 15, 16, 17, 536, 1460, 8946)
PAYLOAD_OFFS = (0, 1, 7, 15)
OUT_MODS = (0, 1, 6, 10, 15)
GAPS = (0, 13)


# ------------------------------------------------------------ the builder --

def template(saddr=(10, 0, 0, 4), daddr=(10, 0, 0, 5), sport=40001, dport=8000, seq=0xFFFFFF00,
             ack=0x01020304, flags=0x18, win=0xADBD, urp=0, ident=0, ttl=64, tos=0) -> bytes:
    """A 54-byte header template: what the first segment would carry.  The IP
    length and both checksum fields hold junk (the calls ignore them)."""
    eth = bytes.fromhex("0a1b2c3d4e5f000c296d5025") + b"\x08\x00"
    ip = struct.pack("!BBHHHBBH4s4s", 0x45, tos, 0xDEAD, ident, 0x4000, ttl, 6, 0xBEEF, bytes(saddr),
                     bytes(daddr))
    tcp = struct.pack("!HHIIBBHHH", sport, dport, seq, ack, 0x50, flags, win, 0xCAFE, urp)
    return eth + ip + tcp


def seed_of(hdr: bytes, l4: int) -> int:
    """src/tcp.c:92-95 on the template's network-order address words: u32
    adds, the carry out of bit 31 lost."""
    return lost_carry_seed(hdr[26:30], hdr[30:34], l4)


def build_frame(hdr: bytes, data: bytes, seq_add: int, last: bool) -> bytes:
    """One segment's frame from the semantics alone."""
    f = bytearray(hdr[:HDR]) + bytearray(data)
    dlen = len(data)
    struct.pack_into("!H", f, 16, 40 + dlen)
    f[24:26] = b"\x00\x00"
    f[24:26] = struct.pack("<H", pyoracle.checksum(bytes(f[14:34]), 20, 0))  # stored raw
    seq0 = struct.unpack_from("!I", hdr, 38)[0]
    struct.pack_into("!I", f, 38, (seq0 + seq_add) & 0xFFFFFFFF)
    if not last:
        f[47] &= ~0x09 & 0xFF  # FIN 0x01, PSH 0x08
    f[50:52] = b"\x00\x00"
    l4 = 20 + dlen
    seg = bytes(f[34:])
    c = pyoracle.checksum(seg, l4, seed_of(hdr, l4))
    ref = pyoracle.reflib()
    if ref is not None:  # the reference's own function agrees with the oracle's arithmetic
        sa, da = struct.unpack("<II", hdr[26:34])
        buf = ctypes.create_string_buffer(seg, l4)
        assert (ref.tcp_udp_checksum(sa, da, 6, buf, l4) & 0xFFFF) == c
    f[50:52] = struct.pack("<H", c)
    return bytes(f)


def build_expected(payload: np.ndarray, sends: np.ndarray, out_size: int):
    """(out, fd, spans): the whole buffer the calls must produce from one of
    `out_size` canary bytes, the frame descriptors, and (send, segment, offset,
    length) of every frame for the mismatch report."""
    out = np.full(out_size, CANARY, dtype=np.uint8)
    fds, spans = [], []
    for j, s in enumerate(sends):
        hdr = bytes(s["hdr"])
        mss, length = int(s["mss"]), int(s["len"])
        nseg = -(-length // mss)
        for i in range(nseg):
            lo = i * mss
            dlen = min(mss, length - lo)
            p0 = int(s["payload_off"]) + lo
            fr = build_frame(hdr, payload[p0:p0 + dlen].tobytes(), lo, i == nseg - 1)
            off = int(s["out_off"]) + i * int(s["stride"])
            out[off:off + len(fr)] = np.frombuffer(fr, dtype=np.uint8)
            fds.append((off, len(fr), 0))
            spans.append((j, i, off, len(fr)))
    return out, np.array(fds, dtype=lvlip.FRAME_DESC_DTYPE), spans


def assert_same(got: np.ndarray, want: np.ndarray, spans, what: str) -> None:
    """Whole-buffer comparison; a mismatch names send, segment and first byte."""
    assert got.shape == want.shape, what
    if np.array_equal(got, want):
        return
    b = int(np.flatnonzero(got != want)[0])
    where = "outside every frame (a stride gap or a neighbour)"
    for j, i, off, ln in spans:
        if off <= b < off + ln:
            where = f"send {j}, segment {i}, frame byte {b - off}"
            break
    pytest.fail(f"{what}: first difference at buffer byte {b} ({where}): got 0x{int(got[b]):02x}, "
                f"want 0x{int(want[b]):02x}; {int((got != want).sum())} bytes differ")


# -------------------------------------------------------------- the cases --

class Case:
    """One call: payload, planned sends, expected buffer and descriptors."""

    def __init__(self, name, payload, sends):
        self.name, self.payload, self.sends = name, payload, sends
        self.nseg, self.out_bytes = lvlip.tso_plan(sends)
        # room for the 16-B rounded read of lvlip_tx_checksum_dev behind the last frame
        self.out_size = (self.out_bytes + 15 & ~15) + 64
        self.want, self.fd, self.spans = build_expected(payload, sends, self.out_size)


def _payload(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


def lay_out(specs, fill=None, seed=1):
    """specs: (hdr, len, mss, payload offset mod 16, out offset mod 16, stride)
    -> (payload, sends), every send in a region of its own."""
    sends = np.zeros(len(specs), dtype=lvlip.TsoSend)
    ppos = opos = 0
    for r, (hdr, length, mss, pmod, omod, stride) in zip(sends, specs):
        r["hdr"] = np.frombuffer(hdr, dtype=np.uint8)
        r["len"], r["mss"], r["stride"] = length, mss, stride
        r["payload_off"] = (ppos + 15 & ~15) + pmod
        ppos = int(r["payload_off"]) + length
        r["out_off"] = (opos + 15 & ~15) + omod
        opos = int(r["out_off"]) + -(-length // mss) * stride
    payload = _payload(ppos, seed) if fill is None else np.full(ppos, fill, dtype=np.uint8)
    return payload, sends


@functools.lru_cache(maxsize=None)
def shape_case(mss: int) -> Case:
    """Every combination for one MSS: 1-3 segments x tail {1, mss-1, mss} x
    payload offset x frame alignment x {frames abut, 13-byte gap}, one call."""
    specs, k = [], 0
    for segs in (1, 2, 3):
        for tail in sorted({t for t in (1, mss - 1, mss) if t >= 1}):
            for pmod in PAYLOAD_OFFS:
                for omod in OUT_MODS:
                    for gap in GAPS:
                        hdr = template(ident=k & 0xFFFF, sport=1024 + k, flags=0x18 | (k & 1))
                        specs.append((hdr, (segs - 1) * mss + tail, mss, pmod, omod, HDR + mss + gap))
                        k += 1
    return Case(f"mss{mss}", *lay_out(specs, seed=mss))


def _wrap_template(mss: int) -> bytes:
    """Addresses whose seed for a full segment is 0xFFFFFF80: the seed itself
    does not wrap, seed + W does."""
    da = 0x01000001
    sa = (0xFFFFFF80 - da - _bswap16(6) - _bswap16(20 + mss)) & 0xFFFFFFFF
    return template(saddr=struct.pack("<I", sa), daddr=struct.pack("<I", da))


@functools.lru_cache(maxsize=None)
def parity_case() -> Case:
    """Odd MSS (every other segment's source starts on an odd byte), payload
    all 0xff, seq0 0xFFFFFF00; seeds that make seed + W wrap, and seeds that
    lose their own carry (10.0.0.200 -> 10.0.0.100)."""
    specs = []
    for mss in (17, 535):
        for hdr in (_wrap_template(mss), template(saddr=(10, 0, 0, 200), daddr=(10, 0, 0, 100))):
            for pmod, omod in ((0, 0), (1, 0), (0, 1), (7, 10), (15, 15)):
                specs.append((hdr, 3 * mss + 5, mss, pmod, omod, HDR + mss))
                specs.append((hdr, 4 * mss, mss, pmod, omod, HDR + mss + 13))
    return Case("parity", *lay_out(specs, fill=0xFF))


@functools.lru_cache(maxsize=None)
def multi_case() -> Case:
    """Three sends with different MSS, templates and strides in one call."""
    specs = [(template(sport=1111, ident=7), 2001, 536, 3, 6, 600),
             (template(saddr=(192, 168, 1, 9), daddr=(172, 16, 0, 1), dport=443, flags=0x19), 100, 17, 1, 15, 71),
             (template(seq=0x7FFFFFFF, win=1, urp=9, flags=0x38), 4000, 1460, 15, 1, 1536)]
    return Case("multi", *lay_out(specs, seed=99))


@functools.lru_cache(maxsize=None)
def single_case() -> Case:
    return Case("single", *lay_out([(template(), 10, 536, 7, 10, HDR + 536)], seed=5))


@functools.lru_cache(maxsize=None)
def big_case() -> Case:
    """1 MiB at MSS 1460: 719 segments, more than one workgroup."""
    return Case("big", *lay_out([(template(), 1 << 20, 1460, 1, 6, 1536)], seed=11))


@functools.lru_cache(maxsize=None)
def fixture():
    with open(GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def fixture_case() -> Case:
    """The reference's three sends (2001, 1072 and 1 B at smss 536), template
    from each send's first recorded frame with PSH set."""
    fx = fixture()
    specs, payloads = [], []
    for k, s in enumerate(fx["sends"]):
        hdr = bytearray(bytes.fromhex(s["frames"][0])[:HDR])
        hdr[47] |= 0x08
        specs.append((bytes(hdr), s["len"], fx["mss"], (1, 7, 0)[k], (6, 0, 15)[k], HDR + fx["mss"]))
        payloads.append(bytes.fromhex(s["payload_hex"]))
    payload, sends = lay_out(specs)
    for r, p in zip(sends, payloads):
        payload[int(r["payload_off"]):int(r["payload_off"]) + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return Case("fixture", payload, sends)


def fixture_frames(case: Case, out: np.ndarray):
    """The frames of the fixture case cut out of a produced buffer, per send."""
    res, k = [], 0
    for s in case.sends:
        n = -(-int(s["len"]) // int(s["mss"]))
        res.append([out[o:o + ln].tobytes() for _, _, o, ln in case.spans[k:k + n]])
        k += n
    return res


ALL_CASES = [pytest.param(functools.partial(shape_case, m), id=f"mss{m}") for m in MSS_LIST] + [
    pytest.param(parity_case, id="parity"), pytest.param(multi_case, id="multi"),
    pytest.param(single_case, id="single"), pytest.param(big_case, id="big"),
    pytest.param(fixture_case, id="fixture")]


# -------------------------------------------------------------- the tests --

def test_layout():
    assert lvlip.TsoSend.itemsize == 96
    assert lvlip.TsoSend.fields["hdr"][1] == 32 and lvlip.TsoSend.fields["mss"][1] == 28
    assert lvlip.lib().lvlip_abi_version() == 2


def test_builder_reproduces_the_reference_frames():
    """The builder alone against the reference's tcp_send frames."""
    case = fixture_case()
    got = fixture_frames(case, case.want)
    for s, frames in zip(fixture()["sends"], got):
        assert [f.hex() for f in frames] == s["frames"]


def test_tso_cpu_reproduces_the_reference_frames():
    case = fixture_case()
    out = np.full(case.out_size, CANARY, dtype=np.uint8)
    out, fd = lvlip.tso_cpu(case.payload, case.sends, out=out)
    for k, (s, frames) in enumerate(zip(fixture()["sends"], fixture_frames(case, out))):
        assert len(frames) == len(s["frames"])
        for i, (a, b) in enumerate(zip(frames, s["frames"])):
            assert a.hex() == b, f"send {k} ({s['len']} B), segment {i}"


@pytest.mark.parametrize("make", ALL_CASES)
def test_tso_cpu_equals_builder(make):
    case = make()
    payload = case.payload.copy()
    out = np.full(case.out_size, CANARY, dtype=np.uint8)
    out, fd = lvlip.tso_cpu(payload, case.sends, out=out)
    assert_same(out, case.want, case.spans, case.name)
    assert np.array_equal(fd, case.fd)
    assert np.array_equal(payload, case.payload)


def test_parity_case_wraps():
    """The parity case's seeds do what the case is for."""
    case = parity_case()
    wrapped = lost = 0
    for s in case.sends:
        hdr, mss = bytes(s["hdr"]), int(s["mss"])
        sa, da = struct.unpack("<II", hdr[26:34])
        raw = sa + da + _bswap16(6) + _bswap16(20 + mss)
        if raw >= 1 << 32:
            lost += 1  # the seed's own carry is lost
        elif raw >= (1 << 32) - 0x100:
            wrapped += 1  # W of a segment of 0xff bytes (>= 8 words of 0xffff) carries seed + W past 2^32
            assert raw + 8 * 0xFFFF >= 1 << 32
    assert wrapped > 0 and lost > 0
    assert all(int(s["mss"]) & 1 for s in case.sends)


def test_tso_plan_totals_and_seg0():
    case = multi_case()
    sends = case.sends.copy()
    sends["seg0"] = 0xDEAD
    nseg, out_bytes = lvlip.tso_plan(sends)
    assert nseg == 4 + 6 + 3 and sends["seg0"].tolist() == [0, 4, 10]
    last = sends[2]
    assert out_bytes == int(last["out_off"]) + 2 * 1536 + HDR + (4000 - 2 * 1460)
    # out_bytes is the largest end, whichever send has it
    sends = sends[::-1].copy()
    assert lvlip.tso_plan(sends) == (13, out_bytes) and sends["seg0"].tolist() == [0, 3, 9]
    for mss in MSS_LIST:
        c = shape_case(mss)
        assert c.nseg == sum(-(-int(s["len"]) // mss) for s in c.sends) == len(c.spans)
        assert c.out_bytes == max(o + ln for _, _, o, ln in c.spans)
        assert c.sends["seg0"].tolist() == np.concatenate(
            [[0], np.cumsum(-(-c.sends["len"].astype(np.int64) // mss))[:-1]]).tolist()
    assert big_case().nseg == 719
    assert lvlip.tso_plan(np.zeros(0, dtype=lvlip.TsoSend)) == (0, 0)


def _bad_sends():
    def base():
        return lvlip.tso_send(template(), 0, 40, 16, out_off=3, stride=70)
    cases = {}
    for name, field, value in (("len0", "len", 0), ("mss0", "mss", 0), ("stride", "stride", 69),
                               ("reserved", "reserved", 1)):
        r = base()
        r[field] = value
        cases[name] = r
    for name, byte, value in (("ethertype", 12, 0x86), ("ihl", 14, 0x46), ("version", 14, 0x65),
                              ("proto", 23, 17), ("tcp_hl", 46, 0x60)):
        r = base()
        r["hdr"][0][byte] = value
        cases[name] = r
    return cases


@pytest.mark.parametrize("name", sorted(_bad_sends()))
def test_malformed_send_refused(name):
    L = lvlip.lib()
    bad = _bad_sends()[name]
    good = lvlip.tso_send(template(), 0, 40, 16, out_off=300, stride=70)
    payload = _payload(64, 3)
    for sends in (bad, np.concatenate([good, bad])):  # alone, and behind a valid send
        sends = np.ascontiguousarray(sends)
        ob = ctypes.c_uint64(7)
        assert L.lvlip_tso_plan(sends.ctypes.data, sends.size, ctypes.byref(ob)) == 0xFFFFFFFF
        with pytest.raises(ValueError):
            lvlip.tso_plan(sends)
        out = np.full(1024, CANARY, dtype=np.uint8)
        fd = np.full(16, 0x5A5A5A5A, dtype=np.uint32)
        sends["seg0"] = np.arange(sends.size) * 3  # what a plan would have left
        assert L.lvlip_tso_cpu(payload.ctypes.data, sends.ctypes.data, sends.size, out.ctypes.data,
                               fd.ctypes.data) == lvlip.EINVAL
        assert (out == CANARY).all() and (fd == 0x5A5A5A5A).all()


def test_plan_refuses_too_many_segments():
    L = lvlip.lib()
    sends = np.concatenate([lvlip.tso_send(template(), 0, 0xFFFFFFFF, 1, stride=55) for _ in range(2)])
    assert L.lvlip_tso_plan(sends.ctypes.data, 2, None) == 0xFFFFFFFF
    assert L.lvlip_tso_plan(sends.ctypes.data, 1, None) == 0xFFFFFFFF  # one send above LVLIP_MAX_BATCH
    sends["len"] = 0x7FFFFFF8
    assert L.lvlip_tso_plan(sends.ctypes.data, 2, None) == 0xFFFFFFF0  # exactly LVLIP_MAX_BATCH


def test_unplanned_or_null_refused_by_cpu_form():
    L = lvlip.lib()
    case = single_case()
    out = np.full(case.out_size, CANARY, dtype=np.uint8)
    sends = case.sends.copy()
    sends["seg0"] = 1
    assert L.lvlip_tso_cpu(case.payload.ctypes.data, sends.ctypes.data, 1, out.ctypes.data, None) == lvlip.EINVAL
    for args in ((None, case.sends.ctypes.data, out.ctypes.data), (case.payload.ctypes.data, None, out.ctypes.data),
                 (case.payload.ctypes.data, case.sends.ctypes.data, None)):
        assert L.lvlip_tso_cpu(args[0], args[1], 1, args[2], None) == lvlip.EINVAL
    assert (out == CANARY).all()
    assert L.lvlip_tso_cpu(None, None, 0, None, None) == lvlip.OK


def test_dev_error_paths_without_gpu():
    """As tests/test_abi.py::test_error_paths_without_gpu: refused before any
    HIP call, so it runs without a device."""
    L = lvlip.lib()
    assert L.lvlip_tso_dev(None, None, 0, 0, None, None, None) == lvlip.OK
    assert L.lvlip_tso_dev(None, None, 0, 5, None, None, None) == lvlip.OK
    assert L.lvlip_tso_dev(None, 4096, 1, 1, 4096, None, None) == lvlip.EINVAL
    assert L.lvlip_tso_dev(4096, None, 1, 1, 4096, None, None) == lvlip.EINVAL
    assert L.lvlip_tso_dev(4096, 4096, 1, 1, None, None, None) == lvlip.EINVAL
    assert L.lvlip_tso_dev(4096, 4096, 1, 0, 4096, None, None) == lvlip.EINVAL
    assert L.lvlip_tso_dev(4096, 4096, 1, 0xFFFFFFFF, 4096, None, None) == lvlip.EINVAL


def test_example_under_sanitizers(tmp_path):
    """examples/tso_frames.c (its own main: plan + CPU form over the shape
    list, buffers malloc'd at exactly the planned sizes) compiled with the
    library's C sources under ASan + UBSan, and run as a program."""
    exe = tmp_path / "tso_frames_san"
    src = [os.path.join(ROOT, "examples", "tso_frames.c")] + [
        os.path.join(ROOT, "level-ip_amd", "csrc", f) for f in ("seg_cpu.c", "csum_cpu.c")]
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "include"), *src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tso_frames ok" in r.stdout
