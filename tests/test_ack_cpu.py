"""The acknowledgement calls (include/lvlip_skb.h, lvlip_ack_*) without a GPU:
the CPU form against the ACK frames the reference's own stack sent
(tests/golden/ack_ref.json, written by tests/golden/make_ack_golden.py from the
unmodified stack), against an independent model over hand-written results, the
plan and its refusals, the layout, the refusals of the CPU and device forms, a
sanitizer build of examples/ack_loop.c, and the kernel's scratch size.

The model (model_frame, model_run) builds a frame with struct.pack from the
semantics in the header; its checksums come from the oracle
(pyoracle.checksum), never from the product.  tests/test_ack_gpu.py shares it,
with the cases."""
import ctypes
import functools
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import lvlip
import pyoracle
from tcp_model import _bswap16, _fold, lost_carry_seed  # noqa: F401  (other tests import them from here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ack_ref.json")
CANARY = 0x5A
M32 = 0xFFFFFFFF
ETH = bytes.fromhex("0a1b2c3d4e5f000c296d5025") + b"\x08\x00"


# --------------------------------------------------------------- the model --

def model_frame(hdr: bytes, rcv_nxt: int, delivered: int, nsack: int, sack, max_sack: int, seed_fn=lost_carry_seed):
    """The ACK frame of one flow from the header's text."""
    b = min(nsack, max_sack, 4)
    optlen = 4 + 8 * b if b else 0
    ip = bytearray(hdr[14:34])
    ip[2:4] = struct.pack("!H", 40 + optlen)
    ip[10:12] = b"\x00\x00"
    ip[10:12] = struct.pack("<H", pyoracle.checksum(bytes(ip), 20, 0))
    tcp = bytearray(hdr[34:54])
    tcp[8:12] = struct.pack("!I", (rcv_nxt + delivered) & M32)
    tcp[12] = ((5 + optlen // 4) << 4) | (tcp[12] & 0x0F)
    tcp[16:18] = b"\x00\x00"
    if b:
        tcp += b"\x01\x01\x05" + bytes([2 + 8 * b])
        for i in reversed(range(b)):
            tcp += struct.pack("!II", int(sack[i][0]), int(sack[i][1]))
    tcp[16:18] = struct.pack("<H", pyoracle.checksum(bytes(tcp), len(tcp), seed_fn(hdr[26:30], hdr[30:34], len(tcp))))
    return bytes(hdr[:14]) + bytes(ip) + bytes(tcp)


def model_run(tmpl: np.ndarray, flows: np.ndarray, res: np.ndarray, flags: int, out_size: int):
    """(out, fd): the whole buffer the calls must leave from one of canary
    bytes, and the descriptors."""
    out = np.full(out_size, CANARY, dtype=np.uint8)
    fd = np.zeros(flows.size, dtype=lvlip.FRAME_DESC_DTYPE)
    for k in range(flows.size):
        off = int(tmpl[k]["out_off"])
        fd[k] = (off, 0, 0)
        if not (flags & lvlip.ACK_ALL) and int(res[k]["placed"]) == 0:
            continue
        fr = model_frame(tmpl[k]["hdr"].tobytes(), int(flows[k]["rcv_nxt"]), int(res[k]["delivered"]),
                         int(res[k]["nsack"]), res[k]["sack"], int(tmpl[k]["max_sack"]))
        out[off:off + len(fr)] = np.frombuffer(fr, dtype=np.uint8)
        fd[k] = (off, len(fr), 0)
    return out, fd


# --------------------------------------------------------------- the cases --

def make_flows(n: int, addr=None) -> np.ndarray:
    """n planned flows: peers 10.0.0.x -> 10.0.0.4 (so that the pseudo-header
    seed does not wrap), distinct by source port; addr overrides (saddr,
    daddr) of all of them."""
    k = np.arange(n)
    fl = np.zeros(n, dtype=lvlip.LRO_FLOW_DTYPE)
    fl["saddr"] = 10 | ((5 + k % 200) << 24) if addr is None else int.from_bytes(addr[0], "little")
    fl["daddr"] = 10 | (4 << 24) if addr is None else int.from_bytes(addr[1], "little")
    port = 1000 + k
    fl["sport"] = ((port & 0xFF) << 8) | (port >> 8)
    fl["dport"] = _bswap16(8000)
    fl["rcv_nxt"] = (0xFFFFF000 + 0x01010101 * k) & M32
    fl["rcv_wnd"], fl["out_off"], fl["user"] = 1 << 16, k << 16, k
    lvlip.lro_plan(fl)
    return fl


def template_hdr(flow, seq: int = 0x0A0B0C0D, flags: int = 0x10, low_nibble: int = 0) -> bytes:
    """The 54 bytes of the stack's own pure ACK to this flow's peer; the fields
    the calls ignore hold garbage."""
    saddr, daddr = struct.pack("<I", int(flow["daddr"])), struct.pack("<I", int(flow["saddr"]))
    ip = struct.pack("!BBHHHBBH4s4s", 0x45, 0, 0xDEAD, 0x1234, 0x4000, 64, 6, 0xBEEF, saddr, daddr)
    tcp = struct.pack("!HHIIBBHHH", _bswap16(int(flow["dport"])), _bswap16(int(flow["sport"])), seq, 0xDEADBEEF,
                      0x50 | low_nibble, flags, 0xADBD, 0xFFFF, 0)
    return ETH + ip + tcp


def make_tmpl(flows: np.ndarray, max_sack, stride: int = 90, first: int = 0) -> np.ndarray:
    """A template per planned flow, slot k at first + k * stride."""
    t = np.zeros(flows.size, dtype=lvlip.ACK_TMPL_DTYPE)
    for k, f in enumerate(flows):
        t[k]["hdr"] = np.frombuffer(template_hdr(f, seq=(0x0A0B0C0D + 977 * k) & M32, low_nibble=k & 1 and 0x0A),
                                    dtype=np.uint8)
    t["out_off"] = first + stride * np.arange(flows.size)
    t["max_sack"] = max_sack
    return t


def random_res(n: int, seed: int) -> np.ndarray:
    """Results as lvlip_lro_advance leaves them (every nsack, about a third of
    the flows without a PLACED frame), and a few no library call wrote: nsack
    above 4, left edge 0."""
    rng = np.random.default_rng(seed)
    res = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
    res["delivered"] = rng.integers(0, 1 << 30, n)
    res["placed"] = rng.integers(0, 3, n)
    res["nsack"] = np.arange(n) % 5
    res["sack"] = rng.integers(1, 1 << 32, (n, 4, 2), dtype=np.uint64).astype(np.uint32)
    if n > 20:
        res["nsack"][7], res["nsack"][11] = 5, M32
        res["sack"][14][0][0] = 0
    return res


class Hand:
    """The hand-written case: nsack 0..4 crossed with max_sack 0..4, clamped
    nsack values, ack_seq wrapping, a left edge 0, placed == 0, slots 91 apart
    so that the frames start at every residue mod 16."""

    def __init__(self):
        combos = [(ns, ms) for ns in range(5) for ms in range(5)] + [(5, 4), (M32, 4), (5, 2), (M32, 0)]
        n = len(combos) + 3
        self.flows = make_flows(n)
        self.tmpl = make_tmpl(self.flows, 4, stride=91, first=3)
        self.res = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
        rng = np.random.default_rng(12)
        self.res["sack"] = rng.integers(1, 1 << 32, (n, 4, 2), dtype=np.uint64).astype(np.uint32)
        self.res["delivered"] = rng.integers(0, 1 << 16, n)
        self.res["placed"] = 1 + np.arange(n) % 3
        for k, (ns, ms) in enumerate(combos):
            self.res[k]["nsack"], self.tmpl[k]["max_sack"] = ns, ms
        k = len(combos)
        self.wrap = k  # rcv_nxt + delivered wraps 2^32
        self.flows[k]["rcv_nxt"], self.res[k]["delivered"], self.res[k]["nsack"] = 0xFFFFFF00, 0x1234, 1
        self.left0 = k + 1  # a block whose left edge is sequence number 0
        self.res[k + 1]["nsack"] = 3
        self.res[k + 1]["sack"][1] = (0, 536)
        self.idle = k + 2  # no PLACED frame
        self.res[k + 2]["placed"], self.res[k + 2]["nsack"] = 0, 2
        self.out_size = lvlip.ack_plan(self.tmpl, self.flows) + 7
        assert sorted({int(o) % 16 for o in self.tmpl["out_off"]}) == list(range(16))


@functools.lru_cache(maxsize=None)
def hand() -> Hand:
    return Hand()


def assert_same_out(got: np.ndarray, want: np.ndarray, tmpl: np.ndarray, what: str) -> None:
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        b = int(np.flatnonzero(got != want)[0])
        k = int(np.searchsorted(tmpl["out_off"], b, side="right")) - 1
        pytest.fail(f"{what}: first difference at out byte {b} (flow {k}, frame byte {b - int(tmpl[k]['out_off'])}): "
                    f"got 0x{int(got[b]):02x}, want 0x{int(want[b]):02x}; {int((got != want).sum())} bytes differ")


@functools.lru_cache(maxsize=None)
def fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_inputs():
    """(fixture, frame buffer, fd, planned flow, template): the reference's
    segments in arrival order, and the template its handshake ACK gives."""
    fx = fixture()
    frames = [bytes.fromhex(h) for h in fx["frames"]]
    f0 = frames[0]
    flow = lvlip.lro_flow(f0[26:30], f0[30:34], *struct.unpack_from("!HH", f0, 34), fx["rcv_nxt"], 8192, out_off=3)
    lvlip.lro_plan(flow)
    buf, fd = lvlip.pack_frames(frames, align_mod=16, seed=4)
    tmpl = lvlip.ack_tmpl(bytes.fromhex(fx["template"]), out_off=5, max_sack=fx["max_sack"])
    return fx, buf, fd, flow, tmpl


def golden_compared(fx):
    """(arrival index, the reference's ACK) for every ACK that carries SACK
    blocks: the immediate ACK of an out-of-order arrival."""
    return [(j, bytes.fromhex(a)) for j, a in enumerate(fx["acks"]) if a is not None]


# --------------------------------------------------------------- the tests --

def test_layout():
    assert lvlip.ACK_TMPL_DTYPE.itemsize == 64
    assert [lvlip.ACK_TMPL_DTYPE.fields[n][1] for n in ("out_off", "hdr", "max_sack", "reserved")] == [0, 8, 62, 63]

    class Tmpl(ctypes.Structure):  # the header's declaration, field for field
        _fields_ = [("out_off", ctypes.c_uint64), ("hdr", ctypes.c_uint8 * 54), ("max_sack", ctypes.c_uint8),
                    ("reserved", ctypes.c_uint8)]
    assert ctypes.sizeof(Tmpl) == 64 and Tmpl.max_sack.offset == 62
    assert lvlip.ACK_MAX_FRAME == 90 == 14 + 20 + 20 + 4 + 4 * 8 and lvlip.ACK_ALL == 1
    for name in ("lvlip_ack_plan", "lvlip_ack_cpu", "lvlip_ack_dev"):
        assert getattr(lvlip.lib(), name).argtypes == lvlip.SIGNATURES[name][1]
    assert lvlip.lib().lvlip_abi_version() == 2


def test_fixture_holds_the_cases():
    """What the golden test rests on, read off the reference's frames."""
    fx = fixture()
    cmp = golden_compared(fx)
    nblocks = [(len(a) - 58) // 8 for _, a in cmp]
    assert len(cmp) >= 6 and all(a[54:57] == b"\x01\x01\x05" for _, a in cmp)
    assert 2 in nblocks and 4 in nblocks
    assert any(struct.unpack_from("!I", a, 42)[0] != fx["rcv_nxt"] for _, a in cmp)
    # two adjacent segments in one block: a block twice the segment size
    assert any(r - le == 2 * fx["seg"] for _, a in cmp for le, r in
               (struct.unpack_from("!II", a, 58 + 8 * i) for i in range((len(a) - 58) // 8)))
    assert len(bytes.fromhex(fx["template"])) == 54


def test_ack_cpu_reproduces_the_reference_acks():
    """After every out-of-order arrival j the reference sent one ACK with its
    SACK list; lvlip_lro_cpu over arrivals 0..j, lvlip_lro_advance and
    lvlip_ack_cpu give that frame byte for byte."""
    fx, buf, fd, flow, tmpl = golden_inputs()
    for j, want in golden_compared(fx):
        _, rec = lvlip.lro_cpu(buf, fd[:j + 1], flow, lvlip.RX_VERIFY_L4)
        assert (rec["status"] == lvlip.LRO_PLACED).all()
        res = lvlip.lro_advance(flow, rec)
        out = np.full(5 + 90 + 9, CANARY, dtype=np.uint8)
        out, afd = lvlip.ack_cpu(tmpl, flow, res, 0, out=out)
        assert (int(afd[0]["offset"]), int(afd[0]["len"])) == (5, len(want)), f"arrival {j}"
        assert out[5:5 + len(want)].tobytes().hex() == want.hex(), f"arrival {j}"
        assert (out[:5] == CANARY).all() and (out[5 + len(want):] == CANARY).all()


@pytest.mark.parametrize("flags", (0, lvlip.ACK_ALL))
def test_ack_cpu_equals_model(flags):
    h = hand()
    want_out, want_fd = model_run(h.tmpl, h.flows, h.res, flags, h.out_size)
    before = [a.copy() for a in (h.tmpl, h.flows, h.res)]
    out = np.full(h.out_size, CANARY, dtype=np.uint8)
    fdbuf = np.full(h.flows.size * 16 + 32, CANARY, dtype=np.uint8)
    rc = lvlip.lib().lvlip_ack_cpu(h.tmpl.ctypes.data, h.flows.ctypes.data, h.res.ctypes.data, h.flows.size, flags,
                                   out.ctypes.data, fdbuf.ctypes.data)
    assert rc == lvlip.OK
    assert_same_out(out, want_out, h.tmpl, f"flags {flags}")
    assert np.array_equal(fdbuf[:-32].view(lvlip.FRAME_DESC_DTYPE), want_fd)
    assert (fdbuf[-32:] == CANARY).all(), "written behind fd"
    for a, b in zip((h.tmpl, h.flows, h.res), before):
        assert np.array_equal(a, b), "t, f and res are only read"
    # the wrapper (plan, then the call) and a NULL fd give the same bytes
    out2, fd2 = lvlip.ack_cpu(h.tmpl, h.flows, h.res, flags, out=np.full(h.out_size, CANARY, dtype=np.uint8))
    assert np.array_equal(out2, want_out) and np.array_equal(fd2, want_fd)
    out3 = np.full(h.out_size, CANARY, dtype=np.uint8)
    assert lvlip.lib().lvlip_ack_cpu(h.tmpl.ctypes.data, h.flows.ctypes.data, h.res.ctypes.data, h.flows.size, flags,
                                     out3.ctypes.data, None) == lvlip.OK
    assert np.array_equal(out3, want_out)


def test_the_named_cases():
    """What the model says about the edge cases, so that none is vacuous."""
    h = hand()
    out, fd = lvlip.ack_cpu(h.tmpl, h.flows, h.res, 0)
    frame = lambda k: out[int(fd[k]["offset"]):int(fd[k]["offset"]) + int(fd[k]["len"])].tobytes()  # noqa: E731
    for k in range(29):
        ns, ms = int(h.res[k]["nsack"]), int(h.tmpl[k]["max_sack"])
        b = min(ns, ms, 4)
        assert int(fd[k]["len"]) == 54 + (4 + 8 * b if b else 0), (ns, ms)
        assert frame(k)[46] >> 4 == 5 + (1 + 2 * b if b else 0) and frame(k)[46] & 15 == (k & 1 and 0x0A)
    assert struct.unpack_from("!I", frame(h.wrap), 42)[0] == 0x00001134  # 0xFFFFFF00 + 0x1234 mod 2^32
    fr = frame(h.left0)  # three blocks, the middle one's left edge 0: written (the reference would drop it)
    assert len(fr) == 54 + 28 and struct.unpack_from("!II", fr, 58 + 8) == (0, 536)
    assert [struct.unpack_from("!II", fr, 58 + 8 * i) for i in (0, 2)] == [tuple(int(v) for v in h.res[h.left0]["sack"][i])
                                                                           for i in (2, 0)], "descending"
    assert int(fd[h.idle]["len"]) == 0 and int(fd[h.idle]["offset"]) == int(h.tmpl[h.idle]["out_off"])
    out_all, fd_all = lvlip.ack_cpu(h.tmpl, h.flows, h.res, lvlip.ACK_ALL)
    assert int(fd_all[h.idle]["len"]) == 54 + 20


def test_pseudo_header_carry_is_lost():
    """Addresses whose u32 sum wraps: the field holds the reference's sum
    (src/tcp.c:92-95 loses the carry), which is not the RFC's."""
    saddr, daddr = bytes((254, 255, 255, 255)), bytes((7, 0, 0, 128))
    flows = make_flows(3, addr=(saddr, daddr))
    tmpl = make_tmpl(flows, 4)
    res = random_res(3, 1)
    res["nsack"], res["placed"] = (0, 2, 4), 1
    assert int(flows[0]["saddr"]) + int(flows[0]["daddr"]) >= 1 << 32
    out, fd = lvlip.ack_cpu(tmpl, flows, res, 0)
    got = out
    rfc = lambda s, d, n: _fold(sum(struct.unpack("<4H", s + d)) + _bswap16(6) + _bswap16(n))  # noqa: E731
    for k in range(3):
        o, n = int(fd[k]["offset"]), int(fd[k]["len"])
        fr = model_frame(tmpl[k]["hdr"].tobytes(), int(flows[k]["rcv_nxt"]), int(res[k]["delivered"]),
                         int(res[k]["nsack"]), res[k]["sack"], 4)
        assert got[o:o + n].tobytes() == fr
        fr_rfc = model_frame(tmpl[k]["hdr"].tobytes(), int(flows[k]["rcv_nxt"]), int(res[k]["delivered"]),
                             int(res[k]["nsack"]), res[k]["sack"], 4, seed_fn=rfc)
        assert fr_rfc[50:52] != fr[50:52], "the RFC's sum differs: the lost carry shows in the field"
        assert fr_rfc[:50] == fr[:50] and fr_rfc[52:] == fr[52:]


# ------------------------------------------------------------------ the plan --

def _plan(t, f, n=None):
    ob = ctypes.c_uint64(7)
    r = lvlip.lib().lvlip_ack_plan(t.ctypes.data, f.ctypes.data, t.size if n is None else n, ctypes.byref(ob))
    return r, ob.value


def _plan_refusals():
    def base():
        fl = make_flows(3)
        return make_tmpl(fl, 4, stride=100), fl
    cases = {}
    for name, byte, value in (("ethertype", 12, 0x86), ("version_ihl", 14, 0x46), ("protocol", 23, 17),
                              ("tcp_hl", 46, 0x60), ("saddr", 26, 11), ("daddr", 33, 99), ("sport", 35, 0x41),
                              ("dport", 37, 0x77)):
        t, fl = base()
        t[1]["hdr"][byte] = value
        cases[name] = (t, fl)
    for name, field, value in (("max_sack", "max_sack", 5), ("reserved", "reserved", 1), ("overlap", "out_off", 189),
                               ("out_off_wraps", "out_off", (1 << 64) - 50)):
        t, fl = base()
        t[1][field] = value
        cases[name] = (t, fl)
    return cases


@pytest.mark.parametrize("name", sorted(_plan_refusals()))
def test_plan_refusals(name):
    t, fl = _plan_refusals()[name]
    before = t.copy()
    assert _plan(t, fl) == (0xFFFFFFFF, 0), name
    assert np.array_equal(t, before)
    with pytest.raises(ValueError):
        lvlip.ack_plan(t, fl)


def test_plan_accepts_and_sizes():
    L = lvlip.lib()
    fl = make_flows(3)
    t = make_tmpl(fl, 4, stride=100)
    assert _plan(t, fl) == (3, 290)
    t[1]["out_off"] = 110  # slot 1 ends where slot 2 begins
    assert _plan(t, fl) == (3, 290)
    t["out_off"] = (1000, 0, 500)  # any order
    assert _plan(t, fl) == (3, 1090) and lvlip.ack_plan(t, fl) == 1090
    t["max_sack"] = (0, 2, 4)
    assert _plan(t, fl)[0] == 3
    assert L.lvlip_ack_plan(t.ctypes.data, fl.ctypes.data, 3, None) == 3
    assert L.lvlip_ack_plan(None, None, 0, None) == 0
    assert L.lvlip_ack_plan(None, fl.ctypes.data, 3, None) == 0xFFFFFFFF
    assert L.lvlip_ack_plan(t.ctypes.data, None, 3, None) == 0xFFFFFFFF
    assert _plan(t, fl, 65537) == (0xFFFFFFFF, 0)  # refused before any template is read


def test_plan_catches_templates_in_the_old_order():
    """lvlip_lro_plan reorders the flows; templates written in the caller's
    order no longer answer their flows, and the plan says so."""
    k = np.arange(17)
    fl = np.zeros(17, dtype=lvlip.LRO_FLOW_DTYPE)
    fl["saddr"], fl["daddr"] = 10 | (5 << 24), 10 | (4 << 24)
    port = 40001 + 7 * ((k * 5) % 17)  # not ascending
    fl["sport"], fl["dport"] = ((port & 0xFF) << 8) | (port >> 8), _bswap16(8000)
    fl["rcv_wnd"], fl["out_off"], fl["user"] = 100, 100 * k, k
    t_old = make_tmpl(fl, 4)
    planned = fl.copy()
    lvlip.lro_plan(planned)
    assert planned["user"].tolist() != list(range(17)), "the plan reordered the flows"
    assert _plan(t_old, planned)[0] == 0xFFFFFFFF
    t_new = make_tmpl(planned, 4)
    assert _plan(t_new, planned) == (17, 17 * 90)
    assert _plan(t_old[planned["user"]].copy(), planned)[0] == 17  # the old templates, carried along


# ------------------------------------------------------------- the refusals --

def test_cpu_and_dev_refusals_without_gpu():
    """Refused before anything is written, and for the device form before any
    HIP call, so this runs without a device (host memory stands in for the
    device pointers)."""
    L = lvlip.lib()
    h = hand()
    n = h.flows.size
    out = np.full(h.out_size, CANARY, dtype=np.uint8)
    fdbuf = np.full(16 * n + 16, CANARY, dtype=np.uint8)
    resbuf = np.zeros(48 * n + 16, dtype=np.uint8)
    r = resbuf.ctypes.data + (-resbuf.ctypes.data % 16)
    ctypes.memmove(r, h.res.ctypes.data, 48 * n)
    d = fdbuf.ctypes.data + (-fdbuf.ctypes.data % 16)
    t, f, o = h.tmpl.ctypes.data, h.flows.ctypes.data, out.ctypes.data
    assert t % 8 == 0 and f % 8 == 0
    both = {"NULL t": (None, f, r, n, 0, o, d), "NULL f": (t, None, r, n, 0, o, d), "NULL res": (t, f, None, n, 0, o, d),
            "NULL out": (t, f, r, n, 0, None, d), "flag bit 1": (t, f, r, n, 2, o, d),
            "flag bit 31": (t, f, r, n, 0x80000001, o, d), "nflows above LVLIP_LRO_MAX_FLOWS": (t, f, r, 65537, 0, o, d)}
    for what, args in both.items():
        assert L.lvlip_ack_cpu(*args) == lvlip.EINVAL, what
        assert L.lvlip_ack_dev(*args, None) == lvlip.EINVAL, what
    dev_only = {"t at 4 mod 8": (t + 4, f, r, n, 0, o, d), "f at 4 mod 8": (t, f + 4, r, n, 0, o, d),
                "res at 8 mod 16": (t, f, r + 8, n, 0, o, d), "fd at 8 mod 16": (t, f, r, n, 0, o, d + 8)}
    for what, args in dev_only.items():
        assert L.lvlip_ack_dev(*args, None) == lvlip.EINVAL, what
    assert (out == CANARY).all() and (fdbuf == CANARY).all()
    assert L.lvlip_ack_cpu(None, None, None, 0, 0, None, None) == lvlip.OK
    assert L.lvlip_ack_cpu(t, f, r, 0, 0, o, d) == lvlip.OK
    assert L.lvlip_ack_cpu(None, None, None, 0, 2, None, None) == lvlip.OK  # nothing to do comes first
    assert L.lvlip_ack_dev(None, None, None, 0, 0, None, None, None) == lvlip.OK
    assert L.lvlip_ack_dev(t, f, r, 0, 0, o, d, None) == lvlip.OK
    assert (out == CANARY).all() and (fdbuf == CANARY).all()


# ------------------------------------------------ the example and the kernel --

def test_example_under_sanitizers(tmp_path):
    """examples/ack_loop.c (its own main: TSO frames, shuffled, coalesced,
    advanced and acknowledged on the CPU forms, every buffer malloc'd at
    exactly its planned size) compiled with the library's C sources under
    ASan + UBSan, and run as a program."""
    exe = tmp_path / "ack_loop_san"
    src = [os.path.join(ROOT, "examples", "ack_loop.c")] + [
        os.path.join(ROOT, "level-ip_amd", "csrc", f) for f in ("ack_cpu.c", "rcv_cpu.c", "seg_cpu.c", "csum_cpu.c")]
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "include"), *src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ack_loop ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_kernel_uses_no_scratch(tmp_path):
    """k_ack keeps the frame's 23 dwords in registers and selects with masks;
    a runtime index would put them in scratch: the private segment is 0."""
    asm = tmp_path / "ack_kernels.s"
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    "-S", "--cuda-device-only", os.path.join(ROOT, "level-ip_amd", "csrc", "ack_kernels.hip"),
                    "-o", str(asm)], check=True, capture_output=True)
    text = asm.read_text()
    kernels = re.findall(r"\.name:\s+(\S*k_ack\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(kernels) == 1, kernels
    assert all(int(size) == 0 for _, size in kernels), kernels
