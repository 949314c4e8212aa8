"""TCP receive coalescing (include/lvlip_skb.h, lvlip_lro_*) without a GPU: the
plan, the CPU form and the advance step against an independent model, against
lvlip_rx_verify_cpu for the ip_rcv verdicts, against the segmentation calls
(a round trip), against what the reference's own tcp_data_queue and
tcp_data_dequeue return (tests/golden/lro_ref.json, written by
tests/golden/make_lro_golden.py from the unmodified stack), the refusals, a
sanitizer build of examples/lro_stream.c, and the kernel's scratch size.

The model (model_rec, model_run, model_advance) parses frames with struct and
numpy from the semantics in the header; its checksums come from the oracle
(pyoracle.checksum), never from the product.  tests/test_lro_gpu.py shares it,
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
import ref_rx_cases
from tcp_model import _bswap16, _fold, pseudo_rfc
from test_tso_cpu import template as tso_template

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lro_ref.json")
CANARY = 0xA5
NONE = 0xFFFFFFFF
ETH = bytes.fromhex("000c296d50250a1b2c3d4e5f") + b"\x08\x00"
PEER, ME = bytes((10, 0, 0, 5)), bytes((10, 0, 0, 4))
FRAME_MODS = (0, 1, 6, 15)
OUT_MODS = (0, 1, 7, 15)
N_LIST = (1, 15, 16, 17, 257)
FLOW_COUNTS = (1, 3, 17)


# -------------------------------------------------------------- the frames --

def tcp_frame(payload: bytes, seq: int, sport: int = 40001, dport: int = 8000, saddr: bytes = PEER,
              daddr: bytes = ME, ack: int = 0x01020304, flags: int = 0x10, ihl: int = 5, hl: int = 5,
              hl_field=None, l4_ok: bool = True, urp: int = 0) -> bytes:
    """An Ethernet/IPv4/TCP frame a correct peer would send: NOP options, both
    checksums right (l4_ok False: the TCP field off by one bit)."""
    topts = b"\x01" * ((hl - 5) * 4)
    tcp = bytearray(struct.pack("!HHIIBBHHH", sport, dport, seq & 0xFFFFFFFF, ack, (hl if hl_field is None else
                                                                                     hl_field) << 4, flags,
                                0xADBD, 0, urp) + topts + payload)
    c = pyoracle.checksum(bytes(tcp), len(tcp), _fold(pseudo_rfc(saddr, daddr, len(tcp))))
    tcp[16:18] = struct.pack("<H", c if l4_ok else c ^ 0x0100)
    ip = bytearray(struct.pack("!BBHHHBBH4s4s", 0x40 | ihl, 0, ihl * 4 + len(tcp), 0x1234, 0x4000, 64, 6, 0, saddr,
                               daddr) + b"\x01" * ((ihl - 5) * 4))
    ip[10:12] = struct.pack("<H", pyoracle.checksum(bytes(ip), len(ip), 0))
    return ETH + bytes(ip) + bytes(tcp)


# --------------------------------------------------------------- the model --

def model_rec(fr: bytes, flows: np.ndarray, flags: int):
    """(flow, rel, dlen, status, tcp_flags, ack_seq, payload offset in the
    frame) of one frame, from the header's text."""
    bad = lambda st: (NONE, 0, 0, st, 0, 0, 0)  # noqa: E731
    n = len(fr)
    if n < 34:
        return bad(lvlip.RX_SHORT)
    if fr[12:14] != b"\x08\x00":
        return bad(lvlip.RX_NOT_IP)
    ihl = fr[14] & 15
    if fr[14] >> 4 != 4:
        return bad(lvlip.RX_BAD_VERSION)
    if ihl < 5:
        return bad(lvlip.RX_BAD_IHL)
    if fr[22] == 0:
        return bad(lvlip.RX_TTL0)
    if n < 14 + ihl * 4:
        return bad(lvlip.RX_SHORT)
    if pyoracle.checksum(fr[14:14 + ihl * 4], ihl * 4, 0) != 0:
        return bad(lvlip.RX_BAD_CSUM)
    proto = fr[23]
    if proto not in (1, 6):
        return bad(lvlip.RX_UNKNOWN_PROTO)
    iplen = struct.unpack_from("!H", fr, 16)[0]
    inside = iplen >= ihl * 4 and n >= 14 + iplen
    t = 14 + ihl * 4
    l4len = iplen - ihl * 4 if inside else 0
    if flags & lvlip.RX_VERIFY_L4:
        if not inside:
            return bad(lvlip.RX_SHORT)
        seed = _fold(pseudo_rfc(fr[26:30], fr[30:34], l4len)) if proto == 6 else 0
        if pyoracle.checksum(fr[t:t + l4len], l4len, seed) != 0:
            return bad(lvlip.RX_BAD_L4)
    if proto != 6:
        return bad(lvlip.LRO_NOT_TCP)
    if not inside or l4len < 20:
        return bad(lvlip.LRO_BAD_TCP_HDR)
    hl = fr[t + 12] >> 4
    if hl < 5 or hl * 4 > l4len:
        return bad(lvlip.LRO_BAD_TCP_HDR)
    seq, ack = struct.unpack_from("!II", fr, t + 4)
    dlen, tf = l4len - hl * 4, fr[t + 13]
    key = fr[26:34] + fr[t:t + 4]
    hit = [k for k, f in enumerate(flows) if f.tobytes()[:12] == key]
    if not hit:
        return (NONE, seq, dlen, lvlip.LRO_NO_FLOW, tf, ack, 0)
    k = hit[0]
    rel = (seq - int(flows[k]["rcv_nxt"])) & 0xFFFFFFFF
    if tf & 0x26:
        st = lvlip.LRO_CONTROL
    elif dlen == 0:
        st = lvlip.LRO_NO_DATA
    elif rel + dlen > int(flows[k]["rcv_wnd"]):
        st = lvlip.LRO_OUT_OF_WINDOW
    else:
        st = lvlip.LRO_PLACED
    return (k, rel, dlen, st, tf, ack, t + hl * 4)


def model_run(frames, flows: np.ndarray, flags: int, out_size: int):
    """(out, rec): the whole buffer the calls must leave from one of canary
    bytes, and the records."""
    out = np.full(out_size, CANARY, dtype=np.uint8)
    rec = np.zeros(len(frames), dtype=lvlip.LRO_REC_DTYPE)
    for i, fr in enumerate(frames):
        fr = bytes(fr)
        k, rel, dlen, st, tf, ack, p = model_rec(fr, flows, flags)
        rec[i] = (k, rel, dlen, st, tf, ack)
        if st == lvlip.LRO_PLACED:
            o = int(flows[k]["out_off"]) + rel
            out[o:o + dlen] = np.frombuffer(fr[p:p + dlen], dtype=np.uint8)
    return out, rec


def model_advance(flows: np.ndarray, rec: np.ndarray):
    """Per flow (delivered, placed, [(left, right), ...] at most 4)."""
    res = []
    for k, f in enumerate(flows):
        iv = sorted((int(r["rel"]), int(r["rel"]) + int(r["dlen"])) for r in rec
                    if r["status"] == lvlip.LRO_PLACED and r["flow"] == k)
        merged = []
        for lo, hi in iv:
            if merged and lo <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], hi)
            else:
                merged.append([lo, hi])
        delivered = merged[0][1] if merged and merged[0][0] == 0 else 0
        isl = [m for m in merged if m[0] != 0][:4]
        nxt = int(f["rcv_nxt"])
        res.append((delivered, len(iv), [((nxt + lo) & 0xFFFFFFFF, (nxt + hi) & 0xFFFFFFFF) for lo, hi in isl]))
    return res


def result_tuples(res: np.ndarray):
    return [(int(r["delivered"]), int(r["placed"]), [tuple(int(v) for v in r["sack"][j]) for j in range(r["nsack"])])
            for r in res]


# --------------------------------------------------------------- the cases --

def plan_flows(nflows: int, wnd: int, omod: int, rcv_nxt0: int = 0xFFFFFF00) -> np.ndarray:
    """nflows planned flows, each owning `wnd` bytes of out that start at
    omod mod 16, a canary gap between neighbours; flow of user cookie 0 wraps
    its sequence space."""
    fl = np.concatenate([lvlip.lro_flow(PEER if u % 3 else bytes((10, 0, 1, u % 256)), ME, 40001 + 7 * u,
                                        8000 + (u & 1), (rcv_nxt0 + 0x01010101 * u) & 0xFFFFFFFF, wnd,
                                        out_off=16 * (1 + u * (wnd // 16 + 3)) + omod, user=u)
                         for u in range(nflows)])
    lvlip.lro_plan(fl)
    return fl


def flow_kw(flow) -> dict:
    """tcp_frame's address and port arguments for a frame of this flow."""
    return dict(sport=_bswap16(int(flow["sport"])), dport=_bswap16(int(flow["dport"])),
                saddr=struct.pack("<I", int(flow["saddr"])), daddr=struct.pack("<I", int(flow["daddr"])))


def specials(flow: np.ndarray, stream: np.ndarray):
    """Every status and edge the header names, on one flow whose stream bytes
    are `stream` (rcv_wnd of them): (name, frame)."""
    nxt, wnd = int(flow["rcv_nxt"]), int(flow["rcv_wnd"])
    kw = flow_kw(flow)
    seg = lambda rel, n: stream[rel:rel + n].tobytes()  # noqa: E731
    rng = np.random.default_rng(5)
    sp = [("edge_met", tcp_frame(seg(wnd - 37, 37), nxt + wnd - 37, **kw)),
          ("edge_over", tcp_frame(seg(wnd - 37, 37) + b"\x00", nxt + wnd - 37, **kw)),
          ("old", tcp_frame(b"old data", nxt - 100, **kw)),                      # rel >= 2^31
          ("far", tcp_frame(b"far", nxt + 0x80000000, **kw)),
          ("hl8", tcp_frame(seg(700, 33), nxt + 700, hl=8, **kw)),
          ("hl15", tcp_frame(seg(740, 90), nxt + 740, hl=15, **kw)),
          ("ihl6", tcp_frame(seg(900, 61), nxt + 900, ihl=6, **kw)),
          ("ihl6_hl8", tcp_frame(seg(961, 17), nxt + 961, ihl=6, hl=8, **kw)),
          ("syn", tcp_frame(seg(1000, 8), nxt + 1000, flags=0x02, **kw)),
          ("rst", tcp_frame(b"", nxt, flags=0x14, **kw)),
          ("urg", tcp_frame(seg(1000, 8), nxt + 1000, flags=0x30, urp=3, **kw)),
          ("pure_ack", tcp_frame(b"", nxt + 5, **kw)),
          ("fin_data", tcp_frame(seg(1100, 29), nxt + 1100, flags=0x11, **kw)),
          ("no_flow", tcp_frame(b"nobody", nxt, **dict(kw, sport=9))),
          ("hl4", tcp_frame(seg(0, 8), nxt, hl_field=4, **kw)),
          ("hl_past", tcp_frame(b"", nxt, hl_field=9, **kw)),
          ("bad_l4", tcp_frame(seg(1200, 77), nxt + 1200, l4_ok=False, **kw)),
          ("cut", tcp_frame(seg(1300, 64), nxt + 1300, **kw)[:-9]),              # ip.len beyond the frame
          ("not_ip", ETH[:12] + b"\x08\x06" + bytes(40)), ("runt", ETH + bytes(11))]
    sp += [("icmp_" + k, ref_rx_cases.echo_frame(k, rng, i)) for i, k in enumerate(ref_rx_cases.KINDS)]
    return sp


class Case:
    """n frames over nflows flows: ragged in-window segments in shuffled order
    with duplicates and partial overlaps (every payload byte is its stream's
    byte at that place, as TCP requires), and the special frames between
    them."""
    WND = 4096

    def __init__(self, n: int, nflows: int, seed: int = 0):
        rng = np.random.default_rng(1000 * n + nflows + seed)
        self.n, self.nflows = n, nflows
        self.flows0 = plan_flows(nflows, self.WND, 0)
        self.streams = [rng.integers(0, 256, self.WND, dtype=np.uint8) for _ in range(nflows)]
        pool = []
        for k, f in enumerate(self.flows0):
            kw = flow_kw(f)
            pos = 0
            while pos < 3000 and len(pool) < 2 * n:
                dlen = int(rng.choice((1, 2, 15, 16, 17, 31, 100, 536, 1460)))
                dlen = min(dlen, 3000 - pos)
                pool.append(tcp_frame(self.streams[k][pos:pos + dlen].tobytes(), int(f["rcv_nxt"]) + pos, **kw))
                if rng.random() < 0.2:  # a retransmit that overlaps its neighbours partially
                    lo = max(0, pos - int(rng.integers(0, 9)))
                    pool.append(tcp_frame(self.streams[k][lo:lo + dlen + 5].tobytes(), int(f["rcv_nxt"]) + lo, **kw))
                pos += dlen if rng.random() < 0.9 else dlen + 40  # a hole now and then
        pool += [fr for _, fr in specials(self.flows0[0], self.streams[0])]
        order = rng.permutation(len(pool))
        if n < len(pool):  # small batches: segments first, a few specials
            order = np.concatenate([order[:n - n // 4], rng.permutation(np.arange(len(pool) - 28, len(pool)))[:n // 4]])
        self.frames = [pool[int(i)] for i in order[:n]]
        while len(self.frames) < n:
            self.frames.append(self.frames[int(rng.integers(0, len(self.frames)))])  # duplicates

    def laid_out(self, fmod: int, omod: int):
        """(buffer, fd, flows, out_size): every frame at fmod mod 16, every
        flow's bytes at omod mod 16."""
        offs, pos = [], 0
        for fr in self.frames:
            pos = (pos + 15 & ~15) + fmod
            offs.append(pos)
            pos += len(fr)
        buf = np.zeros((pos + 15 & ~15) + 16, dtype=np.uint8)
        fd = np.zeros(len(self.frames), dtype=lvlip.FRAME_DESC_DTYPE)
        for i, (o, fr) in enumerate(zip(offs, self.frames)):
            buf[o:o + len(fr)] = np.frombuffer(fr, dtype=np.uint8)
            fd[i] = (o, len(fr), 0)
        flows = self.flows0.copy()
        flows["out_off"] += omod
        return buf, fd, flows, lvlip.lro_plan(flows) + 32


@functools.lru_cache(maxsize=None)
def case(n: int, nflows: int) -> Case:
    return Case(n, nflows)


@functools.lru_cache(maxsize=None)
def expected(n: int, nflows: int, flags: int, omod: int):
    c = case(n, nflows)
    _, _, flows, out_size = c.laid_out(0, omod)
    return model_run(c.frames, flows, flags, out_size)


def assert_same_out(got: np.ndarray, want: np.ndarray, what: str) -> None:
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        b = int(np.flatnonzero(got != want)[0])
        pytest.fail(f"{what}: first difference at out byte {b}: got 0x{int(got[b]):02x}, want 0x{int(want[b]):02x}; "
                    f"{int((got != want).sum())} bytes differ")


def assert_same_rec(got: np.ndarray, want: np.ndarray, what: str) -> None:
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        pytest.fail(f"{what}: record {i}: got {got[i]}, want {want[i]}")


@functools.lru_cache(maxsize=None)
def fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def fixture_inputs():
    """The reference's segments as one batch: frames, and the flow with the
    rcv_nxt the reference had when the first of them arrived."""
    fx = fixture()
    frames = [bytes.fromhex(h) for h in fx["frames"]]
    f0 = frames[0]
    flow = lvlip.lro_flow(f0[26:30], f0[30:34], *struct.unpack_from("!HH", f0, 34), fx["rcv_nxt"], 8192, out_off=3)
    lvlip.lro_plan(flow)
    buf, fd = lvlip.pack_frames(frames, align_mod=16, seed=4)
    return fx, buf, fd, flow


def tso_round_trip_inputs(mss: int, seed: int = 0):
    """A payload cut by lvlip_tso_cpu, its frames shuffled and some twice:
    (payload, frame buffer, fd, planned flow)."""
    rng = np.random.default_rng(mss + seed)
    length = {1: 40, 15: 200, 16: 200, 17: 200}.get(mss, 5 * mss + 3)
    payload = rng.integers(0, 256, length, dtype=np.uint8)
    hdr = tso_template(seq=0xFFFFFF00)
    sends = lvlip.tso_send(hdr, 0, length, mss, out_off=5, stride=54 + mss + 3)
    buf, fd = lvlip.tso_cpu(payload, sends)
    order = rng.permutation(fd.size)
    order = np.concatenate([order, order[:max(1, fd.size // 3)]])
    flow = lvlip.lro_flow(hdr[26:30], hdr[30:34], 40001, 8000, 0xFFFFFF00, 1 << 16, out_off=7)
    lvlip.lro_plan(flow)
    buf = np.concatenate([buf, np.zeros(32, dtype=np.uint8)])
    return payload, buf, np.ascontiguousarray(fd[order]), flow


# --------------------------------------------------------------- the tests --

def test_layout():
    assert lvlip.LRO_FLOW_DTYPE.itemsize == 48 and lvlip.LRO_FLOW_DTYPE.fields["out_off"][1] == 24
    assert lvlip.LRO_REC_DTYPE.itemsize == 16 and lvlip.LRO_REC_DTYPE.fields["status"][1] == 10
    assert lvlip.LRO_RESULT_DTYPE.itemsize == 48
    assert lvlip.lib().lvlip_abi_version() == 2


@pytest.mark.parametrize("flags", (0, lvlip.RX_VERIFY_L4))
@pytest.mark.parametrize("nflows", FLOW_COUNTS)
@pytest.mark.parametrize("n", N_LIST)
def test_lro_cpu_equals_model(n, nflows, flags):
    c = case(n, nflows)
    for fmod, omod in ((0, 0), (1, 7), (6, 15), (15, 1)):
        buf, fd, flows, out_size = c.laid_out(fmod, omod)
        want_out, want_rec = expected(n, nflows, flags, omod)
        out = np.full(out_size, CANARY, dtype=np.uint8)
        before = buf.copy()
        out, rec = lvlip.lro_cpu(buf, fd, flows, flags, out=out)
        assert_same_rec(rec, want_rec, f"n {n}, {nflows} flows, flags {flags}")
        assert_same_out(out, want_out, f"n {n}, {nflows} flows, flags {flags}, frames at {fmod}, out at {omod}")
        assert np.array_equal(buf, before), "the frames are only read"
        assert result_tuples(lvlip.lro_advance(flows, rec)) == model_advance(flows, want_rec)


def test_every_special_gets_its_status():
    """The edge cases by name: the model's status for each is what the header
    says, and the CPU form agrees."""
    flows = plan_flows(1, Case.WND, 0)
    stream = np.random.default_rng(2).integers(0, 256, Case.WND, dtype=np.uint8)
    sp = specials(flows[0], stream)
    L = lvlip
    want = {"edge_met": (1, 1), "edge_over": (21, 21), "old": (21, 21), "far": (21, 21), "hl8": (1, 1),
            "hl15": (1, 1), "ihl6": (1, 1), "ihl6_hl8": (1, 1), "syn": (19, 19), "rst": (19, 19), "urg": (19, 19),
            "pure_ack": (20, 20), "fin_data": (1, 1), "no_flow": (18, 18), "hl4": (17, 17), "hl_past": (17, 17),
            "bad_l4": (1, L.RX_BAD_L4), "cut": (17, L.RX_SHORT), "not_ip": (2, 2), "runt": (3, 3),
            "icmp_ok": (16, 16), "icmp_ok_options": (16, 16), "icmp_ip_csum": (7, 7), "icmp_version": (4, 4),
            "icmp_ihl": (5, 5), "icmp_ttl0": (6, 6), "icmp_proto": (9, 9), "icmp_icmp_csum": (16, L.RX_BAD_L4)}
    assert set(want) == {name for name, _ in sp}
    buf, fd = lvlip.pack_frames([fr for _, fr in sp], align_mod=16, seed=3)
    for j, flags in enumerate((0, lvlip.RX_VERIFY_L4)):
        _, rec = lvlip.lro_cpu(buf, fd, flows, flags)
        for (name, fr), r in zip(sp, rec):
            assert model_rec(fr, flows, flags)[3] == want[name][j], name
            assert int(r["status"]) == want[name][j], name
    old = model_rec(dict(sp)["old"], flows, 0)
    assert old[1] == 0x100000000 - 100 and old[1] >= 1 << 31
    ack = rec[[name for name, _ in sp].index("pure_ack")]
    assert (int(ack["rel"]), int(ack["dlen"]), int(ack["ack_seq"]), int(ack["flow"])) == (5, 0, 0x01020304, 0)


@pytest.mark.parametrize("flags", (0, lvlip.RX_VERIFY_L4))
def test_ip_rcv_statuses_are_rx_verify_cpus(flags):
    """Every record with status 2-9 carries lvlip_rx_verify_cpu's verdict for
    the same flags; every other frame is one it keeps."""
    frs, _ = ref_rx_cases.frames(seed=11, per_kind=6)
    flows = plan_flows(1, Case.WND, 0)
    frs += [bytearray(fr) for _, fr in specials(flows[0], np.zeros(Case.WND, dtype=np.uint8))]
    buf, fd = lvlip.pack_frames(frs, align_mod=16, seed=9)
    _, rec = lvlip.lro_cpu(buf, fd, flows, flags)
    verdict = lvlip.rx_verify_cpu(frs, flags)
    seen = set()
    for r, v in zip(rec, verdict):
        if 2 <= int(r["status"]) <= 9:
            assert int(r["status"]) == int(v)
            seen.add(int(v))
        else:
            assert int(v) == lvlip.RX_OK
    assert seen == {2, 3, 4, 5, 6, 7, 9} | ({8} if flags else set())


@pytest.mark.parametrize("mss", (1, 15, 16, 17, 536, 1460, 8946))
def test_round_trip_with_tso(mss):
    payload, buf, fd, flow = tso_round_trip_inputs(mss)
    out = np.full((1 << 16) + 64, CANARY, dtype=np.uint8)
    out, rec = lvlip.lro_cpu(buf, fd, flow, lvlip.RX_VERIFY_L4, out=out)
    assert (rec["status"] == lvlip.LRO_PLACED).all()
    res = lvlip.lro_advance(flow, rec)[0]
    assert int(res["delivered"]) == payload.size and int(res["nsack"]) == 0 and int(res["placed"]) == fd.size
    assert np.array_equal(out[7:7 + payload.size], payload)
    assert (out[:7] == CANARY).all() and (out[7 + payload.size:] == CANARY).all()


def test_missing_middle_segment_gives_prefix_and_one_island():
    payload, buf, fd, flow = tso_round_trip_inputs(536)
    keep = np.array([d for d in fd if int(d["offset"]) != 5 + 2 * (54 + 536 + 3)], dtype=fd.dtype)  # segment 2 lost
    out, rec = lvlip.lro_cpu(buf, keep, flow)
    res = lvlip.lro_advance(flow, rec)[0]
    assert int(res["delivered"]) == 2 * 536 and int(res["nsack"]) == 1
    left, right = (int(v) for v in res["sack"][0])
    assert left == (0xFFFFFF00 + 3 * 536) & 0xFFFFFFFF and right == (0xFFFFFF00 + payload.size) & 0xFFFFFFFF
    assert np.array_equal(out[7:7 + 1072], payload[:1072]) and np.array_equal(out[7 + 1608:7 + payload.size],
                                                                              payload[1608:])
    assert not out[7 + 1072:7 + 1608].any()  # the hole keeps the buffer's bytes


def test_more_than_four_islands_reports_the_first_four():
    flows = plan_flows(1, Case.WND, 0)
    nxt = int(flows[0]["rcv_nxt"])
    frs = [tcp_frame(b"ab", nxt + 10 * k, **flow_kw(flows[0])) for k in (6, 2, 5, 1, 3, 4)]
    buf, fd = lvlip.pack_frames(frs, align_mod=16, seed=1)
    _, rec = lvlip.lro_cpu(buf, fd, flows)
    res = lvlip.lro_advance(flows, rec)
    assert result_tuples(res) == model_advance(flows, rec)
    assert int(res[0]["delivered"]) == 0 and int(res[0]["nsack"]) == 4
    assert [int(v) for v in res[0]["sack"][:, 0]] == [(nxt + 10 * k) & 0xFFFFFFFF for k in (1, 2, 3, 4)]


def test_lro_cpu_reproduces_the_reference_stream():
    """What tcp_data_queue + tcp_data_dequeue of the unmodified stack returned
    for 7 segments of 536 B arriving as 0, 2, 1, 1, 4, 3, 6."""
    fx, buf, fd, flow = fixture_inputs()
    assert fx["order"] == [0, 2, 1, 1, 4, 3, 6] and fx["count"] == 5 * 536
    out, rec = lvlip.lro_cpu(buf, fd, flow, lvlip.RX_VERIFY_L4)
    res = lvlip.lro_advance(flow, rec)[0]
    assert int(res["delivered"]) == fx["count"]
    assert out[3:3 + fx["count"]].tobytes().hex() == fx["dequeued_hex"]
    assert int(res["nsack"]) == 1 and int(res["sack"][0][0]) == (fx["rcv_nxt"] + 6 * 536) & 0xFFFFFFFF


def _refusals():
    def two():
        return np.concatenate([lvlip.lro_flow(PEER, ME, 1, 2, 0, 100, out_off=0),
                               lvlip.lro_flow(PEER, ME, 1, 3, 0, 100, out_off=100)])
    cases = {}
    for name, field, value in (("wnd0", "rcv_wnd", 0), ("wnd_big", "rcv_wnd", (1 << 30) + 1), ("reserved", "reserved", 1),
                               ("dup_key", "dport", 0x0200), ("overlap", "out_off", 99)):
        f = two()
        f[1][field] = value
        cases[name] = f
    f = two()
    f["pad"][1][7] = 1
    cases["pad"] = f
    return cases


@pytest.mark.parametrize("name", sorted(_refusals()))
def test_plan_refusals(name):
    L = lvlip.lib()
    f = _refusals()[name]
    before = f.copy()
    ob = ctypes.c_uint64(7)
    assert L.lvlip_lro_plan(f.ctypes.data, f.size, ctypes.byref(ob)) == 0xFFFFFFFF and ob.value == 0
    assert np.array_equal(f, before), "a refused plan leaves the flows as they were"
    with pytest.raises(ValueError):
        lvlip.lro_plan(f)


def test_plan_sorts_and_sizes():
    L = lvlip.lib()
    fl = plan_flows(17, 1000, 3)
    keys = [f.tobytes()[:12] for f in fl]
    assert keys == sorted(keys) and sorted(fl["user"].tolist()) == list(range(17))
    assert lvlip.lro_plan(fl) == max(int(f["out_off"]) + 1000 for f in fl)
    big = np.zeros(65537, dtype=lvlip.LRO_FLOW_DTYPE)
    big["rcv_wnd"], big["out_off"], big["sport"] = 1, np.arange(65537), np.arange(65537) & 0xFFFF
    big["saddr"] = np.arange(65537) >> 16
    assert L.lvlip_lro_plan(big.ctypes.data, 65537, None) == 0xFFFFFFFF
    assert L.lvlip_lro_plan(big.ctypes.data, 65536, None) == 65536
    edge = lvlip.lro_flow(PEER, ME, 1, 2, 0, 1 << 30)
    assert lvlip.lro_plan(edge) == 1 << 30
    assert L.lvlip_lro_plan(None, 0, None) == 0


def test_cpu_and_dev_refusals_without_gpu():
    """Refused before anything is written, and for the device form before any
    HIP call, so this runs without a device."""
    L = lvlip.lib()
    c = case(16, 3)
    buf, fd, flows, out_size = c.laid_out(0, 0)
    out = np.full(out_size, CANARY, dtype=np.uint8)
    rec = np.full(16, 0x5A5A, dtype=lvlip.LRO_REC_DTYPE)
    b, d, f, o, r = (a.ctypes.data for a in (buf, fd, flows, out, rec))
    for args in ((None, d, 16, f, 3, 0, o, r), (b, None, 16, f, 3, 0, o, r), (b, d, 16, None, 3, 0, o, r),
                 (b, d, 16, f, 3, 0, None, r), (b, d, 16, f, 3, 0, o, None), (b, d, 16, f, 3, 2, o, r),
                 (b, d, 0xFFFFFFF1, f, 3, 0, o, r), (b, d, 16, f, 65537, 0, o, r)):
        assert L.lvlip_lro_cpu(*args) == lvlip.EINVAL
        assert L.lvlip_lro_dev(*args, None) == lvlip.EINVAL
    unsorted = np.ascontiguousarray(flows[::-1])
    assert L.lvlip_lro_cpu(b, d, 16, unsorted.ctypes.data, 3, 0, o, r) == lvlip.EINVAL
    assert (out == CANARY).all() and (rec["dlen"] == 0x5A5A).all()
    assert L.lvlip_lro_cpu(None, None, 0, None, 0, 0, None, None) == lvlip.OK
    assert L.lvlip_lro_dev(None, None, 0, None, 0, 0, None, None, None) == lvlip.OK
    # no flows at all: every TCP frame is NO_FLOW, nothing is written
    _, rec0 = lvlip.lro_cpu(buf, fd, flows[:0], 0, out=out)
    assert (out == CANARY).all() and not (rec0["status"] == lvlip.LRO_PLACED).any()
    assert (rec0["status"] == lvlip.LRO_NO_FLOW).any()


def test_example_under_sanitizers(tmp_path):
    """examples/lro_stream.c (its own main: TSO frames, shuffled, coalesced
    and advanced on the CPU forms, buffers malloc'd at exactly the planned
    sizes) compiled with the library's C sources under ASan + UBSan, and run
    as a program."""
    exe = tmp_path / "lro_stream_san"
    src = [os.path.join(ROOT, "examples", "lro_stream.c")] + [
        os.path.join(ROOT, "level-ip_amd", "csrc", f) for f in ("rcv_cpu.c", "seg_cpu.c", "csum_cpu.c")]
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "include"), *src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lro_stream ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_kernel_uses_no_scratch(tmp_path):
    """k_lro keeps a segment's first sweeps in registers until the verdict;
    that must not spill: both instantiations have a private segment of 0."""
    asm = tmp_path / "rcv_kernels.s"
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    "-S", "--cuda-device-only", os.path.join(ROOT, "level-ip_amd", "csrc", "rcv_kernels.hip"),
                    "-o", str(asm)], check=True, capture_output=True)
    text = asm.read_text()
    kernels = re.findall(r"\.name:\s+(\S*k_lro\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(kernels) == 2, kernels
    assert all(int(size) == 0 for _, size in kernels), kernels
