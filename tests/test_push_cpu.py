"""The write queue (include/lvlip_skb.h: lvlip_push_plan, lvlip_push_cpu)
without a GPU: the bindings, the reference's tcp_send frames, an independent
model of steps 1-4 for every output byte, rounds of push / ACK / step until the
ring has wrapped three times, the refusals of the plan and of both calls, the
whole loop with loss on the CPU forms with a ring of 16 slots per flow, a
sanitizer build of examples/push_loop.c and the kernels' scratch size.
tests/test_push_gpu.py shares the model's cases and the loop.

The model (model_push) restates the header's text with Python integers; the
bytes of a frame are those lvlip_tso_cpu writes for the send the header names,
with the three template fields the model itself puts in place."""
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import lvlip
from test_tso_cpu import fixture, template

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
CANARY = 0xA5
NO_LIMIT = lvlip.PUSH_NO_LIMIT
FD = lvlip.FRAME_DESC_DTYPE


# ---------------------------------------------------------------- the cases --

class PushCase:
    """Everything one lvlip_push_* call reads and writes."""

    def __init__(self, f, lro, snd, w, payload, ring, fd, sacked):
        self.f, self.lro, self.snd, self.w = f, lro, snd, w
        self.payload, self.ring, self.fd, self.sacked = payload, ring, fd, sacked
        self.nslots, self.ring_bytes, self.nfd = lvlip.push_plan(self.w, self.snd)

    def copy(self):
        c = object.__new__(PushCase)
        for k, v in self.__dict__.items():
            setattr(c, k, v.copy() if isinstance(v, np.ndarray) else v)
        return c


def make_case(specs, seed=0, with_lro=True, with_sacked=True, ring_mod=3, pay_mod=5, odd_stride=True, gap=2) -> PushCase:
    """specs: one dict per flow with mss, cap, nseg, shift (seg0 - q0), slot_nxt,
    push, unsent, span, wnd, una.  Regions and ring ranges are laid out one
    behind the other with canary gaps; the queue's entries and the scoreboard
    hold recognisable bytes."""
    rng = np.random.default_rng(seed)
    n = len(specs)
    f = np.zeros(n, dtype=lvlip.LRO_FLOW_DTYPE)
    f["rcv_nxt"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    f["rcv_nxt"][0] = 0xFFFFFFF0  # rcv_nxt + delivered wraps
    lro = None
    if with_lro:
        lro = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
        lro["delivered"] = rng.integers(0, 100000, n)
    snd = np.zeros(n, dtype=lvlip.SND_FLOW_DTYPE)
    w = np.zeros(n, dtype=lvlip.PUSH_FLOW_DTYPE)
    q, ro, po = gap, 16 + ring_mod, pay_mod
    for k, sp in enumerate(specs):
        mss, cap = sp["mss"], sp["cap"]
        stride = 54 + mss + (2 * (k % 3) + 1 if odd_stride else 0)
        w[k] = lvlip.push_flow(template(sport=40000 + k, seq=0x11223344, ack=0x55667788, win=0x99AA),
                               po, sp["unsent"], mss, ro, cap, q, sp["push"], stride=stride, wnd=sp["wnd"],
                               slot_nxt=sp["slot_nxt"])[0]
        snd[k]["snd_una"] = sp["una"]
        snd[k]["snd_nxt"] = (sp["una"] + sp["span"]) & M32
        snd[k]["seg0"], snd[k]["nseg"] = q + sp["shift"], sp["nseg"]
        snd[k]["win"], snd[k]["rtx"] = (1000 + 257 * k) & 0xFFFF, k % 3
        q += cap + gap
        ro += cap * stride + 7
        po += sp["unsent"] + 3
    payload = rng.integers(0, 256, po + 16, dtype=np.uint8)
    ring = np.full(ro + 64, CANARY, dtype=np.uint8)
    fd = np.zeros(q, dtype=FD)
    fd["offset"], fd["len"], fd["reserved"] = np.arange(q) * 1000 + 1, np.arange(q) + 60, 0xC0FFEE
    sacked = (rng.integers(0, 2, q, dtype=np.uint8) | 0x40) if with_sacked else None  # 0x40: a byte no call writes
    if with_sacked:
        for k in range(n):
            a = int(snd[k]["seg0"])
            sacked[a:a + int(snd[k]["nseg"])] &= 1
    return PushCase(f, lro, snd, w, payload, ring, fd, sacked)


def random_specs(nflows: int, seed: int, mss_list=(1, 7, 536, 1460), cap_list=(1, 2, 5, 64)):
    rng = np.random.default_rng(1000 + seed)
    specs = []
    for k in range(nflows):
        mss, cap = int(rng.choice(mss_list)), int(rng.choice(cap_list))
        nseg = int(rng.integers(0, cap + 1))
        shift = int(rng.integers(0, cap - nseg + 1))
        unsent = int(rng.choice([0, 1, mss, 3 * mss + (mss > 1), 5 * mss - 1, 70 * mss + 3]))
        span = int(rng.integers(0, 4 * mss + 1))
        wnd = int(rng.choice([0, span, max(span - 1, 0), span + mss - 1, span + 2 * mss + mss // 2, span + unsent,
                              NO_LIMIT]))
        push = int(rng.choice([0, 1, 3, cap, cap + 5]))
        una = int(rng.choice([int(rng.integers(0, 1 << 32)), M32 - int(rng.integers(0, 3 * mss + 1))]))
        specs.append(dict(mss=mss, cap=cap, nseg=nseg, shift=shift, slot_nxt=int(rng.integers(0, cap)), push=push,
                          unsent=unsent, span=span, wnd=wnd, una=una))
    return specs


def edge_specs():
    """The cases the header names, one flow each."""
    base = dict(mss=536, cap=5, nseg=0, shift=0, slot_nxt=0, push=5, unsent=3 * 536 + 1, span=0, wnd=NO_LIMIT, una=77)
    e = lambda **kw: dict(base, **kw)  # noqa: E731
    return [e(), e(unsent=0), e(unsent=1), e(mss=1, unsent=3), e(mss=7, unsent=20, push=9),
            e(wnd=2 * 536), e(wnd=2 * 536 + 535), e(wnd=0), e(span=100, wnd=99), e(span=100, wnd=100 + 4 * 536),
            e(push=0), e(cap=1, unsent=5000), e(cap=2, slot_nxt=1, push=2), e(cap=5, slot_nxt=4, push=3),
            e(cap=64, nseg=60, shift=4, slot_nxt=63, push=9, unsent=64 * 536), e(nseg=5, push=2),
            e(nseg=3, shift=2, push=0), e(nseg=2, shift=3, unsent=0),
            e(una=M32 - 600, span=300, unsent=2000), e(mss=1460, unsent=1460 * 4, cap=64, push=70),
            e(wnd=NO_LIMIT, span=NO_LIMIT - 536, unsent=2 * 536)]


CASES = [pytest.param(lambda n=n, s=s: make_case(random_specs(n, s), seed=s), id=f"random{n}-{s}")
         for n in (1, 3, 17) for s in (0, 1, 2, 3)] + [
    pytest.param(lambda: make_case(edge_specs(), seed=9), id="edges"),
    pytest.param(lambda: make_case(edge_specs(), seed=10, with_sacked=False), id="edges-no-sacked"),
    pytest.param(lambda: make_case(random_specs(17, 5), seed=5, with_lro=False), id="random17-no-lro"),
    pytest.param(lambda: make_case(random_specs(17, 6), seed=6, with_lro=False, with_sacked=False), id="random17-neither")]


# ---------------------------------------------------------------- the model --

def model_count(w, s):
    span = (int(s["snd_nxt"]) - int(s["snd_una"])) & M32
    mss, unsent = int(w["mss"]), int(w["unsent"])
    best = 0
    top = min(int(w["cap"]) - int(s["nseg"]), int(w["push"]), -(-unsent // mss))
    for m in range(top + 1):  # the largest count the four conditions allow
        if span + min(m * mss, unsent) <= int(w["wnd"]):
            best = m
    return best, min(best * mss, unsent)


def model_push(c: PushCase):
    """Steps 1-4 on copies: dict of every output."""
    c = c.copy()
    fd_out = np.zeros(c.nslots, dtype=FD)
    res = np.zeros(c.w.size, dtype=lvlip.PUSH_RESULT_DTYPE)
    for k in range(c.w.size):
        w, s = c.w[k], c.snd[k]
        q0, seg0, nseg = int(w["q0"]), int(s["seg0"]), int(s["nseg"])
        moved = 0
        if seg0 != q0:
            c.fd[q0:q0 + nseg] = c.fd[seg0:seg0 + nseg].copy()
            if c.sacked is not None:
                c.sacked[q0:q0 + nseg] = c.sacked[seg0:seg0 + nseg].copy()
            s["seg0"], moved = q0, nseg
        m, nbytes = model_count(w, s)
        if m:
            hdr = bytearray(w["hdr"].tobytes())
            delivered = int(c.lro[k]["delivered"]) if c.lro is not None else 0
            struct.pack_into("!II", hdr, 38, int(s["snd_nxt"]), (int(c.f[k]["rcv_nxt"]) + delivered) & M32)
            struct.pack_into("!H", hdr, 48, int(s["win"]))
            send = lvlip.tso_send(bytes(hdr), int(w["pay_off"]), int(w["unsent"]), int(w["mss"]))
            lvlip.tso_plan(send)
            frames, tfd = lvlip.tso_cpu(c.payload, send)
            for i in range(m):
                o, ln = int(tfd[i]["offset"]), int(tfd[i]["len"])
                at = int(w["ring_off"]) + ((int(w["slot_nxt"]) + i) % int(w["cap"])) * int(w["stride"])
                c.ring[at:at + ln] = frames[o:o + ln]
                fd_out[int(w["slot0"]) + i] = (at, ln, 0)
                c.fd[q0 + nseg + i] = (at, ln, 0)
                if c.sacked is not None:
                    c.sacked[q0 + nseg + i] = 0
        res[k] = (m, nbytes, q0 + nseg, moved)
        s["nseg"] = nseg + m
        s["snd_nxt"] = (int(s["snd_nxt"]) + nbytes) & M32
        w["pay_off"] = int(w["pay_off"]) + nbytes
        w["unsent"] = int(w["unsent"]) - nbytes
        w["slot_nxt"] = (int(w["slot_nxt"]) + m) % int(w["cap"])
    return dict(ring=c.ring, fd=c.fd, sacked=c.sacked, fd_out=fd_out, snd=c.snd, w=c.w, res=res)


def run_cpu(c: PushCase):
    c = c.copy()
    keep = (c.f.copy(), None if c.lro is None else c.lro.copy(), c.payload.copy())
    fd_out, res = lvlip.push_cpu(c.f, c.lro, c.snd, c.w, c.payload, c.ring, c.fd, c.sacked)
    assert c.f.tobytes() == keep[0].tobytes() and c.payload.tobytes() == keep[2].tobytes()
    assert c.lro is None or c.lro.tobytes() == keep[1].tobytes()
    return dict(ring=c.ring, fd=c.fd, sacked=c.sacked, fd_out=fd_out, snd=c.snd, w=c.w, res=res)


def assert_outputs(got: dict, want: dict, what: str = ""):
    for k in ("res", "snd", "w", "fd_out", "fd", "sacked", "ring"):
        if want[k] is None:
            assert got[k] is None
            continue
        g, x = np.ascontiguousarray(got[k]).view(np.uint8).reshape(-1), np.ascontiguousarray(want[k]).view(np.uint8).reshape(-1)
        if not np.array_equal(g, x):
            bad = np.flatnonzero(g != x)
            pytest.fail(f"{what}{k}: {bad.size} bytes differ, first at {int(bad[0])}")


# ---------------------------------------------------------------- the tests --

def test_bindings_and_layout():
    L = lvlip.lib()
    for name in ("lvlip_push_plan", "lvlip_push_cpu", "lvlip_push_dev"):
        assert getattr(L, name) is not None and name in lvlip.SIGNATURES
    t = lvlip.PUSH_FLOW_DTYPE
    assert t.itemsize == 112 and t.itemsize % 16 == 0 and t.fields["hdr"][1] % 4 == 0
    for name, (dt, off) in ((n, t.fields[n][:2]) for n in t.names if n not in ("hdr", "pad")):
        assert off % dt.itemsize == 0, name
    assert lvlip.PUSH_RESULT_DTYPE.itemsize == 16 and lvlip.PUSH_RESULT_DTYPE.names == ("pushed", "bytes", "first", "moved")
    assert L.lvlip_abi_version() == 2


def test_pushed_frames_are_the_references_tcp_send_frames():
    """Every send of tests/golden/tso_ref.json as one flow with an empty queue:
    the frames are the reference's, byte for byte, and lvlip_tso_cpu's."""
    fx = fixture()
    for k, snd_ref in enumerate(fx["sends"]):
        first = bytes.fromhex(snd_ref["frames"][0])
        hdr = bytearray(first[:54])
        hdr[47] |= 0x08
        seq, ack = struct.unpack_from("!II", hdr, 38)
        win, = struct.unpack_from("!H", hdr, 48)
        payload = np.frombuffer(bytes.fromhex(snd_ref["payload_hex"]), dtype=np.uint8)
        nseg = len(snd_ref["frames"])
        mss = fx["mss"]
        # the template's own three fields are ignored: they come from f and s
        tmpl = bytearray(hdr)
        struct.pack_into("!II", tmpl, 38, 0xDEADBEEF, 0xFEEDFACE)
        struct.pack_into("!H", tmpl, 48, 0x1234)
        w = lvlip.push_flow(bytes(tmpl), 0, snd_ref["len"], mss, 3, nseg + k, 1, nseg + 2, stride=54 + mss + 1)
        s = np.zeros(1, dtype=lvlip.SND_FLOW_DTYPE)
        s["snd_una"] = s["snd_nxt"] = seq
        s["seg0"], s["win"] = 1, win
        f = np.zeros(1, dtype=lvlip.LRO_FLOW_DTYPE)
        f["rcv_nxt"] = ack
        nslots, ring_bytes, nfd = lvlip.push_plan(w, s)
        ring, fd = np.full(ring_bytes, CANARY, dtype=np.uint8), np.zeros(nfd, dtype=FD)
        fd_out, res = lvlip.push_cpu(f, None, s, w, payload, ring, fd)
        assert int(res[0]["pushed"]) == nseg and int(res[0]["bytes"]) == snd_ref["len"]
        got = [ring[int(d["offset"]):int(d["offset"]) + int(d["len"])].tobytes().hex() for d in fd_out[:nseg]]
        assert got == snd_ref["frames"]
        send = lvlip.tso_send(bytes(hdr), 0, snd_ref["len"], mss)
        lvlip.tso_plan(send)
        tso, tfd = lvlip.tso_cpu(payload, send)
        assert got == [tso[int(d["offset"]):int(d["offset"]) + int(d["len"])].tobytes().hex() for d in tfd]
        assert not fd_out[nseg:]["len"].any() and np.array_equal(fd[1:1 + nseg], fd_out[:nseg])
        assert int(s[0]["nseg"]) == nseg and int(s[0]["snd_nxt"]) == (seq + snd_ref["len"]) & M32


@pytest.mark.parametrize("make", CASES)
def test_cpu_form_equals_the_model(make):
    c = make()
    assert_outputs(run_cpu(c), model_push(c))


def test_the_cases_cover_what_the_header_names():
    pushed, moved, cut, marks, wraps = 0, 0, 0, 0, 0
    for p in CASES:
        c = p.values[0]()
        want = model_push(c)
        pushed += int((want["res"]["pushed"] > 0).sum())
        moved += int((want["res"]["moved"] > 0).sum())
        need = -(-c.w["unsent"].astype(np.int64) // c.w["mss"])
        room = np.minimum(np.minimum(c.w["cap"].astype(np.int64) - c.snd["nseg"], c.w["push"]), need)
        cut += int(((want["res"]["pushed"] < room) & (want["res"]["pushed"] > 0)).sum())  # the window between segments
        if c.sacked is not None:
            marks += int(((c.snd["seg0"] > c.w["q0"]) & (c.snd["nseg"] > 0) & (want["res"]["pushed"] > 0)).sum())
        wraps += int(((c.w["slot_nxt"].astype(np.int64) + want["res"]["pushed"]) > c.w["cap"]).sum())
        assert c.nslots == int(c.w["push"].sum())
    assert pushed >= 40 and moved >= 20 and cut >= 5 and marks >= 5 and wraps >= 5, (pushed, moved, cut, marks, wraps)
    e = make_case(edge_specs(), seed=9)
    want = model_push(e)
    assert want["res"]["pushed"].tolist() == [4, 0, 1, 3, 3, 2, 2, 0, 0, 4, 0, 1, 2, 3, 4, 0, 0, 0, 4, 4, 1]
    assert int(want["snd"][18]["snd_nxt"]) < int(e.snd[18]["snd_nxt"])  # snd_nxt wrapped past 2^32
    assert int(want["w"][13]["slot_nxt"]) == 2 and int(want["w"][14]["slot_nxt"]) == 3  # the slots wrapped


def live_frames(c: PushCase, k: int):
    s = c.snd[k]
    return [(int(d["offset"]), c.ring[int(d["offset"]):int(d["offset"]) + int(d["len"])].tobytes())
            for d in c.fd[int(s["seg0"]):int(s["seg0"]) + int(s["nseg"])]]


def test_rounds_until_the_ring_has_wrapped_three_times():
    """push -> a synthetic ACK of some head segments -> lvlip_snd_next_cpu ->
    push: the queue's frames always carry consecutive stream bytes from snd_una
    on, and a push never touches a live frame."""
    rng = np.random.default_rng(3)
    specs = [dict(mss=7, cap=5, nseg=0, shift=0, slot_nxt=3, push=3, unsent=0, span=0, wnd=NO_LIMIT, una=M32 - 50),
             dict(mss=536, cap=2, nseg=0, shift=0, slot_nxt=0, push=2, unsent=0, span=0, wnd=3 * 536, una=5),
             dict(mss=1, cap=64, nseg=0, shift=0, slot_nxt=63, push=40, unsent=0, span=0, wnd=NO_LIMIT, una=9)]
    c = make_case(specs, seed=4)
    total = [7 * 23 + 3, 536 * 9 + 100, 64 * 4]
    c.payload = rng.integers(0, 256, sum(total) + 64, dtype=np.uint8)
    start = np.cumsum([5] + total[:-1])
    c.w["pay_off"] = start
    iss = c.snd["snd_una"].copy()
    given = [0, 0, 0]
    filled = np.zeros(3, dtype=np.int64)
    for rnd in range(200):
        for k in range(3):  # the application makes more bytes ready
            more = min(int(rng.integers(0, 4 * int(c.w[k]["mss"]) + 2)), total[k] - given[k])
            c.w[k]["unsent"] += more
            given[k] += more
        before = [live_frames(c, k) for k in range(3)]
        fd_out, res = lvlip.push_cpu(c.f, c.lro, c.snd, c.w, c.payload, c.ring, c.fd, c.sacked)
        filled += res["pushed"]
        sres = np.zeros(3, dtype=lvlip.SND_RESULT_DTYPE)
        for k in range(3):
            s = c.snd[k]
            now = live_frames(c, k)
            assert [b for _, b in now[:len(before[k])]] == [b for _, b in before[k]], "a live frame was overwritten"
            assert len({o for o, _ in now}) == len(now), "two entries share a slot"
            at = (int(s["snd_una"]) - int(iss[k])) & M32
            for _, fr in now:  # consecutive stream bytes from snd_una on
                assert struct.unpack_from("!I", fr, 38)[0] == (int(iss[k]) + at) & M32
                assert fr[54:] == c.payload[int(start[k]) + at:int(start[k]) + at + len(fr) - 54].tobytes()
                at += len(fr) - 54
            assert (int(iss[k]) + at) & M32 == int(s["snd_nxt"])
            p = int(rng.integers(0, int(s["nseg"]) + 1))
            acked = sum(len(fr) - 54 for _, fr in now[:p])
            sres[k]["popped"], sres[k]["acked"], sres[k]["snd_una"] = p, acked, (int(s["snd_una"]) + acked) & M32
        lvlip.snd_next_cpu(c.snd, sres)
        if (filled >= 3 * c.w["cap"] + 1).all() and given == total and not c.snd["nseg"].any() and not c.w["unsent"].any():
            break
    else:
        pytest.fail("the transfer did not finish")
    assert ((c.snd["snd_una"].astype(np.int64) - iss) & M32).tolist() == total and rnd > 10


# ------------------------------------------------------------ the refusals --

def plan_inputs():
    c = make_case(random_specs(3, 1, mss_list=(536,), cap_list=(5,)), seed=1)
    c.snd["seg0"], c.snd["nseg"] = c.w["q0"] + 1, 2
    lvlip.push_plan(c.w, c.snd)
    return c


def _set(field, k, v):
    def change(c):
        c.w[field][k] = v
    return change


def _hdr_byte(i, v):
    def change(c):
        c.w["hdr"][1][i] = v
    return change


def _snd(field, v):
    def change(c):
        c.snd[field][1] = v
    return change


def _overlap_q(c):
    c.w["q0"][2] = c.w["q0"][1] + 4


def _overlap_ring(c):
    c.w["ring_off"][2] = c.w["ring_off"][1] + 4 * int(c.w["stride"][1]) + 100


PLAN_REFUSALS = {
    "ethertype": _hdr_byte(12, 0x86), "version/ihl": _hdr_byte(14, 0x46), "protocol": _hdr_byte(23, 17),
    "TCP header length": _hdr_byte(46, 0x60), "FIN": _hdr_byte(47, 0x11), "SYN": _hdr_byte(47, 0x12),
    "RST": _hdr_byte(47, 0x14), "URG": _hdr_byte(47, 0x30),
    "cap 0": _set("cap", 1, 0), "slot_nxt == cap": _set("slot_nxt", 1, 5), "mss 0": _set("mss", 1, 0),
    "mss above 65495": _set("mss", 1, 65496), "stride below 54 + mss": _set("stride", 1, 54 + 535),
    "unsent above 2^30": _set("unsent", 1, NO_LIMIT + 1), "wnd above 2^30": _set("wnd", 1, NO_LIMIT + 1),
    "reserved": _set("reserved", 1, 1), "pad": lambda c: c.w["pad"][1].__setitem__(5, 1),
    "fd regions overlap": _overlap_q, "ring ranges overlap": _overlap_ring,
    "queue starts below q0": _snd("seg0", 0), "queue ends beyond q0 + cap": _snd("nseg", 5),
    "region passes 2^32": _set("q0", 1, M32 - 3),
}


@pytest.mark.parametrize("what", sorted(PLAN_REFUSALS))
def test_plan_refusals_leave_w_unwritten(what):
    c = plan_inputs()
    c.w["slot0"] = 0xABCD  # the plan would overwrite it
    PLAN_REFUSALS[what](c)
    keep = c.w.copy()
    with pytest.raises(ValueError):
        lvlip.push_plan(c.w, c.snd)
    assert c.w.tobytes() == keep.tobytes()
    rb, nfd = lvlip._U64(7), lvlip._U32(7)
    assert lvlip.lib().lvlip_push_plan(c.w.ctypes.data, c.snd.ctypes.data, 3, rb, nfd) == M32
    assert (rb.value, nfd.value) == (0, 0)


def test_plan_limits_and_sizes():
    L = lvlip.lib()
    c = plan_inputs()
    keep = c.w.copy()
    assert L.lvlip_push_plan(c.w.ctypes.data, c.snd.ctypes.data, 65537, None, None) == M32
    assert L.lvlip_push_plan(None, c.snd.ctypes.data, 3, None, None) == M32
    assert L.lvlip_push_plan(c.w.ctypes.data, None, 3, None, None) == M32
    assert L.lvlip_push_plan(None, None, 0, None, None) == 0
    c.w["push"] = 0x7FFFFFFF  # the total passes LVLIP_MAX_BATCH
    keep = c.w.copy()
    assert L.lvlip_push_plan(c.w.ctypes.data, c.snd.ctypes.data, 3, None, None) == M32
    assert c.w.tobytes() == keep.tobytes()
    c = plan_inputs()
    nslots, ring_bytes, nfd = lvlip.push_plan(c.w, c.snd)
    assert nslots == int(c.w["push"].sum()) and c.w["slot0"].tolist() == np.cumsum([0] + c.w["push"].tolist())[:-1].tolist()
    assert nfd == int((c.w["q0"] + c.w["cap"]).max())
    assert ring_bytes == int((c.w["ring_off"] + (c.w["cap"] - 1) * c.w["stride"].astype(np.uint64) + 54 + c.w["mss"]).max())
    # an empty queue may lie anywhere; abutting regions are not overlapping
    c.snd["nseg"], c.snd["seg0"] = 0, 0
    c.w["q0"] = [0, 5, 10]
    lvlip.push_plan(c.w, c.snd)


def test_refusals_without_gpu():
    """Host memory stands in for the device pointers: a refused call touches
    none of it and makes no HIP call."""
    L = lvlip.lib()
    c = plan_inputs()
    c.lro = np.zeros(3, dtype=lvlip.LRO_RESULT_DTYPE)
    fd_out = np.full(c.nslots + 1, 0x5A5A5A5A, dtype=np.uint32).repeat(4).view(FD)[:c.nslots + 1]
    res = np.full(4 * 4, 0x5A5A5A5A, dtype=np.uint32).view(lvlip.PUSH_RESULT_DTYPE)
    arrays = (c.f, c.lro, c.snd, c.w, c.payload, c.ring, c.fd, c.sacked, fd_out, res)
    keep = [a.copy() for a in arrays]
    f, lro, s, w, pay, ring, fd, sk, fo, r = (a.ctypes.data for a in arrays)
    assert f % 8 == 0 and s % 8 == 0 and w % 8 == 0 and lro % 16 == 0 and fd % 16 == 0 and fo % 16 == 0 and r % 16 == 0
    n, ns = 3, c.nslots
    assert ns > 0
    good = (f, lro, s, w, n, ns, pay, ring, fd, sk, fo, r)
    names = ("f", "lro", "s", "w", "nflows", "nslots", "payload", "base", "fd", "sacked", "fd_out", "res")

    def but(**kw):
        return tuple(kw.get(k, v) for k, v in zip(names, good))

    both = {"NULL f": but(f=None), "NULL s": but(s=None), "NULL w": but(w=None), "NULL fd": but(fd=None),
            "NULL res": but(res=None), "NULL payload": but(payload=None), "NULL base": but(base=None),
            "NULL fd_out": but(fd_out=None), "nflows 0 with slots": but(nflows=0),
            "nflows above LVLIP_LRO_MAX_FLOWS": but(nflows=65537), "nslots above LVLIP_MAX_BATCH": but(nslots=0xFFFFFFF1),
            "NULL f, no slots": but(f=None, nslots=0), "NULL res, no slots": but(res=None, nslots=0)}
    for what, args in both.items():
        assert L.lvlip_push_cpu(*args) == lvlip.EINVAL, what
        assert L.lvlip_push_dev(*args, None) == lvlip.EINVAL, what
    dev_only = {"misaligned f": but(f=f + 4), "misaligned s": but(s=s + 4), "misaligned w": but(w=w + 4),
                "misaligned lro": but(lro=lro + 8), "misaligned fd": but(fd=fd + 8), "misaligned fd_out": but(fd_out=fo + 8),
                "misaligned res": but(res=r + 8)}
    for what, args in dev_only.items():
        assert L.lvlip_push_dev(*args, None) == lvlip.EINVAL, what
    # the host form also refuses what the plan refuses, and a count that is not the plan's
    assert L.lvlip_push_cpu(*but(nslots=ns - 1)) == lvlip.EINVAL
    for what in ("cap 0", "slot_nxt == cap", "FIN", "queue starts below q0", "stride below 54 + mss"):
        d = c.copy()
        PLAN_REFUSALS[what](d)
        before = [a.copy() for a in (d.snd, d.w, d.ring, d.fd, d.sacked)]
        assert L.lvlip_push_cpu(f, lro, d.snd.ctypes.data, d.w.ctypes.data, n, ns, pay, ring, d.fd.ctypes.data,
                                d.sacked.ctypes.data, fo, r) == lvlip.EINVAL, what
        for a, b in zip((d.snd, d.w, d.ring, d.fd, d.sacked), before):
            assert a.tobytes() == b.tobytes(), what
    # no-ops
    assert L.lvlip_push_cpu(*(None,) * 4, 0, 0, *(None,) * 6) == lvlip.OK
    assert L.lvlip_push_dev(*(None,) * 4, 0, 0, *(None,) * 6, None) == lvlip.OK
    for a, k in zip(arrays, keep):
        assert a.tobytes() == k.tobytes()
    if lvlip.device_count() == 0:
        assert L.lvlip_push_dev(*good, None) == lvlip.ENODEV
        assert L.lvlip_push_dev(*but(nslots=0, payload=None, base=None, fd_out=None), None) == lvlip.ENODEV
        for a, k in zip(arrays, keep):
            assert a.tobytes() == k.tobytes()
    with pytest.raises(ValueError):
        lvlip.push_cpu(c.f, None, c.snd[:2].copy(), c.w, c.payload, c.ring, c.fd)
    with pytest.raises(TypeError):
        lvlip.push_cpu(c.f, None, c.snd, c.w.view(np.uint8), c.payload, c.ring, c.fd)
    with pytest.raises(ValueError):
        lvlip.push_cpu(c.f, None, c.snd, c.w, c.payload, c.ring[:100].copy(), c.fd)


def test_no_slots_still_compacts_and_writes_res():
    c = plan_inputs()
    c.w["push"] = 0
    c.nslots = lvlip.push_plan(c.w, c.snd)[0]
    assert c.nslots == 0
    want = model_push(c)
    got = run_cpu(c)
    assert_outputs(got, want)
    assert got["res"]["moved"].tolist() == [2, 2, 2] and (got["snd"]["seg0"] == c.w["q0"]).all()


# ------------------------------------------------------------- the whole loop --

SLOTS, PUSH_ROUNDS = 16, 48


class PushLoop:
    """tests/test_carry_cpu.py's StreamLoop (8 flows x 40 segments of 536 B
    through windows of 8 segments) with a TX ring of 16 slots per flow: every
    round A pushes up to 8 new segments per flow into the slots the ACKs gave
    back, then sends 8 queue entries per flow through the scoreboard.  The
    network: stream segment j of a flow with j = 4 mod 5 is lost the first time
    it is sent; what is sent again arrives."""

    def __init__(self):
        from test_carry_cpu import SEGS, WND_SEGS, StreamLoop

        self.base = b = StreamLoop()
        L, n, mss = b.link, b.nflows, b.mss
        self.n, self.mss, self.segs, self.rtx = n, mss, SEGS, WND_SEGS
        self.stride = 54 + mss + 3
        self.iss = np.array(L.iss, dtype=np.int64)
        self.snd = np.zeros(n, dtype=lvlip.SND_FLOW_DTYPE)
        self.snd["snd_una"] = self.snd["snd_nxt"] = L.iss
        self.snd["seg0"], self.snd["rtx"], self.snd["win"] = np.arange(n) * SLOTS, WND_SEGS, 28200
        self.nslots_rtx, _ = lvlip.snd_plan(self.snd)
        self.w = np.concatenate([lvlip.push_flow(L.sends[k]["hdr"].tobytes(), k * SEGS * mss, SEGS * mss, mss,
                                                 5 + k * SLOTS * self.stride, SLOTS, k * SLOTS, WND_SEGS,
                                                 stride=self.stride) for k in range(n)])
        self.nslots, self.ring_bytes, self.nfd = lvlip.push_plan(self.w, self.snd)

    def wire(self, fd_out, ring, sent):
        """The network on numpy arrays: which of the frames sent are lost."""
        live = fd_out["len"] > 0
        off = fd_out["offset"].astype(np.int64)
        seq = np.zeros(fd_out.size, dtype=np.int64)
        for j in range(4):
            seq = (seq << 8) | ring[off + 38 + j]
        flow = np.arange(fd_out.size) // self.rtx
        seg = np.clip(((seq - self.iss[flow]) & M32) // self.mss, 0, self.segs - 1)
        idx = flow * self.segs + seg
        lost = live & (sent[idx] == 0) & (seg % 5 == 4)
        np.add.at(sent, idx, live.astype(np.int32))
        out = fd_out.copy()
        out["len"][lost] = 0
        return out

    def run_cpu(self):
        b, n = self.base, self.n
        L = b.link
        fb, fa, snd, w = b.fb.copy(), L.fa.copy(), self.snd.copy(), self.w.copy()
        ring = np.full(self.ring_bytes, CANARY, dtype=np.uint8)
        fd, sacked = np.zeros(self.nfd, dtype=FD), np.zeros(self.nfd, dtype=np.uint8)
        stream = np.full(L.stream.size, CANARY, dtype=np.uint8)
        res = np.zeros(n, dtype=lvlip.LRO_RESULT_DTYPE)
        sres = np.zeros(n, dtype=lvlip.SND_RESULT_DTYPE)
        sent = np.zeros(n * self.segs, dtype=np.int32)
        pushed = 0
        for _ in range(PUSH_ROUNDS):
            _, pres = lvlip.push_cpu(fa, None, snd, w, L.payload, ring, fd, sacked)
            pushed += int(pres["pushed"].sum())
            fd_out, pick = lvlip.rtx_sack_cpu(fa, None, snd, sres, sacked, ring, fd)
            wire = self.wire(fd_out, ring, sent)
            _, rec = lvlip.lro_cpu(ring, wire, fb, lvlip.RX_VERIFY_L4, out=stream)
            lvlip.lro_advance_carry(fb, rec, res, res)
            ack, afd = lvlip.ack_cpu(L.tmpl, fb, res, lvlip.ACK_ALL, out=np.full(L.ack_bytes, CANARY, dtype=np.uint8))
            lvlip.lro_next_cpu(fb, res)
            fb["rcv_wnd"] = np.minimum(b.wnd, b.end - fb["out_off"])
            _, arec = lvlip.lro_cpu(ack, afd, fa, lvlip.RX_VERIFY_L4, out=np.zeros(n + 64, dtype=np.uint8))
            sres = lvlip.snd_cpu(fa, snd, arec, ring, fd)
            lvlip.sack_cpu(fa, snd, arec, ack, afd, ring, fd, sacked)
            lvlip.snd_next_cpu(snd, sres)
        return dict(stream=stream, fb=fb, snd=snd, w=w, res=res, sres=sres, ring=ring, fd=fd, sacked=sacked, sent=sent,
                    pres=pres, pushed=pushed)

    def check_done(self, got: dict):
        L = self.base.link
        assert np.array_equal(got["stream"], L.payload), "the streams are not the payloads"
        assert not got["snd"]["nseg"].any() and (got["snd"]["snd_una"] == got["snd"]["snd_nxt"]).all()
        assert not got["w"]["unsent"].any() and (got["fb"]["rcv_nxt"] == got["snd"]["snd_nxt"]).all()
        assert ((got["snd"]["snd_nxt"].astype(np.int64) - self.iss) & M32 == self.segs * self.mss).all()
        assert (got["fb"]["out_off"] == self.base.end).all() and not got["fb"]["rcv_wnd"].any()
        assert got["pushed"] == self.n * self.segs
        assert (got["sent"].reshape(self.n, self.segs)[:, 4::5] >= 2).all(), "every lost frame went out again"
        assert (got["sent"] >= 1).all()


@functools.lru_cache(maxsize=None)
def push_loop_cpu():
    loop = PushLoop()
    return loop, loop.run_cpu()


def test_the_loop_with_a_ring_of_16_slots_on_the_cpu_forms():
    loop, got = push_loop_cpu()
    loop.check_done(got)
    L = loop.base.link
    # the ring and fd are those of 16 slots per flow, against the 40 of stream_loop
    assert loop.nfd == loop.n * SLOTS and L.fd.size == loop.n * 40
    assert got["fd"].size == loop.nfd and got["ring"].size == loop.ring_bytes
    assert loop.ring_bytes == 5 + loop.n * SLOTS * loop.stride - 3
    assert loop.ring_bytes * 5 < (L.ring.size - 64) * 2 + 64
    assert (got["w"]["slot_nxt"] == 40 % SLOTS).all()  # 40 segments through 16 slots: the slots wrapped twice


# ----------------------------------------------------- sanitizers and scratch --

def test_example_under_sanitizers(tmp_path):
    """examples/push_loop.c (its own main: stream_loop.c's transfer with a ring
    of 2 x window slots per flow and a push each round, on the CPU forms, every
    buffer malloc'd at exactly its planned size) compiled with the library's C
    sources under ASan + UBSan, and run as a program."""
    exe = tmp_path / "push_loop_san"
    src = [os.path.join(ROOT, "examples", "push_loop.c")] + [
        os.path.join(ROOT, "level-ip_amd", "csrc", f)
        for f in ("push_cpu.c", "sack_cpu.c", "snd_cpu.c", "ack_cpu.c", "rcv_cpu.c", "seg_cpu.c", "csum_cpu.c")]
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "include"), *src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "push_loop ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_new_kernels_and_k_tso_use_no_scratch(tmp_path):
    """k_push_count, k_push, k_push_step and k_tso, which shares its row with
    k_push: every private segment is 0."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    found = []
    for name, pat in (("push_kernels", r"k_push\w*"), ("seg_kernels", r"k_tso")):
        asm = tmp_path / f"{name}.s"
        subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "-S", "--cuda-device-only", os.path.join(ROOT, "level-ip_amd", "csrc", f"{name}.hip"),
                        "-o", str(asm)], check=True, capture_output=True)
        found += re.findall(r"\.name:\s+(\S*" + pat + r"\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)",
                            asm.read_text())
    names = [name for name, _ in found]
    for want in ("k_push_count", "6k_pushE", "k_push_step", "k_tso"):
        assert any(want in name for name in names), (want, names)
    assert len(found) == 4 and all(int(size) == 0 for _, size in found), found
