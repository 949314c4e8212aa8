"""The peer's window on the calling thread (lvlip_wnd_cpu, rto_cpu.c;
include/lvlip_skb.h "the timer and the peer's window"): the winner rule against
a plain Python restatement over random batches with ties, old and beyond ACKs
and crafted records; frames with IPv4 and TCP options; frames too short to hold
the field; wscale and both caps; LVLIP_WND_APPLY on and off; flows without a
winner; the reference's own ACK frames (tests/golden/ack_ref.json)."""
import json
import os
import struct

import numpy as np
import pytest

import lvlip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
NONE = 0xFFFFFFFF
WND_MAX = 1 << 30
FD, REC = lvlip.FRAME_DESC_DTYPE, lvlip.LRO_REC_DTYPE
P, NO_DATA, OOW, CONTROL = 1, 20, 21, 19


def ack_frame(window: int, ihl: int = 5, hl: int = 5, version: int = 4, cut: int = 0, fill: int = 0x33) -> bytes:
    """An Ethernet/IPv4/TCP frame with `window` at 14 + ihl*4 + 14, option
    bytes as filler, `cut` bytes taken off its end."""
    ip = bytearray([fill]) * (4 * max(ihl, 5))  # a lying nibble still has bytes behind it
    ip[0] = (version << 4) | ihl
    tcp = bytearray([fill]) * (4 * max(hl, 5))
    tcp[12], tcp[13] = hl << 4, 0x10
    tcp[14:16] = struct.pack("!H", window)
    fr = bytes([fill]) * 12 + b"\x08\x00" + bytes(ip) + bytes(tcp)
    return fr[:len(fr) - cut]


def frame_window(fr: bytes):
    """The frame test of lvlip_sack_*; the window, or None."""
    if len(fr) < 34 or fr[14] >> 4 != 4 or fr[14] & 15 < 5:
        return None
    th = 14 + 4 * (fr[14] & 15)
    if len(fr) < th + 20:
        return None
    hl = fr[th + 12] >> 4
    if hl < 5 or len(fr) < th + 4 * hl:
        return None
    return (fr[th + 14] << 8) | fr[th + 15]


def model(f, s, t, w, rec, frames, flags):
    """lvlip_wnd_cpu in plain Python: (res, t, w) as the call leaves them."""
    n = f.size
    t, w = t.copy(), None if w is None else w.copy()
    res = np.zeros(n, dtype=lvlip.WND_RESULT_DTYPE)
    best = [None] * n
    for i, r in enumerate(rec):
        k = int(r["flow"])
        if k >= n or int(r["status"]) not in (P, NO_DATA, OOW) or not int(r["tcp_flags"]) & 0x10:
            continue
        if int(r["rel"]) > int(f["rcv_wnd"][k]):
            continue
        d = (int(r["ack_seq"]) - int(s["snd_una"][k])) & M32
        if d > (int(s["snd_nxt"][k]) - int(s["snd_una"][k])) & M32:
            continue
        raw = frame_window(frames[i])
        if raw is None:
            continue
        res["n_counting"][k] += 1
        if best[k] is None or (d, i) > best[k][:2]:
            best[k] = (d, i, raw)
    for k in range(n):
        if best[k]:
            res["winner"][k], res["raw"][k] = best[k][1], best[k][2]
            t["snd_wnd"][k] = min(best[k][2] << int(t["wscale"][k]), WND_MAX)
        else:
            res["winner"][k] = NONE
        res["snd_wnd"][k] = t["snd_wnd"][k]
        if flags & lvlip.WND_APPLY and w is not None:
            w["wnd"][k] = min(int(t["snd_wnd"][k]), int(t["wnd_cap"][k]))
    return res, t, w


def pack(frames, seed=0, base_mod=None):
    """The frames in one buffer at odd gaps; with base_mod every frame starts
    at an address that is base_mod mod 4 (relative to the buffer)."""
    rng = np.random.default_rng(seed)
    fd = np.zeros(len(frames), dtype=FD)
    chunks, pos = [], 0
    for i, fr in enumerate(frames):
        gap = int(rng.integers(0, 7))
        if base_mod is not None:
            gap = (base_mod - pos) % 4
        chunks.append(bytes([0xEE]) * gap + fr)
        fd["offset"][i], fd["len"][i] = pos + gap, len(fr)
        pos += gap + len(fr)
    return np.frombuffer(b"".join(chunks) + bytes(16), dtype=np.uint8).copy(), fd


def random_case(n, nflows, seed, one_flow=False):
    rng = np.random.default_rng(seed)
    f = np.zeros(nflows, dtype=lvlip.LRO_FLOW_DTYPE)
    f["rcv_wnd"] = rng.integers(1, 5000, nflows)
    s = np.zeros(nflows, dtype=lvlip.SND_FLOW_DTYPE)
    s["snd_una"] = rng.integers(0, 1 << 32, nflows, dtype=np.uint64)
    s["snd_una"][0] = 0xFFFFFF00  # the span wraps
    span = rng.integers(0, 4000, nflows).astype(np.uint64)
    s["snd_nxt"] = (s["snd_una"].astype(np.uint64) + span) & np.uint64(M32)
    t = lvlip.rto_flows(nflows)
    t["wscale"] = rng.integers(0, 15, nflows)
    t["snd_wnd"] = rng.integers(0, WND_MAX + 1, nflows)
    t["wnd_cap"] = rng.integers(0, WND_MAX + 1, nflows)
    t["wnd_cap"][::3] = rng.integers(0, 70000, t["wnd_cap"][::3].size)
    w = np.zeros(nflows, dtype=lvlip.PUSH_FLOW_DTYPE)
    w["wnd"] = 12345
    rec = np.zeros(n, dtype=REC)
    rec["flow"] = 0 if one_flow else rng.integers(0, nflows + 2, n)  # some beyond nflows
    if n:
        rec["flow"][rng.integers(0, n, max(n // 50, 1))] = NONE
    k = np.minimum(rec["flow"], nflows - 1).astype(np.int64)
    rec["status"] = rng.choice([P, NO_DATA, OOW, CONTROL, 18, 3], n, p=[.2, .5, .1, .1, .05, .05])
    rec["tcp_flags"] = rng.choice([0x10, 0x18, 0x08, 0x11], n, p=[.6, .2, .1, .1])
    rec["rel"] = np.where(rng.random(n) < .9, rng.integers(0, 5, n), f["rcv_wnd"][k] + rng.integers(0, 3, n))
    # d: few distinct values so that ties happen; old and beyond among them
    d = rng.choice(np.array([0, 1, 7, 7, 100, 3999, 4000, 1 << 31, M32, 5000], dtype=np.uint64), n)
    d = np.where(rng.random(n) < .5, np.minimum(d, span[k]), d).astype(np.uint64)
    rec["ack_seq"] = (s["snd_una"][k].astype(np.uint64) + d) & np.uint64(M32)
    frames = []
    for i in range(n):
        kind = rng.random()
        ihl, hl = int(rng.integers(5, 9)), int(rng.integers(5, 16))
        if kind < .75:
            frames.append(ack_frame(int(rng.integers(0, 65536)), ihl, hl))
        elif kind < .85:
            frames.append(ack_frame(int(rng.integers(0, 65536)), ihl, hl, cut=int(rng.integers(1, 4 * hl + 10))))
        elif kind < .9:
            frames.append(ack_frame(7, version=int(rng.choice([0, 6, 15]))))
        elif kind < .95:
            frames.append(ack_frame(7, ihl=int(rng.integers(0, 5)), hl=5))
        else:
            frames.append(ack_frame(7, ihl, hl=int(rng.integers(0, 5))))
    return f, s, t, w, rec, frames


def run(f, s, t, w, rec, frames, flags, seed=0, base_mod=None):
    buf, fd = pack(frames, seed, base_mod)
    t, w = t.copy(), None if w is None else w.copy()
    res = lvlip.wnd_cpu(f, s, t, w, rec, buf, fd, flags)
    return res, t, w


def same(got, want):
    for g, x, name in zip(got, want, ("res", "t", "w")):
        assert (g is None) == (x is None)
        if g is not None:
            assert g.tobytes() == x.tobytes(), name


@pytest.mark.parametrize("n,nflows", ((0, 3), (1, 1), (200, 1), (500, 7), (3000, 40), (2000, 300)))
@pytest.mark.parametrize("flags", (0, lvlip.WND_APPLY))
def test_the_winner_rule_on_random_batches(n, nflows, flags):
    case = random_case(n, nflows, seed=n + nflows)
    want = model(*case, flags)
    same(run(*case, flags), want)
    if n >= 500:
        res = want[0]
        assert (res["n_counting"] > 1).any() and ((res["winner"] == NONE).any() or nflows < 300)
        assert int(res["n_counting"].sum()) < n  # records were refused
    if not flags:
        assert (want[2]["wnd"] == 12345).all()
    if flags and n == 0:
        assert (want[2]["wnd"] == np.minimum(case[2]["snd_wnd"], case[2]["wnd_cap"])).all(), "n == 0 still applies"


def test_ties_in_d_go_to_the_later_record_and_larger_d_wins():
    f = np.zeros(1, dtype=lvlip.LRO_FLOW_DTYPE)
    f["rcv_wnd"] = 100
    s = np.zeros(1, dtype=lvlip.SND_FLOW_DTYPE)
    s["snd_una"], s["snd_nxt"] = 1000, 2000
    rec = np.zeros(6, dtype=REC)
    rec["status"], rec["tcp_flags"] = NO_DATA, 0x10
    rec["ack_seq"] = [1500, 1800, 1800, 1000, 2001, 999]  # new, new, new (tie), duplicate, beyond, old
    frames = [ack_frame(10 + i) for i in range(6)]
    res, t, _ = run(f, s, lvlip.rto_flows(1), None, rec, frames, 0)
    assert list(res[0].tolist()) == [4, 2, 12, 12] and t["snd_wnd"][0] == 12
    # the same records in another order: the same (d, i) rule, so now the record moved last wins its tie
    order = [2, 0, 5, 4, 3, 1]
    res, t, _ = run(f, s, lvlip.rto_flows(1), None, rec[order], [frames[i] for i in order], 0)
    assert list(res[0].tolist()) == [4, 5, 11, 11]
    # only duplicates: the later one
    rec["ack_seq"] = 1000
    res, _, _ = run(f, s, lvlip.rto_flows(1), None, rec, frames, 0)
    assert list(res[0].tolist()) == [6, 5, 15, 15]


def test_options_short_frames_scale_and_caps():
    f = np.zeros(1, dtype=lvlip.LRO_FLOW_DTYPE)
    f["rcv_wnd"] = 100
    s = np.zeros(1, dtype=lvlip.SND_FLOW_DTYPE)
    s["snd_nxt"] = 10
    rec = np.zeros(1, dtype=REC)
    rec["status"], rec["tcp_flags"], rec["ack_seq"] = NO_DATA, 0x10, 5

    def one(frame, **kw):
        t = lvlip.rto_flows(1, snd_wnd=777, **kw)
        w = np.zeros(1, dtype=lvlip.PUSH_FLOW_DTYPE)
        res, t, w = run(f, s, t, w, rec, [frame], lvlip.WND_APPLY)
        return list(res[0].tolist()), int(t["snd_wnd"][0]), int(w["wnd"][0])

    for ihl in range(5, 16):
        for hl in range(5, 16):
            assert one(ack_frame(0xBEEF, ihl, hl))[0] == [1, 0, 0xBEEF, 0xBEEF], (ihl, hl)
    full = len(ack_frame(1, 6, 7))
    for cut in range(1, full + 1):  # every length below the whole frame: refused, the state stays
        assert one(ack_frame(0xBEEF, 6, 7, cut=cut)) == ([0, NONE, 0, 777], 777, 777), cut
    assert one(ack_frame(0x1234), wscale=7) == ([1, 0, 0x1234, 0x1234 << 7], 0x1234 << 7, 0x1234 << 7)
    assert one(ack_frame(0xFFFF), wscale=14)[1] == 0xFFFF << 14 and (0xFFFF << 14) < WND_MAX
    assert one(ack_frame(0xFFFF), wscale=14, wnd_cap=5000) == ([1, 0, 0xFFFF, 0xFFFF << 14], 0xFFFF << 14, 5000)
    assert one(ack_frame(0), wnd_cap=5000) == ([1, 0, 0, 0], 0, 0)
    assert one(ack_frame(9, version=6), wnd_cap=100) == ([0, NONE, 0, 777], 777, 100), "no winner: cap still applies"


def test_the_references_own_ack_frames():
    """The ACKs level-ip itself sent (make_ack_golden.py): parsed by
    lvlip_lro_cpu as the sender's reverse plan parses them, each yields the
    window the reference wrote at bytes 48-49."""
    with open(os.path.join(ROOT, "tests", "golden", "ack_ref.json")) as fh:
        fx = json.load(fh)
    acks = [bytes.fromhex(a) for a in fx["acks"] if a]  # null: the stack sent no ACK for that segment
    assert len(acks) >= 5
    a0 = acks[0]
    ack_seq = struct.unpack_from("!I", a0, 42)[0]
    flows = lvlip.lro_flow(a0[26:30], a0[30:34], struct.unpack_from("!H", a0, 34)[0], struct.unpack_from("!H", a0, 36)[0],
                           struct.unpack_from("!I", a0, 38)[0], 4096)
    lvlip.lro_plan(flows)
    s = np.zeros(1, dtype=lvlip.SND_FLOW_DTYPE)
    s["snd_una"], s["snd_nxt"] = ack_seq, (ack_seq + 100000) & M32
    for i, a in enumerate(acks):
        buf, fd = pack([a], seed=i)
        _, rec = lvlip.lro_cpu(buf, fd, flows, 0, out=np.zeros(4096, dtype=np.uint8))
        assert rec["status"][0] == NO_DATA
        t = lvlip.rto_flows(1)
        res = lvlip.wnd_cpu(flows, s, t, None, rec, buf, fd)
        want = struct.unpack_from("!H", a, 48)[0]
        assert list(res[0].tolist()) == [1, 0, want, want] and want > 0
    # all ten in one batch: ack_seq only rises, so the last of the largest wins
    buf, fd = pack(acks, seed=99)
    _, rec = lvlip.lro_cpu(buf, fd, flows, 0, out=np.zeros(4096, dtype=np.uint8))
    res = lvlip.wnd_cpu(flows, s, lvlip.rto_flows(1), None, rec, buf, fd)
    d = (rec["ack_seq"].astype(np.int64) - ack_seq) & M32
    win = max(range(len(acks)), key=lambda i: (d[i], i))
    assert res["n_counting"][0] == len(acks) and res["winner"][0] == win


def test_refusals_and_noops():
    L = lvlip.lib()
    f, s, t, w, rec, frames = random_case(10, 2, 1)
    buf, fd = pack(frames)
    res = np.zeros(2, dtype=lvlip.WND_RESULT_DTYPE)
    p = lambda a: a.ctypes.data  # noqa: E731
    ok = (p(f), p(s), p(t), p(w), 2, p(rec), p(buf), p(fd), 10, 1, p(res))
    keep = (t.tobytes(), w.tobytes())
    for i, v in ((0, None), (1, None), (2, None), (10, None), (5, None), (6, None), (7, None), (9, 2), (9, 3),
                 (4, lvlip.LRO_MAX_FLOWS + 1)):
        bad = list(ok)
        bad[i] = v
        assert L.lvlip_wnd_cpu(*bad) == lvlip.EINVAL, i
    u = t.copy()
    u["wscale"][1] = 15
    assert L.lvlip_wnd_cpu(p(f), p(s), p(u), p(w), 2, p(rec), p(buf), p(fd), 10, 1, p(res)) == lvlip.EINVAL
    assert (t.tobytes(), w.tobytes()) == keep and not res.view(np.uint8).any()
    assert L.lvlip_wnd_cpu(None, None, None, None, 0, None, None, None, 10, 0, None) == lvlip.OK
    assert L.lvlip_wnd_cpu(p(f), p(s), p(t), None, 2, None, None, None, 0, 1, p(res)) == lvlip.OK  # NULL w, n == 0
    assert res["winner"].tolist() == [NONE, NONE] and res["snd_wnd"].tolist() == t["snd_wnd"].tolist()
    # the device form: the same refusals and a misaligned pointer before any HIP call
    dok = ok + (None,)
    for i, v in ((0, None), (2, None), (10, None), (5, None), (9, 2), (0, p(f) + 4), (1, p(s) + 4), (2, p(t) + 4),
                 (3, p(w) + 4), (5, p(rec) + 8), (7, p(fd) + 8), (10, p(res) + 8)):
        bad = list(dok)
        bad[i] = v
        assert L.lvlip_wnd_dev(*bad) == lvlip.EINVAL, i
    assert L.lvlip_wnd_dev(None, None, None, None, 0, None, None, None, 10, 0, None, None) == lvlip.OK
    with pytest.raises(ValueError):
        lvlip.wnd_cpu(f, s, t[:1].copy(), None, rec, buf, fd)
    with pytest.raises(ValueError):
        lvlip.wnd_cpu(f, s, t, None, rec[:3], buf, fd)
    with pytest.raises(ValueError):
        lvlip.wnd_cpu(f, s, t, None, rec, buf[:50].copy(), fd)
