"""A plain restatement of lvlip_rbuf_* (include/lvlip_skb.h, "f1: the receive
buffer"), steps 1-5 flow by flow on Python integers, and the random
cases its tests share.  Not a test file."""
import numpy as np

import lvlip

M32 = 0xFFFFFFFF
MOVED, ADVANCED, UPDATE = lvlip.RBUF_MOVED, lvlip.RBUF_ADVANCED, lvlip.RBUF_UPDATE


def model(f, res, p, t, nread, out, sink):
    """What one call leaves: (f, p, t, gate, rres, out, sink) as new arrays."""
    f, p, t, out = f.copy(), p.copy(), t.copy(), out.copy()
    sink = None if sink is None else sink.copy()
    gate = res.copy()
    rres = np.zeros(f.size, dtype=lvlip.RBUF_RESULT_DTYPE)
    for k in range(f.size):
        base, cap, head = int(p["base_off"][k]), int(p["cap"][k]), int(p["head"][k])
        out_off, rcv_wnd, rcv_nxt = int(f["out_off"][k]), int(f["rcv_wnd"][k]), int(f["rcv_nxt"][k])
        used = out_off - base
        # 1 read
        r = min(0 if nread is None else int(nread[k]), used - head)
        if sink is not None:
            so = int(p["sink_off"][k])
            sink[so:so + r] = out[base + head:base + head + r]
            p["sink_off"][k] = so + r
        head += r
        # 2 live bytes
        span = 0
        for j in range(min(int(res["nsack"][k]), 4)):
            left, right = (int(res["sack"][k, j, 0]) - rcv_nxt) & M32, (int(res["sack"][k, j, 1]) - rcv_nxt) & M32
            if left < right <= rcv_wnd:
                span = max(span, right)
        live = used - head + span
        # 3 reuse
        flags = moved = 0
        if head > 0 and live <= head:
            out[base:base + live] = out[base + head:base + head + live].copy()
            out_off, rcv_wnd, moved, head = out_off - head, rcv_wnd + head, live, 0
            flags |= MOVED
        # 4 window
        edge, adv_edge = (rcv_nxt + rcv_wnd) & M32, int(p["adv_edge"][k])
        if (edge - adv_edge) & M32 >= min((cap + 1) // 2, int(p["mss"][k])):
            adv_edge = edge
            flags |= ADVANCED
            if res["placed"][k] == 0:  # 5 update
                gate["placed"][k] = 1
                flags |= UPDATE
        a = (adv_edge - rcv_nxt) & M32
        field = min(a >> int(p["wscale"][k]), 65535)
        t["hdr"][k, 48], t["hdr"][k, 49] = field >> 8, field & 0xFF
        f["out_off"][k], f["rcv_wnd"][k] = out_off, rcv_wnd
        p["head"][k], p["adv_edge"][k] = head, adv_edge
        rres[k] = (r, out_off - base - head, head, moved, a, field, flags, 0)
    return f, p, t, gate, rres, out, sink


def random_case(nflows: int, seed: int, max_cap: int = 3000, shift: int = 0):
    """(f, res, p, t, nread, out, sink): planned states whose flows between
    them take every branch of the steps; `out` and `sink` hold random bytes
    and start `shift` bytes into the offsets (the buffers lie at every
    alignment to each other)."""
    rng = np.random.default_rng(seed)
    f = np.zeros(nflows, dtype=lvlip.LRO_FLOW_DTYPE)
    p = np.zeros(nflows, dtype=lvlip.RBUF_FLOW_DTYPE)
    res = np.zeros(nflows, dtype=lvlip.LRO_RESULT_DTYPE)
    t = np.zeros(nflows, dtype=lvlip.ACK_TMPL_DTYPE)
    t["hdr"] = rng.integers(0, 256, (nflows, 54))
    t["out_off"], t["max_sack"] = np.arange(nflows) * 90, 4
    nread = np.zeros(nflows, dtype=np.uint32)
    at, sat = shift, shift + 3
    for k in range(nflows):
        cap = int(rng.choice([1, 2, 15, 16, 17, 535, 536, int(rng.integers(1, max_cap + 1)), max_cap]))
        used = int(rng.choice([0, cap, int(rng.integers(0, cap + 1))]))
        head = int(rng.choice([0, used, used // 2, (used + 1) // 2, int(rng.integers(0, used + 1))]))
        rcv_nxt = int(rng.choice([0, 1, M32, M32 - cap // 2, int(rng.integers(0, M32 + 1))]))
        p[k]["base_off"], p[k]["cap"], p[k]["head"], p[k]["sink_off"] = at, cap, head, sat
        p[k]["mss"] = int(rng.choice([1, 536, 1460, 65535]))
        p[k]["wscale"] = int(rng.choice([0, 0, 1, 7, 14]))
        wnd = cap - used
        p[k]["adv_edge"] = (rcv_nxt + wnd - int(rng.choice([0, 0, 1, wnd // 2, wnd, int(rng.integers(0, cap + 1))]))) & M32
        f[k]["saddr"], f[k]["daddr"], f[k]["sport"], f[k]["dport"] = 0x0100000A, 0x0200000A, k, 80
        f[k]["rcv_nxt"], f[k]["rcv_wnd"], f[k]["out_off"] = rcv_nxt, wnd, at + used
        nread[k] = int(rng.choice([0, 1, used - head, max(used - head - 1, 0), cap, M32, int(rng.integers(0, cap + 1))]))
        res[k]["placed"] = int(rng.choice([0, 0, 1, 9]))
        res[k]["delivered"], res[k]["reserved"] = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        res[k]["nsack"] = int(rng.choice([0, 0, 1, 2, 4, 7]))
        for j in range(4):
            kind = int(rng.integers(0, 5))
            lo, hi = sorted(int(x) for x in rng.integers(0, wnd + 1, 2))
            if kind == 0:    # ends beyond the window
                hi = wnd + 1 + int(rng.integers(0, 100))
            elif kind == 1:  # stale: behind rcv_nxt
                lo, hi = -int(rng.integers(1, 5000)), -int(rng.integers(0, 3))
            elif kind == 2:  # empty
                hi = lo
            res[k]["sack"][j] = ((rcv_nxt + lo) & M32, (rcv_nxt + hi) & M32)
        at += cap + int(rng.integers(0, 40))
        sat += cap + int(rng.integers(0, 40))
    out = rng.integers(0, 256, at + 64, dtype=np.uint8)
    sink = rng.integers(0, 256, sat + 64, dtype=np.uint8)
    assert lvlip.rbuf_plan(p, f) >= nflows
    return f, res, p, t, nread, out, sink


def branches(rres, res, nread) -> set:
    """The branches a call took, by name: what the tests assert is covered."""
    fl, got = rres["flags"], set()
    for name, mask in (("moved", (fl & MOVED) != 0), ("rewind", ((fl & MOVED) != 0) & (rres["moved"] == 0)),
                       ("moved_bytes", rres["moved"] > 0), ("kept", ((fl & MOVED) == 0) & (rres["head"] > 0)),
                       ("advanced", (fl & ADVANCED) != 0), ("held", (fl & ADVANCED) == 0),
                       ("update", (fl & UPDATE) != 0), ("advanced_with_data", ((fl & ADVANCED) != 0) & (res["placed"] > 0)),
                       ("read", rres["read"] > 0), ("read_clipped", rres["read"] < nread),
                       ("read_part", (rres["read"] > 0) & (rres["unread"] > 0)), ("clamped", rres["field"] == 65535)):
        if mask.any():
            got.add(name)
    return got


ALL_BRANCHES = {"moved", "rewind", "moved_bytes", "kept", "advanced", "held", "update", "advanced_with_data", "read",
                "read_clipped", "read_part", "clamped"}
