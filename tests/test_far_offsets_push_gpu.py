"""lvlip_push_dev past 4 GiB, on the pattern of tests/test_far_offsets_gpu.py
(its sparse allocation, zones and placement): ring_off and pay_off lie at low
and high offsets of one allocation, one flow's slots start below 2^32 and its
first frame crosses it, and one flow's unsent bytes straddle it too.  Every
32-bit alias of an offset used lands in canary bytes, so a dropped high dword
shows as a wrong byte.  Expected bytes come from lvlip_push_cpu on the 3 MiB
host ring."""
import numpy as np
import pytest

import lvlip
from devbuf import _t, guarded, unguard
from test_far_offsets_gpu import (MiB, TOP, Lay, assert_mixed, blank, far, fd_near, near,
                                  zone)  # noqa: F401  (zone: the module's fixture)
from test_push_cpu import FD, NO_LIMIT
from test_tso_cpu import template

pytestmark = pytest.mark.gpu


def far_case(straddler: str):
    """Five flows, mss 1, 3, 536, 1460, 1460; ring and payload alternate
    between the low and the high zone; the straddler is the last flow's slots
    or its payload."""
    rng = np.random.default_rng(8)
    lay, ring = Lay(), blank()
    n = 5
    w, snd = [], np.zeros(n, dtype=lvlip.SND_FLOW_DTYPE)
    f = np.zeros(n, dtype=lvlip.LRO_FLOW_DTYPE)
    f["rcv_nxt"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    q = 1
    for k, (mss, cap, unsent) in enumerate(((1, 4, 3), (3, 4, 10), (536, 3, 536 * 2 + 5), (1460, 2, 1460 * 2), (1460, 3, 4000))):
        stride = 54 + mss + 3
        last = k == n - 1
        ro = lay.put("x" if last and straddler == "ring" else "hl"[k % 2], cap * stride, before=700)
        po = lay.put("x" if last and straddler == "payload" else "lh"[k % 2], unsent, before=1000)
        ring[po:po + unsent] = rng.integers(0, 256, unsent, dtype=np.uint8)
        w.append(lvlip.push_flow(template(sport=41000 + k), po, unsent, mss, ro, cap, q, cap + 1, stride=stride,
                                 slot_nxt=cap - 1))
        snd[k]["snd_una"] = snd[k]["snd_nxt"] = 0xFFFFF000 + 777 * k
        snd[k]["seg0"], snd[k]["win"] = q, 5000 + k
        q += cap + 1
    return f, snd, np.concatenate(w), ring, q


@pytest.mark.parametrize("straddler", ("ring", "payload"))
def test_push_dev(straddler, zone):  # noqa: F811
    f, snd, w, ring, nfd = far_case(straddler)
    n = w.size
    w_far = w.copy()
    w_far["ring_off"], w_far["pay_off"] = far(w["ring_off"]), far(w["pay_off"])
    nslots, ring_bytes, got_nfd = lvlip.push_plan(w_far, snd)
    assert ring_bytes > TOP and got_nfd == nfd - 1
    assert lvlip.push_plan(w, snd)[0] == nslots and np.array_equal(w["slot0"], w_far["slot0"])
    assert_mixed(w_far["ring_off"], w["cap"] * w["stride"].astype(np.uint64) if straddler == "ring" else None)
    assert_mixed(w_far["pay_off"], w["unsent"] if straddler == "payload" else None)

    want, want_snd, want_w = ring.copy(), snd.copy(), w.copy()
    want_fd, want_sk = np.zeros(nfd, dtype=FD), np.full(nfd, 7, dtype=np.uint8)
    want_out, want_res = lvlip.push_cpu(f, None, want_snd, want_w, want, want, want_fd, want_sk)
    assert (want_res["pushed"] == w["cap"]).tolist() == [False, True, True, True, True] and want_res["pushed"][0] == 3
    assert_mixed(far(want_out["offset"][want_out["len"] > 0]), want_out["len"][want_out["len"] > 0] if straddler == "ring" else None)

    dev = zone.dev
    zone.load(ring)
    s_t, w_t = _t(snd, dev), _t(w_far, dev)
    fd_t, sk_t = guarded(16 * nfd, dev), guarded(nfd, dev)
    fd_t[:16 * nfd] = 0
    sk_t[:nfd] = 7
    out_t, res_t = guarded(16 * nslots, dev), guarded(16 * n, dev)
    lvlip.push_dev(_t(f, dev), None, s_t, w_t, nslots, zone.base, zone.base, fd_t[:16 * nfd], sk_t[:nfd],
                   out_t[:16 * nslots], res_t[:16 * n])
    zone.check(want, "lvlip_push_dev")
    live = want_out["len"] > 0
    got_out = unguard(out_t, 16 * nslots, FD)
    assert np.array_equal(fd_near(got_out)[live], want_out[live]) and np.array_equal(got_out[~live], want_out[~live])
    got_fd = unguard(fd_t, 16 * nfd, FD)
    used = want_fd["len"] > 0
    assert np.array_equal(fd_near(got_fd)[used], want_fd[used]) and not got_fd[~used]["len"].any()
    assert np.array_equal(unguard(sk_t, nfd, np.uint8), want_sk)
    assert unguard(res_t, 16 * n, lvlip.PUSH_RESULT_DTYPE).tobytes() == want_res.tobytes()
    assert s_t.cpu().numpy().tobytes() == want_snd.tobytes()
    got_w = w_t.cpu().numpy().view(lvlip.PUSH_FLOW_DTYPE).copy()
    assert (got_w["pay_off"] >= TOP).any() and np.array_equal(near(got_w["pay_off"]), want_w["pay_off"])
    got_w["pay_off"], got_w["ring_off"] = want_w["pay_off"], near(got_w["ring_off"])
    assert got_w.tobytes() == want_w.tobytes()
    assert not np.array_equal(want, ring) and (np.flatnonzero(want != ring) >= 2 * MiB).any()
    assert NO_LIMIT == 1 << 30
