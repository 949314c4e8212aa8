"""lvlip_sack_dev and lvlip_rtx_sack_dev past 4 GiB, on the pattern of
tests/test_far_offsets_gpu.py (its sparse allocation, zones and placement):
the ACK frames and the queue's frames lie at low and high offsets of one
allocation, one ACK frame or one queue frame starts below 2^32 and crosses it,
and the scoreboard itself lies above 2^32.  Every 32-bit alias of an offset
used lands in canary bytes, so a dropped high dword shows as a wrong byte.
Expected bytes come from the CPU forms on the 3 MiB host ring."""
import numpy as np
import pytest

import lvlip
from devbuf import _t, guarded, unguard
from test_far_offsets_gpu import (MiB, Lay, assert_mixed, blank, far, fd_far, fd_near,
                                  zone)  # noqa: F401  (zone: the module's fixture)
from test_sack_cpu import NO_PICK, make_acks
from test_snd_cpu import Case

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 536, 1460)


def far_case(straddler: str, before: int):
    """Five queues of three frames, 24 ACK frames with whole-segment blocks and
    the scoreboard, placed in a host ring; the straddler is the 1460-byte head
    of the last queue or ACK frame 7."""
    c = Case(nseg=[3] * 5, mss=list(SIZES), rtx=[3] * 5, seed=41)
    rec, aring, afd0 = make_acks(c, 24, seed=6, blocks_only=True)
    lay, ring, fd, afd = Lay(), blank(), c.fd.copy(), afd0.copy()
    head = int(c.snd[4]["seg0"])
    for i, d in enumerate(c.fd):
        o, n = int(d["offset"]), int(d["len"])
        at = lay.put("x" if straddler == "queue" and i == head else "lh"[i % 2], n, before=before)
        ring[at:at + n] = c.ring[o:o + n]
        fd[i]["offset"] = at
    for i, d in enumerate(afd0):
        o, n = int(d["offset"]), int(d["len"])
        at = lay.put("x" if straddler == "ack" and i == 7 else "hl"[i % 2], n, before=before)
        ring[at:at + n] = aring[o:o + n]
        afd[i]["offset"] = at
    board = lay.high(fd.size)
    ring[board:board + fd.size] = 0
    assert_mixed(far(fd["offset"]), fd["len"] if straddler == "queue" else None)
    assert_mixed(far(afd["offset"]), afd["len"] if straddler == "ack" else None)
    return c, rec, ring, fd, afd, board


@pytest.mark.parametrize("straddler,before", (("queue", 30), ("ack", 60), ("ack", 20)))
def test_sack_dev_and_rtx_sack_dev(straddler, before, zone):  # noqa: F811
    """30: the queue head's 54 header bytes cross 2^32.  60: an ACK frame's
    option bytes cross it (the TCP header ends at byte 54).  20: its IPv4
    header does.  Then the selective retransmit over the scoreboard the first
    call left above 2^32."""
    c, rec, ring, fd, afd, board = far_case(straddler, before)
    n, nfd = c.flows.size, fd.size
    want = ring.copy()
    want_res = lvlip.sack_cpu(c.flows, c.snd, rec, want, afd, want, fd, want[board:board + nfd])
    marked = want[board:board + nfd].copy()
    assert 0 < int(marked.sum()) < nfd and int(want_res["n_sacked"].sum()) == int(marked.sum())
    dev = zone.dev
    zone.load(ring)
    ins = [_t(a, dev) for a in (c.flows, c.snd, rec, fd_far(afd), fd_far(fd))]
    o = int(far(board))
    board_t = zone.base[o:o + nfd]
    res_t = guarded(16 * n, dev)
    lvlip.sack_dev(ins[0], ins[1], ins[2], zone.base, ins[3], zone.base, ins[4], board_t, res_t[:16 * n])
    zone.check(want, "lvlip_sack_dev")
    assert unguard(res_t, 16 * n, lvlip.SACK_RESULT_DTYPE).tobytes() == want_res.tobytes()

    want_fd, want_pick = lvlip.rtx_sack_cpu(c.flows, None, c.snd, None, marked, want, fd)
    assert (want_pick != NO_PICK).any() and (want_pick == NO_PICK).any()
    out_t, pick_t = guarded(16 * c.nslots, dev), guarded(4 * c.nslots, dev)
    lvlip.rtx_sack_dev(ins[0], None, ins[1], None, board_t, c.nslots, zone.base, ins[4], out_t[:16 * c.nslots],
                       pick_t[:4 * c.nslots])
    zone.check(want, "lvlip_rtx_sack_dev")
    assert np.array_equal(fd_near(unguard(out_t, 16 * c.nslots, lvlip.FRAME_DESC_DTYPE)), want_fd)
    assert np.array_equal(unguard(pick_t, 4 * c.nslots, np.uint32), want_pick)
    assert not np.array_equal(want, ring) and (np.flatnonzero(want != ring) >= 2 * MiB).any()
