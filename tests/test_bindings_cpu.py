"""What the f1/f2 wrappers of lvlip.py (tso_*, lro_*, ack_*, snd_*, rtx_*,
sack_*, rtx_sack_*) refuse before they reach the C call: the exception's type
and its exact text, and which refusal wins when a call has two things wrong.
The four plan calls' ValueError for a plan the library refuses is pinned too.

The device wrappers test sizes before they touch a stream, so plain CPU torch
tensors reach every refusal here; none of these calls launches anything.
tso_dev alone looks its stream up first and gets a stand-in for it."""
import numpy as np
import pytest
import torch

import lvlip
from test_tso_cpu import template as tso_template

ONE_SEND_SIDE = "one send side per flow"
ONE_RESULT = "one result per flow"
OUT = "out: a contiguous uint8 array of at least the plan's out_bytes"
BASE = "base: a writeable contiguous uint8 array (the ring is rewritten in place)"
SACKED = "sacked: a writeable contiguous uint8 array (the scoreboard is marked in place)"
SACKED_SIZE = "sacked: one byte per fd entry"
PAST_FD = "a queue lies past fd"
PAST_RING = "a frame lies past the ring"
TSO_PLAN = "sends: a writeable contiguous TsoSend array"
LRO_PLAN = "flows: a writeable contiguous LRO_FLOW_DTYPE array"
ACK_PLAN = "tmpl: a contiguous ACK_TMPL_DTYPE array"
SND_PLAN = "snd: a writeable contiguous SND_FLOW_DTYPE array"

FLOW, REC, RES = lvlip.LRO_FLOW_DTYPE, lvlip.LRO_REC_DTYPE, lvlip.LRO_RESULT_DTYPE
SND, SRES, FD = lvlip.SND_FLOW_DTYPE, lvlip.SND_RESULT_DTYPE, lvlip.FRAME_DESC_DTYPE


def z(n, dtype=np.uint8):
    return np.zeros(n, dtype=dtype)


def strided(dtype):
    a = z(4, dtype)[::2]
    assert not a.flags.c_contiguous
    return a


def frozen(a):
    a.flags.writeable = False
    return a


def t(nbytes, dtype=torch.uint8):
    """A CPU tensor of nbytes bytes."""
    size = torch.empty(0, dtype=dtype).element_size()
    assert nbytes % size == 0
    return torch.zeros(nbytes // size, dtype=dtype)


def queue(nseg=1, nfd=1, length=0):
    """(snd, fd) of one flow: a queue of nseg entries over nfd descriptors of
    `length` bytes at offset 0."""
    snd, fd = z(1, SND), z(nfd, FD)
    snd["nseg"], fd["len"] = nseg, length
    return snd, fd


def one_send(length=100, mss=50):
    return lvlip.tso_send(tso_template(), 0, length, mss)


class NoStream:
    """Stands in for a stream where a wrapper must refuse before it uses one."""


SND1, FD1 = queue()              # one valid queue of one empty frame
SND_FAR, FD_FAR = queue(2, 1)    # the queue ends past fd
SND_LONG, FD_LONG = queue(1, 1, 17)  # the frame ends past a 16-byte ring

CASES = {
    # ------------------------------------------------------------------ tso --
    "tso_plan dtype": (lambda: lvlip.tso_plan(z(96)), TypeError, TSO_PLAN),
    "tso_plan strided": (lambda: lvlip.tso_plan(strided(lvlip.TsoSend)), TypeError, TSO_PLAN),
    "tso_plan read-only": (lambda: lvlip.tso_plan(frozen(one_send())), TypeError, TSO_PLAN),
    "tso_plan refused": (lambda: lvlip.tso_plan(z(1, lvlip.TsoSend)), ValueError,
                         "malformed send (or more than LVLIP_MAX_BATCH segments)"),
    "tso_cpu plans first": (lambda: lvlip.tso_cpu(z(0), z(96), out=z(1, np.uint16)), TypeError, TSO_PLAN),
    "tso_cpu payload": (lambda: lvlip.tso_cpu(z(99), one_send()), ValueError, "a send reads past the payload"),
    "tso_cpu payload before out": (lambda: lvlip.tso_cpu(z(99), one_send(), out=z(1)), ValueError,
                                   "a send reads past the payload"),
    "tso_cpu out small": (lambda: lvlip.tso_cpu(z(100), one_send(), out=z(2 * 104 - 1)), ValueError, OUT),
    "tso_cpu out dtype": (lambda: lvlip.tso_cpu(z(100), one_send(), out=z(512, np.uint16)), ValueError, OUT),
    "tso_cpu out strided": (lambda: lvlip.tso_cpu(z(100), one_send(), out=z(1024)[::2]), ValueError, OUT),
    "tso_dev fd_t": (lambda: lvlip.tso_dev(t(100), t(96), 2, t(208), t(31), stream=NoStream()), ValueError,
                     "fd_t: 16 bytes per segment"),
    # ------------------------------------------------------------------ lro --
    "lro_plan dtype": (lambda: lvlip.lro_plan(z(48)), TypeError, LRO_PLAN),
    "lro_plan strided": (lambda: lvlip.lro_plan(strided(FLOW)), TypeError, LRO_PLAN),
    "lro_plan read-only": (lambda: lvlip.lro_plan(frozen(z(1, FLOW))), TypeError, LRO_PLAN),
    "lro_plan refused": (lambda: lvlip.lro_plan(z(2, FLOW)), ValueError,
                         "refused flows (duplicate key, window, reserved bytes, overlapping ranges, too many)"),
    "lro_cpu frame": (lambda: lvlip.lro_cpu(z(16), FD_LONG, z(0, FLOW)), ValueError, "a frame lies past the buffer"),
    "lro_cpu frame before out": (lambda: lvlip.lro_cpu(z(16), FD_LONG, z(0, FLOW), out=z(1, np.uint16)), ValueError,
                                 "a frame lies past the buffer"),
    "lro_cpu out small": (lambda: lvlip.lro_cpu(z(16), FD1, lvlip.lro_flow(b"\n\0\0\5", b"\n\0\0\4", 1, 2, 0, 64, 8),
                                                out=z(71)), ValueError, OUT),
    "lro_cpu out dtype": (lambda: lvlip.lro_cpu(z(16), FD1, z(0, FLOW), out=z(8, np.uint16)), ValueError, OUT),
    "lro_dev rec_t": (lambda: lvlip.lro_dev(t(64), t(32), t(48), 0, t(64), t(31)), ValueError,
                      "rec_t: 16 bytes per frame"),
    "lro_dev rec_t by bytes": (lambda: lvlip.lro_dev(t(64), t(32), None, 0, t(64), t(28, torch.int32)), ValueError,
                               "rec_t: 16 bytes per frame"),
    "lro_advance_dev res_t": (lambda: lvlip.lro_advance_dev(t(96), t(16), t(95)), ValueError,
                              "res_t: 48 bytes per flow"),
    "lro_advance_dev res_t, no records": (lambda: lvlip.lro_advance_dev(t(48), None, t(47)), ValueError,
                                          "res_t: 48 bytes per flow"),
    # ------------------------------------------------------------------ ack --
    "ack_plan dtype": (lambda: lvlip.ack_plan(z(64), z(1, FLOW)), TypeError, ACK_PLAN),
    "ack_plan strided": (lambda: lvlip.ack_plan(strided(lvlip.ACK_TMPL_DTYPE), z(2, FLOW)), TypeError, ACK_PLAN),
    "ack_plan dtype before count": (lambda: lvlip.ack_plan(z(64), z(2, FLOW)), TypeError, ACK_PLAN),
    "ack_plan count": (lambda: lvlip.ack_plan(z(1, lvlip.ACK_TMPL_DTYPE), z(2, FLOW)), ValueError,
                       "one template per flow"),
    "ack_plan refused": (lambda: lvlip.ack_plan(z(1, lvlip.ACK_TMPL_DTYPE), z(1, FLOW)), ValueError,
                         "refused templates (header, max_sack, reserved, not the flow's reverse, overlapping slots, "
                         "too many)"),
    "ack_cpu plans first": (lambda: lvlip.ack_cpu(z(1, lvlip.ACK_TMPL_DTYPE), z(2, FLOW), z(1, RES)), ValueError,
                            "one template per flow"),
    "ack_cpu res": (lambda: lvlip.ack_cpu(z(0, lvlip.ACK_TMPL_DTYPE), z(0, FLOW), z(1, RES)), ValueError, ONE_RESULT),
    "ack_cpu res before out": (lambda: lvlip.ack_cpu(z(0, lvlip.ACK_TMPL_DTYPE), z(0, FLOW), z(1, RES),
                                                     out=z(4, np.uint16)), ValueError, ONE_RESULT),
    "ack_cpu out dtype": (lambda: lvlip.ack_cpu(z(0, lvlip.ACK_TMPL_DTYPE), z(0, FLOW), z(0, RES),
                                                out=z(4, np.uint16)), ValueError, OUT),
    "ack_cpu out strided": (lambda: lvlip.ack_cpu(z(0, lvlip.ACK_TMPL_DTYPE), z(0, FLOW), z(0, RES), out=z(8)[::2]),
                            ValueError, OUT),
    "ack_dev tmpl_t": (lambda: lvlip.ack_dev(t(127), t(96), t(96), 0, t(256)), ValueError, "tmpl_t: 64 bytes per flow"),
    "ack_dev tmpl_t before res_t": (lambda: lvlip.ack_dev(t(127), t(96), t(95), 0, t(256), t(31)), ValueError,
                                    "tmpl_t: 64 bytes per flow"),
    "ack_dev res_t": (lambda: lvlip.ack_dev(t(128), t(96), t(95), 0, t(256)), ValueError, "res_t: 48 bytes per flow"),
    "ack_dev res_t before fd_t": (lambda: lvlip.ack_dev(t(128), t(96), t(95), 0, t(256), t(31)), ValueError,
                                  "res_t: 48 bytes per flow"),
    "ack_dev fd_t": (lambda: lvlip.ack_dev(t(128), t(96), t(96), 0, t(256), t(31)), ValueError,
                     "fd_t: 16 bytes per flow"),
    # ------------------------------------------------------------------ snd --
    "snd_plan dtype": (lambda: lvlip.snd_plan(z(32)), TypeError, SND_PLAN),
    "snd_plan strided": (lambda: lvlip.snd_plan(strided(SND)), TypeError, SND_PLAN),
    "snd_plan read-only": (lambda: lvlip.snd_plan(frozen(z(1, SND))), TypeError, SND_PLAN),
    "snd_plan refused": (lambda: lvlip.snd_plan(np.array([(0, 0, 0, 0, 0, 0, 0, 1, 0)], dtype=SND)), ValueError,
                         "refused send sides (reserved bytes, snd_nxt - snd_una, overlapping queues, too many)"),
    "snd_cpu count": (lambda: lvlip.snd_cpu(z(2, FLOW), SND1, z(0, REC), z(16), FD1), ValueError, ONE_SEND_SIDE),
    "snd_cpu count before queue": (lambda: lvlip.snd_cpu(z(2, FLOW), SND_FAR, z(0, REC), z(16), FD_FAR), ValueError,
                                   ONE_SEND_SIDE),
    "snd_cpu queue": (lambda: lvlip.snd_cpu(z(1, FLOW), SND_FAR, z(0, REC), z(16), FD_FAR), ValueError, PAST_FD),
    "snd_cpu queue before frame": (lambda: lvlip.snd_cpu(z(1, FLOW), SND_FAR, z(0, REC), z(16), FD_LONG), ValueError,
                                   PAST_FD),
    "snd_cpu frame": (lambda: lvlip.snd_cpu(z(1, FLOW), SND_LONG, z(0, REC), z(16), FD_LONG), ValueError, PAST_RING),
    "snd_cpu frame, bytes ring": (lambda: lvlip.snd_cpu(z(1, FLOW), SND_LONG, z(0, REC), bytes(16), FD_LONG),
                                  ValueError, PAST_RING),
    "snd_dev snd_t": (lambda: lvlip.snd_dev(t(96), t(63), t(16), t(64), t(16)), ValueError, "snd_t: 32 bytes per flow"),
    "snd_dev snd_t by bytes": (lambda: lvlip.snd_dev(t(48), t(28, torch.int32), None, t(64), t(16)), ValueError,
                               "snd_t: 32 bytes per flow"),
    "snd_dev snd_t before res_t": (lambda: lvlip.snd_dev(t(96), t(63), t(16), t(64), t(16), t(63)), ValueError,
                                   "snd_t: 32 bytes per flow"),
    "snd_dev res_t": (lambda: lvlip.snd_dev(t(96), t(64), t(16), t(64), t(16), t(63)), ValueError,
                      "res_t: 32 bytes per flow"),
    # ------------------------------------------------------------------ rtx --
    "rtx_cpu count": (lambda: lvlip.rtx_cpu(z(2, FLOW), None, SND1, None, z(16), FD1), ValueError, ONE_SEND_SIDE),
    "rtx_cpu count before base": (lambda: lvlip.rtx_cpu(z(2, FLOW), None, SND1, None, bytes(16), FD1), ValueError,
                                  ONE_SEND_SIDE),
    "rtx_cpu base bytes": (lambda: lvlip.rtx_cpu(z(1, FLOW), None, SND1, None, bytearray(16), FD1), TypeError, BASE),
    "rtx_cpu base dtype": (lambda: lvlip.rtx_cpu(z(1, FLOW), None, SND1, None, z(16, np.int8), FD1), TypeError, BASE),
    "rtx_cpu base strided": (lambda: lvlip.rtx_cpu(z(1, FLOW), None, SND1, None, z(32)[::2], FD1), TypeError, BASE),
    "rtx_cpu base read-only": (lambda: lvlip.rtx_cpu(z(1, FLOW), None, SND1, None, frozen(z(16)), FD1), TypeError,
                               BASE),
    "rtx_cpu base before queue": (lambda: lvlip.rtx_cpu(z(1, FLOW), None, SND_FAR, None, frozen(z(16)), FD_FAR),
                                  TypeError, BASE),
    "rtx_cpu queue": (lambda: lvlip.rtx_cpu(z(1, FLOW), None, SND_FAR, None, z(16), FD_FAR), ValueError, PAST_FD),
    "rtx_cpu frame": (lambda: lvlip.rtx_cpu(z(1, FLOW), None, SND_LONG, None, z(16), FD_LONG), ValueError, PAST_RING),
    "rtx_cpu frame before results": (lambda: lvlip.rtx_cpu(z(1, FLOW), z(2, RES), SND_LONG, None, z(16), FD_LONG),
                                     ValueError, PAST_RING),
    "rtx_cpu lro_res": (lambda: lvlip.rtx_cpu(z(1, FLOW), z(2, RES), SND1, None, z(16), FD1), ValueError, ONE_RESULT),
    "rtx_cpu snd_res": (lambda: lvlip.rtx_cpu(z(1, FLOW), z(1, RES), SND1, z(0, SRES), z(16), FD1), ValueError,
                        ONE_RESULT),
    "rtx_dev snd_t": (lambda: lvlip.rtx_dev(t(96), t(95), t(63), t(63), 2, t(64), t(16), t(31)), ValueError,
                      "snd_t: 32 bytes per flow"),
    "rtx_dev lro_res_t": (lambda: lvlip.rtx_dev(t(96), t(95), t(64), t(63), 2, t(64), t(16), t(31)), ValueError,
                          "lro_res_t: 48 bytes per flow"),
    "rtx_dev snd_res_t": (lambda: lvlip.rtx_dev(t(96), t(96), t(64), t(63), 2, t(64), t(16), t(31)), ValueError,
                          "snd_res_t: 32 bytes per flow"),
    "rtx_dev snd_res_t alone": (lambda: lvlip.rtx_dev(t(96), None, t(64), t(63), 2, t(64), t(16)), ValueError,
                                "snd_res_t: 32 bytes per flow"),
    "rtx_dev fd_out_t": (lambda: lvlip.rtx_dev(t(96), t(96), t(64), t(64), 2, t(64), t(16), t(31)), ValueError,
                         "fd_out_t: 16 bytes per slot"),
    "rtx_dev fd_out_t, no results": (lambda: lvlip.rtx_dev(t(96), None, t(64), None, 2, t(64), t(16), t(31)),
                                     ValueError, "fd_out_t: 16 bytes per slot"),
    # ----------------------------------------------------------------- sack --
    "sack_cpu count": (lambda: lvlip.sack_cpu(z(2, FLOW), SND1, z(0, REC), z(16), z(0, FD), z(16), FD1, bytes(1)),
                       ValueError, ONE_SEND_SIDE),
    "sack_cpu sacked bytes": (lambda: lvlip.sack_cpu(z(1, FLOW), SND1, z(0, REC), z(16), z(0, FD), z(16), FD1,
                                                     bytearray(1)), TypeError, SACKED),
    "sack_cpu sacked dtype": (lambda: lvlip.sack_cpu(z(1, FLOW), SND1, z(0, REC), z(16), z(0, FD), z(16), FD1,
                                                     z(1, np.bool_)), TypeError, SACKED),
    "sack_cpu sacked strided": (lambda: lvlip.sack_cpu(z(1, FLOW), SND1, z(0, REC), z(16), z(0, FD), z(16), FD1,
                                                       z(4)[::2]), TypeError, SACKED),
    "sack_cpu sacked read-only": (lambda: lvlip.sack_cpu(z(1, FLOW), SND1, z(0, REC), z(16), z(0, FD), z(16), FD1,
                                                         frozen(z(1))), TypeError, SACKED),
    "sack_cpu sacked before queue": (lambda: lvlip.sack_cpu(z(1, FLOW), SND_FAR, z(0, REC), z(16), z(0, FD), z(16),
                                                            FD_FAR, frozen(z(1))), TypeError, SACKED),
    "sack_cpu queue": (lambda: lvlip.sack_cpu(z(1, FLOW), SND_FAR, z(0, REC), z(16), z(0, FD), z(16), FD_FAR, z(0)),
                       ValueError, PAST_FD),
    "sack_cpu frame before sacked size": (lambda: lvlip.sack_cpu(z(1, FLOW), SND_LONG, z(0, REC), z(16), z(0, FD),
                                                                 z(16), FD_LONG, z(0)), ValueError, PAST_RING),
    "sack_cpu sacked size": (lambda: lvlip.sack_cpu(z(1, FLOW), SND1, z(1, REC), z(16), z(0, FD), z(16), FD1, z(0)),
                             ValueError, SACKED_SIZE),
    "sack_cpu ack count": (lambda: lvlip.sack_cpu(z(1, FLOW), SND1, z(1, REC), z(16), FD_LONG[:0], z(16), FD1, z(1)),
                           ValueError, "one record per ACK frame"),
    "sack_cpu ack count before ack frame": (lambda: lvlip.sack_cpu(z(1, FLOW), SND1, z(2, REC), z(16), FD_LONG, z(16),
                                                                   FD1, z(1)), ValueError, "one record per ACK frame"),
    "sack_cpu ack frame": (lambda: lvlip.sack_cpu(z(1, FLOW), SND1, z(1, REC), bytes(16), FD_LONG, z(16), FD1, z(1)),
                           ValueError, "an ACK frame lies past ack_base"),
    "sack_dev snd_t": (lambda: lvlip.sack_dev(t(96), t(63), t(32), t(64), t(31), t(64), t(16), t(1), t(15)),
                       ValueError, "snd_t: 32 bytes per flow"),
    "sack_dev ack_fd_t": (lambda: lvlip.sack_dev(t(96), t(64), t(32), t(64), t(31), t(64), t(16), t(1), t(15)),
                          ValueError, "ack_fd_t: 16 bytes per record"),
    "sack_dev res_t": (lambda: lvlip.sack_dev(t(96), t(64), t(32), t(64), t(32), t(64), t(16), t(1), t(31)),
                       ValueError, "res_t: 16 bytes per flow"),
    "sack_dev res_t, no records": (lambda: lvlip.sack_dev(t(96), t(64), None, None, None, t(64), t(16), t(1), t(31)),
                                   ValueError, "res_t: 16 bytes per flow"),
    # ------------------------------------------------------------- rtx_sack --
    "rtx_sack_cpu count": (lambda: lvlip.rtx_sack_cpu(z(2, FLOW), None, SND1, None, None, bytes(16), FD1), ValueError,
                           ONE_SEND_SIDE),
    "rtx_sack_cpu base": (lambda: lvlip.rtx_sack_cpu(z(1, FLOW), None, SND_FAR, None, None, frozen(z(16)), FD_FAR),
                          TypeError, BASE),
    "rtx_sack_cpu queue": (lambda: lvlip.rtx_sack_cpu(z(1, FLOW), None, SND_FAR, None, z(0), z(16), FD_FAR),
                           ValueError, PAST_FD),
    "rtx_sack_cpu frame": (lambda: lvlip.rtx_sack_cpu(z(1, FLOW), None, SND_LONG, None, z(0), z(16), FD_LONG),
                           ValueError, PAST_RING),
    "rtx_sack_cpu sacked size": (lambda: lvlip.rtx_sack_cpu(z(1, FLOW), z(2, RES), SND1, None, z(0), z(16), FD1),
                                 ValueError, SACKED_SIZE),
    "rtx_sack_cpu lro_res": (lambda: lvlip.rtx_sack_cpu(z(1, FLOW), z(2, RES), SND1, None, [0], z(16), FD1),
                             ValueError, ONE_RESULT),
    "rtx_sack_cpu snd_res": (lambda: lvlip.rtx_sack_cpu(z(1, FLOW), None, SND1, z(2, SRES), None, z(16), FD1),
                             ValueError, ONE_RESULT),
    "rtx_sack_dev snd_t": (lambda: lvlip.rtx_sack_dev(t(96), t(95), t(63), t(63), None, 2, t(64), t(16), t(31), t(7)),
                           ValueError, "snd_t: 32 bytes per flow"),
    "rtx_sack_dev lro_res_t": (lambda: lvlip.rtx_sack_dev(t(96), t(95), t(64), t(63), None, 2, t(64), t(16), t(31),
                                                          t(7)), ValueError, "lro_res_t: 48 bytes per flow"),
    "rtx_sack_dev snd_res_t": (lambda: lvlip.rtx_sack_dev(t(96), t(96), t(64), t(63), t(1), 2, t(64), t(16), t(31),
                                                          t(7)), ValueError, "snd_res_t: 32 bytes per flow"),
    "rtx_sack_dev fd_out_t": (lambda: lvlip.rtx_sack_dev(t(96), t(96), t(64), t(64), t(1), 2, t(64), t(16), t(31),
                                                         t(7)), ValueError, "fd_out_t: 16 bytes per slot"),
    "rtx_sack_dev pick_t": (lambda: lvlip.rtx_sack_dev(t(96), None, t(64), None, None, 2, t(64), t(16), t(32), t(7)),
                            ValueError, "pick_t: 4 bytes per slot"),
    "rtx_sack_dev pick_t alone": (lambda: lvlip.rtx_sack_dev(t(96), None, t(64), None, None, 2, t(64), t(16), None,
                                                             t(7)), ValueError, "pick_t: 4 bytes per slot"),
}


@pytest.mark.parametrize("name", CASES)
def test_refusal(name):
    call, exc, text = CASES[name]
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc and str(e.value) == text


def test_the_inputs_are_left_as_they_were():
    """The shared arrays of the table: no refusal wrote to them."""
    for a, b in ((SND1, queue()[0]), (FD1, queue()[1]), (SND_FAR, queue(2, 1)[0]), (FD_LONG, queue(1, 1, 17)[1])):
        assert a.tobytes() == b.tobytes()


def test_the_module_serves_the_cpu_calls_without_torch():
    """`import torch` stays inside the device wrappers."""
    import ast
    import inspect

    tree = ast.parse(inspect.getsource(lvlip))
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert "torch" not in {a.name.split(".")[0] for n in top if isinstance(n, ast.Import) for a in n.names}
    assert "torch" not in {(n.module or "").split(".")[0] for n in top if isinstance(n, ast.ImportFrom)}
