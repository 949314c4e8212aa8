"""lvlip_lro_dev on the MI355X: the records and the stream bytes of the fused
receive kernel (rcv_kernels.hip) against the independent model of
tests/test_lro_cpu.py and against lvlip_lro_cpu, whole buffers compared (0xA5
canary everywhere outside the placed payloads), for every batch size and flow
count crossed with frame alignment, stream alignment and both flag values;
against the reference's own tcp_data_dequeue bytes; behind lvlip_tso_dev on a
stream of the caller's; and the rule that a frame whose checksum fails never
stores a byte."""
import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import _t
from test_lro_cpu import (CANARY, FLOW_COUNTS, FRAME_MODS, N_LIST, OUT_MODS, assert_same_out, assert_same_rec, case,
                          expected, fixture_inputs, flow_kw, model_advance, plan_flows, result_tuples, tcp_frame)
from test_tso_cpu import template as tso_template

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


def run_dev(buf, fd, flows, flags, out_size, dev, stream=None):
    """One lvlip_lro_dev call on fresh device buffers -> (out, rec, frames afterwards)."""
    buf_t, fd_t, fl_t = _t(buf, dev), _t(fd, dev), _t(flows, dev)
    out_t = torch.full((out_size,), CANARY, dtype=torch.uint8, device=dev)
    rec_t = torch.full((16 * max(len(fd), 1),), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    lvlip.lro_dev(buf_t, fd_t, fl_t, flags, out_t, rec_t, stream=stream)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    return out_t.cpu().numpy(), rec_t.cpu().numpy().view(lvlip.LRO_REC_DTYPE)[:len(fd)], buf_t.cpu().numpy()


@pytest.mark.parametrize("nflows", FLOW_COUNTS)
@pytest.mark.parametrize("n", N_LIST)
def test_lro_dev_equals_model_and_cpu(n, nflows, dev):
    c = case(n, nflows)
    for flags in (0, lvlip.RX_VERIFY_L4):
        for fmod in FRAME_MODS:
            for omod in OUT_MODS:
                what = f"n {n}, {nflows} flows, flags {flags}, frames at {fmod}, out at {omod}"
                buf, fd, flows, out_size = c.laid_out(fmod, omod)
                want_out, want_rec = expected(n, nflows, flags, omod)
                out, rec, after = run_dev(buf, fd, flows, flags, out_size, dev)
                assert_same_rec(rec, want_rec, what)
                assert_same_out(out, want_out, what)
                assert np.array_equal(after, buf), "the frames are only read"
                if fmod == omod % 2:  # the CPU form is alignment-blind: a sample is enough
                    cpu = np.full(out_size, CANARY, dtype=np.uint8)
                    cpu, crec = lvlip.lro_cpu(buf, fd, flows, flags, out=cpu)
                    assert_same_rec(rec, crec, what + " (device against CPU form)")
                    assert_same_out(out, cpu, what + " (device against CPU form)")


def test_lro_dev_without_flows(dev):
    c = case(17, 3)
    buf, fd, flows, out_size = c.laid_out(1, 7)
    out, rec, _ = run_dev(buf, fd, flows[:0], lvlip.RX_VERIFY_L4, out_size, dev)
    _, crec = lvlip.lro_cpu(buf, fd, flows[:0], lvlip.RX_VERIFY_L4)
    assert (out == CANARY).all() and np.array_equal(rec, crec)
    assert (rec["status"] == lvlip.LRO_NO_FLOW).any() and not (rec["status"] == lvlip.LRO_PLACED).any()


def test_lro_dev_segments_beyond_the_kept_sweeps(dev):
    """Jumbo segments: what the registers do not keep until the verdict is read
    a second time; every stream alignment, good and bad checksums."""
    flows = plan_flows(1, 40000, 0)
    stream = np.random.default_rng(8).integers(0, 256, 40000, dtype=np.uint8)
    nxt, kw = int(flows[0]["rcv_nxt"]), flow_kw(flows[0])
    cuts = [0, 8946, 8946 + 1537, 8946 + 1537 + 4000, 8946 + 1537 + 4000 + 1521, 30000]
    frs = [tcp_frame(stream[a:b].tobytes(), nxt + a, **kw) for a, b in zip(cuts[:-1], cuts[1:])]
    frs.append(tcp_frame(bytes(9000), nxt + 30000, l4_ok=False, **kw))
    for omod in OUT_MODS:
        fl = flows.copy()
        fl["out_off"] += omod
        buf, fd = lvlip.pack_frames(frs, align_mod=16, seed=omod)
        size = lvlip.lro_plan(fl) + 32
        for flags in (0, lvlip.RX_VERIFY_L4):
            cpu = np.full(size, CANARY, dtype=np.uint8)
            cpu, crec = lvlip.lro_cpu(buf, fd, fl, flags, out=cpu)
            out, rec, _ = run_dev(buf, fd, fl, flags, size, dev)
            assert_same_rec(rec, crec, f"jumbo, out at {omod}, flags {flags}")
            assert_same_out(out, cpu, f"jumbo, out at {omod}, flags {flags}")
            o = int(fl[0]["out_off"])
            assert np.array_equal(out[o:o + 30000], stream[:30000])
            assert int(rec[-1]["status"]) == (lvlip.RX_BAD_L4 if flags else lvlip.LRO_PLACED)


def test_lro_dev_reproduces_the_reference_stream(dev):
    fx, buf, fd, flow = fixture_inputs()
    size = lvlip.lro_plan(flow) + 32
    out, rec, _ = run_dev(buf, fd, flow, lvlip.RX_VERIFY_L4, size, dev)
    res = lvlip.lro_advance(flow, rec)[0]
    assert int(res["delivered"]) == fx["count"]
    assert out[3:3 + fx["count"]].tobytes().hex() == fx["dequeued_hex"]


@pytest.mark.parametrize("mss", (1, 15, 16, 17, 536, 1460, 8946))
def test_tso_dev_into_lro_dev_on_a_callers_stream(mss, dev):
    """Payload -> frames -> payload, both kernels on one non-default stream,
    the frame descriptors never leaving the device (their order shuffled by a
    gather on that stream)."""
    rng = np.random.default_rng(mss)
    length = {1: 40, 15: 200, 16: 200, 17: 200}.get(mss, 5 * mss + 3)
    payload = rng.integers(0, 256, length, dtype=np.uint8)
    hdr = tso_template(seq=0xFFFFFF00)
    sends = lvlip.tso_send(hdr, 0, length, mss, out_off=5, stride=54 + mss + 3)
    nseg, ring_bytes = lvlip.tso_plan(sends)
    flow = lvlip.lro_flow(hdr[26:30], hdr[30:34], 40001, 8000, 0xFFFFFF00, 1 << 16, out_off=7)
    size = lvlip.lro_plan(flow) + 32
    order = rng.permutation(nseg)
    order = np.concatenate([order, order[:max(1, nseg // 3)]])
    stream = torch.cuda.Stream(dev)
    pay_t, sends_t, fl_t = _t(payload, dev), _t(sends, dev), _t(flow, dev)
    order_t = torch.from_numpy(order).to(dev)
    ring_t = torch.zeros((ring_bytes + 15 & ~15) + 16, dtype=torch.uint8, device=dev)
    fd_t = torch.zeros((nseg, 16), dtype=torch.uint8, device=dev)
    out_t = torch.full((size,), CANARY, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        lvlip.tso_dev(pay_t, sends_t, nseg, ring_t, fd_t, stream=stream)
        shuffled = fd_t[order_t].contiguous()
        rec_t = lvlip.lro_dev(ring_t, shuffled, fl_t, lvlip.RX_VERIFY_L4, out_t, stream=stream)
    stream.synchronize()
    rec = rec_t.cpu().numpy().view(lvlip.LRO_REC_DTYPE)[:order.size]
    out = out_t.cpu().numpy()
    assert (rec["status"] == lvlip.LRO_PLACED).all()
    res = lvlip.lro_advance(flow, rec)[0]
    assert int(res["delivered"]) == length and int(res["nsack"]) == 0
    assert np.array_equal(out[7:7 + length], payload)
    assert (out[:7] == CANARY).all() and (out[7 + length:] == CANARY).all()


@pytest.mark.parametrize("bad_first", (False, True))
def test_a_frame_that_fails_its_checksum_stores_nothing(bad_first, dev):
    """A retransmit of segment 2 with other payload bytes and a checksum field
    that cannot verify, behind the good segment and in front of it: out keeps
    the good bytes, the frame is BAD_L4, advance ignores it."""
    flows = plan_flows(1, 8192, 7)
    nxt, kw = int(flows[0]["rcv_nxt"]), flow_kw(flows[0])
    stream = np.random.default_rng(3).integers(0, 256, 5 * 1460, dtype=np.uint8)
    good = [tcp_frame(stream[k * 1460:(k + 1) * 1460].tobytes(), nxt + k * 1460, **kw) for k in range(5)]
    forged = tcp_frame((stream[2 * 1460:3 * 1460] ^ 0xFF).tobytes(), nxt + 2 * 1460, l4_ok=False, **kw)
    frs = good[:2] + ([forged, good[2]] if bad_first else [good[2], forged]) + good[3:]
    bad_at = 2 if bad_first else 3
    size = lvlip.lro_plan(flows) + 32
    for fmod in (0, 1):
        buf, fd = lvlip.pack_frames(frs, align_mod=1, seed=0)
        if fmod:
            buf = np.concatenate([np.zeros(16, dtype=np.uint8), buf])[15:]
            buf = np.concatenate([buf, np.zeros(-buf.size % 16 + 16, dtype=np.uint8)])
            fd["offset"] += 1
        out, rec, _ = run_dev(buf, fd, flows, lvlip.RX_VERIFY_L4, size, dev)
        assert int(rec[bad_at]["status"]) == lvlip.RX_BAD_L4
        assert [int(s) for i, s in enumerate(rec["status"]) if i != bad_at] == [lvlip.LRO_PLACED] * 5
        o = int(flows[0]["out_off"])
        assert np.array_equal(out[o:o + stream.size], stream)
        assert (out[:o] == CANARY).all() and (out[o + stream.size:] == CANARY).all()
        res = lvlip.lro_advance(flows, rec)
        assert result_tuples(res) == model_advance(flows, rec) == [(stream.size, 5, [])]
