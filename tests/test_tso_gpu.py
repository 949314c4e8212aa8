"""lvlip_tso_dev on the MI355X: the frames of the fused segmentation kernel
(seg_kernels.hip) against the independent builder of tests/test_tso_cpu.py,
whole buffers compared (0xA5 canary everywhere outside the frames), over every
case of the shape list; against the reference's own tcp_send frames; through
lvlip_tx_checksum_dev with the descriptors it returns; and on a stream of the
caller's."""
import numpy as np
import pytest
import torch

import devbuf
import lvlip
from test_tso_cpu import (ALL_CASES, CANARY, assert_same, fixture, fixture_case, fixture_frames, multi_case,
                          parity_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


def run_dev(case, dev, stream=None, with_fd=True):
    """One lvlip_tso_dev call on fresh device buffers.  Returns (out, fd,
    payload afterwards) as numpy arrays, plus the device tensors."""
    payload_t = torch.from_numpy(case.payload).to(dev)
    sends_t = torch.from_numpy(case.sends.view(np.uint8).reshape(-1).copy()).to(dev)
    out_t = torch.full((case.out_size,), CANARY, dtype=torch.uint8, device=dev)
    fd_t = torch.full((16 * case.nseg,), 0x5A, dtype=torch.uint8, device=dev) if with_fd else None
    torch.cuda.synchronize(dev)
    lvlip.tso_dev(payload_t, sends_t, case.nseg, out_t, fd_t, stream=stream)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize(dev)
    fd = fd_t.cpu().numpy().view(lvlip.FRAME_DESC_DTYPE) if with_fd else None
    return out_t.cpu().numpy(), fd, payload_t.cpu().numpy(), (out_t, fd_t)


@pytest.mark.parametrize("make", ALL_CASES)
def test_tso_dev_equals_builder(make, dev):
    case = make()
    out, fd, payload, (out_t, fd_t) = run_dev(case, dev)
    assert_same(out, case.want, case.spans, case.name)
    assert np.array_equal(fd, case.fd), case.name
    assert np.array_equal(payload, case.payload), "the payload is only read"
    # the frames are complete: the in-place TX fill finds nothing to change
    status = lvlip.tx_checksum_dev(out_t, fd_t.view(torch.uint8))
    torch.cuda.synchronize(dev)
    assert int(status.sum()) == case.nseg and bool((status == 1).all())
    assert_same(out_t.cpu().numpy(), case.want, case.spans, case.name + " after lvlip_tx_checksum_dev")


def test_tso_dev_equals_tso_cpu(dev):
    for case in (parity_case(), multi_case()):
        cpu = np.full(case.out_size, CANARY, dtype=np.uint8)
        cpu, cfd = lvlip.tso_cpu(case.payload, case.sends, out=cpu)
        out, fd, _, _ = run_dev(case, dev)
        assert_same(out, cpu, case.spans, case.name + " (device against CPU form)")
        assert np.array_equal(fd, cfd)


def test_tso_dev_reproduces_the_reference_frames(dev):
    case = fixture_case()
    out, _, _, _ = run_dev(case, dev)
    for k, (s, frames) in enumerate(zip(fixture()["sends"], fixture_frames(case, out))):
        assert len(frames) == len(s["frames"])
        for i, (a, b) in enumerate(zip(frames, s["frames"])):
            assert a.hex() == b, f"send {k} ({s['len']} B), segment {i}"


def test_tso_dev_on_a_callers_stream(dev):
    case = multi_case()
    stream = torch.cuda.Stream(dev)
    out, fd, payload, _ = run_dev(case, dev, stream=stream)
    assert_same(out, case.want, case.spans, case.name + " on a non-default stream")
    assert np.array_equal(fd, case.fd)
    assert np.array_equal(payload, case.payload)


def test_tso_dev_without_descriptors(dev):
    case = multi_case()
    out, _, _, _ = run_dev(case, dev, with_fd=False)
    assert_same(out, case.want, case.spans, case.name + " (fd NULL)")
