"""Device buffers of the GPU tests: the device itself, numpy arrays copied to
it as bytes, and outputs with canary bytes behind them."""
import numpy as np
import pytest
import torch

import lvlip

CANARY = 0x5A
GUARD = 64           # canary bytes behind guarded()
ALIGNED_GUARD = 256  # and behind guarded_aligned()


def device():
    """cuda:0; the gpu tests fail, not skip, without a HIP device."""
    if not torch.cuda.is_available() or lvlip.device_count() == 0:
        pytest.fail("the gpu tests need a HIP device")
    return torch.device("cuda", 0)


def _t(a: np.ndarray, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def guarded(nbytes: int, dev):
    return torch.full((nbytes + GUARD,), CANARY, dtype=torch.uint8, device=dev)


def guarded_aligned(nbytes: int, dev):
    """A 256-B aligned tensor of nbytes + ALIGNED_GUARD canary bytes."""
    t = torch.full((nbytes + ALIGNED_GUARD + 256,), CANARY, dtype=torch.uint8, device=dev)
    skip = -t.data_ptr() % 256
    return t[skip:skip + nbytes + ALIGNED_GUARD]


def unguard(t, nbytes: int, dtype):
    a = t.cpu().numpy()
    assert (a[nbytes:] == CANARY).all(), "written behind the output"
    return a[:nbytes].view(dtype)
