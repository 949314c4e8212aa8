"""The peer's window on the MI355X (k_wnd_rec, k_wnd_fin, rto_kernels.hip):
every byte of res, t and w of lvlip_wnd_dev against lvlip_wnd_cpu, at the
record and flow counts where the kernels change path (a partial wave, more
than one workgroup, all records of one flow: the peel; more than four flows in
every wave: the pending lanes), with ACK frames at every address mod 4 so the
window's dword straddles a boundary, and determinism."""
import numpy as np
import pytest
import torch

import devbuf
import lvlip
from devbuf import _t, guarded, unguard
from test_wnd_cpu import NONE, pack, random_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return devbuf.device()


def run_dev(dev, f, s, t, w, rec, buf, fd, flags, shift=0):
    """lvlip_wnd_dev on copies; ack_base starts `shift` bytes into its tensor."""
    n = f.size
    f_t, s_t = _t(f, dev), _t(s, dev)
    t_t, w_t = torch.cat([_t(t, dev), guarded(0, dev)]), torch.cat([_t(w, dev), guarded(0, dev)])
    rec_t, fd_t = _t(rec, dev), _t(fd, dev)
    buf_t = _t(np.concatenate([np.zeros(shift, dtype=np.uint8), buf]), dev)[shift:]
    res_t = guarded(16 * n, dev)
    torch.cuda.synchronize(dev)
    lvlip.wnd_dev(f_t, s_t, t_t, w_t, rec_t if rec.size else None, buf_t, fd_t, flags, res_t)
    torch.cuda.synchronize(dev)
    assert np.array_equal(f_t.cpu().numpy(), f.view(np.uint8).reshape(-1)), "f is only read"
    assert np.array_equal(s_t.cpu().numpy(), s.view(np.uint8).reshape(-1)), "s is only read"
    return (unguard(res_t, 16 * n, lvlip.WND_RESULT_DTYPE), unguard(t_t, t.nbytes, lvlip.RTO_FLOW_DTYPE),
            unguard(w_t, w.nbytes, lvlip.PUSH_FLOW_DTYPE))


def run_cpu(f, s, t, w, rec, buf, fd, flags):
    t, w = t.copy(), w.copy()
    return lvlip.wnd_cpu(f, s, t, w, rec, buf, fd, flags), t, w


def check(dev, n, nflows, flags=lvlip.WND_APPLY, one_flow=False, base_mod=None, shift=0, seed=0):
    f, s, t, w, rec, frames = random_case(n, nflows, seed=seed + n + nflows, one_flow=one_flow)
    buf, fd = pack(frames, seed, base_mod)
    want = run_cpu(f, s, t, w, rec, buf, fd, flags)
    got = run_dev(dev, f, s, t, w, rec, buf, fd, flags, shift)
    for g, x, name in zip(got, want, ("res", "t", "w")):
        assert g.tobytes() == x.tobytes(), (name, n, nflows)
    return want


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 1000))
def test_record_counts(n, dev):
    for nflows in (1, 5, 257):
        check(dev, n, nflows)


@pytest.mark.parametrize("nflows", (1, 3, 4, 5, 63, 64, 65, 257))
def test_flow_counts(nflows, dev):
    check(dev, 1000, nflows, flags=0)
    check(dev, 1000, nflows, flags=lvlip.WND_APPLY, seed=1)


def test_all_records_of_one_flow_and_many_flows_in_every_wave(dev):
    res = check(dev, 1000, 3, one_flow=True)[0]
    assert res["n_counting"][0] > 200 and res["winner"][1] == NONE  # the peel path: one flow a wave
    res = check(dev, 1000, 257)[0]
    assert (res["n_counting"] > 0).sum() > 200  # far more than four flows among a wave's 64 records: pending lanes


@pytest.mark.parametrize("mod", (0, 1, 2, 3))
def test_every_address_mod_4(mod, dev):
    """Every frame at `mod` mod 4 and the buffer itself shifted: the dwords at
    14 and at 14 + ihl*4 + 12 are aligned for some frames and straddle a
    boundary for the others; ihl 5..8 moves the second against the first."""
    for shift in (0, 1, 2, 3):
        check(dev, 300, 9, base_mod=mod, shift=shift, seed=mod)


def test_determinism(dev):
    f, s, t, w, rec, frames = random_case(1000, 7, seed=5)
    buf, fd = pack(frames)
    a = run_dev(dev, f, s, t, w, rec, buf, fd, lvlip.WND_APPLY)
    b = run_dev(dev, f, s, t, w, rec, buf, fd, lvlip.WND_APPLY)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_misaligned_pointers_are_refused_before_any_launch(dev):
    f, s, t, w, rec, frames = random_case(10, 2, seed=1)
    buf, fd = pack(frames)
    ten = [_t(a, dev) for a in (f, s, t, w, rec, buf, fd)]
    res = torch.zeros(64, dtype=torch.uint8, device=dev)
    p = [x.data_ptr() for x in ten]
    ok = (p[0], p[1], p[2], p[3], 2, p[4], p[5], p[6], 10, 1, res.data_ptr(), None)
    for i, off in ((0, 4), (1, 4), (2, 4), (3, 4), (5, 8), (7, 8), (10, 8)):
        bad = list(ok)
        bad[i] += off
        assert lvlip.lib().lvlip_wnd_dev(*bad) == lvlip.EINVAL, i
    torch.cuda.synchronize(dev)
    assert not res.any().item() and np.array_equal(ten[2].cpu().numpy(), t.view(np.uint8).reshape(-1))
