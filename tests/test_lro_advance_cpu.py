"""lvlip_lro_advance_dev (include/lvlip_skb.h, adv_kernels.hip) without a GPU:
the two entry points are exported and bound, every refusal the header lists
happens before any HIP call, and the hand-written k_adv_* kernels compile for
gfx950 without scratch.  What the kernels compute is tests/test_lro_advance_gpu.py's."""
import os
import re
import subprocess

import numpy as np

import lvlip
from test_lro_cpu import case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_bound():
    L = lvlip.lib()
    for name in ("lvlip_lro_advance_workspace_bytes", "lvlip_lro_advance_dev"):
        assert name in lvlip.SIGNATURES
        assert getattr(L, name).argtypes == lvlip.SIGNATURES[name][1]
    assert callable(lvlip.lro_advance_dev) and callable(lvlip.lro_advance_workspace_bytes)
    assert L.lvlip_abi_version() == 2


def test_refusals_without_gpu():
    """Host memory stands in for the device pointers: a refused call touches
    none of it and makes no HIP call."""
    L = lvlip.lib()
    c = case(16, 3)
    buf, fd, flows, _ = c.laid_out(0, 0)
    _, rec = lvlip.lro_cpu(buf, fd, flows)
    res = np.full(3 * 48 + 16, 0x5A, dtype=np.uint8)
    ws = np.zeros(1 << 16, dtype=np.uint8)
    f, r, o = flows.ctypes.data, rec.ctypes.data, res.ctypes.data
    o += -o % 16
    w = ws.ctypes.data
    w += -w % 256
    assert f % 8 == 0 and r % 16 == 0
    size = 1 << 15
    refused = {"NULL f": (None, 3, r, 16, o, w, size), "NULL res": (f, 3, r, 16, None, w, size),
               "NULL rec": (f, 3, None, 16, o, w, size), "n above LVLIP_MAX_BATCH": (f, 3, r, 0xFFFFFFF1, o, w, size),
               "nflows above LVLIP_LRO_MAX_FLOWS": (f, 65537, r, 16, o, w, size),
               "NULL workspace": (f, 3, r, 16, o, None, size), "workspace at 128 mod 256": (f, 3, r, 16, o, w + 128, size),
               "workspace at 16 mod 256": (f, 3, r, 16, o, w + 16, size)}
    for what, args in refused.items():
        assert L.lvlip_lro_advance_dev(*args, None) == lvlip.EINVAL, what
    assert (res == 0x5A).all() and not ws.any()
    # no flows: nothing to report, whatever else is given
    assert L.lvlip_lro_advance_dev(None, 0, None, 0, None, None, 0, None) == lvlip.OK
    assert L.lvlip_lro_advance_dev(None, 0, r, 16, None, None, 0, None) == lvlip.OK
    assert L.lvlip_lro_advance_dev(f, 0, r, 16, o, w, size, None) == lvlip.OK
    assert (res == 0x5A).all() and not ws.any()
    assert L.lvlip_lro_advance_workspace_bytes(0, 3) == 0


def test_adv_kernels_use_no_scratch(tmp_path):
    """Every hand-written kernel of adv_kernels.hip (k_adv_*; rocPRIM's are its
    own) has a private segment of 0."""
    asm = tmp_path / "adv_kernels.s"
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    "-S", "--cuda-device-only", os.path.join(ROOT, "level-ip_amd", "csrc", "adv_kernels.hip"),
                    "-o", str(asm)], check=True, capture_output=True)
    text = asm.read_text()
    kernels = re.findall(r"\.name:\s+(\S*k_adv_\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(kernels) >= 1, kernels
    assert {re.search(r"k_adv_[a-z]+", name).group(0) for name, _ in kernels} == {
        "k_adv_keys", "k_adv_reduce", "k_adv_spine", "k_adv_heads", "k_adv_emit"}
    assert all(int(size) == 0 for _, size in kernels), kernels
