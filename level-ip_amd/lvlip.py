"""lvlip — ctypes binding of liblvlip_csum.so (include/lvlip_csum.h).

Host-side mirror of level-ip's checksum interface for tests/ and bench.py.
The names follow the reference:

  checksum(buf, count, start_sum)      src/utils.c:40-55  (include/utils.h:14)
  sum_every_16bits(buf, count)         src/utils.c:22-38  (include/utils.h:13)
  tcp_udp_checksum(saddr, daddr, proto, data, len)   src/tcp.c:87-98
  ip_send_check(iphdr_bytearray)       src/ip_output.c:8-12

plus the batched GPU entry points (batch_dev, Context.batch_host[_flat]).

The library is loaded eagerly and a missing or broken build raises
LvlipUnavailable: there is no Python or CPU fallback for the batched path.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liblvlip_csum.so")
TESTKIT_PATH = os.path.join(HERE, "liblvlip_testkit.so")
LAB_PATH = os.path.join(HERE, "liblvlip_lab.so")

# error codes (include/lvlip_csum.h)
OK, EINVAL, ENODEV, EHIP, ENOMEM, ERANGE = 0, -1, -2, -3, -4, -5
# the product's kernels (include/lvlip_csum.h)
KERNEL_AUTO, KERNEL_FLAT, KERNEL_WINDOW, KERNEL_LANE = 0, 3, 8, 10
# the A/B variants measured against them, in liblvlip_lab.so (lab_kernels.hip);
# batch_dev sends these ids (and FLAT's A/B shapes) there, the product
# returns EINVAL for them.
KERNEL_WAVE, KERNEL_WFLAT, KERNEL_FLAT_OCC = 1, 9, 13
LAB_KERNELS = (KERNEL_WAVE, KERNEL_WFLAT, KERNEL_FLAT_OCC)
# retired ids (EINVAL in both libraries): 6 and 7 (round 1's balanced stream
# kernels), and the lab kernels pruned in round 4 after losing their A/Bs by
# >= 3 % (k_wave_lds 2, k_wave_simple 4, k_flat v1 5, k_rflat 11, k_wsflat 12,
# k_flat2_perm 14, k_window_dyn 15; DESIGN.md §4, last in commit 4e633d9)
RETIRED_KERNELS = (2, 4, 5, 6, 7, 11, 12, 14, 15)
REG_DMA, REG_ZEROCOPY = 0, 1
KERNEL_NAMES = {"auto": KERNEL_AUTO, "wave": KERNEL_WAVE, "flat": KERNEL_FLAT, "window": KERNEL_WINDOW,
                "wflat": KERNEL_WFLAT, "lane": KERNEL_LANE, "flat_occ": KERNEL_FLAT_OCC}
KERNEL_LABELS = {v: k for k, v in KERNEL_NAMES.items()}

# struct lvlip_csum_desc {u64 offset; i32 len; u32 start_sum;}  (16 B)
DESC_DTYPE = np.dtype([("offset", "<u8"), ("len", "<i4"), ("start_sum", "<u4")])
assert DESC_DTYPE.itemsize == 16


class LvlipUnavailable(RuntimeError):
    """liblvlip_csum.so is missing or cannot be loaded."""


class LvlipError(RuntimeError):
    def __init__(self, rc: int, what: str):
        self.rc = rc
        detail = ""
        try:
            detail = _lib.lvlip_last_hip_error().decode()
        except Exception:  # pragma: no cover
            pass
        msg = f"{what}: {_lib.lvlip_strerror(rc).decode()} ({rc})"
        if detail:
            msg += f" [{detail}]"
        super().__init__(msg)


class LaunchCfg(ctypes.Structure):
    _fields_ = [("kernel", ctypes.c_int32), ("unroll", ctypes.c_int32),
                ("waves_per_cu", ctypes.c_int32), ("len_hint", ctypes.c_int32)]


class Iov(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("len", ctypes.c_int32), ("start_sum", ctypes.c_uint32)]


class Frame(ctypes.Structure):  # include/lvlip_skb.h: lvlip_frame
    _fields_ = [("head", ctypes.c_void_p), ("len", ctypes.c_uint32)]


class CtxStats(ctypes.Structure):  # include/lvlip_csum.h: lvlip_ctx_stats
    _fields_ = [("gpu_calls", ctypes.c_uint64), ("cpu_calls", ctypes.c_uint64),
                ("pieces", ctypes.c_uint64), ("h2d_bytes", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# include/lvlip_csum.h: host calls of at most this many packets / frames run on
# the calling thread unless the context says otherwise (LVLIP_CPU_MAX)
CPU_MAX_DEFAULT = 16384


# RX verdicts and flags (include/lvlip_skb.h)
RX_OK, RX_NOT_IP, RX_SHORT, RX_BAD_VERSION, RX_BAD_IHL, RX_TTL0, RX_BAD_CSUM, RX_BAD_L4, \
    RX_UNKNOWN_PROTO = range(1, 10)
RX_VERIFY_L4 = 0x1
ECHO_FULL = 0x1  # lvlip_icmp_echo_reply_dev_ex (include/lvlip_skb.h)
PLAN_MALFORMED = 0xFFFFFFFF


def _share_torch_hip_runtime() -> None:
    """Make this process use ONE HIP runtime.

    PyTorch-ROCm ships its own libamdhip64.so (SONAME libamdhip64.so.7) and its
    libtorch_hip.so asks for it by the name "libamdhip64.so".  If our library were
    loaded first, the dynamic linker would resolve its libamdhip64.so.7 from
    /opt/rocm and torch would later map a second runtime next to it.  Preloading
    torch's copy (RTLD_GLOBAL) makes both resolve to the same file."""
    import importlib.util

    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def _load(path: str) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise LvlipUnavailable(
            f"{path} not built: run `make -C level-ip_amd` (or __graft_entry__.build())")
    try:
        return ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise LvlipUnavailable(f"cannot load {path}: {e}") from e


BUILD_SOURCES = os.path.join(HERE, "BUILD_SOURCES")


def source_build_id(list_file: str = BUILD_SOURCES) -> str:
    """SHA-256 (first 16 hex digits) of the sources a list file names, in its
    order: BUILD_SOURCES (the product, lvlip_build_id()), LAB_SOURCES or
    TESTKIT_SOURCES (the helper libraries' stamps) -- what
    level-ip_amd/Makefile compiles into each library."""
    import hashlib

    root = os.path.dirname(HERE)
    h = hashlib.sha256()
    with open(list_file) as f:
        for rel in f.read().split():
            with open(os.path.join(root, rel), "rb") as g:
                h.update(g.read())
    return h.hexdigest()[:16]


def _stamp(lib: ctypes.CDLL, path: str, symbol: str, list_file: str) -> str:
    """The library's build stamp, checked against the tree's sources; a
    library without the symbol (built before stamps existed) or with another
    stamp is stale and refused."""
    try:
        fn = getattr(lib, symbol)
    except AttributeError:
        raise LvlipUnavailable(f"{path} has no {symbol} (built before build stamps): rebuild with "
                               "`make -C level-ip_amd`") from None
    fn.restype = ctypes.c_char_p
    fn.argtypes = []
    got, want = fn().decode(), source_build_id(list_file)
    if got != want:
        raise LvlipUnavailable(f"{path} was built from other sources (stamp {got}, tree {want}): "
                               "rebuild with `make -C level-ip_amd`")
    return got


_share_torch_hip_runtime()
_lib = _load(LIB_PATH)
BUILD_ID = _stamp(_lib, LIB_PATH, "lvlip_build_id", BUILD_SOURCES)

# every entry point declared in include/lvlip_csum.h, with its ctypes signature
_P, _STR, _INT, _SZ = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_size_t
_U8, _U16, _U32, _U64, _I32 = ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
_PP, _PU32, _PU64 = ctypes.POINTER(_P), ctypes.POINTER(_U32), ctypes.POINTER(_U64)
SIGNATURES = {
    "sum_every_16bits": (_U32, [_P, _INT]),
    "checksum": (_U16, [_P, _INT, _INT]),
    "lvlip_pseudo_sum": (_U32, [_U32, _U32, _U8, _U16]),
    "tcp_udp_checksum": (_INT, [_U32, _U32, _U8, _P, _U16]),
    "tcp_v4_checksum": (_INT, [_P, _U32, _U32]),
    "ip_send_check": (None, [_P]),
    "lvlip_csum_batch_dev": (_INT, [_P, _P, _U32, _P, _P]),
    "lvlip_csum_batch_dev_ex": (_INT, [_P, _P, _U32, _P, _P, ctypes.POINTER(LaunchCfg)]),
    "lvlip_csum_ctx_create": (_INT, [_PP, _INT, _SZ]),
    "lvlip_csum_ctx_destroy": (_INT, [_P]),
    "lvlip_csum_batch_host": (_INT, [_P, ctypes.POINTER(Iov), _U32, _P]),
    "lvlip_csum_batch_host_flat": (_INT, [_P, _P, _SZ, _P, _U32, _P]),
    "lvlip_csum_register": (_INT, [_P, _P, _SZ, _U32]),
    "lvlip_csum_unregister": (_INT, [_P, _P]),
    "lvlip_strerror": (_STR, [_INT]),
    # include/lvlip_skb.h (f1/f2 frame batches)
    "lvlip_rx_verify": (_INT, [_P, ctypes.POINTER(Frame), _U32, _U32, _P]),
    "lvlip_rx_plan": (_U32, [ctypes.POINTER(Frame), _U32, _U32, _P, ctypes.POINTER(Iov), _P]),
    "lvlip_rx_apply": (None, [_U32, _P, _U32, _P, _P]),
    "lvlip_tx_checksum": (_INT, [_P, ctypes.POINTER(Frame), _U32]),
    "lvlip_tx_plan": (_U32, [ctypes.POINTER(Frame), _U32, ctypes.POINTER(Iov), _P]),
    "lvlip_tx_apply": (None, [_U32, _P, _P]),
    "lvlip_icmp_echo_reply_csum": (_U32, [_U16]),
    "lvlip_icmp_echo_reply_fill": (_U32, [ctypes.POINTER(Frame), _U32]),
    "lvlip_frames_workspace_bytes": (_SZ, [_U32]),
    "lvlip_rx_verify_dev": (_INT, [_P, _P, _U32, _U32, _P, _P, _P]),
    "lvlip_tx_checksum_dev": (_INT, [_P, _P, _U32, _P, _P, _P]),
    "lvlip_pseudo_sum_rfc": (_U32, [_U32, _U32, _U8, _U16]),
    "lvlip_icmp_echo_reply_dev": (_INT, [_P, _P, _U32, _P, _P]),
    "lvlip_icmp_echo_reply_dev_ex": (_INT, [_P, _P, _U32, _U32, _P, _P]),
    # Group 4: one batch over several GPUs
    "lvlip_partition_bytes": (_INT, [_P, _U32, _U32, _P]),
    "lvlip_csum_batch_host_flat_multi": (_INT, [_P, _U32, _P, _SZ, _P, _U32, _P]),
    "lvlip_rx_verify_skb_list": (_INT, [_P, _P, _U32, _P, _U32]),
    "lvlip_tx_checksum_skb_list": (_INT, [_P, _P]),
    # round 6: size-based dispatch, counters, context-free CPU frame calls
    "lvlip_csum_ctx_set_cpu_max": (_INT, [_P, _U32]),
    "lvlip_csum_ctx_cpu_max": (_U32, [_P]),
    "lvlip_csum_ctx_stats": (_INT, [_P, ctypes.POINTER(CtxStats)]),
    "lvlip_rx_verify_cpu": (_INT, [ctypes.POINTER(Frame), _U32, _U32, _P]),
    "lvlip_tx_checksum_cpu": (_INT, [ctypes.POINTER(Frame), _U32]),
    "lvlip_rx_verify_skb_list_cpu": (_INT, [_P, _U32, _P, _U32]),
    "lvlip_tx_checksum_skb_list_cpu": (_INT, [_P]),
    # f2 on the device: segmentation (seg_cpu.c, seg_kernels.hip)
    "lvlip_tso_plan": (_U32, [_P, _U32, _PU64]),
    "lvlip_tso_cpu": (_INT, [_P, _P, _U32, _P, _P]),
    "lvlip_tso_dev": (_INT, [_P, _P, _U32, _U32, _P, _P, _P]),
    # f1 on the device: receive coalescing (rcv_cpu.c, rcv_kernels.hip)
    "lvlip_lro_plan": (_U32, [_P, _U32, _PU64]),
    "lvlip_lro_cpu": (_INT, [_P, _P, _U32, _P, _U32, _U32, _P, _P]),
    "lvlip_lro_dev": (_INT, [_P, _P, _U32, _P, _U32, _U32, _P, _P, _P]),
    "lvlip_lro_advance": (_INT, [_P, _U32, _P, _U32, _P]),
    "lvlip_lro_advance_workspace_bytes": (_SZ, [_U32, _U32]),
    "lvlip_lro_advance_dev": (_INT, [_P, _U32, _P, _U32, _P, _P, _SZ, _P]),
    # f1 on the device: state across batches (rcv_cpu.c, adv_kernels.hip, next_kernels.hip)
    "lvlip_lro_advance_carry": (_INT, [_P, _U32, _P, _U32, _P, _P]),
    "lvlip_lro_advance_carry_workspace_bytes": (_SZ, [_U32, _U32]),
    "lvlip_lro_advance_carry_dev": (_INT, [_P, _U32, _P, _U32, _P, _P, _P, _SZ, _P]),
    "lvlip_lro_next_cpu": (_INT, [_P, _P, _U32]),
    "lvlip_lro_next_dev": (_INT, [_P, _P, _U32, _P]),
    # f1 on the device: the acknowledgement (ack_cpu.c, ack_kernels.hip)
    "lvlip_ack_plan": (_U32, [_P, _P, _U32, _PU64]),
    "lvlip_ack_cpu": (_INT, [_P, _P, _P, _U32, _U32, _P, _P]),
    "lvlip_ack_dev": (_INT, [_P, _P, _P, _U32, _U32, _P, _P, _P]),
    # f2 on the device: the ACK side and the retransmit (snd_cpu.c, snd_kernels.hip)
    "lvlip_snd_plan": (_U32, [_P, _U32, _PU32]),
    "lvlip_snd_cpu": (_INT, [_P, _P, _U32, _P, _U32, _P, _P, _P]),
    "lvlip_snd_dev": (_INT, [_P, _P, _U32, _P, _U32, _P, _P, _P, _P]),
    "lvlip_rtx_cpu": (_INT, [_P, _P, _P, _P, _U32, _U32, _P, _P, _P]),
    "lvlip_rtx_dev": (_INT, [_P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P]),
    "lvlip_snd_next_cpu": (_INT, [_P, _P, _U32]),
    "lvlip_snd_next_dev": (_INT, [_P, _P, _U32, _P]),
    # f2 on the device: the scoreboard and the selective retransmit (sack_cpu.c, sack_kernels.hip, snd_*)
    "lvlip_sack_workspace_bytes": (_SZ, [_U32, _U32]),
    "lvlip_sack_cpu": (_INT, [_P, _P, _U32, _P, _P, _P, _U32, _P, _P, _P, _P]),
    "lvlip_sack_dev": (_INT, [_P, _P, _U32, _P, _P, _P, _U32, _P, _P, _P, _P, _P, _SZ, _P]),
    "lvlip_rtx_sack_cpu": (_INT, [_P, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P]),
    "lvlip_rtx_sack_dev": (_INT, [_P, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P]),
    # f2 on the device: the write queue (push_cpu.c, push_kernels.hip)
    "lvlip_push_plan": (_U32, [_P, _P, _U32, _PU64, _PU32]),
    "lvlip_push_cpu": (_INT, [_P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P]),
    "lvlip_push_dev": (_INT, [_P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P, _P]),
    # f2 on the device: the timer and the peer's window (rto_cpu.c, rto_kernels.hip)
    "lvlip_rto_check": (_INT, [_P, _U32]),
    "lvlip_wnd_cpu": (_INT, [_P, _P, _P, _P, _U32, _P, _P, _P, _U32, _U32, _P]),
    "lvlip_wnd_dev": (_INT, [_P, _P, _P, _P, _U32, _P, _P, _P, _U32, _U32, _P, _P]),
    "lvlip_rto_cpu": (_INT, [_P, _P, _P, _P, _U32, _U32, _U32, _P, _P, _P]),
    "lvlip_rto_dev": (_INT, [_P, _P, _P, _P, _U32, _U32, _U32, _P, _P, _P, _P]),
    # f2 on the device: the congestion window (cc_cpu.c, cc_kernels.hip)
    "lvlip_cc_check": (_INT, [_P, _U32]),
    "lvlip_cc_cpu": (_INT, [_P, _P, _P, _P, _P, _U32, _P, _P, _P]),
    "lvlip_cc_dev": (_INT, [_P, _P, _P, _P, _P, _U32, _P, _P, _P, _P]),
    # f2 on the device: the persist timer (persist_cpu.c, persist_kernels.hip)
    "lvlip_persist_check": (_INT, [_P, _U32]),
    "lvlip_persist_cpu": (_INT, [_P, _P, _P, _P, _P, _P, _U32, _U32, _P, _P, _P]),
    "lvlip_persist_dev": (_INT, [_P, _P, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P]),
    # f1: the receive buffer (rbuf_cpu.c)
    "lvlip_rbuf_plan": (_U32, [_P, _P, _U32, ctypes.POINTER(ctypes.c_uint64)]),
    "lvlip_rbuf_check": (_INT, [_P, _P, _U32]),
    "lvlip_rbuf_cpu": (_INT, [_P, _P, _P, _P, _U32, _P, _P, _P, _P, _P]),
    # the end of a connection (fin_cpu.c, fin_kernels.hip)
    "lvlip_fin_check": (_INT, [_P, _P, _U32]),
    "lvlip_fin_cpu": (_INT, [_P, _P, _P, _U32, _P, _P, _P, _P, _U32, _P, _U32, _P, _P, _P, _P]),
    "lvlip_fin_workspace_bytes": (_SZ, [_U32]),
    "lvlip_fin_dev": (_INT, [_P, _P, _P, _U32, _P, _P, _P, _P, _U32, _P, _U32, _P, _P, _P, _P, _P, _P]),
    "lvlip_auto_kernel": (_INT, [_I32, _U32, ctypes.POINTER(LaunchCfg)]),
    "lvlip_batch_launches": (_U32, [_U32, ctypes.POINTER(LaunchCfg)]),
    "lvlip_build_id": (_STR, []),
    "lvlip_abi_version": (_INT, []),
    "lvlip_device_count": (_INT, []),
    "lvlip_last_hip_error": (_STR, []),
}
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(_lib, _name)
    _fn.restype = _res
    _fn.argtypes = _args


def lib() -> ctypes.CDLL:
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != OK:
        raise LvlipError(rc, what)


def _as_u8(buf) -> np.ndarray:
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    return np.frombuffer(bytes(buf), dtype=np.uint8)


# What the f1/f2 wrappers (tso_* .. rtx_sack_*) share.  numpy side first.

_STAND_IN = np.zeros(16, dtype=np.uint8)  # for an empty buffer where a call wants a non-NULL pointer


def _aptr(a, stand_in: bool = False):
    """The address of an array's data; NULL (or the stand-in's) for None and
    for an empty array."""
    if a is not None and a.size:
        return a.ctypes.data
    return _STAND_IN.ctypes.data if stand_in else None


def _is_u8(a, writeable: bool = False) -> bool:
    """A contiguous (and writeable) uint8 array."""
    return isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags.c_contiguous and \
        (a.flags.writeable or not writeable)


def _u8_inplace(buf) -> np.ndarray:
    """_as_u8 that never copies a contiguous uint8 array."""
    return buf if _is_u8(buf) else _as_u8(buf)


def _planned(a: np.ndarray, dtype, what: str, writeable: bool = True) -> None:
    """The array a *_plan call reads (and writes) in place."""
    if a.dtype != dtype or not a.flags.c_contiguous or not (a.flags.writeable or not writeable):
        raise TypeError(what)


def _plan_ok(n: int, refused: str) -> int:
    if n == PLAN_MALFORMED:
        raise ValueError(refused)
    return n


def _out_u8(out, need: int) -> np.ndarray:
    """The caller's frame or stream buffer, checked, or a new zeroed one."""
    if out is None:
        out = np.zeros(need, dtype=np.uint8)
    if out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < need:
        raise ValueError("out: a contiguous uint8 array of at least the plan's out_bytes")
    return out


# The torch side: sizes in bytes, whatever the tensor's dtype.

def _nbytes(t) -> int:
    return t.numel() * t.element_size()


def _records(t, itemsize: int) -> int:
    """Whole records of itemsize bytes in a tensor; 0 for None."""
    return t.numel() * t.element_size() // itemsize if t is not None else 0


def _need(t, name: str, per: int, n: int, unit: str, optional: bool = False) -> None:
    if not (optional and t is None) and t.numel() * t.element_size() < per * n:
        raise ValueError(f"{name}: {per} bytes per {unit}")


def _tptr(t, n: int = 1):
    """A tensor's address; NULL for None and for a batch of n == 0."""
    return t.data_ptr() if n and t is not None else None


def _result(t, name: str, per: int, n: int, unit: str, device, zeroed: bool = False):
    """The caller's result tensor, checked, or a new one of per bytes for
    each of max(n, 1); the wrapper returns its first per * n bytes."""
    if t is None:
        import torch

        return (torch.zeros if zeroed else torch.empty)(per * max(n, 1), dtype=torch.uint8, device=device)
    _need(t, name, per, n, unit)
    return t


def _stream(stream, device):
    if stream:
        return stream
    import torch

    return torch.cuda.current_stream(device)


# --------------------------------------------------------------- per call --

def sum_every_16bits(buf, count: Optional[int] = None) -> int:
    a = _as_u8(buf)
    if count is None:
        count = a.size
    if count > a.size:
        raise ValueError("count exceeds buffer")
    return int(_lib.sum_every_16bits(a.ctypes.data if a.size else None, int(count)))


def checksum(buf, count: Optional[int] = None, start_sum: int = 0) -> int:
    """src/utils.c:40-55; start_sum is the reference's `int` (any u32 bit pattern)."""
    a = _as_u8(buf)
    if count is None:
        count = a.size
    if count > a.size:
        raise ValueError("count exceeds buffer")
    s = ctypes.c_int(ctypes.c_uint32(start_sum & 0xFFFFFFFF).value).value
    return int(_lib.checksum(a.ctypes.data if a.size else None, int(count), s))


def pseudo_sum(saddr: int, daddr: int, proto: int, length: int) -> int:
    """Seed of tcp_udp_checksum (src/tcp.c:87-96), u32 wrap-around."""
    return int(_lib.lvlip_pseudo_sum(saddr & 0xFFFFFFFF, daddr & 0xFFFFFFFF, proto & 0xFF,
                                     length & 0xFFFF))


def tcp_udp_checksum(saddr: int, daddr: int, proto: int, data, length: int) -> int:
    """src/tcp.c:87-98 (len is a uint16_t there, so it is truncated the same way)."""
    length &= 0xFFFF
    a = _as_u8(data)
    if length > a.size:
        raise ValueError("length exceeds buffer")
    return int(_lib.tcp_udp_checksum(saddr & 0xFFFFFFFF, daddr & 0xFFFFFFFF, proto & 0xFF,
                                     a.ctypes.data if a.size else None, length))


def ip_send_check(hdr: bytearray) -> None:
    """src/ip_output.c:8-12: checksum over ihl*4 bytes, stored raw at offset 10."""
    if len(hdr) < max(20, (hdr[0] & 0x0F) * 4):
        raise ValueError("header shorter than ihl*4")
    c = (ctypes.c_char * len(hdr)).from_buffer(hdr)
    _lib.ip_send_check(ctypes.addressof(c))
    del c


# ---------------------------------------------------------- device batches --

def is_lab_kernel(kernel: int, unroll: int = 0) -> bool:
    """The A/B variants that live in liblvlip_lab.so: the lab kernel ids, and
    FLAT's shapes other than the product's (2, 4 or 8 loads per round, block
    order)."""
    if kernel in LAB_KERNELS:
        return True
    return kernel == KERNEL_FLAT and unroll not in (0, 2, 4, 8)


def batch_dev(base_ptr: int, desc_ptr: int, n: int, out_ptr: int, stream: int = 0,
              kernel: int = KERNEL_AUTO, unroll: int = 0, waves_per_cu: int = 0,
              len_hint: int = 0) -> None:
    """lvlip_csum_batch_dev_ex on raw device pointers (async on `stream`); an
    A/B variant id goes to lvlip_lab_batch_dev_ex (liblvlip_lab.so) instead."""
    cfg = LaunchCfg(kernel, unroll, waves_per_cu, min(max(int(len_hint), 0), 0x7FFFFFFF))
    if is_lab_kernel(kernel, unroll):
        _check(lab().lvlip_lab_batch_dev_ex(base_ptr, desc_ptr, n, out_ptr, stream or None,
                                            ctypes.byref(cfg)), "lvlip_lab_batch_dev_ex")
        return
    _check(_lib.lvlip_csum_batch_dev_ex(base_ptr, desc_ptr, n, out_ptr, stream or None,
                                        ctypes.byref(cfg)), "lvlip_csum_batch_dev_ex")


def auto_kernel(len_hint: int, n: int) -> LaunchCfg:
    """The kernel and shape LVLIP_KERNEL_AUTO runs (lvlip_auto_kernel)."""
    cfg = LaunchCfg()
    _lib.lvlip_auto_kernel(min(max(int(len_hint), 0), 0x7FFFFFFF), n, ctypes.byref(cfg))
    return cfg


def batch_launches(n: int, kernel: int = KERNEL_AUTO, unroll: int = 0, waves_per_cu: int = 0,
                   len_hint: int = 0) -> int:
    """Kernel launches one batch_dev call of n descriptors issues with this
    launch config (lvlip_batch_launches; AUTO resolved as the call does)."""
    if is_lab_kernel(kernel, unroll):  # the lab launches 2^30 descriptors at most
        return (n + (1 << 30) - 1) >> 30
    cfg = LaunchCfg(kernel, unroll, waves_per_cu, min(max(int(len_hint), 0), 0x7FFFFFFF))
    return int(_lib.lvlip_batch_launches(n, ctypes.byref(cfg)))


def auto_kernel_name(len_hint: int, n: int) -> str:
    return KERNEL_LABELS[auto_kernel(len_hint, n).kernel]


def batch_torch(base, descs, out=None, kernel: int = KERNEL_AUTO, unroll: int = 0,
                waves_per_cu: int = 0, stream=None, len_hint: int = 0):
    """Checksums a device batch held in torch tensors on the current stream.

    base:  uint8 CUDA tensor (16-B aligned, padded to a 16-B multiple past the last packet)
    descs: CUDA tensor of n*16 bytes (uint8 or int64 view of lvlip_csum_desc[n])
    out:   int16/uint16 CUDA tensor of n elements (allocated when None)
    """
    import torch

    if not (base.is_cuda and descs.is_cuda):
        raise ValueError("batch_torch needs CUDA tensors")
    if descs.device != base.device:
        raise ValueError("base and descs must be on the same device")
    if not (base.is_contiguous() and descs.is_contiguous()):
        raise ValueError("base and descs must be contiguous")
    nbytes = descs.numel() * descs.element_size()
    if nbytes % 16:
        raise ValueError(f"descs holds {nbytes} B, not a multiple of the 16-B descriptor")
    n = nbytes // 16
    if out is None:
        out = torch.empty(n, dtype=torch.int16, device=base.device)
    elif (not out.is_cuda or out.device != base.device or out.element_size() != 2
          or not out.is_contiguous() or out.numel() < n):
        raise ValueError(f"out must be a contiguous 2-byte CUDA tensor of >= {n} elements "
                         "on base's device")
    if stream is None:
        stream = torch.cuda.current_stream(base.device)
    batch_dev(base.data_ptr(), descs.data_ptr(), n, out.data_ptr(), stream.cuda_stream,
              kernel, unroll, waves_per_cu, len_hint)
    return out


def device_count() -> int:
    return int(_lib.lvlip_device_count())


# ------------------------------------------------------------ frame batches --

def frames_array(frames: Sequence[bytearray]):
    """lvlip_frame[n] over writable buffers (bytearray / uint8 ndarray), in place.

    Returns (array, keep); keep holds the buffer views alive while C uses them."""
    n = len(frames)
    arr = (Frame * max(n, 1))()
    keep = []
    for i, f in enumerate(frames):
        if isinstance(f, np.ndarray):
            a = f.view(np.uint8).reshape(-1)
            if not a.flags.c_contiguous:
                raise ValueError("frames must be contiguous")
            ptr, ln = a.ctypes.data, a.size
            keep.append(a)
        else:
            ln = len(f)
            c = (ctypes.c_char * max(ln, 1)).from_buffer(f) if ln else None
            ptr = ctypes.addressof(c) if c is not None else None
            keep.append(c)
        arr[i].head = ptr
        arr[i].len = ln
    return arr, keep


def pseudo_sum_rfc(saddr: int, daddr: int, proto: int, length: int) -> int:
    return int(_lib.lvlip_pseudo_sum_rfc(saddr & 0xFFFFFFFF, daddr & 0xFFFFFFFF, proto & 0xFF,
                                         length & 0xFFFF))


def rx_plan(frames, flags: int = 0):
    """lvlip_rx_plan: (verdict[n] uint8, [(ptr, len, start_sum)] * m, tag[m] uint32)."""
    n = len(frames)
    arr, keep = frames_array(frames)
    verdict = np.zeros(max(n, 1), dtype=np.uint8)
    iov = (Iov * max(2 * n, 1))()
    tag = np.zeros(max(2 * n, 1), dtype=np.uint32)
    m = _lib.lvlip_rx_plan(arr, n, flags, verdict.ctypes.data, iov, tag.ctypes.data)
    del keep
    return verdict[:n], [(iov[k].ptr, iov[k].len, iov[k].start_sum) for k in range(m)], tag[:m]


def rx_apply(verdict: np.ndarray, tag: np.ndarray, csum: np.ndarray) -> np.ndarray:
    v = np.ascontiguousarray(verdict, dtype=np.uint8).copy()
    t = np.ascontiguousarray(tag, dtype=np.uint32)
    c = np.ascontiguousarray(csum, dtype=np.uint16)
    _lib.lvlip_rx_apply(v.size, v.ctypes.data, t.size, t.ctypes.data, c.ctypes.data)
    return v


def tx_plan(frames):
    """lvlip_tx_plan: ([(ptr, len, start_sum)] * m, field pointers[m]) or None if malformed."""
    n = len(frames)
    arr, keep = frames_array(frames)
    iov = (Iov * max(2 * n, 1))()
    field = np.zeros(max(2 * n, 1), dtype=np.uint64)
    m = _lib.lvlip_tx_plan(arr, n, iov, field.ctypes.data)
    del keep
    if m == PLAN_MALFORMED:
        return None
    return [(iov[k].ptr, iov[k].len, iov[k].start_sum) for k in range(m)], field[:m].copy()


CSUM_RECOMPUTE = 0xFFFFFFFF

# struct lvlip_frame_desc {u64 offset; u32 len; u32 reserved;}  (include/lvlip_skb.h)
FRAME_DESC_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u4"), ("reserved", "<u4")])


def pack_frames(frames, align_mod: int = 16, seed: int = 0):
    """Lay frames end to end in one uint8 array (each starting at a random
    offset mod `align_mod`), for the device-resident frame API.  Returns
    (buffer, FRAME_DESC_DTYPE descriptors)."""
    rng = np.random.default_rng(seed)
    offs, pos = [], 0
    for f in frames:
        pos += int(rng.integers(0, align_mod)) if align_mod > 1 else 0
        offs.append(pos)
        pos += len(f)
    buf = np.zeros((pos + 64 + 15) & ~15, dtype=np.uint8)
    d = np.zeros(len(frames), dtype=FRAME_DESC_DTYPE)
    for i, (o, f) in enumerate(zip(offs, frames)):
        buf[o:o + len(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
        d[i]["offset"], d[i]["len"] = o, len(f)
    return buf, d


def _frames_dev(base, fdescs):
    import torch

    n = fdescs.numel() * fdescs.element_size() // 16 if hasattr(fdescs, "numel") else len(fdescs)
    if not hasattr(fdescs, "numel"):
        fdescs = torch.from_numpy(np.ascontiguousarray(fdescs, dtype=FRAME_DESC_DTYPE)
                                  .view(np.uint8).copy()).to(base.device)
    return n, fdescs


def rx_verify_dev(base, fdescs, flags: int = 0, stream=None):
    """lvlip_rx_verify_dev on frames in a CUDA uint8 tensor; returns the verdicts
    (uint8 CUDA tensor), asynchronously on `stream` (default: current)."""
    import torch

    n, fd = _frames_dev(base, fdescs)
    verdict = torch.empty(max(n, 1), dtype=torch.uint8, device=base.device)
    s = _stream(stream, base.device)
    _check(_lib.lvlip_rx_verify_dev(base.data_ptr(), fd.data_ptr(), n, flags, verdict.data_ptr(),
                                    None, s.cuda_stream), "lvlip_rx_verify_dev")
    return verdict[:n]


def tx_checksum_dev(base, fdescs, stream=None):
    """lvlip_tx_checksum_dev in place on frames in a CUDA uint8 tensor; returns
    the per-frame status (1 filled, 0 malformed and untouched)."""
    import torch

    n, fd = _frames_dev(base, fdescs)
    status = torch.empty(max(n, 1), dtype=torch.uint8, device=base.device)
    s = _stream(stream, base.device)
    _check(_lib.lvlip_tx_checksum_dev(base.data_ptr(), fd.data_ptr(), n, status.data_ptr(),
                                      None, s.cuda_stream), "lvlip_tx_checksum_dev")
    return status[:n]


def icmp_echo_reply_dev(base, fdescs, stream=None, flags: int = 0):
    """lvlip_icmp_echo_reply_dev[_ex] (f4) in place on frames in a CUDA uint8
    tensor; returns the per-frame status (1 updated, 2 recomputed, 0
    untouched).  flags 0: the RFC 1624 update, exact for requests whose ICMP
    checksum verified (the caller's precondition); ECHO_FULL: icmpv4_reply's
    full recomputation for any request."""
    import torch

    n, fd = _frames_dev(base, fdescs)
    status = torch.empty(max(n, 1), dtype=torch.uint8, device=base.device)
    s = _stream(stream, base.device)
    if flags == 0:
        rc = _lib.lvlip_icmp_echo_reply_dev(base.data_ptr(), fd.data_ptr(), n, status.data_ptr(), s.cuda_stream)
    else:
        rc = _lib.lvlip_icmp_echo_reply_dev_ex(base.data_ptr(), fd.data_ptr(), n, flags, status.data_ptr(),
                                               s.cuda_stream)
    _check(rc, "lvlip_icmp_echo_reply_dev")
    return status[:n]


# ------------------------------------------- f2 on the device: segmentation --

# struct lvlip_tso_send (include/lvlip_skb.h), 96 B
TsoSend = np.dtype([("payload_off", "<u8"), ("out_off", "<u8"), ("len", "<u4"), ("seg0", "<u4"),
                    ("stride", "<u4"), ("mss", "<u2"), ("reserved", "<u2"), ("hdr", "u1", (54,)),
                    ("pad", "u1", (10,))])
assert TsoSend.itemsize == 96
TSO_HDR = 54


def tso_send(hdr, payload_off: int, length: int, mss: int, out_off: int = 0, stride: int = 0) -> np.ndarray:
    """One TsoSend record; stride 0 means frames that abut (54 + mss)."""
    r = np.zeros(1, dtype=TsoSend)
    r["payload_off"], r["out_off"], r["len"], r["mss"] = payload_off, out_off, length, mss
    r["stride"] = stride or TSO_HDR + mss
    r["hdr"][0] = np.frombuffer(bytes(hdr), dtype=np.uint8)
    return r


def tso_plan(sends: np.ndarray):
    """lvlip_tso_plan: validates the sends and fills their seg0 in place.
    Returns (nseg, out_bytes); ValueError for a malformed send or too many
    segments."""
    _planned(sends, TsoSend, "sends: a writeable contiguous TsoSend array")
    out_bytes = ctypes.c_uint64(0)
    nseg = _plan_ok(int(_lib.lvlip_tso_plan(_aptr(sends), sends.size, ctypes.byref(out_bytes))),
                    "malformed send (or more than LVLIP_MAX_BATCH segments)")
    return nseg, int(out_bytes.value)


def tso_cpu(payload, sends: np.ndarray, out: Optional[np.ndarray] = None):
    """lvlip_tso_cpu: plans the sends and builds their frames on the calling
    thread.  Returns (out, fd): the frame buffer (a new zeroed one of the plan's
    out_bytes unless `out` is given, which then keeps its bytes outside the
    frames) and the FRAME_DESC_DTYPE descriptors."""
    nseg, out_bytes = tso_plan(sends)
    pay = _as_u8(payload)
    if any(int(s["payload_off"]) + int(s["len"]) > pay.size for s in sends):
        raise ValueError("a send reads past the payload")
    out = _out_u8(out, out_bytes)
    fd = np.zeros(nseg, dtype=FRAME_DESC_DTYPE)
    _check(_lib.lvlip_tso_cpu(pay.ctypes.data, sends.ctypes.data, sends.size, out.ctypes.data,
                              fd.ctypes.data), "lvlip_tso_cpu")
    return out, fd


def tso_dev(payload_t, sends_t, nseg: int, out_t, fd_t=None, stream=None):
    """lvlip_tso_dev on CUDA uint8 tensors: payload_t the payload, sends_t the
    planned TsoSend records' bytes (96 each), out_t the frame buffer (at least
    the plan's out_bytes), fd_t (optional) 16 bytes per segment for the frame
    descriptors.  One launch on `stream` (default: current), asynchronous."""
    n = _records(sends_t, TsoSend.itemsize)
    s = _stream(stream, out_t.device)
    _need(fd_t, "fd_t", 16, nseg, "segment", optional=True)
    _check(_lib.lvlip_tso_dev(payload_t.data_ptr(), sends_t.data_ptr(), n, nseg, out_t.data_ptr(), _tptr(fd_t),
                              s.cuda_stream), "lvlip_tso_dev")


# ------------------------------------- f1 on the device: receive coalescing --

# struct lvlip_lro_flow / lvlip_lro_rec / lvlip_lro_result (include/lvlip_skb.h)
LRO_FLOW_DTYPE = np.dtype([("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
                           ("rcv_nxt", "<u4"), ("rcv_wnd", "<u4"), ("reserved", "<u4"), ("out_off", "<u8"),
                           ("user", "<u8"), ("pad", "u1", (8,))])
LRO_REC_DTYPE = np.dtype([("flow", "<u4"), ("rel", "<u4"), ("dlen", "<u2"), ("status", "u1"),
                          ("tcp_flags", "u1"), ("ack_seq", "<u4")])
LRO_RESULT_DTYPE = np.dtype([("delivered", "<u4"), ("placed", "<u4"), ("nsack", "<u4"), ("reserved", "<u4"),
                             ("sack", "<u4", (4, 2))])
assert LRO_FLOW_DTYPE.itemsize == 48 and LRO_REC_DTYPE.itemsize == 16 and LRO_RESULT_DTYPE.itemsize == 48
LRO_PLACED, LRO_NOT_TCP, LRO_BAD_TCP_HDR, LRO_NO_FLOW = 1, 16, 17, 18
LRO_CONTROL, LRO_NO_DATA, LRO_OUT_OF_WINDOW = 19, 20, 21
LRO_MAX_FLOWS = 65536


def lro_flow(saddr: bytes, daddr: bytes, sport: int, dport: int, rcv_nxt: int, rcv_wnd: int, out_off: int = 0,
             user: int = 0) -> np.ndarray:
    """One LRO_FLOW_DTYPE record: addresses as the 4 bytes of the IPv4 header,
    ports as host integers (stored in network order)."""
    r = np.zeros(1, dtype=LRO_FLOW_DTYPE)
    r["saddr"] = int.from_bytes(bytes(saddr), "little")
    r["daddr"] = int.from_bytes(bytes(daddr), "little")
    r["sport"] = ((sport & 0xFF) << 8) | (sport >> 8)
    r["dport"] = ((dport & 0xFF) << 8) | (dport >> 8)
    r["rcv_nxt"], r["rcv_wnd"], r["out_off"], r["user"] = rcv_nxt, rcv_wnd, out_off, user
    return r


def lro_plan(flows: np.ndarray):
    """lvlip_lro_plan: validates the flows and sorts them in place by key.
    Returns out_bytes; ValueError for a refused plan."""
    _planned(flows, LRO_FLOW_DTYPE, "flows: a writeable contiguous LRO_FLOW_DTYPE array")
    out_bytes = ctypes.c_uint64(0)
    _plan_ok(int(_lib.lvlip_lro_plan(_aptr(flows), flows.size, ctypes.byref(out_bytes))),
             "refused flows (duplicate key, window, reserved bytes, overlapping ranges, too many)")
    return int(out_bytes.value)


def lro_cpu(base, fdescs: np.ndarray, flows: np.ndarray, flags: int = 0, out: Optional[np.ndarray] = None):
    """lvlip_lro_cpu over frames in `base` (uint8) described by FRAME_DESC_DTYPE
    records, flows as lro_plan left them.  Returns (out, rec): the stream
    buffer (a new zeroed one of the flows' extent unless `out` is given) and
    the LRO_REC_DTYPE records."""
    buf = _as_u8(base)
    fd = np.ascontiguousarray(fdescs, dtype=FRAME_DESC_DTYPE)
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    if any(int(d["offset"]) + int(d["len"]) > buf.size for d in fd):
        raise ValueError("a frame lies past the buffer")
    need = max((int(f["out_off"]) + int(f["rcv_wnd"]) for f in flows), default=0)
    out = _out_u8(out, need)
    rec = np.zeros(fd.size, dtype=LRO_REC_DTYPE)
    _check(_lib.lvlip_lro_cpu(buf.ctypes.data, fd.ctypes.data, fd.size, _aptr(flows), flows.size, flags,
                              out.ctypes.data, rec.ctypes.data), "lvlip_lro_cpu")
    return out, rec


def lro_dev(base_t, fd_t, flows_t, flags: int, out_t, rec_t=None, stream=None):
    """lvlip_lro_dev on CUDA uint8 tensors: base_t the frames, fd_t 16 bytes per
    frame (FRAME_DESC_DTYPE), flows_t the planned flows' bytes (48 each, may
    be empty), out_t the stream buffer.  Returns rec_t (16 bytes per frame, a
    new tensor unless given).  One launch on `stream` (default: current),
    asynchronous."""
    n = _records(fd_t, 16)
    nflows = _records(flows_t, LRO_FLOW_DTYPE.itemsize)
    rec_t = _result(rec_t, "rec_t", 16, n, "frame", out_t.device)
    s = _stream(stream, out_t.device)
    _check(_lib.lvlip_lro_dev(base_t.data_ptr(), fd_t.data_ptr(), n, _tptr(flows_t, nflows), nflows, flags,
                              out_t.data_ptr(), rec_t.data_ptr(), s.cuda_stream), "lvlip_lro_dev")
    return rec_t


def lro_advance(flows: np.ndarray, rec: np.ndarray) -> np.ndarray:
    """lvlip_lro_advance: LRO_RESULT_DTYPE per planned flow (delivered, placed,
    nsack, sack[4] = (left, right))."""
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    rec = np.ascontiguousarray(rec, dtype=LRO_REC_DTYPE)
    res = np.zeros(flows.size, dtype=LRO_RESULT_DTYPE)
    _check(_lib.lvlip_lro_advance(_aptr(flows), flows.size, _aptr(rec), rec.size, _aptr(res)), "lvlip_lro_advance")
    return res


def lro_advance_workspace_bytes(n: int, nflows: int) -> int:
    """lvlip_lro_advance_workspace_bytes: the device workspace lro_advance_dev
    needs for n records (0 for n == 0, and without a device)."""
    return int(_lib.lvlip_lro_advance_workspace_bytes(n, nflows))


def lro_advance_dev(flows_t, rec_t, res_t=None, workspace_t=None, stream=None):
    """lvlip_lro_advance_dev on CUDA uint8 tensors: flows_t the planned flows'
    bytes (48 each), rec_t 16 bytes per record (what lro_dev returned).
    Returns res_t, 48 bytes per flow (a new tensor unless given):
    res_t.cpu().numpy().view(LRO_RESULT_DTYPE) is lro_advance's array.
    workspace_t (a new tensor unless given) holds at least
    lro_advance_workspace_bytes(n, nflows) bytes at a 256-B aligned address.
    Asynchronous on `stream` (default: current)."""
    import torch

    n = _records(rec_t, 16)
    nflows = _records(flows_t, LRO_FLOW_DTYPE.itemsize)
    device = flows_t.device if flows_t is not None else rec_t.device
    res_t = _result(res_t, "res_t", LRO_RESULT_DTYPE.itemsize, nflows, "flow", device)
    need = lro_advance_workspace_bytes(n, nflows) if n and nflows else 0
    if workspace_t is None and need:
        workspace_t = torch.empty(need, dtype=torch.uint8, device=device)
    s = _stream(stream, device)
    _check(_lib.lvlip_lro_advance_dev(_tptr(flows_t, nflows), nflows, _tptr(rec_t, n), n, res_t.data_ptr(),
                                      _tptr(workspace_t), _records(workspace_t, 1), s.cuda_stream),
           "lvlip_lro_advance_dev")
    return res_t[:LRO_RESULT_DTYPE.itemsize * nflows]


# ------------------------------------- f1 on the device: state across batches --

def lro_advance_carry(flows: np.ndarray, rec: np.ndarray, prev: Optional[np.ndarray] = None,
                      res: Optional[np.ndarray] = None) -> np.ndarray:
    """lvlip_lro_advance_carry: lro_advance over the records and the islands
    `prev` (LRO_RESULT_DTYPE per flow, or None) carries from an earlier batch.
    Returns the LRO_RESULT_DTYPE array: `res` when given (it may be `prev`: in
    place), else a new one."""
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    rec = np.ascontiguousarray(rec, dtype=LRO_REC_DTYPE)
    if prev is not None:
        _planned(prev, LRO_RESULT_DTYPE, "prev: a contiguous LRO_RESULT_DTYPE array", writeable=False)
    if res is None:
        res = np.zeros(flows.size, dtype=LRO_RESULT_DTYPE)
    _planned(res, LRO_RESULT_DTYPE, "res: a writeable contiguous LRO_RESULT_DTYPE array")
    if any(r is not None and r.size != flows.size for r in (prev, res)):
        raise ValueError("one result per flow")
    _check(_lib.lvlip_lro_advance_carry(_aptr(flows), flows.size, _aptr(rec), rec.size, _aptr(prev), _aptr(res)),
           "lvlip_lro_advance_carry")
    return res


def lro_advance_carry_workspace_bytes(n: int, nflows: int) -> int:
    """lvlip_lro_advance_carry_workspace_bytes: the device workspace
    lro_advance_carry_dev needs for n records and nflows flows (not 0 for
    n == 0; 0 without a flow, and without a device)."""
    return int(_lib.lvlip_lro_advance_carry_workspace_bytes(n, nflows))


def lro_advance_carry_dev(flows_t, rec_t, prev_t=None, res_t=None, workspace_t=None, stream=None):
    """lvlip_lro_advance_carry_dev on CUDA uint8 tensors: lro_advance_dev's
    arguments and prev_t, 48 bytes per flow (the results of an earlier batch;
    None for no carry; it may be res_t).  Returns res_t, 48 bytes per flow (a
    new tensor unless given).  workspace_t (a new tensor unless given) holds at
    least lro_advance_carry_workspace_bytes(n, nflows) bytes at a 256-B aligned
    address.  Asynchronous on `stream` (default: current)."""
    import torch

    n = _records(rec_t, 16)
    nflows = _records(flows_t, LRO_FLOW_DTYPE.itemsize)
    device = flows_t.device if flows_t is not None else rec_t.device
    _need(prev_t, "prev_t", LRO_RESULT_DTYPE.itemsize, nflows, "flow", optional=True)
    res_t = _result(res_t, "res_t", LRO_RESULT_DTYPE.itemsize, nflows, "flow", device)
    need = lro_advance_carry_workspace_bytes(n, nflows) if nflows and (n or prev_t is not None) else 0
    if workspace_t is None and need:
        workspace_t = torch.empty(need, dtype=torch.uint8, device=device)
    s = _stream(stream, device)
    _check(_lib.lvlip_lro_advance_carry_dev(_tptr(flows_t, nflows), nflows, _tptr(rec_t, n), n, _tptr(prev_t, nflows),
                                            res_t.data_ptr(), _tptr(workspace_t), _records(workspace_t, 1),
                                            s.cuda_stream), "lvlip_lro_advance_carry_dev")
    return res_t[:LRO_RESULT_DTYPE.itemsize * nflows]


def _next_cpu(fn, what: str, flows: np.ndarray, dtype, res: np.ndarray, res_dtype) -> None:
    _planned(flows, dtype, f"{what}: the flows as a writeable contiguous array of their dtype")
    _planned(res, res_dtype, f"{what}: the results as a writeable contiguous array of their dtype")
    if res.size != flows.size:
        raise ValueError("one result per flow")
    _check(fn(_aptr(flows), _aptr(res), flows.size), what)


def _next_dev(fn, what: str, flows_t, per: int, res_t, res_per: int, stream) -> None:
    nflows = _nbytes(flows_t) // per
    _need(res_t, "res_t", res_per, nflows, "flow")
    s = _stream(stream, flows_t.device)
    _check(fn(_tptr(flows_t, nflows), _tptr(res_t, nflows), nflows, s.cuda_stream), what)


def lro_next_cpu(flows: np.ndarray, res: np.ndarray) -> None:
    """lvlip_lro_next_cpu: moves the planned flows on by res["delivered"], IN
    PLACE (rcv_nxt, out_off, rcv_wnd), and zeroes res["delivered"]; what is
    left of res is the next lro_advance_carry's prev."""
    _next_cpu(_lib.lvlip_lro_next_cpu, "lvlip_lro_next_cpu", flows, LRO_FLOW_DTYPE, res, LRO_RESULT_DTYPE)


def lro_next_dev(flows_t, res_t, stream=None) -> None:
    """lvlip_lro_next_dev on CUDA uint8 tensors (48 bytes per flow each), both
    updated in place.  One launch on `stream` (default: current), asynchronous."""
    _next_dev(_lib.lvlip_lro_next_dev, "lvlip_lro_next_dev", flows_t, LRO_FLOW_DTYPE.itemsize, res_t,
              LRO_RESULT_DTYPE.itemsize, stream)


# ------------------------------------- f1 on the device: the acknowledgement --

# struct lvlip_ack_tmpl (include/lvlip_skb.h), 64 B
ACK_TMPL_DTYPE = np.dtype([("out_off", "<u8"), ("hdr", "u1", (54,)), ("max_sack", "u1"), ("reserved", "u1")])
assert ACK_TMPL_DTYPE.itemsize == 64
ACK_MAX_FRAME = 90
ACK_ALL = 1


def ack_tmpl(hdr, out_off: int = 0, max_sack: int = 4) -> np.ndarray:
    """One ACK_TMPL_DTYPE record from the 54 header bytes of the connection's
    own pure ACK."""
    r = np.zeros(1, dtype=ACK_TMPL_DTYPE)
    r["out_off"], r["max_sack"] = out_off, max_sack
    r["hdr"][0] = np.frombuffer(bytes(hdr)[:54], dtype=np.uint8)
    return r


def ack_plan(tmpl: np.ndarray, flows: np.ndarray) -> int:
    """lvlip_ack_plan: validates the templates against the planned flows
    (template k answers flow k).  Returns out_bytes; ValueError for a refused
    plan."""
    _planned(tmpl, ACK_TMPL_DTYPE, "tmpl: a contiguous ACK_TMPL_DTYPE array", writeable=False)
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    if tmpl.size != flows.size:
        raise ValueError("one template per flow")
    out_bytes = ctypes.c_uint64(0)
    _plan_ok(int(_lib.lvlip_ack_plan(_aptr(tmpl), _aptr(flows), flows.size, ctypes.byref(out_bytes))),
             "refused templates (header, max_sack, reserved, not the flow's reverse, overlapping slots, too many)")
    return int(out_bytes.value)


def ack_cpu(tmpl: np.ndarray, flows: np.ndarray, res: np.ndarray, flags: int = 0,
            out: Optional[np.ndarray] = None):
    """lvlip_ack_cpu: plans the templates and builds the ACK frames on the
    calling thread.  Returns (out, fd): the frame buffer (a new zeroed one of
    the plan's out_bytes unless `out` is given, which then keeps its bytes
    outside the frames) and the FRAME_DESC_DTYPE descriptors, one per flow."""
    out_bytes = ack_plan(tmpl, flows)
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    res = np.ascontiguousarray(res, dtype=LRO_RESULT_DTYPE)
    if res.size != flows.size:
        raise ValueError("one result per flow")
    out = _out_u8(out, out_bytes)
    fd = np.zeros(flows.size, dtype=FRAME_DESC_DTYPE)
    _check(_lib.lvlip_ack_cpu(_aptr(tmpl), _aptr(flows), _aptr(res), flows.size, flags, out.ctypes.data, _aptr(fd)),
           "lvlip_ack_cpu")
    return out, fd


def ack_dev(tmpl_t, flows_t, res_t, flags: int, out_t, fd_t=None, stream=None):
    """lvlip_ack_dev on CUDA uint8 tensors: tmpl_t the planned templates' bytes
    (64 each), flows_t the planned flows' bytes (48 each), res_t 48 bytes per
    flow (what lro_advance_dev returned), out_t the frame buffer (at least the
    plan's out_bytes), fd_t (optional) 16 bytes per flow for the frame
    descriptors.  One launch on `stream` (default: current), asynchronous."""
    nflows = _nbytes(flows_t) // LRO_FLOW_DTYPE.itemsize
    _need(tmpl_t, "tmpl_t", ACK_TMPL_DTYPE.itemsize, nflows, "flow")
    _need(res_t, "res_t", LRO_RESULT_DTYPE.itemsize, nflows, "flow")
    _need(fd_t, "fd_t", 16, nflows, "flow", optional=True)
    s = _stream(stream, out_t.device)
    _check(_lib.lvlip_ack_dev(tmpl_t.data_ptr(), flows_t.data_ptr(), res_t.data_ptr(), nflows, flags,
                              out_t.data_ptr(), _tptr(fd_t), s.cuda_stream), "lvlip_ack_dev")


# ------------------------- f2 on the device: the ACK side and the retransmit --

# struct lvlip_snd_flow / lvlip_snd_result (include/lvlip_skb.h), 32 B each
SND_FLOW_DTYPE = np.dtype([("snd_una", "<u4"), ("snd_nxt", "<u4"), ("seg0", "<u4"), ("nseg", "<u4"),
                           ("slot0", "<u4"), ("rtx", "<u4"), ("win", "<u2"), ("reserved", "<u2"),
                           ("reserved2", "<u4")])
SND_RESULT_DTYPE = np.dtype([("snd_una", "<u4"), ("acked", "<u4"), ("n_new", "<u4"), ("n_dup", "<u4"),
                             ("n_old", "<u4"), ("n_beyond", "<u4"), ("popped", "<u4"), ("inflight", "<u4")])
assert SND_FLOW_DTYPE.itemsize == 32 and SND_RESULT_DTYPE.itemsize == 32


def snd_plan(snd: np.ndarray):
    """lvlip_snd_plan: validates the flows' send sides and fills slot0 in
    place.  Returns (nslots, nfd); ValueError for a refused plan."""
    _planned(snd, SND_FLOW_DTYPE, "snd: a writeable contiguous SND_FLOW_DTYPE array")
    nfd = ctypes.c_uint32(0)
    n = _plan_ok(int(_lib.lvlip_snd_plan(_aptr(snd), snd.size, ctypes.byref(nfd))),
                 "refused send sides (reserved bytes, snd_nxt - snd_una, overlapping queues, too many)")
    return n, int(nfd.value)


def _ring(base, fdescs, snd):
    buf = _u8_inplace(base)
    fd = np.ascontiguousarray(fdescs, dtype=FRAME_DESC_DTYPE)
    ends = snd["seg0"].astype(np.uint64) + snd["nseg"]
    if ((snd["nseg"] > 0) & (ends > fd.size)).any():
        raise ValueError("a queue lies past fd")
    if (fd["offset"] + fd["len"].astype(np.uint64) > buf.size).any():
        raise ValueError("a frame lies past the ring")
    return buf, fd


def snd_cpu(flows: np.ndarray, snd: np.ndarray, rec: np.ndarray, base, fdescs: np.ndarray) -> np.ndarray:
    """lvlip_snd_cpu: the ACK side of one lro_* call's records.  flows the
    planned LRO_FLOW_DTYPE array, snd as snd_plan left it, base / fdescs the TX
    ring that holds the write queues.  Returns SND_RESULT_DTYPE per flow
    (zeros when there is no record: the call is a no-op then)."""
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    snd = np.ascontiguousarray(snd, dtype=SND_FLOW_DTYPE)
    rec = np.ascontiguousarray(rec, dtype=LRO_REC_DTYPE)
    if snd.size != flows.size:
        raise ValueError("one send side per flow")
    buf, fd = _ring(base, fdescs, snd)
    res = np.zeros(flows.size, dtype=SND_RESULT_DTYPE)
    _check(_lib.lvlip_snd_cpu(_aptr(flows), _aptr(snd), flows.size, _aptr(rec), rec.size, _aptr(buf, True),
                              _aptr(fd, True), _aptr(res)), "lvlip_snd_cpu")
    return res


def snd_dev(flows_t, snd_t, rec_t, base_t, fd_t, res_t=None, stream=None):
    """lvlip_snd_dev on CUDA uint8 tensors: flows_t the planned flows' bytes
    (48 each), snd_t the planned send sides' (32 each), rec_t 16 bytes per
    record (what lro_dev returned), base_t / fd_t the TX ring and its
    descriptors.  Returns res_t, 32 bytes per flow (a new tensor unless
    given).  Asynchronous on `stream` (default: current)."""
    nflows = _nbytes(flows_t) // LRO_FLOW_DTYPE.itemsize
    n = _records(rec_t, 16)
    _need(snd_t, "snd_t", SND_FLOW_DTYPE.itemsize, nflows, "flow")
    res_t = _result(res_t, "res_t", SND_RESULT_DTYPE.itemsize, nflows, "flow", flows_t.device, zeroed=True)
    s = _stream(stream, flows_t.device)
    _check(_lib.lvlip_snd_dev(flows_t.data_ptr(), snd_t.data_ptr(), nflows, _tptr(rec_t, n), n, base_t.data_ptr(),
                              fd_t.data_ptr(), res_t.data_ptr(), s.cuda_stream), "lvlip_snd_dev")
    return res_t[:SND_RESULT_DTYPE.itemsize * nflows]


def snd_next_cpu(snd: np.ndarray, res: np.ndarray) -> None:
    """lvlip_snd_next_cpu: moves the planned send sides on by res["popped"],
    IN PLACE (snd_una, seg0, nseg), and consumes res (popped, acked 0; inflight
    the queue's length)."""
    _next_cpu(_lib.lvlip_snd_next_cpu, "lvlip_snd_next_cpu", snd, SND_FLOW_DTYPE, res, SND_RESULT_DTYPE)


def snd_next_dev(snd_t, res_t, stream=None) -> None:
    """lvlip_snd_next_dev on CUDA uint8 tensors (32 bytes per flow each), both
    updated in place.  One launch on `stream` (default: current), asynchronous."""
    _next_dev(_lib.lvlip_snd_next_dev, "lvlip_snd_next_dev", snd_t, SND_FLOW_DTYPE.itemsize, res_t,
              SND_RESULT_DTYPE.itemsize, stream)


def _rtx_cpu(flows, lro_res, snd, snd_res, sacked, base, fdescs, selective: bool):
    """rtx_cpu and, with `selective`, rtx_sack_cpu: lvlip_rtx_sack_cpu takes
    lvlip_rtx_cpu's arguments plus the scoreboard and the picks.  Returns
    (fd_out, pick); pick is None unless selective."""
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    snd = np.ascontiguousarray(snd, dtype=SND_FLOW_DTYPE)
    if snd.size != flows.size:
        raise ValueError("one send side per flow")
    if not _is_u8(base, writeable=True):
        raise TypeError("base: a writeable contiguous uint8 array (the ring is rewritten in place)")
    _, fd = _ring(base, fdescs, snd)
    if sacked is not None:
        sacked = np.ascontiguousarray(sacked, dtype=np.uint8)
        if sacked.size < fd.size:
            raise ValueError("sacked: one byte per fd entry")
    if lro_res is not None:
        lro_res = np.ascontiguousarray(lro_res, dtype=LRO_RESULT_DTYPE)
    if snd_res is not None:
        snd_res = np.ascontiguousarray(snd_res, dtype=SND_RESULT_DTYPE)
    if any(r is not None and r.size != flows.size for r in (lro_res, snd_res)):
        raise ValueError("one result per flow")
    nslots = int(snd["rtx"].astype(np.uint64).sum()) if snd.size else 0
    fd_out = np.zeros(nslots, dtype=FRAME_DESC_DTYPE)
    head = (_aptr(flows), _aptr(lro_res), _aptr(snd), _aptr(snd_res))
    tail = (flows.size, nslots, _aptr(base, True), _aptr(fd, True), _aptr(fd_out))
    if not selective:
        _check(_lib.lvlip_rtx_cpu(*head, *tail), "lvlip_rtx_cpu")
        return fd_out, None
    pick = np.full(nslots, SACK_NO_PICK, dtype=np.uint32)
    _check(_lib.lvlip_rtx_sack_cpu(*head, _aptr(sacked), *tail, _aptr(pick)), "lvlip_rtx_sack_cpu")
    return fd_out, pick


def _rtx_dev(flows_t, lro_res_t, snd_t, snd_res_t, sacked_t, nslots, base_t, fd_t, fd_out_t, pick_t, stream,
             selective: bool):
    """rtx_dev and, with `selective`, rtx_sack_dev, as _rtx_cpu."""
    nflows = _nbytes(flows_t) // LRO_FLOW_DTYPE.itemsize
    _need(snd_t, "snd_t", SND_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(lro_res_t, "lro_res_t", LRO_RESULT_DTYPE.itemsize, nflows, "flow", optional=True)
    _need(snd_res_t, "snd_res_t", SND_RESULT_DTYPE.itemsize, nflows, "flow", optional=True)
    fd_out_t = _result(fd_out_t, "fd_out_t", 16, nslots, "slot", base_t.device)
    if selective:
        pick_t = _result(pick_t, "pick_t", 4, nslots, "slot", base_t.device)
    s = _stream(stream, base_t.device)
    head = (flows_t.data_ptr(), _tptr(lro_res_t), snd_t.data_ptr(), _tptr(snd_res_t))
    tail = (nflows, nslots, base_t.data_ptr(), fd_t.data_ptr(), fd_out_t.data_ptr())
    if not selective:
        _check(_lib.lvlip_rtx_dev(*head, *tail, s.cuda_stream), "lvlip_rtx_dev")
        return fd_out_t[:16 * nslots], None
    _check(_lib.lvlip_rtx_sack_dev(*head, _tptr(sacked_t), *tail, pick_t.data_ptr(), s.cuda_stream),
           "lvlip_rtx_sack_dev")
    return fd_out_t[:16 * nslots], pick_t[:4 * nslots]


def rtx_cpu(flows: np.ndarray, lro_res, snd: np.ndarray, snd_res, base: np.ndarray, fdescs: np.ndarray) -> np.ndarray:
    """lvlip_rtx_cpu: rewrites the live frames at the head of every queue IN
    PLACE in `base` (a writeable contiguous uint8 array).  lro_res
    (LRO_RESULT_DTYPE per flow) and snd_res (SND_RESULT_DTYPE per flow) may be
    None.  Returns fd_out, FRAME_DESC_DTYPE per slot ({0, 0, 0} = no frame)."""
    return _rtx_cpu(flows, lro_res, snd, snd_res, None, base, fdescs, False)[0]


def rtx_dev(flows_t, lro_res_t, snd_t, snd_res_t, nslots: int, base_t, fd_t, fd_out_t=None, stream=None):
    """lvlip_rtx_dev on CUDA uint8 tensors: one launch that rewrites the live
    frames in base_t in place.  lro_res_t (48 bytes per flow) and snd_res_t (32
    per flow) may be None; nslots is what snd_plan returned.  Returns
    fd_out_t, 16 bytes per slot (a new tensor unless given).  Asynchronous on
    `stream` (default: current)."""
    return _rtx_dev(flows_t, lro_res_t, snd_t, snd_res_t, None, nslots, base_t, fd_t, fd_out_t, None, stream, False)[0]


# struct lvlip_sack_result (include/lvlip_skb.h), 16 B
SACK_RESULT_DTYPE = np.dtype([("n_blocks", "<u4"), ("n_valid", "<u4"), ("n_sacked", "<u4"), ("high", "<u4")])
SACK_NO_PICK = 0xFFFFFFFF


def sack_workspace_bytes(n: int, nflows: int) -> int:
    """lvlip_sack_workspace_bytes: bytes of device workspace sack_dev needs
    (0 without a device, for n == 0 and for n above 2^30 - 1)."""
    return int(_lib.lvlip_sack_workspace_bytes(n, nflows))


def sack_cpu(flows: np.ndarray, snd: np.ndarray, rec: np.ndarray, ack_base, ack_fdescs: np.ndarray, base,
             fdescs: np.ndarray, sacked: np.ndarray) -> np.ndarray:
    """lvlip_sack_cpu: marks IN PLACE in `sacked` (a writeable contiguous uint8
    array, one byte per fd index) the queue entries that the SACK blocks of the
    ACK frames ack_fdescs inside ack_base cover; rec their records, one per
    frame.  Returns SACK_RESULT_DTYPE per flow (zeros when the call is a
    no-op)."""
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    snd = np.ascontiguousarray(snd, dtype=SND_FLOW_DTYPE)
    rec = np.ascontiguousarray(rec, dtype=LRO_REC_DTYPE)
    if snd.size != flows.size:
        raise ValueError("one send side per flow")
    if not _is_u8(sacked, writeable=True):
        raise TypeError("sacked: a writeable contiguous uint8 array (the scoreboard is marked in place)")
    buf, fd = _ring(base, fdescs, snd)
    if sacked.size < fd.size:
        raise ValueError("sacked: one byte per fd entry")
    abuf = _u8_inplace(ack_base)
    afd = np.ascontiguousarray(ack_fdescs, dtype=FRAME_DESC_DTYPE)
    if afd.size != rec.size:
        raise ValueError("one record per ACK frame")
    if (afd["offset"] + afd["len"].astype(np.uint64) > abuf.size).any():
        raise ValueError("an ACK frame lies past ack_base")
    res = np.zeros(flows.size, dtype=SACK_RESULT_DTYPE)
    _check(_lib.lvlip_sack_cpu(_aptr(flows), _aptr(snd), flows.size, _aptr(rec), _aptr(abuf, True), _aptr(afd),
                               rec.size, _aptr(buf, True), _aptr(fd, True), _aptr(sacked, True), _aptr(res)),
           "lvlip_sack_cpu")
    return res


def sack_dev(flows_t, snd_t, rec_t, ack_base_t, ack_fd_t, base_t, fd_t, sacked_t, res_t=None, workspace_t=None,
             stream=None):
    """lvlip_sack_dev on CUDA uint8 tensors: marks sacked_t (one byte per fd
    entry) in place.  rec_t 16 bytes per ACK frame, ack_fd_t their descriptors
    inside ack_base_t, base_t / fd_t the TX ring.  Returns res_t, 16 bytes per
    flow (a new tensor unless given).  workspace_t: at least
    sack_workspace_bytes(n, nflows) bytes, 256-B aligned (allocated here unless
    given).  Asynchronous on `stream` (default: current)."""
    import torch

    nflows = _nbytes(flows_t) // LRO_FLOW_DTYPE.itemsize
    n = _records(rec_t, 16)
    _need(snd_t, "snd_t", SND_FLOW_DTYPE.itemsize, nflows, "flow")
    if n:
        _need(ack_fd_t, "ack_fd_t", 16, n, "record")
    res_t = _result(res_t, "res_t", SACK_RESULT_DTYPE.itemsize, nflows, "flow", flows_t.device, zeroed=True)
    if workspace_t is None:
        workspace_t = torch.empty(max(sack_workspace_bytes(n, nflows), 256), dtype=torch.uint8,
                                  device=flows_t.device)
    s = _stream(stream, flows_t.device)
    # an empty batch sends rec, ack_base and ack_fd down as NULL, whatever the caller gave
    _check(_lib.lvlip_sack_dev(flows_t.data_ptr(), snd_t.data_ptr(), nflows, _tptr(rec_t, n),
                               ack_base_t.data_ptr() if n else None, ack_fd_t.data_ptr() if n else None, n,
                               base_t.data_ptr(), fd_t.data_ptr(), sacked_t.data_ptr(), res_t.data_ptr(),
                               workspace_t.data_ptr(), _nbytes(workspace_t), s.cuda_stream), "lvlip_sack_dev")
    return res_t[:SACK_RESULT_DTYPE.itemsize * nflows]


def rtx_sack_cpu(flows: np.ndarray, lro_res, snd: np.ndarray, snd_res, sacked, base: np.ndarray, fdescs: np.ndarray):
    """lvlip_rtx_sack_cpu: rtx_cpu over the first entries of every queue whose
    byte in `sacked` (uint8 per fd index, or None) is 0.  Rewrites `base` in
    place.  Returns (fd_out, pick): FRAME_DESC_DTYPE and the uint32 fd index
    per slot (SACK_NO_PICK for a dead slot)."""
    return _rtx_cpu(flows, lro_res, snd, snd_res, sacked, base, fdescs, True)


def rtx_sack_dev(flows_t, lro_res_t, snd_t, snd_res_t, sacked_t, nslots: int, base_t, fd_t, fd_out_t=None,
                 pick_t=None, stream=None):
    """lvlip_rtx_sack_dev on CUDA uint8 tensors: the selection pass, then
    rtx_dev's kernel over the picked entries.  sacked_t (one byte per fd entry),
    lro_res_t and snd_res_t may be None.  Returns (fd_out_t, pick_t): 16 and 4
    bytes per slot (new tensors unless given).  Asynchronous on `stream`
    (default: current)."""
    return _rtx_dev(flows_t, lro_res_t, snd_t, snd_res_t, sacked_t, nslots, base_t, fd_t, fd_out_t, pick_t, stream,
                    True)


# ------------------------------------------- f2 on the device: the write queue --

# struct lvlip_push_flow (112 B) / lvlip_push_result (16 B), include/lvlip_skb.h
PUSH_FLOW_DTYPE = np.dtype([("pay_off", "<u8"), ("ring_off", "<u8"), ("unsent", "<u4"), ("stride", "<u4"),
                            ("cap", "<u4"), ("q0", "<u4"), ("slot_nxt", "<u4"), ("push", "<u4"), ("slot0", "<u4"),
                            ("wnd", "<u4"), ("mss", "<u2"), ("reserved", "<u2"), ("hdr", "u1", (54,)),
                            ("pad", "u1", (6,))])
PUSH_RESULT_DTYPE = np.dtype([("pushed", "<u4"), ("bytes", "<u4"), ("first", "<u4"), ("moved", "<u4")])
PUSH_NO_LIMIT = 0x40000000
assert PUSH_FLOW_DTYPE.itemsize == 112 and PUSH_RESULT_DTYPE.itemsize == 16


def push_flow(hdr, pay_off: int, unsent: int, mss: int, ring_off: int, cap: int, q0: int, push: int,
              stride: int = 0, wnd: int = PUSH_NO_LIMIT, slot_nxt: int = 0) -> np.ndarray:
    """One lvlip_push_flow (a 1-element PUSH_FLOW_DTYPE array); stride 0 means
    54 + mss."""
    w = np.zeros(1, dtype=PUSH_FLOW_DTYPE)
    w["pay_off"], w["unsent"], w["mss"], w["ring_off"], w["cap"], w["q0"] = pay_off, unsent, mss, ring_off, cap, q0
    w["push"], w["stride"], w["wnd"], w["slot_nxt"] = push, stride or 54 + mss, wnd, slot_nxt
    w["hdr"][0] = np.frombuffer(bytes(hdr), dtype=np.uint8)
    return w


def push_plan(push: np.ndarray, snd: np.ndarray):
    """lvlip_push_plan: validates the write sides against the send sides and
    fills slot0 in place.  Returns (nslots, ring_bytes, nfd); ValueError for a
    refused plan."""
    _planned(push, PUSH_FLOW_DTYPE, "push: a writeable contiguous PUSH_FLOW_DTYPE array")
    _planned(snd, SND_FLOW_DTYPE, "snd: a contiguous SND_FLOW_DTYPE array", writeable=False)
    if snd.size != push.size:
        raise ValueError("one send side per write side")
    ring_bytes, nfd = ctypes.c_uint64(0), ctypes.c_uint32(0)
    n = _plan_ok(int(_lib.lvlip_push_plan(_aptr(push), _aptr(snd), push.size, ctypes.byref(ring_bytes),
                                          ctypes.byref(nfd))),
                 "refused write sides (template, cap, slot_nxt, mss, stride, unsent, wnd, reserved bytes, "
                 "overlapping regions, a queue outside its region, too many)")
    return n, int(ring_bytes.value), int(nfd.value)


def push_cpu(flows: np.ndarray, lro_res, snd: np.ndarray, push: np.ndarray, payload, base: np.ndarray,
             fdescs: np.ndarray, sacked=None):
    """lvlip_push_cpu: compacts every queue to its q0 and appends up to `push`
    new segments per flow, IN PLACE in snd, push, base (the ring), fdescs and
    sacked (uint8 per fd index, or None).  lro_res (LRO_RESULT_DTYPE per flow)
    may be None.  Returns (fd_out, res): FRAME_DESC_DTYPE per slot ({0, 0, 0} =
    no frame) and PUSH_RESULT_DTYPE per flow."""
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    _planned(snd, SND_FLOW_DTYPE, "snd: a writeable contiguous SND_FLOW_DTYPE array")
    _planned(push, PUSH_FLOW_DTYPE, "push: a writeable contiguous PUSH_FLOW_DTYPE array")
    _planned(fdescs, FRAME_DESC_DTYPE, "fdescs: a writeable contiguous FRAME_DESC_DTYPE array")
    if snd.size != flows.size or push.size != flows.size:
        raise ValueError("one send side and one write side per flow")
    if not _is_u8(base, writeable=True):
        raise TypeError("base: a writeable contiguous uint8 array (frames are built in place)")
    if sacked is not None and not _is_u8(sacked, writeable=True):
        raise TypeError("sacked: a writeable contiguous uint8 array")
    pay = _u8_inplace(payload)
    if lro_res is not None:
        lro_res = np.ascontiguousarray(lro_res, dtype=LRO_RESULT_DTYPE)
        if lro_res.size != flows.size:
            raise ValueError("one result per flow")
    if push.size:
        if int((push["q0"].astype(np.uint64) + push["cap"]).max()) > min(fdescs.size, sacked.size if sacked is not None
                                                                         else fdescs.size):
            raise ValueError("a region lies past fd or sacked")
        if int((push["ring_off"] + (push["cap"].astype(np.uint64) - 1) * push["stride"] + 54 + push["mss"]).max()) \
                > base.size:
            raise ValueError("a slot lies past the ring")
        if int((push["pay_off"] + push["unsent"]).max()) > pay.size:
            raise ValueError("unsent bytes lie past the payload")
    nslots = int(push["push"].astype(np.uint64).sum()) if push.size else 0
    fd_out = np.zeros(nslots, dtype=FRAME_DESC_DTYPE)
    res = np.zeros(flows.size, dtype=PUSH_RESULT_DTYPE)
    _check(_lib.lvlip_push_cpu(_aptr(flows), _aptr(lro_res), _aptr(snd), _aptr(push), flows.size, nslots,
                               _aptr(pay, True), _aptr(base, True), _aptr(fdescs, True), _aptr(sacked),
                               _aptr(fd_out, True), _aptr(res)), "lvlip_push_cpu")
    return fd_out, res


def push_dev(flows_t, lro_res_t, snd_t, push_t, nslots: int, payload_t, base_t, fd_t, sacked_t=None, fd_out_t=None,
             res_t=None, stream=None):
    """lvlip_push_dev on CUDA uint8 tensors: flows_t 48, snd_t 32 and push_t 112
    bytes per flow (snd_t and push_t are updated in place), base_t the ring,
    fd_t its descriptors, sacked_t (may be None) the scoreboard; nslots is what
    push_plan returned.  lro_res_t (48 bytes per flow) may be None.  Returns
    (fd_out_t, res_t): 16 bytes per slot and 16 per flow (new tensors unless
    given).  Three launches on `stream` (default: current), asynchronous."""
    nflows = _nbytes(flows_t) // LRO_FLOW_DTYPE.itemsize
    _need(snd_t, "snd_t", SND_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(push_t, "push_t", PUSH_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(lro_res_t, "lro_res_t", LRO_RESULT_DTYPE.itemsize, nflows, "flow", optional=True)
    fd_out_t = _result(fd_out_t, "fd_out_t", 16, nslots, "slot", base_t.device)
    res_t = _result(res_t, "res_t", PUSH_RESULT_DTYPE.itemsize, nflows, "flow", base_t.device)
    s = _stream(stream, base_t.device)
    _check(_lib.lvlip_push_dev(flows_t.data_ptr(), _tptr(lro_res_t), snd_t.data_ptr(), push_t.data_ptr(), nflows,
                               nslots, payload_t.data_ptr(), base_t.data_ptr(), fd_t.data_ptr(), _tptr(sacked_t),
                               fd_out_t.data_ptr(), res_t.data_ptr(), s.cuda_stream), "lvlip_push_dev")
    return fd_out_t[:16 * nslots], res_t[:PUSH_RESULT_DTYPE.itemsize * nflows]


# ------------------------ f2 on the device: the timer and the peer's window --

# struct lvlip_rto_flow (32 B) / lvlip_rto_result / lvlip_wnd_result (16 B each), include/lvlip_skb.h
RTO_FLOW_DTYPE = np.dtype([("srtt", "<i4"), ("rttvar", "<i4"), ("rto", "<u4"), ("expires", "<u4"),
                           ("dupacks", "<u4"), ("snd_wnd", "<u4"), ("wnd_cap", "<u4"), ("armed", "u1"),
                           ("backoff", "u1"), ("dead", "u1"), ("wscale", "u1")])
RTO_RESULT_DTYPE = np.dtype([("fired", "<u4"), ("sample", "<u4"), ("rto", "<u4"), ("backoff", "<u4")])
WND_RESULT_DTYPE = np.dtype([("n_counting", "<u4"), ("winner", "<u4"), ("raw", "<u4"), ("snd_wnd", "<u4")])
RTO_FAST, RTO_TIMEOUT, RTO_FASTRTX, RTO_NO_SAMPLE = 1, 1, 2, 0xFFFFFFFF
WND_APPLY, WND_NO_WINNER = 1, 0xFFFFFFFF
assert RTO_FLOW_DTYPE.itemsize == 32 and RTO_RESULT_DTYPE.itemsize == 16 and WND_RESULT_DTYPE.itemsize == 16


def rto_flows(nflows: int, rto: int = 1000, wnd_cap: int = PUSH_NO_LIMIT, snd_wnd: int = PUSH_NO_LIMIT,
              wscale: int = 0) -> np.ndarray:
    """nflows fresh lvlip_rto_flow states: rto 1000 ms (src/tcp_input.c:196),
    no sample, no timer, the window open until an ACK says otherwise."""
    t = np.zeros(nflows, dtype=RTO_FLOW_DTYPE)
    t["rto"], t["wnd_cap"], t["snd_wnd"], t["wscale"] = rto, wnd_cap, snd_wnd, wscale
    return t


def rto_check(rto: np.ndarray) -> None:
    """lvlip_rto_check: ValueError for a state the calls refuse."""
    _planned(rto, RTO_FLOW_DTYPE, "rto: a contiguous RTO_FLOW_DTYPE array", writeable=False)
    if _lib.lvlip_rto_check(_aptr(rto), rto.size) != OK:
        raise ValueError("refused timer state (wscale, snd_wnd, wnd_cap, armed, dead, too many)")


def wnd_cpu(flows: np.ndarray, snd: np.ndarray, rto: np.ndarray, push, rec: np.ndarray, ack_base,
            ack_fdescs: np.ndarray, flags: int = 0) -> np.ndarray:
    """lvlip_wnd_cpu: the peer's window from the ACK frames ack_fdescs inside
    ack_base (rec their records), IN PLACE in rto["snd_wnd"] and, with
    WND_APPLY, in push["wnd"] (push may be None).  Returns WND_RESULT_DTYPE per
    flow."""
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    snd = np.ascontiguousarray(snd, dtype=SND_FLOW_DTYPE)
    rec = np.ascontiguousarray(rec, dtype=LRO_REC_DTYPE)
    _planned(rto, RTO_FLOW_DTYPE, "rto: a writeable contiguous RTO_FLOW_DTYPE array")
    if push is not None:
        _planned(push, PUSH_FLOW_DTYPE, "push: a writeable contiguous PUSH_FLOW_DTYPE array")
    if snd.size != flows.size or rto.size != flows.size or (push is not None and push.size != flows.size):
        raise ValueError("one send side, one timer state and one write side per flow")
    abuf = _u8_inplace(ack_base)
    afd = np.ascontiguousarray(ack_fdescs, dtype=FRAME_DESC_DTYPE)
    if afd.size != rec.size:
        raise ValueError("one record per ACK frame")
    if (afd["offset"] + afd["len"].astype(np.uint64) > abuf.size).any():
        raise ValueError("an ACK frame lies past ack_base")
    res = np.zeros(flows.size, dtype=WND_RESULT_DTYPE)
    _check(_lib.lvlip_wnd_cpu(_aptr(flows), _aptr(snd), _aptr(rto), _aptr(push), flows.size, _aptr(rec),
                              _aptr(abuf, True) if rec.size else None, _aptr(afd), rec.size, flags, _aptr(res)),
           "lvlip_wnd_cpu")
    return res


def wnd_dev(flows_t, snd_t, rto_t, push_t, rec_t, ack_base_t, ack_fd_t, flags: int = 0, res_t=None, stream=None):
    """lvlip_wnd_dev on CUDA uint8 tensors: flows_t 48, snd_t 32, rto_t 32 and
    push_t (may be None) 112 bytes per flow; rto_t and push_t are updated in
    place.  rec_t 16 bytes per ACK frame, ack_fd_t their descriptors inside
    ack_base_t.  Returns res_t, 16 bytes per flow (a new tensor unless given).
    Asynchronous on `stream` (default: current)."""
    nflows = _nbytes(flows_t) // LRO_FLOW_DTYPE.itemsize
    n = _records(rec_t, 16)
    _need(snd_t, "snd_t", SND_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(rto_t, "rto_t", RTO_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(push_t, "push_t", PUSH_FLOW_DTYPE.itemsize, nflows, "flow", optional=True)
    if n:
        _need(ack_fd_t, "ack_fd_t", 16, n, "record")
    res_t = _result(res_t, "res_t", WND_RESULT_DTYPE.itemsize, nflows, "flow", flows_t.device, zeroed=True)
    s = _stream(stream, flows_t.device)
    _check(_lib.lvlip_wnd_dev(flows_t.data_ptr(), snd_t.data_ptr(), rto_t.data_ptr(), _tptr(push_t), nflows,
                              _tptr(rec_t, n), ack_base_t.data_ptr() if n else None,
                              ack_fd_t.data_ptr() if n else None, n, flags, res_t.data_ptr(), s.cuda_stream),
           "lvlip_wnd_dev")
    return res_t[:WND_RESULT_DTYPE.itemsize * nflows]


def rto_cpu(snd: np.ndarray, snd_res, push_res, rto: np.ndarray, now: int, flags: int = 0, sacked=None):
    """lvlip_rto_cpu: one round of the retransmission timer, IN PLACE in rto
    and, for flows that timed out, in `sacked` (uint8 per fd index, or None).
    snd as snd_next_* / push_* left it; snd_res (SND_RESULT_DTYPE) and push_res
    (PUSH_RESULT_DTYPE) may be None.  Returns (gate, res): the SND_RESULT_DTYPE
    array to hand to rtx_* / rtx_sack_* as snd_res, and RTO_RESULT_DTYPE per
    flow."""
    snd = np.ascontiguousarray(snd, dtype=SND_FLOW_DTYPE)
    _planned(rto, RTO_FLOW_DTYPE, "rto: a writeable contiguous RTO_FLOW_DTYPE array")
    if snd_res is not None:
        snd_res = np.ascontiguousarray(snd_res, dtype=SND_RESULT_DTYPE)
    if push_res is not None:
        push_res = np.ascontiguousarray(push_res, dtype=PUSH_RESULT_DTYPE)
    if rto.size != snd.size or any(r is not None and r.size != snd.size for r in (snd_res, push_res)):
        raise ValueError("one timer state and one result per flow")
    if sacked is not None:
        if not _is_u8(sacked, writeable=True):
            raise TypeError("sacked: a writeable contiguous uint8 array")
        ends = snd["seg0"].astype(np.uint64) + snd["nseg"]
        if ((snd["nseg"] > 0) & (ends > sacked.size)).any():
            raise ValueError("a queue lies past sacked")
    gate = np.zeros(snd.size, dtype=SND_RESULT_DTYPE)
    res = np.zeros(snd.size, dtype=RTO_RESULT_DTYPE)
    _check(_lib.lvlip_rto_cpu(_aptr(snd), _aptr(snd_res), _aptr(push_res), _aptr(rto), snd.size, now & 0xFFFFFFFF,
                              flags, _aptr(sacked), _aptr(gate), _aptr(res)), "lvlip_rto_cpu")
    return gate, res


def rto_dev(snd_t, snd_res_t, push_res_t, rto_t, now: int, flags: int = 0, sacked_t=None, gate_t=None, res_t=None,
            stream=None):
    """lvlip_rto_dev on CUDA uint8 tensors: snd_t 32 and rto_t 32 bytes per
    flow (rto_t updated in place), snd_res_t (32 per flow) and push_res_t (16
    per flow) may be None, sacked_t (may be None) the scoreboard.  Returns
    (gate_t, res_t): 32 and 16 bytes per flow (new tensors unless given).  One
    launch on `stream` (default: current), asynchronous."""
    nflows = _nbytes(snd_t) // SND_FLOW_DTYPE.itemsize
    _need(rto_t, "rto_t", RTO_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(snd_res_t, "snd_res_t", SND_RESULT_DTYPE.itemsize, nflows, "flow", optional=True)
    _need(push_res_t, "push_res_t", PUSH_RESULT_DTYPE.itemsize, nflows, "flow", optional=True)
    gate_t = _result(gate_t, "gate_t", SND_RESULT_DTYPE.itemsize, nflows, "flow", snd_t.device)
    res_t = _result(res_t, "res_t", RTO_RESULT_DTYPE.itemsize, nflows, "flow", snd_t.device)
    s = _stream(stream, snd_t.device)
    _check(_lib.lvlip_rto_dev(snd_t.data_ptr(), _tptr(snd_res_t), _tptr(push_res_t), rto_t.data_ptr(), nflows,
                              now & 0xFFFFFFFF, flags, _tptr(sacked_t), gate_t.data_ptr(), res_t.data_ptr(),
                              s.cuda_stream), "lvlip_rto_dev")
    return gate_t[:SND_RESULT_DTYPE.itemsize * nflows], res_t[:RTO_RESULT_DTYPE.itemsize * nflows]


# ------------------------------------ f2 on the device: the congestion window --

# struct lvlip_cc_flow (32 B) / lvlip_cc_result (16 B), include/lvlip_skb.h
CC_FLOW_DTYPE = np.dtype([("cwnd", "<u4"), ("ssthresh", "<u4"), ("recover", "<u4"), ("acc", "<u4"),
                          ("cwnd_max", "<u4"), ("mss", "<u2"), ("in_rec", "u1"), ("reserved", "u1"),
                          ("reserved2", "<u4", (2,))])
CC_RESULT_DTYPE = np.dtype([("cwnd", "<u4"), ("sacked_bytes", "<u4"), ("n_sacked", "<u4"), ("event", "<u4")])
CC_FLOW, CC_RESULT = CC_FLOW_DTYPE, CC_RESULT_DTYPE
CC_MAX_WND = 0x40000000
CC_EV_TIMEOUT, CC_EV_ENTER, CC_EV_EXIT, CC_EV_SLOWSTART, CC_EV_AVOID = 0x01, 0x02, 0x04, 0x08, 0x10
assert CC_FLOW_DTYPE.itemsize == 32 and CC_RESULT_DTYPE.itemsize == 16


def cc_init(mss, cwnd_max: int = CC_MAX_WND, nflows: Optional[int] = None) -> np.ndarray:
    """Fresh lvlip_cc_flow states, one per entry of mss (or nflows of one mss):
    cwnd at RFC 5681's initial window min(4 mss, max(2 mss, 4380)), held to
    cwnd_max, ssthresh 2^30."""
    m = np.atleast_1d(np.asarray(mss, dtype=np.int64))
    if nflows is not None:
        m = np.broadcast_to(m, (nflows,))
    c = np.zeros(m.size, dtype=CC_FLOW_DTYPE)
    c["mss"], c["cwnd_max"], c["ssthresh"] = m, cwnd_max, CC_MAX_WND
    c["cwnd"] = np.minimum(np.minimum(4 * m, np.maximum(2 * m, 4380)), c["cwnd_max"])
    return c


def cc_check(cc: np.ndarray) -> None:
    """lvlip_cc_check: ValueError for a state the calls refuse."""
    _planned(cc, CC_FLOW_DTYPE, "cc: a contiguous CC_FLOW_DTYPE array", writeable=False)
    if _lib.lvlip_cc_check(_aptr(cc), cc.size) != OK:
        raise ValueError("refused congestion state (mss, cwnd, cwnd_max, ssthresh, in_rec, reserved, too many)")


def cc_cpu(snd: np.ndarray, snd_res, prev, cc: np.ndarray, rto: np.ndarray, fdescs=None, sacked=None) -> np.ndarray:
    """lvlip_cc_cpu: one round of the congestion window, IN PLACE in cc and in
    rto["wnd_cap"].  snd as the previous round's rto_* saw it; snd_res
    (SND_RESULT_DTYPE, before snd_next_*) and prev (the previous round's
    RTO_RESULT_DTYPE) may be None; sacked (uint8 per fd index) may be None, and
    then fdescs may be.  Returns CC_RESULT_DTYPE per flow."""
    snd = np.ascontiguousarray(snd, dtype=SND_FLOW_DTYPE)
    _planned(cc, CC_FLOW_DTYPE, "cc: a writeable contiguous CC_FLOW_DTYPE array")
    _planned(rto, RTO_FLOW_DTYPE, "rto: a writeable contiguous RTO_FLOW_DTYPE array")
    if snd_res is not None:
        snd_res = np.ascontiguousarray(snd_res, dtype=SND_RESULT_DTYPE)
    if prev is not None:
        prev = np.ascontiguousarray(prev, dtype=RTO_RESULT_DTYPE)
    if cc.size != snd.size or rto.size != snd.size or any(r is not None and r.size != snd.size
                                                          for r in (snd_res, prev)):
        raise ValueError("one congestion state, one timer state and one result per flow")
    if sacked is not None:
        if not _is_u8(sacked) or fdescs is None:
            raise TypeError("sacked: a contiguous uint8 array, with the queue's descriptors")
        fdescs = np.ascontiguousarray(fdescs, dtype=FRAME_DESC_DTYPE)
        ends = snd["seg0"].astype(np.uint64) + snd["nseg"]
        if ((snd["nseg"] > 0) & (ends > min(sacked.size, fdescs.size))).any():
            raise ValueError("a queue lies past sacked or fdescs")
    elif fdescs is not None:
        fdescs = np.ascontiguousarray(fdescs, dtype=FRAME_DESC_DTYPE)
    res = np.zeros(snd.size, dtype=CC_RESULT_DTYPE)
    _check(_lib.lvlip_cc_cpu(_aptr(snd), _aptr(snd_res), _aptr(prev), _aptr(cc), _aptr(rto), snd.size,
                             _aptr(fdescs, sacked is not None), _aptr(sacked, sacked is not None), _aptr(res)),
           "lvlip_cc_cpu")
    return res


def cc_dev(snd_t, snd_res_t, prev_t, cc_t, rto_t, fd_t=None, sacked_t=None, res_t=None, stream=None):
    """lvlip_cc_dev on CUDA uint8 tensors: snd_t 32, cc_t 32 and rto_t 32 bytes
    per flow (cc_t and rto_t's wnd_cap updated in place); snd_res_t (32 per
    flow) and prev_t (16 per flow) may be None; sacked_t (may be None, and then
    fd_t may be) the scoreboard of the queue entries fd_t.  Returns res_t, 16
    bytes per flow (a new tensor unless given).  Asynchronous on `stream`
    (default: current)."""
    nflows = _nbytes(snd_t) // SND_FLOW_DTYPE.itemsize
    _need(cc_t, "cc_t", CC_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(rto_t, "rto_t", RTO_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(snd_res_t, "snd_res_t", SND_RESULT_DTYPE.itemsize, nflows, "flow", optional=True)
    _need(prev_t, "prev_t", RTO_RESULT_DTYPE.itemsize, nflows, "flow", optional=True)
    if sacked_t is not None and fd_t is None:
        raise TypeError("sacked_t needs the queue's descriptors fd_t")
    res_t = _result(res_t, "res_t", CC_RESULT_DTYPE.itemsize, nflows, "flow", snd_t.device)
    s = _stream(stream, snd_t.device)
    _check(_lib.lvlip_cc_dev(snd_t.data_ptr(), _tptr(snd_res_t), _tptr(prev_t), cc_t.data_ptr(), rto_t.data_ptr(),
                             nflows, _tptr(fd_t), _tptr(sacked_t), res_t.data_ptr(), s.cuda_stream), "lvlip_cc_dev")
    return res_t[:CC_RESULT_DTYPE.itemsize * nflows]


# ---------------------------------------- f2 on the device: the persist timer --

# struct lvlip_persist_flow / lvlip_persist_result (16 B each), include/lvlip_skb.h
PERSIST_FLOW_DTYPE = np.dtype([("expires", "<u4"), ("interval", "<u4"), ("probes", "<u4"), ("armed", "u1"),
                               ("reserved", "u1", (3,))])
PERSIST_RESULT_DTYPE = np.dtype([("fired", "<u4"), ("interval", "<u4"), ("probes", "<u4"), ("seq", "<u4")])
PERSIST_MAX_MS, PERSIST_SLOT = 60000, 64
assert PERSIST_FLOW_DTYPE.itemsize == 16 and PERSIST_RESULT_DTYPE.itemsize == 16


def persist_flows(nflows: int) -> np.ndarray:
    """nflows fresh lvlip_persist_flow states: no timer."""
    return np.zeros(nflows, dtype=PERSIST_FLOW_DTYPE)


def persist_check(persist: np.ndarray) -> None:
    """lvlip_persist_check: ValueError for a state the calls refuse."""
    _planned(persist, PERSIST_FLOW_DTYPE, "persist: a contiguous PERSIST_FLOW_DTYPE array", writeable=False)
    if _lib.lvlip_persist_check(_aptr(persist), persist.size) != OK:
        raise ValueError("refused persist state (armed, reserved, interval, too many)")


def persist_cpu(flows: np.ndarray, lro_res, snd: np.ndarray, push: np.ndarray, rto: np.ndarray, persist: np.ndarray,
                now: int, out: Optional[np.ndarray] = None):
    """lvlip_persist_cpu: one round of the zero-window persist timer, IN PLACE
    in persist and in rto["dupacks"].  flows, snd and push as push_* left them;
    lro_res (LRO_RESULT_DTYPE) may be None.  Returns (out, fd_out, res): the
    probes' buffer (PERSIST_SLOT bytes per flow; the caller's `out`, or a new
    zeroed one), FRAME_DESC_DTYPE and PERSIST_RESULT_DTYPE per flow."""
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    snd = np.ascontiguousarray(snd, dtype=SND_FLOW_DTYPE)
    push = np.ascontiguousarray(push, dtype=PUSH_FLOW_DTYPE)
    _planned(rto, RTO_FLOW_DTYPE, "rto: a writeable contiguous RTO_FLOW_DTYPE array")
    _planned(persist, PERSIST_FLOW_DTYPE, "persist: a writeable contiguous PERSIST_FLOW_DTYPE array")
    if lro_res is not None:
        lro_res = np.ascontiguousarray(lro_res, dtype=LRO_RESULT_DTYPE)
    n = flows.size
    if any(a.size != n for a in (snd, push, rto, persist)) or (lro_res is not None and lro_res.size != n):
        raise ValueError("one send side, write side, timer state and persist state per flow")
    out = _out_u8(out, PERSIST_SLOT * n)
    if not out.flags.writeable:
        raise ValueError("out: writeable")
    fd_out = np.zeros(n, dtype=FRAME_DESC_DTYPE)
    res = np.zeros(n, dtype=PERSIST_RESULT_DTYPE)
    _check(_lib.lvlip_persist_cpu(_aptr(flows), _aptr(lro_res), _aptr(snd), _aptr(push), _aptr(rto), _aptr(persist),
                                  n, now & 0xFFFFFFFF, _aptr(out), _aptr(fd_out), _aptr(res)), "lvlip_persist_cpu")
    return out, fd_out, res


def persist_dev(flows_t, lro_res_t, snd_t, push_t, rto_t, persist_t, now: int, out_t, fd_out_t=None, res_t=None,
                stream=None):
    """lvlip_persist_dev on CUDA uint8 tensors: flows_t 48, snd_t 32, push_t
    112, rto_t 32 and persist_t 16 bytes per flow (persist_t and rto_t's
    dupacks updated in place), lro_res_t (48 per flow) may be None; out_t
    PERSIST_SLOT bytes per flow at any alignment.  Returns (fd_out_t, res_t):
    16 bytes per flow each (new tensors unless given).  One launch on `stream`
    (default: current), asynchronous."""
    nflows = _nbytes(flows_t) // LRO_FLOW_DTYPE.itemsize
    _need(snd_t, "snd_t", SND_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(push_t, "push_t", PUSH_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(rto_t, "rto_t", RTO_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(persist_t, "persist_t", PERSIST_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(lro_res_t, "lro_res_t", LRO_RESULT_DTYPE.itemsize, nflows, "flow", optional=True)
    _need(out_t, "out_t", PERSIST_SLOT, nflows, "flow")
    fd_out_t = _result(fd_out_t, "fd_out_t", 16, nflows, "flow", flows_t.device)
    res_t = _result(res_t, "res_t", PERSIST_RESULT_DTYPE.itemsize, nflows, "flow", flows_t.device)
    s = _stream(stream, flows_t.device)
    _check(_lib.lvlip_persist_dev(flows_t.data_ptr(), _tptr(lro_res_t), snd_t.data_ptr(), push_t.data_ptr(),
                                  rto_t.data_ptr(), persist_t.data_ptr(), nflows, now & 0xFFFFFFFF, out_t.data_ptr(),
                                  fd_out_t.data_ptr(), res_t.data_ptr(), s.cuda_stream), "lvlip_persist_dev")
    return fd_out_t[:16 * nflows], res_t[:PERSIST_RESULT_DTYPE.itemsize * nflows]


# ------------------------------------------------------ f1: the receive buffer --

# struct lvlip_rbuf_flow (48 B) / lvlip_rbuf_result (32 B), include/lvlip_skb.h
RBUF_FLOW_DTYPE = np.dtype([("base_off", "<u8"), ("sink_off", "<u8"), ("cap", "<u4"), ("head", "<u4"),
                            ("adv_edge", "<u4"), ("piece0", "<u4"), ("mss", "<u2"), ("wscale", "u1"),
                            ("reserved", "u1", (13,))])
RBUF_RESULT_DTYPE = np.dtype([("read", "<u4"), ("unread", "<u4"), ("head", "<u4"), ("moved", "<u4"), ("adv", "<u4"),
                              ("field", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
RBUF_PIECE = 16384
RBUF_MOVED, RBUF_ADVANCED, RBUF_UPDATE = 1, 2, 4
assert RBUF_FLOW_DTYPE.itemsize == 48 and RBUF_RESULT_DTYPE.itemsize == 32


def rbuf_flows(flows: np.ndarray, mss: int, wscale: int = 0, sink_off=0) -> np.ndarray:
    """Fresh lvlip_rbuf_flow states for the planned flows: the buffer is the
    flow's region as it stands, nothing read, the whole window advertised.
    sink_off: one offset per flow (or one for all).  Not yet planned."""
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    p = np.zeros(flows.size, dtype=RBUF_FLOW_DTYPE)
    p["base_off"], p["cap"] = flows["out_off"], flows["rcv_wnd"]
    p["adv_edge"] = flows["rcv_nxt"] + flows["rcv_wnd"]
    p["mss"], p["wscale"], p["sink_off"] = mss, wscale, sink_off
    return p


def rbuf_plan(rbuf: np.ndarray, flows: np.ndarray) -> int:
    """lvlip_rbuf_plan: validates the states against the planned flows and
    writes piece0 IN PLACE.  Returns the number of copy pieces; ValueError for
    a refused plan."""
    _planned(rbuf, RBUF_FLOW_DTYPE, "rbuf: a writeable contiguous RBUF_FLOW_DTYPE array")
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    if rbuf.size != flows.size:
        raise ValueError("one buffer state per flow")
    npieces = ctypes.c_uint64(0)
    _plan_ok(int(_lib.lvlip_rbuf_plan(_aptr(rbuf), _aptr(flows), flows.size, ctypes.byref(npieces))),
             "refused buffer states (an invariant against the flow, cap, mss, wscale, reserved, overlapping "
             "buffers, too many)")
    return int(npieces.value)


def rbuf_check(rbuf: np.ndarray, flows: np.ndarray) -> None:
    """lvlip_rbuf_check: ValueError for a state the calls refuse."""
    _planned(rbuf, RBUF_FLOW_DTYPE, "rbuf: a contiguous RBUF_FLOW_DTYPE array", writeable=False)
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    if rbuf.size != flows.size:
        raise ValueError("one buffer state per flow")
    rc = _lib.lvlip_rbuf_check(_aptr(rbuf), _aptr(flows), flows.size)
    if rc == EINVAL:
        raise ValueError("refused buffer state (an invariant against the flow, piece0, cap, mss, wscale, reserved, "
                         "overlapping buffers, too many)")
    _check(rc, "lvlip_rbuf_check")


def rbuf_cpu(flows: np.ndarray, res: np.ndarray, rbuf: np.ndarray, tmpl: np.ndarray, nread, out: np.ndarray,
             sink: Optional[np.ndarray] = None):
    """lvlip_rbuf_cpu: one round of the receive buffer, IN PLACE in flows
    (out_off, rcv_wnd), rbuf, tmpl (the window field), out (the moved bytes)
    and sink (the bytes read; None drops them).  res (LRO_RESULT_DTYPE) as
    lro_next_* left it; nread: uint32 per flow, or None for 0.  Returns (gate,
    rres): LRO_RESULT_DTYPE for ack_*, and RBUF_RESULT_DTYPE per flow."""
    _planned(flows, LRO_FLOW_DTYPE, "flows: a writeable contiguous LRO_FLOW_DTYPE array")
    _planned(rbuf, RBUF_FLOW_DTYPE, "rbuf: a writeable contiguous RBUF_FLOW_DTYPE array")
    _planned(tmpl, ACK_TMPL_DTYPE, "tmpl: a writeable contiguous ACK_TMPL_DTYPE array")
    res = np.ascontiguousarray(res, dtype=LRO_RESULT_DTYPE)
    n = flows.size
    if nread is not None:
        nread = np.ascontiguousarray(nread, dtype=np.uint32)
    if any(a.size != n for a in (res, rbuf, tmpl)) or (nread is not None and nread.size != n):
        raise ValueError("one result, buffer state, template and read count per flow")
    for a, what in ((out, "out"), (sink, "sink")):
        if a is not None and not _is_u8(a, writeable=True):
            raise ValueError(f"{what}: a writeable contiguous uint8 array")
    gate = np.zeros(n, dtype=LRO_RESULT_DTYPE)
    rres = np.zeros(n, dtype=RBUF_RESULT_DTYPE)
    _check(_lib.lvlip_rbuf_cpu(_aptr(flows), _aptr(res), _aptr(rbuf), _aptr(tmpl), n, _aptr(nread), _aptr(out),
                               _aptr(sink), _aptr(gate), _aptr(rres)), "lvlip_rbuf_cpu")
    return gate, rres


# ------------------------------------------------- the end of a connection --

# struct lvlip_fin_flow (32 B) / lvlip_fin_result (16 B), include/lvlip_skb.h
FIN_FLOW_DTYPE = np.dtype([("base", "<u4"), ("fin_seq", "<u4"), ("expires", "<u4"), ("interval", "<u4"),
                           ("retries", "<u4"), ("state", "u1"), ("flags", "u1"), ("reserved", "u1", (10,))])
FIN_RESULT_DTYPE = np.dtype([("events", "<u4"), ("state", "<u4"), ("seq", "<u4"), ("interval", "<u4")])
TCP_ESTABLISHED, TCP_FIN_WAIT_1, TCP_FIN_WAIT_2, TCP_CLOSED = 3, 4, 5, 6
TCP_CLOSE_WAIT, TCP_CLOSING, TCP_LAST_ACK, TCP_TIME_WAIT = 7, 8, 9, 10
FIN_CLOSE_REQ, FIN_MAX_MS, FIN_2MSL_MS = 1, 60000, 60000
FIN_EV_PEER_FIN, FIN_EV_ACK_OWED, FIN_EV_SENT, FIN_EV_RESENT = 0x01, 0x02, 0x04, 0x08
FIN_EV_ACKED, FIN_EV_TW_DONE, FIN_EV_LATE_WRITE = 0x10, 0x20, 0x40
assert FIN_FLOW_DTYPE.itemsize == 32 and FIN_RESULT_DTYPE.itemsize == 16


def fin_flows(flows: np.ndarray) -> np.ndarray:
    """Fresh lvlip_fin_flow states for the planned flows: ESTABLISHED, base =
    rcv_nxt."""
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    x = np.zeros(flows.size, dtype=FIN_FLOW_DTYPE)
    x["base"], x["state"] = flows["rcv_nxt"], TCP_ESTABLISHED
    return x


def fin_check(fin: np.ndarray, flows: np.ndarray) -> None:
    """lvlip_fin_check: ValueError for a state the calls refuse."""
    _planned(fin, FIN_FLOW_DTYPE, "fin: a contiguous FIN_FLOW_DTYPE array", writeable=False)
    flows = np.ascontiguousarray(flows, dtype=LRO_FLOW_DTYPE)
    if fin.size != flows.size:
        raise ValueError("one close state per flow")
    if _lib.lvlip_fin_check(_aptr(fin), _aptr(flows), flows.size) != OK:
        raise ValueError("refused close state (state, reserved, interval, base, too many)")


def fin_cpu(flows: np.ndarray, gin: np.ndarray, rec, snd: np.ndarray, push: np.ndarray, rto: np.ndarray,
            fin: np.ndarray, close, now: int, out: Optional[np.ndarray] = None):
    """lvlip_fin_cpu: one round of the connections' close, IN PLACE in flows
    (rcv_nxt), snd (snd_nxt) and fin.  gin (LRO_RESULT_DTYPE) is what ack_*
    would have been given, rec (LRO_REC_DTYPE, or None) the round's records,
    close one uint8 per flow or None.  Returns (out, fd_out, gate, res): the
    FINs' buffer (PERSIST_SLOT bytes per flow; the caller's `out`, or a new
    zeroed one), FRAME_DESC_DTYPE, LRO_RESULT_DTYPE for ack_* and
    FIN_RESULT_DTYPE per flow."""
    _planned(flows, LRO_FLOW_DTYPE, "flows: a writeable contiguous LRO_FLOW_DTYPE array")
    _planned(snd, SND_FLOW_DTYPE, "snd: a writeable contiguous SND_FLOW_DTYPE array")
    _planned(fin, FIN_FLOW_DTYPE, "fin: a writeable contiguous FIN_FLOW_DTYPE array")
    gin = np.ascontiguousarray(gin, dtype=LRO_RESULT_DTYPE)
    push = np.ascontiguousarray(push, dtype=PUSH_FLOW_DTYPE)
    rto = np.ascontiguousarray(rto, dtype=RTO_FLOW_DTYPE)
    rec = None if rec is None else np.ascontiguousarray(rec, dtype=LRO_REC_DTYPE)
    close = None if close is None else np.ascontiguousarray(close, dtype=np.uint8)
    n = flows.size
    if any(a.size != n for a in (gin, snd, push, rto, fin)) or (close is not None and close.size != n):
        raise ValueError("one result, send side, write side, timer state, close state and close byte per flow")
    out = _out_u8(out, PERSIST_SLOT * n)
    if not out.flags.writeable:
        raise ValueError("out: writeable")
    fd_out = np.zeros(n, dtype=FRAME_DESC_DTYPE)
    gate = np.zeros(n, dtype=LRO_RESULT_DTYPE)
    res = np.zeros(n, dtype=FIN_RESULT_DTYPE)
    _check(_lib.lvlip_fin_cpu(_aptr(flows), _aptr(gin), _aptr(rec), 0 if rec is None else rec.size, _aptr(snd),
                              _aptr(push), _aptr(rto), _aptr(fin), n, _aptr(close), now & 0xFFFFFFFF, _aptr(out),
                              _aptr(fd_out), _aptr(gate), _aptr(res)), "lvlip_fin_cpu")
    return out, fd_out, gate, res


def fin_workspace_bytes(nflows: int) -> int:
    """lvlip_fin_workspace_bytes: the device workspace fin_dev needs."""
    return int(_lib.lvlip_fin_workspace_bytes(nflows))


def fin_dev(flows_t, gin_t, rec_t, snd_t, push_t, rto_t, fin_t, close_t, now: int, out_t, gate_t, ws_t,
            fd_out_t=None, res_t=None, stream=None):
    """lvlip_fin_dev on CUDA uint8 tensors: flows_t 48, gin_t 48, snd_t 32,
    push_t 112, rto_t 32 and fin_t 32 bytes per flow (flows_t's rcv_nxt, snd_t's
    snd_nxt and fin_t updated in place); rec_t 16 bytes per record or None;
    close_t one byte per flow or None; out_t PERSIST_SLOT bytes per flow at any
    alignment; gate_t 48 bytes per flow, written; ws_t fin_workspace_bytes.
    Returns (fd_out_t, res_t): 16 bytes per flow each (new tensors unless
    given).  A memset and two launches on `stream` (default: current),
    asynchronous."""
    nflows = _nbytes(flows_t) // LRO_FLOW_DTYPE.itemsize
    n = _records(rec_t, LRO_REC_DTYPE.itemsize)
    _need(gin_t, "gin_t", LRO_RESULT_DTYPE.itemsize, nflows, "flow")
    _need(snd_t, "snd_t", SND_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(push_t, "push_t", PUSH_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(rto_t, "rto_t", RTO_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(fin_t, "fin_t", FIN_FLOW_DTYPE.itemsize, nflows, "flow")
    _need(close_t, "close_t", 1, nflows, "flow", optional=True)
    _need(out_t, "out_t", PERSIST_SLOT, nflows, "flow")
    _need(gate_t, "gate_t", LRO_RESULT_DTYPE.itemsize, nflows, "flow")
    if _nbytes(ws_t) < fin_workspace_bytes(nflows):
        raise ValueError("ws_t: fin_workspace_bytes(nflows) bytes")
    fd_out_t = _result(fd_out_t, "fd_out_t", 16, nflows, "flow", flows_t.device)
    res_t = _result(res_t, "res_t", FIN_RESULT_DTYPE.itemsize, nflows, "flow", flows_t.device)
    s = _stream(stream, flows_t.device)
    _check(_lib.lvlip_fin_dev(flows_t.data_ptr(), gin_t.data_ptr(), _tptr(rec_t, n), n, snd_t.data_ptr(),
                              push_t.data_ptr(), rto_t.data_ptr(), fin_t.data_ptr(), nflows, _tptr(close_t),
                              now & 0xFFFFFFFF, out_t.data_ptr(), fd_out_t.data_ptr(), gate_t.data_ptr(),
                              res_t.data_ptr(), ws_t.data_ptr(), s.cuda_stream), "lvlip_fin_dev")
    return fd_out_t[:16 * nflows], res_t[:FIN_RESULT_DTYPE.itemsize * nflows]


# ----------------------------------------------------- Group 4: several GPUs --

def partition_bytes(descs: np.ndarray, parts: int) -> list:
    """lvlip_partition_bytes: cuts[0..parts] of the byte-balanced contiguous
    partition (part p = descriptors [cuts[p], cuts[p+1]))."""
    d = np.ascontiguousarray(descs, dtype=DESC_DTYPE)
    cuts = np.zeros(parts + 1, dtype=np.uint32)
    _check(_lib.lvlip_partition_bytes(d.ctypes.data if d.size else None, d.size, parts, cuts.ctypes.data),
           "lvlip_partition_bytes")
    return [int(c) for c in cuts]


def batch_host_flat_multi(ctxs, base: np.ndarray, descs: np.ndarray) -> np.ndarray:
    """lvlip_csum_batch_host_flat_multi over Contexts (one per device, or
    several on one device), one host thread each."""
    base = _as_u8(base)
    d = np.ascontiguousarray(descs, dtype=DESC_DTYPE)
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
    out = np.empty(d.size, dtype=np.uint16)
    _check(_lib.lvlip_csum_batch_host_flat_multi(arr, len(ctxs), base.ctypes.data, base.size, d.ctypes.data,
                                                 d.size, out.ctypes.data), "lvlip_csum_batch_host_flat_multi")
    return out


def frames_variant_dev(mode: int, variant: int, base, fdescs, stream=None):
    """The frame calls' A/B variants (lvlip_lab_frames_dev, liblvlip_lab.so):
    mode 0 TX fill, 1 RX header on the flat sweep, 2 RX + L4; variant bits 1
    plain field stores, 2 eight loads per round, 4 block order; modes 4 / 5
    the echo reply (LVLIP_ECHO_FULL / flags 0) with the reply's store form as
    the variant (0 byte stores, 2-6 u16 stores with a cache policy).  Returns
    the per-frame status / verdict tensor."""
    import torch

    n, fd = _frames_dev(base, fdescs)
    out8 = torch.empty(max(n, 1), dtype=torch.uint8, device=base.device)
    s = _stream(stream, base.device)
    _check(lab().lvlip_lab_frames_dev(mode, variant, base.data_ptr(), fd.data_ptr(), n, out8.data_ptr(),
                                      s.cuda_stream), "lvlip_lab_frames_dev")
    return out8[:n]


def icmp_echo_reply_csum(req_csum: int) -> int:
    """f4 (RFC 1624): reply checksum field from a verified request's field, or
    CSUM_RECOMPUTE."""
    return int(_lib.lvlip_icmp_echo_reply_csum(req_csum & 0xFFFF))


def icmp_echo_reply_fill(frames) -> int:
    """In place: echo requests -> replies' ICMP part (type 0 + checksum).
    Returns how many needed a full recomputation; raises on a non-request."""
    arr, keep = frames_array(frames)
    r = int(_lib.lvlip_icmp_echo_reply_fill(arr, len(frames)))
    del keep
    if r == PLAN_MALFORMED:
        raise ValueError("not an ICMP echo request frame")
    return r


def rx_verify_cpu(frames, flags: int = 0) -> np.ndarray:
    """lvlip_rx_verify_cpu: the RX verdicts on the calling thread (no context)."""
    n = len(frames)
    arr, keep = frames_array(frames)
    verdict = np.zeros(max(n, 1), dtype=np.uint8)
    _check(_lib.lvlip_rx_verify_cpu(arr, n, flags, verdict.ctypes.data), "lvlip_rx_verify_cpu")
    del keep
    return verdict[:n]


def tx_checksum_cpu(frames) -> None:
    """lvlip_tx_checksum_cpu: the TX fill on the calling thread (no context)."""
    arr, keep = frames_array(frames)
    _check(_lib.lvlip_tx_checksum_cpu(arr, len(frames)), "lvlip_tx_checksum_cpu")
    del keep


def tx_apply(field: np.ndarray, csum: np.ndarray) -> None:
    f = np.ascontiguousarray(field, dtype=np.uint64)
    c = np.ascontiguousarray(csum, dtype=np.uint16)
    _lib.lvlip_tx_apply(f.size, f.ctypes.data, c.ctypes.data)


# ------------------------------------------------------------ host batches --

class Context:
    """lvlip_csum_ctx: pinned arena + device arena + streams, one thread at a time.

    cpu_max: host calls of at most this many packets / frames run on the
    calling thread with the library's CPU code (lvlip_csum_ctx_set_cpu_max);
    None keeps the library's default (LVLIP_CPU_MAX, else CPU_MAX_DEFAULT), 0
    sends every call to the GPU."""

    def __init__(self, device: int = 0, arena_bytes: int = 0, cpu_max: Optional[int] = None):
        self._h = ctypes.c_void_p()
        _check(_lib.lvlip_csum_ctx_create(ctypes.byref(self._h), device, arena_bytes),
               "lvlip_csum_ctx_create")
        if cpu_max is not None:
            self.set_cpu_max(cpu_max)

    def set_cpu_max(self, cpu_max: int) -> None:
        _check(_lib.lvlip_csum_ctx_set_cpu_max(self._h, int(cpu_max)), "lvlip_csum_ctx_set_cpu_max")

    @property
    def cpu_max(self) -> int:
        return int(_lib.lvlip_csum_ctx_cpu_max(self._h))

    def stats(self) -> dict:
        st = CtxStats()
        _check(_lib.lvlip_csum_ctx_stats(self._h, ctypes.byref(st)), "lvlip_csum_ctx_stats")
        return st.as_dict()

    def close(self) -> None:
        if self._h:
            _lib.lvlip_csum_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def batch_host(self, packets: Sequence, start_sums: Sequence[int]) -> np.ndarray:
        """packets: sequence of bytes-like / uint8 arrays (the skb payloads)."""
        n = len(packets)
        keep = [_as_u8(p) for p in packets]
        iov = (Iov * n)()
        for i, (a, s) in enumerate(zip(keep, start_sums)):
            iov[i].ptr = a.ctypes.data if a.size else None
            iov[i].len = a.size
            iov[i].start_sum = s & 0xFFFFFFFF
        out = np.empty(n, dtype=np.uint16)
        _check(_lib.lvlip_csum_batch_host(self._h, iov, n, out.ctypes.data),
               "lvlip_csum_batch_host")
        return out

    def batch_host_flat(self, base: np.ndarray, descs: np.ndarray) -> np.ndarray:
        base = _as_u8(base)
        descs = np.ascontiguousarray(descs, dtype=DESC_DTYPE)
        n = descs.size
        out = np.empty(n, dtype=np.uint16)
        _check(_lib.lvlip_csum_batch_host_flat(self._h, base.ctypes.data, base.size,
                                               descs.ctypes.data, n, out.ctypes.data),
               "lvlip_csum_batch_host_flat")
        return out

    def register(self, buf: np.ndarray, flags: int = REG_DMA) -> None:
        """f3: pin `buf` (a contiguous uint8 array kept alive by the caller) in
        place; batches inside it skip the pinned-arena gather."""
        a = buf.view(np.uint8).reshape(-1)
        if not a.flags.c_contiguous:
            raise ValueError("register needs a contiguous buffer")
        _check(_lib.lvlip_csum_register(self._h, a.ctypes.data, a.size, flags),
               "lvlip_csum_register")

    def unregister(self, buf: np.ndarray) -> None:
        _check(_lib.lvlip_csum_unregister(self._h, buf.ctypes.data), "lvlip_csum_unregister")

    def rx_verify(self, frames, flags: int = 0) -> np.ndarray:
        """lvlip_rx_verify (f1): one verdict per frame (RX_*), frames untouched."""
        n = len(frames)
        arr, keep = frames_array(frames)
        verdict = np.zeros(max(n, 1), dtype=np.uint8)
        _check(_lib.lvlip_rx_verify(self._h, arr, n, flags, verdict.ctypes.data),
               "lvlip_rx_verify")
        del keep
        return verdict[:n]

    def tx_checksum(self, frames) -> None:
        """lvlip_tx_checksum (f2): fills TCP/ICMP and IPv4 checksums in place."""
        arr, keep = frames_array(frames)
        _check(_lib.lvlip_tx_checksum(self._h, arr, len(frames)), "lvlip_tx_checksum")
        del keep


# ------------------------------------------------------------------ testkit --

_testkit = None


def testkit() -> ctypes.CDLL:
    global _testkit
    if _testkit is None:
        tk = _load(TESTKIT_PATH)
        _stamp(tk, TESTKIT_PATH, "lvlip_testkit_build_id", os.path.join(HERE, "TESTKIT_SOURCES"))
        tk.lvlip_testkit_fill.restype = ctypes.c_int
        tk.lvlip_testkit_fill.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                          ctypes.c_uint64, ctypes.c_void_p]
        tk.lvlip_testkit_paint.restype = ctypes.c_int
        tk.lvlip_testkit_paint.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_uint32, ctypes.c_void_p]
        _testkit = tk
    return _testkit


_lab = None


def lab() -> ctypes.CDLL:
    """liblvlip_lab.so: read-bandwidth probes and the A/B kernels (diagnostics only)."""
    global _lab
    if _lab is None:
        lb = _load(LAB_PATH)
        _stamp(lb, LAB_PATH, "lvlip_lab_build_id", os.path.join(HERE, "LAB_SOURCES"))
        lb.lvlip_lab_probe.restype = ctypes.c_int
        lb.lvlip_lab_probe.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p]
        lb.lvlip_lab_atomics.restype = ctypes.c_int
        lb.lvlip_lab_atomics.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_uint32, ctypes.c_void_p]
        lb.lvlip_lab_probe_tl.restype = ctypes.c_int
        lb.lvlip_lab_probe_tl.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_void_p]
        lb.lvlip_lab_probe_chunk.restype = ctypes.c_int
        lb.lvlip_lab_probe_chunk.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                             ctypes.c_int, ctypes.c_void_p]
        lb.lvlip_lab_batch_dev_ex.restype = ctypes.c_int
        lb.lvlip_lab_batch_dev_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(LaunchCfg)]
        lb.lvlip_lab_frames_dev.restype = ctypes.c_int
        lb.lvlip_lab_frames_dev.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        lb.lvlip_lab_probe_pkwin.restype = ctypes.c_int
        lb.lvlip_lab_probe_pkwin.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        _lab = lb
    return _lab
