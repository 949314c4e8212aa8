#!/usr/bin/env python3
"""Generate tests/golden/tso_ref.json: the data frames the REFERENCE's own
tcp_send writes, for the segmentation calls' tests (include/lvlip_skb.h,
lvlip_tso_*).

Runs only where oracle/_ref/libref.so exists (level-ip's own src/*.c, compiled
unmodified by oracle/Makefile).  One child process per payload length drives the
stack the way tests/ref_stack_child.py drives the drop-in build: fd 0 becomes
one end of a socketpair that stands for the tap device, an ARP request teaches
the stack the peer's MAC, then

  tcp_v4_connect   the SYN                                  (src/tcp.c:156-168)
  tcp_send         the payload, queued as smss-sized skbs   (src/tcp_output.c:445-478)
  tcp_send_next    the SYN again and every data segment     (src/tcp_output.c:198-225)

and the frames with payload are collected from the socketpair.  The stack's
smss is 536 (src/tcp.c:114-115), so 2001 B gives three full segments and a ragged
tail, 1072 B an exact multiple, 1 B a single tiny segment.  Sequence numbers
and the source port are time-seeded (src/tcp.c:138-154): the tests take the
header template from each send's first recorded frame.

usage: python tests/golden/make_tso_golden.py   (from the repo root)
"""
from __future__ import annotations

import ctypes
import json
import os
import socket
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402  (SkBuff, _frame_to_skb)
import pyoracle  # noqa: E402

LENGTHS = (2001, 1072, 1)
SMSS = 536


def payload_of(length: int) -> bytes:
    return bytes(((7 * i + 3 + length) & 0xFF) for i in range(length))


def child(length: int, out_path: str) -> None:
    lib = ctypes.CDLL(pyoracle.REF_SO)
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    os.dup2(a.fileno(), 0)
    lib.netdev_init()
    lib.route_init()
    lib.arp_rcv.argtypes = [ctypes.POINTER(make_golden.SkBuff)]
    tap_mac = bytes.fromhex("0a1b2c3d4e5f")
    tap_ip, stack_ip = (10, 0, 0, 5), (10, 0, 0, 4)
    arp = (b"\xff" * 6 + tap_mac + b"\x08\x06" +
           struct.pack("!HHBBH", 1, 0x0800, 6, 4, 1) + tap_mac + bytes(tap_ip) + bytes(6) + bytes(stack_ip))
    lib.arp_rcv(make_golden._frame_to_skb(lib, arp))
    b.settimeout(2.0)
    b.recv(2048)  # the ARP reply

    lib.sk_alloc.restype = ctypes.c_void_p
    lib.sk_alloc.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.sock_init_data.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.tcp_v4_connect.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.tcp_send.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    lib.tcp_send_next.argtypes = [ctypes.c_void_p, ctypes.c_int]
    tcp_ops = ctypes.addressof(ctypes.c_char.in_dll(lib, "tcp_ops"))
    sk = lib.sk_alloc(tcp_ops, 6)
    sock = ctypes.create_string_buffer(1024)  # struct socket (include/socket.h:59-71), zeroed
    lib.sock_init_data(ctypes.addressof(sock), sk)
    addr = struct.pack("=H", socket.AF_INET) + struct.pack("!H", 8000) + bytes(tap_ip) + bytes(8)
    addr_buf = ctypes.create_string_buffer(addr, len(addr))

    nseg = (length + SMSS - 1) // SMSS
    lib.tcp_v4_connect(sk, ctypes.addressof(addr_buf), 16, 0)
    b.recv(4096)  # the SYN
    payload = payload_of(length)
    lib.tcp_send(sk, payload, len(payload))  # queued behind the SYN in flight
    lib.tcp_send_next(sk, 1 + nseg)
    got = [b.recv(4096) for _ in range(1 + nseg)]
    # the data frames: TCP header length 5 and an IP length beyond the two headers
    frames = [f for f in got if (f[46] >> 4) == 5 and struct.unpack("!H", f[16:18])[0] > 40]
    if len(frames) != nseg:
        raise SystemExit(f"{length} B: {len(frames)} data frames, expected {nseg}")
    with open(out_path, "w") as f:
        json.dump({"len": length, "payload_hex": payload.hex(), "frames": [x.hex() for x in frames]}, f)


def main() -> None:
    if pyoracle.reflib() is None:
        raise SystemExit("oracle/_ref/libref.so missing: run `make -C oracle` where the reference is present")
    sends = []
    for length in LENGTHS:
        tmp = os.path.join(HERE, f".tso_{length}.json")
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(length), tmp], check=True,
                           stdin=subprocess.DEVNULL)
            with open(tmp) as f:
                sends.append(json.load(f))
        finally:
            if os.path.exists(tmp):
                os.unlink(tmp)
    out = os.path.join(HERE, "tso_ref.json")
    with open(out, "w") as f:
        json.dump({"mss": SMSS, "sends": sends}, f, indent=1)
    print(out, os.path.getsize(out))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), sys.argv[3])
    else:
        main()
