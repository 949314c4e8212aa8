#!/usr/bin/env python3
"""Generate tests/golden/lro_ref.json: what the REFERENCE's own receive path
(tcp_input_state -> tcp_data_queue, then tcp_data_dequeue) makes of data
segments that arrive out of order and twice, for the receive-coalescing calls'
tests (include/lvlip_skb.h, lvlip_lro_*).

Runs only where oracle/_ref/libref.so exists (level-ip's own src/*.c, compiled
unmodified by oracle/Makefile).  A child process drives the stack the way
make_tso_golden.py does: fd 0 becomes one end of a socketpair that stands for
the tap device, an ARP request teaches the stack the peer's MAC, then

  tcp_v4_connect    the SYN (its source port and iss are read off the wire)
  tcp_input_state   the peer's SYN-ACK: ESTABLISHED, rcv_nxt = irs + 1
                    (src/tcp_input.c:148-214)
  tcp_input_state   7 data segments of 536 B in the order 0, 2, 1, 1, 4, 3, 6,
                    each in an skb filled as tcp_init_segment fills it
                    (src/tcp.c:36-51: header fields to host order, seq, dlen,
                    len, end_seq, payload) -> tcp_data_queue
                    (src/tcp_data.c:87-128)
  tcp_data_dequeue  what the application would read (src/tcp_data.c:49-85)

The fixture holds the frames as they were on the wire, the rcv_nxt in front
of the first of them, and the bytes and count tcp_data_dequeue returned.

usage: python tests/golden/make_lro_golden.py   (from the repo root)
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

SEG = 536
ORDER = (0, 2, 1, 1, 4, 3, 6)
IRS = 0x10000000
STACK_MAC, TAP_MAC = bytes.fromhex("000c296d5025"), bytes.fromhex("0a1b2c3d4e5f")
TAP_IP, STACK_IP = bytes((10, 0, 0, 5)), bytes((10, 0, 0, 4))


def payload_of(k: int) -> bytes:
    return bytes(((11 * i + 5 + 37 * k) & 0xFF) for i in range(SEG))


def _fold(x: int) -> int:
    while x >> 16:
        x = (x & 0xFFFF) + (x >> 16)
    return x


def frame(sport: int, dport: int, seq: int, ack: int, flags: int, data: bytes) -> bytes:
    """Peer -> stack, as a correct peer sends it (RFC pseudo header)."""
    tcp = bytearray(struct.pack("!HHIIBBHHH", sport, dport, seq, ack, 0x50, flags, 0xFFFF, 0, 0) + data)
    pseudo = sum(struct.unpack("<4H", TAP_IP + STACK_IP)) + 0x0600 + (((len(tcp) & 0xFF) << 8) | (len(tcp) >> 8))
    tcp[16:18] = struct.pack("<H", pyoracle.checksum(bytes(tcp), len(tcp), _fold(pseudo)))
    ip = bytearray(struct.pack("!BBHHHBBH4s4s", 0x45, 0, 20 + len(tcp), 0x2000, 0x4000, 64, 6, 0, TAP_IP, STACK_IP))
    ip[10:12] = struct.pack("<H", pyoracle.checksum(bytes(ip), 20, 0))
    return STACK_MAC + TAP_MAC + b"\x08\x00" + bytes(ip) + bytes(tcp)


def feed(lib, sk: int, fr: bytes) -> None:
    """tcp_in's work on one frame (src/tcp.c:57-85) with the socket known."""
    skb = make_golden._frame_to_skb(lib, fr)
    th = skb.contents.data + 34
    raw = ctypes.string_at(th, 20)
    sport, dport, seq, ack, off_flags, win, csum, urp = struct.unpack("!HHIIHHHH", raw)
    # tcp_init_segment: the multi-byte fields to host order, the flag bytes stay
    ctypes.memmove(th, struct.pack("=HHII", sport, dport, seq, ack) + raw[12:14] + struct.pack("=HHH", win, csum, urp),
                   20)
    dlen = len(fr) - 54
    flags = raw[13]
    skb.contents.seq = seq
    skb.contents.dlen = dlen
    skb.contents.len = dlen + ((flags >> 1) & 1) + (flags & 1)
    skb.contents.end_seq = (seq + dlen) & 0xFFFFFFFF
    skb.contents.payload = th + 20
    lib.tcp_input_state(sk, th, skb)


def child(out_path: str) -> None:
    lib = ctypes.CDLL(pyoracle.REF_SO)
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    os.dup2(a.fileno(), 0)
    lib.netdev_init()
    lib.route_init()
    lib.arp_rcv.argtypes = [ctypes.POINTER(make_golden.SkBuff)]
    arp = (b"\xff" * 6 + TAP_MAC + b"\x08\x06" +
           struct.pack("!HHBBH", 1, 0x0800, 6, 4, 1) + TAP_MAC + TAP_IP + bytes(6) + STACK_IP)
    lib.arp_rcv(make_golden._frame_to_skb(lib, arp))
    b.settimeout(2.0)
    b.recv(2048)  # the ARP reply

    lib.sk_alloc.restype = ctypes.c_void_p
    lib.sk_alloc.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.sock_init_data.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.tcp_v4_connect.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.tcp_input_state.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(make_golden.SkBuff)]
    lib.tcp_data_dequeue.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    tcp_ops = ctypes.addressof(ctypes.c_char.in_dll(lib, "tcp_ops"))
    sk = lib.sk_alloc(tcp_ops, 6)
    sock = ctypes.create_string_buffer(1024)  # struct socket (include/socket.h:59-71), zeroed
    lib.sock_init_data(ctypes.addressof(sock), sk)
    addr = struct.pack("=H", socket.AF_INET) + struct.pack("!H", 8000) + TAP_IP + bytes(8)
    addr_buf = ctypes.create_string_buffer(addr, len(addr))
    lib.tcp_v4_connect(sk, ctypes.addressof(addr_buf), 16, 0)
    syn = b.recv(4096)
    stack_port, peer_port, iss = struct.unpack("!HHI", syn[34:42])
    if peer_port != 8000 or not syn[47] & 0x02:
        raise SystemExit("the first frame is not the SYN")

    def drain():
        b.settimeout(0.05)
        try:
            while True:
                b.recv(4096)
        except (socket.timeout, BlockingIOError):
            pass

    feed(lib, sk, frame(8000, stack_port, IRS, iss + 1, 0x12, b""))  # SYN-ACK
    drain()  # the ACK of the handshake
    rcv_nxt = IRS + 1
    frames = [frame(8000, stack_port, rcv_nxt + k * SEG, iss + 1, 0x10, payload_of(k)) for k in ORDER]
    for fr in frames:
        feed(lib, sk, fr)
        drain()  # duplicate ACKs for what arrived out of order
    buf = ctypes.create_string_buffer(16384)
    count = lib.tcp_data_dequeue(sk, buf, 16384)
    with open(out_path, "w") as f:
        json.dump({"seg": SEG, "order": list(ORDER), "rcv_nxt": rcv_nxt, "frames": [x.hex() for x in frames],
                   "count": count, "dequeued_hex": buf.raw[:max(count, 0)].hex()}, f, indent=1)


def main() -> None:
    if pyoracle.reflib() is None:
        raise SystemExit("oracle/_ref/libref.so missing: run `make -C oracle` where the reference is present")
    out = os.path.join(HERE, "lro_ref.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True, stdin=subprocess.DEVNULL)
    with open(out) as f:
        fx = json.load(f)
    want = b"".join(payload_of(k) for k in range(5))
    if fx["count"] != len(want) or bytes.fromhex(fx["dequeued_hex"]) != want:
        raise SystemExit(f"the reference returned {fx['count']} bytes; segments 0-4 are {len(want)}")
    print(out, os.path.getsize(out))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
