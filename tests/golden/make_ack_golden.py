#!/usr/bin/env python3
"""Generate tests/golden/ack_ref.json: the ACK frames the REFERENCE's own
receive path emits while data segments arrive out of order, SACK option
included, for the acknowledgement calls' tests (include/lvlip_skb.h,
lvlip_ack_*).

Runs only where oracle/_ref/libref.so exists (level-ip's own src/*.c, compiled
unmodified by oracle/Makefile).  A child process drives the stack the way
make_lro_golden.py does (socketpair for the tap device, ARP, tcp_v4_connect,
the peer's SYN-ACK through tcp_input_state), with one difference that matters:
the SYN-ACK carries the options MSS and SACK-permitted (02 04 05 b4 01 01 04
02, hl 7).  Without them tcp_parse_opts clears sackok
(src/tcp_input.c:51-57) and the stack never writes a SACK block.

The stack's handshake ACK is kept: its 54 bytes are the template.  Then 536-B
segments arrive in the order ORDER, and after EACH arrival every frame the
stack emitted is recorded.  An out-of-order arrival makes tcp_data_queue
compute the SACK list and send an immediate ACK (src/tcp_data.c:110-125 ->
tcp_calculate_sacks, src/tcp.c:454-485 -> tcp_send_ack,
src/tcp_output.c:247-267); an in-order one only arms the delayed-ACK timer
(src/tcp_input.c:486-490), so it emits nothing here.

The fixture holds the template frame, the rcv_nxt in front of the first
segment, the arrival frames in order and, per arrival, the hex of the ACK it
caused (null if none).  main() refuses to write a fixture that lacks the
cases the tests rest on: see check().

usage: python tests/golden/make_ack_golden.py   (from the repo root)
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
from make_lro_golden import IRS, SEG, STACK_IP, STACK_MAC, TAP_IP, TAP_MAC, _fold, payload_of  # noqa: E402

ORDER = (2, 4, 5, 0, 1, 7, 9, 11, 13, 9)
SYNACK_OPTS = bytes.fromhex("020405b401010402")  # MSS 1460, NOP, NOP, SACK permitted


def frame(sport: int, dport: int, seq: int, ack: int, flags: int, data: bytes, opts: bytes = b"") -> bytes:
    """Peer -> stack, as a correct peer sends it (RFC pseudo header)."""
    hl = 5 + len(opts) // 4
    tcp = bytearray(struct.pack("!HHIIBBHHH", sport, dport, seq, ack, hl << 4, flags, 0xFFFF, 0, 0) + opts + data)
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
    hl = raw[12] >> 4
    dlen = len(fr) - 34 - 4 * hl
    flags = raw[13]
    skb.contents.seq = seq
    skb.contents.dlen = dlen
    skb.contents.len = dlen + ((flags >> 1) & 1) + (flags & 1)
    skb.contents.end_seq = (seq + dlen) & 0xFFFFFFFF
    skb.contents.payload = th + 4 * hl
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
        got = []
        b.settimeout(0.05)
        try:
            while True:
                got.append(b.recv(4096))
        except (socket.timeout, BlockingIOError):
            pass
        return got

    feed(lib, sk, frame(8000, stack_port, IRS, iss + 1, 0x12, b"", SYNACK_OPTS))  # SYN-ACK
    hs = drain()  # the ACK of the handshake
    if len(hs) != 1 or len(hs[0]) != 54:
        raise SystemExit(f"the handshake gave {[len(x) for x in hs]} instead of one 54-byte ACK")
    rcv_nxt = IRS + 1
    frames = [frame(8000, stack_port, rcv_nxt + k * SEG, iss + 1, 0x10, payload_of(k)) for k in ORDER]
    acks = []
    for fr in frames:
        feed(lib, sk, fr)
        got = drain()
        if len(got) > 1:
            raise SystemExit(f"one arrival caused {len(got)} frames")
        acks.append(got[0].hex() if got else None)
    with open(out_path, "w") as f:
        json.dump({"seg": SEG, "order": list(ORDER), "rcv_nxt": rcv_nxt, "template": hs[0].hex(), "max_sack": 4,
                   "frames": [x.hex() for x in frames], "acks": acks}, f, indent=1)


def blocks_of(ack: bytes):
    """The SACK blocks of a frame as the option lists them: [(left, right)]."""
    opt = ack[54:]
    if not opt:
        return []
    if opt[:3] != b"\x01\x01\x05" or opt[3] != len(opt) - 2:
        raise SystemExit(f"not a SACK option: {opt.hex()}")
    return [struct.unpack_from("!II", opt, 4 + 8 * i) for i in range((len(opt) - 4) // 8)]


def check(fx: dict) -> None:
    """The cases the tests rest on, from the arrival order alone (a model of
    the ofo queue) and from what the stack sent."""
    have, nxt = set(), 0
    compared = []
    for j, (k, ack) in enumerate(zip(fx["order"], fx["acks"])):
        ooo = k != nxt
        have.add(k)
        while nxt in have:
            nxt += 1
        if ooo != (ack is not None):
            raise SystemExit(f"arrival {j} (segment {k}): out of order {ooo}, ACK {ack is not None}")
        if not ooo:
            continue
        ack = bytes.fromhex(ack)
        isl = []
        for s in sorted(x for x in have if x >= nxt):
            if isl and isl[-1][1] == s:
                isl[-1][1] = s + 1
            else:
                isl.append([s, s + 1])
        if any(fx["rcv_nxt"] + lo * SEG == 0 for lo, _ in isl):
            raise SystemExit("an island at sequence number 0")
        ack_seq = struct.unpack_from("!I", ack, 42)[0]
        compared.append(dict(blocks=blocks_of(ack), islands=isl, advanced=ack_seq != fx["rcv_nxt"],
                             merged=any(hi - lo > 1 for lo, hi in isl)))
    if len(compared) < 6:
        raise SystemExit(f"only {len(compared)} ACKs with SACK blocks")
    for what, ok in (("two blocks", any(len(c["blocks"]) == 2 for c in compared)),
                     ("two adjacent segments merged into one block",
                      any(c["merged"] and len(c["blocks"]) == len(c["islands"]) for c in compared)),
                     ("four blocks cut from five islands",
                      any(len(c["blocks"]) == 4 and len(c["islands"]) == 5 for c in compared)),
                     ("ack_seq beyond the first rcv_nxt", any(c["advanced"] and c["blocks"] for c in compared))):
        if not ok:
            raise SystemExit(f"the fixture lacks an ACK with {what}")


def main() -> None:
    if pyoracle.reflib() is None:
        raise SystemExit("oracle/_ref/libref.so missing: run `make -C oracle` where the reference is present")
    out = os.path.join(HERE, "ack_ref.json")
    tmp = out + ".tmp"
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], check=True, stdin=subprocess.DEVNULL)
    with open(tmp) as f:
        fx = json.load(f)
    try:
        check(fx)
    except SystemExit:
        os.unlink(tmp)
        raise
    os.replace(tmp, out)
    print(out, os.path.getsize(out))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
