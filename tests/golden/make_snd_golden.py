#!/usr/bin/env python3
"""Generate tests/golden/snd_ref.json: what the REFERENCE's own stack does with
the ACK field of incoming segments (src/tcp_input.c:311-356 and
tcp_clean_rto_queue, :66-92) and the bytes it sends when its retransmission
timer fires (tcp_retransmission_timeout, src/tcp_output.c:359-381), for the
tests of the ACK side and the retransmit (include/lvlip_skb.h, lvlip_snd_* and
lvlip_rtx_*).

Runs only where oracle/_ref/libref.so exists (level-ip's own src/*.c, compiled
unmodified by oracle/Makefile).  A child process drives the stack the way
make_lro_golden.py does (socketpair for the tap device, ARP, tcp_v4_connect,
the peer's SYN-ACK through tcp_input_state; no MSS option, so smss stays 536,
src/tcp.c:115), then calls tcp_send with 2001 bytes: four skbs of 536, 536, 536
and 393 bytes on the write queue.

tcp_queue_transmit_skb transmits a segment only while nothing is in flight
(src/tcp_output.c:142), so the transfer has two stages, and every ACK case is
fed in both:

  stage A  the first segment is out (snd_nxt = snd_una + 536), the queue holds
           four skbs.  Pure ACKs: old, equal to snd_una, beyond snd_nxt, in
           mid-segment, then on the segment's boundary, which here is snd_nxt:
           it pops the head, and the stack sends the other three
           (src/tcp_input.c:482-485 -> tcp_send_next).
  stage B  three segments in flight.  Pure ACKs: old, equal to snd_una,
           beyond, on a boundary (pops one); then 100 bytes of in-order data
           arrive and move rcv_nxt, and the retransmission timer is fired by
           calling the handler the stack itself armed (tsk->retransmit), which
           sends the head of the queue again with the new ack_seq; then an ACK
           in mid-segment and one equal to snd_nxt, which empties the queue.

After every ACK the child reads snd_una, snd_nxt and the write queue's length
out of the socket (x86-64 offsets of include/sock.h and include/tcp.h, checked
against the SYN and the queue of four before anything is recorded).  The
fixture holds the four data frames as the stack sent them, the cases with the
state before and after each, and the re-sent frame with the state it was sent
from.  All six cases could be driven, in both stages; main() refuses to write
a fixture that lacks one, see check().

usage: python tests/golden/make_snd_golden.py   (from the repo root)
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
from make_lro_golden import IRS, STACK_IP, STACK_MAC, TAP_IP, TAP_MAC, feed, frame  # noqa: E402

assert STACK_IP and STACK_MAC
SENT = 2001
SEGS = (536, 536, 536, 393)
DATA = 100  # in-order bytes that move rcv_nxt before the retransmit
NAMES = ("old", "snd_una", "mid_segment", "boundary", "snd_nxt", "beyond")
# struct sock / struct tcp_sock / struct socket / struct timer on x86-64 (glibc: pthread_cond_t 48, pthread_mutex_t 40)
WRITE_QLEN, SND_UNA, SND_NXT, RCV_NXT, RCV_WND, RETRANSMIT = 152, 200, 204, 228, 232, 264
SOCKET_REFCNT, TIMER_HANDLER, TIMER_ARG = 24, 32, 40


def payload() -> bytes:
    return bytes((7 * i + 3) & 0xFF for i in range(SENT))


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
    lib.tcp_send.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
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

    u32 = lambda off: ctypes.c_uint32.from_address(sk + off).value  # noqa: E731
    state = lambda: dict(snd_una=u32(SND_UNA), snd_nxt=u32(SND_NXT), queue=u32(WRITE_QLEN))  # noqa: E731
    if state() != dict(snd_una=iss, snd_nxt=(iss + 1) & 0xFFFFFFFF, queue=1):
        raise SystemExit(f"the socket's layout is not the one assumed: {state()} after a SYN with seq {iss}")

    def drain():
        got = []
        b.settimeout(0.05)
        try:
            while True:
                got.append(b.recv(4096))
        except (socket.timeout, BlockingIOError):
            pass
        return got

    feed(lib, sk, frame(8000, stack_port, IRS, iss + 1, 0x12, b""))  # SYN-ACK
    drain()  # the ACK of the handshake
    rcv_nxt = (IRS + 1) & 0xFFFFFFFF
    if u32(RCV_NXT) != rcv_nxt or state()["queue"] != 0:
        raise SystemExit("the socket's layout is not the one assumed (rcv_nxt, or the SYN still queued)")
    if lib.tcp_send(sk, payload(), SENT) != SENT:
        raise SystemExit("tcp_send")
    queue = drain()
    if len(queue) != 1 or state()["queue"] != 4:
        raise SystemExit(f"tcp_send put {len(queue)} frames on the wire and {state()['queue']} skbs on the queue")
    una0 = (iss + 1) & 0xFFFFFFFF
    cases = []

    def ack(stage: str, name: str, ack_seq: int):
        """One pure ACK; returns the frames it caused."""
        before = state()
        feed(lib, sk, frame(8000, stack_port, u32(RCV_NXT), ack_seq & 0xFFFFFFFF, 0x10, b""))
        got = drain()
        cases.append(dict(stage=stage, name=name, ack_seq=ack_seq & 0xFFFFFFFF, before=before, after=state()))
        return got

    for name, a_seq in (("old", una0 - 1), ("snd_una", una0), ("beyond", una0 + 537), ("mid_segment", una0 + 300)):
        if ack("A", name, a_seq):
            raise SystemExit(f"stage A, {name}: the stack sent something")
    sent = ack("A", "boundary", una0 + 536)
    cases.append(dict(cases[-1], name="snd_nxt"))  # one segment in flight: its boundary is snd_nxt
    queue += sent
    if [len(f) - 54 for f in queue] != list(SEGS):
        raise SystemExit(f"the data frames carry {[len(f) - 54 for f in queue]} bytes")
    una1, nxt1 = una0 + 536, una0 + SENT
    for name, a_seq in (("old", una1 - 200), ("snd_una", una1), ("beyond", nxt1 + 1), ("boundary", una1 + 536)):
        if ack("B", name, a_seq):
            raise SystemExit(f"stage B, {name}: the stack sent something")

    # in-order data moves rcv_nxt; then the retransmission timer's own handler, called as the timer thread calls it
    feed(lib, sk, frame(8000, stack_port, rcv_nxt, (una1 + 536) & 0xFFFFFFFF, 0x10, bytes(range(DATA))))
    drain()
    if u32(RCV_NXT) != (rcv_nxt + DATA) & 0xFFFFFFFF:
        raise SystemExit("the data did not move rcv_nxt")
    timer = ctypes.c_void_p.from_address(sk + RETRANSMIT).value
    if not timer or ctypes.c_void_p.from_address(timer + TIMER_ARG).value != sk:
        raise SystemExit("no retransmission timer armed for this socket")
    ctypes.c_int.from_address(ctypes.addressof(sock) + SOCKET_REFCNT).value = 1  # socket_release frees at 0
    handler = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p)(ctypes.c_void_p.from_address(timer + TIMER_HANDLER).value)
    at = state()
    handler(sk)
    resent = drain()
    if len(resent) != 1:
        raise SystemExit(f"the timer sent {len(resent)} frames")
    resend = dict(frame=resent[0].hex(), index=4 - at["queue"], state=at, rcv_nxt=u32(RCV_NXT), rcv_wnd=u32(RCV_WND))

    if ack("B", "mid_segment", una1 + 536 + 100):
        raise SystemExit("stage B, mid_segment: the stack sent something")
    ack("B", "snd_nxt", nxt1)
    with open(out_path, "w") as f:
        json.dump({"sent": SENT, "segs": list(SEGS), "iss": iss, "rcv_nxt": rcv_nxt, "queue": [x.hex() for x in queue],
                   "cases": cases, "resend": resend}, f, indent=1)


def check(fx: dict) -> None:
    """Every one of the six cases in both stages, each being what its name
    says by the arithmetic of the state before it, and a re-sent head."""
    M = 0xFFFFFFFF
    for stage in "AB":
        have = {c["name"]: c for c in fx["cases"] if c["stage"] == stage}
        for name in NAMES:
            if name not in have:
                raise SystemExit(f"the fixture lacks the case {name} in stage {stage}")
            c = have[name]
            una, nxt = c["before"]["snd_una"], c["before"]["snd_nxt"]
            d, span = (c["ack_seq"] - una) & M, (nxt - una) & M
            ends = []
            for h in fx["queue"]:
                fr = bytes.fromhex(h)
                ends.append((struct.unpack_from("!I", fr, 38)[0] + len(fr) - 54 - una) & M)
            ok = {"old": d >= 1 << 31, "snd_una": d == 0, "beyond": span < d < 1 << 31,
                  "mid_segment": 0 < d < span and d not in ends, "boundary": 0 < d <= span and d in ends,
                  "snd_nxt": d == span}[name]
            if not ok:
                raise SystemExit(f"stage {stage}: the case {name} is not one (d {d}, span {span})")
    r = fx["resend"]
    sent = bytes.fromhex(r["frame"])
    first = bytes.fromhex(fx["queue"][r["index"]])
    if len(sent) != len(first) or sent[54:] != first[54:] or sent[38:42] != first[38:42]:
        raise SystemExit("the re-sent frame is not the head of the queue")
    if struct.unpack_from("!I", sent, 42)[0] != (fx["rcv_nxt"] + DATA) & M or sent[42:46] == first[42:46]:
        raise SystemExit("the re-sent frame does not carry the moved rcv_nxt")


def main() -> None:
    if pyoracle.reflib() is None:
        raise SystemExit("oracle/_ref/libref.so missing: run `make -C oracle` where the reference is present")
    out = os.path.join(HERE, "snd_ref.json")
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
