#!/usr/bin/env python3
"""Generate tests/golden/fin_ref.json: what the REFERENCE's own stack sends and
which states it passes through while a connection ends, for the tests of
lvlip_fin_* (include/lvlip_skb.h, "the end of a connection"):

  tcp_close -> tcp_queue_fin   src/tcp.c:255-285, src/tcp_output.c:506-523
  tcp_input_state              the fifth check's "our FIN was acked"
                               (src/tcp_input.c:359-389) and the eighth check
                               (:417-467), through the frames of a peer
  tcp_enter_time_wait          src/tcp.c:402-411

Runs only where oracle/_ref/libref.so exists.  A child process drives the stack
the way make_rto_golden.py does (its Stack: socketpair for the tap device, ARP,
tcp_v4_connect, the peer's SYN-ACK); the handshake's ACK is kept as the header
template.

Four episodes, each a fresh socket:

  active        close; the peer acknowledges our FIN; the peer's FIN
  passive       the peer's FIN; close; the peer acknowledges our FIN
  simultaneous  close; the peer's FIN, which does not acknowledge ours; the
                peer's ACK of our FIN
  fin_ack       close; the peer's FIN, which acknowledges ours

Every step records the frame fed (if any), every frame the stack emitted, and
sk->state, rcv_nxt and snd_nxt AFTER the step.  Only recorded bytes and numbers
are written.

usage: python tests/golden/make_fin_golden.py   (from the repo root)
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
from make_lro_golden import IRS, STACK_IP, TAP_IP, TAP_MAC, feed, frame  # noqa: E402
from make_rto_golden import RCV_NXT, SND_NXT, SND_UNA, Stack  # noqa: E402

SK_STATE = 164  # struct sock on x86-64: int state behind write_queue (qlen at 152) and int protocol
ESTABLISHED, FIN_WAIT_1, FIN_WAIT_2, CLOSE, CLOSE_WAIT, CLOSING, LAST_ACK, TIME_WAIT = 3, 4, 5, 6, 7, 8, 9, 10
FIN, ACK = 0x01, 0x10


class Closer(Stack):
    """One established socket whose frames are kept."""

    def __init__(self, lib, b):
        self.hs = None
        super().__init__(lib, b)
        if self.sk_state() != ESTABLISHED:
            raise SystemExit(f"sk->state is not where it is assumed: {self.sk_state()}")

    def drain(self):
        got = []
        self.b.settimeout(0.05)
        try:
            while True:
                got.append(self.b.recv(4096))
        except (socket.timeout, BlockingIOError):
            pass
        if self.hs is None:
            self.hs = got  # the handshake's ACK
        return got

    def sk_state(self):
        return ctypes.c_int.from_address(self.sk + SK_STATE).value

    def after(self, op, fed, got):
        return dict(op=op, fed=fed.hex() if fed else None, emitted=[x.hex() for x in got], state=self.sk_state(),
                    rcv_nxt=self.u32(RCV_NXT), snd_nxt=self.u32(SND_NXT), snd_una=self.u32(SND_UNA))

    def start(self):
        if len(self.hs) != 1 or len(self.hs[0]) != 54:
            raise SystemExit(f"the handshake gave {[len(x) for x in self.hs]} instead of one 54-byte ACK")
        return self.after("established", None, [])

    def close(self):
        rc = self.lib.tcp_close(self.sk)
        if rc != 0:
            raise SystemExit(f"tcp_close returned {rc}")
        return self.after("close", None, self.drain())

    def peer(self, op, flags, ack=None, seq=None):
        fr = frame(8000, self.port, self.u32(RCV_NXT) if seq is None else seq,
                   self.u32(SND_NXT) if ack is None else ack, flags, b"")
        feed(self.lib, self.sk, fr)
        return self.after(op, fr, self.drain())


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
    lib.tcp_close.argtypes = [ctypes.c_void_p]

    episodes = []
    st = Closer(lib, b)
    episodes.append(dict(name="active", template=st.hs[0].hex(),
                         steps=[st.start(), st.close(), st.peer("peer_ack", ACK), st.peer("peer_fin", FIN | ACK)]))
    st = Closer(lib, b)
    episodes.append(dict(name="passive", template=st.hs[0].hex(),
                         steps=[st.start(), st.peer("peer_fin", FIN | ACK), st.close(), st.peer("peer_ack", ACK)]))
    st = Closer(lib, b)
    steps = [st.start(), st.close()]
    steps.append(st.peer("peer_fin", FIN | ACK, ack=st.u32(SND_UNA)))
    steps.append(st.peer("peer_ack", ACK))
    episodes.append(dict(name="simultaneous", template=st.hs[0].hex(), steps=steps))
    st = Closer(lib, b)
    episodes.append(dict(name="fin_ack", template=st.hs[0].hex(),
                         steps=[st.start(), st.close(), st.peer("peer_fin", FIN | ACK)]))
    with open(out_path, "w") as f:
        json.dump({"irs": IRS, "episodes": episodes}, f, indent=1)


def check(fx: dict) -> None:
    """The frames and states the tests rest on are there."""
    by = {e["name"]: e["steps"] for e in fx["episodes"]}
    if set(by) != {"active", "passive", "simultaneous", "fin_ack"}:
        raise SystemExit(f"episodes {sorted(by)}")
    for name, steps in by.items():
        fins = [bytes.fromhex(x) for s in steps if s["op"] == "close" for x in s["emitted"]]
        acks = [bytes.fromhex(x) for s in steps if s["op"] == "peer_fin" for x in s["emitted"]]
        if len(fins) != 1 or len(fins[0]) != 54 or not fins[0][47] & FIN:
            raise SystemExit(f"{name}: close emitted {[x.hex() for x in fins]}")
        if len(acks) != 1 or len(acks[0]) != 54 or acks[0][47] & FIN:
            raise SystemExit(f"{name}: the peer's FIN was answered by {[x.hex() for x in acks]}")
    states = {name: [s["state"] for s in steps] for name, steps in by.items()}
    if states["active"] != [ESTABLISHED, FIN_WAIT_1, FIN_WAIT_2, TIME_WAIT]:
        raise SystemExit(f"active: {states['active']}")
    if states["simultaneous"] != [ESTABLISHED, FIN_WAIT_1, CLOSING, TIME_WAIT]:
        raise SystemExit(f"simultaneous: {states['simultaneous']}")
    if states["fin_ack"] != [ESTABLISHED, FIN_WAIT_1, TIME_WAIT]:
        raise SystemExit(f"fin_ack: {states['fin_ack']}")
    if states["passive"][:2] != [ESTABLISHED, CLOSE_WAIT]:
        raise SystemExit(f"passive: {states['passive']}")


def main() -> None:
    if pyoracle.reflib() is None:
        raise SystemExit("oracle/_ref/libref.so missing: run `make -C oracle` where the reference is present")
    out = os.path.join(HERE, "fin_ref.json")
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
