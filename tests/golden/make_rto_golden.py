#!/usr/bin/env python3
"""Generate tests/golden/rto_ref.json: what the REFERENCE's own stack does to
srtt, rttvar, rto, backoff and its retransmission timer, for the tests of
lvlip_rto_* (include/lvlip_skb.h, "the timer and the peer's window"):

  tcp_rtt                      src/tcp.c:424-452, called directly
  tcp_retransmission_timeout   src/tcp_output.c:359-401, by calling the handler
                               the stack itself armed, as make_snd_golden.py does
  tcp_rearm_rto_timer          on the first skb of an empty queue (tcp_send on an
                               established socket, src/tcp_output.c:138-140)
  tcp_stop_rto_timer           on an emptied queue: an ACK of everything through
                               tcp_input_state (src/tcp_input.c:330-336, :86-89)

Runs only where oracle/_ref/libref.so exists.  A child process drives the stack
the way make_snd_golden.py does (socketpair for the tap device, ARP,
tcp_v4_connect, the peer's SYN-ACK).

The clock.  The reference's tick (src/timer.c:6) is a file-static that stays 0
without its timer thread, so timer_get_tick() returns 0 throughout.  tcp_rtt
computes r = tick - (expires - rto); a clock value is therefore stood for by
writing the armed timer's `expires` field: expires = rto - r makes the sample r
(`now` is subtracted).  The field's offset is checked against the timer the
first tcp_send arms (expires == 0 + rto).

Three sessions, each a fresh socket:

  backoff   arm, then timeouts from rto 1000 until one finds rto > 60000 and
            ends the connection; a sample with backoff > 0 in between
  samples   a sample with no timer, arm, a first sample (after one of r = 0,
            which leaves srtt 0 and so is "first" again, src/tcp.c:434), 20 and
            more later samples (r = 0, 1, large, negative, below / equal to /
            above srtt), one timeout, a sample with backoff > 0, the ACK that
            empties the queue (stop), arm again, and an emptying ACK that is
            sampled first
  large     arm, a first sample, one of 2 000 000 ms, one more

Every step records srtt, rttvar, rto, backoff and armed (tsk->retransmit !=
NULL) AFTER the step.  Only recorded numbers are written.

usage: python tests/golden/make_rto_golden.py   (from the repo root)
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

M = 0xFFFFFFFF
# struct sock / struct tcp_sock / struct socket / struct timer on x86-64, as in make_snd_golden.py
WRITE_QLEN, SND_UNA, SND_NXT, RCV_NXT = 152, 200, 204, 228
BACKOFF, SRTT, RTTVAR, RTO, RETRANSMIT = 245, 248, 252, 256, 264
SOCKET_REFCNT, TIMER_EXPIRES, TIMER_HANDLER, TIMER_ARG = 24, 20, 32, 40
# later samples of the "samples" session: ("abs", r) or ("rel", r - srtt)
LATER = [("abs", 0), ("abs", 1), ("abs", 50000), ("rel", -1), ("rel", 0), ("rel", 1), ("abs", -5), ("abs", 7),
         ("abs", 13), ("abs", 200), ("abs", 199), ("abs", 201), ("abs", 1000), ("abs", 3), ("abs", 3), ("abs", 3),
         ("abs", 3), ("abs", 60), ("abs", 61), ("abs", 59), ("abs", 2), ("abs", 10), ("abs", 10), ("abs", 10)]


class Stack:
    """One established socket of the reference stack."""

    def __init__(self, lib, b):
        self.lib, self.b = lib, b
        tcp_ops = ctypes.addressof(ctypes.c_char.in_dll(lib, "tcp_ops"))
        self.sk = sk = lib.sk_alloc(tcp_ops, 6)
        self.sock = ctypes.create_string_buffer(1024)  # struct socket, zeroed
        lib.sock_init_data(ctypes.addressof(self.sock), sk)
        addr = struct.pack("=H", socket.AF_INET) + struct.pack("!H", 8000) + TAP_IP + bytes(8)
        self.addr = ctypes.create_string_buffer(addr, len(addr))
        lib.tcp_v4_connect(sk, ctypes.addressof(self.addr), 16, 0)
        syn = b.recv(4096)
        self.port, peer_port, iss = struct.unpack("!HHI", syn[34:42])
        if peer_port != 8000 or not syn[47] & 0x02:
            raise SystemExit("the first frame is not the SYN")
        feed(lib, sk, frame(8000, self.port, IRS, iss + 1, 0x12, b""))  # SYN-ACK
        self.drain()
        if self.u32(RCV_NXT) != (IRS + 1) & M or self.u32(WRITE_QLEN) != 0 or self.u32(SND_UNA) != (iss + 1) & M:
            raise SystemExit("the socket's layout is not the one assumed")
        if self.state() != dict(srtt=0, rttvar=0, rto=1000, backoff=0, armed=0):
            raise SystemExit(f"an established socket starts as {self.state()}")  # src/tcp_input.c:194-196

    def u32(self, off):
        return ctypes.c_uint32.from_address(self.sk + off).value

    def i32(self, off):
        return ctypes.c_int32.from_address(self.sk + off).value

    def timer(self):
        return ctypes.c_void_p.from_address(self.sk + RETRANSMIT).value

    def state(self):
        return dict(srtt=self.i32(SRTT), rttvar=self.i32(RTTVAR), rto=self.u32(RTO),
                    backoff=ctypes.c_uint8.from_address(self.sk + BACKOFF).value, armed=int(bool(self.timer())))

    def drain(self):
        self.b.settimeout(0.05)
        try:
            while True:
                self.b.recv(4096)
        except (socket.timeout, BlockingIOError):
            pass

    def set_sample(self, r):
        """The clock value at which tcp_rtt measures r: expires = rto - r."""
        t = self.timer()
        if t:
            ctypes.c_uint32.from_address(t + TIMER_EXPIRES).value = (self.u32(RTO) - r) & M

    def push(self):
        """tcp_send on an empty queue: one skb, the timer armed at 0 + rto."""
        if self.u32(WRITE_QLEN) != 0:
            raise SystemExit("push: the queue is not empty")
        if self.lib.tcp_send(self.sk, bytes(100), 100) != 100:
            raise SystemExit("tcp_send")
        self.drain()
        t = self.timer()
        if not t or ctypes.c_void_p.from_address(t + TIMER_ARG).value != self.sk:
            raise SystemExit("no retransmission timer armed for this socket")
        expires = ctypes.c_uint32.from_address(t + TIMER_EXPIRES).value
        if expires != self.u32(RTO) or self.u32(WRITE_QLEN) != 1:
            raise SystemExit(f"the timer's layout is not the one assumed (expires {expires}, rto {self.u32(RTO)})")
        return dict(op="push", expires_minus_now=expires, after=self.state())

    def rtt(self, r, op="rtt"):
        self.set_sample(r)
        self.lib.tcp_rtt(self.sk)
        return dict(op=op, r=r, after=self.state())

    def timeout(self):
        t = self.timer()
        ctypes.c_int.from_address(ctypes.addressof(self.sock) + SOCKET_REFCNT).value = 1000  # socket_release frees at 0
        handler = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p)(ctypes.c_void_p.from_address(t + TIMER_HANDLER).value)
        before = self.u32(RTO)
        handler(self.sk)
        self.drain()
        return dict(op="timeout", dead=int(before > 60000), queue=self.u32(WRITE_QLEN), after=self.state())

    def ack_all(self, r):
        """An ACK of snd_nxt through tcp_input_state at the clock value that makes the sample r."""
        self.set_sample(r)
        feed(self.lib, self.sk, frame(8000, self.port, self.u32(RCV_NXT), self.u32(SND_NXT), 0x10, b""))
        self.drain()
        if self.u32(WRITE_QLEN) != 0:
            raise SystemExit("the ACK did not empty the queue")
        return dict(op="ack_all", r=r, after=self.state())


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
    lib.tcp_rtt.argtypes = [ctypes.c_void_p]
    lib.tcp_rtt.restype = None

    # ---- backoff: 1000 -> 64000, then the timeout that finds rto > 60000
    st = Stack(lib, b)
    steps = [st.push()]
    while True:
        steps.append(st.timeout())
        if steps[-1]["dead"]:
            break
        if len(steps) == 3:
            steps.append(st.rtt(100, op="rtt_backoff"))
        if len(steps) > 20:
            raise SystemExit("rto never passed 60000")
    sessions = [dict(name="backoff", steps=steps)]

    # ---- samples
    st = Stack(lib, b)
    st.lib.tcp_rtt(st.sk)
    steps = [dict(op="rtt_unarmed", r=0, after=st.state()), st.push(), st.rtt(0), st.rtt(120)]
    for kind, v in LATER:
        steps.append(st.rtt(v if kind == "abs" else st.i32(SRTT) + v))
        steps[-1]["kind"] = kind
    steps.append(st.timeout())
    steps.append(st.rtt(100, op="rtt_backoff"))
    steps.append(st.ack_all(100))  # backoff > 0: no sample, then the stop
    steps.append(st.push())
    steps.append(st.rtt(40))
    steps.append(st.ack_all(80))   # sampled, then the stop
    sessions.append(dict(name="samples", steps=steps))
    if any(s["op"] == "timeout" and s["dead"] for s in steps):
        raise SystemExit("samples: the session's one timeout ended the connection")

    # ---- large: a sample of more than half an hour
    st = Stack(lib, b)
    sessions.append(dict(name="large", steps=[st.push(), st.rtt(120), st.rtt(2000000), st.rtt(120)]))
    with open(out_path, "w") as f:
        json.dump({"sessions": sessions}, f, indent=1)


def check(fx: dict) -> None:
    """The sequences the tests rely on are all there."""
    by = {s["name"]: s["steps"] for s in fx["sessions"]}
    bo = by["backoff"]
    rtos = [s["after"]["rto"] for s in bo if s["op"] == "timeout"]
    if bo[0]["op"] != "push" or bo[0]["after"]["rto"] != 1000 or bo[0]["after"]["armed"] != 1:
        raise SystemExit("backoff: no arm at rto 1000")
    if rtos[0] != 2000 or max(rtos) <= 60000 or not bo[-1]["dead"] or bo[-1]["after"]["armed"]:
        raise SystemExit(f"backoff: the timeouts left rto {rtos}")
    if not any(s["op"] == "rtt_backoff" and s["after"]["backoff"] > 0 for s in bo):
        raise SystemExit("backoff: no sample with backoff > 0")
    sm = by["samples"]
    if sm[0]["op"] != "rtt_unarmed" or sm[0]["after"] != dict(srtt=0, rttvar=0, rto=1000, backoff=0, armed=0):
        raise SystemExit("samples: the sample with no timer changed something")
    rtt = [s for s in sm if s["op"] == "rtt"]
    if rtt[1]["after"]["srtt"] != 120 or rtt[1]["after"]["rttvar"] != 60:
        raise SystemExit("samples: no first sample")
    later = rtt[2:]
    rs = [s["r"] for s in later]
    if len(later) < 20 or 0 not in rs or 1 not in rs or max(rs) < 50000 or min(rs) >= 0:
        raise SystemExit("samples: a later sample is missing")
    if not {"abs", "rel"} <= {s.get("kind") for s in later}:
        raise SystemExit("samples: no sample relative to srtt")
    stops = [s for s in sm if s["op"] == "ack_all"]
    if len(stops) != 2 or any(s["after"]["armed"] or s["after"]["backoff"] for s in stops):
        raise SystemExit("samples: the emptying ACK did not stop the timer")
    if max(s.get("r", 0) for s in by["large"]) < 1000000:
        raise SystemExit("large: no large sample")


def main() -> None:
    if pyoracle.reflib() is None:
        raise SystemExit("oracle/_ref/libref.so missing: run `make -C oracle` where the reference is present")
    out = os.path.join(HERE, "rto_ref.json")
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
