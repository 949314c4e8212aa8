"""tests/sanitize/fin_hostile.c: the close state's check and CPU form on crafted
states and records, and flow_fin_step on boundary values, as a stand-alone
program of its own process under ASan + UBSan; and flow_fin_step's boundary
cases through the library.  Nothing here is loaded into Python under a
sanitizer and nothing runs on a GPU."""
import os
import subprocess

import numpy as np

import lvlip
from fin_model import ACKED, CLOSED, CLOSING, FW1, LAST_ACK, M32, RESENT, TW, TW_DONE, make_sides

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_SRCS = ("fin_cpu.c", "csum_cpu.c")


def test_hostile_state_and_records_under_sanitizers(tmp_path):
    """Records of no flow and of no status, rel + dlen that wraps, garbage
    templates, 65 536 flows with the frame buffer malloc'd to its last frame
    byte, garbage close state: refused with nothing written, or values change
    and no address does."""
    exe = tmp_path / "fin_hostile_san"
    csrc = os.path.join(ROOT, "level-ip_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "sanitize", "fin_hostile.c")] + [os.path.join(csrc, f) for f in C_SRCS]
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", csrc, *src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    assert "fin_hostile ok" in r.stdout


def step(state, expires, interval, now, una_back=1, retries=0, nseg=0):
    """One flow whose FIN is out, through lvlip_fin_cpu: (x', events)."""
    f, s, w, _ = make_sides(1)
    s["snd_una"] = s["snd_nxt"] - np.uint32(una_back)
    s["nseg"] = nseg
    x = lvlip.fin_flows(f)
    x["state"], x["expires"], x["interval"], x["retries"] = state, expires, interval, retries
    x["fin_seq"] = s["snd_nxt"] - np.uint32(1)
    _, _, _, res = lvlip.fin_cpu(f, np.zeros(1, dtype=lvlip.LRO_RESULT_DTYPE), None, s, w, lvlip.rto_flows(1), x, None, now)
    return x, int(res["events"][0])


def test_flow_fin_step_at_its_boundaries():
    """The timer's test is strict and unsigned, the doubling is formed in 64
    bits and stops at 60000, retries saturates, an interval of 0 stays 0, and
    the acknowledgement test is an equality mod 2^32."""
    for expires, now, fires in ((9, 10, 1), (10, 10, 0), (11, 10, 0), (M32, 0, 0), (0, M32, 1), (M32 - 1, M32, 1)):
        for state in (FW1, CLOSING, LAST_ACK):
            x, ev = step(state, expires, 1000, now)
            assert ev == (RESENT if fires else 0) and int(x["state"][0]) == state
            assert int(x["expires"][0]) == ((now + 2000) & M32 if fires else expires)
        x, ev = step(TW, expires, 60000, now, una_back=0)
        assert (ev, int(x["state"][0])) == ((TW_DONE, CLOSED) if fires else (0, TW))
    for iv, twice in ((0, 0), (1, 2), (29999, 59998), (30000, 60000), (30001, 60000), (60000, 60000)):
        assert int(step(FW1, 0, iv, 5)[0]["interval"][0]) == twice
    for r, nxt in ((0, 1), (M32 - 1, M32), (M32, M32)):
        assert int(step(LAST_ACK, 0, 10, 5, retries=r)[0]["retries"][0]) == nxt
    for back, acked in ((0, 1), (1, 0), (2, 0), (M32, 0)):
        assert bool(step(FW1, 100, 10, 5, una_back=back)[1] & ACKED) == bool(acked)
    x, ev = step(FW1, 0, 700, 5, nseg=3)
    assert ev == 0 and int(x["expires"][0]) == 705 and int(x["interval"][0]) == 700, "held while data is in flight"


# -------------------------------------------------------------- the example --

EXAMPLE_SRCS = ("fin_cpu.c", "rto_cpu.c", "push_cpu.c", "sack_cpu.c", "snd_cpu.c", "ack_cpu.c", "rcv_cpu.c", "seg_cpu.c",
                "csum_cpu.c")


def test_example_runs_to_its_own_check():
    exe = os.path.join(ROOT, "examples", "build", "fin_loop")
    subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fin_loop ok" in r.stdout, r.stdout + r.stderr


def test_example_under_sanitizers(tmp_path):
    """examples/fin_loop.c with the library's C sources as strict C99 under
    ASan + UBSan: every buffer is malloc'd at exactly its planned size."""
    exe = tmp_path / "fin_loop_san"
    csrc = os.path.join(ROOT, "level-ip_amd", "csrc")
    src = [os.path.join(ROOT, "examples", "fin_loop.c")] + [os.path.join(csrc, f) for f in EXAMPLE_SRCS]
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", csrc, *src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and "fin_loop ok" in r.stdout
