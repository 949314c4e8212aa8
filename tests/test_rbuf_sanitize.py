"""tests/sanitize/rbuf_hostile.c: the receive buffer's plan, check and CPU form
on crafted states and results, as a stand-alone program of its own process
under ASan + UBSan.  Nothing here is loaded into Python and nothing runs on a
GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_SRCS = ("rbuf_cpu.c",)


def test_hostile_state_and_results_under_sanitizers(tmp_path):
    """nsack 7, wild edges, head beyond used, cap 2^30 over an allocation of
    400 bytes: refused with nothing written, or values change and no address
    does."""
    exe = tmp_path / "rbuf_hostile_san"
    csrc = os.path.join(ROOT, "level-ip_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "sanitize", "rbuf_hostile.c")] + [os.path.join(csrc, f) for f in C_SRCS]
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", csrc, *src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    assert "rbuf_hostile ok" in r.stdout
