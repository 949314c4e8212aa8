"""flow_step.h (level-ip_amd/csrc) stands alone: a C main that includes nothing
else compiles as strict C99 without a warning and runs every shared per-flow
step once on boundary states under ASan + UBSan, as its own process.  What the
steps compute is pinned by the rto, wnd, cc, push and snd suites, on both
sides; this checks that the one definition is plain C and defined at the
edges of its arguments."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include "flow_step.h"

int main(void)
{
    uint32_t acc = 0, bytes;
    /* the timer: rto at its top, srtt and rttvar at both ends, a sample taken and the backoff doubled or the flow dead */
    const int32_t edge[2] = {INT32_MAX, INT32_MIN};
    for (int i = 0; i < 4; i++) {
        lvlip_rto_flow x = {0};
        x.srtt = edge[i & 1], x.rttvar = edge[(i & 1) ^ 1], x.rto = 0xFFFFFFFFu, x.expires = 5u, x.armed = 1;
        x.dupacks = 0xFFFFFFFFu, x.backoff = (uint8_t)(i >> 1 ? 255 : 0);
        flow_rto_out o = flow_rto_step(&x, 7u, 0xFFFFFFFFu, 1u, 0xFFFFFFFFu, 7u, LVLIP_RTO_FAST); /* r = 3: a sample */
        acc += o.fired + o.sample + x.rto;
        x.dead = 0, x.armed = 1, x.expires = 0u, x.rto = i & 1 ? 0xFFFFFFFFu : LVLIP_RTO_DEAD_MS;
        o = flow_rto_step(&x, 0xFFFFFFFFu, 0u, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu, LVLIP_RTO_FAST); /* fires */
        if (o.fired != LVLIP_RTO_TIMEOUT || x.dead != (i & 1)) return 1;
        o = flow_rto_step(&x, 1u, 1u, 0u, 3u, 0u, LVLIP_RTO_FAST); /* a dead flow stays as it is */
        acc += o.fired + x.rto + x.backoff;
    }
    /* the congestion window: cwnd at its ceiling, the largest mss, every count at 2^32 - 1 */
    for (uint32_t fired = 0; fired < 3u; fired++)
        for (uint32_t ss = 0; ss < 2u; ss++) {
            lvlip_cc_flow c = {0};
            c.cwnd = c.cwnd_max = LVLIP_CC_MAX_WND, c.mss = 65495u, c.acc = 0xFFFFFFFFu, c.recover = 0x80000000u;
            c.ssthresh = ss ? LVLIP_CC_MAX_WND : 0u;
            acc += flow_cc_step(&c, 0xFFFFFFFFu, 0x3FFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, fired, 1u);
            acc += flow_cc_step(&c, 1u, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u); /* a flight of 2^32 - 1 */
            if (c.cwnd > LVLIP_CC_MAX_WND || c.cwnd < c.mss) return 2;
        }
    if (flow_cc_cap(LVLIP_CC_MAX_WND, UINT64_MAX, &bytes) != LVLIP_CC_MAX_WND || bytes != LVLIP_CC_MAX_WND) return 3;
    /* the peer's window: the largest field at the largest scale, and a scale no check has seen */
    if (flow_wnd_scale(0xFFFFu, 14u) != 0xFFFFu << 14 || flow_wnd_scale(0xFFFFu, 255u) > FLOW_WND_MAX) return 4;
    if (flow_wnd_apply(FLOW_WND_MAX, 0u) != 0u || flow_wnd_apply(0u, FLOW_WND_MAX) != 0u) return 5;
    /* the push count: everything at 2^32 - 1 around the largest mss, and an mss of 0 */
    for (uint32_t mss = 0; mss < 2u; mss++) {
        lvlip_push_flow w = {0};
        lvlip_snd_flow s = {0};
        w.unsent = w.wnd = w.push = w.cap = 0xFFFFFFFFu, w.mss = (uint16_t)(mss ? 65495u : 0u);
        s.snd_una = 1u;
        const uint32_t m = flow_push_count(&w, &s, &bytes); /* span 2^32 - 1 == wnd: no room */
        s.snd_una = 0u;
        const uint32_t m2 = flow_push_count(&w, &s, &bytes);
        /* ceil((2^32 - 1) / 65495) segments, the last one short */
        if (m != 0u || m2 != (mss ? 65578u : 0u) || bytes != (mss ? 0xFFFFFFFFu : 0u)) return 6;
    }
    /* the ACK class at each border */
    if (flow_ack_class(0u, 0u) != FLOW_ACK_DUP || flow_ack_class(0xFFFFFFFFu, 0xFFFFFFFFu) != FLOW_ACK_NEW) return 7;
    if (flow_ack_class(0x7FFFFFFFu, 0u) != FLOW_ACK_BEYOND || flow_ack_class(0x80000000u, 0u) != FLOW_ACK_OLD) return 8;
    return acc == 0x12345u ? 9 : 0; /* acc keeps the calls from being folded away */
}
"""


def test_header_alone_is_c99_and_clean_at_the_edges(tmp_path):
    src, exe = tmp_path / "flow_step_main.c", tmp_path / "flow_step_main"
    src.write_text(MAIN)
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "level-ip_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_header_includes_only_the_public_header_and_stdint():
    text = open(os.path.join(ROOT, "level-ip_amd", "csrc", "flow_step.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert sorted(includes) == ['"lvlip_skb.h"', "<stdint.h>"]
