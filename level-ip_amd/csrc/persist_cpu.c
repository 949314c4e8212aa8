/*
 * persist_cpu.c — the zero-window persist timer and its probe
 * (include/lvlip_skb.h, "f2 on the device: the persist timer"): the state
 * check and the call on the calling thread.  The device form
 * (persist_kernels.hip) leaves the same bytes.
 *
 * The reference has no persist timer (RFC 1122 4.2.2.17).  The timer's steps
 * are flow_step.h's; the probe is a segment of no bytes that is not the last,
 * through tcp_seg_write, the frame writer lvlip_tso_cpu and lvlip_push_cpu
 * use, on the template as lvlip_push_cpu patches it.
 */
#include "flow_step.h"
#include "tcp_hdr.h"

int lvlip_persist_check(const lvlip_persist_flow *p, uint32_t nflows)
{
    if (nflows == 0) return LVLIP_OK;
    if (!p || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++) {
        if (p[k].armed > 1u || p[k].reserved[0] || p[k].reserved[1] || p[k].reserved[2]) return LVLIP_EINVAL;
        if (p[k].interval > LVLIP_PERSIST_MAX_MS || (p[k].armed && p[k].interval == 0)) return LVLIP_EINVAL;
    }
    return LVLIP_OK;
}

int lvlip_persist_cpu(const lvlip_lro_flow *f, const lvlip_lro_result *lro, const lvlip_snd_flow *s,
                      const lvlip_push_flow *w, lvlip_rto_flow *t, lvlip_persist_flow *p, uint32_t nflows,
                      uint32_t now, void *out, lvlip_frame_desc *fd_out, lvlip_persist_result *res)
{
    if (nflows == 0) return LVLIP_OK;
    if (!f || !s || !w || !t || !p || !out || !fd_out || !res) return LVLIP_EINVAL;
    if (nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    if (lvlip_persist_check(p, nflows) != LVLIP_OK) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++) {
        const flow_persist_out o = flow_persist_step(&p[k], t[k].dead, s[k].nseg, w[k].unsent, w[k].wnd, w[k].mss,
                                                     t[k].rto, now);
        const uint32_t seq = s[k].snd_una - 1u;
        if (o.clear) t[k].dupacks = 0;
        res[k].fired = o.fired, res[k].interval = o.interval, res[k].probes = o.probes;
        res[k].seq = o.fired ? seq : 0u;
        fd_out[k].offset = (uint64_t)LVLIP_PERSIST_SLOT * k;
        fd_out[k].len = o.fired ? TCP_FRAME_HDR : 0u;
        fd_out[k].reserved = 0;
        if (!o.fired) continue;
        /* the template as tcp_transmit_skb would fill it now (src/tcp_output.c:107-109) */
        uint8_t hdr[TCP_FRAME_HDR];
        memcpy(hdr, w[k].hdr, sizeof hdr);
        put_be32(hdr + 42, f[k].rcv_nxt + (lro ? lro[k].delivered : 0u));
        hdr[48] = (uint8_t)(s[k].win >> 8);
        hdr[49] = (uint8_t)s[k].win;
        tcp_seg_write((uint8_t *)out + fd_out[k].offset, hdr, hdr, 0u, seq, 0);
    }
    return LVLIP_OK;
}
