/*
 * rto_cpu.c — the retransmission timer and the peer's window
 * (include/lvlip_skb.h, "f2 on the device: the timer and the peer's window"):
 * the state check and both calls on the calling thread.  The device forms
 * (rto_kernels.hip) leave the same bytes.
 *
 * lvlip_rto_cpu is tcp_rtt (src/tcp.c:424-452), tcp_retransmission_timeout
 * (src/tcp_output.c:359-401), tcp_rearm_rto_timer on the first skb of an empty
 * queue (:138-140) and tcp_stop_rto_timer on an emptied one
 * (src/tcp_input.c:86-89), once per flow and round; lvlip_wnd_cpu reads the
 * window field the reference leaves as a TODO (src/tcp_input.c:352-354).
 */
#include "flow_step.h"
#include "tcp_hdr.h"

int lvlip_rto_check(const lvlip_rto_flow *t, uint32_t nflows)
{
    if (nflows == 0) return LVLIP_OK;
    if (!t || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++) {
        if (t[k].wscale > LVLIP_WSCALE_MAX || t[k].armed > 1u || t[k].dead > 1u) return LVLIP_EINVAL;
        if (t[k].snd_wnd > FLOW_WND_MAX || t[k].wnd_cap > FLOW_WND_MAX) return LVLIP_EINVAL;
    }
    return LVLIP_OK;
}

/* ---------------------------------------------------------------- window -- */

/* The frame test of lvlip_sack_* (sack_blocks, sack_cpu.c) on the len bytes at
 * p; *raw gets the window field in host order.  Only bytes inside the frame
 * are read. */
static int wnd_frame(const uint8_t *p, uint32_t len, uint32_t *raw)
{
    if (len < 34u || (p[14] >> 4) != 4u || (p[14] & 0x0fu) < 5u) return 0;
    const uint32_t th = 14u + 4u * (p[14] & 0x0fu);
    if (len < th + 20u) return 0;
    const uint32_t hl = p[th + 12u] >> 4;
    if (hl < 5u || len < th + 4u * hl) return 0;
    *raw = ((uint32_t)p[th + 14u] << 8) | p[th + 15u];
    return 1;
}

int lvlip_wnd_cpu(const lvlip_lro_flow *f, const lvlip_snd_flow *s, lvlip_rto_flow *t, lvlip_push_flow *w,
                  uint32_t nflows, const lvlip_lro_rec *rec, const void *ack_base, const lvlip_frame_desc *ack_fd,
                  uint32_t n, uint32_t flags, lvlip_wnd_result *res)
{
    if (nflows == 0) return LVLIP_OK;
    if (!f || !s || !t || !res || (n && (!rec || !ack_base || !ack_fd))) return LVLIP_EINVAL;
    if (n > LVLIP_MAX_BATCH || nflows > LVLIP_LRO_MAX_FLOWS || (flags & ~LVLIP_WND_APPLY)) return LVLIP_EINVAL;
    if (lvlip_rto_check(t, nflows) != LVLIP_OK) return LVLIP_EINVAL;
    memset(res, 0, (size_t)nflows * sizeof *res);
    /* res[k].raw holds the winner's d + 1 until the flows are finished */
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t k = rec_ack_flow(&rec[i], f, nflows);
        if (k == FLOW_NONE) continue;
        const uint32_t d = rec[i].ack_seq - s[k].snd_una;
        uint32_t raw;
        if (flow_ack_class(d, s[k].snd_nxt - s[k].snd_una) > FLOW_ACK_DUP) continue; /* old or beyond */
        if (!wnd_frame((const uint8_t *)ack_base + ack_fd[i].offset, ack_fd[i].len, &raw)) continue;
        res[k].n_counting++;
        if (d + 1u >= res[k].raw) { /* i ascends: the later record among equals */
            res[k].raw = d + 1u;
            res[k].winner = i;
            res[k].snd_wnd = raw;
        }
    }
    for (uint32_t k = 0; k < nflows; k++) {
        if (res[k].raw) {
            res[k].raw = res[k].snd_wnd;
            t[k].snd_wnd = flow_wnd_scale(res[k].raw, t[k].wscale);
        } else {
            res[k].winner = FLOW_NONE;
        }
        res[k].snd_wnd = t[k].snd_wnd;
        if ((flags & LVLIP_WND_APPLY) && w) w[k].wnd = flow_wnd_apply(t[k].snd_wnd, t[k].wnd_cap);
    }
    return LVLIP_OK;
}

/* ----------------------------------------------------------------- timer -- */

int lvlip_rto_cpu(const lvlip_snd_flow *s, const lvlip_snd_result *snd, const lvlip_push_result *push,
                  lvlip_rto_flow *t, uint32_t nflows, uint32_t now, uint32_t flags, uint8_t *sacked,
                  lvlip_snd_result *gate, lvlip_rto_result *res)
{
    if (nflows == 0) return LVLIP_OK;
    if (!s || !t || !gate || !res) return LVLIP_EINVAL;
    if (nflows > LVLIP_LRO_MAX_FLOWS || (flags & ~LVLIP_RTO_FAST)) return LVLIP_EINVAL;
    if (lvlip_rto_check(t, nflows) != LVLIP_OK) return LVLIP_EINVAL;
    memset(gate, 0, (size_t)nflows * sizeof *gate);
    for (uint32_t k = 0; k < nflows; k++) {
        const uint32_t nseg = s[k].nseg;
        const flow_rto_out o = flow_rto_step(&t[k], nseg, push ? push[k].pushed : 0u, snd ? snd[k].n_new : 0u,
                                             snd ? snd[k].n_dup : 0u, now, flags);
        res[k].fired = o.fired, res[k].sample = o.sample, res[k].rto = t[k].rto, res[k].backoff = t[k].backoff;
        gate[k].popped = o.fired ? 0u : nseg;
        if (o.fired == LVLIP_RTO_TIMEOUT && sacked && nseg) memset(sacked + s[k].seg0, 0, nseg);
    }
    return LVLIP_OK;
}
