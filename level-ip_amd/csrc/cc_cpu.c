/*
 * cc_cpu.c — the congestion window (include/lvlip_skb.h, "f2 on the device:
 * the congestion window"): the state check and the call on the calling
 * thread.  The device form (cc_kernels.hip) leaves the same bytes.
 *
 * The reference has no congestion control (its cwnd, include/tcp.h:211, is
 * never touched); the steps are RFC 5681 (slow start, avoidance, the cut on a
 * timeout), RFC 3465 (byte counting), RFC 6582 (recover) and RFC 6675 (pipe).
 */
#include "flow_step.h"
#include "tcp_hdr.h" /* TCP_FRAME_HDR, the header of every frame lvlip_tso_* / lvlip_push_* build; TCP_MSS_MAX */

int lvlip_cc_check(const lvlip_cc_flow *c, uint32_t nflows)
{
    if (nflows == 0) return LVLIP_OK;
    if (!c || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++) {
        const uint32_t mss = c[k].mss;
        if (mss == 0 || mss > TCP_MSS_MAX) return LVLIP_EINVAL;
        if (c[k].cwnd < mss || c[k].cwnd > LVLIP_CC_MAX_WND) return LVLIP_EINVAL;
        if (c[k].cwnd_max < mss || c[k].cwnd_max > LVLIP_CC_MAX_WND) return LVLIP_EINVAL;
        if (c[k].ssthresh > LVLIP_CC_MAX_WND || c[k].in_rec > 1u) return LVLIP_EINVAL;
        if (c[k].reserved || c[k].reserved2[0] || c[k].reserved2[1]) return LVLIP_EINVAL;
    }
    return LVLIP_OK;
}

int lvlip_cc_cpu(const lvlip_snd_flow *s, const lvlip_snd_result *snd, const lvlip_rto_result *prev,
                 lvlip_cc_flow *c, lvlip_rto_flow *t, uint32_t nflows, const lvlip_frame_desc *fd,
                 const uint8_t *sacked, lvlip_cc_result *res)
{
    if (nflows == 0) return LVLIP_OK;
    if (!s || !c || !t || !res || (sacked && !fd)) return LVLIP_EINVAL;
    if (lvlip_cc_check(c, nflows) != LVLIP_OK) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++) {
        lvlip_cc_flow *x = &c[k];
        if (t[k].dead) {
            res[k].cwnd = x->cwnd, res[k].sacked_bytes = 0, res[k].n_sacked = 0, res[k].event = 0;
            continue;
        }
        /* 1: loss, 2: ACKs */
        const uint32_t event = flow_cc_step(x, s[k].snd_una, s[k].snd_nxt, snd ? snd[k].acked : 0u,
                                            snd ? snd[k].n_new : 0u, prev ? prev[k].fired : 0u,
                                            prev ? prev[k].backoff : 0u);
        /* 3: pipe */
        uint64_t sum = 0;
        uint32_t n_sacked = 0, bytes;
        if (sacked) {
            const uint32_t nseg = s[k].nseg;
            const uint32_t p = snd && snd[k].popped < nseg ? snd[k].popped : snd ? nseg : 0u;
            const uint64_t q1 = (uint64_t)s[k].seg0 + nseg;
            for (uint64_t q = (uint64_t)s[k].seg0 + p; q < q1; q++) {
                if (!sacked[q]) continue;
                n_sacked++;
                if (fd[q].len >= TCP_FRAME_HDR) sum += fd[q].len - TCP_FRAME_HDR;
            }
        }
        /* 4: output */
        t[k].wnd_cap = flow_cc_cap(x->cwnd, sum, &bytes);
        res[k].cwnd = x->cwnd, res[k].sacked_bytes = bytes, res[k].n_sacked = n_sacked, res[k].event = event;
    }
    return LVLIP_OK;
}
