/*
 * cc_cpu.c — the congestion window (include/lvlip_skb.h, "f2 on the device:
 * the congestion window"): the state check and the call on the calling
 * thread.  The device form (cc_kernels.hip) leaves the same bytes.
 *
 * The reference has no congestion control (its cwnd, include/tcp.h:211, is
 * never touched); the steps are RFC 5681 (slow start, avoidance, the cut on a
 * timeout), RFC 3465 (byte counting), RFC 6582 (recover) and RFC 6675 (pipe).
 */
#include "lvlip_skb.h"

#define CC_HDR 54u /* the header of every frame lvlip_tso_* / lvlip_push_* build */
#define CC_MSS_MAX 65495u

int lvlip_cc_check(const lvlip_cc_flow *c, uint32_t nflows)
{
    if (nflows == 0) return LVLIP_OK;
    if (!c || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++) {
        const uint32_t mss = c[k].mss;
        if (mss == 0 || mss > CC_MSS_MAX) return LVLIP_EINVAL;
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
        const uint32_t mss = x->mss, nxt = s[k].snd_nxt, una = s[k].snd_una;
        const uint32_t flight = nxt - una;
        const uint32_t a = snd ? snd[k].acked : 0u, n_new = snd ? snd[k].n_new : 0u;
        const uint32_t fired = prev ? prev[k].fired : 0u, bo = prev ? prev[k].backoff : 0u;
        const uint32_t half = flight / 2u > 2u * mss ? flight / 2u : 2u * mss;
        uint32_t event = 0;
        /* 1: loss */
        if (fired == LVLIP_RTO_TIMEOUT) {
            if (bo == 1u) x->ssthresh = half;
            x->cwnd = mss, x->acc = 0, x->in_rec = 0, x->recover = nxt;
            event |= LVLIP_CC_EV_TIMEOUT;
        } else if (fired == LVLIP_RTO_FASTRTX && !x->in_rec) {
            x->ssthresh = half, x->cwnd = half, x->acc = 0, x->in_rec = 1, x->recover = nxt;
            event |= LVLIP_CC_EV_ENTER;
        }
        /* 2: ACKs */
        if (n_new && a) {
            uint64_t cwnd = x->cwnd;
            if (x->in_rec) {
                if (a >= (uint32_t)(x->recover - una)) {
                    x->in_rec = 0, x->acc = 0;
                    cwnd = x->ssthresh;
                    event |= LVLIP_CC_EV_EXIT;
                }
            } else if (cwnd < x->ssthresh) {
                const uint64_t cap = (uint64_t)n_new * mss;
                cwnd += a < cap ? a : cap;
                event |= LVLIP_CC_EV_SLOWSTART;
            } else {
                uint64_t acc = (uint64_t)x->acc + a;
                if (acc >= cwnd) {
                    acc -= cwnd;
                    cwnd += mss;
                    event |= LVLIP_CC_EV_AVOID;
                }
                x->acc = (uint32_t)(acc < cwnd ? acc : cwnd);
            }
            x->cwnd = (uint32_t)(cwnd < x->cwnd_max ? cwnd : x->cwnd_max);
        }
        /* 3: pipe */
        uint64_t bytes = 0;
        uint32_t n_sacked = 0;
        if (sacked) {
            const uint32_t nseg = s[k].nseg;
            const uint32_t p = snd && snd[k].popped < nseg ? snd[k].popped : snd ? nseg : 0u;
            const uint64_t q1 = (uint64_t)s[k].seg0 + nseg;
            for (uint64_t q = (uint64_t)s[k].seg0 + p; q < q1; q++) {
                if (!sacked[q]) continue;
                n_sacked++;
                if (fd[q].len >= CC_HDR) bytes += fd[q].len - CC_HDR;
            }
            if (bytes > LVLIP_CC_MAX_WND) bytes = LVLIP_CC_MAX_WND;
        }
        /* 4: output */
        const uint64_t cap = (uint64_t)x->cwnd + bytes;
        t[k].wnd_cap = cap < LVLIP_CC_MAX_WND ? (uint32_t)cap : LVLIP_CC_MAX_WND;
        res[k].cwnd = x->cwnd, res[k].sacked_bytes = (uint32_t)bytes, res[k].n_sacked = n_sacked, res[k].event = event;
    }
    return LVLIP_OK;
}
