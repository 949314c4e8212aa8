/*
 * snd_cpu.c — the ACK side of a coalesced batch and the retransmit
 * (include/lvlip_skb.h, "f2 on the device: the ACK side and the retransmit"):
 * the plan, and both calls on the calling thread.  The device forms
 * (snd_kernels.hip) leave the same bytes.
 *
 * lvlip_snd_cpu is the fifth check of tcp_input_state (src/tcp_input.c:311-356)
 * with tcp_clean_rto_queue (:66-92) over the records of one lvlip_lro_* call;
 * lvlip_rtx_cpu is what tcp_retransmission_timeout (src/tcp_output.c:359-381)
 * and tcp_send_next (:198-225) do to a queued segment: tcp_transmit_skb
 * (:93-129) writes ack_seq and the window again and sums the whole segment.
 */
#include "flow_step.h"
#include "tcp_hdr.h"

#define SND_HDR TCP_FRAME_HDR

/* ------------------------------------------------------------------ plan -- */

uint32_t lvlip_snd_plan(lvlip_snd_flow *s, uint32_t nflows, uint32_t *nfd)
{
    if (nfd) *nfd = 0;
    if (nflows == 0) return 0;
    if (!s || nflows > LVLIP_LRO_MAX_FLOWS) return FLOW_NONE;
    uint64_t segs = 0, slots = 0;
    uint32_t top = 0, queues = 0;
    for (uint32_t k = 0; k < nflows; k++) {
        if (s[k].reserved != 0 || s[k].reserved2 != 0) return FLOW_NONE;
        if ((uint32_t)(s[k].snd_nxt - s[k].snd_una) > 0x40000000u) return FLOW_NONE;
        if ((uint64_t)s[k].seg0 + s[k].nseg > 0xFFFFFFFFull) return FLOW_NONE;
        segs += s[k].nseg;
        slots += s[k].rtx;
        if (s[k].nseg) {
            queues++;
            if (s[k].seg0 + s[k].nseg > top) top = s[k].seg0 + s[k].nseg;
        }
    }
    if (segs > LVLIP_MAX_BATCH || slots > LVLIP_MAX_BATCH) return FLOW_NONE;
    /* no two queues [seg0, seg0 + nseg) that hold an entry may overlap */
    if (queues > 1u) {
        uint64_t *r = malloc((size_t)queues * 2u * sizeof *r);
        if (!r) return FLOW_NONE;
        uint32_t m = 0;
        for (uint32_t k = 0; k < nflows; k++) {
            if (!s[k].nseg) continue;
            r[2u * m] = s[k].seg0;
            r[2u * m + 1u] = (uint64_t)s[k].seg0 + s[k].nseg;
            m++;
        }
        const int ok = ranges_disjoint(r, m);
        free(r);
        if (!ok) return FLOW_NONE;
    }
    uint32_t slot = 0;
    for (uint32_t k = 0; k < nflows; k++) {
        s[k].slot0 = slot;
        slot += s[k].rtx;
    }
    if (nfd) *nfd = top;
    return slot;
}

/* -------------------------------------------------------------- ACK side -- */

/* seq + dlen of the frame at p (src/tcp.c:46-50), from its 54 header bytes */
static inline uint32_t frame_end_seq(const uint8_t *p)
{
    const uint32_t iplen = ((uint32_t)p[16] << 8) | p[17];
    return be32(p + 38) + iplen - 4u * (p[14] & 0x0fu) - 4u * (p[46] >> 4);
}

int lvlip_snd_cpu(const lvlip_lro_flow *f, const lvlip_snd_flow *s, uint32_t nflows, const lvlip_lro_rec *rec,
                  uint32_t n, const void *base, const lvlip_frame_desc *fd, lvlip_snd_result *res)
{
    if (nflows == 0 || n == 0) return LVLIP_OK;
    if (!f || !s || !rec || !base || !fd || !res) return LVLIP_EINVAL;
    if (n > LVLIP_MAX_BATCH || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    memset(res, 0, (size_t)nflows * sizeof *res);
    for (uint32_t i = 0; i < n; i++) {
        const lvlip_lro_rec *r = &rec[i];
        const uint32_t k = rec_ack_flow(r, f, nflows);
        if (k == FLOW_NONE) continue;
        const uint32_t d = r->ack_seq - s[k].snd_una, span = s[k].snd_nxt - s[k].snd_una;
        switch (flow_ack_class(d, span)) {
        case FLOW_ACK_NEW:
            res[k].n_new++;
            if (d > res[k].acked) res[k].acked = d;
            break;
        case FLOW_ACK_DUP: res[k].n_dup++; break;
        case FLOW_ACK_OLD: res[k].n_old++; break;
        default: res[k].n_beyond++;
        }
    }
    for (uint32_t k = 0; k < nflows; k++) {
        res[k].snd_una = s[k].snd_una + res[k].acked;
        /* tcp_clean_rto_queue, src/tcp_input.c:72-84: stop at the first frame not fully acknowledged */
        uint32_t p = 0;
        for (; p < s[k].nseg; p++) {
            const lvlip_frame_desc *d = &fd[s[k].seg0 + p];
            if (d->len < SND_HDR) break;
            if (frame_end_seq((const uint8_t *)base + d->offset) - s[k].snd_una > res[k].acked) break;
        }
        res[k].popped = p;
        res[k].inflight = s[k].nseg - p;
    }
    return LVLIP_OK;
}

/* ------------------------------------------------------------ retransmit -- */

/* one slot: queue entry e of flow k (FLOW_NONE: dead) rewritten in place as tcp_transmit_skb leaves it */
static void rtx_slot(const lvlip_lro_flow *f, const lvlip_lro_result *lro, const lvlip_snd_flow *s, uint32_t k,
                     uint32_t e, void *base, const lvlip_frame_desc *fd, lvlip_frame_desc *o)
{
    o->offset = 0, o->len = 0, o->reserved = 0;
    if (e == FLOW_NONE) return;
    const lvlip_frame_desc d = fd[e];
    uint8_t *p = (uint8_t *)base + d.offset, *ih = p + 14, *th = p + 34;
    uint32_t iplen, hl;
    if (!rtx_frame_ok(p, d.len, &iplen, &hl)) return;
    /* tcp_transmit_skb, src/tcp_output.c:107,109 and :122,123 */
    put_be32(th + 8, f[k].rcv_nxt + (lro ? lro[k].delivered : 0u));
    th[14] = (uint8_t)(s[k].win >> 8);
    th[15] = (uint8_t)s[k].win;
    tcp_csum_tail(ih, th, iplen - 20u);
    *o = d;
}

static int rtx_args(const lvlip_lro_flow *f, const lvlip_snd_flow *s, uint32_t nflows, uint32_t nslots,
                    const void *base, const lvlip_frame_desc *fd, const lvlip_frame_desc *fd_out)
{
    if (!f || !s || !base || !fd || !fd_out) return LVLIP_EINVAL;
    if (nflows == 0 || nflows > LVLIP_LRO_MAX_FLOWS || nslots > LVLIP_MAX_BATCH) return LVLIP_EINVAL;
    if (s[nflows - 1u].slot0 > nslots || nslots - s[nflows - 1u].slot0 != s[nflows - 1u].rtx) return LVLIP_EINVAL;
    return LVLIP_OK;
}

int lvlip_rtx_cpu(const lvlip_lro_flow *f, const lvlip_lro_result *lro, const lvlip_snd_flow *s,
                  const lvlip_snd_result *snd, uint32_t nflows, uint32_t nslots, void *base,
                  const lvlip_frame_desc *fd, lvlip_frame_desc *fd_out)
{
    if (nslots == 0) return LVLIP_OK;
    if (rtx_args(f, s, nflows, nslots, base, fd, fd_out) != LVLIP_OK) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++) {
        const uint32_t popped = snd ? snd[k].popped : 0u;
        for (uint32_t j = 0; j < s[k].rtx; j++) {
            const int live = popped < s[k].nseg && j < s[k].nseg - popped;
            rtx_slot(f, lro, s, k, live ? s[k].seg0 + popped + j : FLOW_NONE, base, fd, &fd_out[s[k].slot0 + j]);
        }
    }
    return LVLIP_OK;
}

/* the selective retransmit ("the scoreboard and the selective retransmit"): slot j is the j-th
 * queue entry behind the popped ones whose scoreboard byte is 0 */
int lvlip_rtx_sack_cpu(const lvlip_lro_flow *f, const lvlip_lro_result *lro, const lvlip_snd_flow *s,
                       const lvlip_snd_result *snd, const uint8_t *sacked, uint32_t nflows, uint32_t nslots,
                       void *base, const lvlip_frame_desc *fd, lvlip_frame_desc *fd_out, uint32_t *pick)
{
    if (nslots == 0) return LVLIP_OK;
    if (!pick || rtx_args(f, s, nflows, nslots, base, fd, fd_out) != LVLIP_OK) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++) {
        const uint32_t popped = snd ? snd[k].popped : 0u;
        uint32_t q = popped < s[k].nseg ? popped : s[k].nseg;
        for (uint32_t j = 0; j < s[k].rtx; j++) {
            while (q < s[k].nseg && sacked && sacked[s[k].seg0 + q] != 0) q++;
            const uint32_t e = q < s[k].nseg ? s[k].seg0 + q++ : FLOW_NONE;
            pick[s[k].slot0 + j] = e;
            rtx_slot(f, lro, s, k, e, base, fd, &fd_out[s[k].slot0 + j]);
        }
    }
    return LVLIP_OK;
}

/* ------------------------------------------------------------------ next -- */

int lvlip_snd_next_cpu(lvlip_snd_flow *s, lvlip_snd_result *res, uint32_t nflows)
{
    if (nflows == 0) return LVLIP_OK;
    if (!s || !res || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++) {
        const uint32_t p = res[k].popped < s[k].nseg ? res[k].popped : s[k].nseg;
        s[k].snd_una = res[k].snd_una;
        s[k].seg0 += p;
        s[k].nseg -= p;
        res[k].popped = 0;
        res[k].acked = 0;
        res[k].inflight = s[k].nseg;
    }
    return LVLIP_OK;
}
