/*
 * ack_cpu.c — the acknowledgement of a coalesced batch (include/lvlip_skb.h,
 * "f1 on the device: the acknowledgement"): the plan, and the frames on the
 * calling thread.  The device form (ack_kernels.hip) writes the same bytes.
 *
 * What tcp_send_ack does per connection (src/tcp_output.c:247-267 ->
 * tcp_write_options, :65-91 -> tcp_transmit_skb, :93-129 -> ip_output,
 * src/ip_output.c:14-56), with the template standing for the socket's state
 * and the flow's lvlip_lro_result for rcv_nxt and the SACK list.
 */
#include "tcp_hdr.h"

#define ACK_HDR TCP_FRAME_HDR
#define NONE 0xFFFFFFFFu

/* ------------------------------------------------------------------ plan -- */

static int tmpl_ok(const lvlip_ack_tmpl *t, const lvlip_lro_flow *f)
{
    const uint8_t *h = t->hdr;
    if (t->max_sack > 4u || t->reserved != 0 || !tcp_tmpl_ok(h)) return 0;
    /* the reverse of the flow: what the peer sends from is where the ACK goes */
    if (memcmp(h + 26, &f->daddr, 4) != 0 || memcmp(h + 30, &f->saddr, 4) != 0) return 0;
    if (memcmp(h + 34, &f->dport, 2) != 0 || memcmp(h + 36, &f->sport, 2) != 0) return 0;
    return t->out_off <= UINT64_MAX - LVLIP_ACK_MAX_FRAME;
}

uint32_t lvlip_ack_plan(const lvlip_ack_tmpl *t, const lvlip_lro_flow *f, uint32_t nflows, uint64_t *out_bytes)
{
    if (out_bytes) *out_bytes = 0;
    if (nflows == 0) return 0;
    if (!t || !f || nflows > LVLIP_LRO_MAX_FLOWS) return NONE;
    uint64_t top = 0;
    for (uint32_t k = 0; k < nflows; k++) {
        if (!tmpl_ok(&t[k], &f[k])) return NONE;
        if (t[k].out_off + LVLIP_ACK_MAX_FRAME > top) top = t[k].out_off + LVLIP_ACK_MAX_FRAME;
    }
    /* no two slots [out_off, out_off + LVLIP_ACK_MAX_FRAME) may overlap */
    uint64_t *r = malloc((size_t)nflows * 2u * sizeof *r);
    if (!r) return NONE;
    for (uint32_t k = 0; k < nflows; k++) {
        r[2u * k] = t[k].out_off;
        r[2u * k + 1u] = t[k].out_off + LVLIP_ACK_MAX_FRAME;
    }
    const int ok = ranges_disjoint(r, nflows);
    free(r);
    if (!ok) return NONE;
    if (out_bytes) *out_bytes = top;
    return nflows;
}

/* ------------------------------------------------------------ the frames -- */

int lvlip_ack_cpu(const lvlip_ack_tmpl *t, const lvlip_lro_flow *f, const lvlip_lro_result *res,
                  uint32_t nflows, uint32_t flags, void *out, lvlip_frame_desc *fd)
{
    if (nflows == 0) return LVLIP_OK;
    if (!t || !f || !res || !out) return LVLIP_EINVAL;
    if ((flags & ~LVLIP_ACK_ALL) || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++) {
        const uint64_t off = t[k].out_off;
        if (!(flags & LVLIP_ACK_ALL) && res[k].placed == 0) {
            if (fd) fd[k].offset = off, fd[k].len = 0, fd[k].reserved = 0;
            continue;
        }
        /* tcp_options_len, src/tcp_output.c:227-245 */
        uint32_t b = res[k].nsack < 4u ? res[k].nsack : 4u;
        if (b > t[k].max_sack) b = t[k].max_sack;
        const uint32_t optlen = b ? 4u + 8u * b : 0u;
        uint8_t *p = (uint8_t *)out + off;
        uint8_t *ih = p + 14, *th = p + 34;
        memcpy(p, t[k].hdr, ACK_HDR);
        /* tcp_send_ack: hl (src/tcp_output.c:261); tcp_transmit_skb: ack_seq,
         * the options (:107,113-115) */
        put_be32(th + 8, f[k].rcv_nxt + res[k].delivered);
        th[12] = (uint8_t)(((5u + optlen / 4u) << 4) | (th[12] & 0x0fu));
        if (b) {
            /* tcp_write_options, src/tcp_output.c:71-86: the last block first */
            uint8_t *o = th + 20;
            o[0] = 1, o[1] = 1, o[2] = 5, o[3] = (uint8_t)(2u + 8u * b);
            o += 4;
            for (uint32_t i = b; i-- > 0; o += 8) {
                put_be32(o, res[k].sack[i].left);
                put_be32(o + 4, res[k].sack[i].right);
            }
        }
        ip_output_tail(ih, 40u + optlen);
        tcp_csum_tail(ih, th, 20u + optlen);
        if (fd) fd[k].offset = off, fd[k].len = ACK_HDR + optlen, fd[k].reserved = 0;
    }
    return LVLIP_OK;
}
