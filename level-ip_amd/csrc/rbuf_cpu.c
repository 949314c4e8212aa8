/*
 * rbuf_cpu.c — the receive buffer (include/lvlip_skb.h, "f1: the receive
 * buffer"): the plan, the state check and the call on the calling
 * thread.  There is no device form yet.
 *
 * The read is tcp_data_dequeue's copy (src/tcp_data.c:49-85); where the
 * reference frees the skbs it has copied out, the bytes that are left move to
 * the buffer's front.  The steps are flow_step.h's; the copies are memcpy
 * (step 3's two ranges cannot overlap).
 */
#include <stdlib.h>

#include "flow_step.h"
#include "tcp_hdr.h"

/* the invariants of one flow against its lro flow; the disjointness and
 * piece0 are the batch's */
static int rbuf_flow_ok(const lvlip_rbuf_flow *x, const lvlip_lro_flow *f)
{
    if (x->cap == 0u || x->cap > LVLIP_LRO_MAX_WND || x->mss == 0u || x->wscale > LVLIP_WSCALE_MAX) return 0;
    for (size_t j = 0; j < sizeof x->reserved; j++)
        if (x->reserved[j]) return 0;
    if (x->base_off > UINT64_MAX - x->cap || x->base_off > f->out_off) return 0;
    const uint64_t used = f->out_off - x->base_off;
    if (used > x->cap || f->rcv_wnd != x->cap - used || x->head > used) return 0;
    return 1;
}

/* 0, LVLIP_EINVAL or LVLIP_ENOMEM; with_pieces: piece0 must be the plan's */
static int rbuf_state(const lvlip_rbuf_flow *p, const lvlip_lro_flow *f, uint32_t nflows, int with_pieces,
                      uint64_t *npieces)
{
    if (!p || !f || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    uint64_t sum = 0;
    for (uint32_t k = 0; k < nflows; k++) {
        if (!rbuf_flow_ok(&p[k], &f[k])) return LVLIP_EINVAL;
        if (with_pieces && p[k].piece0 != sum) return LVLIP_EINVAL;
        sum += ((uint64_t)p[k].cap + LVLIP_RBUF_PIECE - 1u) / LVLIP_RBUF_PIECE;
    }
    if (sum > 0x80000000ull) return LVLIP_EINVAL;
    uint64_t *r = malloc((size_t)nflows * 2u * sizeof *r);
    if (!r) return LVLIP_ENOMEM;
    for (uint32_t k = 0; k < nflows; k++) {
        r[2u * k] = p[k].base_off;
        r[2u * k + 1u] = p[k].base_off + p[k].cap;
    }
    const int ok = ranges_disjoint(r, nflows);
    free(r);
    if (!ok) return LVLIP_EINVAL;
    if (npieces) *npieces = sum;
    return LVLIP_OK;
}

uint32_t lvlip_rbuf_plan(lvlip_rbuf_flow *p, const lvlip_lro_flow *f, uint32_t nflows, uint64_t *npieces)
{
    if (nflows == 0) {
        if (npieces) *npieces = 0;
        return 0;
    }
    uint64_t sum = 0;
    if (rbuf_state(p, f, nflows, 0, &sum) != LVLIP_OK) return FLOW_NONE;
    uint32_t at = 0;
    for (uint32_t k = 0; k < nflows; k++) {
        p[k].piece0 = at;
        at += (uint32_t)(((uint64_t)p[k].cap + LVLIP_RBUF_PIECE - 1u) / LVLIP_RBUF_PIECE);
    }
    if (npieces) *npieces = sum;
    return nflows;
}

int lvlip_rbuf_check(const lvlip_rbuf_flow *p, const lvlip_lro_flow *f, uint32_t nflows)
{
    if (nflows == 0) return LVLIP_OK;
    return rbuf_state(p, f, nflows, 1, NULL);
}

int lvlip_rbuf_cpu(lvlip_lro_flow *f, const lvlip_lro_result *res, lvlip_rbuf_flow *p, lvlip_ack_tmpl *t,
                   uint32_t nflows, const uint32_t *nread, void *out, void *sink, lvlip_lro_result *gate,
                   lvlip_rbuf_result *rres)
{
    if (nflows == 0) return LVLIP_OK;
    if (!f || !res || !p || !t || !out || !gate || !rres || gate == res) return LVLIP_EINVAL;
    if (nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    const int rc = lvlip_rbuf_check(p, f, nflows);
    if (rc != LVLIP_OK) return rc;
    for (uint32_t k = 0; k < nflows; k++) {
        uint8_t *buf = (uint8_t *)out + p[k].base_off;
        const flow_rbuf_out o = flow_rbuf_step(&p[k], &f[k].out_off, &f[k].rcv_wnd, f[k].rcv_nxt,
                                               nread ? nread[k] : 0u, sink != NULL, res[k].sack, res[k].nsack,
                                               res[k].placed);
        if (sink && o.read) memcpy((uint8_t *)sink + o.rd_to, buf + o.rd_from, o.read);
        if (o.moved) memcpy(buf, buf + o.mv_from, o.moved); /* moved <= mv_from: disjoint */
        t[k].hdr[48] = (uint8_t)(o.field >> 8);
        t[k].hdr[49] = (uint8_t)o.field;
        gate[k] = res[k];
        if (o.flags & LVLIP_RBUF_UPDATE) gate[k].placed = 1u;
        rres[k].read = o.read, rres[k].unread = o.unread, rres[k].head = p[k].head, rres[k].moved = o.moved;
        rres[k].adv = o.adv, rres[k].field = o.field, rres[k].flags = o.flags, rres[k].reserved = 0u;
    }
    return LVLIP_OK;
}
