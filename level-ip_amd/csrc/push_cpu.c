/*
 * push_cpu.c — the write queue (include/lvlip_skb.h, "f2 on the device: the
 * write queue"): the plan, and the call on the calling thread.  The device
 * form (push_kernels.hip) leaves the same bytes.
 *
 * tcp_send (src/tcp_output.c:445-478) cuts a write into segments and
 * tcp_queue_transmit_skb (:131-156) appends each to the write queue; here a
 * round's worth of every flow's ready bytes becomes frames in the flow's slots
 * of the TX ring, through tcp_seg_write, the frame writer lvlip_tso_cpu uses.
 */
#include "flow_step.h"
#include "tcp_hdr.h"

#define PUSH_MAX_BYTES 0x40000000u
#define TCP_NO_PUSH_FLAGS 0x27u /* byte 13 of the TCP header: FIN 0x01, SYN 0x02, RST 0x04, URG 0x20 */

/* flow k's own fields and its queue, as the plan wants them */
static int flow_ok(const lvlip_push_flow *w, const lvlip_snd_flow *s)
{
    if (w->cap == 0 || w->slot_nxt >= w->cap) return 0;
    if (w->mss == 0 || w->mss > TCP_MSS_MAX || w->stride < TCP_FRAME_HDR + w->mss) return 0;
    if (w->unsent > PUSH_MAX_BYTES || w->wnd > PUSH_MAX_BYTES || w->reserved != 0) return 0;
    for (size_t i = 0; i < sizeof w->pad; i++)
        if (w->pad[i] != 0) return 0;
    if (!tcp_tmpl_ok(w->hdr) || (w->hdr[47] & TCP_NO_PUSH_FLAGS)) return 0;
    if ((uint64_t)w->q0 + w->cap > 0xFFFFFFFFull) return 0;
    if ((uint64_t)w->cap * w->stride > UINT64_MAX - w->ring_off) return 0;
    if (s->nseg && (s->seg0 < w->q0 || (uint64_t)s->seg0 + s->nseg > (uint64_t)w->q0 + w->cap)) return 0;
    return 1;
}

uint32_t lvlip_push_plan(lvlip_push_flow *w, const lvlip_snd_flow *s, uint32_t nflows, uint64_t *ring_bytes,
                         uint32_t *nfd)
{
    if (ring_bytes) *ring_bytes = 0;
    if (nfd) *nfd = 0;
    if (nflows == 0) return 0;
    if (!w || !s || nflows > LVLIP_LRO_MAX_FLOWS) return FLOW_NONE;
    uint64_t slots = 0, caps = 0, top = 0;
    uint32_t topq = 0;
    for (uint32_t k = 0; k < nflows; k++) {
        if (!flow_ok(&w[k], &s[k])) return FLOW_NONE;
        slots += w[k].push;
        caps += w[k].cap;
        const uint64_t end = w[k].ring_off + (uint64_t)(w[k].cap - 1u) * w[k].stride + TCP_FRAME_HDR + w[k].mss;
        if (end > top) top = end;
        if (w[k].q0 + w[k].cap > topq) topq = w[k].q0 + w[k].cap;
    }
    if (slots > LVLIP_MAX_BATCH || caps > LVLIP_MAX_BATCH) return FLOW_NONE;
    /* no two fd regions and no two ring ranges may share an element */
    if (nflows > 1u) {
        uint64_t *r = malloc((size_t)nflows * 2u * sizeof *r);
        if (!r) return FLOW_NONE;
        for (uint32_t k = 0; k < nflows; k++) {
            r[2u * k] = w[k].q0;
            r[2u * k + 1u] = (uint64_t)w[k].q0 + w[k].cap;
        }
        int ok = ranges_disjoint(r, nflows);
        for (uint32_t k = 0; ok && k < nflows; k++) {
            r[2u * k] = w[k].ring_off;
            r[2u * k + 1u] = w[k].ring_off + (uint64_t)w[k].cap * w[k].stride;
        }
        ok = ok && ranges_disjoint(r, nflows);
        free(r);
        if (!ok) return FLOW_NONE;
    }
    uint32_t slot = 0;
    for (uint32_t k = 0; k < nflows; k++) {
        w[k].slot0 = slot;
        slot += w[k].push;
    }
    if (ring_bytes) *ring_bytes = top;
    if (nfd) *nfd = topq;
    return slot;
}

int lvlip_push_cpu(const lvlip_lro_flow *f, const lvlip_lro_result *lro, lvlip_snd_flow *s, lvlip_push_flow *w,
                   uint32_t nflows, uint32_t nslots, const void *payload, void *base, lvlip_frame_desc *fd,
                   uint8_t *sacked, lvlip_frame_desc *fd_out, lvlip_push_result *res)
{
    if (nflows > LVLIP_LRO_MAX_FLOWS || nslots > LVLIP_MAX_BATCH) return LVLIP_EINVAL;
    if (nslots && (!payload || !base || !fd_out || nflows == 0)) return LVLIP_EINVAL;
    if (nflows == 0) return LVLIP_OK;
    if (!f || !s || !w || !fd || !res) return LVLIP_EINVAL;
    uint64_t slot = 0;
    for (uint32_t k = 0; k < nflows; k++) {
        if (!flow_ok(&w[k], &s[k]) || w[k].slot0 != slot) return LVLIP_EINVAL;
        slot += w[k].push;
    }
    if (slot != nslots) return LVLIP_EINVAL;

    for (uint32_t k = 0; k < nflows; k++) {
        lvlip_push_flow *t = &w[k];
        lvlip_snd_flow *q = &s[k];
        /* 1: the queue down to q0 */
        uint32_t moved = 0;
        if (q->seg0 != t->q0) {
            memmove(&fd[t->q0], &fd[q->seg0], (size_t)q->nseg * sizeof *fd);
            if (sacked) memmove(&sacked[t->q0], &sacked[q->seg0], q->nseg);
            q->seg0 = t->q0;
            moved = q->nseg;
        }
        /* 2: the count */
        uint32_t bytes;
        const uint32_t m = flow_push_count(t, q, &bytes);
        /* 3: the template as tcp_transmit_skb would fill it now (src/tcp_output.c:107-109) */
        uint8_t hdr[TCP_FRAME_HDR];
        memcpy(hdr, t->hdr, sizeof hdr);
        put_be32(hdr + 42, f[k].rcv_nxt + (lro ? lro[k].delivered : 0u));
        hdr[48] = (uint8_t)(q->win >> 8);
        hdr[49] = (uint8_t)q->win;
        const uint8_t *src = (const uint8_t *)payload + t->pay_off;
        const uint32_t first = t->q0 + q->nseg;
        for (uint32_t i = 0; i < t->push; i++) {
            lvlip_frame_desc *o = &fd_out[t->slot0 + i];
            o->offset = 0, o->len = 0, o->reserved = 0;
            if (i >= m) continue;
            const uint64_t done = (uint64_t)i * t->mss;
            const uint32_t dlen = t->unsent - done < t->mss ? (uint32_t)(t->unsent - done) : t->mss;
            o->offset = t->ring_off + (((uint64_t)t->slot_nxt + i) % t->cap) * t->stride;
            o->len = TCP_FRAME_HDR + dlen;
            tcp_seg_write((uint8_t *)base + o->offset, hdr, src + done, dlen, q->snd_nxt + (uint32_t)done,
                          done + dlen == t->unsent);
            fd[first + i] = *o;
            if (sacked) sacked[first + i] = 0;
        }
        /* 4 */
        res[k].pushed = m, res[k].bytes = bytes, res[k].first = first, res[k].moved = moved;
        q->nseg += m;
        q->snd_nxt += bytes;
        t->pay_off += bytes;
        t->unsent -= bytes;
        t->slot_nxt = (uint32_t)(((uint64_t)t->slot_nxt + m) % t->cap);
    }
    return LVLIP_OK;
}
