/*
 * fin_cpu.c — the end of a connection (include/lvlip_skb.h, "the end of a
 * connection: FIN and TIME-WAIT"): the state check and the call on the calling
 * thread.  The device form (fin_kernels.hip) leaves the same bytes.
 *
 * tcp_close -> tcp_queue_fin (src/tcp.c:255-285, src/tcp_output.c:506-523), the
 * fifth and eighth checks of tcp_input_state (src/tcp_input.c:359-389,
 * :417-467) and tcp_enter_time_wait (src/tcp.c:402-411).  The states' steps are
 * flow_step.h's; the FIN is a segment of no bytes through tcp_seg_write, the
 * frame writer lvlip_persist_cpu uses, on the template as it patches it.
 */
#include "flow_step.h"
#include "tcp_hdr.h"

/* everything lvlip_fin_check tests but base */
static int fin_state_ok(const lvlip_fin_flow *x)
{
    if (x->state < LVLIP_TCP_ESTABLISHED || x->state > LVLIP_TCP_TIME_WAIT) return 0;
    for (unsigned j = 0; j < sizeof x->reserved; j++)
        if (x->reserved[j]) return 0;
    return x->interval <= LVLIP_FIN_MAX_MS;
}

int lvlip_fin_check(const lvlip_fin_flow *x, const lvlip_lro_flow *f, uint32_t nflows)
{
    if (nflows == 0) return LVLIP_OK;
    if (!x || !f || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++)
        if (!fin_state_ok(&x[k]) || x[k].base != f[k].rcv_nxt) return LVLIP_EINVAL;
    return LVLIP_OK;
}

size_t lvlip_fin_workspace_bytes(uint32_t nflows)
{
    const size_t b = ((size_t)2u * nflows + 15u) & ~(size_t)15u;
    return b ? b : 16u;
}

int lvlip_fin_cpu(lvlip_lro_flow *f, const lvlip_lro_result *gin, const lvlip_lro_rec *rec, uint32_t n,
                  lvlip_snd_flow *s, const lvlip_push_flow *w, const lvlip_rto_flow *t, lvlip_fin_flow *x,
                  uint32_t nflows, const uint8_t *close, uint32_t now, void *out, lvlip_frame_desc *fd_out,
                  lvlip_lro_result *gate, lvlip_fin_result *res)
{
    if (nflows == 0) return LVLIP_OK;
    if (!f || !gin || !s || !w || !t || !x || !out || !fd_out || !gate || !res || (!rec && n)) return LVLIP_EINVAL;
    if (gate == gin || nflows > LVLIP_LRO_MAX_FLOWS || n > LVLIP_MAX_BATCH) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++)
        if (!fin_state_ok(&x[k])) return LVLIP_EINVAL;
    /* 1: the FIN records.  res[k].events holds bit 0 for hit and bit 1 for again until flow k's turn below. */
    for (uint32_t k = 0; k < nflows; k++) res[k].events = 0;
    for (uint32_t i = 0; i < n; i++) {
        const lvlip_lro_rec *r = &rec[i];
        if (r->flow >= nflows || !(r->tcp_flags & 0x01u)) continue;
        if (r->status != LVLIP_LRO_PLACED && r->status != LVLIP_LRO_NO_DATA) continue;
        const uint32_t k = r->flow, key = r->rel + r->dlen;
        const uint32_t target = f[k].rcv_nxt + gin[k].delivered - x[k].base;
        if (key == target) res[k].events |= 1u;
        if (key == target - 1u) res[k].events |= 2u;
    }
    for (uint32_t k = 0; k < nflows; k++) {
        const uint32_t hit = res[k].events & 1u, again = res[k].events & 2u;
        const flow_fin_out o = flow_fin_step(&x[k], t[k].dead, f[k].rcv_nxt, s[k].snd_una, s[k].snd_nxt, s[k].nseg,
                                             w[k].unsent, t[k].rto, hit, again, close ? close[k] : 0u, now);
        f[k].rcv_nxt = o.rcv_nxt;
        s[k].snd_nxt = o.snd_nxt;
        gate[k] = gin[k];
        if ((o.events & LVLIP_FIN_EV_ACK_OWED) && gin[k].placed == 0) gate[k].placed = 1;
        res[k].events = o.events, res[k].state = x[k].state;
        res[k].seq = o.frame ? x[k].fin_seq : 0u, res[k].interval = o.interval;
        fd_out[k].offset = (uint64_t)LVLIP_PERSIST_SLOT * k;
        fd_out[k].len = o.frame ? TCP_FRAME_HDR : 0u;
        fd_out[k].reserved = 0;
        if (!o.frame) continue;
        /* the template as tcp_transmit_skb would fill it now (src/tcp_output.c:107-109); tcp_queue_fin's flags */
        uint8_t hdr[TCP_FRAME_HDR];
        memcpy(hdr, w[k].hdr, sizeof hdr);
        put_be32(hdr + 42, o.rcv_nxt + gin[k].delivered);
        hdr[47] = (uint8_t)((hdr[47] & ~0x08u) | 0x11u);
        hdr[48] = (uint8_t)(s[k].win >> 8);
        hdr[49] = (uint8_t)s[k].win;
        tcp_seg_write((uint8_t *)out + fd_out[k].offset, hdr, hdr, 0u, x[k].fin_seq, 1);
    }
    return LVLIP_OK;
}
