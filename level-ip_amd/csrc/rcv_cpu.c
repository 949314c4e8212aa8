/*
 * rcv_cpu.c — TCP receive coalescing (include/lvlip_skb.h, "f1 on the device:
 * receive coalescing"): the plan, the batch on the calling thread, the
 * advance step, alone and with the islands an earlier batch left, and the step
 * that moves the flows on to the next batch.  The device forms
 * (rcv_kernels.hip, adv_kernels.hip, next_kernels.hip) write the same records,
 * results and bytes.
 *
 * What ip_rcv (src/ip_input.c:17-60), tcp_in / tcp_init_segment
 * (src/tcp.c:36-85), tcp_data_queue (src/tcp_data.c:87-128) and
 * tcp_data_dequeue (:49-85) do per skb, with a planned flow standing for the
 * socket's tcb.
 */
#include "tcp_hdr.h"

#define ETH_HDR_LEN 14u
#define PROTO_ICMP 1u
#define PROTO_TCP 6u
#define TCP_CONTROL 0x26u /* byte 13 of the TCP header: SYN 0x02, RST 0x04, URG 0x20 */
#define NONE 0xFFFFFFFFu

static inline uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }

/* lvlip_pseudo_sum_rfc (skb_batch.c): the pseudo header as 16-bit halves; len is at most 65535 */
static inline uint32_t pseudo_rfc(uint32_t s, uint32_t d, uint32_t proto, uint32_t len)
{
    return (s & 0xffffu) + (s >> 16) + (d & 0xffffu) + (d >> 16) + bswap16((uint16_t)proto) + bswap16((uint16_t)len);
}

/* ------------------------------------------------------------------ plan -- */

static int key_cmp(const void *a, const void *b) { return memcmp(a, b, 12); }

uint32_t lvlip_lro_plan(lvlip_lro_flow *f, uint32_t n, uint64_t *out_bytes)
{
    static const uint8_t zero[8] = {0};
    if (out_bytes) *out_bytes = 0;
    if (n == 0) return 0;
    if (!f || n > LVLIP_LRO_MAX_FLOWS) return NONE;
    uint64_t top = 0;
    for (uint32_t k = 0; k < n; k++) {
        if (f[k].rcv_wnd == 0 || f[k].rcv_wnd > LVLIP_LRO_MAX_WND || f[k].reserved != 0) return NONE;
        if (memcmp(f[k].pad, zero, sizeof zero) != 0) return NONE;
        if (f[k].out_off > UINT64_MAX - f[k].rcv_wnd) return NONE;
        const uint64_t end = f[k].out_off + f[k].rcv_wnd;
        if (end > top) top = end;
    }
    /* no two ranges [out_off, out_off + rcv_wnd) may overlap */
    uint64_t *r = malloc((size_t)n * 2u * sizeof *r);
    if (!r) return NONE;
    for (uint32_t k = 0; k < n; k++) {
        r[2u * k] = f[k].out_off;
        r[2u * k + 1u] = f[k].out_off + f[k].rcv_wnd;
    }
    int bad = !ranges_disjoint(r, n);
    free(r);
    if (bad) return NONE;
    /* a duplicate key shows as equal neighbours after the sort; the flows are
     * reordered only when the whole plan is good */
    lvlip_lro_flow *s = malloc((size_t)n * sizeof *s);
    if (!s) return NONE;
    memcpy(s, f, (size_t)n * sizeof *s);
    qsort(s, n, sizeof *s, key_cmp);
    for (uint32_t k = 1; k < n && !bad; k++) bad = key_cmp(&s[k - 1u], &s[k]) == 0;
    if (!bad) memcpy(f, s, (size_t)n * sizeof *s);
    free(s);
    if (bad) return NONE;
    if (out_bytes) *out_bytes = top;
    return n;
}

/* ------------------------------------------------------------- the batch -- */

/* the flow with these 12 key bytes, or NONE: the device's search */
static uint32_t find_flow(const lvlip_lro_flow *f, uint32_t nflows, const uint8_t key[12])
{
    uint32_t lo = 0, hi = nflows;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (memcmp(&f[mid], key, 12) < 0) lo = mid + 1u;
        else hi = mid;
    }
    return lo < nflows && memcmp(&f[lo], key, 12) == 0 ? lo : NONE;
}

/* One frame: its record, and where its payload goes (*src, *dst set only for
 * PLACED).  The decisions up to UNKNOWN_PROTO are rx_verdict_one's
 * (skb_batch.c), in ip_rcv's order. */
static void lro_one(const uint8_t *h, uint32_t flen, const lvlip_lro_flow *f, uint32_t nflows, uint32_t flags,
                    lvlip_lro_rec *r, const uint8_t **src, uint64_t *dst)
{
    memset(r, 0, sizeof *r);
    r->flow = NONE;
    if (flen < ETH_HDR_LEN + 20u) { r->status = LVLIP_RX_SHORT; return; }
    if (be16(h + 12) != 0x0800u) { r->status = LVLIP_RX_NOT_IP; return; } /* src/netdev.c:67-80 */
    const uint8_t *ih = h + ETH_HDR_LEN;
    const uint32_t ihl = ih[0] & 0x0fu;
    if ((ih[0] >> 4) != 4u) { r->status = LVLIP_RX_BAD_VERSION; return; } /* src/ip_input.c:22 */
    if (ihl < 5u) { r->status = LVLIP_RX_BAD_IHL; return; }                /* :27 */
    if (ih[8] == 0u) { r->status = LVLIP_RX_TTL0; return; }                /* :32 */
    if (flen < ETH_HDR_LEN + ihl * 4u) { r->status = LVLIP_RX_SHORT; return; }
    if (checksum((void *)ih, (int)(ihl * 4u), 0) != 0) { r->status = LVLIP_RX_BAD_CSUM; return; } /* :38-43 */
    const uint32_t proto = ih[9];
    if (proto != PROTO_TCP && proto != PROTO_ICMP) { r->status = LVLIP_RX_UNKNOWN_PROTO; return; } /* :51-60 */
    const uint32_t iplen = be16(ih + 2);
    const int inside = iplen >= ihl * 4u && flen >= ETH_HDR_LEN + iplen;
    const uint32_t l4len = inside ? iplen - ihl * 4u : 0u;
    const uint8_t *th = ih + ihl * 4u;
    if (flags & LVLIP_RX_VERIFY_L4) {
        if (!inside) { r->status = LVLIP_RX_SHORT; return; }
        const uint32_t seed = proto == PROTO_TCP ? pseudo_rfc(le32(ih + 12), le32(ih + 16), PROTO_TCP, l4len) : 0u;
        if (checksum((void *)th, (int)l4len, (int)seed) != 0) { r->status = LVLIP_RX_BAD_L4; return; }
    }
    /* ip_rcv keeps the frame */
    if (proto != PROTO_TCP) { r->status = LVLIP_LRO_NOT_TCP; return; }
    if (!inside || l4len < 20u) { r->status = LVLIP_LRO_BAD_TCP_HDR; return; }
    const uint32_t hl = th[12] >> 4;
    if (hl < 5u || hl * 4u > l4len) { r->status = LVLIP_LRO_BAD_TCP_HDR; return; }
    /* tcp_init_segment, src/tcp.c:40-50 */
    const uint32_t seq = be32(th + 4);
    const uint32_t dlen = l4len - hl * 4u;
    r->dlen = (uint16_t)dlen;
    r->tcp_flags = th[13];
    r->ack_seq = be32(th + 8);
    r->rel = seq;
    uint8_t key[12];
    memcpy(key, ih + 12, 8);
    memcpy(key + 8, th, 4);
    const uint32_t k = find_flow(f, nflows, key);
    if (k == NONE) { r->status = LVLIP_LRO_NO_FLOW; return; }
    r->flow = k;
    r->rel = seq - f[k].rcv_nxt;
    if (th[13] & TCP_CONTROL) { r->status = LVLIP_LRO_CONTROL; return; }
    if (dlen == 0u) { r->status = LVLIP_LRO_NO_DATA; return; }
    if ((uint64_t)r->rel + dlen > f[k].rcv_wnd) { r->status = LVLIP_LRO_OUT_OF_WINDOW; return; }
    r->status = LVLIP_LRO_PLACED;
    *src = th + hl * 4u;
    *dst = f[k].out_off + r->rel;
}

int lvlip_lro_cpu(const void *base, const lvlip_frame_desc *fd, uint32_t n, const lvlip_lro_flow *f,
                  uint32_t nflows, uint32_t flags, void *out, lvlip_lro_rec *rec)
{
    if (n == 0) return LVLIP_OK;
    if (!base || !fd || !out || !rec || (nflows && !f)) return LVLIP_EINVAL;
    if (n > LVLIP_MAX_BATCH || nflows > LVLIP_LRO_MAX_FLOWS || (flags & ~LVLIP_RX_VERIFY_L4)) return LVLIP_EINVAL;
    for (uint32_t k = 1; k < nflows; k++)
        if (key_cmp(&f[k - 1u], &f[k]) >= 0) return LVLIP_EINVAL; /* not as the plan left them */
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t *src = NULL;
        uint64_t dst = 0;
        lro_one((const uint8_t *)base + fd[i].offset, fd[i].len, f, nflows, flags, &rec[i], &src, &dst);
        if (rec[i].status == LVLIP_LRO_PLACED) memcpy((uint8_t *)out + dst, src, rec[i].dlen);
    }
    return LVLIP_OK;
}

/* --------------------------------------------------------------- advance -- */

/* an interval of a flow's union; bit 63 of hi marks a carried block, which
 * `placed` does not count */
#define IVAL_CARRIED (1ull << 63)

typedef struct ival {
    uint32_t flow, lo;
    uint64_t hi;
} ival;

static int ival_cmp(const void *a, const void *b)
{
    const ival *x = a, *y = b;
    if (x->flow != y->flow) return x->flow < y->flow ? -1 : 1;
    if (x->lo != y->lo) return x->lo < y->lo ? -1 : 1;
    return x->hi < y->hi ? -1 : x->hi > y->hi;
}

/* "Carried blocks" (include/lvlip_skb.h): block j of prev counts for flow f
 * when l < r <= rcv_wnd, both taken from f's rcv_nxt mod 2^32 */
static inline int carried_block(const lvlip_lro_flow *f, const lvlip_lro_result *prev, uint32_t j, uint32_t *l,
                                uint32_t *r)
{
    if (j >= prev->nsack) return 0;
    *l = prev->sack[j].left - f->rcv_nxt;
    *r = prev->sack[j].right - f->rcv_nxt;
    return *l < *r && *r <= f->rcv_wnd;
}

/* lvlip_lro_advance (prev NULL) and lvlip_lro_advance_carry.  prev may be res:
 * every interval is taken before res is zeroed. */
static int advance(const lvlip_lro_flow *f, uint32_t nflows, const lvlip_lro_rec *rec, uint32_t n,
                   const lvlip_lro_result *prev, lvlip_lro_result *res)
{
    if ((nflows && (!f || !res)) || (n && !rec)) return LVLIP_EINVAL;
    size_t m = 0;
    uint32_t l, r;
    for (uint32_t i = 0; i < n; i++) m += rec[i].status == LVLIP_LRO_PLACED && rec[i].flow < nflows;
    for (uint32_t k = 0; prev && k < nflows; k++)
        for (uint32_t j = 0; j < 4u; j++) m += (size_t)carried_block(&f[k], &prev[k], j, &l, &r);
    ival *v = NULL;
    if (m) {
        v = malloc(m * sizeof *v);
        if (!v) return LVLIP_ENOMEM;
    }
    m = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (rec[i].status != LVLIP_LRO_PLACED || rec[i].flow >= nflows) continue;
        v[m].flow = rec[i].flow;
        v[m].lo = rec[i].rel;
        v[m].hi = (uint64_t)rec[i].rel + rec[i].dlen;
        m++;
    }
    for (uint32_t k = 0; prev && k < nflows; k++)
        for (uint32_t j = 0; j < 4u; j++) {
            if (!carried_block(&f[k], &prev[k], j, &l, &r)) continue;
            v[m].flow = k;
            v[m].lo = l;
            v[m].hi = r | IVAL_CARRIED;
            m++;
        }
    if (nflows) memset(res, 0, (size_t)nflows * sizeof *res);
    if (m == 0) return LVLIP_OK;
    qsort(v, m, sizeof *v, ival_cmp);
    for (size_t a = 0; a < m;) {
        lvlip_lro_result *o = &res[v[a].flow];
        const uint32_t rcv_nxt = f[v[a].flow].rcv_nxt;
        size_t b = a;
        while (b < m && v[b].flow == v[a].flow) {
            /* one island: everything that touches or overlaps [lo, hi) */
            const uint64_t lo = v[b].lo;
            uint64_t hi = v[b].hi & ~IVAL_CARRIED;
            o->placed += !(v[b].hi & IVAL_CARRIED);
            for (b++; b < m && v[b].flow == v[a].flow && v[b].lo <= hi; b++) {
                if ((v[b].hi & ~IVAL_CARRIED) > hi) hi = v[b].hi & ~IVAL_CARRIED;
                o->placed += !(v[b].hi & IVAL_CARRIED);
            }
            if (lo == 0) {
                o->delivered = (uint32_t)hi; /* <= rcv_wnd <= 2^30 */
            } else if (o->nsack < 4u) {
                o->sack[o->nsack].left = rcv_nxt + (uint32_t)lo;
                o->sack[o->nsack].right = rcv_nxt + (uint32_t)hi;
                o->nsack++;
            }
        }
        a = b;
    }
    free(v);
    return LVLIP_OK;
}

int lvlip_lro_advance(const lvlip_lro_flow *f, uint32_t nflows, const lvlip_lro_rec *rec, uint32_t n,
                      lvlip_lro_result *res)
{
    return advance(f, nflows, rec, n, NULL, res);
}

int lvlip_lro_advance_carry(const lvlip_lro_flow *f, uint32_t nflows, const lvlip_lro_rec *rec, uint32_t n,
                            const lvlip_lro_result *prev, lvlip_lro_result *res)
{
    return advance(f, nflows, rec, n, prev, res);
}

/* ------------------------------------------------------------------ next -- */

int lvlip_lro_next_cpu(lvlip_lro_flow *f, lvlip_lro_result *res, uint32_t nflows)
{
    if (nflows == 0) return LVLIP_OK;
    if (!f || !res || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nflows; k++) {
        const uint32_t d = res[k].delivered < f[k].rcv_wnd ? res[k].delivered : f[k].rcv_wnd;
        f[k].rcv_nxt += d;
        f[k].out_off += d;
        f[k].rcv_wnd -= d;
        res[k].delivered = 0;
    }
    return LVLIP_OK;
}
