/*
 * seg_cpu.c — TCP segmentation from a header template (include/lvlip_skb.h,
 * "f2 on the device: segmentation"): the plan, and the frames on the calling
 * thread.  The device form (seg_kernels.hip) writes the same bytes.
 *
 * What tcp_send does per segment (src/tcp_output.c:445-478 ->
 * tcp_transmit_skb, src/tcp_output.c:93-129 -> ip_output,
 * src/ip_output.c:14-56), with the template standing for the socket's state.
 */
#include "tcp_hdr.h"

#define TSO_HDR TCP_FRAME_HDR
#define TSO_MSS_MAX TCP_MSS_MAX

static int send_ok(const lvlip_tso_send *s)
{
    if (s->len == 0 || s->mss == 0 || s->mss > TSO_MSS_MAX || s->reserved != 0) return 0;
    if (s->stride < TSO_HDR + s->mss) return 0;
    return tcp_tmpl_ok(s->hdr);
}

static inline uint64_t send_segs(const lvlip_tso_send *s)
{
    return ((uint64_t)s->len + s->mss - 1u) / s->mss;
}

/* total segments, or 0xFFFFFFFF; with `planned`, seg0 must already be the
 * running count */
static uint32_t walk(const lvlip_tso_send *s, uint32_t n, int planned, uint64_t *out_bytes)
{
    uint64_t total = 0, top = 0;
    for (uint32_t j = 0; j < n; j++) {
        if (!send_ok(&s[j])) return 0xFFFFFFFFu;
        if (planned && s[j].seg0 != total) return 0xFFFFFFFFu;
        const uint64_t k = send_segs(&s[j]);
        const uint64_t dlast = s[j].len - (k - 1u) * s[j].mss;
        const uint64_t end = s[j].out_off + (k - 1u) * s[j].stride + TSO_HDR + dlast;
        if (end > top) top = end;
        total += k;
        if (total > LVLIP_MAX_BATCH) return 0xFFFFFFFFu;
    }
    if (out_bytes) *out_bytes = top;
    return (uint32_t)total;
}

uint32_t lvlip_tso_plan(lvlip_tso_send *s, uint32_t n, uint64_t *out_bytes)
{
    if (out_bytes) *out_bytes = 0;
    if (n == 0) return 0;
    if (!s) return 0xFFFFFFFFu;
    const uint32_t total = walk(s, n, 0, out_bytes);
    if (total == 0xFFFFFFFFu) {
        if (out_bytes) *out_bytes = 0;
        return total;
    }
    uint64_t run = 0;
    for (uint32_t j = 0; j < n; j++) {
        s[j].seg0 = (uint32_t)run;
        run += send_segs(&s[j]);
    }
    return total;
}

int lvlip_tso_cpu(const void *payload, const lvlip_tso_send *s, uint32_t n, void *out,
                  lvlip_frame_desc *fd)
{
    if (n == 0) return LVLIP_OK;
    if (!payload || !s || !out) return LVLIP_EINVAL;
    if (walk(s, n, 1, NULL) == 0xFFFFFFFFu) return LVLIP_EINVAL;
    for (uint32_t j = 0; j < n; j++) {
        const lvlip_tso_send *t = &s[j];
        const uint8_t *src = (const uint8_t *)payload + t->payload_off;
        const uint32_t seq0 = be32(t->hdr + 38);
        const uint64_t k = send_segs(t);
        for (uint64_t i = 0; i < k; i++) {
            const uint64_t done = i * t->mss;
            const uint32_t dlen = t->len - done < t->mss ? (uint32_t)(t->len - done) : t->mss;
            const uint64_t off = t->out_off + i * t->stride;
            /* PSH on the last segment only (src/tcp_output.c:466), and FIN with it */
            tcp_seg_write((uint8_t *)out + off, t->hdr, src + done, dlen, seq0 + (uint32_t)done, i + 1u == k);
            if (fd) {
                lvlip_frame_desc *d = &fd[t->seg0 + i];
                d->offset = off;
                d->len = TSO_HDR + dlen;
                d->reserved = 0;
            }
        }
    }
    return LVLIP_OK;
}
