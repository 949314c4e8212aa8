/*
 * tcp_hdr.h — what the CPU forms of the device-resident TCP path (seg_cpu.c,
 * rcv_cpu.c, ack_cpu.c, snd_cpu.c, sack_cpu.c) share: the byte helpers, the
 * test a 54-byte header template has to pass, the two checksum fields as
 * ip_output and tcp_transmit_skb leave them, the plans' overlap check, which
 * records carry an ACK and which queue entries a retransmit can rewrite.  tcp_hdr_dev.h is
 * the same arithmetic on the device.  Not installed; static inline only, so a
 * file that uses part of it compiles without a warning.
 */
#ifndef LVLIP_TCP_HDR_H
#define LVLIP_TCP_HDR_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "lvlip_skb.h"

#define TCP_FRAME_HDR 54u /* Ethernet 14 + IPv4 20 + TCP 20 */

static inline uint32_t le32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

static inline uint32_t be32(const uint8_t *p)
{
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

static inline void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

static inline uint16_t bswap16(uint16_t x) { return (uint16_t)((x << 8) | (x >> 8)); }

/* the 54 bytes at h are a template frames can be built from */
static inline int tcp_tmpl_ok(const uint8_t *h)
{
    if (h[12] != 0x08 || h[13] != 0x00) return 0; /* ethertype IPv4 */
    if (h[14] != 0x45) return 0;                  /* version 4, ihl 5 */
    if (h[23] != 6) return 0;                     /* IP_TCP */
    if ((h[46] >> 4) != 5) return 0;              /* TCP header length, no options */
    return 1;
}

/* ip_output on the IPv4 header at ih: len, csum 0, then ip_send_check
 * (src/ip_output.c:35,42,53) */
static inline void ip_output_tail(uint8_t *ih, uint32_t iplen)
{
    ih[2] = (uint8_t)(iplen >> 8);
    ih[3] = (uint8_t)iplen;
    ih[10] = ih[11] = 0;
    const uint16_t ic = checksum(ih, 20, 0);
    memcpy(ih + 10, &ic, 2);
}

/* tcp_transmit_skb's last step on the l4 bytes at th behind the IPv4 header at
 * ih: csum 0, then tcp_v4_checksum (src/tcp_output.c:110,126).  The pseudo
 * header is added as src/tcp.c:92-95 adds it: u32 adds, the carry out of bit
 * 31 is lost; checksum() folds once, on (seed + the segment's words) mod 2^32. */
static inline void tcp_csum_tail(const uint8_t *ih, uint8_t *th, uint32_t l4)
{
    th[16] = th[17] = 0;
    const uint32_t seed = le32(ih + 12) + le32(ih + 16) + bswap16(6) + bswap16((uint16_t)l4);
    const uint16_t tc = checksum(th, (int)l4, (int)seed);
    memcpy(th + 16, &tc, 2);
}

#define TCP_MSS_MAX 65495u /* 65535 - 40: the IPv4 total length is 16 bits */
#define TCP_FIN_PSH 0x09u  /* byte 13 of the TCP header: FIN 0x01, PSH 0x08 */

/* One segment of tcp_send at f (src/tcp_output.c:445-478 -> tcp_transmit_skb,
 * :93-129 -> ip_output, src/ip_output.c:14-56): the template's 54 bytes, dlen
 * payload bytes from src, the IP length and checksum, seq (:106), PSH and FIN
 * on the last segment only (:466), the TCP checksum.  The one frame writer of
 * lvlip_tso_cpu and lvlip_push_cpu. */
static inline void tcp_seg_write(uint8_t *f, const uint8_t *hdr, const uint8_t *src, uint32_t dlen, uint32_t seq,
                                 int last)
{
    uint8_t *ih = f + 14, *th = f + 34;
    memcpy(f, hdr, TCP_FRAME_HDR);
    memcpy(f + TCP_FRAME_HDR, src, dlen);
    ip_output_tail(ih, 40u + dlen);
    put_be32(th + 4, seq);
    if (!last) th[13] &= (uint8_t)~TCP_FIN_PSH;
    tcp_csum_tail(ih, th, 20u + dlen);
}

static inline int range_cmp(const void *a, const void *b)
{
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : x > y;
}

/* r holds n non-empty ranges as (start, end) pairs; they are sorted by start
 * in place.  1 when each ends before the next begins: no two share an element. */
static inline int ranges_disjoint(uint64_t *r, size_t n)
{
    qsort(r, n, 2u * sizeof *r, range_cmp);
    for (size_t k = 1; k < n; k++)
        if (r[2u * k - 1u] > r[2u * k]) return 0;
    return 1;
}

/* "Which records carry an ACK" (include/lvlip_skb.h): the record's flow when it
 * counts for lvlip_snd_* and lvlip_sack_*, else 0xFFFFFFFF.  First check,
 * src/tcp_input.c:106-107, on the segment's start; fifth check, :312. */
static inline uint32_t rec_ack_flow(const lvlip_lro_rec *r, const lvlip_lro_flow *f, uint32_t nflows)
{
    if (r->flow >= nflows) return 0xFFFFFFFFu;
    if (r->status != LVLIP_LRO_PLACED && r->status != LVLIP_LRO_NO_DATA && r->status != LVLIP_LRO_OUT_OF_WINDOW)
        return 0xFFFFFFFFu;
    if (!(r->tcp_flags & 0x10u) || r->rel > f[r->flow].rcv_wnd) return 0xFFFFFFFFu;
    return r->flow;
}

/* The refusals of lvlip_rtx_*: the len bytes at p are a frame a retransmit can
 * rewrite.  *iplen and *hl get the IP length and the TCP header's words. */
static inline int rtx_frame_ok(const uint8_t *p, uint32_t len, uint32_t *iplen, uint32_t *hl)
{
    if (len < TCP_FRAME_HDR) return 0;
    *iplen = ((uint32_t)p[16] << 8) | p[17];
    *hl = p[46] >> 4;
    return p[14] == 0x45 && 14u + *iplen <= len && *hl >= 5u && 20u + 4u * *hl <= *iplen;
}

#endif
