/*
 * ack_loop.c — INTEGRATION.md §2e with its last step, as a plain C program:
 * the receive loop on the CPU forms of include/lvlip_skb.h, up to the ACK
 * frame that goes back to the peer.
 *
 * A payload is cut into 536-byte frames by lvlip_tso_plan / lvlip_tso_cpu (the
 * sender), some frames are withheld and the rest shuffled (the network),
 * lvlip_lro_plan / lvlip_lro_cpu / lvlip_lro_advance put the stream back
 * together (the receiver), and lvlip_ack_plan / lvlip_ack_cpu build the
 * acknowledgement: ack_seq at the end of the prefix, the first four of five
 * islands as SACK blocks, last block first.  Every buffer is malloc'd at
 * exactly its planned size, so a sanitizer build (the CPU tests compile this
 * file with the library's C sources under -fsanitize=address,undefined) sees
 * any byte read or written outside it.
 *
 *   make -C examples && examples/build/ack_loop
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lvlip_csum.h"
#include "lvlip_skb.h"

#define CANARY 0xA5
#define MSS 536u
#define NSEG 14u
#define RCV_NXT 0xFFFFF000u /* the stream crosses the sequence wrap */
#define ACK_OFF 7u          /* the ACK slot: an odd offset */

static int fails;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            if (fails++ < 20) {                        \
                fprintf(stderr, "FAIL: " __VA_ARGS__); \
                fputc('\n', stderr);                   \
            }                                          \
        }                                              \
    } while (0)

/* peer -> stack: the data segments */
static const uint8_t DATA_HDR[54] = {
    0x00, 0x0c, 0x29, 0x6d, 0x50, 0x25, 0x0a, 0x1b, 0x2c, 0x3d, 0x4e, 0x5f, 0x08, 0x00, /* eth */
    0x45, 0x00, 0x00, 0x00, 0x12, 0x34, 0x40, 0x00, 0x40, 0x06, 0x00, 0x00,             /* ip  */
    10, 0, 0, 5, 10, 0, 0, 4,                                                           /* peer -> stack */
    0x1f, 0x40, 0x9c, 0x41, 0xff, 0xff, 0xf0, 0x00, 0x01, 0x02, 0x03, 0x04,             /* tcp: seq = RCV_NXT */
    0x50, 0x18, 0xad, 0xbd, 0x00, 0x00, 0x00, 0x00};                                    /* ACK|PSH */

/* stack -> peer: the stack's own pure ACK (seq = snd_nxt = the peer's ack_seq) */
static const uint8_t ACK_HDR[54] = {
    0x0a, 0x1b, 0x2c, 0x3d, 0x4e, 0x5f, 0x00, 0x0c, 0x29, 0x6d, 0x50, 0x25, 0x08, 0x00, /* eth */
    0x45, 0x00, 0x00, 0x28, 0x00, 0x00, 0x40, 0x00, 0x40, 0x06, 0x00, 0x00,             /* ip  */
    10, 0, 0, 4, 10, 0, 0, 5,                                                           /* stack -> peer */
    0x9c, 0x41, 0x1f, 0x40, 0x01, 0x02, 0x03, 0x04, 0x00, 0x00, 0x00, 0x00,             /* tcp */
    0x50, 0x10, 0xad, 0xbd, 0x00, 0x00, 0x00, 0x00};                                    /* ACK */

static const uint8_t LOST[] = {2, 5, 7, 9, 11}; /* islands 3-4, 6, 8, 10, 12-13 behind the prefix 0-1 */

static uint32_t rnd(uint32_t *s) { return *s = *s * 1664525u + 1013904223u; }

static uint32_t be32(const uint8_t *p)
{
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

static int lost(uint32_t seg)
{
    for (size_t k = 0; k < sizeof LOST; k++)
        if (LOST[k] == seg) return 1;
    return 0;
}

/* both checksums of a frame the library built, verified the way a receiver
 * does: summing over the stored field gives 0 */
static int sums_ok(const uint8_t *fr, uint32_t len)
{
    uint32_t s, d;
    memcpy(&s, fr + 26, 4), memcpy(&d, fr + 30, 4);
    const uint32_t l4 = len - 34u;
    const uint32_t seed = s + d + 0x0600u + (((l4 & 0xffu) << 8) | (l4 >> 8));
    return checksum((void *)(fr + 14), 20, 0) == 0 && checksum((void *)(fr + 34), (int)l4, (int)seed) == 0;
}

int main(void)
{
    const uint32_t len = NSEG * MSS;
    uint32_t seed = 1;
    uint8_t *payload = malloc(len);
    for (uint32_t i = 0; i < len; i++) payload[i] = (uint8_t)(rnd(&seed) >> 24);

    /* the sender */
    lvlip_tso_send s;
    memset(&s, 0, sizeof s);
    s.len = len, s.mss = MSS, s.stride = 54u + MSS + 3u, s.out_off = 5;
    memcpy(s.hdr, DATA_HDR, 54);
    uint64_t ring_bytes = 0;
    const uint32_t nseg = lvlip_tso_plan(&s, 1, &ring_bytes);
    CHECK(nseg == NSEG, "tso plan: %u segments", nseg);
    uint8_t *ring = malloc(ring_bytes);
    lvlip_frame_desc *fd = malloc((size_t)nseg * sizeof *fd);
    CHECK(lvlip_tso_cpu(payload, &s, 1, ring, fd) == LVLIP_OK, "tso");

    /* the network: five segments lost, the rest shuffled */
    uint32_t n = 0;
    for (uint32_t i = 0; i < nseg; i++)
        if (!lost(i)) fd[n++] = fd[i];
    for (uint32_t i = n - 1; i > 0; i--) {
        const uint32_t j = rnd(&seed) % (i + 1u);
        const lvlip_frame_desc t = fd[i];
        fd[i] = fd[j], fd[j] = t;
    }

    /* the receiver: one flow that owns exactly `len` stream bytes */
    lvlip_lro_flow f;
    memset(&f, 0, sizeof f);
    memcpy(&f.saddr, DATA_HDR + 26, 4), memcpy(&f.daddr, DATA_HDR + 30, 4);
    memcpy(&f.sport, DATA_HDR + 34, 2), memcpy(&f.dport, DATA_HDR + 36, 2);
    f.rcv_nxt = RCV_NXT, f.rcv_wnd = len, f.out_off = 0;
    uint64_t stream_bytes = 0;
    CHECK(lvlip_lro_plan(&f, 1, &stream_bytes) == 1 && stream_bytes == len, "lro plan");
    uint8_t *stream = malloc(stream_bytes);
    memset(stream, CANARY, stream_bytes);
    lvlip_lro_rec *rec = malloc((size_t)n * sizeof *rec);
    lvlip_lro_result res;
    CHECK(lvlip_lro_cpu(ring, fd, n, &f, 1, LVLIP_RX_VERIFY_L4, stream, rec) == LVLIP_OK, "lro");
    CHECK(lvlip_lro_advance(&f, 1, rec, n, &res) == LVLIP_OK, "advance");
    CHECK(res.delivered == 2u * MSS && res.placed == n && res.nsack == 4, "advance: delivered %u, %u blocks",
          res.delivered, res.nsack);
    CHECK(memcmp(stream, payload, 2u * MSS) == 0, "the prefix is not the payload");

    /* the acknowledgement */
    lvlip_ack_tmpl t;
    memset(&t, 0, sizeof t);
    t.out_off = ACK_OFF, t.max_sack = 4;
    memcpy(t.hdr, ACK_HDR, 54);
    uint64_t ack_bytes = 0;
    CHECK(lvlip_ack_plan(&t, &f, 1, &ack_bytes) == 1 && ack_bytes == ACK_OFF + LVLIP_ACK_MAX_FRAME, "ack plan");
    uint8_t *ack = malloc(ack_bytes);
    memset(ack, CANARY, ack_bytes);
    lvlip_frame_desc afd;
    CHECK(lvlip_ack_cpu(&t, &f, &res, 1, 0, ack, &afd) == LVLIP_OK, "ack");
    const uint8_t *fr = ack + ACK_OFF;
    CHECK(afd.offset == ACK_OFF && afd.len == 90 && afd.reserved == 0, "ack: fd {%llu, %u}",
          (unsigned long long)afd.offset, afd.len);
    CHECK(be32(fr + 42) == RCV_NXT + 2u * MSS, "ack_seq %08x", be32(fr + 42));
    CHECK(be32(fr + 38) == 0x01020304u && fr[47] == 0x10 && (fr[46] >> 4) == 14, "seq, flags or data offset");
    CHECK(fr[16] == 0 && fr[17] == 76, "ip length %u", fr[17]);
    CHECK(fr[54] == 1 && fr[55] == 1 && fr[56] == 5 && fr[57] == 34, "the option's head");
    static const uint8_t ISL[4][2] = {{3, 5}, {6, 7}, {8, 9}, {10, 11}}; /* 12-13 is the fifth: cut */
    for (uint32_t i = 0; i < 4; i++) {
        const uint8_t *b = fr + 58 + 8u * i; /* position i holds block 3 - i */
        CHECK(be32(b) == RCV_NXT + ISL[3 - i][0] * MSS && be32(b + 4) == RCV_NXT + ISL[3 - i][1] * MSS,
              "block at position %u: %08x-%08x", i, be32(b), be32(b + 4));
        CHECK(res.sack[3 - i].left == be32(b) && res.sack[3 - i].right == be32(b + 4), "not descending");
    }
    CHECK(sums_ok(fr, afd.len), "a checksum of the ACK does not verify");
    for (uint32_t i = 0; i < ACK_OFF; i++) CHECK(ack[i] == CANARY, "byte %u in front of the ACK", i);

    /* SACK not negotiated: 54 bytes, the rest of the slot keeps its bytes */
    t.max_sack = 0;
    memset(ack, CANARY, ack_bytes);
    CHECK(lvlip_ack_cpu(&t, &f, &res, 1, 0, ack, &afd) == LVLIP_OK && afd.len == 54, "ack without SACK");
    CHECK((fr[46] >> 4) == 5 && fr[17] == 40 && be32(fr + 42) == RCV_NXT + 2u * MSS && sums_ok(fr, 54),
          "the plain ACK");
    for (uint32_t i = ACK_OFF + 54u; i < ack_bytes; i++) CHECK(ack[i] == CANARY, "byte %u behind the plain ACK", i);

    /* nothing placed: no ACK unless asked for */
    lvlip_lro_result idle;
    memset(&idle, 0, sizeof idle);
    memset(ack, CANARY, ack_bytes);
    CHECK(lvlip_ack_cpu(&t, &f, &idle, 1, 0, ack, &afd) == LVLIP_OK && afd.len == 0 && afd.offset == ACK_OFF,
          "an idle flow");
    for (uint32_t i = 0; i < ack_bytes; i++) CHECK(ack[i] == CANARY, "byte %u written for an idle flow", i);
    CHECK(lvlip_ack_cpu(&t, &f, &idle, 1, LVLIP_ACK_ALL, ack, NULL) == LVLIP_OK && be32(fr + 42) == RCV_NXT &&
              sums_ok(fr, 54),
          "LVLIP_ACK_ALL");

    /* templates the plan refuses */
    lvlip_ack_tmpl bad = t;
    memcpy(bad.hdr, DATA_HDR, 54); /* the peer's direction, not the reverse of the flow */
    CHECK(lvlip_ack_plan(&bad, &f, 1, NULL) == 0xFFFFFFFFu, "a template in the flow's own direction");
    bad = t, bad.max_sack = 5;
    CHECK(lvlip_ack_plan(&bad, &f, 1, NULL) == 0xFFFFFFFFu, "max_sack 5");

    free(ack), free(rec), free(stream), free(fd), free(ring), free(payload);
    if (fails) {
        fprintf(stderr, "ack_loop: %d checks failed\n", fails);
        return 1;
    }
    printf("ack_loop ok: %u of %u segments coalesced, ACK %08x with 4 of 5 islands as SACK blocks\n", n, nseg,
           RCV_NXT + 2u * MSS);
    return 0;
}
