/*
 * lro_stream.c — INTEGRATION.md §2e as a plain C program: the receive loop on
 * the CPU forms of include/lvlip_skb.h.
 *
 * For every MSS of the list a payload is cut into frames by lvlip_tso_plan /
 * lvlip_tso_cpu (the sender), the frame descriptors are shuffled and some are
 * listed twice (the network), and lvlip_lro_plan / lvlip_lro_cpu /
 * lvlip_lro_advance put the byte stream back together (the receiver), with
 * LVLIP_RX_VERIFY_L4 and without.  The stream buffer is malloc'd at exactly
 * the planned size, so a sanitizer build (the CPU tests compile this file
 * with the library's C sources under -fsanitize=address,undefined) sees any
 * byte read or written outside it.  Then one segment is withheld: the prefix
 * stops in front of it and one SACK block covers the rest.
 *
 *   make -C examples && examples/build/lro_stream
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lvlip_csum.h"
#include "lvlip_skb.h"

#define CANARY 0xA5
#define RCV_NXT 0xFFFFFF00u /* the stream crosses the sequence wrap */

static const uint16_t MSS[] = {1, 15, 16, 17, 536, 1460, 8946};

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

static const uint8_t HDR[54] = {
    0x00, 0x0c, 0x29, 0x6d, 0x50, 0x25, 0x0a, 0x1b, 0x2c, 0x3d, 0x4e, 0x5f, 0x08, 0x00, /* eth */
    0x45, 0x00, 0x00, 0x00, 0x12, 0x34, 0x40, 0x00, 0x40, 0x06, 0x00, 0x00,             /* ip  */
    10, 0, 0, 5, 10, 0, 0, 4,                                                           /* peer -> stack */
    0x9c, 0x41, 0x1f, 0x40, 0xff, 0xff, 0xff, 0x00, 0x01, 0x02, 0x03, 0x04,             /* tcp: seq = RCV_NXT */
    0x50, 0x18, 0xad, 0xbd, 0x00, 0x00, 0x00, 0x00};                                    /* ACK|PSH */

static uint32_t rnd(uint32_t *s) { return *s = *s * 1664525u + 1013904223u; }

static void one_mss(uint16_t mss, uint32_t flags)
{
    const uint32_t len = mss < 32 ? 20u * mss + 3u : 5u * mss + 3u;
    uint32_t seed = mss;
    uint8_t *payload = malloc(len);
    for (uint32_t i = 0; i < len; i++) payload[i] = (uint8_t)(rnd(&seed) >> 24);

    /* the sender: frames 3 bytes apart, the first at an odd offset */
    lvlip_tso_send s;
    memset(&s, 0, sizeof s);
    s.len = len, s.mss = mss, s.stride = 54u + mss + 3u, s.out_off = 5;
    memcpy(s.hdr, HDR, 54);
    uint64_t ring_bytes = 0;
    const uint32_t nseg = lvlip_tso_plan(&s, 1, &ring_bytes);
    CHECK(nseg != 0xFFFFFFFFu, "mss %u: tso plan", mss);
    uint8_t *ring = malloc(ring_bytes);
    lvlip_frame_desc *fd = malloc((size_t)(2u * nseg) * sizeof *fd);
    CHECK(lvlip_tso_cpu(payload, &s, 1, ring, fd) == LVLIP_OK, "mss %u: tso", mss);

    /* the network: shuffled, every third frame twice */
    uint32_t n = nseg;
    for (uint32_t i = 0; i < nseg; i += 3) fd[n++] = fd[i];
    for (uint32_t i = n - 1; i > 0; i--) {
        const uint32_t j = rnd(&seed) % (i + 1u);
        const lvlip_frame_desc t = fd[i];
        fd[i] = fd[j], fd[j] = t;
    }

    /* the receiver: one flow that owns exactly `len` bytes at offset 7 */
    lvlip_lro_flow f;
    memset(&f, 0, sizeof f);
    memcpy(&f.saddr, HDR + 26, 4), memcpy(&f.daddr, HDR + 30, 4);
    memcpy(&f.sport, HDR + 34, 2), memcpy(&f.dport, HDR + 36, 2);
    f.rcv_nxt = RCV_NXT, f.rcv_wnd = len, f.out_off = 7, f.user = 42;
    uint64_t out_bytes = 0;
    CHECK(lvlip_lro_plan(&f, 1, &out_bytes) == 1 && out_bytes == 7u + len, "mss %u: lro plan", mss);
    uint8_t *out = malloc(out_bytes);
    memset(out, CANARY, out_bytes);
    lvlip_lro_rec *rec = malloc((size_t)n * sizeof *rec);
    lvlip_lro_result res;
    CHECK(lvlip_lro_cpu(ring, fd, n, &f, 1, flags, out, rec) == LVLIP_OK, "mss %u: lro", mss);
    CHECK(lvlip_lro_advance(&f, 1, rec, n, &res) == LVLIP_OK, "mss %u: advance", mss);
    for (uint32_t i = 0; i < n; i++)
        CHECK(rec[i].status == LVLIP_LRO_PLACED && rec[i].flow == 0 && rec[i].ack_seq == 0x01020304u,
              "mss %u frame %u: status %u", mss, i, rec[i].status);
    CHECK(res.delivered == len && res.placed == n && res.nsack == 0, "mss %u: delivered %u of %u", mss,
          res.delivered, len);
    CHECK(memcmp(out + 7, payload, len) == 0, "mss %u: the stream is not the payload", mss);
    for (uint32_t i = 0; i < 7; i++) CHECK(out[i] == CANARY, "mss %u: byte %u in front of the stream", mss, i);

    /* the same with segment 1 lost (when there is one beyond it) */
    if (nseg >= 3) {
        uint32_t m = 0;
        for (uint32_t i = 0; i < n; i++)
            if (fd[i].offset != s.out_off + s.stride) fd[m++] = fd[i];
        memset(out, CANARY, out_bytes);
        CHECK(lvlip_lro_cpu(ring, fd, m, &f, 1, flags, out, rec) == LVLIP_OK, "mss %u: lro with a hole", mss);
        CHECK(lvlip_lro_advance(&f, 1, rec, m, &res) == LVLIP_OK, "mss %u: advance with a hole", mss);
        CHECK(res.delivered == mss && res.nsack == 1 && res.sack[0].left == RCV_NXT + 2u * mss &&
                  res.sack[0].right == RCV_NXT + len,
              "mss %u: hole: delivered %u, %u blocks", mss, res.delivered, res.nsack);
        for (uint32_t i = 0; i < mss; i++) CHECK(out[7u + mss + i] == CANARY, "mss %u: the hole was written", mss);
    }

    /* a frame for nobody, and flows the plan refuses */
    f.sport ^= 0x0100;
    CHECK(lvlip_lro_cpu(ring, fd, 1, &f, 1, flags, out, rec) == LVLIP_OK && rec[0].status == LVLIP_LRO_NO_FLOW,
          "mss %u: a frame of another port", mss);
    lvlip_lro_flow two[2] = {f, f};
    CHECK(lvlip_lro_plan(two, 2, NULL) == 0xFFFFFFFFu, "a duplicate key must be refused");
    two[1].dport ^= 1;
    CHECK(lvlip_lro_plan(two, 2, NULL) == 0xFFFFFFFFu, "overlapping ranges must be refused");
    two[1].out_off = f.out_off + f.rcv_wnd;
    CHECK(lvlip_lro_plan(two, 2, &out_bytes) == 2 && out_bytes == 7u + 2u * (uint64_t)len, "two flows side by side");

    free(rec), free(out), free(fd), free(ring), free(payload);
}

int main(void)
{
    for (size_t k = 0; k < sizeof MSS / sizeof MSS[0]; k++) {
        one_mss(MSS[k], 0);
        one_mss(MSS[k], LVLIP_RX_VERIFY_L4);
    }
    if (fails) {
        fprintf(stderr, "lro_stream: %d checks failed\n", fails);
        return 1;
    }
    printf("lro_stream ok: %zu MSS values, shuffled and duplicated frames back into their streams\n",
           sizeof MSS / sizeof MSS[0]);
    return 0;
}
