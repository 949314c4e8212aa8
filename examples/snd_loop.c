/*
 * snd_loop.c — INTEGRATION.md §2f as a plain C program: a whole transfer with
 * loss and recovery on the CPU forms of include/lvlip_skb.h.
 *
 * Side A sends: lvlip_tso_plan / lvlip_tso_cpu cut three connections' payloads
 * into frames in a TX ring, which is then each connection's write queue.  The
 * network drops every fifth frame and shuffles the rest.  Side B receives:
 * lvlip_lro_cpu places the payload, lvlip_lro_advance finds the prefix and the
 * islands over all records so far, lvlip_ack_cpu builds one ACK per
 * connection.  Back on side A a SECOND lvlip_lro_* plan, for the reverse
 * direction, parses those ACK frames into records; lvlip_snd_cpu reads their
 * ack_seq (snd_una, the frames popped from the queue), and lvlip_rtx_cpu
 * rewrites the next RTX frames of every queue in place with the current
 * ack_seq, window and a fresh checksum.  Those go out again (the first of them
 * is lost once more), until every queue is empty and B's streams hold the
 * payloads.  Every buffer is malloc'd at exactly its planned size, so a
 * sanitizer build (the CPU tests compile this file with the library's C
 * sources under -fsanitize=address,undefined) sees any byte read or written
 * outside it.
 *
 *   make -C examples && examples/build/snd_loop
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lvlip_csum.h"
#include "lvlip_skb.h"

#define NF 3u
#define MSS 536u
#define RTX 3u          /* frames a retransmit sends from the head of a queue */
#define WIN 29200u      /* A's advertised window */
#define IRS 0x01020304u /* B's sequence number: what A acknowledges */
#define MAX_ROUNDS 40u

static const uint32_t LEN[NF] = {12u * MSS + 100u, 7u * MSS, 21u * MSS + 1u};
static const uint32_t ISS[NF] = {0xFFFFF000u, 0x7FFFFFF0u, 5u}; /* the first crosses the sequence wrap */

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

/* A -> B, connection k: source port 40000 + k */
static void hdr_a_to_b(uint8_t *h, uint32_t k, uint32_t seq, uint32_t ack, uint8_t flags)
{
    static const uint8_t H[54] = {
        0x00, 0x0c, 0x29, 0x6d, 0x50, 0x25, 0x0a, 0x1b, 0x2c, 0x3d, 0x4e, 0x5f, 0x08, 0x00, /* eth */
        0x45, 0x00, 0x00, 0x00, 0x12, 0x34, 0x40, 0x00, 0x40, 0x06, 0x00, 0x00,             /* ip  */
        10, 0, 0, 4, 10, 0, 0, 5,                                                           /* A -> B */
        0, 0, 0x1f, 0x40, 0, 0, 0, 0, 0, 0, 0, 0, 0x50, 0, 0x72, 0x10, 0, 0, 0, 0};         /* tcp */
    memcpy(h, H, 54);
    h[34] = (uint8_t)((40000u + k) >> 8), h[35] = (uint8_t)(40000u + k);
    h[38] = (uint8_t)(seq >> 24), h[39] = (uint8_t)(seq >> 16), h[40] = (uint8_t)(seq >> 8), h[41] = (uint8_t)seq;
    h[42] = (uint8_t)(ack >> 24), h[43] = (uint8_t)(ack >> 16), h[44] = (uint8_t)(ack >> 8), h[45] = (uint8_t)ack;
    h[47] = flags;
}

/* B -> A: the same with addresses and ports exchanged */
static void hdr_b_to_a(uint8_t *h, uint32_t k, uint32_t seq)
{
    uint8_t t[54];
    hdr_a_to_b(t, k, seq, 0, 0x10);
    memcpy(h, t, 54);
    memcpy(h, t + 6, 6), memcpy(h + 6, t, 6);
    memcpy(h + 26, t + 30, 4), memcpy(h + 30, t + 26, 4);
    memcpy(h + 34, t + 36, 2), memcpy(h + 36, t + 34, 2);
}

static uint32_t rnd(uint32_t *s) { return *s = *s * 1664525u + 1013904223u; }

static uint32_t be32(const uint8_t *p)
{
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

/* the TCP checksum of a frame the library built, verified the way a receiver
 * does: summing over the stored field gives 0 */
static int sum_ok(const uint8_t *fr, uint32_t len)
{
    uint32_t s, d;
    memcpy(&s, fr + 26, 4), memcpy(&d, fr + 30, 4);
    const uint32_t l4 = len - 34u;
    const uint32_t seed = s + d + 0x0600u + (((l4 & 0xffu) << 8) | (l4 >> 8));
    return checksum((void *)(fr + 34), (int)l4, (int)seed) == 0;
}

static void shuffle(lvlip_frame_desc *fd, uint32_t n, uint32_t *seed)
{
    for (uint32_t i = n; i-- > 1u;) {
        const uint32_t j = rnd(seed) % (i + 1u);
        const lvlip_frame_desc t = fd[i];
        fd[i] = fd[j], fd[j] = t;
    }
}

int main(void)
{
    uint32_t seed = 1, total = 0;
    for (uint32_t k = 0; k < NF; k++) total += LEN[k];
    uint8_t *payload = malloc(total);
    for (uint32_t i = 0; i < total; i++) payload[i] = (uint8_t)(rnd(&seed) >> 24);

    /* ---- side A: the frames, which are the write queues */
    lvlip_tso_send send[NF];
    memset(send, 0, sizeof send);
    uint64_t poff = 0, roff = 1;
    for (uint32_t k = 0; k < NF; k++) {
        send[k].payload_off = poff, send[k].out_off = roff, send[k].len = LEN[k], send[k].mss = MSS;
        send[k].stride = 54u + MSS + 1u + 2u * k;
        hdr_a_to_b(send[k].hdr, k, ISS[k], IRS, 0x18);
        poff += LEN[k];
        roff += (uint64_t)((LEN[k] + MSS - 1u) / MSS) * send[k].stride;
    }
    uint64_t ring_bytes = 0;
    const uint32_t nseg = lvlip_tso_plan(send, NF, &ring_bytes);
    CHECK(nseg != 0xFFFFFFFFu, "tso plan");
    uint8_t *ring = malloc(ring_bytes);
    lvlip_frame_desc *fd = malloc((size_t)nseg * sizeof *fd);
    CHECK(lvlip_tso_cpu(payload, send, NF, ring, fd) == LVLIP_OK, "tso");

    /* the reverse plan: B's ACKs as A receives them.  Both plans sort by
     * addresses and ports; ascending source ports keep index k on both sides */
    lvlip_lro_flow fa[NF], fb[NF];
    memset(fa, 0, sizeof fa), memset(fb, 0, sizeof fb);
    uint64_t soff = 0;
    for (uint32_t k = 0; k < NF; k++) {
        uint8_t h[54];
        hdr_a_to_b(h, k, 0, 0, 0);
        memcpy(&fb[k].saddr, h + 26, 4), memcpy(&fb[k].daddr, h + 30, 4);
        memcpy(&fb[k].sport, h + 34, 2), memcpy(&fb[k].dport, h + 36, 2);
        fb[k].rcv_nxt = ISS[k], fb[k].rcv_wnd = LEN[k], fb[k].out_off = soff, fb[k].user = k;
        soff += LEN[k];
        hdr_b_to_a(h, k, 0);
        memcpy(&fa[k].saddr, h + 26, 4), memcpy(&fa[k].daddr, h + 30, 4);
        memcpy(&fa[k].sport, h + 34, 2), memcpy(&fa[k].dport, h + 36, 2);
        fa[k].rcv_nxt = IRS, fa[k].rcv_wnd = 1, fa[k].out_off = k, fa[k].user = k;
    }
    uint64_t stream_bytes = 0, sink_bytes = 0;
    CHECK(lvlip_lro_plan(fb, NF, &stream_bytes) == NF && stream_bytes == total, "lro plan, forward");
    CHECK(lvlip_lro_plan(fa, NF, &sink_bytes) == NF && sink_bytes == NF, "lro plan, reverse");
    for (uint32_t k = 0; k < NF; k++) CHECK(fa[k].user == k && fb[k].user == k, "the plans reordered the flows");
    uint8_t *stream = malloc(stream_bytes), *sink = malloc(sink_bytes);
    memset(stream, 0xA5, stream_bytes);

    lvlip_snd_flow s[NF];
    memset(s, 0, sizeof s);
    for (uint32_t k = 0; k < NF; k++) {
        s[k].snd_una = ISS[k], s[k].snd_nxt = ISS[k] + LEN[k];
        s[k].seg0 = send[k].seg0, s[k].nseg = (LEN[k] + MSS - 1u) / MSS;
        s[k].rtx = RTX, s[k].win = WIN;
    }
    uint32_t nfd = 0;
    const uint32_t nslots = lvlip_snd_plan(s, NF, &nfd);
    CHECK(nslots == NF * RTX && nfd == nseg, "snd plan: %u slots, %u descriptors", nslots, nfd);
    lvlip_frame_desc *fd_out = malloc((size_t)nslots * sizeof *fd_out);

    /* ---- side B: the ACK templates */
    lvlip_ack_tmpl t[NF];
    memset(t, 0, sizeof t);
    for (uint32_t k = 0; k < NF; k++) {
        t[k].out_off = 3u + (uint64_t)k * (LVLIP_ACK_MAX_FRAME + 1u), t[k].max_sack = 4;
        hdr_b_to_a(t[k].hdr, k, IRS);
    }
    uint64_t ack_bytes = 0;
    CHECK(lvlip_ack_plan(t, fb, NF, &ack_bytes) == NF, "ack plan");
    uint8_t *ackbuf = malloc(ack_bytes);
    lvlip_frame_desc afd[NF];
    lvlip_lro_rec arec[NF];
    lvlip_lro_result resb[NF];
    lvlip_snd_result sres[NF];

    /* ---- the first flight: every fifth frame lost, the rest shuffled */
    lvlip_frame_desc *wire = malloc((size_t)nseg * sizeof *wire);
    uint32_t nwire = 0, lost = 0;
    for (uint32_t i = 0; i < nseg; i++) {
        if (i % 5u == 4u) lost++;
        else wire[nwire++] = fd[i];
    }
    shuffle(wire, nwire, &seed);

    lvlip_lro_rec *rec = NULL; /* every record B has had: the advance step sees the whole transfer */
    uint32_t nrec = 0, round = 0, resent = 0, acks = 0;
    for (;; round++) {
        CHECK(round < MAX_ROUNDS, "no progress");
        if (round >= MAX_ROUNDS) break;
        /* B: place, advance over all records so far, acknowledge */
        rec = realloc(rec, (size_t)(nrec + nwire) * sizeof *rec);
        CHECK(lvlip_lro_cpu(ring, wire, nwire, fb, NF, LVLIP_RX_VERIFY_L4, stream, rec + nrec) == LVLIP_OK, "lro");
        for (uint32_t i = 0; i < nwire; i++)
            CHECK(rec[nrec + i].status == LVLIP_LRO_PLACED, "round %u: frame %u has status %u", round, i,
                  rec[nrec + i].status);
        nrec += nwire;
        CHECK(lvlip_lro_advance(fb, NF, rec, nrec, resb) == LVLIP_OK, "advance");
        CHECK(lvlip_ack_cpu(t, fb, resb, NF, LVLIP_ACK_ALL, ackbuf, afd) == LVLIP_OK, "ack");

        /* A: the ACK frames through the reverse plan, then the ACK side */
        CHECK(lvlip_lro_cpu(ackbuf, afd, NF, fa, NF, LVLIP_RX_VERIFY_L4, sink, arec) == LVLIP_OK, "lro, reverse");
        for (uint32_t k = 0; k < NF; k++)
            CHECK(arec[k].status == LVLIP_LRO_NO_DATA && arec[k].flow == k &&
                      arec[k].ack_seq == ISS[k] + resb[k].delivered,
                  "round %u: ACK %u parsed as status %u, flow %u", round, k, arec[k].status, arec[k].flow);
        acks += NF;
        CHECK(lvlip_snd_cpu(fa, s, NF, arec, NF, ring, fd, sres) == LVLIP_OK, "snd");
        uint32_t left = 0;
        for (uint32_t k = 0; k < NF; k++) {
            CHECK(sres[k].n_old == 0 && sres[k].n_beyond == 0 && sres[k].n_new + sres[k].n_dup == 1, "classes");
            CHECK(sres[k].snd_una == ISS[k] + resb[k].delivered, "snd_una of connection %u", k);
            CHECK(sres[k].popped == resb[k].delivered / MSS + (resb[k].delivered == LEN[k] && LEN[k] % MSS) -
                                        (s[k].seg0 - send[k].seg0),
                  "round %u: connection %u popped %u", round, k, sres[k].popped);
            s[k].snd_una = sres[k].snd_una, s[k].seg0 += sres[k].popped, s[k].nseg -= sres[k].popped;
            CHECK(s[k].nseg == sres[k].inflight, "inflight");
            left += s[k].nseg;
        }
        if (left == 0) break;

        /* A: the head of every queue again, rewritten in place */
        CHECK(lvlip_rtx_cpu(fa, NULL, s, NULL, NF, nslots, ring, fd, fd_out) == LVLIP_OK, "rtx");
        nwire = 0;
        for (uint32_t k = 0; k < NF; k++)
            for (uint32_t j = 0; j < RTX; j++) {
                const lvlip_frame_desc d = fd_out[s[k].slot0 + j];
                CHECK((d.len != 0) == (j < s[k].nseg), "round %u: slot %u of connection %u", round, j, k);
                if (d.len == 0) {
                    CHECK(d.offset == 0 && d.reserved == 0, "a dead slot");
                    continue;
                }
                const uint8_t *fr = ring + d.offset;
                CHECK(d.offset == fd[s[k].seg0 + j].offset && d.len == fd[s[k].seg0 + j].len, "fd_out");
                CHECK(be32(fr + 38) == s[k].snd_una + j * MSS, "seq of a re-sent frame");
                CHECK(be32(fr + 42) == IRS && fr[48] == (WIN >> 8) && fr[49] == (WIN & 0xff) && sum_ok(fr, d.len),
                      "ack_seq, window or checksum of a re-sent frame");
                resent++;
                if (round == 0 && k == 0 && j == 0) lost++; /* lost a second time */
                else wire[nwire++] = d;
            }
        shuffle(wire, nwire, &seed);
    }

    CHECK(memcmp(stream, payload, total) == 0, "the streams are not the payloads");
    for (uint32_t k = 0; k < NF; k++)
        CHECK(resb[k].delivered == LEN[k] && s[k].snd_una == ISS[k] + LEN[k] && s[k].nseg == 0, "connection %u", k);

    free(rec), free(wire), free(ackbuf), free(fd_out), free(sink), free(stream), free(fd), free(ring), free(payload);
    if (fails) {
        fprintf(stderr, "snd_loop: %d checks failed\n", fails);
        return 1;
    }
    printf("snd_loop ok: %u bytes over %u connections in %u rounds, %u frames lost, %u re-sent, %u ACKs\n", total, NF,
           round + 1u, lost, resent, acks);
    return 0;
}
