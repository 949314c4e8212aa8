/*
 * sack_loop.c — INTEGRATION.md §2g as a plain C program: the transfer of
 * snd_loop.c (three connections, every fifth frame of the first flight lost,
 * the first re-sent frame lost once more) run twice on the CPU forms of
 * include/lvlip_skb.h: once with lvlip_rtx_cpu, which sends the head of every
 * queue again whatever the peer holds, and once with lvlip_sack_cpu and
 * lvlip_rtx_sack_cpu, which read the SACK blocks of B's ACK frames into a
 * scoreboard and re-send only entries it does not mark.  It prints the frames
 * each run re-sent and the rounds it took.  Every buffer is malloc'd at
 * exactly its planned size, so a sanitizer build (the CPU tests compile this
 * file with the library's C sources under -fsanitize=address,undefined) sees
 * any byte read or written outside it.
 *
 *   make -C examples && examples/build/sack_loop
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lvlip_csum.h"
#include "lvlip_skb.h"

#define NF 3u
#define MSS 536u
#define RTX 3u          /* frames a retransmit sends per queue */
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

static void shuffle(lvlip_frame_desc *fd, uint32_t n, uint32_t *seed)
{
    for (uint32_t i = n; i-- > 1u;) {
        const uint32_t j = rnd(seed) % (i + 1u);
        const lvlip_frame_desc t = fd[i];
        fd[i] = fd[j], fd[j] = t;
    }
}

/* one whole transfer; *rounds and *resent report it */
static void transfer(int use_sack, uint32_t *rounds, uint32_t *resent)
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
    uint32_t *pick = malloc((size_t)nslots * sizeof *pick);
    uint8_t *sacked = calloc(nfd, 1); /* the scoreboard: one byte per fd index */

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
    lvlip_sack_result kres[NF];

    /* ---- the first flight: every fifth frame lost, the rest shuffled */
    lvlip_frame_desc *wire = malloc((size_t)nseg * sizeof *wire);
    uint32_t nwire = 0;
    for (uint32_t i = 0; i < nseg; i++)
        if (i % 5u != 4u) wire[nwire++] = fd[i];
    shuffle(wire, nwire, &seed);

    lvlip_lro_rec *rec = NULL;
    uint32_t nrec = 0, round = 0;
    *resent = 0;
    for (;; round++) {
        CHECK(round < MAX_ROUNDS, "no progress");
        if (round >= MAX_ROUNDS) break;
        /* B: place, advance over all records so far, acknowledge */
        rec = realloc(rec, (size_t)(nrec + nwire) * sizeof *rec);
        CHECK(lvlip_lro_cpu(ring, wire, nwire, fb, NF, LVLIP_RX_VERIFY_L4, stream, rec + nrec) == LVLIP_OK, "lro");
        nrec += nwire;
        CHECK(lvlip_lro_advance(fb, NF, rec, nrec, resb) == LVLIP_OK, "advance");
        CHECK(lvlip_ack_cpu(t, fb, resb, NF, LVLIP_ACK_ALL, ackbuf, afd) == LVLIP_OK, "ack");

        /* A: the ACK frames through the reverse plan, the ACK side, the scoreboard */
        CHECK(lvlip_lro_cpu(ackbuf, afd, NF, fa, NF, LVLIP_RX_VERIFY_L4, sink, arec) == LVLIP_OK, "lro, reverse");
        CHECK(lvlip_snd_cpu(fa, s, NF, arec, NF, ring, fd, sres) == LVLIP_OK, "snd");
        if (use_sack) {
            CHECK(lvlip_sack_cpu(fa, s, NF, arec, ackbuf, afd, NF, ring, fd, sacked, kres) == LVLIP_OK, "sack");
            for (uint32_t k = 0; k < NF; k++)
                CHECK(kres[k].n_blocks == resb[k].nsack && kres[k].n_valid == kres[k].n_blocks,
                      "round %u: connection %u: %u blocks read, %u valid, %u sent", round, k, kres[k].n_blocks,
                      kres[k].n_valid, resb[k].nsack);
        }
        uint32_t left = 0;
        for (uint32_t k = 0; k < NF; k++) {
            CHECK(sres[k].snd_una == ISS[k] + resb[k].delivered, "snd_una of connection %u", k);
            s[k].snd_una = sres[k].snd_una, s[k].seg0 += sres[k].popped, s[k].nseg -= sres[k].popped;
            left += s[k].nseg;
        }
        if (left == 0) break;

        /* A: re-send, the head of every queue or its first unmarked entries */
        if (use_sack)
            CHECK(lvlip_rtx_sack_cpu(fa, NULL, s, NULL, sacked, NF, nslots, ring, fd, fd_out, pick) == LVLIP_OK,
                  "rtx_sack");
        else
            CHECK(lvlip_rtx_cpu(fa, NULL, s, NULL, NF, nslots, ring, fd, fd_out) == LVLIP_OK, "rtx");
        nwire = 0;
        for (uint32_t g = 0; g < nslots; g++) {
            if (use_sack) {
                CHECK((pick[g] == 0xFFFFFFFFu) == (fd_out[g].len == 0), "slot %u: pick and fd_out", g);
                if (pick[g] != 0xFFFFFFFFu) CHECK(sacked[pick[g]] == 0, "slot %u re-sends a marked entry", g);
            }
            if (fd_out[g].len == 0) continue;
            (*resent)++;
            if (round == 0 && g == 0) continue; /* lost a second time */
            wire[nwire++] = fd_out[g];
        }
        shuffle(wire, nwire, &seed);
    }
    *rounds = round + 1u;

    CHECK(memcmp(stream, payload, total) == 0, "the streams are not the payloads");
    for (uint32_t k = 0; k < NF; k++)
        CHECK(resb[k].delivered == LEN[k] && s[k].snd_una == ISS[k] + LEN[k] && s[k].nseg == 0, "connection %u", k);
    free(rec), free(wire), free(ackbuf), free(sacked), free(pick), free(fd_out), free(sink), free(stream), free(fd);
    free(ring), free(payload);
}

int main(void)
{
    uint32_t rounds[2], resent[2];
    transfer(0, &rounds[0], &resent[0]);
    transfer(1, &rounds[1], &resent[1]);
    CHECK(resent[1] <= resent[0], "the scoreboard re-sent more frames (%u) than the head of the queue (%u)", resent[1],
          resent[0]);
    if (fails) {
        fprintf(stderr, "sack_loop: %d checks failed\n", fails);
        return 1;
    }
    printf("sack_loop ok: head of the queue: %u frames re-sent in %u rounds; with the scoreboard: %u in %u\n", resent[0],
           rounds[0], resent[1], rounds[1]);
    return 0;
}
