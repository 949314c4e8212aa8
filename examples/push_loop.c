/*
 * push_loop.c — INTEGRATION.md §2h as a plain C program: the transfer of
 * stream_loop.c with the sender's write queue on the library too, on the CPU
 * forms of include/lvlip_skb.h.
 *
 * What differs from stream_loop.c:
 *   - nothing is cut into frames before round 1.  Each connection has a TX
 *     ring of CAP = 2 x window frame slots and CAP fd entries, whatever its
 *     transfer's length; every round lvlip_push_cpu moves the queue back to the
 *     start of its fd region, cuts up to PUSH new segments from the unsent
 *     bytes into the slots the ACKs gave back, and appends them;
 *   - the application hands its bytes over a piece at a time (unsent grows by
 *     WRITE bytes a round), so most pushes end on a short segment with PSH;
 *   - the network's loss is by stream segment (fd indices are reused now):
 *     segment 4 mod 5 of a connection is lost the first time it is sent.
 * Every buffer is malloc'd at exactly the size its plan gives, so a sanitizer
 * build (the CPU tests compile this file with the library's C sources under
 * -fsanitize=address,undefined) sees any byte read or written outside it.
 *
 *   make -C examples && examples/build/push_loop
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lvlip_csum.h"
#include "lvlip_skb.h"

#define NF 3u
#define MSS 536u
#define RTX 4u          /* frames A sends per connection and round */
#define WND (4u * MSS)  /* B's window: smaller than every transfer */
#define WIN 29200u      /* A's advertised window */
#define IRS 0x01020304u /* B's sequence number: what A acknowledges */
#define CAP (2u * WND / MSS) /* frame slots and fd entries per connection */
#define PUSH 4u         /* segments A may append per connection and round */
#define WRITE 1500u     /* bytes the application writes per connection and round */
#define MAX_ROUNDS 128u

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

int main(void)
{
    uint32_t seed = 1, total = 0;
    for (uint32_t k = 0; k < NF; k++) total += LEN[k];
    uint8_t *payload = malloc(total);
    for (uint32_t i = 0; i < total; i++) payload[i] = (uint8_t)(rnd(&seed) >> 24);

    /* B's flows: a window of WND at the start of a region of LEN bytes, which the
     * window slides through.  The reverse plan parses B's ACKs on side A.  Both
     * plans sort by addresses and ports; ascending source ports keep index k */
    lvlip_lro_flow fa[NF], fb[NF];
    uint64_t end[NF]; /* where connection k's region ends */
    memset(fa, 0, sizeof fa), memset(fb, 0, sizeof fb);
    uint64_t soff = 0;
    for (uint32_t k = 0; k < NF; k++) {
        uint8_t h[54];
        hdr_a_to_b(h, k, 0, 0, 0);
        memcpy(&fb[k].saddr, h + 26, 4), memcpy(&fb[k].daddr, h + 30, 4);
        memcpy(&fb[k].sport, h + 34, 2), memcpy(&fb[k].dport, h + 36, 2);
        fb[k].rcv_nxt = ISS[k], fb[k].rcv_wnd = WND, fb[k].out_off = soff, fb[k].user = k;
        soff += LEN[k];
        end[k] = soff;
        CHECK(WND < LEN[k], "connection %u fits one window", k);
        hdr_b_to_a(h, k, 0);
        memcpy(&fa[k].saddr, h + 26, 4), memcpy(&fa[k].daddr, h + 30, 4);
        memcpy(&fa[k].sport, h + 34, 2), memcpy(&fa[k].dport, h + 36, 2);
        fa[k].rcv_nxt = IRS, fa[k].rcv_wnd = 1, fa[k].out_off = k, fa[k].user = k;
    }
    uint64_t first_bytes = 0, sink_bytes = 0;
    CHECK(lvlip_lro_plan(fb, NF, &first_bytes) == NF && first_bytes <= total, "lro plan, forward");
    CHECK(lvlip_lro_plan(fa, NF, &sink_bytes) == NF && sink_bytes == NF, "lro plan, reverse");
    for (uint32_t k = 0; k < NF; k++) CHECK(fa[k].user == k && fb[k].user == k, "the plans reordered the flows");
    /* the regions together: what the windows may ever reach */
    uint8_t *stream = malloc(total), *sink = malloc(sink_bytes);
    memset(stream, 0xA5, total);

    /* ---- side A: empty queues, and the write sides that will fill them */
    lvlip_snd_flow s[NF];
    lvlip_push_flow w[NF];
    memset(s, 0, sizeof s), memset(w, 0, sizeof w);
    uint64_t poff = 0, roff = 1;
    uint32_t nsegs = 0;
    for (uint32_t k = 0; k < NF; k++) {
        s[k].snd_una = s[k].snd_nxt = ISS[k];
        s[k].seg0 = k * CAP, s[k].rtx = RTX, s[k].win = WIN;
        w[k].pay_off = poff, w[k].ring_off = roff, w[k].stride = 54u + MSS + 1u + 2u * k;
        w[k].cap = CAP, w[k].q0 = k * CAP, w[k].push = PUSH, w[k].wnd = 0x40000000u, w[k].mss = MSS;
        hdr_a_to_b(w[k].hdr, k, 0, 0, 0x18); /* seq, ack_seq and window come from s and fa */
        poff += LEN[k];
        roff += (uint64_t)CAP * w[k].stride;
        nsegs += (LEN[k] + MSS - 1u) / MSS;
    }
    uint32_t nfd = 0, nfd_push = 0;
    uint64_t ring_bytes = 0;
    const uint32_t nslots = lvlip_snd_plan(s, NF, &nfd);
    CHECK(nslots == NF * RTX && nfd == 0, "snd plan: %u slots, %u descriptors", nslots, nfd);
    const uint32_t npush = lvlip_push_plan(w, s, NF, &ring_bytes, &nfd_push);
    nfd = nfd_push;
    CHECK(npush == NF * PUSH && nfd == NF * CAP && CAP == 8u, "push plan: %u slots, %u descriptors", npush, nfd);
    uint8_t *ring = malloc(ring_bytes);
    lvlip_frame_desc *fd = calloc(nfd, sizeof *fd);
    lvlip_frame_desc *pfd = malloc((size_t)npush * sizeof *pfd);
    lvlip_push_result pres[NF];
    lvlip_frame_desc *fd_out = malloc((size_t)nslots * sizeof *fd_out);
    lvlip_frame_desc *wire = malloc((size_t)nslots * sizeof *wire);
    uint32_t *pick = malloc((size_t)nslots * sizeof *pick);
    lvlip_lro_rec *rec = malloc((size_t)nslots * sizeof *rec); /* one round's frames, whatever the transfer's length */
    uint8_t *sacked = calloc(nfd, 1), *sent = calloc(nsegs, 1);
    uint32_t seg_base[NF], written[NF];
    for (uint32_t k = 0, at = 0; k < NF; at += (LEN[k] + MSS - 1u) / MSS, k++) seg_base[k] = at, written[k] = 0;

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
    lvlip_lro_result resb[NF]; /* B's results: each round's prev and res */
    lvlip_snd_result sres[NF];
    lvlip_sack_result kres[NF];
    memset(resb, 0, sizeof resb), memset(sres, 0, sizeof sres), memset(kres, 0, sizeof kres);

    uint32_t round = 0, lost = 0, resent = 0, beyond = 0, slid = 0, pushed = 0, moved = 0;
    for (;; round++) {
        CHECK(round < MAX_ROUNDS, "no progress");
        if (round >= MAX_ROUNDS) break;
        /* the application writes; A appends what fits into the slots the ACKs gave back */
        for (uint32_t k = 0; k < NF; k++) {
            const uint32_t more = LEN[k] - written[k] < WRITE ? LEN[k] - written[k] : WRITE;
            w[k].unsent += more, written[k] += more;
        }
        CHECK(lvlip_push_cpu(fa, NULL, s, w, NF, npush, payload, ring, fd, sacked, pfd, pres) == LVLIP_OK, "push");
        for (uint32_t k = 0; k < NF; k++) {
            CHECK(s[k].seg0 == w[k].q0 && s[k].nseg <= CAP && pres[k].first + pres[k].pushed == s[k].seg0 + s[k].nseg,
                  "round %u: queue %u after the push", round, k);
            pushed += pres[k].pushed, moved += pres[k].moved;
        }
        /* A: the first RTX entries of every queue B does not hold, rewritten in place */
        CHECK(lvlip_rtx_sack_cpu(fa, NULL, s, sres, sacked, NF, nslots, ring, fd, fd_out, pick) == LVLIP_OK, "rtx");
        uint32_t nwire = 0;
        for (uint32_t j = 0; j < nslots; j++) {
            if (fd_out[j].len == 0) continue;
            CHECK(pick[j] < nfd, "pick of a live slot");
            const uint32_t k = j / RTX;
            const uint8_t *q = ring + fd_out[j].offset + 38;
            const uint32_t seq = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
            const uint32_t seg = (seq - ISS[k]) / MSS;
            CHECK(seg < (LEN[k] + MSS - 1u) / MSS, "round %u: slot %u carries segment %u", round, j, seg);
            if (seg >= (LEN[k] + MSS - 1u) / MSS) continue;
            if (!sent[seg_base[k] + seg]) {
                sent[seg_base[k] + seg] = 1;
                if (seg % 5u == 4u) { /* lost the first time */
                    lost++;
                    continue;
                }
            } else {
                resent++;
            }
            wire[nwire++] = fd_out[j];
        }
        shuffle(wire, nwire, &seed);

        /* B: place, advance with the islands carried in resb, acknowledge, move on */
        CHECK(lvlip_lro_cpu(ring, wire, nwire, fb, NF, LVLIP_RX_VERIFY_L4, stream, rec) == LVLIP_OK, "lro");
        for (uint32_t i = 0; i < nwire; i++) {
            CHECK(rec[i].status == LVLIP_LRO_PLACED || rec[i].status == LVLIP_LRO_OUT_OF_WINDOW,
                  "round %u: frame %u has status %u", round, i, rec[i].status);
            beyond += rec[i].status == LVLIP_LRO_OUT_OF_WINDOW;
        }
        CHECK(lvlip_lro_advance_carry(fb, NF, rec, nwire, resb, resb) == LVLIP_OK, "advance");
        CHECK(lvlip_ack_cpu(t, fb, resb, NF, LVLIP_ACK_ALL, ackbuf, afd) == LVLIP_OK, "ack");
        uint32_t want_ack[NF];
        for (uint32_t k = 0; k < NF; k++) want_ack[k] = fb[k].rcv_nxt + resb[k].delivered;
        CHECK(lvlip_lro_next_cpu(fb, resb, NF) == LVLIP_OK, "lro next");
        for (uint32_t k = 0; k < NF; k++) {
            CHECK(fb[k].rcv_nxt == want_ack[k] && resb[k].delivered == 0, "connection %u moved on", k);
            /* the application has the bytes: the window opens again, up to the region's end */
            const uint64_t room = end[k] - fb[k].out_off;
            slid += fb[k].rcv_wnd < WND && room > fb[k].rcv_wnd;
            fb[k].rcv_wnd = room < WND ? (uint32_t)room : WND;
        }

        /* A: the ACK frames through the reverse plan, the ACK side, the scoreboard, and on */
        CHECK(lvlip_lro_cpu(ackbuf, afd, NF, fa, NF, LVLIP_RX_VERIFY_L4, sink, arec) == LVLIP_OK, "lro, reverse");
        for (uint32_t k = 0; k < NF; k++)
            CHECK(arec[k].status == LVLIP_LRO_NO_DATA && arec[k].flow == k && arec[k].ack_seq == want_ack[k],
                  "round %u: ACK %u parsed as status %u, flow %u", round, k, arec[k].status, arec[k].flow);
        CHECK(lvlip_snd_cpu(fa, s, NF, arec, NF, ring, fd, sres) == LVLIP_OK, "snd");
        CHECK(lvlip_sack_cpu(fa, s, NF, arec, ackbuf, afd, NF, ring, fd, sacked, kres) == LVLIP_OK, "sack");
        CHECK(lvlip_snd_next_cpu(s, sres, NF) == LVLIP_OK, "snd next");
        uint32_t left = 0;
        for (uint32_t k = 0; k < NF; k++) {
            CHECK(s[k].snd_una == want_ack[k] && sres[k].popped == 0 && sres[k].inflight == s[k].nseg,
                  "round %u: send side %u", round, k);
            left += s[k].nseg + w[k].unsent + (LEN[k] - written[k]);
        }
        if (left == 0) break;
    }

    CHECK(memcmp(stream, payload, total) == 0, "the streams are not the payloads");
    for (uint32_t k = 0; k < NF; k++)
        CHECK(fb[k].rcv_nxt == ISS[k] + LEN[k] && fb[k].rcv_wnd == 0 && fb[k].out_off == end[k] &&
                  s[k].snd_una == s[k].snd_nxt && s[k].nseg == 0 && w[k].unsent == 0 && w[k].pay_off == end[k],
              "connection %u", k);
    CHECK(lost > 0 && resent >= lost && slid > 0, "%u lost, %u re-sent, %u window moves", lost, resent, slid);
    CHECK(pushed >= nsegs, "%u segments pushed", pushed);
    CHECK(moved > 0 && pushed > NF * CAP, "%u entries moved, %u pushed: the rings wrapped", moved, pushed);

    free(sent), free(sacked), free(rec), free(pick), free(wire), free(ackbuf), free(fd_out), free(sink), free(stream);
    free(pfd), free(fd), free(ring), free(payload);
    if (fails) {
        fprintf(stderr, "push_loop: %d checks failed\n", fails);
        return 1;
    }
    printf("push_loop ok: %u bytes over %u connections in %u rounds through %u ring slots each, %u segments pushed, "
           "%u entries moved, %u lost, %u re-sent, %u beyond the window\n", total, NF, round + 1u, CAP, pushed, moved,
           lost, resent, beyond);
    return 0;
}
