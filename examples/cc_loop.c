/*
 * cc_loop.c — INTEGRATION.md §2j as a plain C program: the transfer of
 * rto_loop.c (the clock, the gate of lvlip_rto_cpu, B's real window through
 * lvlip_wnd_cpu) with a congestion window, on the CPU forms of
 * include/lvlip_skb.h.
 *
 * What differs from rto_loop.c:
 *   - B's window is 16 segments and the application writes as fast as the
 *     window allows, so what bounds a connection is the congestion window;
 *   - lvlip_cc_cpu runs in every round, after lvlip_sack_cpu and before
 *     lvlip_wnd_cpu: from the round's lvlip_snd_result, the previous round's
 *     lvlip_rto_result, the scoreboard and the queue's descriptors it writes
 *     t.wnd_cap, which lvlip_wnd_cpu carries into w.wnd.  A connection opens at
 *     the initial window, grows in slow start, halves when a third duplicate
 *     ACK fires and starts again from one segment after a timeout.
 * main runs the transfer twice, with and without the call (wnd_cap left at
 * 2^30, as rto_loop.c has it), and prints rounds, re-sent frames and the
 * largest snd_nxt - snd_una seen per connection for both.
 * Every buffer is malloc'd at exactly the size its plan gives, so a sanitizer
 * build sees any byte read or written outside it.
 *
 *   make -C examples && examples/build/cc_loop
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lvlip_csum.h"
#include "lvlip_skb.h"

#define NF 3u
#define MSS 536u
#define RTX 4u          /* frames A may re-send per connection and round */
#define WND (16u * MSS) /* B's window: four initial windows */
#define WIN 29200u      /* A's advertised window */
#define IRS 0x01020304u /* B's sequence number: what A acknowledges */
#define CAP (2u * WND / MSS) /* frame slots and fd entries per connection */
#define PUSH 16u        /* segments A may append per connection and round */
#define WRITE WND       /* bytes the application writes per connection and round */
#define TICK 250u       /* ms of A's clock per round */
#define MAX_ROUNDS 2000u
#define IW (4u * MSS)   /* RFC 5681 3.1: min(4 mss, max(2 mss, 4380)) at mss 536 */

static const uint32_t LEN[NF] = {62u * MSS + 100u, 37u * MSS, 101u * MSS + 1u};
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

typedef struct loop_stats {
    uint32_t rounds, lost, resent, beyond, timeouts, fast, events, flight[NF];
} loop_stats;

/* the wire: frame d of connection k goes to B unless it is a first transmission of segment 4 mod 5 */
static void to_wire(const uint8_t *ring, lvlip_frame_desc d, uint32_t k, int first, lvlip_frame_desc *wire,
                    uint32_t *nwire, loop_stats *st)
{
    if (d.len == 0) return;
    const uint8_t *q = ring + d.offset + 38;
    const uint32_t seq = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
    const uint32_t seg = (seq - ISS[k]) / MSS;
    CHECK(seg < (LEN[k] + MSS - 1u) / MSS, "connection %u sends segment %u", k, seg);
    if (first && seg % 5u == 4u) {
        st->lost++;
        return;
    }
    st->resent += !first;
    wire[(*nwire)++] = d;
}

static void run(int cc, loop_stats *st)
{
    uint32_t seed = 1, total = 0;
    memset(st, 0, sizeof *st);
    for (uint32_t k = 0; k < NF; k++) total += LEN[k];
    uint8_t *payload = malloc(total);
    for (uint32_t i = 0; i < total; i++) payload[i] = (uint8_t)(rnd(&seed) >> 24);

    lvlip_lro_flow fa[NF], fb[NF];
    uint64_t end[NF];
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
        hdr_b_to_a(h, k, 0);
        memcpy(&fa[k].saddr, h + 26, 4), memcpy(&fa[k].daddr, h + 30, 4);
        memcpy(&fa[k].sport, h + 34, 2), memcpy(&fa[k].dport, h + 36, 2);
        fa[k].rcv_nxt = IRS, fa[k].rcv_wnd = 1, fa[k].out_off = k, fa[k].user = k;
    }
    uint64_t first_bytes = 0, sink_bytes = 0;
    CHECK(lvlip_lro_plan(fb, NF, &first_bytes) == NF && first_bytes <= total, "lro plan, forward");
    CHECK(lvlip_lro_plan(fa, NF, &sink_bytes) == NF && sink_bytes == NF, "lro plan, reverse");
    uint8_t *stream = malloc(total), *sink = malloc(sink_bytes);
    memset(stream, 0xA5, total);

    /* ---- side A: empty queues, the write sides, and the timer and window state */
    lvlip_snd_flow s[NF];
    lvlip_push_flow w[NF];
    lvlip_rto_flow tm[NF];
    lvlip_cc_flow c[NF];
    memset(s, 0, sizeof s), memset(w, 0, sizeof w), memset(tm, 0, sizeof tm), memset(c, 0, sizeof c);
    uint64_t poff = 0, roff = 1;
    for (uint32_t k = 0; k < NF; k++) {
        s[k].snd_una = s[k].snd_nxt = ISS[k];
        s[k].seg0 = k * CAP, s[k].rtx = RTX, s[k].win = WIN;
        w[k].pay_off = poff, w[k].ring_off = roff, w[k].stride = 54u + MSS + 1u + 2u * k;
        w[k].cap = CAP, w[k].q0 = k * CAP, w[k].push = PUSH, w[k].wnd = WND, w[k].mss = MSS;
        hdr_a_to_b(w[k].hdr, k, 0, 0, 0x18);
        tm[k].rto = 1000u, tm[k].snd_wnd = WND; /* src/tcp_input.c:196 */
        c[k].mss = MSS, c[k].cwnd = IW, c[k].ssthresh = c[k].cwnd_max = LVLIP_CC_MAX_WND;
        tm[k].wnd_cap = cc ? c[k].cwnd : LVLIP_CC_MAX_WND;
        if (cc) w[k].wnd = IW; /* the first push runs before the first lvlip_wnd_cpu */
        poff += LEN[k];
        roff += (uint64_t)CAP * w[k].stride;
    }
    CHECK(lvlip_rto_check(tm, NF) == LVLIP_OK && lvlip_cc_check(c, NF) == LVLIP_OK, "state check");
    uint32_t nfd = 0, nfd_push = 0;
    uint64_t ring_bytes = 0;
    const uint32_t nslots = lvlip_snd_plan(s, NF, &nfd);
    const uint32_t npush = lvlip_push_plan(w, s, NF, &ring_bytes, &nfd_push);
    nfd = nfd_push;
    CHECK(nslots == NF * RTX && npush == NF * PUSH && nfd == NF * CAP, "plans: %u, %u slots, %u descriptors", nslots, npush,
          nfd);
    uint8_t *ring = malloc(ring_bytes);
    lvlip_frame_desc *fd = calloc(nfd, sizeof *fd);
    lvlip_frame_desc *pfd = malloc((size_t)npush * sizeof *pfd);
    lvlip_frame_desc *fd_out = malloc((size_t)nslots * sizeof *fd_out);
    lvlip_frame_desc *wire = malloc((size_t)(nslots + npush) * sizeof *wire);
    uint32_t *pick = malloc((size_t)nslots * sizeof *pick);
    lvlip_lro_rec *rec = malloc((size_t)(nslots + npush) * sizeof *rec);
    uint8_t *sacked = calloc(nfd, 1);
    uint32_t written[NF] = {0};

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
    lvlip_snd_result sres[NF], gate[NF];
    lvlip_sack_result kres[NF];
    lvlip_push_result pres[NF];
    lvlip_rto_result rres[NF];
    lvlip_wnd_result wres[NF];
    lvlip_cc_result cres[NF];
    memset(resb, 0, sizeof resb), memset(sres, 0, sizeof sres), memset(kres, 0, sizeof kres);
    memset(rres, 0, sizeof rres);

    uint32_t round = 0, now = 0;
    for (;; round++) {
        CHECK(round < MAX_ROUNDS, "no progress");
        if (round >= MAX_ROUNDS) break;
        now += TICK;
        for (uint32_t k = 0; k < NF; k++) {
            const uint32_t more = LEN[k] - written[k] < WRITE ? LEN[k] - written[k] : WRITE;
            w[k].unsent += more, written[k] += more;
        }
        /* A: append what the peer's window and the free slots allow; the new frames go out as they are */
        CHECK(lvlip_push_cpu(fa, NULL, s, w, NF, npush, payload, ring, fd, sacked, pfd, pres) == LVLIP_OK, "push");
        for (uint32_t k = 0; k < NF; k++) {
            const uint32_t flight = s[k].snd_nxt - s[k].snd_una;
            CHECK(flight <= WND || pres[k].pushed == 0, "round %u: connection %u pushed past the peer's window", round, k);
            CHECK(!cc || flight <= tm[k].wnd_cap || pres[k].pushed == 0,
                  "round %u: connection %u has %u bytes in flight, wnd_cap %u", round, k, flight, tm[k].wnd_cap);
            CHECK(!cc || round || flight <= IW, "connection %u opens with %u bytes", k, flight);
            if (flight > st->flight[k]) st->flight[k] = flight;
        }
        /* A: the timer.  sres is last round's consumed result: its n_new and n_dup survive lvlip_snd_next_cpu */
        CHECK(lvlip_rto_cpu(s, sres, pres, tm, NF, now, LVLIP_RTO_FAST, sacked, gate, rres) == LVLIP_OK, "rto");
        for (uint32_t k = 0; k < NF; k++) {
            st->timeouts += rres[k].fired == LVLIP_RTO_TIMEOUT, st->fast += rres[k].fired == LVLIP_RTO_FASTRTX;
            CHECK(!tm[k].dead, "connection %u timed out for good", k);
            CHECK(gate[k].popped == (rres[k].fired ? 0u : s[k].nseg), "round %u: gate %u", round, k);
        }
        CHECK(lvlip_rtx_sack_cpu(fa, NULL, s, gate, sacked, NF, nslots, ring, fd, fd_out, pick) == LVLIP_OK, "rtx");
        uint32_t nwire = 0;
        for (uint32_t j = 0; j < npush; j++) to_wire(ring, pfd[j], j / PUSH, 1, wire, &nwire, st);
        for (uint32_t j = 0; j < nslots; j++) {
            CHECK(fd_out[j].len == 0 || rres[j / RTX].fired, "round %u: a silent connection re-sent", round);
            to_wire(ring, fd_out[j], j / RTX, 0, wire, &nwire, st);
        }
        shuffle(wire, nwire, &seed);

        /* B: place, advance, move on; the application reads late, then the ACK carries the window as it stands */
        CHECK(lvlip_lro_cpu(ring, wire, nwire, fb, NF, LVLIP_RX_VERIFY_L4, stream, rec) == LVLIP_OK, "lro");
        for (uint32_t i = 0; i < nwire; i++) {
            CHECK(rec[i].status == LVLIP_LRO_PLACED || rec[i].status == LVLIP_LRO_OUT_OF_WINDOW,
                  "round %u: frame %u has status %u", round, i, rec[i].status);
            st->beyond += rec[i].status == LVLIP_LRO_OUT_OF_WINDOW;
        }
        CHECK(lvlip_lro_advance_carry(fb, NF, rec, nwire, resb, resb) == LVLIP_OK, "advance");
        CHECK(lvlip_lro_next_cpu(fb, resb, NF) == LVLIP_OK, "lro next");
        for (uint32_t k = 0; k < NF; k++) {
            const uint64_t room = end[k] - fb[k].out_off; /* the application reads at once: the window reopens */
            fb[k].rcv_wnd = room < WND ? (uint32_t)room : WND;
            t[k].hdr[48] = (uint8_t)(fb[k].rcv_wnd >> 8), t[k].hdr[49] = (uint8_t)fb[k].rcv_wnd;
        }
        CHECK(lvlip_ack_cpu(t, fb, resb, NF, LVLIP_ACK_ALL, ackbuf, afd) == LVLIP_OK, "ack");

        /* A: the ACKs through the reverse plan; ACK side, scoreboard, the peer's window, and on */
        CHECK(lvlip_lro_cpu(ackbuf, afd, NF, fa, NF, LVLIP_RX_VERIFY_L4, sink, arec) == LVLIP_OK, "lro, reverse");
        CHECK(lvlip_snd_cpu(fa, s, NF, arec, NF, ring, fd, sres) == LVLIP_OK, "snd");
        CHECK(lvlip_sack_cpu(fa, s, NF, arec, ackbuf, afd, NF, ring, fd, sacked, kres) == LVLIP_OK, "sack");
        /* the congestion window: sres is unconsumed, s is as this round's lvlip_rto_cpu saw it, rres is its result */
        if (cc) {
            CHECK(lvlip_cc_cpu(s, sres, rres, c, tm, NF, fd, sacked, cres) == LVLIP_OK, "cc");
            for (uint32_t k = 0; k < NF; k++) {
                st->events |= cres[k].event;
                CHECK(cres[k].cwnd == c[k].cwnd && c[k].cwnd >= MSS && tm[k].wnd_cap == c[k].cwnd + cres[k].sacked_bytes &&
                          cres[k].n_sacked <= s[k].nseg && cres[k].sacked_bytes <= cres[k].n_sacked * MSS,
                      "round %u: connection %u: cwnd %u, %u bytes in %u marked entries of %u", round, k, cres[k].cwnd,
                      cres[k].sacked_bytes, cres[k].n_sacked, s[k].nseg);
            }
        }
        CHECK(lvlip_wnd_cpu(fa, s, tm, w, NF, arec, ackbuf, afd, NF, LVLIP_WND_APPLY, wres) == LVLIP_OK, "wnd");
        for (uint32_t k = 0; k < NF; k++) {
            const uint32_t want = fb[k].rcv_wnd < tm[k].wnd_cap ? fb[k].rcv_wnd : tm[k].wnd_cap;
            CHECK(wres[k].winner == k && wres[k].raw == fb[k].rcv_wnd && w[k].wnd == want,
                  "round %u: connection %u reads window %u, B has %u", round, k, wres[k].raw, fb[k].rcv_wnd);
        }
        CHECK(lvlip_snd_next_cpu(s, sres, NF) == LVLIP_OK, "snd next");
        uint32_t left = 0;
        for (uint32_t k = 0; k < NF; k++) left += s[k].nseg + w[k].unsent + (LEN[k] - written[k]);
        if (left == 0) break;
    }
    st->rounds = round + 1u;

    CHECK(memcmp(stream, payload, total) == 0, "the streams are not the payloads");
    for (uint32_t k = 0; k < NF; k++)
        CHECK(fb[k].rcv_nxt == ISS[k] + LEN[k] && fb[k].out_off == end[k] && s[k].snd_una == s[k].snd_nxt &&
                  s[k].nseg == 0 && w[k].unsent == 0 && w[k].pay_off == end[k],
              "connection %u", k);
    free(sacked), free(rec), free(pick), free(wire), free(ackbuf), free(fd_out), free(sink), free(stream);
    free(pfd), free(fd), free(ring), free(payload);
}

int main(void)
{
    loop_stats g, u;
    run(1, &g);
    run(0, &u);
    CHECK(g.lost > 0 && g.resent >= g.lost && u.resent >= u.lost, "%u lost, %u re-sent with the call; %u and %u without",
          g.lost, g.resent, u.lost, u.resent);
    CHECK((g.events & LVLIP_CC_EV_SLOWSTART) && (g.events & (LVLIP_CC_EV_TIMEOUT | LVLIP_CC_EV_ENTER)) && !u.events,
          "events %#x with the call, %#x without", g.events, u.events);
    for (uint32_t k = 0; k < NF; k++)
        CHECK(g.flight[k] <= u.flight[k] && u.flight[k] == WND, "connection %u: at most %u bytes in flight, %u without", k,
              g.flight[k], u.flight[k]);
    if (fails) {
        fprintf(stderr, "cc_loop: %d checks failed\n", fails);
        return 1;
    }
    const loop_stats *r[2] = {&g, &u};
    for (int i = 0; i < 2; i++)
        printf("%s lvlip_cc_cpu: %u rounds, %u frames re-sent (%u timeouts, %u fast retransmits, %u lost, %u beyond the "
               "window), largest snd_nxt - snd_una %u, %u, %u\n", i ? "without" : "with", r[i]->rounds, r[i]->resent,
               r[i]->timeouts, r[i]->fast, r[i]->lost, r[i]->beyond, r[i]->flight[0], r[i]->flight[1], r[i]->flight[2]);
    printf("cc_loop ok\n");
    return 0;
}
