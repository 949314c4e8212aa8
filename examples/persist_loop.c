/*
 * persist_loop.c — INTEGRATION.md §2k as a plain C program: the transfer of
 * rto_loop.c with a receiver that stops reading, on the CPU forms of
 * include/lvlip_skb.h.
 *
 * What differs from rto_loop.c:
 *   - B's application reads nothing in rounds [STOP0, STOP1): its window is
 *     what lvlip_lro_next_cpu leaves of it and falls below one segment;
 *   - B acknowledges only a round in which a frame of the connection arrived
 *     (rto_loop.c acknowledges every round, which is what reopens a closed
 *     window there), and the ACKs of round STOP1, which carry the reopened
 *     window, are lost;
 *   - A runs lvlip_persist_cpu behind lvlip_rto_cpu: a connection with bytes to
 *     send, nothing in flight and no window for its first segment starts the
 *     persist timer and probes when it runs out; the probes go to B from their
 *     own buffer, beside the ring's frames, and B's answer to one carries its
 *     window as it stands.
 * main runs the transfer twice: with the call it ends and every stream byte
 * is checked; without it the connections that had drained their queues when
 * the window closed never send again, however many rounds they are given.
 * Every buffer is malloc'd at exactly the size its plan gives, so a sanitizer
 * build sees any byte read or written outside it.
 *
 *   make -C examples && examples/build/persist_loop
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
#define WND (4u * MSS)  /* B's window: smaller than every transfer */
#define WIN 29200u      /* A's advertised window */
#define IRS 0x01020304u /* B's sequence number: what A acknowledges */
#define CAP (2u * WND / MSS) /* frame slots and fd entries per connection */
#define PUSH 4u         /* segments A may append per connection and round */
#define WRITE 1500u     /* bytes the application writes per connection and round */
#define TICK 250u       /* ms of A's clock per round */
#define MAX_ROUNDS 2000u
#define STOP0 3u          /* B reads nothing in rounds [STOP0, STOP1) */
#define STOP1 60u
#define HANG_ROUNDS 400u   /* what the run without the persist timer is given */

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

typedef struct loop_stats {
    uint32_t rounds, lost, resent, beyond, timeouts, fast, samples, closed, probes, stalled, done;
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

static void run(int persist, uint32_t max_rounds, loop_stats *st)
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
    lvlip_persist_flow ps[NF]; /* all zero: no timer */
    memset(s, 0, sizeof s), memset(w, 0, sizeof w), memset(tm, 0, sizeof tm), memset(ps, 0, sizeof ps);
    uint64_t poff = 0, roff = 1;
    for (uint32_t k = 0; k < NF; k++) {
        s[k].snd_una = s[k].snd_nxt = ISS[k];
        s[k].seg0 = k * CAP, s[k].rtx = RTX, s[k].win = WIN;
        w[k].pay_off = poff, w[k].ring_off = roff, w[k].stride = 54u + MSS + 1u + 2u * k;
        w[k].cap = CAP, w[k].q0 = k * CAP, w[k].push = PUSH, w[k].wnd = WND, w[k].mss = MSS;
        hdr_a_to_b(w[k].hdr, k, 0, 0, 0x18);
        tm[k].rto = 1000u, tm[k].snd_wnd = WND, tm[k].wnd_cap = 0x40000000u; /* src/tcp_input.c:196; no congestion window */
        poff += LEN[k];
        roff += (uint64_t)CAP * w[k].stride;
    }
    CHECK(lvlip_rto_check(tm, NF) == LVLIP_OK && lvlip_persist_check(ps, NF) == LVLIP_OK, "state checks");
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
    lvlip_lro_rec *rec = malloc((size_t)(nslots + npush + NF) * sizeof *rec);
    /* the probes: slot k is the 64 bytes at 64 k, of which a probe fills 54; the last slot ends with its frame */
    uint8_t *probes = malloc((size_t)LVLIP_PERSIST_SLOT * (NF - 1u) + 54u);
    lvlip_frame_desc bfd[NF];
    lvlip_persist_result bres[NF];
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
    memset(resb, 0, sizeof resb), memset(sres, 0, sizeof sres), memset(kres, 0, sizeof kres);

    uint32_t round = 0, now = 0;
    for (;; round++) {
        if (round >= max_rounds) break;
        now += TICK;
        for (uint32_t k = 0; k < NF; k++) {
            const uint32_t more = LEN[k] - written[k] < WRITE ? LEN[k] - written[k] : WRITE;
            w[k].unsent += more, written[k] += more;
        }
        /* A: append what the peer's window and the free slots allow; the new frames go out as they are */
        CHECK(lvlip_push_cpu(fa, NULL, s, w, NF, npush, payload, ring, fd, sacked, pfd, pres) == LVLIP_OK, "push");
        for (uint32_t k = 0; k < NF; k++)
            CHECK((uint32_t)(s[k].snd_nxt - s[k].snd_una) <= WND || pres[k].pushed == 0,
                  "round %u: connection %u pushed past the peer's window", round, k);
        /* A: the timer.  sres is last round's consumed result: its n_new and n_dup survive lvlip_snd_next_cpu */
        CHECK(lvlip_rto_cpu(s, sres, pres, tm, NF, now, LVLIP_RTO_FAST, sacked, gate, rres) == LVLIP_OK, "rto");
        for (uint32_t k = 0; k < NF; k++) {
            st->timeouts += rres[k].fired == LVLIP_RTO_TIMEOUT, st->fast += rres[k].fired == LVLIP_RTO_FASTRTX;
            st->samples += rres[k].sample != 0xFFFFFFFFu;
            CHECK(!tm[k].dead, "connection %u timed out for good", k);
            CHECK(gate[k].popped == (rres[k].fired ? 0u : s[k].nseg), "round %u: gate %u", round, k);
        }
        /* A: the persist timer, on the same clock; its probes go out beside the ring's frames */
        memset(bfd, 0, sizeof bfd);
        if (persist) {
            CHECK(lvlip_persist_cpu(fa, NULL, s, w, tm, ps, NF, now, probes, bfd, bres) == LVLIP_OK, "persist");
            for (uint32_t k = 0; k < NF; k++) {
                CHECK(!bres[k].fired || (s[k].nseg == 0 && bres[k].seq == s[k].snd_una - 1u && bfd[k].len == 54u),
                      "round %u: the probe of connection %u", round, k);
                st->probes += bres[k].fired, st->stalled += ps[k].armed;
            }
        }
        CHECK(lvlip_rtx_sack_cpu(fa, NULL, s, gate, sacked, NF, nslots, ring, fd, fd_out, pick) == LVLIP_OK, "rtx");
        uint32_t nwire = 0;
        for (uint32_t j = 0; j < npush; j++) to_wire(ring, pfd[j], j / PUSH, 1, wire, &nwire, st);
        for (uint32_t j = 0; j < nslots; j++) {
            CHECK(fd_out[j].len == 0 || rres[j / RTX].fired, "round %u: a silent connection re-sent", round);
            to_wire(ring, fd_out[j], j / RTX, 0, wire, &nwire, st);
        }
        shuffle(wire, nwire, &seed);

        /* B: place, advance, move on; the application reads or not, then the ACK carries the window as it stands */
        CHECK(lvlip_lro_cpu(ring, wire, nwire, fb, NF, LVLIP_RX_VERIFY_L4, stream, rec) == LVLIP_OK, "lro");
        for (uint32_t i = 0; i < nwire; i++) {
            CHECK(rec[i].status == LVLIP_LRO_PLACED || rec[i].status == LVLIP_LRO_OUT_OF_WINDOW,
                  "round %u: frame %u has status %u", round, i, rec[i].status);
            st->beyond += rec[i].status == LVLIP_LRO_OUT_OF_WINDOW;
        }
        CHECK(lvlip_lro_cpu(probes, bfd, NF, fb, NF, LVLIP_RX_VERIFY_L4, stream, rec + nwire) == LVLIP_OK, "lro, probes");
        int heard[NF] = {0};
        for (uint32_t i = 0; i < nwire + NF; i++) {
            if (i >= nwire && bfd[i - nwire].len)
                CHECK(rec[i].status == LVLIP_LRO_NO_DATA && rec[i].rel == 0xFFFFFFFFu && rec[i].flow == i - nwire,
                      "round %u: B takes the probe of connection %u as status %u", round, i - nwire, rec[i].status);
            if (rec[i].flow < NF) heard[rec[i].flow] = 1;
        }
        CHECK(lvlip_lro_advance_carry(fb, NF, rec, nwire + NF, resb, resb) == LVLIP_OK, "advance");
        CHECK(lvlip_lro_next_cpu(fb, resb, NF) == LVLIP_OK, "lro next");
        for (uint32_t k = 0; k < NF; k++) {
            if (round < STOP0 || round >= STOP1) { /* the application has read: the window opens again, up to the region's end */
                const uint64_t room = end[k] - fb[k].out_off;
                fb[k].rcv_wnd = room < WND ? (uint32_t)room : WND;
            }
            st->closed += fb[k].rcv_wnd < MSS && fb[k].rcv_wnd < end[k] - fb[k].out_off; /* below the next segment */
            t[k].hdr[48] = (uint8_t)(fb[k].rcv_wnd >> 8), t[k].hdr[49] = (uint8_t)fb[k].rcv_wnd;
        }
        CHECK(lvlip_ack_cpu(t, fb, resb, NF, LVLIP_ACK_ALL, ackbuf, afd) == LVLIP_OK, "ack");
        /* B acknowledges what it hears, nothing else; and the wire loses the window update of round STOP1 */
        for (uint32_t k = 0; k < NF; k++)
            if (!heard[k] || round == STOP1) afd[k].len = 0;

        /* A: the ACKs through the reverse plan; ACK side, scoreboard, the peer's window, and on */
        CHECK(lvlip_lro_cpu(ackbuf, afd, NF, fa, NF, LVLIP_RX_VERIFY_L4, sink, arec) == LVLIP_OK, "lro, reverse");
        CHECK(lvlip_snd_cpu(fa, s, NF, arec, NF, ring, fd, sres) == LVLIP_OK, "snd");
        CHECK(lvlip_sack_cpu(fa, s, NF, arec, ackbuf, afd, NF, ring, fd, sacked, kres) == LVLIP_OK, "sack");
        CHECK(lvlip_wnd_cpu(fa, s, tm, w, NF, arec, ackbuf, afd, NF, LVLIP_WND_APPLY, wres) == LVLIP_OK, "wnd");
        for (uint32_t k = 0; k < NF; k++)
            CHECK(wres[k].winner == 0xFFFFFFFFu || (wres[k].winner == k && wres[k].raw == fb[k].rcv_wnd &&
                                                    w[k].wnd == fb[k].rcv_wnd),
                  "round %u: connection %u reads window %u, B has %u", round, k, wres[k].raw, fb[k].rcv_wnd);
        CHECK(lvlip_snd_next_cpu(s, sres, NF) == LVLIP_OK, "snd next");
        uint32_t left = 0;
        for (uint32_t k = 0; k < NF; k++) left += s[k].nseg + w[k].unsent + (LEN[k] - written[k]);
        if (left == 0) {
            st->done = 1;
            break;
        }
    }
    st->rounds = round + st->done;

    if (st->done) {
        CHECK(memcmp(stream, payload, total) == 0, "the streams are not the payloads");
        for (uint32_t k = 0; k < NF; k++)
            CHECK(fb[k].rcv_nxt == ISS[k] + LEN[k] && fb[k].out_off == end[k] && s[k].snd_una == s[k].snd_nxt &&
                      s[k].nseg == 0 && w[k].unsent == 0 && w[k].pay_off == end[k] && !ps[k].armed,
                  "connection %u", k);
    } else { /* what hangs: bytes to send, nothing in flight, no window, and no timer that would change it */
        for (uint32_t k = 0; k < NF; k++)
            CHECK(s[k].nseg != 0 || w[k].unsent == 0 || (w[k].wnd < MSS && !tm[k].armed),
                  "connection %u is not done and not stalled", k);
    }
    free(probes);
    free(sacked), free(rec), free(pick), free(wire), free(ackbuf), free(fd_out), free(sink), free(stream);
    free(pfd), free(fd), free(ring), free(payload);
}

int main(void)
{
    loop_stats g, u;
    run(1, MAX_ROUNDS, &g);
    run(0, HANG_ROUNDS, &u);
    CHECK(g.done && g.rounds > STOP1, "with the persist timer the transfer ends: %u rounds", g.rounds);
    CHECK(g.probes >= 3 && g.stalled > g.probes && g.closed > 0, "%u probes over %u armed rounds, %u windows below one segment", g.probes,
          g.stalled, g.closed);
    CHECK(g.lost > 0 && g.resent >= g.lost && g.timeouts + g.fast > 0, "%u lost, %u re-sent", g.lost, g.resent);
    CHECK(!u.done && u.rounds == HANG_ROUNDS && u.probes == 0, "without it the transfer hangs: done %u after %u rounds",
          u.done, u.rounds);
    if (fails) {
        fprintf(stderr, "persist_loop: %d checks failed\n", fails);
        return 1;
    }
    printf("persist_loop ok: %u rounds, %u probes over %u rounds with the timer armed, %u rounds with a window below one segment, "
           "%u frames re-sent (%u timeouts, %u fast retransmits, %u lost); without the persist timer not done after %u "
           "rounds\n", g.rounds, g.probes, g.stalled, g.closed, g.resent, g.timeouts, g.fast, g.lost, u.rounds);
    return 0;
}
