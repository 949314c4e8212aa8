/*
 * fin_loop.c — INTEGRATION.md §2m as a plain C program: three connections
 * carry a short transfer from A to B and then both ends close them, on the CPU
 * forms of include/lvlip_skb.h.
 *
 * What it shows beside rto_loop.c:
 *   - each endpoint has, per connection, a receive side (lvlip_lro_flow), a send
 *     side, a write side whose template its FIN is built from, a timer and an
 *     lvlip_fin_flow that starts as {base = rcv_nxt, ESTABLISHED};
 *   - lvlip_fin_cpu runs once per round at each end, behind the receive calls,
 *     lvlip_snd_next_cpu, lvlip_push_cpu and lvlip_rto_cpu and in front of
 *     lvlip_ack_cpu, which gets the call's `gate` and no LVLIP_ACK_ALL: an ACK
 *     goes out where data was placed or a FIN is owed one, and nowhere else;
 *   - after SENT the ACK template's sequence number is fin_seq + 1: the
 *     templates are the caller's, so the loop writes snd_nxt into them;
 *   - A's application closes everything in round CLOSE_AT, while data is still
 *     unsent: the FIN waits for `unsent` to reach 0.  B's closes connection 0
 *     in the same round (it goes on receiving in FIN_WAIT) and the others once
 *     it has seen A's FIN (CLOSE_WAIT -> LAST_ACK);
 *   - the wire loses A's first FIN of connection 1: the FIN's own timer sends
 *     it again.
 * main runs the loop twice: with the call all six endpoints reach CLOSED (the
 * active closers after 2 MSL of TIME_WAIT); without it every connection stays
 * ESTABLISHED and snd_nxt stops at the last data byte.  Every buffer is
 * malloc'd at exactly the size its plan gives.
 *
 *   make -C examples && examples/build/fin_loop
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
#define PUSH 4u         /* segments A may append per connection and round */
#define CAP 8u          /* frame slots and fd entries per connection */
#define WIN 29200u      /* the window both ends advertise */
#define IRS 0x01020304u /* B's sequence number */
#define TICK 250u       /* ms of the clock per round */
#define CLOSE_AT 1u
#define MAX_ROUNDS 1000u
#define IDLE_ROUNDS 60u /* what the run without the call is given */

static const uint32_t LEN[NF] = {9u * MSS + 100u, 3u * MSS, 14u * MSS + 1u};
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
static void hdr_a_to_b(uint8_t *h, uint32_t k, uint8_t flags)
{
    static const uint8_t H[54] = {
        0x00, 0x0c, 0x29, 0x6d, 0x50, 0x25, 0x0a, 0x1b, 0x2c, 0x3d, 0x4e, 0x5f, 0x08, 0x00, /* eth */
        0x45, 0x00, 0x00, 0x00, 0x12, 0x34, 0x40, 0x00, 0x40, 0x06, 0x00, 0x00,             /* ip  */
        10, 0, 0, 4, 10, 0, 0, 5,                                                           /* A -> B */
        0, 0, 0x1f, 0x40, 0, 0, 0, 0, 0, 0, 0, 0, 0x50, 0, 0x72, 0x10, 0, 0, 0, 0};         /* tcp */
    memcpy(h, H, 54);
    h[34] = (uint8_t)((40000u + k) >> 8), h[35] = (uint8_t)(40000u + k);
    h[47] = flags;
}

/* B -> A: the same with addresses and ports exchanged */
static void hdr_b_to_a(uint8_t *h, uint32_t k, uint8_t flags)
{
    uint8_t t[54];
    hdr_a_to_b(t, k, flags);
    memcpy(h, t, 54);
    memcpy(h, t + 6, 6), memcpy(h + 6, t, 6);
    memcpy(h + 26, t + 30, 4), memcpy(h + 30, t + 26, 4);
    memcpy(h + 34, t + 36, 2), memcpy(h + 36, t + 34, 2);
}

static void put_seq(uint8_t *hdr, uint32_t seq)
{
    hdr[38] = (uint8_t)(seq >> 24), hdr[39] = (uint8_t)(seq >> 16), hdr[40] = (uint8_t)(seq >> 8), hdr[41] = (uint8_t)seq;
}

static void flow_of(lvlip_lro_flow *f, const uint8_t *h, uint32_t rcv_nxt, uint32_t wnd, uint64_t off, uint32_t k)
{
    memcpy(&f->saddr, h + 26, 4), memcpy(&f->daddr, h + 30, 4);
    memcpy(&f->sport, h + 34, 2), memcpy(&f->dport, h + 36, 2);
    f->rcv_nxt = rcv_nxt, f->rcv_wnd = wnd, f->out_off = off, f->user = k;
}

typedef struct loop_stats {
    uint32_t rounds, done, fins, resent, lost, acks_a, acks_b, time_wait, last_ack, late;
} loop_stats;

static void run(int fin, uint32_t max_rounds, loop_stats *st)
{
    uint32_t seed = 1, total = 0;
    memset(st, 0, sizeof *st);
    for (uint32_t k = 0; k < NF; k++) total += LEN[k];
    uint8_t *payload = malloc(total);
    for (uint32_t i = 0; i < total; i++) payload[i] = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);

    /* ---- the receive sides: fb takes A's frames at B, fa takes B's at A */
    lvlip_lro_flow fa[NF], fb[NF];
    memset(fa, 0, sizeof fa), memset(fb, 0, sizeof fb);
    uint64_t soff = 0, end[NF];
    for (uint32_t k = 0; k < NF; k++) {
        uint8_t h[54];
        hdr_a_to_b(h, k, 0);
        flow_of(&fb[k], h, ISS[k], LEN[k], soff, k);
        soff += LEN[k], end[k] = soff;
        hdr_b_to_a(h, k, 0);
        flow_of(&fa[k], h, IRS, 1, k, k);
    }
    uint64_t stream_bytes = 0, sink_bytes = 0;
    CHECK(lvlip_lro_plan(fb, NF, &stream_bytes) == NF && stream_bytes == total, "lro plan, forward");
    CHECK(lvlip_lro_plan(fa, NF, &sink_bytes) == NF && sink_bytes == NF, "lro plan, reverse");
    uint8_t *stream = malloc(total), *sink = malloc(sink_bytes);
    memset(stream, 0xA5, total);

    /* ---- the send sides, write sides and timers: A's carry the data, B's only its FIN */
    lvlip_snd_flow sa[NF], sb[NF];
    lvlip_push_flow wa[NF], wb[NF];
    lvlip_rto_flow ta[NF], tb[NF];
    memset(sa, 0, sizeof sa), memset(sb, 0, sizeof sb), memset(wa, 0, sizeof wa), memset(wb, 0, sizeof wb);
    memset(ta, 0, sizeof ta), memset(tb, 0, sizeof tb);
    uint64_t poff = 0, roff = 1;
    for (uint32_t k = 0; k < NF; k++) {
        sa[k].snd_una = sa[k].snd_nxt = ISS[k], sa[k].seg0 = k * CAP, sa[k].rtx = RTX, sa[k].win = WIN;
        wa[k].pay_off = poff, wa[k].ring_off = roff, wa[k].stride = 54u + MSS + 1u + 2u * k, wa[k].unsent = LEN[k];
        wa[k].cap = CAP, wa[k].q0 = k * CAP, wa[k].push = PUSH, wa[k].wnd = 0x40000000u, wa[k].mss = MSS;
        hdr_a_to_b(wa[k].hdr, k, 0x18);
        ta[k].rto = tb[k].rto = 1000u, ta[k].snd_wnd = ta[k].wnd_cap = tb[k].snd_wnd = tb[k].wnd_cap = 0x40000000u;
        poff += LEN[k], roff += (uint64_t)CAP * wa[k].stride;
        sb[k].snd_una = sb[k].snd_nxt = IRS, sb[k].seg0 = k, sb[k].win = WIN; /* an empty queue of its own */
        wb[k].mss = MSS;
        hdr_b_to_a(wb[k].hdr, k, 0x10);
    }
    uint32_t nfd = 0;
    uint64_t ring_bytes = 0;
    const uint32_t nslots = lvlip_snd_plan(sa, NF, NULL);
    const uint32_t npush = lvlip_push_plan(wa, sa, NF, &ring_bytes, &nfd);
    CHECK(nslots == NF * RTX && npush == NF * PUSH && nfd == NF * CAP, "plans: %u, %u slots, %u descriptors", nslots, npush, nfd);
    uint8_t *ring = malloc(ring_bytes), *sacked = calloc(nfd, 1);
    lvlip_frame_desc *fd = calloc(nfd, sizeof *fd);
    lvlip_frame_desc *pfd = malloc((size_t)npush * sizeof *pfd), *fd_out = malloc((size_t)nslots * sizeof *fd_out);
    lvlip_frame_desc *wire = malloc((size_t)(nslots + npush) * sizeof *wire);
    uint32_t *pick = malloc((size_t)nslots * sizeof *pick);
    lvlip_lro_rec *rec = malloc((size_t)(nslots + npush + 2u * NF) * sizeof *rec);
    uint8_t no_ring[64] = {0};
    lvlip_frame_desc no_fd[NF];
    memset(no_fd, 0, sizeof no_fd);

    /* ---- the close state, the ACK templates of both ends, and the FINs' and ACKs' buffers */
    lvlip_fin_flow xa[NF], xb[NF];
    lvlip_ack_tmpl qa[NF], qb[NF];
    memset(xa, 0, sizeof xa), memset(xb, 0, sizeof xb), memset(qa, 0, sizeof qa), memset(qb, 0, sizeof qb);
    for (uint32_t k = 0; k < NF; k++) {
        xa[k].base = fa[k].rcv_nxt, xb[k].base = fb[k].rcv_nxt, xa[k].state = xb[k].state = LVLIP_TCP_ESTABLISHED;
        qa[k].out_off = qb[k].out_off = 3u + (uint64_t)k * (LVLIP_ACK_MAX_FRAME + 1u), qb[k].max_sack = 4;
        hdr_a_to_b(qa[k].hdr, k, 0x10), hdr_b_to_a(qb[k].hdr, k, 0x10);
        put_seq(qa[k].hdr, ISS[k]), put_seq(qb[k].hdr, IRS); /* what the next pure ACK carries: snd_nxt */
    }
    CHECK(lvlip_fin_check(xa, fa, NF) == LVLIP_OK && lvlip_fin_check(xb, fb, NF) == LVLIP_OK, "fresh close states");
    uint64_t acka_bytes = 0, ackb_bytes = 0;
    CHECK(lvlip_ack_plan(qa, fa, NF, &acka_bytes) == NF && lvlip_ack_plan(qb, fb, NF, &ackb_bytes) == NF, "ack plans");
    const size_t fin_bytes = (size_t)LVLIP_PERSIST_SLOT * (NF - 1u) + 54u; /* the last slot ends with its frame */
    uint8_t *acka = malloc(acka_bytes), *fina = malloc(fin_bytes);
    uint8_t *from_b = malloc(ackb_bytes + fin_bytes); /* B's ACKs, then B's FINs: one buffer for A's receive call */
    lvlip_frame_desc afd_a[NF], ffd_a[NF], fd_b[2u * NF]; /* fd_b: B's ACKs, then B's FINs */
    lvlip_lro_rec arec[2u * NF];
    lvlip_lro_result resa[NF], resb[NF], gate_a[NF], gate_b[NF];
    lvlip_snd_result sres[NF], sresb[NF], gate[NF];
    lvlip_push_result pres[NF];
    lvlip_rto_result rres[NF];
    lvlip_fin_result ea[NF], eb[NF];
    uint8_t close_a[NF], close_b[NF];
    memset(resa, 0, sizeof resa), memset(resb, 0, sizeof resb), memset(sres, 0, sizeof sres);
    memset(afd_a, 0, sizeof afd_a), memset(ffd_a, 0, sizeof ffd_a), memset(fd_b, 0, sizeof fd_b);
    uint32_t narec = 0, lost_once = 0;

    uint32_t round = 0, now = 0;
    for (; round < max_rounds; round++) {
        now += TICK;
        /* A: new segments, the timer */
        CHECK(lvlip_push_cpu(fa, NULL, sa, wa, NF, npush, payload, ring, fd, sacked, pfd, pres) == LVLIP_OK, "push");
        CHECK(lvlip_rto_cpu(sa, sres, pres, ta, NF, now, LVLIP_RTO_FAST, sacked, gate, rres) == LVLIP_OK, "rto");
        /* A: last round's frames from B through its receive side, then the close and the ACKs it owes */
        if (fin) {
            CHECK(lvlip_lro_advance_carry(fa, NF, arec, narec, resa, resa) == LVLIP_OK, "advance, reverse");
            CHECK(lvlip_lro_next_cpu(fa, resa, NF) == LVLIP_OK, "lro next, reverse");
            for (uint32_t k = 0; k < NF; k++) close_a[k] = round >= CLOSE_AT;
            CHECK(lvlip_fin_cpu(fa, resa, arec, narec, sa, wa, ta, xa, NF, close_a, now, fina, ffd_a, gate_a, ea) == LVLIP_OK,
                  "fin, A");
            CHECK(lvlip_fin_check(xa, fa, NF) == LVLIP_OK, "round %u: A's close state", round);
            for (uint32_t k = 0; k < NF; k++) {
                put_seq(qa[k].hdr, sa[k].snd_nxt); /* fin_seq + 1 once the FIN is out */
                CHECK(!(ea[k].events & LVLIP_FIN_EV_SENT) || (wa[k].unsent == 0 && ea[k].seq == ISS[k] + LEN[k]),
                      "round %u: connection %u sent its FIN with %u bytes unsent", round, k, wa[k].unsent);
                st->fins += !!(ea[k].events & LVLIP_FIN_EV_SENT), st->resent += !!(ea[k].events & LVLIP_FIN_EV_RESENT);
                st->late += !!(ea[k].events & LVLIP_FIN_EV_LATE_WRITE);
                st->time_wait += (ea[k].events & LVLIP_FIN_EV_TW_DONE) != 0;
            }
            CHECK(lvlip_ack_cpu(qa, fa, gate_a, NF, 0, acka, afd_a) == LVLIP_OK, "ack, A");
            for (uint32_t k = 0; k < NF; k++) {
                CHECK((afd_a[k].len != 0) == !!(ea[k].events & LVLIP_FIN_EV_ACK_OWED), "round %u: A's ACK of connection %u", round, k);
                st->acks_a += afd_a[k].len != 0;
            }
            if (!lost_once && (ea[1].events & LVLIP_FIN_EV_SENT)) ffd_a[1].len = 0, lost_once = 1, st->lost++; /* the wire */
        }
        CHECK(lvlip_rtx_sack_cpu(fa, NULL, sa, gate, sacked, NF, nslots, ring, fd, fd_out, pick) == LVLIP_OK, "rtx");
        uint32_t nwire = 0;
        for (uint32_t j = 0; j < npush; j++)
            if (pfd[j].len) wire[nwire++] = pfd[j];
        for (uint32_t j = 0; j < nslots; j++)
            if (fd_out[j].len) wire[nwire++] = fd_out[j];

        /* B: the ring's frames, A's FINs and A's ACKs are one round's records */
        CHECK(lvlip_lro_cpu(ring, wire, nwire, fb, NF, LVLIP_RX_VERIFY_L4, stream, rec) == LVLIP_OK, "lro");
        CHECK(lvlip_lro_cpu(fina, ffd_a, NF, fb, NF, LVLIP_RX_VERIFY_L4, stream, rec + nwire) == LVLIP_OK, "lro, FINs");
        CHECK(lvlip_lro_cpu(acka, afd_a, NF, fb, NF, LVLIP_RX_VERIFY_L4, stream, rec + nwire + NF) == LVLIP_OK, "lro, ACKs");
        const uint32_t nrec = nwire + 2u * NF;
        CHECK(lvlip_lro_advance_carry(fb, NF, rec, nrec, resb, resb) == LVLIP_OK, "advance");
        /* B's ACK side: the only thing A can acknowledge is B's FIN */
        CHECK(lvlip_snd_cpu(fb, sb, NF, rec, nrec, no_ring, no_fd, sresb) == LVLIP_OK, "snd, B");
        CHECK(lvlip_snd_next_cpu(sb, sresb, NF) == LVLIP_OK, "snd next, B");
        CHECK(lvlip_lro_next_cpu(fb, resb, NF) == LVLIP_OK, "lro next");
        memcpy(gate_b, resb, sizeof gate_b);
        if (fin) {
            for (uint32_t k = 0; k < NF; k++)
                close_b[k] = round >= CLOSE_AT && (k == 0 || xb[k].state == LVLIP_TCP_CLOSE_WAIT);
            CHECK(lvlip_fin_cpu(fb, resb, rec, nrec, sb, wb, tb, xb, NF, close_b, now, from_b + ackb_bytes, fd_b + NF, gate_b,
                                eb) == LVLIP_OK, "fin, B");
            CHECK(lvlip_fin_check(xb, fb, NF) == LVLIP_OK, "round %u: B's close state", round);
            for (uint32_t k = 0; k < NF; k++) {
                put_seq(qb[k].hdr, sb[k].snd_nxt);
                fd_b[NF + k].offset += ackb_bytes;
                CHECK(!(eb[k].events & LVLIP_FIN_EV_PEER_FIN) || fb[k].rcv_nxt == ISS[k] + LEN[k] + 1u,
                      "round %u: B took the FIN of connection %u in front of a hole", round, k);
                st->fins += !!(eb[k].events & LVLIP_FIN_EV_SENT), st->resent += !!(eb[k].events & LVLIP_FIN_EV_RESENT);
                st->last_ack += (eb[k].events & LVLIP_FIN_EV_ACKED) && xb[k].state == LVLIP_TCP_CLOSED;
                st->time_wait += (eb[k].events & LVLIP_FIN_EV_TW_DONE) != 0;
            }
        }
        /* no LVLIP_ACK_ALL: an ACK where data was placed or the gate says a FIN is owed one */
        CHECK(lvlip_ack_cpu(qb, fb, gate_b, NF, 0, from_b, fd_b) == LVLIP_OK, "ack, B");
        for (uint32_t k = 0; k < NF; k++) st->acks_b += fd_b[k].len != 0;

        /* A: B's ACKs and FINs through the reverse plan; the ACK side moves snd_una past data and FIN alike */
        narec = 2u * NF;
        CHECK(lvlip_lro_cpu(from_b, fd_b, narec, fa, NF, LVLIP_RX_VERIFY_L4, sink, arec) == LVLIP_OK, "lro, reverse");
        CHECK(lvlip_snd_cpu(fa, sa, NF, arec, narec, ring, fd, sres) == LVLIP_OK, "snd");
        CHECK(lvlip_snd_next_cpu(sa, sres, NF) == LVLIP_OK, "snd next");
        uint32_t closed = 0;
        for (uint32_t k = 0; k < NF; k++)
            closed += (xa[k].state == LVLIP_TCP_CLOSED) + (xb[k].state == LVLIP_TCP_CLOSED);
        if (closed == 2u * NF) {
            st->done = 1;
            break;
        }
    }
    st->rounds = round + st->done;

    CHECK(memcmp(stream, payload, total) == 0, "the streams are not the payloads");
    for (uint32_t k = 0; k < NF; k++) {
        const uint32_t last = ISS[k] + LEN[k] + (uint32_t)st->done; /* the FIN takes one sequence number */
        CHECK(sa[k].snd_nxt == last && sa[k].snd_una == last && fb[k].rcv_nxt == last && fb[k].out_off == end[k] &&
                  sa[k].nseg == 0 && wa[k].unsent == 0, "connection %u at A: snd_nxt %u, wanted %u", k, sa[k].snd_nxt, last);
        CHECK(sb[k].snd_nxt == IRS + st->done && sb[k].snd_una == sb[k].snd_nxt && fa[k].rcv_nxt == sb[k].snd_nxt,
              "connection %u at B", k);
        if (!st->done)
            CHECK(xa[k].state == LVLIP_TCP_ESTABLISHED && xb[k].state == LVLIP_TCP_ESTABLISHED, "connection %u left ESTABLISHED", k);
    }
    free(from_b), free(fina), free(acka), free(rec), free(pick), free(wire), free(fd_out), free(pfd), free(fd);
    free(sacked), free(ring), free(sink), free(stream), free(payload);
}

int main(void)
{
    loop_stats g, u;
    run(1, MAX_ROUNDS, &g);
    run(0, IDLE_ROUNDS, &u);
    CHECK(g.done && g.rounds > LVLIP_FIN_2MSL_MS / TICK, "with the call all six endpoints close: %u rounds", g.rounds);
    CHECK(g.fins == 2u * NF && g.lost == 1 && g.resent >= 1, "%u FINs, %u lost, %u sent again", g.fins, g.lost, g.resent);
    CHECK(g.time_wait >= 1 && g.last_ack >= 1 && g.acks_a == NF && g.late == 0, "%u through TIME_WAIT, %u through LAST_ACK, %u ACKs from A",
          g.time_wait, g.last_ack, g.acks_a);
    CHECK(!u.done && u.rounds == IDLE_ROUNDS && u.fins == 0, "without it nothing closes: done %u after %u rounds", u.done, u.rounds);
    if (fails) {
        fprintf(stderr, "fin_loop: %d checks failed\n", fails);
        return 1;
    }
    printf("fin_loop ok: %u rounds, %u FINs (%u lost, %u sent again), %u endpoints through TIME_WAIT and %u through LAST_ACK, "
           "%u ACKs from A and %u from B; without the call nothing closed in %u rounds\n", g.rounds, g.fins, g.lost, g.resent,
           g.time_wait, g.last_ack, g.acks_a, g.acks_b, u.rounds);
    return 0;
}
