/*
 * cc_hostile.c — lvlip_cc_cpu (include/lvlip_skb.h, "the congestion window")
 * under ASan + UBSan, as a stand-alone program: tests/test_cc_cpu.py compiles
 * it with the library's C sources and runs it.
 *
 * State at the ends of every field's range (cwnd = cwnd_max = 2^30, mss 1 and
 * 65495, acked = 2^30 with n_new = 2^32 - 1, acc at 2^30, a recover behind
 * snd_una, a flight of 2^32 - 1), popped beyond the queue, descriptors of 0,
 * 53, 54 and 2^32 - 1 bytes, and every array malloc'd at EXACTLY its size with
 * the queues ending at the arrays' last entry, so a read one entry past a
 * queue is a heap overflow.  Every result is compared with a restatement in
 * 64-bit arithmetic; the state a call leaves goes into the next one for as
 * long as lvlip_cc_check takes it.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lvlip_csum.h"
#include "lvlip_skb.h"

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

static uint32_t rnd(uint32_t *s) { return *s = *s * 1664525u + 1013904223u; }

#define MAXW LVLIP_CC_MAX_WND
#define RND(n) ((rnd(&seed) >> 8) % (n)) /* the generator's low bits have short periods */
#define PICK(a) (a)[RND(sizeof(a) / sizeof *(a))]

enum { NF = 64, QLEN = 37, ROUNDS = 400 };

int main(void)
{
    static const uint32_t LENS[] = {0u, 53u, 54u, 55u, 590u, 0xFFFFFFFFu};
    static const uint32_t MSS[] = {1u, 536u, 65495u};
    static const uint32_t WNDS[] = {0u, 1u, 2144u, 65495u, MAXW - 1u, MAXW};
    static const uint32_t ACKED[] = {0u, 1u, 536u, MAXW, 0xFFFFFFFFu};
    static const uint32_t NNEW[] = {0u, 1u, 7u, 0xFFFFFFFFu};
    static const uint32_t POPPED[] = {0u, 1u, QLEN - 1u, QLEN, QLEN + 1u, 0xFFFFFFFFu};
    static const uint32_t FLIGHT[] = {0u, 1u, 8040u, MAXW, 0xFFFFFFFFu};
    static const uint32_t UNA[] = {0u, 5u, 0x7FFFFFFFu, 0xFFFFF000u, 0xFFFFFFFFu};
    uint32_t seed = 11, events = 0, refused = 0;
    /* exactly sized: NF flows, and NF queues of QLEN entries that end at the last entry of fd and sacked */
    lvlip_snd_flow *s = malloc(NF * sizeof *s);
    lvlip_snd_result *snd = malloc(NF * sizeof *snd);
    lvlip_rto_result *prev = malloc(NF * sizeof *prev);
    lvlip_cc_flow *c = malloc(NF * sizeof *c), *c0 = malloc(NF * sizeof *c0);
    lvlip_rto_flow *t = malloc(NF * sizeof *t), *t0 = malloc(NF * sizeof *t0);
    lvlip_cc_result *res = malloc(NF * sizeof *res);
    lvlip_frame_desc *fd = malloc((size_t)NF * QLEN * sizeof *fd);
    uint8_t *sacked = malloc((size_t)NF * QLEN);
    memset(s, 0, NF * sizeof *s), memset(snd, 0, NF * sizeof *snd), memset(prev, 0, NF * sizeof *prev);
    memset(c, 0, NF * sizeof *c), memset(t, 0, NF * sizeof *t);
    for (uint32_t k = 0; k < NF; k++) {
        const uint32_t mss = MSS[k % 3u];
        c[k].mss = (uint16_t)mss, c[k].cwnd = c[k].cwnd_max = k % 5u ? MAXW : mss, c[k].ssthresh = k % 2u ? MAXW : 0u;
        t[k].rto = 1000u, t[k].wnd_cap = 7u, t[k].dead = k == 9u;
        s[k].seg0 = k * QLEN, s[k].nseg = QLEN;
    }
    CHECK(lvlip_cc_check(c, NF) == LVLIP_OK, "the first state");

    for (uint32_t r = 0; r < ROUNDS; r++) {
        for (uint32_t i = 0; i < (uint32_t)NF * QLEN; i++) {
            fd[i].offset = ((uint64_t)rnd(&seed) << 32) | rnd(&seed), fd[i].len = PICK(LENS), fd[i].reserved = 0;
            sacked[i] = (uint8_t)(rnd(&seed) >> 30 ? 0u : (rnd(&seed) >> 24) | 1u);
        }
        for (uint32_t k = 0; k < NF; k++) {
            /* one flow in 64 carries what leaves a state lvlip_cc_check names: a flight above 2^31, which no plan
             * passes, or recovery with ssthresh below mss (the header's limits) */
            const int rare = RND(64u) == 0u;
            uint32_t flight = PICK(FLIGHT);
            if (flight > MAXW && !rare) flight = MAXW;
            s[k].snd_una = PICK(UNA), s[k].snd_nxt = s[k].snd_una + flight;
            s[k].nseg = r % 3u ? QLEN : RND(QLEN + 1u), s[k].seg0 = (k + 1u) * QLEN - s[k].nseg;
            snd[k].acked = PICK(ACKED), snd[k].n_new = PICK(NNEW), snd[k].popped = PICK(POPPED);
            prev[k].fired = RND(4u), prev[k].backoff = RND(3u); /* fired 3 is no value: nothing fires */
            /* state at the ends of the ranges; the arithmetic's own results otherwise */
            if (RND(4u) == 0u) {
                const uint32_t mss = c[k].mss;
                uint32_t v = PICK(WNDS);
                c[k].cwnd = v < mss ? mss : v;
                v = PICK(WNDS);
                c[k].cwnd_max = v < mss ? mss : v;
                c[k].ssthresh = PICK(WNDS), c[k].acc = PICK(WNDS), c[k].in_rec = RND(2u);
                if (c[k].in_rec && c[k].ssthresh < mss && !rare) c[k].ssthresh = mss;
                c[k].recover = s[k].snd_una - (RND(3u) ? 0u : 5000u); /* at or behind snd_una */
            }
        }
        memcpy(c0, c, NF * sizeof *c), memcpy(t0, t, NF * sizeof *t);
        const int with_snd = r % 5u != 4u, with_prev = r % 7u != 6u, with_marks = r % 11u != 10u;
        const int rc = lvlip_cc_cpu(s, with_snd ? snd : NULL, with_prev ? prev : NULL, c, t, NF, with_marks ? fd : NULL,
                                    with_marks ? sacked : NULL, res);
        if (lvlip_cc_check(c0, NF) != LVLIP_OK) {
            /* a hostile flight or ssthresh left a state the check names (the header's limits): refused whole */
            CHECK(rc == LVLIP_EINVAL && !memcmp(c, c0, NF * sizeof *c) && !memcmp(t, t0, NF * sizeof *t), "refusal %u", r);
            refused++;
            for (uint32_t k = 0; k < NF; k++) {
                const uint32_t mss = c[k].mss;
                c[k].cwnd = c[k].cwnd_max = mss, c[k].ssthresh = MAXW;
            }
            continue;
        }
        CHECK(rc == LVLIP_OK, "round %u returns %d", r, rc);
        for (uint32_t k = 0; k < NF; k++) {
            const lvlip_cc_flow x = c0[k], y = c[k];
            lvlip_rto_flow tt = t[k];
            tt.wnd_cap = t0[k].wnd_cap;
            CHECK(!memcmp(&tt, &t0[k], sizeof tt), "round %u flow %u: t beyond wnd_cap", r, k);
            if (t0[k].dead) {
                CHECK(!memcmp(&x, &y, sizeof x) && t[k].wnd_cap == t0[k].wnd_cap && res[k].cwnd == x.cwnd &&
                          !res[k].sacked_bytes && !res[k].n_sacked && !res[k].event, "round %u: the dead flow", r);
                continue;
            }
            uint64_t bytes = 0;
            uint32_t cnt = 0;
            const uint32_t p = !with_snd ? 0u : snd[k].popped < s[k].nseg ? snd[k].popped : s[k].nseg;
            for (uint32_t q = s[k].seg0 + p; with_marks && q < s[k].seg0 + s[k].nseg; q++)
                if (sacked[q]) cnt++, bytes += fd[q].len >= 54u ? fd[q].len - 54u : 0u;
            if (bytes > MAXW) bytes = MAXW;
            const uint64_t cap = (uint64_t)y.cwnd + bytes;
            CHECK(res[k].n_sacked == cnt && res[k].sacked_bytes == bytes && res[k].cwnd == y.cwnd &&
                      t[k].wnd_cap == (cap < MAXW ? cap : MAXW),
                  "round %u flow %u: %u marked, %u bytes, cwnd %u, wnd_cap %u", r, k, res[k].n_sacked, res[k].sacked_bytes,
                  res[k].cwnd, t[k].wnd_cap);
            CHECK(y.mss == x.mss && y.cwnd_max == x.cwnd_max && y.in_rec <= 1u && !y.reserved && !y.reserved2[0] &&
                      !y.reserved2[1] && y.acc <= (uint64_t)MAXW + x.mss, "round %u flow %u: state", r, k);
            const uint32_t ev = res[k].event;
            CHECK(!(ev & ~0x1Fu) && !((ev & LVLIP_CC_EV_TIMEOUT) && (ev & LVLIP_CC_EV_ENTER)), "round %u: event %#x", r, ev);
            if (ev & (LVLIP_CC_EV_SLOWSTART | LVLIP_CC_EV_AVOID | LVLIP_CC_EV_EXIT))
                CHECK(y.cwnd <= x.cwnd_max, "round %u flow %u: cwnd %u above the ceiling %u", r, k, y.cwnd, x.cwnd_max);
            if (ev & LVLIP_CC_EV_TIMEOUT) CHECK(y.cwnd <= x.mss || ev != LVLIP_CC_EV_TIMEOUT, "round %u: a timeout", r);
            if (!ev) { /* step 2's last line still holds cwnd to the ceiling */
                const int acks = with_snd && snd[k].n_new && snd[k].acked;
                CHECK(y.cwnd == (acks && x.cwnd > x.cwnd_max ? x.cwnd_max : x.cwnd) && y.ssthresh == x.ssthresh &&
                          y.in_rec == x.in_rec, "round %u flow %u: no event", r, k);
            }
            events |= ev;
        }
    }
    CHECK(events == 0x1Fu, "events seen: %#x", events);
    CHECK(refused > 0 && refused < ROUNDS / 2u, "%u of %u rounds refused", refused, (unsigned)ROUNDS);
    free(sacked), free(fd), free(res), free(t0), free(t), free(c0), free(c), free(prev), free(snd), free(s);
    if (fails) {
        fprintf(stderr, "cc_hostile: %d checks failed\n", fails);
        return 1;
    }
    printf("cc_hostile ok\n");
    return 0;
}
