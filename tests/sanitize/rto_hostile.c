/*
 * rto_hostile.c — lvlip_wnd_cpu and lvlip_rto_cpu (include/lvlip_skb.h, "the
 * timer and the peer's window") under ASan + UBSan, as a stand-alone program:
 * tests/test_rto_cpu.py compiles it with the library's C sources and runs it.
 *
 * lvlip_wnd_cpu: every record field a crafted record can carry (flows beyond
 * the plan, every status, rel beyond the window, every class of ack_seq)
 * against frames malloc'd at EXACTLY their length, so a read one byte past a
 * frame is a heap overflow: every length from 0 up to a whole frame with IPv4
 * and TCP options, header nibbles that lie in both directions, versions other
 * than 4.  lvlip_rto_cpu: timer state at the ends of every field's range
 * (INT32_MIN / INT32_MAX estimators, rto and expires at 0 and 2^32 - 1, a
 * backoff of 255, dupack counts that wrap), queues at the end of the fd index
 * space against a scoreboard malloc'd at exactly the planned size.
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

/* a frame of exactly len bytes in its own allocation */
static uint8_t *frame(uint32_t len, uint32_t vihl, uint32_t hl, uint32_t *seed)
{
    uint8_t *p = malloc(len ? len : 1u);
    for (uint32_t i = 0; i < len; i++) p[i] = (uint8_t)(rnd(seed) >> 24);
    if (len > 14u) p[14] = (uint8_t)vihl;
    const uint32_t th = 14u + 4u * (vihl & 15u);
    if (len > th + 12u) p[th + 12u] = (uint8_t)(hl << 4);
    return p;
}

static void hostile_wnd(void)
{
    enum { NF = 3, N = 4096 };
    uint32_t seed = 7;
    lvlip_lro_flow f[NF];
    lvlip_snd_flow s[NF];
    lvlip_rto_flow t[NF];
    lvlip_push_flow w[NF];
    lvlip_wnd_result res[NF];
    memset(f, 0, sizeof f), memset(s, 0, sizeof s), memset(t, 0, sizeof t), memset(w, 0, sizeof w);
    for (uint32_t k = 0; k < NF; k++) {
        f[k].rcv_wnd = 10u + k;
        s[k].snd_una = 0xFFFFFFF0u + 8u * k, s[k].snd_nxt = s[k].snd_una + 100u;
        t[k].rto = 1000u, t[k].wscale = (uint8_t)(7u * k), t[k].wnd_cap = k ? 0x40000000u : 3u;
    }
    lvlip_lro_rec *rec = malloc(N * sizeof *rec);
    lvlip_frame_desc *fd = malloc(N * sizeof *fd);
    uint8_t **fr = malloc(N * sizeof *fr);
    /* the frames live in separate allocations: offsets are relative to the lowest one */
    uintptr_t lo = UINTPTR_MAX;
    static const uint8_t status[] = {0, 1, 2, 3, 7, 16, 17, 18, 19, 20, 21, 22, 255};
    for (uint32_t i = 0; i < N; i++) {
        const uint32_t vihl = (i % 7u == 0u) ? rnd(&seed) >> 24 : 0x40u | (5u + rnd(&seed) % 11u);
        const uint32_t hl = (i % 5u == 0u) ? rnd(&seed) % 16u : 5u + rnd(&seed) % 11u;
        const uint32_t whole = 14u + 4u * (vihl & 15u) + 4u * hl;
        const uint32_t len = (i % 3u == 0u) ? whole : rnd(&seed) % (whole + 2u);
        fr[i] = frame(len, vihl, hl, &seed);
        fd[i].len = len, fd[i].reserved = 0;
        if ((uintptr_t)fr[i] < lo) lo = (uintptr_t)fr[i];
        rec[i].flow = (i % 11u == 0u) ? rnd(&seed) : rnd(&seed) % (NF + 1u);
        rec[i].rel = (i % 13u == 0u) ? rnd(&seed) : rnd(&seed) % 14u;
        rec[i].dlen = (uint16_t)rnd(&seed);
        rec[i].status = status[rnd(&seed) % sizeof status];
        rec[i].tcp_flags = (uint8_t)((rnd(&seed) >> 8) | ((i & 1u) ? 0x10u : 0u));
        const uint32_t k = rec[i].flow < NF ? rec[i].flow : 0u;
        static const uint32_t d[] = {0u, 1u, 50u, 100u, 101u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
        rec[i].ack_seq = s[k].snd_una + d[rnd(&seed) % 8u];
    }
    for (uint32_t i = 0; i < N; i++) fd[i].offset = (uint64_t)((uintptr_t)fr[i] - lo);
    uint32_t counted = 0;
    for (uint32_t flags = 0; flags < 2u; flags++) {
        CHECK(lvlip_wnd_cpu(f, s, t, flags ? w : NULL, NF, rec, (const void *)lo, fd, N, flags, res) == LVLIP_OK, "wnd");
        for (uint32_t k = 0; k < NF; k++) {
            counted += res[k].n_counting;
            CHECK(res[k].winner == 0xFFFFFFFFu || res[k].winner < N, "winner %u", res[k].winner);
            CHECK(t[k].snd_wnd <= 0x40000000u && res[k].snd_wnd == t[k].snd_wnd, "snd_wnd %u", t[k].snd_wnd);
            CHECK(!flags || w[k].wnd <= t[k].wnd_cap, "w.wnd %u above its cap", w[k].wnd);
        }
    }
    CHECK(counted > 0 && counted < 2u * N, "%u records counted", counted);
    CHECK(lvlip_wnd_cpu(f, s, t, w, NF, NULL, NULL, NULL, 0, LVLIP_WND_APPLY, res) == LVLIP_OK, "wnd with no record");
    CHECK(lvlip_wnd_cpu(f, s, t, w, NF, rec, (const void *)lo, fd, N, 2u, res) == LVLIP_EINVAL, "a flag bit refused");
    for (uint32_t i = 0; i < N; i++) free(fr[i]);
    free(fr), free(fd), free(rec);
}

static void hostile_rto(void)
{
    enum { NF = 64 };
    uint32_t seed = 3;
    static const uint32_t edge[] = {0u, 1u, 2u, 3u, 199u, 200u, 1000u, 60000u, 60001u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu,
                                    0xFFFFFFFFu};
    enum { NE = sizeof edge / sizeof edge[0] };
    lvlip_snd_flow s[NF];
    lvlip_snd_result snd[NF], gate[NF];
    lvlip_push_result push[NF];
    lvlip_rto_flow t[NF];
    lvlip_rto_result res[NF];
    /* queues packed at the top of a scoreboard of exactly that many bytes */
    uint32_t nfd = 0;
    memset(s, 0, sizeof s);
    for (uint32_t k = 0; k < NF; k++) {
        s[k].seg0 = nfd, s[k].nseg = k % 9u == 0u ? 0u : 1u + rnd(&seed) % 70u;
        nfd += s[k].nseg;
    }
    uint32_t planned = 0;
    CHECK(lvlip_snd_plan(s, NF, &planned) == 0 && planned == nfd, "snd plan");
    uint8_t *sacked = malloc(nfd);
    uint32_t fired = 0, dead = 0;
    for (uint32_t it = 0; it < 400u; it++) {
        memset(sacked, 1, nfd);
        for (uint32_t k = 0; k < NF; k++) {
            t[k].srtt = (int32_t)edge[rnd(&seed) % NE], t[k].rttvar = (int32_t)edge[rnd(&seed) % NE];
            t[k].rto = edge[rnd(&seed) % NE], t[k].expires = edge[rnd(&seed) % NE], t[k].dupacks = edge[rnd(&seed) % NE];
            t[k].snd_wnd = 0, t[k].wnd_cap = 0x40000000u, t[k].wscale = 14;
            t[k].armed = rnd(&seed) >> 31, t[k].dead = (rnd(&seed) >> 28) == 0u, t[k].backoff = (uint8_t)edge[rnd(&seed) % NE];
            memset(&snd[k], 0xEE, sizeof snd[k]);
            snd[k].n_new = edge[rnd(&seed) % 4u] * (rnd(&seed) >> 31), snd[k].n_dup = edge[rnd(&seed) % NE];
            push[k].pushed = edge[rnd(&seed) % NE], push[k].bytes = push[k].first = push[k].moved = 0xEEEEEEEEu;
        }
        const uint32_t now = edge[rnd(&seed) % NE];
        CHECK(lvlip_rto_cpu(s, it % 3u ? snd : NULL, it % 5u ? push : NULL, t, NF, now, it & 1u, it % 7u ? sacked : NULL,
                            gate, res) == LVLIP_OK, "rto");
        for (uint32_t k = 0; k < NF; k++) {
            CHECK(res[k].fired <= 2u && gate[k].popped == (res[k].fired ? 0u : s[k].nseg) && gate[k].snd_una == 0 &&
                      gate[k].inflight == 0, "iteration %u, flow %u", it, k);
            CHECK(t[k].armed <= 1u && t[k].dead <= 1u, "flags of flow %u", k);
            fired += res[k].fired != 0u, dead += t[k].dead;
        }
    }
    CHECK(fired > 100u && dead > 100u, "%u fired, %u dead", fired, dead);
    t[5].wscale = 15;
    CHECK(lvlip_rto_cpu(s, NULL, NULL, t, NF, 0, 0, NULL, gate, res) == LVLIP_EINVAL, "a wscale of 15 refused");
    free(sacked);
}

int main(void)
{
    hostile_wnd();
    hostile_rto();
    if (fails) {
        fprintf(stderr, "rto_hostile: %d checks failed\n", fails);
        return 1;
    }
    printf("rto_hostile ok\n");
    return 0;
}
