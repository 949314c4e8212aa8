/*
 * persist_hostile.c — lvlip_persist_check and lvlip_persist_cpu (include/
 * lvlip_skb.h, "the persist timer") and flow_step.h's flow_persist_step under
 * ASan + UBSan, as a stand-alone program of strict C99:
 * tests/test_persist_cpu.py compiles it with the library's C sources and runs
 * it.
 *
 * The calls: every NULL among the pointers, nflows at and above the limit with
 * arrays and a probe buffer malloc'd at exactly their planned sizes (so a
 * store past slot k's 54 bytes of the last flow is a heap overflow), persist
 * state with garbage in every field (refused, nothing written), and send, write
 * and timer sides at the ends of every field's range.  The step: every
 * combination of boundary values of its scalars, where no arithmetic may
 * overflow a signed type or shift out of range.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lvlip_csum.h"
#include "lvlip_skb.h"

#include "flow_step.h"

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

static const uint32_t EDGE[] = {0u, 1u, 2u, 535u, 536u, 537u, 59999u, 60000u, 60001u, 0x7FFFFFFFu, 0x80000000u,
                                0xFFFFFFFEu, 0xFFFFFFFFu};
enum { NE = sizeof EDGE / sizeof EDGE[0] };

static void hostile_step(void)
{
    uint32_t fired = 0, armed = 0, cleared = 0, n = 0;
    for (uint32_t a = 0; a < NE; a++)         /* expires */
        for (uint32_t b = 0; b < NE; b++)     /* interval */
            for (uint32_t c = 0; c < NE; c++) /* now */
                for (uint32_t d = 0; d < 64u; d++) {
                    lvlip_persist_flow x;
                    memset(&x, 0, sizeof x);
                    x.expires = EDGE[a], x.interval = EDGE[b], x.probes = EDGE[(a + b + c) % NE];
                    x.armed = (uint8_t)(d & 1u);
                    const uint32_t dead = (d >> 1) & 1u, nseg = (d >> 2) & 1u;
                    const uint32_t unsent = EDGE[(d >> 3) % NE], wnd = EDGE[(c + d) % NE], rto = EDGE[(b + d) % NE];
                    const uint32_t mss = 1u + EDGE[(a + d) % 9u];
                    const lvlip_persist_flow was = x;
                    const flow_persist_out o = flow_persist_step(&x, dead, nseg, unsent, wnd, mss, rto, EDGE[c]);
                    n++;
                    CHECK(o.fired <= 1u && o.clear <= 1u && !(o.fired && o.clear), "fired %u, clear %u", o.fired, o.clear);
                    CHECK(!dead || (memcmp(&x, &was, sizeof x) == 0 && !o.fired && !o.clear && !o.interval && !o.probes),
                          "a dead flow changed");
                    CHECK(!o.fired || (was.armed && was.expires < EDGE[c] && nseg == 0 && unsent > 0), "fired unasked");
                    CHECK(!o.fired || (x.interval <= LVLIP_PERSIST_MAX_MS && x.expires == EDGE[c] + x.interval &&
                                       (x.probes == was.probes + 1u || x.probes == 0xFFFFFFFFu)), "the fired state");
                    CHECK(was.armed || !x.armed || (!o.fired && x.interval >= 1u && x.interval <= LVLIP_PERSIST_MAX_MS &&
                                                    x.probes == 0), "arming");
                    CHECK(!o.clear || (was.armed && !x.armed && !x.expires && !x.interval && !x.probes), "the clear");
                    fired += o.fired, armed += !was.armed && x.armed, cleared += o.clear;
                }
    CHECK(fired > 100u && armed > 100u && cleared > 100u, "%u fired, %u armed, %u cleared of %u", fired, armed, cleared, n);
}

static void hostile_calls(void)
{
    const uint32_t NF = LVLIP_LRO_MAX_FLOWS;
    uint32_t seed = 5;
    lvlip_lro_flow *f = calloc(NF, sizeof *f);
    lvlip_lro_result *lro = calloc(NF, sizeof *lro);
    lvlip_snd_flow *s = calloc(NF, sizeof *s);
    lvlip_push_flow *w = calloc(NF, sizeof *w);
    lvlip_rto_flow *t = calloc(NF, sizeof *t);
    lvlip_persist_flow *p = calloc(NF, sizeof *p);
    lvlip_frame_desc *fd = malloc(NF * sizeof *fd);
    lvlip_persist_result *res = malloc(NF * sizeof *res);
    /* the last slot ends with its frame: bytes 54 .. 63 of it are not the call's to write */
    const size_t out_bytes = (size_t)LVLIP_PERSIST_SLOT * (NF - 1u) + 54u;
    uint8_t *out = malloc(out_bytes);
    memset(out, 0x5A, out_bytes);
    uint32_t fired = 0;
    for (uint32_t it = 0; it < 6u; it++) {
        for (uint32_t k = 0; k < NF; k++) {
            f[k].rcv_nxt = EDGE[rnd(&seed) % NE], lro[k].delivered = EDGE[rnd(&seed) % NE];
            s[k].snd_una = EDGE[rnd(&seed) % NE], s[k].nseg = (rnd(&seed) >> 29) == 0u, s[k].win = (uint16_t)rnd(&seed);
            w[k].unsent = EDGE[rnd(&seed) % NE], w[k].wnd = EDGE[rnd(&seed) % NE], w[k].mss = (uint16_t)EDGE[rnd(&seed) % NE];
            for (uint32_t i = 0; i < 54u; i++) w[k].hdr[i] = (uint8_t)(rnd(&seed) >> 24); /* no template at all */
            t[k].rto = EDGE[rnd(&seed) % NE], t[k].dupacks = EDGE[rnd(&seed) % NE], t[k].dead = (rnd(&seed) >> 28) == 0u;
            p[k].armed = (uint8_t)(rnd(&seed) >> 31);
            p[k].interval = p[k].armed ? 1u + rnd(&seed) % LVLIP_PERSIST_MAX_MS : EDGE[rnd(&seed) % 8u];
            p[k].expires = EDGE[rnd(&seed) % NE], p[k].probes = EDGE[rnd(&seed) % NE];
        }
        const uint32_t now = EDGE[rnd(&seed) % NE];
        CHECK(lvlip_persist_check(p, NF) == LVLIP_OK, "check at the limit");
        CHECK(lvlip_persist_cpu(f, it & 1u ? lro : NULL, s, w, t, p, NF, now, out, fd, res) == LVLIP_OK, "cpu at the limit");
        for (uint32_t k = 0; k < NF; k++) {
            CHECK(fd[k].offset == 64u * (uint64_t)k && fd[k].len == (res[k].fired ? 54u : 0u) && res[k].fired <= 1u,
                  "iteration %u, flow %u", it, k);
            CHECK(p[k].armed <= 1u && p[k].interval <= LVLIP_PERSIST_MAX_MS, "state of flow %u", k);
            fired += res[k].fired;
        }
        CHECK(lvlip_persist_check(p, NF) == LVLIP_OK, "what the call leaves is a state it takes");
    }
    CHECK(fired > 1000u, "%u fired", fired);

    /* refusals: nothing is written */
    uint8_t keep[54];
    memcpy(keep, out, sizeof keep);
    const lvlip_persist_flow p0 = p[0];
    const lvlip_rto_flow t0 = t[0];
    memset(fd, 0xEE, sizeof *fd), memset(res, 0xEE, sizeof *res);
    const void *arg[8] = {f, s, w, t, p, out, fd, res};
    for (uint32_t i = 0; i < 8u; i++) {
        const void *a[8];
        memcpy(a, arg, sizeof a);
        a[i] = NULL;
        CHECK(lvlip_persist_cpu(a[0], lro, a[1], a[2], (lvlip_rto_flow *)a[3], (lvlip_persist_flow *)a[4], 1, 7, (void *)a[5],
                                (lvlip_frame_desc *)a[6], (lvlip_persist_result *)a[7]) == LVLIP_EINVAL, "NULL argument %u", i);
    }
    CHECK(lvlip_persist_cpu(NULL, NULL, NULL, NULL, NULL, NULL, 0, 7, NULL, NULL, NULL) == LVLIP_OK, "nflows == 0");
    CHECK(lvlip_persist_cpu(f, lro, s, w, t, p, NF + 1u, 7, out, fd, res) == LVLIP_EINVAL, "above the limit");
    CHECK(lvlip_persist_check(p, NF + 1u) == LVLIP_EINVAL && lvlip_persist_check(NULL, 1) == LVLIP_EINVAL &&
              lvlip_persist_check(NULL, 0) == LVLIP_OK, "check's own refusals");
    static const lvlip_persist_flow bad[] = {{0, 0, 0, 2, {0, 0, 0}},       {0, 1000, 0, 255, {0, 0, 0}},
                                             {0, 1000, 0, 1, {0, 1, 0}},    {0, 0, 0, 0, {0, 0, 255}},
                                             {0, 60001u, 0, 1, {0, 0, 0}},  {0, 0xFFFFFFFFu, 0, 0, {0, 0, 0}},
                                             {5, 0, 9, 1, {0, 0, 0}},       {0, 0x80000000u, 0, 1, {0, 0, 0}}};
    for (uint32_t i = 0; i < sizeof bad / sizeof bad[0]; i++) {
        p[NF - 1u] = bad[i];
        CHECK(lvlip_persist_check(p, NF) == LVLIP_EINVAL && lvlip_persist_check(p, NF - 1u) == LVLIP_OK, "bad state %u", i);
        CHECK(lvlip_persist_cpu(f, lro, s, w, t, p, NF, 7, out, fd, res) == LVLIP_EINVAL, "bad state %u taken", i);
    }
    uint8_t ee[16];
    memset(ee, 0xEE, sizeof ee);
    CHECK(memcmp(keep, out, sizeof keep) == 0 && memcmp(&p0, &p[0], sizeof p0) == 0 && memcmp(&t0, &t[0], sizeof t0) == 0 &&
              memcmp(fd, ee, 16) == 0 && memcmp(res, ee, 16) == 0, "a refused call wrote");
    free(out), free(res), free(fd), free(p), free(t), free(w), free(s), free(lro), free(f);
}

int main(void)
{
    hostile_step();
    hostile_calls();
    if (fails) {
        fprintf(stderr, "persist_hostile: %d checks failed\n", fails);
        return 1;
    }
    printf("persist_hostile ok\n");
    return 0;
}
