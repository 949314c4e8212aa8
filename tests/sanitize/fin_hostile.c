/*
 * fin_hostile.c — lvlip_fin_check and lvlip_fin_cpu (include/lvlip_skb.h, "the
 * end of a connection") and flow_step.h's flow_fin_step under ASan + UBSan, as
 * a stand-alone program of strict C99: tests/test_fin_sanitize.py compiles it
 * with the library's C sources and runs it.
 *
 * The calls: every NULL among the pointers, nflows at and above the limit with
 * arrays and a frame buffer malloc'd at exactly their sizes (so a store past
 * the 54 bytes of the last flow's slot is a heap overflow), records whose flow
 * is no flow, whose status is no status and whose rel + dlen wraps, close state
 * with garbage in every field (refused, nothing written), and receive, send,
 * write and timer sides at the ends of every field's range.  The step: every
 * state against boundary values of its scalars, where no arithmetic may
 * overflow a signed type.
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

static const uint32_t EDGE[] = {0u, 1u, 2u, 535u, 536u, 59999u, 60000u, 60001u, 0x7FFFFFFFu, 0x80000000u,
                                0xFFFFFFFEu, 0xFFFFFFFFu};
enum { NE = sizeof EDGE / sizeof EDGE[0] };

static int known(uint32_t st) { return st >= LVLIP_TCP_ESTABLISHED && st <= LVLIP_TCP_TIME_WAIT; }

static void hostile_step(void)
{
    uint32_t seen = 0, n = 0;
    for (uint32_t st = LVLIP_TCP_ESTABLISHED; st <= LVLIP_TCP_TIME_WAIT; st++)
        for (uint32_t a = 0; a < NE; a++)         /* expires */
            for (uint32_t b = 0; b < NE; b++)     /* now */
                for (uint32_t d = 0; d < 256u; d++) {
                    lvlip_fin_flow x;
                    memset(&x, 0, sizeof x);
                    x.state = (uint8_t)st, x.flags = (uint8_t)(d & 1u);
                    x.expires = EDGE[a], x.interval = EDGE[(a + d) % 7u], x.retries = EDGE[(a + b + d) % NE];
                    x.base = EDGE[(b + d) % NE];
                    const uint32_t dead = (d >> 1 & 3u) == 3u, hit = d >> 3 & 1u, again = d >> 4 & 1u, close = d >> 5 & 1u;
                    const uint32_t nseg = d >> 6 & 1u, unsent = d >> 7 & 1u;
                    const uint32_t nxt = EDGE[(a + 2u * b + d) % NE], rcv = EDGE[(3u * a + b + d) % NE];
                    x.fin_seq = nxt - 1u;
                    const uint32_t una = (d & 4u) ? nxt : nxt - 1u;
                    const lvlip_fin_flow was = x;
                    const flow_fin_out o = flow_fin_step(&x, dead, rcv, una, nxt, nseg, unsent, EDGE[(b + d) % NE], hit, again,
                                                         close, EDGE[b]);
                    n++;
                    seen |= o.events;
                    CHECK(known(x.state) && x.interval <= LVLIP_FIN_MAX_MS, "state %u, interval %u", x.state, x.interval);
                    CHECK(o.frame == !!(o.events & (LVLIP_FIN_EV_SENT | LVLIP_FIN_EV_RESENT)), "frame against events");
                    CHECK(o.rcv_nxt == rcv + !!(o.events & LVLIP_FIN_EV_PEER_FIN) && x.base == o.rcv_nxt, "rcv_nxt");
                    CHECK(o.snd_nxt == nxt + !!(o.events & LVLIP_FIN_EV_SENT), "snd_nxt");
                    CHECK(!(o.events & LVLIP_FIN_EV_PEER_FIN) || (o.events & LVLIP_FIN_EV_ACK_OWED), "a FIN owes an ACK");
                    if (dead || st == LVLIP_TCP_CLOSED) {
                        lvlip_fin_flow y = was;
                        y.base = rcv;
                        CHECK(memcmp(&x, &y, sizeof x) == 0 && !o.events && !o.frame && !o.interval, "step 0 changed a flow");
                    }
                    CHECK(!(o.events & LVLIP_FIN_EV_SENT) || ((x.flags & 1u) && unsent == 0 && x.fin_seq == nxt &&
                                                              x.interval >= 1u && x.expires == EDGE[b] + x.interval &&
                                                              x.retries == 0), "the sent state");
                    CHECK(!(o.events & LVLIP_FIN_EV_RESENT) || (was.expires < EDGE[b] && nseg == 0 &&
                                                                x.expires == EDGE[b] + x.interval &&
                                                                (x.retries == was.retries + 1u || x.retries == 0xFFFFFFFFu)),
                          "the resent state");
                    CHECK(!(o.events & LVLIP_FIN_EV_TW_DONE) || x.state == LVLIP_TCP_CLOSED, "TW_DONE");
                }
    CHECK(seen == 0x7Fu, "events %#x of %u steps", seen, n);
}

static void hostile_calls(void)
{
    const uint32_t NF = LVLIP_LRO_MAX_FLOWS, NR = 200000u;
    uint32_t seed = 5;
    lvlip_lro_flow *f = calloc(NF, sizeof *f);
    lvlip_lro_result *gin = calloc(NF, sizeof *gin);
    lvlip_lro_rec *rec = calloc(NR, sizeof *rec);
    lvlip_snd_flow *s = calloc(NF, sizeof *s);
    lvlip_push_flow *w = calloc(NF, sizeof *w);
    lvlip_rto_flow *t = calloc(NF, sizeof *t);
    lvlip_fin_flow *x = calloc(NF, sizeof *x);
    uint8_t *close = malloc(NF);
    lvlip_frame_desc *fd = malloc(NF * sizeof *fd);
    lvlip_lro_result *gate = malloc(NF * sizeof *gate);
    lvlip_fin_result *res = malloc(NF * sizeof *res);
    /* the last slot ends with its frame: bytes 54 .. 63 of it are not the call's to write */
    const size_t out_bytes = (size_t)LVLIP_PERSIST_SLOT * (NF - 1u) + 54u;
    uint8_t *out = malloc(out_bytes);
    memset(out, 0x5A, out_bytes);
    uint32_t frames = 0, fins = 0;
    for (uint32_t it = 0; it < 5u; it++) {
        for (uint32_t k = 0; k < NF; k++) {
            f[k].rcv_nxt = EDGE[rnd(&seed) % NE], gin[k].delivered = EDGE[rnd(&seed) % NE], gin[k].placed = rnd(&seed) >> 31;
            gin[k].nsack = rnd(&seed), gin[k].sack[3].right = rnd(&seed);
            s[k].snd_nxt = EDGE[rnd(&seed) % NE], s[k].snd_una = s[k].snd_nxt - (rnd(&seed) >> 31);
            s[k].nseg = (rnd(&seed) >> 29) == 0u, s[k].win = (uint16_t)rnd(&seed);
            w[k].unsent = (rnd(&seed) >> 29) == 0u ? EDGE[rnd(&seed) % NE] : 0u;
            for (uint32_t i = 0; i < 54u; i++) w[k].hdr[i] = (uint8_t)(rnd(&seed) >> 24); /* no template at all */
            t[k].rto = EDGE[rnd(&seed) % NE], t[k].dead = (rnd(&seed) >> 28) == 0u;
            x[k].state = (uint8_t)(LVLIP_TCP_ESTABLISHED + rnd(&seed) % 8u), x[k].flags = (uint8_t)(rnd(&seed) >> 24);
            x[k].interval = EDGE[rnd(&seed) % 7u], x[k].expires = EDGE[rnd(&seed) % NE], x[k].retries = EDGE[rnd(&seed) % NE];
            x[k].base = f[k].rcv_nxt - EDGE[rnd(&seed) % NE], x[k].fin_seq = s[k].snd_nxt - 1u;
            close[k] = (uint8_t)(rnd(&seed) >> 30 ? 0u : rnd(&seed) >> 24);
        }
        for (uint32_t i = 0; i < NR; i++) {
            rec[i].flow = (rnd(&seed) >> 28) == 0u ? EDGE[rnd(&seed) % NE] : rnd(&seed) % NF;
            const uint32_t k = rec[i].flow < NF ? rec[i].flow : 0u;
            rec[i].dlen = (uint16_t)(rnd(&seed) >> 30 ? 0u : rnd(&seed));
            rec[i].rel = f[k].rcv_nxt + gin[k].delivered - x[k].base - rec[i].dlen - (rnd(&seed) >> 30 == 0u);
            rec[i].status = (uint8_t)(rnd(&seed) >> 29 ? (rec[i].dlen ? LVLIP_LRO_PLACED : LVLIP_LRO_NO_DATA) : rnd(&seed) >> 24);
            rec[i].tcp_flags = (uint8_t)(rnd(&seed) >> 24), rec[i].ack_seq = rnd(&seed);
        }
        const uint32_t now = EDGE[rnd(&seed) % NE];
        CHECK(lvlip_fin_cpu(f, gin, rec, NR, s, w, t, x, NF, it & 1u ? close : NULL, now, out, fd, gate, res) == LVLIP_OK,
              "cpu at the limit");
        for (uint32_t k = 0; k < NF; k++) {
            const uint32_t sent = !!(res[k].events & (LVLIP_FIN_EV_SENT | LVLIP_FIN_EV_RESENT));
            CHECK(fd[k].offset == 64u * (uint64_t)k && fd[k].len == (sent ? 54u : 0u) && res[k].events < 0x80u,
                  "iteration %u, flow %u", it, k);
            CHECK(res[k].state == x[k].state && gate[k].delivered == gin[k].delivered && gate[k].nsack == gin[k].nsack &&
                      gate[k].sack[3].right == gin[k].sack[3].right, "result and gate of flow %u", k);
            frames += sent, fins += !!(res[k].events & LVLIP_FIN_EV_PEER_FIN);
        }
        CHECK(lvlip_fin_check(x, f, NF) == LVLIP_OK, "what the call leaves is a state the check takes");
    }
    CHECK(frames > 1000u && fins > 1000u, "%u frames, %u FINs taken", frames, fins);

    /* refusals: nothing is written */
    uint8_t keep[54];
    memcpy(keep, out, sizeof keep);
    const lvlip_fin_flow x0 = x[0];
    const lvlip_lro_flow f0 = f[0];
    const lvlip_snd_flow s0 = s[0];
    memset(fd, 0xEE, sizeof *fd), memset(res, 0xEE, sizeof *res), memset(gate, 0xEE, sizeof *gate);
    const void *arg[10] = {f, gin, s, w, t, x, out, fd, gate, res};
    for (uint32_t i = 0; i < 10u; i++) {
        const void *a[10];
        memcpy(a, arg, sizeof a);
        a[i] = NULL;
        CHECK(lvlip_fin_cpu((lvlip_lro_flow *)a[0], a[1], rec, 1, (lvlip_snd_flow *)a[2], a[3], a[4], (lvlip_fin_flow *)a[5], 1,
                            close, 7, (void *)a[6], (lvlip_frame_desc *)a[7], (lvlip_lro_result *)a[8],
                            (lvlip_fin_result *)a[9]) == LVLIP_EINVAL, "NULL argument %u", i);
    }
    CHECK(lvlip_fin_cpu(f, gin, NULL, 1, s, w, t, x, 1, close, 7, out, fd, gate, res) == LVLIP_EINVAL, "NULL rec with n > 0");
    CHECK(lvlip_fin_cpu(f, gin, rec, 1, s, w, t, x, 1, close, 7, out, fd, (lvlip_lro_result *)gin, res) == LVLIP_EINVAL,
          "gate == gin");
    CHECK(lvlip_fin_cpu(NULL, NULL, NULL, 9, NULL, NULL, NULL, NULL, 0, NULL, 7, NULL, NULL, NULL, NULL) == LVLIP_OK,
          "nflows == 0");
    CHECK(lvlip_fin_cpu(f, gin, rec, 1, s, w, t, x, NF + 1u, close, 7, out, fd, gate, res) == LVLIP_EINVAL, "above the limit");
    CHECK(lvlip_fin_cpu(f, gin, rec, 0xFFFFFFF1u, s, w, t, x, 1, close, 7, out, fd, gate, res) == LVLIP_EINVAL, "n above");
    CHECK(lvlip_fin_check(x, f, NF + 1u) == LVLIP_EINVAL && lvlip_fin_check(NULL, f, 1) == LVLIP_EINVAL &&
              lvlip_fin_check(x, NULL, 1) == LVLIP_EINVAL && lvlip_fin_check(NULL, NULL, 0) == LVLIP_OK, "check's own refusals");
    const lvlip_fin_flow good = x[NF - 1u];
    for (uint32_t i = 0; i < 6u; i++) {
        lvlip_fin_flow b = good;
        if (i == 0) b.state = 0;
        if (i == 1) b.state = 2;
        if (i == 2) b.state = 11;
        if (i == 3) b.reserved[9] = 1;
        if (i == 4) b.reserved[0] = 255;
        if (i == 5) b.interval = 60001u;
        x[NF - 1u] = b;
        CHECK(lvlip_fin_check(x, f, NF) == LVLIP_EINVAL && lvlip_fin_check(x, f, NF - 1u) == LVLIP_OK, "bad state %u", i);
        CHECK(lvlip_fin_cpu(f, gin, rec, NR, s, w, t, x, NF, close, 7, out, fd, gate, res) == LVLIP_EINVAL, "bad state %u taken", i);
    }
    x[NF - 1u] = good;
    x[NF - 1u].base ^= 1u;
    CHECK(lvlip_fin_check(x, f, NF) == LVLIP_EINVAL, "a base that is not rcv_nxt");
    uint8_t ee[48];
    memset(ee, 0xEE, sizeof ee);
    CHECK(memcmp(keep, out, sizeof keep) == 0 && memcmp(&x0, &x[0], sizeof x0) == 0 && memcmp(&f0, &f[0], sizeof f0) == 0 &&
              memcmp(&s0, &s[0], sizeof s0) == 0 && memcmp(fd, ee, 16) == 0 && memcmp(res, ee, 16) == 0 &&
              memcmp(gate, ee, 48) == 0, "a refused call wrote");
    free(out), free(res), free(gate), free(fd), free(close), free(x), free(t), free(w), free(s), free(rec), free(gin), free(f);
}

int main(void)
{
    hostile_step();
    hostile_calls();
    if (fails) {
        fprintf(stderr, "fin_hostile: %d checks failed\n", fails);
        return 1;
    }
    printf("fin_hostile ok\n");
    return 0;
}
