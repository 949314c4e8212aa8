/*
 * rbuf_hostile.c — lvlip_rbuf_plan, lvlip_rbuf_check and lvlip_rbuf_cpu
 * (include/lvlip_skb.h, "the receive buffer") under ASan + UBSan, as a
 * stand-alone program of strict C99: tests/test_rbuf_sanitize.py compiles it
 * with the library's C sources and runs it.
 *
 * The calls get states they must refuse with nothing written (head beyond
 * used, a region that does not end with its buffer, cap 0 and above 2^30,
 * overlapping buffers, garbage in the reserved bytes) and states they take but
 * whose results are crafted: nsack 7, blocks with wild edges, read counts of
 * 2^32 - 1, and a buffer that claims cap 2^30 over an allocation of a few
 * hundred bytes: a read takes unread bytes only and a move at most `head`
 * bytes from base + head, so whatever the islands claim both stay below
 * base + 2 * used, and `out` is malloc'd at exactly that (a copy that follows
 * cap, rcv_wnd or an island's edge is a heap overflow).  These change values,
 * never an address.
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

static const uint32_t EDGE[] = {0u, 1u, 2u, 99u, 100u, 101u, 199u, 200u, 201u, 0x3FFFFFFFu, 0x40000000u, 0x40000001u,
                                0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
enum { NE = sizeof EDGE / sizeof EDGE[0], N = 4 };

/* N flows of cap 2^30 each that have used `used` bytes and read `head` of them;
 * the caller's out holds 2 * used bytes of flow 0 */
static void claim(lvlip_lro_flow *f, lvlip_rbuf_flow *p, uint32_t used, uint32_t head, uint32_t rcv_nxt)
{
    memset(f, 0, N * sizeof *f);
    memset(p, 0, N * sizeof *p);
    for (uint32_t k = 0; k < N; k++) {
        p[k].base_off = (uint64_t)k << 30;
        p[k].cap = 0x40000000u, p[k].head = head, p[k].mss = 536, p[k].wscale = (uint8_t)(k * 4u);
        p[k].sink_off = (uint64_t)k * used;
        f[k].sport = (uint16_t)k, f[k].rcv_nxt = rcv_nxt;
        f[k].out_off = p[k].base_off + used, f[k].rcv_wnd = p[k].cap - used;
        p[k].adv_edge = rcv_nxt + f[k].rcv_wnd;
    }
}

static void hostile_results(void)
{
    uint32_t seed = 7, moved = 0, reads = 0, calls = 0;
    lvlip_lro_flow f[N];
    lvlip_rbuf_flow p[N];
    lvlip_lro_result res[N], gate[N];
    lvlip_rbuf_result rres[N];
    lvlip_ack_tmpl t[N];
    uint32_t nread[N];
    for (uint32_t a = 0; a < NE; a++)
        for (uint32_t b = 0; b < NE; b++)
            for (uint32_t c = 0; c < 9u; c++) {
                const uint32_t used = 200u, head = EDGE[c] <= used ? EDGE[c] : used;
                /* only flow 0's buffer exists: the others' would start 2^30 bytes on */
                claim(f, p, used, head, EDGE[a]);
                CHECK(lvlip_rbuf_plan(p, f, 1, NULL) == 1u, "plan refused a sound state");
                uint8_t *out = malloc(2u * used), *sink = malloc(used);
                if (!out || !sink) exit(2);
                memset(out, 0x11, 2u * used);
                memset(sink, 0x22, used);
                memset(t, 0, sizeof t);
                for (uint32_t j = 0; j < 4u; j++) {
                    res[0].sack[j].left = EDGE[(a + j) % NE] + (rnd(&seed) & 3u);
                    res[0].sack[j].right = EDGE[(b + j) % NE] + EDGE[a];
                }
                res[0].nsack = 7u, res[0].placed = c & 1u, res[0].delivered = EDGE[b], res[0].reserved = 0u;
                nread[0] = EDGE[b];
                const int rc = lvlip_rbuf_cpu(f, res, p, t, 1, nread, out, c & 2u ? NULL : sink, gate, rres);
                CHECK(rc == LVLIP_OK, "a sound state with crafted results: %d", rc);
                CHECK(rres[0].read <= used - head && rres[0].moved <= used && rres[0].head <= used, "rres");
                CHECK(f[0].out_off - p[0].base_off <= used && f[0].out_off + f[0].rcv_wnd == p[0].base_off + p[0].cap,
                      "the invariants after the call");
                CHECK(lvlip_rbuf_check(p, f, 1) == LVLIP_OK, "the state a call leaves is refused");
                CHECK(gate[0].nsack == 7u && memcmp(gate[0].sack, res[0].sack, sizeof res[0].sack) == 0, "gate");
                moved += (rres[0].flags & LVLIP_RBUF_MOVED) != 0u, reads += rres[0].read != 0u, calls++;
                free(out);
                free(sink);
            }
    CHECK(moved && reads && moved < calls, "the crafted results take both sides: %u moved, %u read of %u", moved, reads,
          calls);
}

static void refused(void)
{
    lvlip_lro_flow f[N], f0[N];
    lvlip_rbuf_flow p[N], p0[N];
    lvlip_lro_result res[N], gate[N];
    lvlip_rbuf_result rres[N];
    lvlip_ack_tmpl t[N];
    uint8_t out[8];
    memset(res, 0, sizeof res);
    for (uint32_t what = 0; what < 9u; what++) {
        claim(f, p, 100u, 50u, 0xFFFFFF00u);
        CHECK(lvlip_rbuf_plan(p, f, N, NULL) == N, "plan refused a sound state");
        switch (what) {
        case 0: p[1].head = 101u; break;                                /* head beyond used */
        case 1: p[1].head = 0xFFFFFFFFu; break;
        case 2: f[2].rcv_wnd += 1u; break;                              /* the region ends behind the buffer */
        case 3: f[2].out_off = p[2].base_off - 1u; break;               /* and starts in front of it */
        case 4: p[3].cap = 0x40000001u, f[3].rcv_wnd += 1u; break;
        case 5: p[0].cap = 0u, f[0].out_off = p[0].base_off, f[0].rcv_wnd = 0u; break;
        case 6: p[2].base_off -= 1u, f[2].out_off -= 1u; break;         /* overlaps flow 1's last byte */
        case 7: p[3].reserved[0] = 0x80u; break;
        default: p[2].piece0 += 1u; break;                              /* not the plan's */
        }
        memcpy(f0, f, sizeof f);
        memcpy(p0, p, sizeof p);
        memset(t, 0x33, sizeof t);
        memset(gate, 0x44, sizeof gate);
        memset(rres, 0x55, sizeof rres);
        memset(out, 0x66, sizeof out);
        CHECK(lvlip_rbuf_check(p, f, N) == LVLIP_EINVAL, "check took broken state %u", what);
        if (what < 8u) CHECK(lvlip_rbuf_plan(p, f, N, NULL) == 0xFFFFFFFFu, "plan took broken state %u", what);
        /* out is 8 bytes: a call that went on would write far outside it */
        CHECK(lvlip_rbuf_cpu(f, res, p, t, N, NULL, out, NULL, gate, rres) == LVLIP_EINVAL, "cpu took broken state %u",
              what);
        CHECK(!memcmp(f, f0, sizeof f) && !memcmp(p, p0, sizeof p), "a refusal wrote the state (%u)", what);
        CHECK(((uint8_t *)t)[56] == 0x33 && ((uint8_t *)gate)[4] == 0x44 && ((uint8_t *)rres)[0] == 0x55 && out[0] == 0x66,
              "a refusal wrote its outputs (%u)", what);
    }
    /* NULLs and the limit */
    claim(f, p, 100u, 50u, 5u);
    CHECK(lvlip_rbuf_plan(p, f, N, NULL) == N, "plan");
    CHECK(lvlip_rbuf_cpu(NULL, res, p, t, N, NULL, out, NULL, gate, rres) == LVLIP_EINVAL, "NULL f");
    CHECK(lvlip_rbuf_cpu(f, NULL, p, t, N, NULL, out, NULL, gate, rres) == LVLIP_EINVAL, "NULL res");
    CHECK(lvlip_rbuf_cpu(f, res, NULL, t, N, NULL, out, NULL, gate, rres) == LVLIP_EINVAL, "NULL p");
    CHECK(lvlip_rbuf_cpu(f, res, p, NULL, N, NULL, out, NULL, gate, rres) == LVLIP_EINVAL, "NULL t");
    CHECK(lvlip_rbuf_cpu(f, res, p, t, N, NULL, NULL, NULL, gate, rres) == LVLIP_EINVAL, "NULL out");
    CHECK(lvlip_rbuf_cpu(f, res, p, t, N, NULL, out, NULL, NULL, rres) == LVLIP_EINVAL, "NULL gate");
    CHECK(lvlip_rbuf_cpu(f, res, p, t, N, NULL, out, NULL, gate, NULL) == LVLIP_EINVAL, "NULL rres");
    CHECK(lvlip_rbuf_cpu(f, res, p, t, N, NULL, out, NULL, res, rres) == LVLIP_EINVAL, "gate == res");
    CHECK(lvlip_rbuf_cpu(f, res, p, t, LVLIP_LRO_MAX_FLOWS + 1u, NULL, out, NULL, gate, rres) == LVLIP_EINVAL, "limit");
    CHECK(lvlip_rbuf_check(p, f, LVLIP_LRO_MAX_FLOWS + 1u) == LVLIP_EINVAL, "limit");
    CHECK(lvlip_rbuf_cpu(NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL) == LVLIP_OK, "nflows 0");
}

int main(void)
{
    hostile_results();
    refused();
    if (fails) {
        fprintf(stderr, "rbuf_hostile: %d checks failed\n", fails);
        return 1;
    }
    puts("rbuf_hostile ok");
    return 0;
}
