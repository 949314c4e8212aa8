/*
 * sack_hostile.c — lvlip_sack_cpu and lvlip_rtx_sack_cpu over hostile inputs,
 * as a program of its own for an ASan + UBSan build (tests/test_sack_cpu.py
 * compiles it with sack_cpu.c, snd_cpu.c and csum_cpu.c): records no library
 * call wrote (any flow, status, flags and rel), ACK frames of random bytes
 * whose fd.len cuts them anywhere, option lists of random kinds and lengths,
 * and queue entries of random header bytes and lengths.  Every buffer is
 * malloc'd at exactly the bytes its descriptors cover, so a read or write
 * outside a frame, the queues or the scoreboard is an error report.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lvlip_csum.h"
#include "lvlip_skb.h"

#define NF 5u
#define NACK 64u
#define NSEG 40u /* queue entries in all */

static uint32_t rnd(uint32_t *s) { return *s = *s * 1664525u + 1013904223u, *s >> 8; }

int main(void)
{
    uint32_t seed = 7, marked = 0, live = 0;
    for (uint32_t it = 0; it < 400u; it++) {
        lvlip_lro_flow f[NF];
        lvlip_snd_flow s[NF];
        memset(f, 0, sizeof f), memset(s, 0, sizeof s);
        uint32_t q = 0;
        for (uint32_t k = 0; k < NF; k++) {
            f[k].rcv_wnd = 1u + rnd(&seed) % 100u;
            s[k].snd_una = it % 3u ? rnd(&seed) << 8 : 0xFFFFFFF0u + k;
            s[k].snd_nxt = s[k].snd_una + rnd(&seed) % 5000u;
            s[k].seg0 = q, s[k].nseg = k == 2u ? 0u : NSEG / 4u, s[k].rtx = rnd(&seed) % 6u;
            q += s[k].nseg;
        }
        uint32_t nfd = 0;
        const uint32_t nslots = lvlip_snd_plan(s, NF, &nfd);
        if (nslots == 0xFFFFFFFFu || nfd != NSEG) return 2;

        /* the TX ring: entries of 0 .. 99 bytes, mostly plausible headers with a random twist */
        lvlip_frame_desc fd[NSEG];
        uint64_t ring_bytes = 0;
        for (uint32_t i = 0; i < NSEG; i++) {
            fd[i].offset = ring_bytes, fd[i].len = rnd(&seed) % 4u ? 54u + rnd(&seed) % 46u : rnd(&seed) % 60u;
            fd[i].reserved = 0;
            ring_bytes += fd[i].len;
        }
        uint8_t *ring = malloc(ring_bytes ? ring_bytes : 1u);
        for (uint64_t i = 0; i < ring_bytes; i++) ring[i] = (uint8_t)rnd(&seed);
        for (uint32_t i = 0; i < NSEG; i++) {
            if (fd[i].len < 54u || rnd(&seed) % 8u == 0u) continue;
            uint8_t *p = ring + fd[i].offset;
            const uint32_t k = i / (NSEG / 4u) + (i / (NSEG / 4u) >= 2u), pay = rnd(&seed) % (fd[i].len - 53u);
            const uint32_t seq = s[k].snd_una + (i % (NSEG / 4u)) * 20u;
            p[14] = 0x45, p[16] = 0, p[17] = (uint8_t)(40u + pay), p[46] = 0x50;
            p[38] = (uint8_t)(seq >> 24), p[39] = (uint8_t)(seq >> 16), p[40] = (uint8_t)(seq >> 8), p[41] = (uint8_t)seq;
            live++;
        }

        /* the ACK frames: random bytes; most get a header that leads to the options, which stay random
         * or get a SACK option over whole entries; fd.len cuts some of them anywhere */
        lvlip_frame_desc afd[NACK];
        lvlip_lro_rec rec[NACK];
        uint64_t ack_bytes = 0;
        uint32_t full[NACK];
        for (uint32_t i = 0; i < NACK; i++) {
            full[i] = 34u + rnd(&seed) % 101u; /* up to 14 + 60 + 60 */
            afd[i].offset = ack_bytes, afd[i].reserved = 0;
            afd[i].len = rnd(&seed) % 4u ? full[i] : rnd(&seed) % (full[i] + 1u);
            ack_bytes += afd[i].len;
        }
        uint8_t *acks = malloc(ack_bytes ? ack_bytes : 1u);
        for (uint64_t i = 0; i < ack_bytes; i++) acks[i] = (uint8_t)rnd(&seed);
        for (uint32_t i = 0; i < NACK; i++) {
            const uint32_t k = rnd(&seed) % NF;
            rec[i].flow = rnd(&seed) % 10u ? k : rnd(&seed) % 2u ? 0xFFFFFFFFu : NF + rnd(&seed) % 3u;
            rec[i].rel = rnd(&seed) % 120u, rec[i].dlen = (uint16_t)rnd(&seed);
            rec[i].status = rnd(&seed) % 4u ? (uint8_t)LVLIP_LRO_PLACED : (uint8_t)rnd(&seed);
            rec[i].tcp_flags = rnd(&seed) % 8u ? 0x10u : (uint8_t)rnd(&seed);
            rec[i].ack_seq = rnd(&seed);
            uint8_t *p = acks + afd[i].offset;
            if (afd[i].len < 15u || rnd(&seed) % 6u == 0u) continue;
            const uint32_t ihl = 5u + (rnd(&seed) % 3u ? 0u : rnd(&seed) % 11u), th = 14u + 4u * ihl;
            p[14] = (uint8_t)(0x40u | ihl);
            if (afd[i].len < th + 13u) continue;
            const uint32_t room = (full[i] > th + 20u ? full[i] - th - 20u : 0u) / 4u;
            const uint32_t hl = 5u + (room > 10u ? 10u : room);
            p[th + 12u] = (uint8_t)(hl << 4);
            if (hl < 8u || afd[i].len < th + 4u * hl || rnd(&seed) % 3u == 0u) continue; /* the options stay random */
            const uint32_t b = 1u + rnd(&seed) % ((4u * hl - 22u) / 8u > 4u ? 4u : (4u * hl - 22u) / 8u);
            uint8_t *o = p + th + 20u;
            o[0] = 1, o[1] = 1, o[2] = 5, o[3] = (uint8_t)(2u + 8u * b);
            for (uint32_t j = 0; j < b; j++) {
                const uint32_t l = s[k].snd_una + 20u * (rnd(&seed) % 10u), r = l + 20u * (rnd(&seed) % 4u);
                uint8_t *w = o + 4u + 8u * j;
                w[0] = (uint8_t)(l >> 24), w[1] = (uint8_t)(l >> 16), w[2] = (uint8_t)(l >> 8), w[3] = (uint8_t)l;
                w[4] = (uint8_t)(r >> 24), w[5] = (uint8_t)(r >> 16), w[6] = (uint8_t)(r >> 8), w[7] = (uint8_t)r;
            }
        }

        uint8_t *sacked = calloc(NSEG, 1);
        lvlip_sack_result *res = malloc(NF * sizeof *res);
        if (lvlip_sack_cpu(f, s, NF, rec, acks, afd, NACK, ring, fd, sacked, res) != LVLIP_OK) return 3;
        uint32_t sum = 0;
        for (uint32_t i = 0; i < NSEG; i++) sum += sacked[i];
        uint32_t told = 0;
        for (uint32_t k = 0; k < NF; k++) told += res[k].n_sacked;
        if (sum != told) return 4;
        marked += sum;

        lvlip_frame_desc *fd_out = malloc((nslots ? nslots : 1u) * sizeof *fd_out);
        uint32_t *pick = malloc((nslots ? nslots : 1u) * sizeof *pick);
        if (lvlip_rtx_sack_cpu(f, NULL, s, NULL, sacked, NF, nslots, ring, fd, fd_out, pick) != LVLIP_OK) return 5;
        for (uint32_t g = 0; g < nslots; g++)
            if (pick[g] != 0xFFFFFFFFu && (pick[g] >= NSEG || sacked[pick[g]])) return 6;
        free(pick), free(fd_out), free(res), free(sacked), free(acks), free(ring);
    }
    if (marked < 100u || live < 1000u) { /* the inputs must reach the marking, or the run shows nothing */
        fprintf(stderr, "sack_hostile: only %u entries marked, %u live\n", marked, live);
        return 1;
    }
    printf("sack_hostile ok: %u entries marked\n", marked);
    return 0;
}
