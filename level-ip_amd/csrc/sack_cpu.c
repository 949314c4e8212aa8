/*
 * sack_cpu.c — the sender's scoreboard (include/lvlip_skb.h, "f2 on the
 * device: the scoreboard and the selective retransmit"): lvlip_sack_cpu reads
 * the SACK blocks of a batch of ACK frames and marks the queue entries they
 * cover, on the calling thread.  sack_kernels.hip leaves the same bytes.
 * lvlip_rtx_sack_cpu shares lvlip_rtx_cpu's frame path and lives beside it in
 * snd_cpu.c.
 *
 * The reference never reads an incoming block: tcp_parse_opts
 * (src/tcp_input.c:7-60) handles SACK-permitted only.  The blocks read here
 * are the ones its tcp_write_options writes (src/tcp_output.c:65-91).
 */
#include "tcp_hdr.h"

#define NONE 0xFFFFFFFFu

typedef struct sack_blk {
    uint64_t key; /* flow << 32 | l */
    uint64_t end; /* r; after the union the island's end */
} sack_blk;

static int blk_cmp(const void *a, const void *b)
{
    const uint64_t x = ((const sack_blk *)a)->key, y = ((const sack_blk *)b)->key;
    return x < y ? -1 : x > y;
}

/* The first four SACK blocks of the len frame bytes at p, as (left, right) in
 * host order in blk[0 .. 8); returns how many.  Only bytes inside the frame
 * are read. */
static uint32_t sack_blocks(const uint8_t *p, uint32_t len, uint32_t *blk)
{
    if (len < 34u || (p[14] >> 4) != 4u || (p[14] & 0x0fu) < 5u) return 0;
    const uint32_t th = 14u + 4u * (p[14] & 0x0fu);
    if (len < th + 20u) return 0;
    const uint32_t hl = p[th + 12u] >> 4;
    if (hl < 5u || len < th + 4u * hl) return 0;
    const uint8_t *o = p + th + 20u;
    const uint32_t optlen = 4u * hl - 20u;
    uint32_t pos = 0, nb = 0;
    while (pos < optlen && nb < 4u) {
        const uint32_t kind = o[pos];
        if (kind == 0u) break;
        if (kind == 1u) {
            pos++;
            continue;
        }
        if (pos + 1u >= optlen) break;
        const uint32_t l = o[pos + 1u];
        if (l < 2u || pos + l > optlen) break;
        if (kind == 5u && l >= 10u && l <= 34u && (l - 2u) % 8u == 0u) {
            for (uint32_t j = 0; j < (l - 2u) / 8u && nb < 4u; j++, nb++) {
                blk[2u * nb] = be32(o + pos + 2u + 8u * j);
                blk[2u * nb + 1u] = be32(o + pos + 6u + 8u * j);
            }
        }
        pos += l;
    }
    return nb;
}

int lvlip_sack_cpu(const lvlip_lro_flow *f, const lvlip_snd_flow *s, uint32_t nflows, const lvlip_lro_rec *rec,
                   const void *ack_base, const lvlip_frame_desc *ack_fd, uint32_t n, const void *base,
                   const lvlip_frame_desc *fd, uint8_t *sacked, lvlip_sack_result *res)
{
    if (nflows == 0 || n == 0) return LVLIP_OK;
    if (!f || !s || !rec || !ack_base || !ack_fd || !base || !fd || !sacked || !res) return LVLIP_EINVAL;
    if (n > LVLIP_MAX_BATCH || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    /* the block list holds the blocks of the counting frames, not four per record */
    size_t cap = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t blk[8];
        if (rec_ack_flow(&rec[i], f, nflows) != NONE)
            cap += sack_blocks((const uint8_t *)ack_base + ack_fd[i].offset, ack_fd[i].len, blk);
    }
    sack_blk *b = malloc((cap ? cap : 1u) * sizeof *b);
    if (!b) return LVLIP_ENOMEM;
    memset(res, 0, (size_t)nflows * sizeof *res);
    size_t m = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t k = rec_ack_flow(&rec[i], f, nflows);
        if (k == NONE) continue;
        uint32_t blk[8];
        const uint32_t nb = sack_blocks((const uint8_t *)ack_base + ack_fd[i].offset, ack_fd[i].len, blk);
        const uint32_t span = s[k].snd_nxt - s[k].snd_una;
        res[k].n_blocks += nb;
        for (uint32_t j = 0; j < nb; j++) {
            const uint32_t l = blk[2u * j] - s[k].snd_una, r = blk[2u * j + 1u] - s[k].snd_una;
            if (!(l < r && r <= span)) continue; /* D-SACK or stale, empty, beyond snd_nxt */
            res[k].n_valid++;
            if (r > res[k].high) res[k].high = r;
            b[m].key = ((uint64_t)k << 32) | l;
            b[m].end = r;
            m++;
        }
    }
    /* the union per flow: blocks that touch or overlap are one island, b[0 .. ni) */
    qsort(b, m, sizeof *b, blk_cmp);
    size_t ni = 0;
    for (size_t i = 0; i < m; i++) {
        if (ni && (b[ni - 1u].key >> 32) == (b[i].key >> 32) && (b[ni - 1u].end >= (b[i].key & 0xFFFFFFFFu))) {
            if (b[i].end > b[ni - 1u].end) b[ni - 1u].end = b[i].end;
        } else {
            b[ni++] = b[i];
        }
    }
    size_t ia = 0;
    for (uint32_t k = 0; k < nflows; k++) {
        while (ia < ni && (b[ia].key >> 32) < k) ia++;
        size_t ib = ia;
        while (ib < ni && (b[ib].key >> 32) == k) ib++;
        for (uint32_t i = 0; i < s[k].nseg; i++) {
            const uint32_t q = s[k].seg0 + i;
            const uint8_t *p = (const uint8_t *)base + fd[q].offset;
            uint32_t iplen, hl;
            if (ib > ia && rtx_frame_ok(p, fd[q].len, &iplen, &hl) && iplen > 20u + 4u * hl) {
                const uint32_t a = be32(p + 38) - s[k].snd_una;
                const uint64_t e = (uint64_t)a + (iplen - 20u - 4u * hl);
                /* the last island that starts at or before a */
                size_t lo = ia, hi = ib;
                while (lo < hi) {
                    const size_t mid = lo + (hi - lo) / 2u;
                    if ((b[mid].key & 0xFFFFFFFFu) <= a) lo = mid + 1u;
                    else hi = mid;
                }
                if (lo > ia && b[lo - 1u].end >= e) sacked[q] = 1;
            }
            res[k].n_sacked += sacked[q] == 1;
        }
        ia = ib;
    }
    free(b);
    return LVLIP_OK;
}
