/*
 * tso_frames.c — INTEGRATION.md §2a' as a plain C program: lvlip_tso_plan and
 * lvlip_tso_cpu (include/lvlip_skb.h) over the segmentation calls' shape list.
 *
 * For every MSS of the list, one call builds the frames of every combination
 * of segment count (1-3), tail length (1, mss - 1, mss), payload offset, frame
 * alignment and stride (frames that abut, and a 13-byte gap).  The payload and
 * the frame buffer are malloc'd at exactly the sizes the sends need, so a
 * sanitizer build (the CPU tests compile this file with the library's C
 * sources under -fsanitize=address,undefined) sees any byte read or written
 * outside them.  Every frame is then checked field by field against the
 * per-call drop-ins the reference's call sites use (ip_send_check's
 * arithmetic, tcp_udp_checksum), the payload slices against the source, and
 * every byte outside the frames against the canary.  Malformed sends must be
 * refused with the buffer untouched.
 *
 *   make -C examples && examples/build/tso_frames
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lvlip_csum.h"
#include "lvlip_skb.h"

#define CANARY 0xA5

static const uint16_t MSS[] = {1, 2, 15, 16, 17, 536, 1460, 8946};
static const uint32_t POFF[] = {0, 1, 7, 15};
static const uint32_t OMOD[] = {0, 1, 6, 10, 15};

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

static void template_hdr(uint8_t *h, uint32_t k)
{
    static const uint8_t base[54] = {
        0x0a, 0x1b, 0x2c, 0x3d, 0x4e, 0x5f, 0x00, 0x0c, 0x29, 0x6d, 0x50, 0x25, 0x08, 0x00, /* eth */
        0x45, 0x00, 0xde, 0xad, 0x12, 0x34, 0x40, 0x00, 0x40, 0x06, 0xbe, 0xef,             /* ip  */
        10, 0, 0, 200, 10, 0, 0, 100,          /* 10.0.0.200 -> 10.0.0.100: the seed loses its carry */
        0x9c, 0x41, 0x1f, 0x40, 0xff, 0xff, 0xff, 0x00, 0x01, 0x02, 0x03, 0x04,             /* tcp: seq wraps */
        0x50, 0x19, 0xad, 0xbd, 0xca, 0xfe, 0x00, 0x07};                                    /* ACK|PSH|FIN  */
    memcpy(h, base, 54);
    h[19] = (uint8_t)k; /* ip.id low byte: a different template per send */
    h[35] = (uint8_t)(k >> 3);
}

static void check_frames(const uint8_t *payload, const lvlip_tso_send *s, uint32_t n, const uint8_t *out,
                         uint64_t out_bytes, const lvlip_frame_desc *fd)
{
    uint8_t *covered = calloc(out_bytes ? out_bytes : 1, 1);
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t k = (s[j].len + s[j].mss - 1u) / s[j].mss;
        for (uint32_t i = 0; i < k; i++) {
            const uint32_t done = i * s[j].mss;
            const uint32_t dlen = s[j].len - done < s[j].mss ? s[j].len - done : s[j].mss;
            const uint64_t off = s[j].out_off + (uint64_t)i * s[j].stride;
            const uint8_t *f = out + off;
            uint8_t hdr[54], l4[20 + 65535];
            memset(covered + off, 1, 54u + dlen);
            CHECK(fd[s[j].seg0 + i].offset == off && fd[s[j].seg0 + i].len == 54u + dlen &&
                      fd[s[j].seg0 + i].reserved == 0,
                  "send %u seg %u: frame descriptor", j, i);
            /* the fields that change, put back: the rest must be the template */
            memcpy(hdr, f, 54);
            memcpy(hdr + 16, s[j].hdr + 16, 2);
            memcpy(hdr + 24, s[j].hdr + 24, 2);
            memcpy(hdr + 38, s[j].hdr + 38, 4);
            hdr[47] = s[j].hdr[47];
            memcpy(hdr + 50, s[j].hdr + 50, 2);
            CHECK(memcmp(hdr, s[j].hdr, 54) == 0, "send %u seg %u: copied header fields", j, i);
            CHECK(((uint32_t)f[16] << 8 | f[17]) == 40u + dlen, "send %u seg %u: ip.len", j, i);
            const uint32_t seq0 = (uint32_t)s[j].hdr[38] << 24 | (uint32_t)s[j].hdr[39] << 16 |
                                  (uint32_t)s[j].hdr[40] << 8 | s[j].hdr[41];
            const uint32_t seq = (uint32_t)f[38] << 24 | (uint32_t)f[39] << 16 | (uint32_t)f[40] << 8 | f[41];
            CHECK(seq == seq0 + done, "send %u seg %u: seq", j, i);
            CHECK(f[47] == (i + 1 == k ? s[j].hdr[47] : (s[j].hdr[47] & ~0x09)), "send %u seg %u: flags", j, i);
            CHECK(memcmp(f + 54, payload + s[j].payload_off + done, dlen) == 0, "send %u seg %u: payload", j, i);
            /* ip_send_check (src/ip_output.c:8-12) and tcp_v4_checksum (src/tcp.c:87-103) */
            memcpy(hdr, f + 14, 20);
            hdr[10] = hdr[11] = 0;
            uint16_t c = checksum(hdr, 20, 0), got;
            memcpy(&got, f + 24, 2);
            CHECK(c == got, "send %u seg %u: ip csum %04x != %04x", j, i, got, c);
            memcpy(l4, f + 34, 20u + dlen);
            l4[16] = l4[17] = 0;
            uint32_t sa, da;
            memcpy(&sa, f + 26, 4);
            memcpy(&da, f + 30, 4);
            c = (uint16_t)tcp_udp_checksum(sa, da, 6, l4, (uint16_t)(20u + dlen));
            memcpy(&got, f + 50, 2);
            CHECK(c == got, "send %u seg %u: tcp csum %04x != %04x", j, i, got, c);
        }
    }
    for (uint64_t b = 0; b < out_bytes; b++)
        if (!covered[b] && out[b] != CANARY) {
            CHECK(0, "byte %llu outside every frame was written", (unsigned long long)b);
            break;
        }
    free(covered);
}

static void run_mss(uint16_t mss)
{
    lvlip_tso_send *s = calloc(3 * 3 * 4 * 5 * 2, sizeof *s);
    uint32_t n = 0;
    uint64_t out_pos = 0, pay_pos = 0;
    for (uint32_t segs = 1; segs <= 3; segs++)
        for (uint32_t tk = 0; tk < 3; tk++) {
            const uint32_t tail = tk == 0 ? 1u : tk == 1 ? mss - 1u : mss;
            if (tail == 0 || (tk == 1 && tail == 1) || (tk == 2 && mss == 1)) continue; /* no duplicates */
            for (uint32_t p = 0; p < 4; p++)
                for (uint32_t o = 0; o < 5; o++)
                    for (uint32_t g = 0; g < 2; g++) {
                        lvlip_tso_send *t = &s[n];
                        t->len = (segs - 1u) * mss + tail;
                        t->mss = mss;
                        t->stride = 54u + mss + (g ? 13u : 0u);
                        t->payload_off = ((pay_pos + 15u) & ~15ull) + POFF[p];
                        pay_pos = t->payload_off + t->len;
                        t->out_off = ((out_pos + 15u) & ~15ull) + OMOD[o];
                        out_pos = t->out_off + (uint64_t)segs * t->stride;
                        template_hdr(t->hdr, n);
                        n++;
                    }
        }
    uint64_t out_bytes = 0;
    const uint32_t nseg = lvlip_tso_plan(s, n, &out_bytes);
    CHECK(nseg != 0xFFFFFFFFu && out_bytes <= out_pos, "mss %u: plan", mss);
    uint8_t *payload = malloc(pay_pos), *out = malloc(out_bytes);
    lvlip_frame_desc *fd = malloc(nseg * sizeof *fd);
    for (uint64_t b = 0; b < pay_pos; b++) payload[b] = (uint8_t)(b * 131u + (b >> 8) + mss);
    memset(out, CANARY, out_bytes);
    CHECK(lvlip_tso_cpu(payload, s, n, out, fd) == LVLIP_OK, "mss %u: lvlip_tso_cpu", mss);
    check_frames(payload, s, n, out, out_bytes, fd);
    /* without descriptors: the same bytes */
    uint8_t *out2 = malloc(out_bytes);
    memset(out2, CANARY, out_bytes);
    CHECK(lvlip_tso_cpu(payload, s, n, out2, NULL) == LVLIP_OK && memcmp(out, out2, out_bytes) == 0,
          "mss %u: fd == NULL", mss);
    free(out2);
    free(fd);
    free(out);
    free(payload);
    free(s);
}

static void run_malformed(void)
{
    uint8_t payload[64] = {0}, out[256], want[256];
    memset(out, CANARY, sizeof out);
    memset(want, CANARY, sizeof want);
    for (int k = 0; k < 9; k++) {
        lvlip_tso_send s;
        memset(&s, 0, sizeof s);
        s.len = 40;
        s.mss = 16;
        s.stride = 70;
        template_hdr(s.hdr, 0);
        switch (k) {
            case 0: s.len = 0; break;
            case 1: s.mss = 0; break;
            case 2: s.stride = 69; break;
            case 3: s.reserved = 1; break;
            case 4: s.hdr[12] = 0x86; break; /* ethertype */
            case 5: s.hdr[14] = 0x46; break; /* ihl 6 */
            case 6: s.hdr[23] = 17; break;   /* UDP */
            case 7: s.hdr[46] = 0x60; break; /* TCP options */
            default: break;                  /* valid, but not planned: seg0 wrong */
        }
        uint64_t ob = 1;
        if (k < 8) {
            CHECK(lvlip_tso_plan(&s, 1, &ob) == 0xFFFFFFFFu, "malformed %d: plan accepted it", k);
        } else {
            s.seg0 = 5;
        }
        CHECK(lvlip_tso_cpu(payload, &s, 1, out, NULL) == LVLIP_EINVAL, "malformed %d: cpu accepted it", k);
        CHECK(memcmp(out, want, sizeof out) == 0, "malformed %d: buffer written", k);
    }
    CHECK(lvlip_tso_cpu(NULL, NULL, 0, NULL, NULL) == LVLIP_OK, "n == 0");
    CHECK(lvlip_tso_plan(NULL, 0, NULL) == 0, "plan of nothing");
}

int main(void)
{
    for (size_t m = 0; m < sizeof MSS / sizeof MSS[0]; m++) run_mss(MSS[m]);
    run_malformed();
    if (fails) {
        fprintf(stderr, "tso_frames: %d checks failed\n", fails);
        return 1;
    }
    printf("tso_frames ok: %zu MSS values, plan + CPU frames, canaries intact\n", sizeof MSS / sizeof MSS[0]);
    return 0;
}
