// tests/sanitize/frames_san.cpp — TEST INFRASTRUCTURE ONLY: the host frame
// calls (level-ip_amd/csrc/frames_host.cpp) and the host context
// (csum_ctx.cpp) under ASan + UBSan and under TSan on the CPU, over the HIP
// stand-in of tests/sanitize/hip_emu.cpp (tests/test_sanitize_host.py).
//
// Every frame sits in an allocation that ends at its last byte.  Contexts have
// a 1 MiB arena (many pieces), once reading the arena in place and once through
// the copies (LVLIP_DIRECT_MAX=0); frames come scattered, in a slab registered
// for DMA and for zero-copy (shuffled order), as BUFLEN-long RX skbs, with a
// malformed frame in a late piece (every frame must come back untouched), and
// from three contexts on three threads at once.  One more slab per kind is
// registered from an address that is not 16-B aligned, with the bytes before
// it poisoned under ASan: no copy may start before a region's first byte.
// The piece table (below) then runs every host batch path at 4 KiB to 1 MiB
// arenas and pins each call's piece count and bytes moved.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "lvlip_csum.h"
#include "lvlip_skb.h"

#if defined(__SANITIZE_ADDRESS__)  // gcc's -fsanitize=address (the test builds with g++)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) __asan_poison_memory_region((p), (n))
#define UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#endif
#ifndef POISON
#define POISON(p, n) ((void)(p), (void)(n))
#define UNPOISON(p, n) ((void)(p), (void)(n))
#endif

extern "C" uint16_t oracle_checksum(const void* addr, int count, int start_sum);
extern "C" int oracle_tcp_udp_checksum(uint32_t saddr, uint32_t daddr, uint8_t proto, const uint8_t* data,
                                       uint16_t len);

static int g_fail = 0;
#define CHECK(c, ...)                                            \
    do {                                                         \
        if (!(c)) {                                              \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                        \
            fputc('\n', stderr);                                 \
            if (__atomic_add_fetch(&g_fail, 1, __ATOMIC_RELAXED) > 20) exit(1); \
        }                                                        \
    } while (0)

struct Rng {
    uint64_t s;
    uint32_t operator()() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

// Ethernet + IPv4 (ihl 5-7) + TCP (20-40 B header) or ICMP, 10.0.0.1-120
// (no carry lost in the reference's pseudo-header sum), fields junk.
static uint32_t frame_len(Rng& r, bool& tcp, uint32_t& ihl, uint32_t& l4hdr) {
    tcp = r() & 1u;
    ihl = 5u + r() % 3u;
    l4hdr = tcp ? 20u + 4u * (r() % 6u) : 8u;
    return 14u + ihl * 4u + l4hdr + r() % 1461u;
}
static void fill_frame(Rng& r, uint8_t* f, uint32_t flen, bool tcp, uint32_t ihl, uint32_t l4hdr) {
    const uint32_t iplen = flen - 14u;
    for (uint32_t b = 0; b < flen; ++b) f[b] = (uint8_t)r();
    f[12] = 0x08, f[13] = 0x00;
    uint8_t* ih = f + 14;
    ih[0] = (uint8_t)(0x40u | ihl), ih[2] = (uint8_t)(iplen >> 8), ih[3] = (uint8_t)iplen;
    ih[8] = 64, ih[9] = tcp ? 6 : 1;
    ih[12] = 10, ih[13] = 0, ih[14] = 0, ih[15] = (uint8_t)(1u + r() % 120u);
    ih[16] = 10, ih[17] = 0, ih[18] = 0, ih[19] = (uint8_t)(1u + r() % 120u);
    if (tcp) ih[ihl * 4u + 12u] = (uint8_t)((l4hdr / 4u) << 4);
}

// After TX: every frame's fields are the reference's (src/tcp.c:87-98,
// src/icmpv4.c:46-47, src/ip_output.c:8-12), and RX accepts every frame.
static void check_filled(lvlip_csum_ctx* ctx, std::vector<lvlip_frame>& fr, const char* what) {
    const uint32_t n = (uint32_t)fr.size();
    for (uint32_t i = 0; i < n; ++i) {
        uint8_t* ih = fr[i].head + 14;
        const uint32_t ihl = ih[0] & 15u, iplen = ((uint32_t)ih[2] << 8) | ih[3];
        CHECK(oracle_checksum(ih, (int)(ihl * 4u), 0) == 0, "%s: frame %u ip header", what, i);
        uint8_t* l4 = ih + ihl * 4u;
        const uint32_t l4len = iplen - ihl * 4u;
        if (ih[9] == 6) {
            uint16_t fld;
            memcpy(&fld, l4 + 16, 2);
            uint8_t save[2] = {l4[16], l4[17]};
            l4[16] = l4[17] = 0;
            uint32_t s, d;
            memcpy(&s, ih + 12, 4);
            memcpy(&d, ih + 16, 4);
            CHECK((uint16_t)oracle_tcp_udp_checksum(s, d, 6, l4, (uint16_t)l4len) == fld, "%s: frame %u tcp", what, i);
            l4[16] = save[0], l4[17] = save[1];
        } else {
            CHECK(oracle_checksum(l4, (int)l4len, 0) == 0, "%s: frame %u icmp", what, i);
        }
    }
    std::vector<uint8_t> v(n, 0);
    for (uint32_t flags = 0; flags <= LVLIP_RX_VERIFY_L4; ++flags) {
        std::fill(v.begin(), v.end(), 0);
        CHECK(lvlip_rx_verify(ctx, fr.data(), n, flags, v.data()) == LVLIP_OK, "%s: rx", what);
        uint32_t ok = 0;
        for (uint32_t i = 0; i < n; ++i) ok += v[i] == LVLIP_RX_OK;
        CHECK(ok == n, "%s: rx flags %u: %u of %u ok", what, flags, ok, n);
    }
}

static void scattered(lvlip_csum_ctx* ctx, uint32_t n, uint64_t seed) {
    Rng r{seed};
    std::vector<lvlip_frame> fr(n);
    for (uint32_t i = 0; i < n; ++i) {
        bool tcp;
        uint32_t ihl, l4hdr;
        const uint32_t flen = frame_len(r, tcp, ihl, l4hdr);
        uint8_t* f = (uint8_t*)malloc(flen);
        fill_frame(r, f, flen, tcp, ihl, l4hdr);
        fr[i] = {f, flen};
    }
    CHECK(lvlip_tx_checksum(ctx, fr.data(), n) == LVLIP_OK, "scattered tx");
    check_filled(ctx, fr, "scattered");
    // a malformed frame in a late piece: the earlier pieces were already
    // written, and must be restored
    fr[n - n / 8].head[14] = 0x65;
    for (auto& f : fr) f.head[24] ^= 0x5a;
    std::vector<uint8_t> snap;
    for (auto& f : fr) snap.insert(snap.end(), f.head, f.head + f.len);
    CHECK(lvlip_tx_checksum(ctx, fr.data(), n) == LVLIP_EINVAL, "malformed refused");
    size_t o = 0;
    uint32_t changed = 0;
    for (auto& f : fr) {
        changed += memcmp(snap.data() + o, f.head, f.len) != 0;
        o += f.len;
    }
    CHECK(changed == 0, "malformed: %u frames changed", changed);
    for (auto& f : fr) free(f.head);
}

// lead > 0: the region starts lead bytes into its allocation (not 16-B
// aligned), the first frame at its first byte, the lead bytes poisoned (ASan
// poisons whole 8-B granules from the allocation's start: lead 13 poisons
// the first 8, which a span rounded down to 16 from address 0 would read).
static void slab(lvlip_csum_ctx* ctx, uint32_t n, uint64_t seed, uint32_t reg, uint32_t lead = 0) {
    Rng r{seed};
    std::vector<uint32_t> len(n), off(n), ihl(n), l4h(n);
    std::vector<bool> tcp(n);
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        bool t;
        len[i] = frame_len(r, t, ihl[i], l4h[i]);
        tcp[i] = t;
        if (i || !lead) pos += r() % 24u;
        off[i] = (uint32_t)pos;
        pos += len[i];
    }
    uint8_t* raw = (uint8_t*)malloc(lead + pos);
    uint8_t* s = raw + lead;
    POISON(raw, lead);
    for (uint32_t i = 0; i < n; ++i) fill_frame(r, s + off[i], len[i], tcp[i], ihl[i], l4h[i]);
    CHECK(lvlip_csum_register(ctx, s, pos, reg) == LVLIP_OK, "register");
    std::vector<lvlip_frame> fr(n);
    for (uint32_t i = 0; i < n; ++i) fr[i] = {s + off[i], len[i]};
    for (uint32_t i = n - 1; i > 0; --i) std::swap(fr[i], fr[r() % (i + 1)]);
    CHECK(lvlip_tx_checksum(ctx, fr.data(), n) == LVLIP_OK, "slab tx reg %u", reg);
    check_filled(ctx, fr, reg == LVLIP_REG_DMA ? "slab dma" : "slab zerocopy");
    CHECK(lvlip_csum_unregister(ctx, s) == LVLIP_OK, "unregister");
    // as received skbs: each frame at the start of a BUFLEN (1600-B) buffer
    // whose end is the frame's end, garbage past the IP total length, some
    // total lengths past the buffer
    const uint32_t m = n < 3000 ? n : 3000, buflen = 1600;
    std::vector<uint8_t*> bufs(m);
    std::vector<lvlip_frame> sk(m);
    std::vector<uint8_t> want(m);
    for (uint32_t i = 0; i < m; ++i) {
        bufs[i] = (uint8_t*)malloc(buflen);
        for (uint32_t b = 0; b < buflen; ++b) bufs[i][b] = (uint8_t)r();
        const uint32_t l = len[i] < buflen ? len[i] : buflen;
        memcpy(bufs[i], s + off[i], l);
        want[i] = len[i] <= buflen ? LVLIP_RX_OK : LVLIP_RX_SHORT;
        if (i % 97 == 5) {  // total length past the buffer, the header checksum fixed up
            uint8_t* ih = bufs[i] + 14;
            ih[2] = 0x07, ih[3] = 0xd0, ih[10] = ih[11] = 0;
            const uint16_t c = oracle_checksum(ih, (int)((ih[0] & 15u) * 4u), 0);
            memcpy(ih + 10, &c, 2);
            want[i] = LVLIP_RX_SHORT;
        }
        sk[i] = {bufs[i], buflen};
    }
    std::vector<uint8_t> v(m, 0);
    CHECK(lvlip_rx_verify(ctx, sk.data(), m, LVLIP_RX_VERIFY_L4, v.data()) == LVLIP_OK, "rx skbs");
    for (uint32_t i = 0; i < m; ++i) CHECK(v[i] == want[i], "rx skb %u: %u want %u", i, v[i], want[i]);
    for (auto* b : bufs) free(b);
    UNPOISON(raw, lead);
    free(raw);
}

// The packet batches of the same context (csum_ctx.cpp): scattered exact-size
// packets at every alignment (lvlip_csum_batch_host: a gather per packet) and
// one flat buffer ending at its last packet's last byte (a gather per span).
static void packets(lvlip_csum_ctx* ctx, uint32_t n, uint64_t seed) {
    Rng r{seed};
    std::vector<uint8_t*> mem(n);
    std::vector<lvlip_csum_iov> iov(n);
    for (uint32_t i = 0; i < n; ++i) {
        const int32_t len = (r() % 97u == 0) ? -(int32_t)(r() % 5u) : (int32_t)(r() % 3001u);
        const uint32_t off = r() % 16u;
        const size_t bytes = off + (len > 0 ? (size_t)len : 0) + (len <= 0);
        mem[i] = (uint8_t*)malloc(bytes);
        for (size_t b = 0; b < bytes; ++b) mem[i][b] = (uint8_t)r();
        iov[i] = {mem[i] + off, len, r()};
    }
    std::vector<uint16_t> out(n, 0);
    CHECK(lvlip_csum_batch_host(ctx, iov.data(), n, out.data()) == LVLIP_OK, "batch_host");
    for (uint32_t i = 0; i < n; ++i)
        CHECK(out[i] == oracle_checksum(iov[i].ptr, iov[i].len, (int)iov[i].start_sum), "batch_host %u", i);
    for (auto* p : mem) free(p);
    std::vector<lvlip_csum_desc> d(n);
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        pos += r() % 40u;
        d[i] = {pos, (int32_t)(r() % 1601u), r()};
        pos += (uint64_t)d[i].len;
    }
    uint8_t* base = (uint8_t*)malloc(pos ? pos : 1);
    for (uint64_t b = 0; b < pos; ++b) base[b] = (uint8_t)r();
    CHECK(lvlip_csum_batch_host_flat(ctx, base, pos, d.data(), n, out.data()) == LVLIP_OK, "batch_host_flat");
    for (uint32_t i = 0; i < n; ++i)
        CHECK(out[i] == oracle_checksum(base + d[i].offset, d[i].len, (int)d[i].start_sum), "flat %u", i);
    free(base);
}

// ---- The piece table ----
// Every host batch path cuts its call into device pieces; how many, and how
// many bytes they move, is part of each path's behaviour.  Each case below
// checks its results byte for byte as above and the deltas of
// lvlip_ctx_stats.pieces and h2d_bytes across the call against kExpect: the
// numbers this program printed when it was built from the sources before the
// six loops were merged into one.  Counts, not timings: they match exactly, in
// both launch forms (pieces read in place, and through the copies).
struct Expect {
    const char* name;
    uint64_t pieces, h2d_bytes;
};
static const Expect kExpect[] = {
    {"a4k/pk_scattered", 298, 917856},
    {"a4k/flat_dense", 303, 921504},
    {"a4k/flat_shuffled", 298, 917856},
    {"a4k/pk_tiny", 69, 278464},
    {"a4k/iov_dma_dense", 308, 921481},
    {"a4k/iov_dma_shuffled", 298, 917856},
    {"a4k/iov_zc_dense", 308, 921481},
    {"a4k/iov_zc_shuffled", 297, 913264},
    {"a4k/fr_scat_tx", 131, 471504},
    {"a4k/fr_scat_rx", 12, 47936},
    {"a4k/fr_scat_rxl4", 131, 471504},
    {"a4k/fr_scat_tx_bad", 115, 415072},
    {"a4k/fr_dma_tx", 126, 462490},
    {"a4k/fr_dma_rx", 12, 47920},
    {"a4k/fr_dma_rxl4", 126, 462490},
    {"a4k/fr_dma_shuf_tx", 127, 460784},
    {"a4k/fr_dma_shuf_rx", 12, 47920},
    {"a4k/fr_dma_shuf_rxl4", 127, 460784},
    {"a4k/fr_dma_tx_bad", 112, 411088},
    {"a4k/fr_zc_tx", 136, 486345},
    {"a4k/fr_zc_rx", 133, 480059},
    {"a4k/fr_zc_rxl4", 136, 486345},
    {"a4k/fr_zc_shuf_tx", 133, 480059},
    {"a4k/fr_zc_shuf_rx", 133, 480059},
    {"a4k/fr_zc_shuf_rxl4", 133, 480059},
    {"a4k/fr_zc_tx_bad", 121, 434859},
    {"a256k/pk_scattered", 36, 4569440},
    {"a256k/flat_dense", 36, 4604288},
    {"a256k/flat_shuffled", 36, 4569440},
    {"a256k/pk_tiny", 3, 278544},
    {"a256k/iov_dma_dense", 61, 4604421},
    {"a256k/iov_dma_shuffled", 36, 4569440},
    {"a256k/iov_zc_dense", 61, 4604421},
    {"a256k/iov_zc_shuffled", 18, 4547124},
    {"a256k/fr_scat_tx", 21, 2364464},
    {"a256k/fr_scat_rx", 4, 239488},
    {"a256k/fr_scat_rxl4", 21, 2364464},
    {"a256k/fr_scat_tx_bad", 20, 2332480},
    {"a256k/fr_dma_tx", 21, 2411649},
    {"a256k/fr_dma_rx", 4, 239504},
    {"a256k/fr_dma_rxl4", 21, 2411649},
    {"a256k/fr_dma_shuf_tx", 21, 2399712},
    {"a256k/fr_dma_shuf_rx", 4, 239504},
    {"a256k/fr_dma_shuf_rxl4", 21, 2399712},
    {"a256k/fr_dma_tx_bad", 20, 2336239},
    {"a256k/fr_zc_tx", 21, 2413524},
    {"a256k/fr_zc_rx", 21, 2378194},
    {"a256k/fr_zc_rxl4", 21, 2413524},
    {"a256k/fr_zc_shuf_tx", 21, 2378194},
    {"a256k/fr_zc_shuf_rx", 21, 2378194},
    {"a256k/fr_zc_shuf_rxl4", 21, 2378194},
    {"a256k/fr_zc_tx_bad", 20, 2331365},
    {"a1m/pk_scattered", 5, 4569440},
    {"a1m/flat_dense", 5, 4604680},
    {"a1m/flat_shuffled", 5, 4569440},
    {"a1m/pk_tiny", 1, 278544},
    {"a1m/iov_dma_dense", 48, 4604481},
    {"a1m/iov_dma_shuffled", 5, 4569440},
    {"a1m/iov_zc_dense", 48, 4604481},
    {"a1m/iov_zc_shuffled", 5, 4547124},
    {"a1m/fr_scat_tx", 3, 2364464},
    {"a1m/fr_scat_rx", 1, 239488},
    {"a1m/fr_scat_rxl4", 3, 2364464},
    {"a1m/fr_scat_tx_bad", 3, 2364464},
    {"a1m/fr_dma_tx", 3, 2411708},
    {"a1m/fr_dma_rx", 1, 239504},
    {"a1m/fr_dma_rxl4", 3, 2411708},
    {"a1m/fr_dma_shuf_tx", 3, 2399712},
    {"a1m/fr_dma_shuf_rx", 1, 239504},
    {"a1m/fr_dma_shuf_rxl4", 3, 2399712},
    {"a1m/fr_dma_tx_bad", 3, 2411708},
    {"a1m/fr_zc_tx", 3, 2413613},
    {"a1m/fr_zc_rx", 3, 2378194},
    {"a1m/fr_zc_rxl4", 3, 2413613},
    {"a1m/fr_zc_shuf_tx", 3, 2378194},
    {"a1m/fr_zc_shuf_rx", 3, 2378194},
    {"a1m/fr_zc_shuf_rxl4", 3, 2378194},
    {"a1m/fr_zc_tx_bad", 3, 2413613},
    {"fail3/pk_scattered", 3, 391792},
    {"fail3/flat_dense", 3, 391185},
    {"fail3/flat_shuffled", 3, 391792},
    {"fail3/iov_dma_dense", 3, 468388},
    {"fail3/iov_dma_shuffled", 3, 391792},
    {"fail3/iov_zc_dense", 3, 468388},
    {"fail3/iov_zc_shuffled", 3, 782696},
    {"fail3/fr_scat_tx", 3, 113584},
    {"fail3/fr_dma_tx", 3, 113937},
    {"fail3/fr_zc_tx", 3, 112553},
};

struct Count {
    lvlip_csum_ctx* c;
    lvlip_ctx_stats s0;
    explicit Count(lvlip_csum_ctx* ctx) : c(ctx) { lvlip_csum_ctx_stats(c, &s0); }
    void is(const char* cfg, const char* what) {
        lvlip_ctx_stats s1;
        lvlip_csum_ctx_stats(c, &s1);
        const uint64_t p = s1.pieces - s0.pieces, h = s1.h2d_bytes - s0.h2d_bytes;
        char name[64];
        snprintf(name, sizeof name, "%s/%s", cfg, what);
        printf("    {\"%s\", %llu, %llu},\n", name, (unsigned long long)p, (unsigned long long)h);
        for (const Expect& e : kExpect)
            if (!strcmp(e.name, name)) {
                CHECK(p == e.pieces && h == e.h2d_bytes, "%s: %llu pieces, %llu bytes; expected %llu, %llu", name,
                      (unsigned long long)p, (unsigned long long)h, (unsigned long long)e.pieces,
                      (unsigned long long)e.h2d_bytes);
                return;
            }
        CHECK(false, "%s: not in the piece table", name);
    }
};

template <class T>
static void shuffle(Rng& r, std::vector<T>& v) {
    for (size_t i = v.size() - 1; i > 0; --i) std::swap(v[i], v[r() % (i + 1)]);
}

// n packets of up to maxlen bytes (a few empty or negative) in one buffer that
// ends at the last one's last byte, in address order with small gaps.
struct Flat {
    uint8_t* base = nullptr;
    uint64_t bytes = 0;
    std::vector<lvlip_csum_desc> d;
};
static Flat make_flat(Rng& r, uint32_t n, uint32_t maxlen) {
    Flat f;
    f.d.resize(n);
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        pos += r() % 40u;
        const int32_t len = (r() % 97u == 0) ? -(int32_t)(r() % 5u) : (int32_t)(r() % (maxlen + 1u));
        f.d[i] = {pos, len, r()};
        pos += len > 0 ? (uint64_t)len : 0u;
    }
    f.bytes = pos;
    f.base = (uint8_t*)malloc(pos);
    CHECK(((uintptr_t)f.base & 15u) == 0, "flat buffer not 16-B aligned");
    for (uint64_t b = 0; b < pos; ++b) f.base[b] = (uint8_t)r();
    return f;
}
static void run_flat(lvlip_csum_ctx* ctx, const Flat& f, const std::vector<lvlip_csum_desc>& d, bool iov,
                     const char* cfg, const char* what, int want = LVLIP_OK) {
    const uint32_t n = (uint32_t)d.size();
    std::vector<uint16_t> out(n, 0);
    std::vector<lvlip_csum_iov> v(iov ? n : 0);
    for (uint32_t i = 0; iov && i < n; ++i) v[i] = {f.base + d[i].offset, d[i].len, d[i].start_sum};
    Count cnt(ctx);
    const int rc = iov ? lvlip_csum_batch_host(ctx, v.data(), n, out.data())
                       : lvlip_csum_batch_host_flat(ctx, f.base, f.bytes, d.data(), n, out.data());
    CHECK(rc == want, "%s/%s: rc %d", cfg, what, rc);
    cnt.is(cfg, what);
    for (uint32_t i = 0; rc == LVLIP_OK && i < n; ++i)
        CHECK(out[i] == oracle_checksum(f.base + d[i].offset, d[i].len, (int)d[i].start_sum), "%s/%s: packet %u", cfg,
              what, i);
}

// The packet paths: the gather (scattered packets, and a pile of tiny ones
// that fills a piece's descriptors before its bytes), the flat call dense and
// shuffled, and the iov call over a DMA and a zero-copy region, dense and
// shuffled.  fail: LVLIP_FAIL_PIECE is set, every call fails at its 3rd piece.
static void table_packets(lvlip_csum_ctx* ctx, const char* cfg, uint32_t n, uint32_t maxlen, uint64_t seed,
                          bool fail) {
    Rng r{seed};
    const int want = fail ? LVLIP_EHIP : LVLIP_OK;
    Flat f = make_flat(r, n, maxlen);
    std::vector<lvlip_csum_desc> shuf = f.d;
    shuffle(r, shuf);
    run_flat(ctx, f, shuf, true, cfg, "pk_scattered", want);
    run_flat(ctx, f, f.d, false, cfg, "flat_dense", want);
    run_flat(ctx, f, shuf, false, cfg, "flat_shuffled", want);
    if (!fail) {
        Flat tiny = make_flat(r, 10000, 40);
        run_flat(ctx, tiny, tiny.d, true, cfg, "pk_tiny");
        free(tiny.base);
    }
    for (uint32_t reg : {(uint32_t)LVLIP_REG_DMA, (uint32_t)LVLIP_REG_ZEROCOPY}) {
        const bool dma = reg == LVLIP_REG_DMA;
        CHECK(lvlip_csum_register(ctx, f.base, f.bytes, reg) == LVLIP_OK, "register");
        run_flat(ctx, f, f.d, true, cfg, dma ? "iov_dma_dense" : "iov_zc_dense", want);
        run_flat(ctx, f, shuf, true, cfg, dma ? "iov_dma_shuffled" : "iov_zc_shuffled", want);
        CHECK(lvlip_csum_unregister(ctx, f.base) == LVLIP_OK, "unregister");
    }
    free(f.base);
}

// n filled frames, each in its own allocation (slab false) or in one buffer
// in address order with small gaps.
struct FrameSet {
    uint8_t* slab = nullptr;
    uint64_t bytes = 0;
    std::vector<lvlip_frame> fr;
};
static FrameSet make_frames(Rng& r, uint32_t n, bool slab) {
    FrameSet s;
    s.fr.resize(n);
    std::vector<uint32_t> len(n), off(n), ihl(n), l4h(n);
    std::vector<bool> tcp(n);
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        bool t;
        len[i] = frame_len(r, t, ihl[i], l4h[i]);
        tcp[i] = t;
        pos += r() % 24u;
        off[i] = (uint32_t)pos;
        pos += len[i];
    }
    if (slab) {
        s.bytes = pos;
        s.slab = (uint8_t*)malloc(pos);
        CHECK(((uintptr_t)s.slab & 15u) == 0, "slab not 16-B aligned");
    }
    for (uint32_t i = 0; i < n; ++i) {
        uint8_t* f = slab ? s.slab + off[i] : (uint8_t*)malloc(len[i]);
        fill_frame(r, f, len[i], tcp[i], ihl[i], l4h[i]);
        s.fr[i] = {f, len[i]};
    }
    return s;
}
static void free_frames(FrameSet& s) {
    if (s.slab) free(s.slab);
    else
        for (auto& f : s.fr) free(f.head);
}
static void run_rx(lvlip_csum_ctx* ctx, std::vector<lvlip_frame>& fr, uint32_t flags, const char* cfg,
                   const char* what) {
    const uint32_t n = (uint32_t)fr.size();
    std::vector<uint8_t> v(n, 0xee);
    Count cnt(ctx);
    CHECK(lvlip_rx_verify(ctx, fr.data(), n, flags, v.data()) == LVLIP_OK, "%s/%s", cfg, what);
    cnt.is(cfg, what);
    uint32_t ok = 0;
    for (uint32_t i = 0; i < n; ++i) ok += v[i] == LVLIP_RX_OK;
    CHECK(ok == n, "%s/%s: %u of %u ok", cfg, what, ok, n);
}
// A TX call that must fail with `want` and leave every frame as it was.
static void run_tx_refused(lvlip_csum_ctx* ctx, std::vector<lvlip_frame>& fr, int want, const char* cfg,
                           const char* what) {
    std::vector<uint8_t> snap;
    for (auto& f : fr) snap.insert(snap.end(), f.head, f.head + f.len);
    Count cnt(ctx);
    const int rc = lvlip_tx_checksum(ctx, fr.data(), (uint32_t)fr.size());
    CHECK(rc == want, "%s/%s: rc %d", cfg, what, rc);
    cnt.is(cfg, what);
    size_t o = 0;
    uint32_t changed = 0;
    for (auto& f : fr) {
        changed += memcmp(snap.data() + o, f.head, f.len) != 0;
        o += f.len;
    }
    CHECK(changed == 0, "%s/%s: %u frames changed", cfg, what, changed);
}
// TX, the two RX calls, then TX with a malformed frame in a late piece (the
// earlier pieces' stores are undone), over `fr` and, when given, over the
// same frames in shuffled order.
static void run_frames(lvlip_csum_ctx* ctx, FrameSet& s, bool shuffled, const char* cfg, const char* tag, Rng& r,
                       bool fail) {
    char what[48];
    auto name = [&](const char* call, bool sh) {
        snprintf(what, sizeof what, "%s%s_%s", tag, sh ? "_shuf" : "", call);
        return what;
    };
    const uint32_t n = (uint32_t)s.fr.size();
    if (fail) {  // LVLIP_FAIL_PIECE=3: the first two pieces' stores are undone
        for (auto& f : s.fr) f.head[24] ^= 0x5a;
        run_tx_refused(ctx, s.fr, LVLIP_EHIP, cfg, name("tx", false));
        return;
    }
    std::vector<lvlip_frame> sh = s.fr;
    shuffle(r, sh);
    for (int k = 0; k < (shuffled ? 2 : 1); ++k) {
        std::vector<lvlip_frame>& fr = k ? sh : s.fr;
        for (auto& f : fr) f.head[24] ^= 0x5a;  // the header checksum is stale again
        Count cnt(ctx);
        CHECK(lvlip_tx_checksum(ctx, fr.data(), n) == LVLIP_OK, "%s/%s", cfg, name("tx", k));
        cnt.is(cfg, name("tx", k));
        run_rx(ctx, fr, 0, cfg, name("rx", k));
        run_rx(ctx, fr, LVLIP_RX_VERIFY_L4, cfg, name("rxl4", k));
        check_filled(ctx, fr, what);
    }
    s.fr[n - n / 8].head[14] = 0x65;
    for (auto& f : s.fr) f.head[24] ^= 0x5a;
    run_tx_refused(ctx, s.fr, LVLIP_EINVAL, cfg, name("tx_bad", false));
}
static void table_frames(lvlip_csum_ctx* ctx, const char* cfg, uint32_t n, uint64_t seed, bool fail) {
    Rng r{seed};
    FrameSet sc = make_frames(r, n, false);
    run_frames(ctx, sc, false, cfg, "fr_scat", r, fail);
    free_frames(sc);
    for (uint32_t reg : {(uint32_t)LVLIP_REG_DMA, (uint32_t)LVLIP_REG_ZEROCOPY}) {
        FrameSet sl = make_frames(r, n, true);
        CHECK(lvlip_csum_register(ctx, sl.slab, sl.bytes, reg) == LVLIP_OK, "register");
        run_frames(ctx, sl, true, cfg, reg == LVLIP_REG_DMA ? "fr_dma" : "fr_zc", r, fail);
        CHECK(lvlip_csum_unregister(ctx, sl.slab) == LVLIP_OK, "unregister");
        free_frames(sl);
    }
}

// The iov call over a registered region, 4 KiB arena: one packet of 4092 B at
// offset 8 fits the arena gathered (4096 B) but not as a span (bytes 0 to
// 4112), alone and as the last of 301 with earlier pieces in flight.  The
// dense path must leave the whole call to the gather.
static void iov_span_refused(lvlip_csum_ctx* ctx) {
    Rng r{77};
    for (uint32_t small : {0u, 300u}) {
        const uint64_t bytes = 8u + 4092u + small * 64u;
        uint8_t* base = (uint8_t*)malloc(bytes);
        CHECK(((uintptr_t)base & 15u) == 0, "region not 16-B aligned");
        for (uint64_t b = 0; b < bytes; ++b) base[b] = (uint8_t)r();
        std::vector<lvlip_csum_iov> v;
        for (uint32_t i = 0; i < small; ++i) v.push_back({base + 64u * i, (int32_t)(1u + r() % 60u), r()});
        v.push_back({base + 64u * small + 8u, 4092, r()});
        CHECK(lvlip_csum_register(ctx, base, bytes, LVLIP_REG_DMA) == LVLIP_OK, "register");
        std::vector<uint16_t> out(v.size(), 0);
        CHECK(lvlip_csum_batch_host(ctx, v.data(), (uint32_t)v.size(), out.data()) == LVLIP_OK, "iov span %u", small);
        for (size_t i = 0; i < v.size(); ++i)
            CHECK(out[i] == oracle_checksum(v[i].ptr, v[i].len, (int)v[i].start_sum), "iov span %u: packet %zu", small,
                  i);
        CHECK(lvlip_csum_unregister(ctx, base) == LVLIP_OK, "unregister");
        free(base);
    }
}

static void piece_table() {
    struct Cfg {
        const char* name;
        size_t arena;
        const char *piece_max, *first_piece, *fail_piece;
        uint32_t n, maxlen;
    };
    const Cfg cfgs[] = {
        {"a4k", 4096, nullptr, nullptr, nullptr, 600, 3000},
        {"a256k", 256u << 10, "131072", "16384", nullptr, 3000, 3000},
        {"a1m", 1u << 20, nullptr, nullptr, nullptr, 3000, 3000},
        {"fail3", 256u << 10, "131072", "16384", "3", 3000, 3000},
    };
    auto env = [](const char* k, const char* v) { v ? setenv(k, v, 1) : unsetenv(k); };
    for (const Cfg& g : cfgs) {
        env("LVLIP_PIECE_MAX", g.piece_max);
        env("LVLIP_FIRST_PIECE", g.first_piece);
        env("LVLIP_FAIL_PIECE", g.fail_piece);
        lvlip_csum_ctx* ctx = nullptr;
        CHECK(lvlip_csum_ctx_create(&ctx, 0, g.arena) == LVLIP_OK, "ctx_create");
        CHECK(lvlip_csum_ctx_set_cpu_max(ctx, 0) == LVLIP_OK, "cpu_max");
        table_packets(ctx, g.name, g.n, g.maxlen, 21, g.fail_piece != nullptr);
        table_frames(ctx, g.name, g.n, 31, g.fail_piece != nullptr);
        if (g.arena == 4096) iov_span_refused(ctx);
        CHECK(lvlip_csum_ctx_destroy(ctx) == LVLIP_OK, "destroy");
    }
    env("LVLIP_PIECE_MAX", nullptr);
    env("LVLIP_FIRST_PIECE", nullptr);
    env("LVLIP_FAIL_PIECE", nullptr);
}

int main() {
    setenv("LVLIP_CPU_MAX", "0", 1);  // every call takes the device path, whatever its size
    for (int direct = 0; direct < 2; ++direct) {
        // direct: pieces read in place; else through the H2D / D2H copies.
        // And the host steps on the pool (LVLIP_INLINE_MAX 0) or, for calls
        // of up to 32 768 items, on the calling thread (the default)
        setenv("LVLIP_DIRECT_MAX", direct ? "4194304" : "0", 1);
        setenv("LVLIP_INLINE_MAX", direct ? "32768" : "0", 1);
        lvlip_csum_ctx* ctx = nullptr;
        CHECK(lvlip_csum_ctx_create(&ctx, 0, 1u << 20) == LVLIP_OK, "ctx_create");
        scattered(ctx, 12000, 1 + direct);
        packets(ctx, 12000, 7 + direct);
        slab(ctx, 12000, 3 + direct, LVLIP_REG_DMA);
        slab(ctx, 6000, 5 + direct, LVLIP_REG_ZEROCOPY);
        slab(ctx, 4000, 9 + direct, LVLIP_REG_DMA, 13);
        slab(ctx, 4000, 13 + direct, LVLIP_REG_ZEROCOPY, 13);
        CHECK(lvlip_csum_ctx_destroy(ctx) == LVLIP_OK, "destroy");
        piece_table();
    }
    unsetenv("LVLIP_DIRECT_MAX");
    setenv("LVLIP_INLINE_MAX", "0", 1);  // the threads below use their pools
    // one context per thread, at once (the reference's core, IPC and timer
    // threads, src/main.c:83-89)
    std::vector<std::thread> th;
    for (int t = 0; t < 3; ++t)
        th.emplace_back([t] {
            lvlip_csum_ctx* c = nullptr;
            CHECK(lvlip_csum_ctx_create(&c, 0, 1u << 20) == LVLIP_OK, "thread ctx");
            scattered(c, 4000, 100 + t);
            CHECK(lvlip_csum_ctx_destroy(c) == LVLIP_OK, "thread destroy");
        });
    for (auto& x : th) x.join();
    if (g_fail) {
        fprintf(stderr, "%d failures\n", g_fail);
        return 1;
    }
    printf("frames_san: all checks passed\n");
    return 0;
}
