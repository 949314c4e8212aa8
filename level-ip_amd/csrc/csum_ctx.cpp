// csum_ctx.cpp — Group 3 of include/lvlip_csum.h: host-resident batches.
//
// level-ip's packets live in malloc'd skb heads (src/skbuff.c:5-20) at offsets
// 14 (IPv4 header, include/ip.h:47-50) and 34 (TCP/ICMP, include/tcp.h:224-227),
// i.e. 2 mod 4.  The context's slots, arenas and streams are described in
// ctx_impl.h; the host frame calls over the same context are frames_host.cpp.
//
// One context belongs to one thread at a time (no locks on the hot path):
// the reference calls checksum() from the core, IPC and timer threads
// (src/main.c:83-89, src/timer.c:74), so each gets its own context.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "ctx_impl.h"

namespace {

constexpr size_t kDefaultArena = 64ull << 20;
constexpr uint64_t kDirectMax = 4ull << 20;  // measured: DESIGN.md §5
constexpr uint64_t kPieceMax = 32ull << 20;  // measured: DESIGN.md §5
constexpr uint64_t kBlockMin = 4ull << 20;   // ~80 us of PCIe: DESIGN.md §9

}  // namespace

namespace lvlip_ctx {

int fail(lvlip_csum_ctx* c, hipError_t e, const char* what, int code) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", what, hipGetErrorString(e));
    if (c) snprintf(c->err, sizeof c->err, "%s", msg);
    lvlip_set_last_hip_error(msg);  // what lvlip_last_hip_error() returns on this thread
    fprintf(stderr, "lvlip_csum: %s\n", msg);
    return code;
}

int drain(lvlip_csum_ctx* c, Slot& s) {
    if (!s.busy) return LVLIP_OK;
    hipError_t e = hipSuccess;
    if (s.sleep) {
        // hipEventSynchronize spins (with or without hipEventBlockingSync, as
        // measured: DESIGN.md §9), so a long piece is polled between 20-us sleeps
        const timespec nap{0, 20000};
        while ((e = hipEventQuery(s.done)) == hipErrorNotReady) nanosleep(&nap, nullptr);
    }
    if (e == hipSuccess) e = hipEventSynchronize(s.done);
    s.busy = false;
    if (e != hipSuccess) return fail(c, e, "hipEventSynchronize");
    memcpy(s.user_out, s.h_out, s.out_bytes);
    return LVLIP_OK;
}

int count_piece(lvlip_csum_ctx* c, uint64_t bytes) {
    c->stats.pieces++;
    c->stats.h2d_bytes += bytes;
    if (c->fail_piece && ++c->call_pieces == c->fail_piece)
        return fail(c, hipErrorLaunchFailure, "injected failure (LVLIP_FAIL_PIECE)");
    return LVLIP_OK;
}

int arm_slot(lvlip_csum_ctx* c, Slot& s, void* user_out, size_t out_bytes, uint64_t piece_bytes) {
    const hipError_t e = hipEventRecord(s.done, s.stream);
    if (e != hipSuccess) return fail(c, e, "hipEventRecord");
    s.sleep = c->block_min && piece_bytes >= c->block_min;
    s.user_out = user_out;
    s.out_bytes = out_bytes;
    s.busy = true;
    return LVLIP_OK;
}

// Two slots' copies issued on their own streams run side by side, share the
// link and finish together; each slot's kernel and result copy then ran with
// the link idle, 8.5 % of a registered batch's time (the pipeline's trace,
// DESIGN.md §5).  Each piece's copy now waits for the previous piece's (the
// other slot's) copy event, so the copies run one after the other in issue
// order and each piece is summed while the next one's copy runs.  The first
// piece of a call waits for nothing: a cross-stream wait in front of a
// call's only piece cost small batches up to ~0.5 ms (a copy stream shared
// by both slots, tried first, did that for every piece).
int h2d_ordered(lvlip_csum_ctx* c, Slot& s, void* dst, const void* src, size_t n, const char* what) {
    hipError_t e;
    if (c->copy_order && c->last_copy && c->last_copy != &s &&
        (e = hipStreamWaitEvent(s.stream, c->last_copy->copied, 0)) != hipSuccess)
        return fail(c, e, "hipStreamWaitEvent");
    if ((e = hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s.stream)) != hipSuccess) return fail(c, e, what);
    if (c->copy_order) {
        if ((e = hipEventRecord(s.copied, s.stream)) != hipSuccess) return fail(c, e, "hipEventRecord");
        c->last_copy = &s;
    }
    return LVLIP_OK;
}

const Region* find_region(const lvlip_csum_ctx* c, const void* p, uint64_t len) {
    const uint8_t* a = (const uint8_t*)p;
    for (const Region& r : c->regions)
        if (a >= r.host && a + len <= r.host + r.bytes) return &r;
    return nullptr;
}

}  // namespace lvlip_ctx

namespace {

using namespace lvlip_ctx;

// An environment variable as a number clamped to [lo, hi]; dflt when unset.
long long env_ll(const char* name, long long dflt, long long lo, long long hi) {
    const char* e = getenv(name);
    const long long v = e ? atoll(e) : dflt;
    return v < lo ? lo : v > hi ? hi : v;
}

void free_slot(Slot& s) {
    if (s.h_bytes) (void)hipHostFree(s.h_bytes);
    if (s.h_desc) (void)hipHostFree(s.h_desc);
    if (s.h_out) (void)hipHostFree(s.h_out);
    if (s.d_bytes) (void)hipFree(s.d_bytes);
    if (s.d_desc) (void)hipFree(s.d_desc);
    if (s.d_out) (void)hipFree(s.d_out);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.copied) (void)hipEventDestroy(s.copied);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    s = Slot{};
}

// A packet piece through the device (launch_piece): count checksums of 2 B
// each, the bytes' H2D ordered behind the previous piece's.
int launch_packets(lvlip_csum_ctx* c, Slot& s, uint64_t bytes, uint32_t count, uint16_t* user_out,
                   const uint8_t* src = nullptr, const uint8_t* dev_base = nullptr) {
    lvlip_launch_cfg cfg{};
    cfg.kernel = LVLIP_KERNEL_AUTO;  // the piece's average length picks the kernel
    cfg.len_hint = (int32_t)(bytes / count > 0x7fffffffull ? 0x7fffffff : bytes / count);
    if (dev_base && cfg.len_hint >= 896) {
        // packets read in place over PCIe: the flat sweep (U 8) reads them
        // faster than the stream kernel AUTO picks from 896 B for HBM
        // (scripts/lab_zerocopy.py)
        cfg.kernel = LVLIP_KERNEL_FLAT;
        cfg.unroll = 8;
    }
    return launch_piece(c, s, bytes, count, sizeof(uint16_t), true, user_out, src, dev_base,
                        [&](const uint8_t* base, const lvlip_csum_desc* d, uint16_t* out) {
                            return lvlip_csum_batch_dev_ex(base, d, count, out, s.stream, &cfg);
                        });
}

// The code of the first item (in batch order) that `check` refuses, or
// LVLIP_OK, checked on the pool threads: the host calls' up-front passes over
// a whole batch ran on the calling thread before the first piece, 1-2 ms per
// 1M descriptors with the link idle.
template <class F>
int first_failure(lvlip_csum_ctx* c, uint32_t n, const F& check) {
    std::atomic<uint64_t> first{~0ull};  // (item << 8) | -code of the earliest refusal seen
    parallel_ranges(c, n, 65536, [&first, &check](uint64_t lo, uint64_t hi) {
        for (uint64_t q = lo; q < hi; ++q) {
            const int r = check((uint32_t)q);
            if (r == LVLIP_OK) continue;
            const uint64_t key = (q << 8) | (uint64_t)(-r);
            uint64_t cur = first.load(std::memory_order_relaxed);
            while (key < cur && !first.compare_exchange_weak(cur, key, std::memory_order_relaxed)) {
            }
            return;  // the rest of this range comes later in batch order
        }
    });
    const uint64_t f = first.load(std::memory_order_relaxed);
    return f == ~0ull ? LVLIP_OK : -(int)(f & 0xffu);
}

// The packets of a host call on the calling thread (cpu_max): Group 1's
// checksum() per packet, the reference's own arithmetic (src/utils.c:40-55).
template <class Ptr, class Len, class Seed>
int cpu_batch(lvlip_csum_ctx* c, uint32_t n, uint16_t* out, const Ptr& ptr_of, const Len& len_of,
              const Seed& seed_of) {
    c->stats.cpu_calls++;
    for (uint32_t q = 0; q < n; ++q) {
        const int32_t l = len_of(q);
        out[q] = checksum(l > 0 ? (void*)ptr_of(q) : nullptr, l, (int)seed_of(q));
    }
    return LVLIP_OK;
}

// Gathers n packets (ptr_of, len_of, seed_of) into the pinned arena, each at
// the next 16-B aligned offset, piece by piece (the scattered path of
// lvlip_csum_batch_host, and the flat call's path for descriptors that do not
// cover their span densely in order).
template <class Ptr, class Len, class Seed>
int gather_batch(lvlip_csum_ctx* c, uint32_t n, uint16_t* out, const Ptr& ptr_of, const Len& len_of,
                 const Seed& seed_of) {
    NoDone cb;
    return run_pieces(
        c, n,
        // lay out a piece: packet k at the next 16-B aligned offset, up to the
        // piece size (a larger packet alone, up to the arena).  The offsets
        // are a running sum, so the cut writes the descriptors as it goes ...
        [&](Slot& s, uint32_t first, uint32_t) {
            Cut p;
            for (uint32_t i = first; i < n && p.k < c->max_desc; ++i, ++p.k) {
                const int32_t len = len_of(i);
                const uint64_t need = len > 0 ? (uint64_t)len : 0;
                if (p.bytes + need > (p.k ? c->piece : c->arena)) break;
                s.h_desc[p.k] = lvlip_csum_desc{p.bytes, len, seed_of(i)};
                p.bytes = align16(p.bytes + need);
            }
            return p;
        },
        // ... then the bytes are gathered, packets split over the host
        // threads, nontemporal stores (copy_nt), the next packets prefetched
        [&](Slot& s, uint32_t first, const Cut& p) {
            uint8_t* dst = s.h_bytes;
            const lvlip_csum_desc* hd = s.h_desc;
            parallel_ranges(c, p.k, 1024, [=](uint64_t lo, uint64_t hi) {
                for (uint64_t q = lo; q < hi; ++q) {
                    if (q + 8 < hi && hd[q + 8].len > 0)
                        for (int32_t l = 0; l < hd[q + 8].len; l += 64)
                            __builtin_prefetch((const uint8_t*)ptr_of(first + (uint32_t)q + 8) + l);
                    if (hd[q].len > 0)
                        copy_nt(dst + hd[q].offset, (const uint8_t*)ptr_of(first + (uint32_t)q), (uint64_t)hd[q].len);
                }
                _mm_sfence();
            });
        },
        [&](Slot& s, uint32_t first, const Cut& p) {
            return launch_packets(c, s, p.bytes ? p.bytes : 16, p.k, out + first);
        },
        cb);
}

// Zero-copy: descriptors only (offsets from the region's first byte rounded
// down to 16), kernel reads the registered pages in place.  `addr_of(i)`
// gives packet i's byte address; the whole batch lies in region `r`.  Pieces
// of at most an arena's bytes (the descriptors of the next piece are written,
// on the pool threads, while the kernel reads the previous one's packets;
// a piece was max_desc descriptors before, for a 1M-packet batch one piece
// whose 16 MB of descriptors were written before the kernel started).
template <class AddrOf, class DescOf, class LenOf>
int zerocopy_batch(lvlip_csum_ctx* c, const Region& r, uint32_t n, uint16_t* out, AddrOf addr_of,
                   DescOf desc_of, LenOf len_of) {
    const uint8_t* h0 = (const uint8_t*)((uintptr_t)r.host & ~(uintptr_t)15);
    const uint8_t* d0 = r.dev - (r.host - h0);
    NoDone cb;
    return run_pieces(
        c, n,
        [&](Slot&, uint32_t first, uint32_t) {
            Cut p;  // nothing is moved: any packet may start a piece
            for (uint32_t i = first; i < n && p.k < c->max_desc; ++i, ++p.k) {
                const int32_t l = len_of(i);
                const uint64_t need = l > 0 ? (uint64_t)l : 0u;
                if (p.k && p.bytes + need > c->arena) break;
                p.bytes += need;
            }
            return p;
        },
        [&](Slot& s, uint32_t first, const Cut& p) {
            lvlip_csum_desc* hd = s.h_desc;
            parallel_ranges(c, p.k, 16384, [&, hd, first](uint64_t lo, uint64_t hi) {
                for (uint64_t q = lo; q < hi; ++q) {
                    lvlip_csum_desc dq = desc_of(first + (uint32_t)q);
                    dq.offset = (uint64_t)((const uint8_t*)addr_of(first + (uint32_t)q) - h0);
                    hd[q] = dq;
                }
            });
        },
        [&](Slot& s, uint32_t first, const Cut& p) {
            return launch_packets(c, s, p.bytes ? p.bytes : 16, p.k, out + first, nullptr, d0);
        },
        cb);
}

// Whether a packet's 16-B span fits the arena: what the paths that move spans
// (host_flat_impl's dense path) need of every packet.
inline bool span_fits(const lvlip_csum_ctx* c, uint64_t offset, int32_t len) {
    return align16(offset + (len > 0 ? (uint64_t)len : 0u)) - (offset & ~15ull) <= c->arena;
}

// lvlip_csum_batch_host_flat's GPU path over validated descriptors (every
// packet span_fits).  dense: 1 / 0 when the caller has scanned the batch
// (span_dense), -1 to scan here.  Dense batches move their spans (the copy
// engine straight from a registered region, else one nontemporal copy per
// span into the pinned arena); other batches are read in place from a
// zero-copy region, or gathered packet by packet.
int host_flat_impl(lvlip_csum_ctx* c, const uint8_t* b, size_t base_bytes, const lvlip_csum_desc* d, uint32_t n,
                   uint16_t* out, int dense) {
    const Region* reg = c->regions.empty() ? nullptr : find_region(c, b, base_bytes);
    if (dense < 0) {
        SpanScan sc;
        span_scan(c, n, 4096, &sc, [b, d](uint32_t q, SpanScan& s) {
            if (d[q].len > 0) span_add(s, (uint64_t)(uintptr_t)(b + d[q].offset), (uint64_t)d[q].len);
            return true;
        });
        dense = span_dense(sc, c->span_ratio);
    }
    if (!dense) {
        if (reg && (reg->flags & LVLIP_REG_ZEROCOPY))
            return zerocopy_batch(
                c, *reg, n, out, [&](uint32_t q) { return b + d[q].offset; }, [&](uint32_t q) { return d[q]; },
                [&](uint32_t q) { return d[q].len; });
        return gather_batch(
            c, n, out, [b, d](uint32_t q) { return b + d[q].offset; }, [d](uint32_t q) { return d[q].len; },
            [d](uint32_t q) { return d[q].start_sum; });
    }
    // a piece's bytes: from a registered region the whole arena (no gather to
    // overlap with the copies, and each copy costs the copy engine ~18 us
    // between pieces: DESIGN.md §5), else LVLIP_PIECE_MAX.  A dense batch in
    // a zero-copy region moves its spans as from a DMA region (tcp1500:
    // 54.6-55.2 against 52.5 GB/s in place)
    const uint64_t limit = reg ? c->arena : c->piece;
    NoDone cb;
    return run_pieces(
        c, n,
        // A piece is a run of descriptors whose byte span [lo16, hi) fits the
        // limit (a single larger span alone, up to the arena).  The span is
        // moved whole, keeping each packet's offset mod 16 (so odd/unaligned
        // starts stay exactly as given).
        [&](Slot&, uint32_t first, uint32_t) {
            Cut p;
            uint64_t lo16 = ~0ull, hi = 0;
            for (uint32_t i = first; i < n && p.k < c->max_desc; ++i, ++p.k) {
                const uint64_t o = d[i].offset;
                const uint64_t e = o + (d[i].len > 0 ? (uint64_t)d[i].len : 0);
                const uint64_t nlo = (o & ~15ull) < lo16 ? (o & ~15ull) : lo16;
                const uint64_t nhi = e > hi ? e : hi;
                if (align16(nhi) - nlo > (p.k ? limit : c->arena)) break;
                lo16 = nlo;
                hi = nhi;
            }
            p.lo = lo16;
            p.bytes = hi > lo16 ? hi - lo16 : 0;
            return p;
        },
        [&](Slot& s, uint32_t first, const Cut& p) {
            if (p.bytes && !reg) {
                // the span in 64-B blocks over the threads, nontemporal stores
                uint8_t* dst = s.h_bytes;
                const uint8_t* src = b + p.lo;
                const uint64_t span = p.bytes, nblk = (span + 63) / 64;
                parallel_ranges(c, nblk, 8192, [=](uint64_t lo, uint64_t hi) {
                    const uint64_t e = hi * 64 < span ? hi * 64 : span;
                    copy_nt(dst + lo * 64, src + lo * 64, e - lo * 64);
                    _mm_sfence();
                });
            }
            lvlip_csum_desc* hd = s.h_desc;
            const lvlip_csum_desc* src = d + first;
            const uint64_t base16 = p.lo;
            parallel_ranges(c, p.k, 16384, [hd, src, base16](uint64_t lo, uint64_t hi) {
                for (uint64_t q = lo; q < hi; ++q) {
                    hd[q] = src[q];
                    hd[q].offset = src[q].offset - base16;
                }
            });
        },
        [&](Slot& s, uint32_t first, const Cut& p) {
            // f3 DMA: the copy engine reads the registered span directly.  Its
            // last bytes up to the next 16 B may lie past base_bytes, so copy
            // exactly the span and let the kernel's 16-B tail read the arena.
            return launch_packets(c, s, p.bytes ? p.bytes : 16, p.k, out + first,
                                  p.bytes && reg ? b + p.lo : nullptr);
        },
        cb);
}

}  // namespace

extern "C" {

int lvlip_csum_ctx_create(lvlip_csum_ctx** out, int device, size_t arena_bytes) {
    if (!out) return LVLIP_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return LVLIP_ENODEV;
    if (device < 0 || device >= ndev) return LVLIP_ENODEV;
    if (arena_bytes == 0) arena_bytes = kDefaultArena;
    if (arena_bytes < 4096) arena_bytes = 4096;
    arena_bytes = align16(arena_bytes);

    auto* c = new (std::nothrow) lvlip_csum_ctx();
    if (!c) return LVLIP_ENOMEM;
    c->device = device;
    c->arena = arena_bytes;
    const long long kU32 = 0xffffffffll, kMax = 0x7fffffffffffffffll;
    const unsigned hw = std::thread::hardware_concurrency();
    c->threads = (int)env_ll("LVLIP_GATHER_THREADS", hw ? (hw < 16 ? hw : 16) : 1, 1, 64);
    // LVLIP_DIRECT_MAX: pieces of at most this many bytes skip the H2D/D2H
    // copies (launch_piece); 0 turns that off
    c->direct_max = (uint64_t)env_ll("LVLIP_DIRECT_MAX", (long long)kDirectMax, 0, kMax);
    // LVLIP_PIECE_MAX: bytes per piece, so that even a batch of a few MB is cut
    // into pieces whose gather, copies and kernel overlap across the two slots
    // (0, or more than the arena: the arena)
    const uint64_t pm = (uint64_t)env_ll("LVLIP_PIECE_MAX", (long long)kPieceMax, 0, (long long)arena_bytes);
    c->piece = pm ? align16(pm) : arena_bytes;
    // LVLIP_FIRST_PIECE: the host frame calls' first piece, in bytes; later
    // pieces double up to the piece size (0 or unset: 4 MiB; a value >= the
    // piece size turns the ramp off).  At most the piece size: the ramp's
    // shifts never overflow
    const uint64_t fp = (uint64_t)env_ll("LVLIP_FIRST_PIECE", 0, 0, (long long)c->piece);
    c->first_piece = fp ? align16(fp) : (4ull << 20);
    if (c->first_piece > c->piece) c->first_piece = c->piece;
    // LVLIP_INLINE_MAX: host calls of at most this many packets / frames keep
    // their host steps on the calling thread (ctx_impl.h; 0: never)
    c->inline_max = (uint32_t)env_ll("LVLIP_INLINE_MAX", 32768, 0, kU32);
    // LVLIP_SPAN_RATIO (1-64): the density rule's span-to-bytes ratio (span_dense)
    c->span_ratio = (uint32_t)env_ll("LVLIP_SPAN_RATIO", 2, 1, 64);
    // LVLIP_CPU_MAX: host calls of at most this many packets / frames run on
    // the calling thread (lvlip_csum_ctx_set_cpu_max; 0: always the GPU)
    c->cpu_max = (uint32_t)env_ll("LVLIP_CPU_MAX", LVLIP_CPU_MAX_DEFAULT, 0, kU32);
    // LVLIP_FAIL_PIECE: the error paths' test hook (ctx_impl.h), never set in production
    c->fail_piece = (uint32_t)env_ll("LVLIP_FAIL_PIECE", 0, 0, kU32);
    if (c->fail_piece)
        fprintf(stderr, "lvlip_csum: LVLIP_FAIL_PIECE=%u is set (a test hook): piece %u of every GPU call will fail\n",
                c->fail_piece, c->fail_piece);
    // LVLIP_BLOCK_MIN: a piece of at least this many bytes is waited for by
    // polling between short sleeps instead of by spinning: the pipeline's
    // other slot keeps the GPU busy meanwhile, so the late wake-up costs no
    // throughput and the waiting thread little CPU (0: always spin)
    c->block_min = (uint64_t)env_ll("LVLIP_BLOCK_MIN", (long long)kBlockMin, 0, kMax);
    c->copy_order = env_ll("LVLIP_COPY_ORDER", 1, -kMax, kMax) != 0;
    c->frame_trace = env_ll("LVLIP_FRAME_TRACE", 0, 0, kMax) == 1;
    // descriptors per piece: one per 64 B of arena (a piece of smaller packets
    // simply ends at this count; the next piece takes the rest)
    c->max_desc = (uint32_t)(arena_bytes / 64 < 4096 ? 4096 : arena_bytes / 64);

    DeviceGuard g(device);
    for (auto& s : c->slot) {
        hipError_t e;
        if ((e = hipHostMalloc((void**)&s.h_bytes, arena_bytes, hipHostMallocDefault)) != hipSuccess ||
            (e = hipHostMalloc((void**)&s.h_desc, (size_t)c->max_desc * sizeof(lvlip_csum_desc),
                               hipHostMallocDefault)) != hipSuccess ||
            (e = hipHostMalloc((void**)&s.h_out, (size_t)c->max_desc * sizeof(uint16_t),
                               hipHostMallocDefault)) != hipSuccess ||
            (e = hipMalloc((void**)&s.d_bytes, arena_bytes)) != hipSuccess ||
            (e = hipMalloc((void**)&s.d_desc, (size_t)c->max_desc * sizeof(lvlip_csum_desc))) != hipSuccess ||
            (e = hipMalloc((void**)&s.d_out, (size_t)c->max_desc * sizeof(uint16_t))) != hipSuccess ||
            (e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&s.copied, hipEventDisableTiming)) != hipSuccess ||
            (e = hipHostGetDevicePointer((void**)&s.dh_bytes, s.h_bytes, 0)) != hipSuccess ||
            (e = hipHostGetDevicePointer((void**)&s.dh_desc, s.h_desc, 0)) != hipSuccess ||
            (e = hipHostGetDevicePointer((void**)&s.dh_out, s.h_out, 0)) != hipSuccess) {
            fail(c, e, "lvlip_csum_ctx_create");
            for (auto& t : c->slot) free_slot(t);
            delete c;
            return LVLIP_ENOMEM;
        }
    }
    // Start the copy engine now: the first piece that goes through it (a call
    // larger than direct_max) otherwise pays its start-up, ~7 ms measured on
    // the first 15K-frame TX call of a context against 0.9 ms for the next.
    // Each slot copies `warm` bytes of its arena each way once
    // (LVLIP_WARM_BYTES, default 1 MiB; 0 skips it).
    {
        const size_t warm = (size_t)env_ll("LVLIP_WARM_BYTES", 1 << 20, 0, (long long)arena_bytes);
        hipError_t e = hipSuccess;
        for (auto& s : c->slot) {
            if (!warm || e != hipSuccess) break;
            if ((e = hipMemcpyAsync(s.d_bytes, s.h_bytes, warm, hipMemcpyHostToDevice, s.stream)) == hipSuccess)
                e = hipMemcpyAsync(s.h_bytes, s.d_bytes, warm, hipMemcpyDeviceToHost, s.stream);
        }
        for (auto& s : c->slot)
            if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
        // and the kernels' code object, so the first call launches at once
        if (e == hipSuccess && lvlip_kernels_load() != 0) e = hipErrorInvalidDeviceFunction;
        if (e != hipSuccess) {
            fail(c, e, "lvlip_csum_ctx_create (copy engine start)");
            for (auto& t : c->slot) free_slot(t);
            delete c;
            return LVLIP_EHIP;
        }
    }
    *out = c;
    return LVLIP_OK;
}

int lvlip_csum_ctx_destroy(lvlip_csum_ctx* c) {
    if (!c) return LVLIP_EINVAL;
    DeviceGuard g(c->device);
    for (auto& s : c->slot) {
        if (s.busy) (void)hipEventSynchronize(s.done);
        free_slot(s);
    }
    for (const Region& r : c->regions) (void)hipHostUnregister(r.host);
    free(c->frame_scratch);
    free(c->frame_scratch2);
    free(c->host_scratch);
    delete c;
    return LVLIP_OK;
}

int lvlip_csum_ctx_set_cpu_max(lvlip_csum_ctx* c, uint32_t cpu_max) {
    if (!c) return LVLIP_EINVAL;
    c->cpu_max = cpu_max;
    return LVLIP_OK;
}

uint32_t lvlip_csum_ctx_cpu_max(const lvlip_csum_ctx* c) { return c ? c->cpu_max : 0u; }

int lvlip_csum_ctx_stats(const lvlip_csum_ctx* c, lvlip_ctx_stats* out) {
    if (!c || !out) return LVLIP_EINVAL;
    *out = c->stats;
    return LVLIP_OK;
}

int lvlip_csum_register(lvlip_csum_ctx* c, void* ptr, size_t bytes, uint32_t flags) {
    if (!c || !ptr || bytes == 0 || flags > LVLIP_REG_ZEROCOPY) return LVLIP_EINVAL;
    uint8_t* p = (uint8_t*)ptr;
    for (const Region& r : c->regions)
        if (p < r.host + r.bytes && r.host < p + bytes) return LVLIP_EINVAL;  // overlap
    DeviceGuard g(c->device);
    hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterMapped);
    if (e != hipSuccess) return fail(c, e, "hipHostRegister");
    void* dev = nullptr;
    if ((e = hipHostGetDevicePointer(&dev, ptr, 0)) != hipSuccess) {
        (void)hipHostUnregister(ptr);
        return fail(c, e, "hipHostGetDevicePointer");
    }
    Region r;
    r.host = p;
    r.bytes = bytes;
    r.dev = (uint8_t*)dev;
    r.flags = flags;
    try {  // no exception leaves the C ABI
        c->regions.push_back(r);
    } catch (...) {
        (void)hipHostUnregister(ptr);
        return LVLIP_ENOMEM;
    }
    return LVLIP_OK;
}

int lvlip_csum_unregister(lvlip_csum_ctx* c, void* ptr) {
    if (!c || !ptr) return LVLIP_EINVAL;
    for (size_t k = 0; k < c->regions.size(); ++k) {
        if (c->regions[k].host != (uint8_t*)ptr) continue;
        DeviceGuard g(c->device);
        for (auto& s : c->slot) {  // nothing in flight may still read it
            const int rc = drain(c, s);
            if (rc != LVLIP_OK) return rc;
        }
        const hipError_t e = hipHostUnregister(ptr);
        c->regions.erase(c->regions.begin() + (long)k);
        return e == hipSuccess ? LVLIP_OK : fail(c, e, "hipHostUnregister");
    }
    return LVLIP_EINVAL;
}

int lvlip_csum_batch_host(lvlip_csum_ctx* c, const lvlip_csum_iov* pkts, uint32_t n,
                          uint16_t* out) {
    if (!c || (n && (!pkts || !out)) || n > LVLIP_MAX_BATCH) return LVLIP_EINVAL;
    if (n == 0) return LVLIP_OK;
    begin_call(c, n);
    if (first_failure(c, n, [pkts](uint32_t i) { return pkts[i].len > 0 && !pkts[i].ptr ? LVLIP_EINVAL : LVLIP_OK; }) !=
        LVLIP_OK)
        return LVLIP_EINVAL;
    const uint64_t arena = c->arena;
    if (first_failure(c, n, [pkts, arena](uint32_t i) {
            return pkts[i].len > 0 && align16((uint64_t)pkts[i].len) > arena ? LVLIP_ERANGE : LVLIP_OK;
        }) != LVLIP_OK)
        return LVLIP_ERANGE;  // a single packet larger than the arena (on every path)
    auto ptr_of = [pkts](uint32_t q) { return (const uint8_t*)pkts[q].ptr; };
    auto len_of = [pkts](uint32_t q) { return pkts[q].len; };
    auto seed_of = [pkts](uint32_t q) { return pkts[q].start_sum; };
    if (n <= c->cpu_max) return cpu_batch(c, n, out, ptr_of, len_of, seed_of);
    DeviceGuard g(c->device);
    begin_gpu_call(c);
    int rc = 1;  // no code of the library's: not taken by a region path yet
    if (!c->regions.empty()) {
        // f3: all packets inside one registered region (the region of the
        // first non-empty packet; regions never overlap) -> no gather at all:
        // packets that cover their span densely and in order go as a flat
        // batch over the region (the copy engine moves the spans); a
        // zero-copy region's other batches are read in place; a DMA region's
        // are gathered below
        uint32_t i0 = 0;
        while (i0 < n && pkts[i0].len <= 0) ++i0;
        const Region* r = i0 < n ? find_region(c, pkts[i0].ptr, (uint64_t)pkts[i0].len) : nullptr;
        if (r) {
            // one pass on the pool threads: every packet inside r, the
            // packets' span, bytes and jumps, whether each one's 16-B span
            // fits the arena (the flat call's rule), and their flat
            // descriptors relative to r (written whether or not they are
            // used; the array is trimmed after a huge call)
            lvlip_csum_desc* fd = (lvlip_csum_desc*)scratch(c->host_scratch, c->host_scratch_bytes,
                                                            sizeof(lvlip_csum_desc) * (size_t)n);
            const uint8_t *r0 = r->host, *r1 = r->host + r->bytes;
            std::atomic<bool> unfit{false};
            SpanScan sc;
            const bool inside = span_scan(c, n, 4096, &sc, [&, fd, r0, r1](uint32_t q, SpanScan& s) {
                const int32_t len = pkts[q].len;
                uint64_t o = 0;
                if (len > 0) {
                    const uint8_t* p = (const uint8_t*)pkts[q].ptr;
                    if (p < r0 || p + len > r1) return false;
                    o = (uint64_t)(p - r0);
                    span_add(s, o, (uint64_t)len);
                    if (!span_fits(c, o, len)) unfit.store(true, std::memory_order_relaxed);
                }
                if (fd) fd[q] = lvlip_csum_desc{o, len, pkts[q].start_sum};
                return true;
            });
            // a packet whose 16-B span exceeds the arena cannot move as a
            // span: the batch is then read in place or gathered, where a
            // packet needs only its own bytes rounded up to 16 (checked above)
            if (inside && fd && !unfit.load(std::memory_order_relaxed) && span_dense(sc, c->span_ratio))
                rc = host_flat_impl(c, r->host, r->bytes, fd, n, out, 1);
            else if (inside && (r->flags & LVLIP_REG_ZEROCOPY))
                rc = zerocopy_batch(
                    c, *r, n, out, [&](uint32_t q) { return pkts[q].len > 0 ? (const uint8_t*)pkts[q].ptr : r->host; },
                    [&](uint32_t q) {
                        lvlip_csum_desc d{};
                        d.len = pkts[q].len;
                        d.start_sum = pkts[q].start_sum;
                        return d;
                    },
                    [&](uint32_t q) { return pkts[q].len; });
        }
    }
    if (rc > 0) rc = gather_batch(c, n, out, ptr_of, len_of, seed_of);
    trim_scratch(c);
    return rc;
}

int lvlip_csum_batch_host_flat(lvlip_csum_ctx* c, const void* base, size_t base_bytes,
                               const lvlip_csum_desc* d, uint32_t n, uint16_t* out) {
    if (!c || (n && (!base || !d || !out)) || n > LVLIP_MAX_BATCH) return LVLIP_EINVAL;
    if (n == 0) return LVLIP_OK;
    begin_call(c, n);
    const uint8_t* b = (const uint8_t*)base;
    const int bad = first_failure(c, n, [c, d, base_bytes](uint32_t q) {
        if (d[q].offset + (d[q].len > 0 ? (uint64_t)d[q].len : 0u) > base_bytes) return LVLIP_EINVAL;
        // a single packet whose 16-B span exceeds the arena: refuse before any
        // piece is in flight (a piece still in flight would later write into out[])
        return span_fits(c, d[q].offset, d[q].len) ? LVLIP_OK : LVLIP_ERANGE;
    });
    if (bad != LVLIP_OK) return bad;
    if (n <= c->cpu_max)
        return cpu_batch(
            c, n, out, [b, d](uint32_t q) { return b + d[q].offset; }, [d](uint32_t q) { return d[q].len; },
            [d](uint32_t q) { return d[q].start_sum; });
    DeviceGuard g(c->device);
    begin_gpu_call(c);
    const int rc = host_flat_impl(c, b, base_bytes, d, n, out, -1);
    trim_scratch(c);
    return rc;
}

// Group 4: one host thread per context, each on its part of the batch.  The
// parts' descriptors keep their offsets from `base`, so each context gathers
// (or DMAs) only its own span.
int lvlip_csum_batch_host_flat_multi(lvlip_csum_ctx* const* ctxs, uint32_t nctx, const void* base,
                                     size_t base_bytes, const lvlip_csum_desc* d, uint32_t n, uint16_t* out) {
    if (!ctxs || nctx == 0 || (n && (!base || !d || !out)) || n > LVLIP_MAX_BATCH) return LVLIP_EINVAL;
    for (uint32_t k = 0; k < nctx; ++k) {
        if (!ctxs[k]) return LVLIP_EINVAL;
        for (uint32_t j = 0; j < k; ++j)
            if (ctxs[j] == ctxs[k]) return LVLIP_EINVAL;  // one thread per context
    }
    if (n == 0) return LVLIP_OK;
    std::vector<uint32_t> cuts;
    std::vector<int> rcs;
    std::vector<std::thread> th;
    std::vector<std::string> errs;  // each part's lvlip_last_hip_error() (thread-local)
    try {  // no exception leaves the C ABI
        cuts.resize(nctx + 1u);
        rcs.assign(nctx, LVLIP_OK);
        errs.resize(nctx);
        th.reserve(nctx);
    } catch (...) {
        return LVLIP_ENOMEM;
    }
    int rc = lvlip_partition_bytes(d, n, nctx, cuts.data());
    if (rc != LVLIP_OK) return rc;
    auto part = [&](uint32_t k) noexcept {
        const uint32_t lo = cuts[k], hi = cuts[k + 1];
        if (hi > lo) rcs[k] = lvlip_csum_batch_host_flat(ctxs[k], base, base_bytes, d + lo, hi - lo, out + lo);
        if (rcs[k] != LVLIP_OK) {
            try {
                errs[k] = lvlip_last_hip_error();
            } catch (...) {
            }
        }
    };
    // parts 1.. on threads of their own; a part whose thread cannot be
    // started runs on the calling thread after part 0 (a thread shortage
    // costs the overlap, not the call)
    uint32_t started = 1;
    try {
        for (; started < nctx; ++started) th.emplace_back(part, started);
    } catch (...) {
    }
    part(0);
    for (uint32_t k = started; k < nctx; ++k) part(k);
    for (auto& t : th) t.join();
    for (uint32_t k = 0; k < nctx; ++k)
        if (rcs[k] != LVLIP_OK) {
            // the failing part's HIP message, on the caller's thread
            lvlip_set_last_hip_error(errs[k].c_str());
            return rcs[k];
        }
    return LVLIP_OK;
}

}  // extern "C"
