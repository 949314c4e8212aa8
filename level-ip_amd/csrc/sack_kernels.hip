// sack_kernels.hip — the sender's scoreboard on the device (include/lvlip_skb.h,
// "f2 on the device: the scoreboard and the selective retransmit"): the SACK
// blocks of a batch of ACK frames -> one byte per queue entry the peer holds.
// sack_cpu.c is the same on the calling thread, bit for bit.  The selection
// pass and the rewrite of lvlip_rtx_sack_dev are k_pick and k_rtx in
// snd_kernels.hip, beside the retransmit whose frame path they share.
//
// adv_kernels.hip solves the same shape of problem, a union of intervals per
// flow, and both take the keys, the sort and the workspace's pieces from
// interval_union.h; here an element is a block, not a record: up to 4 n
// elements, the key flow << 32 | l, the value the 32-bit r.  res is zeroed on
// the stream, then:
//
//   k_sack_parse  one lane per ACK record.  A record that carries an ACK
//                 (rec_ack_flow, the predicate of k_snd_rec) has its frame's
//                 option bytes, at most 40, loaded as the aligned dwords that
//                 hold them, funnelled (v_alignbyte) and parked in the lane's
//                 own 44 bytes of LDS (stride 11 dwords: no bank is shared by
//                 two lanes of a row), where the RFC 793 walk reads them byte
//                 by byte: a walk over registers would index them at run time,
//                 which hipcc turns into scratch.  Every block goes straight to
//                 key[4 i + b] and val[4 i + b]; an invalid or absent block
//                 takes IU_NO_KEY.  n_blocks, n_valid and high are reduced
//                 within the wave before any atomic, flow by flow, SACK_PEEL
//                 times (wave_peel), as k_snd_rec does
//   rocPRIM       radix_sort_pairs over the key bits, r as value
//   rocPRIM       inclusive max-scan of flow << 32 | r -> H: the largest end
//                 so far inside the element's flow
//   rocPRIM       inclusive max-scan of (head ? i + 1 : 0) -> S: the island's
//                 first element.  Element i is a head when i == 0 or H[i - 1]
//                 is below its key (interval_union.h says why both work)
//   k_sack_mark   a wave per flow and chunk of its queue (blockIdx.y strides
//                 the queue, so a queue of many thousands of entries is spread
//                 over 8 to SACK_Y waves, by the flow count): the flow's range
//                 [ra, rb) of the sorted keys by the 64-way search, then one
//                 lane per queue entry:
//                 the entry's header fields, a binary search inside [ra, rb)
//                 for p, the last element with l < e, and the byte is stored
//                 when the island of p starts at or before a and H[p] reaches
//                 e.  (The island that covers [a, e) holds every element with
//                 l in [a, e), so p is in it; the elements up to p of one
//                 island are contiguous from its start to H[p].)  The wave
//                 then counts its entries' bytes that are 1 and adds them to
//                 n_sacked: one atomic per wave
//
// Integer add and max are the only reductions and the sort is by key only
// where order matters (equal keys differ in r, and a running maximum does not
// depend on their order), so the bytes do not depend on the run.
//
// Workspace (sack_plan; every part 256-B aligned): two key arrays (H takes
// the one the sort leaves free), two value arrays (S takes the free one),
// rocPRIM's temporary storage, the largest of the three calls'.
//
// Bounds.  rec, ack_fd: index below n.  An ACK frame is read only inside
// [F, F + fd.len) rounded to dwords, and only after fd.len covered the bytes:
// 15 for version and ihl, 14 + 4 ihl + 20 for hl, 14 + 4 ihl + 4 hl for the
// options.  key, val, H, S: index below 4 n.  Queue entries come from the
// planned s; an entry's 54 header bytes are read only when fd.len >= 54.
// sacked and res are indexed by the planned queue entries and flows only.  A
// crafted record changes values, never an address.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "interval_union.h"
#include "lvlip_skb.h"
#include "tcp_hdr_dev.h"
#include "wave_ops.h"

namespace lvlip {

constexpr uint32_t SACK_NONE = 0xFFFFFFFFu;
constexpr uint32_t SACK_TILE = 256;            // records per workgroup of k_sack_parse: one per thread
constexpr uint32_t SACK_OPT = 11;              // dwords of LDS per lane: 40 option bytes, and an odd stride
constexpr int SACK_PEEL = 4;                   // flows a wave reduces before lanes go alone
constexpr uint32_t SACK_WAVES = 4;             // waves (flows) per workgroup of k_sack_mark
constexpr uint32_t SACK_Y = 1024;              // most chunks a queue is spread over
constexpr uint32_t SACK_Y_MIN = 8;             // fewest: 65 536 flows still give a long queue eight waves
constexpr uint32_t SACK_GRID = 1u << 17;       // workgroups of k_sack_mark the chunk count aims at
constexpr uint32_t SACK_MAX_N = 0x3FFFFFFFu;   // 4 n + 1 must fit 32 bits: S holds element indices + 1

__device__ __forceinline__ uint32_t lds_byte(const uint32_t* o, uint32_t at) {
    return (o[at >> 2] >> (8u * (at & 3u))) & 0xffu;
}

__device__ __forceinline__ uint32_t lds_be32(const uint32_t* o, uint32_t at) {
    return (lds_byte(o, at) << 24) | (lds_byte(o, at + 1u) << 16) | (lds_byte(o, at + 2u) << 8) | lds_byte(o, at + 3u);
}

__global__ __launch_bounds__(256) void k_sack_parse(const lvlip_lro_flow* f, const lvlip_snd_flow* s, uint32_t nflows,
                                                    const lvlip_lro_rec* rec, const uint8_t* ack_base,
                                                    const lvlip_frame_desc* ack_fd, uint32_t n, uint64_t* key,
                                                    uint32_t* val, lvlip_sack_result* res) {
    __shared__ uint32_t opts[SACK_TILE * SACK_OPT];
    uint32_t* o = opts + threadIdx.x * SACK_OPT;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * SACK_TILE + threadIdx.x;
    uint32_t flow = SACK_NONE, nb = 0u, nv = 0u, high = 0u;
    if (i < n) {
        flow = rec_ack_flow(load_global(reinterpret_cast<uint64_t>(rec + i)), f, nflows);
        uint32_t optlen = 0u;
        if (flow != SACK_NONE) {
            const uint4 d = load_global(reinterpret_cast<uint64_t>(ack_fd + i));  // offset lo, hi, len, -
            const uint64_t F = reinterpret_cast<uint64_t>(ack_base) + (((uint64_t)d.y << 32) | d.x);
            typedef __attribute__((address_space(1))) const uint8_t gby;
            if (d.z >= 34u) {
                const uint32_t vi = *reinterpret_cast<gby*>(F + 14u);  // version | ihl
                const uint32_t th = 14u + 4u * (vi & 0xfu);
                if ((vi >> 4) == 4u && (vi & 0xfu) >= 5u && d.z >= th + 20u) {
                    const uint32_t hl = *reinterpret_cast<gby*>(F + th + 12u) >> 4;
                    if (hl >= 5u && d.z >= th + 4u * hl) {
                        optlen = 4u * hl - 20u;
#pragma unroll
                        for (uint32_t j = 0; j < 10u; ++j)
                            if (4u * j < optlen) o[j] = load_u32_any(F + th + 20u + 4u * j);
                    }
                }
            }
        }
        const uint32_t una = flow != SACK_NONE ? s[flow].snd_una : 0u;
        const uint32_t span = flow != SACK_NONE ? s[flow].snd_nxt - una : 0u;
        uint32_t pos = 0u;
        while (pos < optlen && nb < 4u) {
            const uint32_t kind = lds_byte(o, pos);
            if (kind == 0u) break;
            if (kind == 1u) {
                pos++;
                continue;
            }
            if (pos + 1u >= optlen) break;
            const uint32_t len = lds_byte(o, pos + 1u);
            if (len < 2u || pos + len > optlen) break;
            if (kind == 5u && len >= 10u && len <= 34u && (len - 2u) % 8u == 0u) {
                for (uint32_t j = 0; j < (len - 2u) / 8u && nb < 4u; ++j, ++nb) {
                    const uint32_t l = lds_be32(o, pos + 2u + 8u * j) - una;
                    const uint32_t r = lds_be32(o, pos + 6u + 8u * j) - una;
                    const bool valid = l < r && r <= span;  // not D-SACK or stale, empty, beyond snd_nxt
                    key[4u * i + nb] = valid ? ((uint64_t)flow << 32) | l : IU_NO_KEY;
                    val[4u * i + nb] = valid ? r : 0u;
                    nv += valid ? 1u : 0u;
                    if (valid) high = max(high, r);
                }
            }
            pos += len;
        }
        for (uint32_t b = nb; b < 4u; ++b) {
            key[4u * i + b] = IU_NO_KEY;
            val[4u * i + b] = 0u;
        }
    }
    // ---- n_blocks, n_valid, high: the wave's sums and maximum per flow, then three atomics
    const bool pending = wave_peel<SACK_PEEL>(nb != 0u, flow, [=](uint32_t fl, bool mine) {
        const uint32_t cb = wave_add_u32(mine ? nb : 0u), cv = wave_add_u32(mine ? nv : 0u);
        const uint32_t mx = wave_max_u32(mine ? high : 0u);
        uint32_t* w = reinterpret_cast<uint32_t*>(res + fl);  // n_blocks n_valid n_sacked high
        if (lane == 0u) atomicAdd(w, cb);
        if (lane == 1u && cv) atomicAdd(w + 1, cv);
        if (lane == 2u && mx) atomicMax(w + 3, mx);
    });
    if (pending) {
        uint32_t* w = reinterpret_cast<uint32_t*>(res + flow);
        atomicAdd(w, nb);
        if (nv) atomicAdd(w + 1, nv);
        if (high) atomicMax(w + 3, high);
    }
}

// flow << 32 | r of sorted element i: what the first scan takes the running maximum of
struct sack_end {
    const uint64_t* key;
    const uint32_t* val;
    __host__ __device__ uint64_t operator()(uint32_t i) const { return (key[i] & 0xFFFFFFFF00000000ull) | val[i]; }
};

// i + 1 where an island starts at sorted element i, else 0: what the second scan takes the maximum of
struct sack_head {
    const uint64_t* key;
    const uint64_t* H;
    __host__ __device__ uint32_t operator()(uint32_t i) const { return i == 0u || H[i - 1u] < key[i] ? i + 1u : 0u; }
};

__global__ __launch_bounds__(256) void k_sack_mark(const lvlip_snd_flow* s, uint32_t nflows, const uint8_t* base,
                                                   const lvlip_frame_desc* fd, const uint64_t* key, const uint64_t* H,
                                                   const uint32_t* S, uint32_t m, uint8_t* sacked,
                                                   lvlip_sack_result* res) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k64 = (uint64_t)blockIdx.x * SACK_WAVES + (threadIdx.x >> 6);
    if (k64 >= nflows) return;  // the whole wave
    const uint32_t k = (uint32_t)k64;
    const uint32_t una = s[k].snd_una, seg0 = s[k].seg0, nseg = s[k].nseg;
    const uint64_t first = (uint64_t)blockIdx.y * 64u, stride = (uint64_t)gridDim.y * 64u;
    if (first >= nseg) return;  // the whole wave
    const uint32_t ra = wave_lower_bound(key, m, (uint64_t)k << 32, lane);
    const uint32_t rb = wave_lower_bound(key, m, ((uint64_t)k + 1u) << 32, lane);
    uint32_t count = 0u;
    for (uint64_t c0 = first; c0 < nseg; c0 += stride) {
        const uint64_t i = c0 + lane;
        if (i >= nseg) continue;
        const uint32_t q = seg0 + (uint32_t)i;
        bool covered = false;
        const uint4 d = load_global(reinterpret_cast<uint64_t>(fd + q));  // offset lo, hi, len, -
        if (ra < rb && d.z >= (uint32_t)TCP_FRAME_HDR) {
            const uint64_t F = reinterpret_cast<uint64_t>(base) + (((uint64_t)d.y << 32) | d.x);
            uint32_t iplen, hl;
            if (rtx_frame_ok(load_u32_any(F + 14u), load_u32_any(F + 44u), d.z, &iplen, &hl) &&
                iplen > 20u + 4u * hl) {
                const uint32_t a = __builtin_bswap32(load_u32_any(F + 38u)) - una;
                const uint64_t e = (uint64_t)a + (iplen - 20u - 4u * hl);
                const uint32_t x = e - 1u > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)(e - 1u);
                uint32_t lo = ra, hi = rb;  // l of [ra, lo) <= x < l of [hi, rb)
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo) / 2u;
                    if ((uint32_t)key[mid] <= x) lo = mid + 1u;
                    else hi = mid;
                }
                if (lo > ra) {
                    const uint32_t p = lo - 1u;
                    covered = (uint32_t)key[S[p] - 1u] <= a && (H[p] & 0xFFFFFFFFull) >= e;
                }
            }
        }
        if (covered) sacked[q] = 1;
        count += covered || sacked[q] == 1 ? 1u : 0u;
    }
    count = wave_add_u32(count);
    if (lane == 0u && count) atomicAdd(&res[k].n_sacked, count);
}

struct sack_layout {
    size_t key[2], val[2], tmp, tmp_bytes, total;
};

static hipError_t sack_scan_end(void* tmp, size_t& bytes, const uint64_t* key, const uint32_t* val, uint64_t* H,
                                uint32_t m, hipStream_t st) {
    auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0u), sack_end{key, val});
    return rocprim::inclusive_scan(tmp, bytes, in, H, m, rocprim::maximum<uint64_t>(), st);
}

static hipError_t sack_scan_head(void* tmp, size_t& bytes, const uint64_t* key, const uint64_t* H, uint32_t* S,
                                 uint32_t m, hipStream_t st) {
    auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0u), sack_head{key, H});
    return rocprim::inclusive_scan(tmp, bytes, in, S, m, rocprim::maximum<uint32_t>(), st);
}

// false when a size query of rocPRIM's fails (no device)
static bool sack_plan(uint32_t n, sack_layout& L) {
    const uint32_t m = 4u * n;
    const auto query = [m](size_t& bytes) {
        rocprim::double_buffer<uint64_t> k(nullptr, nullptr);
        rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
        size_t a = 0, b = 0, c = 0;
        hipError_t e = iu_sort(nullptr, a, k, v, m, nullptr);
        if (e == hipSuccess) e = sack_scan_end(nullptr, b, nullptr, nullptr, nullptr, m, nullptr);
        if (e == hipSuccess) e = sack_scan_head(nullptr, c, nullptr, nullptr, nullptr, m, nullptr);
        bytes = a > b ? (a > c ? a : c) : (b > c ? b : c);
        return e;
    };
    if (!iu_tmp_bytes(m, query, L.tmp_bytes)) return false;
    size_t at = 0;
    for (int j = 0; j < 2; ++j) L.key[j] = iu_carve(at, (size_t)m * 8u);
    for (int j = 0; j < 2; ++j) L.val[j] = iu_carve(at, (size_t)m * 4u);
    L.tmp = iu_carve(at, L.tmp_bytes);
    L.total = at;
    return true;
}

}  // namespace lvlip

extern "C" {

size_t lvlip_sack_workspace_bytes(uint32_t n, uint32_t /*nflows*/) {
    if (n == 0 || n > lvlip::SACK_MAX_N || !lvlip::iu_have_device()) return 0;
    lvlip::sack_layout L;
    return lvlip::sack_plan(n, L) ? L.total : 0;
}

int lvlip_sack_dev(const lvlip_lro_flow* f, const lvlip_snd_flow* s, uint32_t nflows, const lvlip_lro_rec* rec,
                   const void* ack_base, const lvlip_frame_desc* ack_fd, uint32_t n, const void* base,
                   const lvlip_frame_desc* fd, uint8_t* sacked, lvlip_sack_result* res, void* workspace,
                   size_t workspace_bytes, void* stream) {
    using namespace lvlip;
    if (nflows == 0 || n == 0) return LVLIP_OK;
    if (!f || !s || !rec || !ack_base || !ack_fd || !base || !fd || !sacked || !res || !workspace) return LVLIP_EINVAL;
    if (n > LVLIP_MAX_BATCH || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    if (((uintptr_t)f & 7u) || ((uintptr_t)s & 7u) || ((uintptr_t)rec & 15u) || ((uintptr_t)ack_fd & 15u) ||
        ((uintptr_t)fd & 15u) || ((uintptr_t)res & 15u) || ((uintptr_t)workspace & 255u))
        return LVLIP_EINVAL;
    if (n > SACK_MAX_N) return LVLIP_ERANGE;  // no workspace serves it
    sack_layout L;
    if (!sack_plan(n, L)) return LVLIP_ENODEV;
    if (workspace_bytes < L.total) return LVLIP_ERANGE;

    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    const uint32_t m = 4u * n;
    rocprim::double_buffer<uint64_t> keys((uint64_t*)(ws + L.key[0]), (uint64_t*)(ws + L.key[1]));
    rocprim::double_buffer<uint32_t> vals((uint32_t*)(ws + L.val[0]), (uint32_t*)(ws + L.val[1]));
    hipError_t e;

    int rc = lvlip_launch_status(hipMemsetAsync(res, 0, (size_t)nflows * sizeof *res, st), "lvlip_sack_dev: memset");
    if (rc != LVLIP_OK) return rc;
    const uint32_t pgrid = (uint32_t)(((uint64_t)n + SACK_TILE - 1u) / SACK_TILE);
    hipLaunchKernelGGL(k_sack_parse, dim3(pgrid), dim3(SACK_TILE), 0, st, f, s, nflows, rec, (const uint8_t*)ack_base,
                       ack_fd, n, keys.current(), vals.current(), res);
    if ((rc = lvlip_launched("k_sack_parse")) != LVLIP_OK) return rc;
    size_t tmp_bytes = L.tmp_bytes;
    if ((e = iu_sort(ws + L.tmp, tmp_bytes, keys, vals, m, st)) != hipSuccess)
        return lvlip_launch_status(e, "lvlip_sack_dev: radix sort");
    const uint64_t* sorted = keys.current();
    uint64_t* H = keys.alternate();  // the sort is done with both
    uint32_t* S = vals.alternate();
    tmp_bytes = L.tmp_bytes;
    if ((e = sack_scan_end(ws + L.tmp, tmp_bytes, sorted, vals.current(), H, m, st)) != hipSuccess)
        return lvlip_launch_status(e, "lvlip_sack_dev: scan of the ends");
    tmp_bytes = L.tmp_bytes;
    if ((e = sack_scan_head(ws + L.tmp, tmp_bytes, sorted, H, S, m, st)) != hipSuccess)
        return lvlip_launch_status(e, "lvlip_sack_dev: scan of the heads");
    // a queue's chunks.  The queue lengths are in device memory, so the grid is sized from the flow count:
    // SACK_GRID workgroups in all, at most SACK_Y and at least SACK_Y_MIN chunks a queue.  A wave whose
    // chunk lies behind its queue's end leaves after three loads
    const uint32_t fgrid = (nflows + SACK_WAVES - 1u) / SACK_WAVES;
    uint32_t y = SACK_GRID / fgrid;
    y = y > SACK_Y ? SACK_Y : y < SACK_Y_MIN ? SACK_Y_MIN : y;
    hipLaunchKernelGGL(k_sack_mark, dim3(fgrid, y), dim3(256), 0, st, s, nflows, (const uint8_t*)base, fd, sorted,
                       (const uint64_t*)H, (const uint32_t*)S, m, sacked, res);
    return lvlip_launched("k_sack_mark");
}

}  // extern "C"
