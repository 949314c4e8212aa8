// adv_kernels.hip — lvlip_lro_advance on the device (include/lvlip_skb.h,
// "f1 on the device: receive coalescing"): the records lvlip_lro_dev left in
// HBM -> per planned flow the contiguous prefix, the PLACED count and the
// first four islands beyond the prefix, every byte what rcv_cpu.c's
// lvlip_lro_advance writes for the same records.  Nothing leaves the caller's
// stream: six steps, each a completed launch before the next one reads it.
// The keys, the sort and the workspace's pieces are interval_union.h's, which
// the scoreboard (sack_kernels.hip) builds its unions from too.
//
//   k_adv_keys    one lane per record, one 16-B load: the 8-B key
//                 flow << 32 | rel (IU_NO_KEY for a record that does not
//                 count: not PLACED, or flow >= nflows) and the 2-B dlen (0
//                 when it does not count)
//   rocPRIM       radix_sort_pairs over the key bits, the dlen as value.
//                 Stable and deterministic; equal keys may differ in dlen only,
//                 and nothing below depends on their order (a running maximum
//                 and a test against it: see k_adv_heads)
//   k_adv_reduce  per tile of ADV_TILE sorted elements the maximum of
//                 V = flow << 33 | (rel + dlen).  The end needs 33 bits; the
//                 flow on top of it makes a plain max-scan segmented, because
//                 the flow never decreases along the sorted array
//   k_adv_spine   one wave: the exclusive max-scan of the tile maxima in place,
//                 ceil(tiles / 64) consecutive tiles per lane
//   k_adv_heads   the tile's inclusive max-scan with the spine's carry: H[i],
//                 the largest end so far inside i's flow, and one bit per
//                 element, set where an island starts: i == 0, or the scan
//                 before i is below flow_i << 33 | rel_i (another flow, or an
//                 end below rel_i: intervals that touch are one island).  One
//                 ballot word per wave into the bitmap
//   k_adv_emit    one wave per planned flow: its range [a, b) of the sorted keys
//                 by a 64-way search (placed = b - a), then the bitmap from a,
//                 256 words a round, until the sixth head or b: the island at
//                 rel 0 and four more need five islands' ends, and an island ends
//                 at H before the next head or at H[b - 1].  Twelve lanes store
//                 the result's twelve words; a flow without a record gets zeros
//
// lvlip_lro_advance_carry_dev is the same pipeline over n + 4 nflows elements:
// k_adv_keys_carry also writes, for slot n + 4 k + j, block j of prev[k] as the
// interval [l, r) relative to f[k].rcv_nxt when l < r <= f[k].rcv_wnd (IU_NO_KEY
// otherwise), and per flow the count of such blocks, which k_adv_emit_carry
// takes off `placed`.  A carried block is up to 2^30 bytes long, so this form
// sorts and scans 4-B lengths: k_adv_reduce and k_adv_heads are templates over
// the length's type, and lvlip_lro_advance_dev keeps the 2-B instantiation it
// had.  prev may be res: the key step has read it before the emit step, a later
// launch, writes it.
//
// Workspace (adv_plan; every part 256-B aligned): two key arrays and two dlen
// arrays (the sort's double buffers; H takes the key array the sort leaves
// free), the tile maxima, the bitmap, the carry form's counts, rocPRIM's temporary
// storage.
//
// Bounds.  Every index into rec is below n and every one into the key arrays
// below the element count (a live test in
// 64 bits from blockIdx, or a search bounded by the element count), every
// bitmap word at most (count - 1) / 64, every index into f, prev, res and the
// counts below nflows; a crafted record (flow 0xFFFFFFFF, rel 0xFFFFFFFF, dlen
// 65535) or a crafted prev (nsack 7, any edges) changes values, never an address.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "interval_union.h"
#include "lvlip_skb.h"
#include "tcp_hdr_dev.h"  // lvlip_launch_status, lvlip_launched
#include "wave_ops.h"

namespace lvlip {

constexpr uint32_t ADV_TILE = 256;      // sorted elements per scan tile: one per thread
constexpr uint32_t ADV_SPINE = 64;      // lanes of the spine's one wave
constexpr uint32_t ADV_HEADS = 6;       // heads k_adv_emit looks for: five islands and the fifth one's end
constexpr int ADV_ROUNDS = 4;           // bitmap words a lane of k_adv_emit has in flight
constexpr uint64_t ADV_END_MASK = (1ull << 33) - 1u;

__device__ __forceinline__ uint64_t adv_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// flow << 33 | end of the interval
__device__ __forceinline__ uint64_t adv_val(uint64_t key, uint32_t len) {
    return ((key >> 32) << 33) | ((key & 0xFFFFFFFFull) + len);
}

// flow << 33 | start of the interval: what the scan before an element is compared with
__device__ __forceinline__ uint64_t adv_start(uint64_t key) { return ((key >> 32) << 33) | (key & 0xFFFFFFFFull); }

__global__ __launch_bounds__(256) void k_adv_keys(const lvlip_lro_rec* rec, uint32_t n, uint32_t nflows,
                                                  uint64_t* key, uint16_t* len) {
    const uint64_t i = (uint64_t)blockIdx.x * ADV_TILE + threadIdx.x;
    if (i >= n) return;
    const uint4 r = reinterpret_cast<const uint4*>(rec)[i];  // flow, rel, dlen | status << 16 | flags << 24, ack
    const bool counts = ((r.z >> 16) & 0xffu) == LVLIP_LRO_PLACED && r.x < nflows;
    key[i] = counts ? ((uint64_t)r.x << 32) | r.y : IU_NO_KEY;
    len[i] = counts ? (uint16_t)(r.z & 0xffffu) : (uint16_t)0;
}

// The carry form's keys and 4-B lengths.  The first cblocks workgroups take
// the carried blocks, four lanes per flow (so a flow's lanes share a wave);
// the others the records, as k_adv_keys does.
__global__ __launch_bounds__(256) void k_adv_keys_carry(const lvlip_lro_rec* rec, uint32_t n,
                                                        const lvlip_lro_flow* f, const lvlip_lro_result* prev,
                                                        uint32_t nflows, uint32_t cblocks, uint64_t* key,
                                                        uint32_t* len, uint32_t* ncarry) {
    if (blockIdx.x < cblocks) {
        const uint32_t t = blockIdx.x * ADV_TILE + threadIdx.x;  // below 4 * 65536 + 256
        const uint32_t k = t >> 2, j = t & 3u;
        const bool live = k < nflows;
        const uint32_t g = live ? k : 0u;
        const uint32_t rcv_nxt = f[g].rcv_nxt, rcv_wnd = f[g].rcv_wnd;
        const uint32_t nsack = prev[g].nsack;
        const uint2 blk = reinterpret_cast<const uint2*>(prev[g].sack)[j];  // left, right
        const uint32_t l = blk.x - rcv_nxt, r = blk.y - rcv_nxt;
        const bool counts = live && j < nsack && l < r && r <= rcv_wnd;
        uint32_t c = counts ? 1u : 0u;
        c += (uint32_t)__shfl_xor((int)c, 1, 64);
        c += (uint32_t)__shfl_xor((int)c, 2, 64);
        if (!live) return;
        const uint64_t slot = (uint64_t)n + t;  // below n + 4 nflows
        key[slot] = counts ? ((uint64_t)k << 32) | l : IU_NO_KEY;
        len[slot] = counts ? r - l : 0u;
        if (j == 0u) ncarry[k] = c;
        return;
    }
    const uint64_t i = (uint64_t)(blockIdx.x - cblocks) * ADV_TILE + threadIdx.x;
    if (i >= n) return;
    const uint4 r = reinterpret_cast<const uint4*>(rec)[i];
    const bool counts = ((r.z >> 16) & 0xffu) == LVLIP_LRO_PLACED && r.x < nflows;
    key[i] = counts ? ((uint64_t)r.x << 32) | r.y : IU_NO_KEY;
    len[i] = counts ? r.z & 0xffffu : 0u;
}

template <class LenT>
__global__ __launch_bounds__(256) void k_adv_reduce(const uint64_t* key, const LenT* len, uint32_t n,
                                                    uint64_t* agg) {
    __shared__ uint64_t part[ADV_TILE / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * ADV_TILE + threadIdx.x;
    uint64_t v = i < n ? adv_val(key[i], len[i]) : 0ull;  // 0 is below every element: the identity
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v = adv_max(v, __shfl_xor(v, d, 64));
    if (lane == 0u) part[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0u) agg[blockIdx.x] = adv_max(adv_max(part[0], part[1]), adv_max(part[2], part[3]));
}

// in place: agg[t] becomes the maximum of the tiles before t (0 for tile 0)
__global__ __launch_bounds__(64) void k_adv_spine(uint64_t* agg, uint32_t ntiles) {
    const uint32_t lane = threadIdx.x;
    const uint32_t per = (ntiles + ADV_SPINE - 1u) / ADV_SPINE;
    const uint64_t t0 = (uint64_t)lane * per;
    const uint64_t t1 = t0 + per < ntiles ? t0 + per : ntiles;
    uint64_t m = 0;
    for (uint64_t t = t0; t < t1; ++t) m = adv_max(m, agg[t]);
    const uint64_t incl = wave_scan_max_u64(m, lane);
    const uint64_t before = __shfl_up(incl, 1, 64);
    uint64_t carry = lane == 0u ? 0ull : before;
    for (uint64_t t = t0; t < t1; ++t) {
        const uint64_t own = agg[t];
        agg[t] = carry;
        carry = adv_max(carry, own);
    }
}

template <class LenT>
__global__ __launch_bounds__(256) void k_adv_heads(const uint64_t* key, const LenT* len, uint32_t n,
                                                   const uint64_t* agg, uint64_t* H, uint64_t* bitmap) {
    __shared__ uint64_t part[ADV_TILE / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * ADV_TILE + threadIdx.x;
    const bool live = i < n;
    const uint64_t k = live ? key[i] : 0ull;
    const uint64_t v = live ? adv_val(k, len[i]) : 0ull;
    const uint64_t in_wave = wave_scan_max_u64(v, lane);
    if (lane == 63u) part[wave] = in_wave;
    __syncthreads();
    uint64_t carry = agg[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) carry = adv_max(carry, part[w]);
    const uint64_t incl = adv_max(in_wave, carry);
    const uint64_t up = __shfl_up(incl, 1, 64);
    const uint64_t before = lane == 0u ? carry : up;  // the scan of everything before i
    const bool head = live && (i == 0u || before < adv_start(k));
    // incl's flow is i's own: no earlier element has a larger one
    if (live) H[i] = incl & ADV_END_MASK;
    const uint64_t heads = __ballot(head);
    if (lane == 0u && live) bitmap[i >> 6] = heads;
}

// k_adv_emit (ncarry NULL) and k_adv_emit_carry: of a flow's elements,
// ncarry[flow] are carried blocks, which `placed` does not count
__device__ __forceinline__ void adv_emit(const lvlip_lro_flow* f, uint32_t nflows, const uint64_t* key,
                                         const uint64_t* H, const uint64_t* bitmap, uint32_t n,
                                         lvlip_lro_result* res, const uint32_t* ncarry) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t flow = (uint64_t)blockIdx.x * (256u / 64u) + (threadIdx.x >> 6);
    if (flow >= nflows) return;  // the whole wave
    uint32_t* out = reinterpret_cast<uint32_t*>(res + flow);
    const uint32_t a = wave_lower_bound(key, n, flow << 32, lane);
    const uint32_t b = wave_lower_bound(key, n, (flow + 1u) << 32, lane);
    if (a == b) {
        if (lane < 12u) out[lane] = 0u;
        return;
    }
    // ---- the first ADV_HEADS heads of [a, b): lane j ends up with head j's index
    const uint32_t wfirst = a >> 6, wlast = (b - 1u) >> 6;
    uint32_t pos = 0u, found = 0u;
    for (uint64_t wb = wfirst; wb <= wlast && found < ADV_HEADS; wb += 64u * ADV_ROUNDS) {
        uint64_t word[ADV_ROUNDS];
#pragma unroll
        for (int r = 0; r < ADV_ROUNDS; ++r) {
            const uint64_t w = wb + 64u * (uint32_t)r + lane;
            uint64_t x = w <= wlast ? bitmap[w] : 0ull;
            if (w == wfirst) x &= ~0ull << (a & 63u);
            if (w == wlast && (b & 63u)) x &= ~0ull >> (64u - (b & 63u));
            word[r] = x;
        }
#pragma unroll
        for (int r = 0; r < ADV_ROUNDS; ++r) {
            uint64_t x = word[r];
            const uint32_t cnt = (uint32_t)__popcll(x);
            if (found >= ADV_HEADS || __ballot(cnt != 0u) == 0ull) continue;  // the same in every lane
            const uint32_t upto = wave_scan_add_u32(cnt, lane);
            const uint32_t base = found + upto - cnt;  // this lane's first head is head `base`
            const uint32_t bit0 = (uint32_t)(wb + 64u * (uint32_t)r + lane) << 6;
            for (uint32_t j = found; j < ADV_HEADS; ++j) {
                const bool own = j >= base && j < base + cnt;
                uint32_t mine = 0u;
                if (own) {
                    mine = bit0 + (uint32_t)__builtin_ctzll(x);
                    x &= x - 1u;
                }
                const uint64_t who = __ballot(own);
                if (who == 0ull) break;  // the round's heads are used up
                const uint32_t got = __shfl(mine, (int)__builtin_ctzll(who), 64);
                if (lane == j) pos = got;
            }
            const uint32_t total = found + __shfl(upto, 63, 64);
            found = total < ADV_HEADS ? total : ADV_HEADS;
        }
    }
    // ---- island j is [rel of head j, H before head j + 1); the last one found ends at b
    const uint32_t next = __shfl_down(pos, 1, 64);
    const bool isl = lane < found && lane < ADV_HEADS - 1u;
    const uint32_t stop = lane + 1u < found ? next : b;
    const uint32_t lo = isl ? (uint32_t)key[pos] : 0u;
    const uint32_t hi = isl ? (uint32_t)H[stop - 1u] : 0u;
    const uint32_t rcv_nxt = f[flow].rcv_nxt;
    const uint32_t first0 = __shfl(lo, 0, 64) == 0u ? 1u : 0u;  // the prefix: only the lowest island can start at 0
    const uint32_t delivered = first0 ? __shfl(hi, 0, 64) : 0u;
    const uint32_t nisl = found > first0 ? found - first0 : 0u;
    const uint32_t nsack = nisl < 4u ? nisl : 4u;
    const uint32_t s = lane >= 4u && lane < 12u ? (lane - 4u) >> 1 : 0u;
    const uint32_t left = __shfl(rcv_nxt + lo, (int)(s + first0), 64);
    const uint32_t right = __shfl(rcv_nxt + hi, (int)(s + first0), 64);
    uint32_t v = (lane & 1u) ? right : left;
    if (s >= nsack) v = 0u;
    if (lane == 0u) v = delivered;
    if (lane == 1u) v = b - a - (ncarry ? ncarry[flow] : 0u);
    if (lane == 2u) v = nsack;
    if (lane == 3u) v = 0u;
    if (lane < 12u) out[lane] = v;
}

__global__ __launch_bounds__(256) void k_adv_emit(const lvlip_lro_flow* f, uint32_t nflows, const uint64_t* key,
                                                  const uint64_t* H, const uint64_t* bitmap, uint32_t n,
                                                  lvlip_lro_result* res) {
    adv_emit(f, nflows, key, H, bitmap, n, res, nullptr);
}

__global__ __launch_bounds__(256) void k_adv_emit_carry(const lvlip_lro_flow* f, uint32_t nflows,
                                                        const uint64_t* key, const uint64_t* H,
                                                        const uint64_t* bitmap, uint32_t n, lvlip_lro_result* res,
                                                        const uint32_t* ncarry) {
    adv_emit(f, nflows, key, H, bitmap, n, res, ncarry);
}

struct adv_layout {
    size_t key[2], len[2], agg, bitmap, ncarry, tmp, tmp_bytes, total;
};

// n elements with lengths of LenT and counts for `counted` flows (0: none).
// false when rocPRIM's size query fails (no device)
template <class LenT>
static bool adv_plan(uint32_t n, uint32_t counted, adv_layout& L) {
    const auto query = [n](size_t& bytes) {
        rocprim::double_buffer<uint64_t> k(nullptr, nullptr);
        rocprim::double_buffer<LenT> v(nullptr, nullptr);
        return iu_sort(nullptr, bytes, k, v, n, nullptr);
    };
    if (!iu_tmp_bytes(n, query, L.tmp_bytes)) return false;
    const size_t ntiles = ((size_t)n + ADV_TILE - 1u) / ADV_TILE, words = ((size_t)n + 63u) / 64u;
    size_t at = 0;
    for (int j = 0; j < 2; ++j) L.key[j] = iu_carve(at, (size_t)n * 8u);
    for (int j = 0; j < 2; ++j) L.len[j] = iu_carve(at, (size_t)n * sizeof(LenT));
    L.agg = iu_carve(at, ntiles * 8u);
    L.bitmap = iu_carve(at, words * 8u);
    L.ncarry = iu_carve(at, (size_t)counted * 4u);
    L.tmp = iu_carve(at, L.tmp_bytes);
    L.total = at;
    return true;
}

// the scans over the sorted elements, then the results: what both forms launch behind their sort
template <class LenT>
static int adv_scan_emit(const lvlip_lro_flow* f, uint32_t nflows, const uint64_t* sorted, const LenT* slen,
                         uint32_t n, uint64_t* H, uint64_t* agg, uint64_t* bitmap, const uint32_t* ncarry,
                         lvlip_lro_result* res, hipStream_t s) {
    const uint32_t ntiles = (uint32_t)(((uint64_t)n + ADV_TILE - 1u) / ADV_TILE);
    int rc;
    hipLaunchKernelGGL(k_adv_reduce<LenT>, dim3(ntiles), dim3(ADV_TILE), 0, s, sorted, slen, n, agg);
    if ((rc = lvlip_launched("k_adv_reduce")) != LVLIP_OK) return rc;
    hipLaunchKernelGGL(k_adv_spine, dim3(1), dim3(ADV_SPINE), 0, s, agg, ntiles);
    if ((rc = lvlip_launched("k_adv_spine")) != LVLIP_OK) return rc;
    hipLaunchKernelGGL(k_adv_heads<LenT>, dim3(ntiles), dim3(ADV_TILE), 0, s, sorted, slen, n, (const uint64_t*)agg, H,
                       bitmap);
    if ((rc = lvlip_launched("k_adv_heads")) != LVLIP_OK) return rc;
    const uint32_t egrid = (uint32_t)(((uint64_t)nflows + 3u) / 4u);
    if (ncarry) {
        hipLaunchKernelGGL(k_adv_emit_carry, dim3(egrid), dim3(256), 0, s, f, nflows, sorted, (const uint64_t*)H,
                           (const uint64_t*)bitmap, n, res, ncarry);
        return lvlip_launched("k_adv_emit_carry");
    }
    hipLaunchKernelGGL(k_adv_emit, dim3(egrid), dim3(256), 0, s, f, nflows, sorted, (const uint64_t*)H,
                       (const uint64_t*)bitmap, n, res);
    return lvlip_launched("k_adv_emit");
}

// the carry form's elements, or 0 when they pass what the element indices hold
static inline uint32_t adv_carry_elems(uint32_t n, uint32_t nflows) {
    const uint64_t e = (uint64_t)n + 4ull * nflows;
    return n <= LVLIP_MAX_BATCH && nflows <= LVLIP_LRO_MAX_FLOWS && e <= LVLIP_MAX_BATCH ? (uint32_t)e : 0u;
}

// both layouts of the carry form: its own, and with prev == NULL the plain form's inside the same workspace
static bool adv_plan_carry(uint32_t n, uint32_t nflows, adv_layout& L, size_t& total) {
    if (!adv_plan<uint32_t>(adv_carry_elems(n, nflows), nflows, L)) return false;
    total = L.total;
    adv_layout P;
    if (n) {
        if (!adv_plan<uint16_t>(n, 0u, P)) return false;
        if (P.total > total) total = P.total;
    }
    return true;
}

}  // namespace lvlip

extern "C" {

size_t lvlip_lro_advance_workspace_bytes(uint32_t n, uint32_t /*nflows*/) {
    if (n == 0 || n > LVLIP_MAX_BATCH || !lvlip::iu_have_device()) return 0;
    lvlip::adv_layout L;
    return lvlip::adv_plan<uint16_t>(n, 0u, L) ? L.total : 0;
}

size_t lvlip_lro_advance_carry_workspace_bytes(uint32_t n, uint32_t nflows) {
    if (nflows == 0 || lvlip::adv_carry_elems(n, nflows) == 0 || !lvlip::iu_have_device()) return 0;
    lvlip::adv_layout L;
    size_t total = 0;
    return lvlip::adv_plan_carry(n, nflows, L, total) ? total : 0;
}

int lvlip_lro_advance_dev(const lvlip_lro_flow* f, uint32_t nflows, const lvlip_lro_rec* rec, uint32_t n,
                          lvlip_lro_result* res, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace lvlip;
    if (n > LVLIP_MAX_BATCH || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    if ((nflows && (!f || !res)) || (n && !rec)) return LVLIP_EINVAL;
    if (((uintptr_t)f & 7u) || ((uintptr_t)rec & 15u) || ((uintptr_t)res & 15u)) return LVLIP_EINVAL;
    if (nflows == 0) return LVLIP_OK;
    if (n && (!workspace || ((uintptr_t)workspace & 255u))) return LVLIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        return lvlip_launch_status(hipMemsetAsync(res, 0, (size_t)nflows * sizeof *res, s),
                                   "lvlip_lro_advance_dev: hipMemsetAsync");
    }
    adv_layout L;
    if (!adv_plan<uint16_t>(n, 0u, L)) return LVLIP_ENODEV;
    if (workspace_bytes < L.total) return LVLIP_ERANGE;

    uint8_t* ws = (uint8_t*)workspace;
    const uint32_t ntiles = (uint32_t)(((uint64_t)n + ADV_TILE - 1u) / ADV_TILE);
    rocprim::double_buffer<uint64_t> keys((uint64_t*)(ws + L.key[0]), (uint64_t*)(ws + L.key[1]));
    rocprim::double_buffer<uint16_t> lens((uint16_t*)(ws + L.len[0]), (uint16_t*)(ws + L.len[1]));
    hipError_t e;
    int rc;

    hipLaunchKernelGGL(k_adv_keys, dim3(ntiles), dim3(ADV_TILE), 0, s, rec, n, nflows, keys.current(),
                       lens.current());
    if ((rc = lvlip_launched("k_adv_keys")) != LVLIP_OK) return rc;
    size_t tmp_bytes = L.tmp_bytes;
    if ((e = iu_sort(ws + L.tmp, tmp_bytes, keys, lens, n, s)) != hipSuccess)
        return lvlip_launch_status(e, "lvlip_lro_advance_dev: radix sort");
    // H takes the key array the sort is done with
    return adv_scan_emit<uint16_t>(f, nflows, keys.current(), lens.current(), n, keys.alternate(),
                                   (uint64_t*)(ws + L.agg), (uint64_t*)(ws + L.bitmap), nullptr, res, s);
}

int lvlip_lro_advance_carry_dev(const lvlip_lro_flow* f, uint32_t nflows, const lvlip_lro_rec* rec, uint32_t n,
                                const lvlip_lro_result* prev, lvlip_lro_result* res, void* workspace,
                                size_t workspace_bytes, void* stream) {
    using namespace lvlip;
    if (n > LVLIP_MAX_BATCH || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    if ((nflows && (!f || !res)) || (n && !rec)) return LVLIP_EINVAL;
    if (((uintptr_t)f & 7u) || ((uintptr_t)rec & 15u) || ((uintptr_t)res & 15u) || ((uintptr_t)prev & 15u))
        return LVLIP_EINVAL;
    if (nflows == 0) return LVLIP_OK;
    const uint32_t elems = adv_carry_elems(n, nflows);
    if (elems == 0) return LVLIP_EINVAL;
    if ((n || prev) && (!workspace || ((uintptr_t)workspace & 255u))) return LVLIP_EINVAL;
    if (n == 0 && !prev) return lvlip_lro_advance_dev(f, nflows, rec, n, res, workspace, workspace_bytes, stream);
    adv_layout L;
    size_t total = 0;
    if (!adv_plan_carry(n, nflows, L, total)) return LVLIP_ENODEV;
    if (workspace_bytes < total) return LVLIP_ERANGE;
    // without a carry the elements are the records: the plain form's launches and its 2-B lengths
    if (!prev) return lvlip_lro_advance_dev(f, nflows, rec, n, res, workspace, workspace_bytes, stream);

    hipStream_t s = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    rocprim::double_buffer<uint64_t> keys((uint64_t*)(ws + L.key[0]), (uint64_t*)(ws + L.key[1]));
    rocprim::double_buffer<uint32_t> lens((uint32_t*)(ws + L.len[0]), (uint32_t*)(ws + L.len[1]));
    uint32_t* ncarry = (uint32_t*)(ws + L.ncarry);
    const uint32_t cblocks = (4u * nflows + ADV_TILE - 1u) / ADV_TILE;
    const uint32_t rblocks = (uint32_t)(((uint64_t)n + ADV_TILE - 1u) / ADV_TILE);
    hipError_t e;
    int rc;
    hipLaunchKernelGGL(k_adv_keys_carry, dim3(cblocks + rblocks), dim3(ADV_TILE), 0, s, rec, n, f, prev, nflows,
                       cblocks, keys.current(), lens.current(), ncarry);
    if ((rc = lvlip_launched("k_adv_keys_carry")) != LVLIP_OK) return rc;
    size_t tmp_bytes = L.tmp_bytes;
    if ((e = iu_sort(ws + L.tmp, tmp_bytes, keys, lens, elems, s)) != hipSuccess)
        return lvlip_launch_status(e, "lvlip_lro_advance_carry_dev: radix sort");
    return adv_scan_emit<uint32_t>(f, nflows, keys.current(), lens.current(), elems, keys.alternate(),
                                   (uint64_t*)(ws + L.agg), (uint64_t*)(ws + L.bitmap), ncarry, res, s);
}

}  // extern "C"
