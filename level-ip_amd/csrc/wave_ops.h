// wave_ops.h — what one 64-lane wave does as a whole in the protocol kernels:
// the 64-way search over a sorted key array that k_adv_emit (adv_kernels.hip)
// and k_sack_mark (sack_kernels.hip) find a flow's range with, the sums, maxima
// and scans they, k_snd_rec (snd_kernels.hip), k_wnd_rec (rto_kernels.hip) and
// k_cc_sum (cc_kernels.hip) reduce with, and the flow-by-flow loop k_snd_rec,
// k_wnd_rec and k_sack_parse run before their atomics.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace lvlip {

// the sum of the wave's 64 values, in every lane
__device__ __forceinline__ uint32_t wave_add_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

// their maximum, in every lane
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off, 64));
    return v;
}

// the same on 64-bit values: k_cc_sum's byte sum (cc_kernels.hip) and k_wnd_rec's keys (rto_kernels.hip)
__device__ __forceinline__ uint64_t wave_add_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    return v;
}

// and their maximum
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 64);
        v = v > o ? v : o;
    }
    return v;
}

// the sum of lanes 0 .. lane
__device__ __forceinline__ uint32_t wave_scan_add_u32(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// the maximum of lanes 0 .. lane
__device__ __forceinline__ uint64_t wave_scan_max_u64(uint64_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t o = __shfl_up(v, d, 64);
        if (lane >= d) v = v > o ? v : o;
    }
    return v;
}

// The wave's pending lanes, flow by flow, before any atomic: reduce(fl, mine)
// runs in every lane for the flow fl of the first pending lane, mine set in
// fl's pending lanes, which are then done; ROUNDS times.  So a batch of one
// flow costs a wave a few atomics, not 64 on one address.  Returns whether the
// lane is still pending: it belongs to a wave of many flows, whose addresses
// do not collide, and issues its own atomics.  The callers' lambdas capture by
// value: with captures by reference hipcc gives k_sack_parse 50 VGPRs, not 46.
template <int ROUNDS, class Reduce>
__device__ __forceinline__ bool wave_peel(bool pending, uint32_t flow, Reduce reduce) {
    uint64_t todo = __builtin_amdgcn_ballot_w64(pending);
    for (int it = 0; it < ROUNDS && todo; ++it) {
        const uint32_t fl = (uint32_t)__builtin_amdgcn_readlane((int)flow, __builtin_ctzll(todo));
        const bool mine = pending && flow == fl;
        reduce(fl, mine);
        todo &= ~__builtin_amdgcn_ballot_w64(mine);
        if (mine) pending = false;
    }
    return pending;
}

// the first index of key[0, n) whose key is not below target; every lane gets it
__device__ __forceinline__ uint32_t wave_lower_bound(const uint64_t* key, uint32_t n, uint64_t target,
                                                     uint32_t lane) {
    uint32_t lo = 0, hi = n;  // key[< lo] < target <= key[>= hi]
    while (lo < hi) {
        const uint64_t step = ((uint64_t)(hi - lo) + 63u) / 64u;
        const uint64_t p = lo + lane * step;  // 64 probes, ascending
        const bool less = p < hi && key[p] < target;
        const uint32_t c = (uint32_t)__popcll(__ballot(less));  // the keys ascend: the first c probes
        if (c == 0u) {
            hi = lo;
        } else {
            const uint64_t top = lo + c * step;
            lo = (uint32_t)(lo + (c - 1u) * step + 1u);
            if (top < hi) hi = (uint32_t)top;
        }
    }
    return lo;
}

}  // namespace lvlip
