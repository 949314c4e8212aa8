// wave_search.h — the 64-way search over a sorted key array that k_adv_emit
// (adv_kernels.hip) and k_sack_mark (sack_kernels.hip) find a flow's range with.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace lvlip {

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
