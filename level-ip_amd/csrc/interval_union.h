// interval_union.h — what the advance step (adv_kernels.hip: records) and the
// scoreboard (sack_kernels.hip: SACK blocks) share on the way to a union of
// intervals per flow.  An interval's key is flow << 32 | start.  The keys are
// sorted, with a value that gives the interval's end; a max-scan of
// flow | end over the sorted array then leaves in H[i] the largest end so far
// inside i's flow: the flow sits above the end and never decreases along the
// array, which makes a plain maximum segmented.  Element i heads an island
// where the scan before it is below flow | start of i: another flow, or
// every end so far below its start (intervals that touch are one island).
// The scan is each file's own (k_adv_reduce, k_adv_spine and k_adv_heads in
// the advance step, rocPRIM's in the scoreboard: DESIGN.md §9c has the timings
// that keep them apart); the keys, the sort, the workspace's parts and the size
// query are in this file.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

namespace lvlip {

constexpr uint32_t IU_KEY_BITS = 49;              // 17 bits of flow above 32 of start
constexpr uint64_t IU_NO_KEY = 0x10000ull << 32;  // an element that does not count: it sorts behind every flow

static inline size_t up256(size_t x) { return (x + 255u) & ~(size_t)255u; }

// the workspace's next part, 256-B aligned: its offset, and `at` moves behind it
static inline size_t iu_carve(size_t& at, size_t bytes) {
    const size_t part = at;
    at += up256(bytes);
    return part;
}

// stable and deterministic; equal keys may differ in their values only, and
// neither a running maximum nor a test against it depends on their order
template <class V>
static hipError_t iu_sort(void* tmp, size_t& bytes, rocprim::double_buffer<uint64_t>& k, rocprim::double_buffer<V>& v,
                          uint32_t n, hipStream_t st) {
    return rocprim::radix_sort_pairs(tmp, bytes, k, v, n, 0u, IU_KEY_BITS, st);
}

// The temporary storage a step's rocPRIM calls need for n elements: query(bytes)
// asks rocPRIM, which asks the runtime for the device's architecture, so the
// answer is kept per step (Query's type, which holds the calls and their value
// types), element count, device and thread.  false when the query fails (no device)
template <class Query>
static bool iu_tmp_bytes(uint32_t n, Query query, size_t& bytes) {
    static thread_local uint32_t seen_n = 0;
    static thread_local int seen_dev = -1;
    static thread_local size_t seen_bytes = 0;
    int device = -1;
    if (hipGetDevice(&device) != hipSuccess) return false;
    if (n != seen_n || device != seen_dev) {
        size_t b = 0;
        if (query(b) != hipSuccess) return false;
        seen_n = n;
        seen_dev = device;
        seen_bytes = b;
    }
    bytes = seen_bytes;
    return true;
}

// what a *_workspace_bytes call answers 0 without
static inline bool iu_have_device() {
    int devices = 0;
    return hipGetDeviceCount(&devices) == hipSuccess && devices > 0;
}

}  // namespace lvlip
