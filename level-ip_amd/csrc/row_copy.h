// row_copy.h — the pieces a 16-lane DPP row uses to move one frame's payload
// between two byte streams of any mutual alignment and sum it on the way:
// shared by k_tso (seg_kernels.hip: payload -> frames) and k_lro
// (rcv_kernels.hip: frames -> payload).  Everything is laid out by DESTINATION
// chunk (seg_kernels.hip's header comment has the reasoning).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "csum_dev.h"

namespace lvlip {

constexpr uint32_t ROW = 16;  // lanes per frame: one DPP row

// u32 sum over each 16-lane DPP row, left in every lane of the row
// (quad_perm(1,0,3,2), quad_perm(2,3,0,1), row_ror:4, row_ror:8)
__device__ __forceinline__ uint32_t row_sum_dpp(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);
    return v;
}

// bytes [sh, sh + 16) of the 32 bytes lo:hi, 0 <= sh <= 15
__device__ __forceinline__ uint4 funnel16(const uint4 lo, const uint4 hi, uint32_t sh) {
    const uint32_t q = sh >> 2, r = sh & 3u;
    const uint32_t e0 = q == 0u ? lo.x : q == 1u ? lo.y : q == 2u ? lo.z : lo.w;
    const uint32_t e1 = q == 0u ? lo.y : q == 1u ? lo.z : q == 2u ? lo.w : hi.x;
    const uint32_t e2 = q == 0u ? lo.z : q == 1u ? lo.w : q == 2u ? hi.x : hi.y;
    const uint32_t e3 = q == 0u ? lo.w : q == 1u ? hi.x : q == 2u ? hi.y : hi.z;
    const uint32_t e4 = q == 0u ? hi.x : q == 1u ? hi.y : q == 2u ? hi.z : hi.w;
    return make_uint4(__builtin_amdgcn_alignbyte(e1, e0, r), __builtin_amdgcn_alignbyte(e2, e1, r),
                      __builtin_amdgcn_alignbyte(e3, e2, r), __builtin_amdgcn_alignbyte(e4, e3, r));
}

// word sum of a destination-aligned chunk, added to acc; sel swaps the bytes
// of every u16 for frames at odd addresses
__device__ __forceinline__ uint32_t chunk_acc(const uint4 v, uint32_t sel, uint32_t acc) {
    acc = dot2_acc(__builtin_amdgcn_perm(v.x, v.x, sel), acc);
    acc = dot2_acc(__builtin_amdgcn_perm(v.y, v.y, sel), acc);
    acc = dot2_acc(__builtin_amdgcn_perm(v.z, v.z, sel), acc);
    acc = dot2_acc(__builtin_amdgcn_perm(v.w, v.w, sel), acc);
    return acc;
}

__device__ __forceinline__ uint32_t halves(uint32_t x) { return (x & 0xffffu) + (x >> 16); }

__device__ __forceinline__ uint32_t bswap16u(uint32_t x) { return ((x & 0xffu) << 8) | ((x >> 8) & 0xffu); }

// Bytes [b0, b1) of the chunk at the 16-B aligned address a: a whole chunk as
// one nontemporal 16-B store, a partial one as the dwords and bytes inside the
// range (plain vector stores), nothing outside it.
__device__ __forceinline__ void store_chunk(uint64_t a, const uint4 v, int b0, int b1) {
    typedef __attribute__((address_space(1))) u32x4 gvec;
    typedef __attribute__((address_space(1))) uint32_t gdw;
    typedef __attribute__((address_space(1))) uint8_t gby;
    if (b0 <= 0 && b1 >= 16) {
        __builtin_nontemporal_store(u32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<gvec*>(a));
        return;
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int s = min(max(b0 - 4 * d, 0), 4);
        const int e = min(max(b1 - 4 * d, 0), 4);
        if (s == 0 && e == 4) {
            *reinterpret_cast<gdw*>(a + 4u * d) = w[d];
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b >= s && b < e) *reinterpret_cast<gby*>(a + 4u * d + b) = (uint8_t)(w[d] >> (8 * b));
        }
    }
}

// One round of a row's sweep over a destination range: U destination chunks
// per lane (chunk k0 + 16 u + tl of nch).  Chunk k's byte j is byte
// 16 k - lead + j of the `dlen` source bytes at S (lead = the bytes in front
// of them in destination chunk 0).  Loads the one or two aligned source chunks
// that hold them, never a chunk without a byte of the range, and leaves the
// funnelled, masked chunk (zero outside the range) in v[u].
template <int U, bool NT>
__device__ __forceinline__ void row_gather(uint64_t S, int lead, uint32_t dlen, uint32_t nch, uint32_t k0,
                                           uint32_t tl, uint4 (&v)[U]) {
    uint4 lo[U], hi[U];
    int jlo[U], jhi[U];
    uint32_t sh[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t k = k0 + (uint32_t)u * ROW + tl;
        const int rel = (int)(16u * k) - lead;
        jlo[u] = min(max(-rel, 0), 16);
        jhi[u] = min(max((int)dlen - rel, 0), 16);
        const bool has = k < nch && jlo[u] < jhi[u];
        if (!has) jlo[u] = jhi[u] = 0;
        const uint64_t A = S + (uint64_t)(int64_t)rel;
        const uint64_t a0 = A & ~15ull;
        sh[u] = (uint32_t)(A & 15ull);
        const bool need_lo = has && (int)sh[u] + jlo[u] < 16;
        const bool need_hi = has && (int)sh[u] + jhi[u] > 16;
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        lo[u] = need_lo ? (NT ? load_nt_global(a0) : load_global(a0)) : z;
        hi[u] = need_hi ? (NT ? load_nt_global(a0 + 16u) : load_global(a0 + 16u)) : z;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = mask_chunk(funnel16(lo[u], hi[u], sh[u]), jlo[u], jhi[u]);
}

}  // namespace lvlip
