// tcp_hdr_dev.h — the 54 header bytes of an Ethernet/IPv4/TCP frame in
// registers, as k_tso (seg_kernels.hip), k_ack (ack_kernels.hip) and k_rtx
// (snd_kernels.hip) patch and sum them, and the small pieces these kernels and
// k_lro (rcv_kernels.hip) repeat around them.  tcp_hdr.h is the same
// arithmetic on the CPU.
//
// The frame's dwords.  h[k] holds frame bytes 4 k .. 4 k + 3 as loaded (little
// endian): the IPv4 header starts at byte 14, the upper half of h[3], and the
// TCP header at byte 34, the upper half of h[8].  Both word sums are taken from
// the registers: a header's u16 words are the halves of its dwords.  The TCP
// sum W is folded once, on (seed + W) mod 2^32 (finish, src/utils.c:46-54),
// where the seed loses the carry out of bit 31 as the reference's does.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "csum_dev.h"
#include "row_copy.h"

namespace lvlip {

constexpr int TCP_FRAME_HDR = 54;  // Ethernet 14 + IPv4 20 + TCP 20

// tcp_udp_checksum's start value for l4len bytes of TCP (src/tcp.c:92-95):
// u32 adds, the carry out of bit 31 is lost
__device__ __forceinline__ uint32_t hdr_tcp_seed(const uint32_t* h, uint32_t l4len) {
    const uint32_t saddr = (h[6] >> 16) | (h[7] << 16), daddr = (h[7] >> 16) | (h[8] << 16);
    return saddr + daddr + 0x0600u + bswap16u(l4len);
}

// the word sum of the TCP header's 20 bytes, frame bytes 34 .. 53
__device__ __forceinline__ uint32_t hdr_tcp_words(const uint32_t* h) {
    return (h[8] >> 16) + halves(h[9]) + halves(h[10]) + halves(h[11]) + halves(h[12]) + (h[13] & 0xffffu);
}

// tcp_transmit_skb's ack_seq (src/tcp_output.c:107,122), frame bytes 42 .. 45; ack in network order
__device__ __forceinline__ void hdr_put_ack(uint32_t* h, uint32_t ack) {
    h[10] = (h[10] & 0xffffu) | (ack << 16);
    h[11] = (h[11] & 0xffff0000u) | (ack >> 16);
}

// block j - 1 of blk[] (zeros for j == 0 and j > N): compare masks over
// registers with constant indices, not a select chain or a runtime index,
// which hipcc turns into a table in scratch
template <int N>
__device__ __forceinline__ uint4 pick_block(uint32_t j, const uint4 (&blk)[N]) {
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint32_t m = j == (uint32_t)i + 1u ? ~0u : 0u;
        r.x |= blk[i].x & m;
        r.y |= blk[i].y & m;
        r.z |= blk[i].z & m;
        r.w |= blk[i].w & m;
    }
    return r;
}

// Destination chunk c of a frame whose dwords are blk[] and whose first byte
// is byte fo of chunk 0: bytes [16 c + 16 - fo, 16 c + 32 - fo) of
// {16 zero bytes, the blocks, zeros}
template <int N>
__device__ __forceinline__ uint4 hdr_chunk(uint32_t c, int fo, const uint4 (&blk)[N]) {
    const uint4 nx = pick_block(c + 1u, blk);
    const uint4 cu = fo == 0 ? nx : pick_block(c, blk);
    return funnel16(cu, nx, (uint32_t)(16 - fo) & 15u);
}

// The owner of slot g of a plan's running count: the last of s[0 .. n) whose
// KEY is <= g.  KEY never falls along s and s[0]'s is 0; among records that
// share a KEY only the last owns a slot.
template <auto KEY, class T>
__device__ __forceinline__ uint32_t slot_owner(const T* s, uint32_t n, uint32_t g) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (s[mid].*KEY <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// one 16-byte record (an lvlip_frame_desc, an lvlip_lro_rec) at the 16-B
// aligned address a: one store, the counterpart of load_global (csum_dev.h)
__device__ __forceinline__ void store_global(uint64_t a, const u32x4 v) {
    typedef __attribute__((address_space(1))) u32x4 gvec;
    *reinterpret_cast<gvec*>(a) = v;
}

// the four bytes at any address a: the one or two aligned dwords that hold them
__device__ __forceinline__ uint32_t load_u32_any(uint64_t a) {
    typedef __attribute__((address_space(1))) const uint32_t gdw;
    const uint64_t a0 = a & ~3ull;
    const uint32_t r = (uint32_t)(a & 3ull);
    const uint32_t lo = *reinterpret_cast<gdw*>(a0);
    const uint32_t hi = r ? *reinterpret_cast<gdw*>(a0 + 4u) : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, r);
}

// "Which records carry an ACK" (include/lvlip_skb.h): the flow of the record r
// (flow, rel, dlen | status << 16 | flags << 24, ack_seq) when it counts for
// lvlip_snd_* and lvlip_sack_*, else 0xFFFFFFFF.  First check,
// src/tcp_input.c:106-107, on the segment's start; fifth check, :312.
__device__ __forceinline__ uint32_t rec_ack_flow(const uint4 r, const lvlip_lro_flow* f, uint32_t nflows) {
    const uint32_t status = (r.z >> 16) & 0xffu, flags = r.z >> 24;
    const bool kind = status == LVLIP_LRO_PLACED || status == LVLIP_LRO_NO_DATA || status == LVLIP_LRO_OUT_OF_WINDOW;
    if (r.x < nflows && kind && (flags & 0x10u)) {
        if (r.y <= f[r.x].rcv_wnd) return r.x;
    }
    return 0xFFFFFFFFu;
}

// The refusals of lvlip_rtx_* on the dwords a (frame bytes 14-17) and b (bytes
// 44-47) of a queue entry of len >= 54 bytes: version | ihl 0x45, the segment
// inside the entry, hl at least 5 and inside the segment
__device__ __forceinline__ bool rtx_frame_ok(uint32_t a, uint32_t b, uint32_t len, uint32_t* iplen, uint32_t* hl) {
    *iplen = bswap16u(a >> 16);
    *hl = (b >> 20) & 0xfu;
    return (a & 0xffu) == 0x45u && 14u + *iplen <= len && *hl >= 5u && 20u + 4u * *hl <= *iplen;
}

}  // namespace lvlip

// What a device call returns for the status of its launch or enqueued step
// (csum_kernels.hip, hidden): LVLIP_OK, LVLIP_ENODEV for hipErrorNoDevice, else
// LVLIP_EHIP with "what: <HIP's text>" left for lvlip_last_hip_error().
extern "C" int lvlip_launch_status(hipError_t e, const char* what);

// the same for the kernel just launched
static inline int lvlip_launched(const char* what) { return lvlip_launch_status(hipGetLastError(), what); }

// An entry point's alignment refusal: whether one of the pointers is not a
// multiple of A bytes (8 for flow arrays, 16 for records, descriptors and
// results, which the kernels load as vectors).  NULL passes.
template <uintptr_t A, class... P>
static inline bool any_misaligned(const P*... p) {
    return (... || (((uintptr_t)p & (A - 1u)) != 0u));
}
