// ack_kernels.hip — the acknowledgement of a coalesced batch on the device
// (include/lvlip_skb.h, "f1 on the device: the acknowledgement"): per planned
// flow a 54-byte header template, rcv_nxt and the lvlip_lro_result that
// lvlip_lro_advance_dev left in HBM -> one finished pure ACK with its SACK
// option, every byte what ack_cpu.c writes.  One launch, nothing but loads and
// stores: no workspace, no atomics, no LDS.
//
// Work mapping.  Eight lanes per flow, eight flows per wave, 32 per 256-thread
// workgroup.  A frame is at most 90 bytes at any address F, so it touches at
// most (15 + 90 + 15) / 16 = 7 aligned 16-B chunks: lane c of the group owns
// destination chunk c, the 16 aligned bytes at (F & ~15) + 16 c.  The work is
// latency-bound (three dependent-free loads, some hundred VALU instructions,
// one store per lane), so nothing is shared between the lanes of a group:
// every lane loads the flow's 64 + 4 + 48 bytes (the same addresses in all
// eight lanes: one request), builds the whole frame in registers and keeps
// its own chunk.
//
// The frame in registers.  Dwords h[0..13] are the template's 54 bytes (the
// top half of h[13] is replaced), patched as tcp_transmit_skb and ip_output
// patch them (tcp_hdr_dev.h; k_tso does the same for data segments).  The option
// starts at byte 54 = 2 mod 4, so its nine dwords ow[0..8] (01 01 05 len, then
// left and right of each block in network order, zero beyond the b blocks
// written) straddle the frame's dwords: frame dword 13 is urp | ow[0] << 16
// and dword 13 + i is ow[i-1] >> 16 | ow[i] << 16.  Both word sums are taken
// from the registers: the TCP header starts at byte 34, so its u16 words are
// the halves of h[8..13] and of ow[], and zero dwords add nothing.
//
// Which block goes where (sack[b-1-i] at position i, b known only at run time)
// and which 16 bytes a lane keeps (chunk c at frame offset 16 c - (F & 15))
// are selected with compare masks over registers with constant indices
// (ack_sel4 here, hdr_chunk in tcp_hdr_dev.h), never with a runtime index into
// an array, which hipcc would put in scratch.
// Chunks the frame covers whole leave as one 16-B store; the first and the
// last leave as the dwords and bytes inside [F, F + 54 + optlen) and nothing
// else (store_chunk, row_copy.h), so the rest of a 90-byte slot and an abutting
// neighbour's frame are never written.
//
// Bounds.  Every load index is below nflows (a group past the end reads flow 0
// and stores nothing); b is clamped to 4 whatever res holds; a lane stores only
// while its chunk index is below ceil(((F & 15) + 54 + optlen) / 16) <= 7, and
// then only bytes of the frame.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "csum_dev.h"
#include "row_copy.h"
#include "tcp_hdr_dev.h"

namespace lvlip {

constexpr uint32_t ACK_GROUP = 8;                  // lanes per flow
constexpr uint32_t ACK_FLOWS = 256 / ACK_GROUP;    // flows per workgroup
constexpr int ACK_HDR = TCP_FRAME_HDR;
constexpr int ACK_BLOCKS = 6;                      // 16-B blocks of the frame's 23 dwords

// a[j] for j = 0 .. 3, 0 beyond
__device__ __forceinline__ uint32_t ack_sel4(uint32_t j, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3) {
    return (j == 0u ? a0 : 0u) | (j == 1u ? a1 : 0u) | (j == 2u ? a2 : 0u) | (j == 3u ? a3 : 0u);
}

__global__ __launch_bounds__(256) void k_ack(const lvlip_ack_tmpl* t, const lvlip_lro_flow* f,
                                             const lvlip_lro_result* res, uint32_t nflows, uint32_t flags,
                                             uint8_t* out, lvlip_frame_desc* fd) {
    const uint32_t c = threadIdx.x & (ACK_GROUP - 1u);  // this lane's destination chunk
    const uint64_t g64 = (uint64_t)blockIdx.x * ACK_FLOWS + (threadIdx.x / ACK_GROUP);
    const bool live = g64 < nflows;
    const uint32_t g = live ? (uint32_t)g64 : 0u;

    // ---- the flow's inputs: 8 x 8 B of the template (8-B aligned), rcv_nxt, 3 x 16 B of the result
    const uint2* tw = reinterpret_cast<const uint2*>(t + g);
    uint2 tv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) tv[k] = tw[k];
    const uint32_t rcv_nxt = f[g].rcv_nxt;
    const uint4* rw = reinterpret_cast<const uint4*>(res + g);
    const uint4 r0 = rw[0], r1 = rw[1], r2 = rw[2];  // delivered placed nsack -, sack[0] sack[1], sack[2] sack[3]

    const uint64_t off = (uint64_t)tv[0].x | ((uint64_t)tv[0].y << 32);
    uint32_t h[14];
#pragma unroll
    for (int k = 0; k < 7; ++k) h[2 * k] = tv[k + 1].x, h[2 * k + 1] = tv[k + 1].y;
    const uint32_t max_sack = (h[13] >> 16) & 0xffu;

    const bool acked = live && ((flags & LVLIP_ACK_ALL) != 0u || r0.y != 0u);
    uint32_t b = r0.z < 4u ? r0.z : 4u;  // tcp_options_len, src/tcp_output.c:227-245
    b = b < max_sack ? b : max_sack;
    const uint32_t optlen = b ? 4u + 8u * b : 0u;
    const int L = ACK_HDR + (int)optlen;

    // ---- the option: position i holds sack[b - 1 - i] (src/tcp_output.c:78-86)
    uint32_t ow[9];
    ow[0] = b ? 0x00050101u | ((2u + 8u * b) << 24) : 0u;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t j = b - 1u - i;  // wraps to >= 4 for i >= b: nothing selected
        ow[1 + 2 * i] = __builtin_bswap32(ack_sel4(j, r1.x, r1.z, r2.x, r2.z));
        ow[2 + 2 * i] = __builtin_bswap32(ack_sel4(j, r1.y, r1.w, r2.y, r2.w));
    }

    // ---- the 54 header bytes
    h[4] = (h[4] & 0xffff0000u) | bswap16u(40u + optlen);       // ip.len, src/ip_output.c:35,46
    h[6] &= 0xffff0000u;                                          // ip.csum = 0, src/ip_output.c:42
    const uint32_t ipw = (h[3] >> 16) + halves(h[4]) + halves(h[5]) + halves(h[6]) + halves(h[7]) +
                         (h[8] & 0xffffu);
    h[6] |= (uint32_t)finish(0u, ipw);                            // ip_send_check, src/ip_output.c:8-12
    hdr_put_ack(h, __builtin_bswap32(rcv_nxt + r0.x));
    h[11] = (h[11] & 0xff0fffffu) | ((5u + optlen / 4u) << 20);   // hl, src/tcp_output.c:261
    h[12] &= 0xffffu;                                             // tcp.csum = 0, src/tcp_output.c:110
    h[13] = (h[13] & 0xffffu) | (ow[0] << 16);                    // urp, then the option's first two bytes
    uint32_t thw = hdr_tcp_words(h);
#pragma unroll
    for (int i = 0; i < 9; ++i) thw += halves(ow[i]);
    h[12] |= (uint32_t)finish(hdr_tcp_seed(h, 20u + optlen), thw) << 16;  // src/tcp_output.c:126

    // ---- the frame's dwords as six 16-B blocks; dword 13 + i = ow[i-1] >> 16 | ow[i] << 16
    uint32_t w[10];  // frame dwords 14 .. 23 (22 ends the longest frame; 23 is zero)
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = (ow[i] >> 16) | (ow[i + 1] << 16);
    w[8] = ow[8] >> 16;
    w[9] = 0u;
    const uint4 blk[ACK_BLOCKS] = {make_uint4(h[0], h[1], h[2], h[3]),   make_uint4(h[4], h[5], h[6], h[7]),
                                   make_uint4(h[8], h[9], h[10], h[11]), make_uint4(h[12], h[13], w[0], w[1]),
                                   make_uint4(w[2], w[3], w[4], w[5]),   make_uint4(w[6], w[7], w[8], w[9])};

    // ---- lane c keeps destination chunk c
    const uint64_t F = reinterpret_cast<uint64_t>(out) + off;  // the frame's first byte
    const int fo = (int)(F & 15ull);
    const uint64_t D = F - (uint64_t)fo;
    const uint32_t nch = acked ? (uint32_t)(fo + L + 15) >> 4 : 0u;  // chunks the frame touches: 4 .. 7
    if (c < nch) store_chunk(D + 16ull * c, hdr_chunk(c, fo, blk), c == 0u ? fo : 0, min(16, fo + L - (int)(16u * c)));
    if (fd && live && c == 0u)
        store_global(reinterpret_cast<uint64_t>(fd + g),
                     u32x4{(uint32_t)off, (uint32_t)(off >> 32), acked ? (uint32_t)L : 0u, 0u});
}

}  // namespace lvlip

extern "C" {

int lvlip_ack_dev(const lvlip_ack_tmpl* t, const lvlip_lro_flow* f, const lvlip_lro_result* res, uint32_t nflows,
                  uint32_t flags, void* out, lvlip_frame_desc* fd, void* stream) {
    if (nflows == 0) return LVLIP_OK;
    if (!t || !f || !res || !out) return LVLIP_EINVAL;
    if ((flags & ~LVLIP_ACK_ALL) || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    if (((uintptr_t)t & 7u) || ((uintptr_t)f & 7u) || ((uintptr_t)res & 15u) || ((uintptr_t)fd & 15u))
        return LVLIP_EINVAL;
    const uint32_t grid = (nflows + lvlip::ACK_FLOWS - 1u) / lvlip::ACK_FLOWS;
    hipLaunchKernelGGL(lvlip::k_ack, dim3(grid), dim3(256), 0, (hipStream_t)stream, t, f, res, nflows, flags,
                       (uint8_t*)out, fd);
    return lvlip_launch_status(hipGetLastError(), "k_ack");
}

}  // extern "C"
