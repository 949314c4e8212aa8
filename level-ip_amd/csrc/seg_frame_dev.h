// seg_frame_dev.h — one segment of tcp_send built by one DPP row: the body
// k_tso (seg_kernels.hip) and k_push (push_kernels.hip) share.  Payload copy
// and TCP checksum in one pass, the 54 header bytes built in registers, the
// chunks that hold header bytes merged with their payload bytes and stored
// last; seg_kernels.hip's head comment has the layout and the parity argument.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "csum_dev.h"
#include "row_copy.h"
#include "tcp_hdr_dev.h"

namespace lvlip {

constexpr uint32_t TSO_ROW = 16;                 // lanes per segment
constexpr uint32_t TSO_SEGS = 256 / TSO_ROW;     // segments per workgroup
constexpr int TSO_U = 4;                         // sweeps of a row in flight
constexpr int TSO_HDR = TCP_FRAME_HDR;

// The frame of one segment, by the 16 lanes of a row (tl = the lane's index in
// it; every argument the same in all of them).  h[0..13] are the template's
// dwords as loaded (h[13]'s upper half is whatever follows the template); IP
// length, both checksums and seq are written here.  patch(h), called behind
// the payload sweep, returns the segment's seq in host order and may set other
// fields of the template first.  F is the frame's first byte, S the segment's
// first payload byte (both any alignment); FIN and PSH of the template stay on
// a `last` segment only.  A row that is not live loads and
// stores nothing.  Exactly the 54 + dlen bytes at F are stored.
template <class PATCH>
__device__ __forceinline__ void tso_frame(uint32_t tl, bool live, uint32_t (&h)[14], uint64_t F, uint64_t S,
                                          uint32_t dlen, bool last, PATCH&& patch) {
    const int f = (int)(F & 15ull);
    const uint64_t D = F - (uint64_t)f;                            // destination chunk 0
    const int L = TSO_HDR + (int)dlen;
    const uint32_t nch = live ? (uint32_t)(f + L + 15) >> 4 : 0u;  // chunks the frame touches
    const uint32_t hk = (uint32_t)(f + TSO_HDR + 15) >> 4;         // of them with header bytes: 4 or 5
    const uint32_t sel = (F & 1ull) ? 0x02030001u : 0x03020100u;

    // ---- payload: copy and sum, destination chunk by destination chunk
    uint32_t acc = 0;
    uint4 keep = make_uint4(0u, 0u, 0u, 0u);  // the payload bytes of this lane's header chunk
    for (uint32_t k0 = 0; k0 < nch; k0 += TSO_ROW * TSO_U) {
        // chunk k's byte j is payload byte 16 k - f - 54 + j of the segment
        uint4 v[TSO_U];
        row_gather<TSO_U, true>(S, f + TSO_HDR, dlen, nch, k0, tl, v);
#pragma unroll
        for (int u = 0; u < TSO_U; ++u) {
            const uint32_t k = k0 + (uint32_t)u * TSO_ROW + tl;
            acc = chunk_acc(v[u], sel, acc);
            if (k < nch) {
                if (k >= hk) store_chunk(D + 16ull * k, v[u], 0, min(16, f + L - (int)(16u * k)));
                else keep = v[u];  // k = tl < hk <= 5: the first round's first sweep
            }
        }
    }
    const uint32_t W = row_sum_dpp(acc);  // the payload's word sum, in every lane of the row

    // ---- the 54 header bytes (every lane of the row the same)
    const uint32_t seq = patch(h);
    h[13] &= 0xffffu;                                             // bytes 52-53; the rest is not the template's
    h[4] = (h[4] & 0xffff0000u) | bswap16u(40u + dlen);         // ip.len, src/ip_output.c:35,46
    h[6] &= 0xffff0000u;                                          // ip.csum = 0, src/ip_output.c:42
    const uint32_t ipw = (h[3] >> 16) + halves(h[4]) + halves(h[5]) + halves(h[6]) + halves(h[7]) +
                         (h[8] & 0xffffu);
    h[6] |= (uint32_t)finish(0u, ipw);                            // ip_send_check, src/ip_output.c:8-12
    const uint32_t nseq = __builtin_bswap32(seq);                 // src/tcp_output.c:106,121
    h[9] = (h[9] & 0xffffu) | (nseq << 16);
    h[10] = (h[10] & 0xffff0000u) | (nseq >> 16);
    if (!last) h[11] &= ~(0x09u << 24);                           // FIN, PSH: the last segment's
    h[12] &= 0xffffu;                                             // tcp.csum = 0, src/tcp_output.c:110
    const uint32_t thw = hdr_tcp_words(h);
    h[12] |= (uint32_t)finish(hdr_tcp_seed(h, 20u + dlen), thw + W) << 16;  // src/tcp_output.c:126

    // ---- the chunks with header bytes, merged with the payload bytes kept back
    if (tl < hk && tl < nch) {
        const uint4 blk[4] = {make_uint4(h[0], h[1], h[2], h[3]), make_uint4(h[4], h[5], h[6], h[7]),
                              make_uint4(h[8], h[9], h[10], h[11]), make_uint4(h[12], h[13], 0u, 0u)};
        const uint4 hv = hdr_chunk(tl, f, blk);
        const uint4 v = make_uint4(keep.x | hv.x, keep.y | hv.y, keep.z | hv.z, keep.w | hv.w);
        store_chunk(D + 16ull * tl, v, tl == 0u ? f : 0, min(16, f + L - (int)(16u * tl)));
    }
}

}  // namespace lvlip
