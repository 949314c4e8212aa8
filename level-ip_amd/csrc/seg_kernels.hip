// seg_kernels.hip — TCP segmentation on the device (include/lvlip_skb.h, "f2 on
// the device: segmentation"): payload in HBM + one 54-byte header template per
// send -> finished Ethernet/IPv4/TCP frames, payload copy and TCP checksum in
// one pass (one read, one write of every payload byte).  seg_cpu.c is the same
// on the calling thread, bit for bit.
//
// Work mapping.  One DPP row (16 lanes) per segment, four segments per wave,
// 16 per 256-thread workgroup; segment g -> send by a binary search over the
// sends' seg0 (lvlip_tso_plan's running count).  A row sweeps its segment's
// destination chunks 16 at a time, TSO_U sweeps (1 KiB of one frame) in flight
// per row: a 590-B frame (MSS 536) is 38 chunks = one round at 59 % of the
// lanes, a 1514-B frame two rounds' worth at 100 %, a 9000-B frame nine rounds;
// a wave always has four frames' streams going.  The kernel cannot pick the
// shape per send from the host (the sends are in device memory), so the row
// is the one shape for every MSS.
//
// Alignment.  Everything is laid out by DESTINATION chunk: chunk k of a frame
// at address F is the 16 aligned bytes at (F & ~15) + 16 k.  Its payload bytes
// come from source address A = S + 16 k - (F & 15) - 54 onwards (S = the
// segment's first payload byte), which is independent of F mod 16: the lane
// loads the one or two aligned source chunks that hold them (never a chunk
// without a byte of the segment's payload) and funnels bytes [A & 15,
// (A & 15) + 16) out of the pair (v_alignbyte).  Whole chunks leave as 16-B
// nontemporal stores (nobody on this XCD reads a frame again; `nt` keeps the
// line policy streaming, MI355X store table); a frame's first and last chunk,
// when the frame covers only part of them, leave as dword and byte stores of
// exactly the frame's bytes, so a stride gap or an abutting neighbour frame is
// never written.
//
// Checksum parity.  The reference sums the TCP segment's u16 words, which are
// aligned to the TCP header: frame byte 34 + 2 w.  The funnelled data is
// destination-aligned, so an aligned u16 holds one TCP word when F is even
// and the high byte of one word with the low byte of the next when F is odd;
// in the odd case the two bytes of every u16 are swapped before summing
// (v_perm), which again adds every even-offset byte once and every odd-offset
// byte times 256: the exact word sum W (mod 2^32), whatever the source's
// alignment.  The fold happens once, on (seed + W) mod 2^32, as in
// src/utils.c:46-54.
//
// The 54 header bytes are built in registers by every lane of the row from
// the template (14 dwords), patched as tcp_transmit_skb and ip_output patch
// them (tcp_hdr_dev.h); the chunks that hold header bytes (the first 4 or 5) are kept back
// until the row's sum is known and then leave with header and payload bytes
// merged, one store per chunk.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "seg_frame_dev.h"

namespace lvlip {

// the row's work itself is tso_frame (seg_frame_dev.h), which k_push
// (push_kernels.hip) runs too; this kernel maps segments to sends
__global__ __launch_bounds__(256) void k_tso(const uint8_t* payload, const lvlip_tso_send* s, uint32_t n,
                                             uint32_t nseg, uint8_t* out, lvlip_frame_desc* fd) {
    const uint32_t tl = threadIdx.x & (TSO_ROW - 1u);
    const uint64_t g64 = (uint64_t)blockIdx.x * TSO_SEGS + (threadIdx.x / TSO_ROW);
    bool live = g64 < nseg;
    const uint32_t g = live ? (uint32_t)g64 : 0u;

    // the send of segment g: the last one whose seg0 is <= g (seg0 rises
    // strictly: every send has a segment, and s[0].seg0 == 0)
    const lvlip_tso_send* t = s + slot_owner<&lvlip_tso_send::seg0>(s, n, g);
    const uint32_t mss = t->mss, len = t->len;
    const uint32_t i = g - t->seg0;
    const uint64_t done = (uint64_t)i * mss;
    live = live && g >= t->seg0 && done < len;  // a caller's nseg beyond the plan's: nothing to do
    const uint32_t dlen = live ? (len - done < mss ? (uint32_t)(len - done) : mss) : 0u;
    const bool last = done + dlen == len;

    uint32_t h[14];
    {
        const uint32_t* hw = reinterpret_cast<const uint32_t*>(t->hdr);  // offset 32 of an 8-B aligned struct
#pragma unroll
        for (int k = 0; k < 14; ++k) h[k] = hw[k];
    }

    const uint64_t off = t->out_off + (uint64_t)i * t->stride;
    const uint64_t F = reinterpret_cast<uint64_t>(out) + off;      // the frame's first byte
    const uint64_t S = reinterpret_cast<uint64_t>(payload) + t->payload_off + done;
    const uint32_t seq0 = __builtin_bswap32((h[9] >> 16) | (h[10] << 16));
    tso_frame(tl, live, h, F, S, dlen, last, [=](uint32_t(&)[14]) { return seq0 + (uint32_t)done; });
    if (fd && live && tl == 0u)
        store_global(reinterpret_cast<uint64_t>(fd + g), u32x4{(uint32_t)off, (uint32_t)(off >> 32), (uint32_t)TSO_HDR + dlen, 0u});
}

}  // namespace lvlip

extern "C" {

int lvlip_tso_dev(const void* payload, const lvlip_tso_send* s, uint32_t n, uint32_t nseg, void* out,
                  lvlip_frame_desc* fd, void* stream) {
    if (n == 0) return LVLIP_OK;
    if (!payload || !s || !out || nseg == 0 || nseg > LVLIP_MAX_BATCH) return LVLIP_EINVAL;
    const uint32_t grid = (uint32_t)(((uint64_t)nseg + lvlip::TSO_SEGS - 1u) / lvlip::TSO_SEGS);
    hipLaunchKernelGGL(lvlip::k_tso, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)payload, s,
                       n, nseg, (uint8_t*)out, fd);
    return lvlip_launch_status(hipGetLastError(), "k_tso");
}

}  // extern "C"
