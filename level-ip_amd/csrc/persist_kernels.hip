// persist_kernels.hip — the zero-window persist timer and its probe on the
// device (include/lvlip_skb.h, "f2 on the device: the persist timer"): per
// planned flow its send side, write side, timer and persist state -> the
// persist state a round later and, for a flow whose timer ran out, one
// finished 54-byte probe, every byte what persist_cpu.c writes.  One launch,
// nothing but loads and stores: no workspace, no atomics, no LDS.
//
// Work mapping.  k_ack's (ack_kernels.hip): eight lanes per flow, eight flows
// per wave, 32 per 256-thread workgroup.  A probe is 54 bytes at out + 64 k
// for any `out`, so it touches at most (15 + 54 + 15) / 16 = 5 aligned 16-B
// chunks: lane c of the group owns destination chunk c, the 16 aligned bytes
// at (F & ~15) + 16 c, and lanes 5 .. 7 store nothing.  The work is
// latency-bound (a dozen independent loads, some sixty VALU instructions, one
// store per lane), so nothing is shared between the lanes of a group: every
// lane loads the flow's words (the same addresses in all eight lanes: one
// request), runs the timer's step (flow_step.h, which persist_cpu.c calls
// too), builds the whole frame in registers and keeps its own chunk.  The
// group's first lane stores p[k] (16 B), res[k] and fd_out[k] (one 16-B store
// each) and, only when step 2 asks for it, the four bytes of t[k].dupacks.
//
// The frame in registers.  Dwords h[0..13] are the template's 54 bytes
// (w[k].hdr lies at offset 52 of an 8-B aligned struct: 14 aligned dwords, the
// top half of the last being the struct's pad), patched as k_push and k_rtx
// patch them (tcp_hdr_dev.h) and summed from the registers.  Which 16 bytes a
// lane keeps is selected with compare masks over registers with constant
// indices (hdr_chunk), never with a runtime index into an array, which hipcc
// would put in scratch.  Chunks the frame covers whole leave as one 16-B
// store; the first and the last leave as the dwords and bytes inside
// [F, F + 54) and nothing else (store_chunk, row_copy.h), so bytes 54 .. 63 of
// a slot and the neighbour's slot are never written.
//
// Bounds.  Every load index is below nflows (a group past the end reads flow 0
// and stores nothing); a lane stores only while its chunk index is below
// ceil(((F & 15) + 54) / 16) <= 5, and then only bytes of the frame; the state
// stores go to index k < nflows of the caller's arrays.  All loads of a flow
// are issued before its stores (the stores take their data), and no flow reads
// what another writes.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "csum_dev.h"
#include "flow_step.h"
#include "row_copy.h"
#include "tcp_hdr_dev.h"

namespace lvlip {

constexpr uint32_t PERSIST_GROUP = 8;                     // lanes per flow
constexpr uint32_t PERSIST_FLOWS = 256 / PERSIST_GROUP;   // flows per workgroup
constexpr int PERSIST_BLOCKS = 4;                         // 16-B blocks of the frame's 14 dwords

__global__ __launch_bounds__(256) void k_persist(const lvlip_lro_flow* f, const lvlip_lro_result* lro,
                                                 const lvlip_snd_flow* s, const lvlip_push_flow* w,
                                                 lvlip_rto_flow* t, lvlip_persist_flow* p, uint32_t nflows,
                                                 uint32_t now, uint8_t* out, lvlip_frame_desc* fd_out,
                                                 lvlip_persist_result* res) {
    const uint32_t c = threadIdx.x & (PERSIST_GROUP - 1u);  // this lane's destination chunk
    const uint64_t g64 = (uint64_t)blockIdx.x * PERSIST_FLOWS + (threadIdx.x / PERSIST_GROUP);
    const bool live = g64 < nflows;
    const uint32_t g = live ? (uint32_t)g64 : 0u;

    // ---- the flow's inputs
    const lvlip_push_flow* wk = w + g;
    const uint32_t* hw = reinterpret_cast<const uint32_t*>(wk->hdr);  // offset 52 of an 8-B aligned struct
    uint32_t h[14];
#pragma unroll
    for (int j = 0; j < 14; ++j) h[j] = hw[j];
    const uint32_t unsent = wk->unsent, wnd = wk->wnd, mss = wk->mss;
    const uint32_t una = s[g].snd_una, nseg = s[g].nseg, win = s[g].win;
    const uint32_t rto = t[g].rto, dead = t[g].dead;
    const uint32_t ack = f[g].rcv_nxt + (lro ? lro[g].delivered : 0u);
    lvlip_persist_flow x = p[g];

    // ---- the timer (steps 0-4), the same in every lane of the group
    const flow_persist_out o = flow_persist_step(&x, dead, nseg, unsent, wnd, mss, rto, now);
    const bool fired = live && o.fired != 0u;
    const uint32_t seq = una - 1u;

    // ---- the 54 header bytes
    h[4] = (h[4] & 0xffff0000u) | bswap16u(40u);                  // ip.len, src/ip_output.c:35,46
    h[6] &= 0xffff0000u;                                          // ip.csum = 0, src/ip_output.c:42
    const uint32_t ipw = (h[3] >> 16) + halves(h[4]) + halves(h[5]) + halves(h[6]) + halves(h[7]) +
                         (h[8] & 0xffffu);
    h[6] |= (uint32_t)finish(0u, ipw);                            // ip_send_check, src/ip_output.c:8-12
    const uint32_t sq = __builtin_bswap32(seq);                   // frame bytes 38 .. 41, src/tcp_output.c:106
    h[9] = (h[9] & 0xffffu) | (sq << 16);
    h[10] = (h[10] & 0xffff0000u) | (sq >> 16);
    hdr_put_ack(h, __builtin_bswap32(ack));
    h[11] &= ~(0x09u << 24);                                      // not the last segment: no FIN, no PSH (:466)
    h[12] = bswap16u(win);                                        // window; tcp.csum = 0, src/tcp_output.c:110
    h[13] &= 0xffffu;                                             // urp; the struct's pad is no frame byte
    h[12] |= (uint32_t)finish(hdr_tcp_seed(h, 20u), hdr_tcp_words(h)) << 16;  // src/tcp_output.c:126

    const uint4 blk[PERSIST_BLOCKS] = {make_uint4(h[0], h[1], h[2], h[3]), make_uint4(h[4], h[5], h[6], h[7]),
                                       make_uint4(h[8], h[9], h[10], h[11]), make_uint4(h[12], h[13], 0u, 0u)};

    // ---- lane c keeps destination chunk c
    const uint64_t off = (uint64_t)LVLIP_PERSIST_SLOT * g;
    const uint64_t F = reinterpret_cast<uint64_t>(out) + off;  // the frame's first byte
    const int fo = (int)(F & 15ull);
    const uint64_t D = F - (uint64_t)fo;
    const uint32_t nch = fired ? (uint32_t)(fo + TCP_FRAME_HDR + 15) >> 4 : 0u;  // chunks the frame touches: 4 or 5
    if (c < nch)
        store_chunk(D + 16ull * c, hdr_chunk(c, fo, blk), c == 0u ? fo : 0, min(16, fo + TCP_FRAME_HDR - (int)(16u * c)));

    // ---- the state, by the group's first lane
    if (live && c == 0u) {
        if (!dead) p[g] = x;  // a dead flow's state is not stored
        if (o.clear) t[g].dupacks = 0u;
        store_global(reinterpret_cast<uint64_t>(res + g), u32x4{o.fired, o.interval, o.probes, o.fired ? seq : 0u});
        store_global(reinterpret_cast<uint64_t>(fd_out + g),
                     u32x4{(uint32_t)off, 0u, o.fired ? (uint32_t)TCP_FRAME_HDR : 0u, 0u});
    }
}

}  // namespace lvlip

extern "C" {

int lvlip_persist_dev(const lvlip_lro_flow* f, const lvlip_lro_result* lro, const lvlip_snd_flow* s,
                      const lvlip_push_flow* w, lvlip_rto_flow* t, lvlip_persist_flow* p, uint32_t nflows,
                      uint32_t now, void* out, lvlip_frame_desc* fd_out, lvlip_persist_result* res, void* stream) {
    if (nflows == 0) return LVLIP_OK;
    if (!f || !s || !w || !t || !p || !out || !fd_out || !res) return LVLIP_EINVAL;
    if (nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    if (any_misaligned<8>(f, s, w, t, p) || any_misaligned<16>(lro, fd_out, res)) return LVLIP_EINVAL;
    const uint32_t grid = (nflows + lvlip::PERSIST_FLOWS - 1u) / lvlip::PERSIST_FLOWS;
    hipLaunchKernelGGL(lvlip::k_persist, dim3(grid), dim3(256), 0, (hipStream_t)stream, f, lro, s, w, t, p, nflows, now,
                       (uint8_t*)out, fd_out, res);
    return lvlip_launched("k_persist");
}

}  // extern "C"
