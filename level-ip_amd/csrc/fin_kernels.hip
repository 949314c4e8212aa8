// fin_kernels.hip — the end of a connection on the device (include/lvlip_skb.h,
// "the end of a connection: FIN and TIME-WAIT"): per connection its receive
// side, send side, write side, timer and close state and the round's records ->
// the close state a round later, rcv_nxt past the peer's FIN, snd_nxt past our
// own, the gate for lvlip_ack_* and, for a flow that sends or re-sends its FIN,
// one finished 54-byte frame, every byte what fin_cpu.c writes.  A memset of
// the workspace and two launches, nothing but loads and stores: no atomics, no
// LDS.
//
// k_fin_scan.  One lane per record.  A lane whose record is a FIN of a planned
// flow (status PLACED or NO_DATA, tcp_flags & 1) gathers f[flow].rcv_nxt,
// gin[flow].delivered and x[flow].base and stores the constant 1 into ws[2 flow]
// (hit) or ws[2 flow + 1] (again).  Lanes that store to one byte store the same
// value, so the result does not depend on their order; ws was zeroed on the
// stream before.  The kernel reads f and x, which k_fin writes: the two are
// separate launches on one stream.
//
// k_fin.  k_persist's mapping (persist_kernels.hip): eight lanes per flow,
// eight flows per wave, 32 per 256-thread workgroup.  A frame is 54 bytes at
// out + 64 k for any `out`, so it touches at most (15 + 54 + 15) / 16 = 5
// aligned 16-B chunks: lane c of the group owns destination chunk c, and lanes
// 5 .. 7 store no frame byte.  Every lane loads the flow's words (the same
// addresses in all eight lanes: one request each), runs flow_fin_step
// (flow_step.h, which fin_cpu.c calls too), builds the whole frame in
// registers (tcp_hdr_dev.h, as k_persist) and keeps its own chunk; chunks are
// picked with compare masks over registers with constant indices (hdr_chunk),
// never with a runtime index.  The group's first lane stores x[k] (its first
// 24 bytes as three 8-B stores; the reserved bytes behind them never change),
// res[k] and fd_out[k] (one 16-B store each), gate[k] (three 16-B stores) and,
// only when the step changed them, the four bytes of f[k].rcv_nxt and of
// s[k].snd_nxt.
//
// Bounds.  k_fin_scan: a lane loads rec[i] only for i < n; it gathers and
// stores only for rec.flow < nflows, at ws[2 flow] and ws[2 flow + 1], both
// below 2 nflows <= lvlip_fin_workspace_bytes(nflows).  k_fin: every load index
// is below nflows (a group past the end reads flow 0 and stores nothing; nflows
// > 0 at every launch); ws is read at bytes 2 k and 2 k + 1; a lane stores
// frame bytes only while its chunk index is below ceil(((F & 15) + 54) / 16) <=
// 5, and then only bytes inside [F, F + 54) with F = out + 64 k (store_chunk
// writes a first or last chunk as the dwords and bytes inside the range), so
// bytes 54 .. 63 of a slot and the neighbour's slot are never written; the
// state stores go to index k < nflows of the caller's arrays, each inside
// element k (x 24 of 32 B, res and fd_out 16 B, gate 48 B, the two scalar fields
// 4 B).  All loads of a flow are issued before its stores (the stores take
// their data), gate is not gin, and no flow reads what another writes.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "csum_dev.h"
#include "flow_step.h"
#include "row_copy.h"
#include "tcp_hdr_dev.h"

namespace lvlip {

constexpr uint32_t FIN_GROUP = 8;                 // lanes per flow
constexpr uint32_t FIN_FLOWS = 256 / FIN_GROUP;   // flows per workgroup
constexpr int FIN_BLOCKS = 4;                     // 16-B blocks of the frame's 14 dwords

__global__ __launch_bounds__(256) void k_fin_scan(const lvlip_lro_flow* f, const lvlip_lro_result* gin,
                                                  const lvlip_lro_rec* rec, uint32_t n, const lvlip_fin_flow* x,
                                                  uint32_t nflows, uint8_t* ws) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4 r = load_global(reinterpret_cast<uint64_t>(rec + i));  // flow, rel, dlen | status << 16 | flags << 24
    const uint32_t flow = r.x, status = (r.z >> 16) & 0xffu;
    if (flow >= nflows || !(r.z & (1u << 24))) return;
    if (status != LVLIP_LRO_PLACED && status != LVLIP_LRO_NO_DATA) return;
    const uint32_t key = r.y + (r.z & 0xffffu);
    const uint32_t target = f[flow].rcv_nxt + gin[flow].delivered - x[flow].base;
    if (key == target) ws[2ull * flow] = 1;
    if (key == target - 1u) ws[2ull * flow + 1ull] = 1;
}

__global__ __launch_bounds__(256) void k_fin(lvlip_lro_flow* f, const lvlip_lro_result* gin, lvlip_snd_flow* s,
                                             const lvlip_push_flow* w, const lvlip_rto_flow* t, lvlip_fin_flow* xs,
                                             uint32_t nflows, const uint8_t* close, uint32_t now, uint8_t* out,
                                             lvlip_frame_desc* fd_out, lvlip_lro_result* gate, lvlip_fin_result* res,
                                             const uint8_t* ws) {
    const uint32_t c = threadIdx.x & (FIN_GROUP - 1u);  // this lane's destination chunk
    const uint64_t g64 = (uint64_t)blockIdx.x * FIN_FLOWS + (threadIdx.x / FIN_GROUP);
    const bool live = g64 < nflows;
    const uint32_t g = live ? (uint32_t)g64 : 0u;

    // ---- the flow's inputs
    const lvlip_push_flow* wk = w + g;
    const uint32_t* hw = reinterpret_cast<const uint32_t*>(wk->hdr);  // offset 52 of an 8-B aligned struct
    uint32_t h[14];
#pragma unroll
    for (int j = 0; j < 14; ++j) h[j] = hw[j];
    const uint32_t unsent = wk->unsent;
    const uint32_t una = s[g].snd_una, nxt = s[g].snd_nxt, nseg = s[g].nseg, win = s[g].win;
    const uint32_t rto = t[g].rto, dead = t[g].dead;
    const uint32_t rcv_nxt = f[g].rcv_nxt;
    const uint64_t ga = reinterpret_cast<uint64_t>(gin + g);
    const uint4 g0 = load_global(ga), g1 = load_global(ga + 16u), g2 = load_global(ga + 32u);  // g0: delivered, placed
    const uint32_t hit = ws[2ull * g], again = ws[2ull * g + 1ull];
    const uint32_t cl = close ? close[g] : 0u;
    // x[k]'s words 0 .. 5 (8-B aligned: three 8-B loads); the reserved bytes behind them are not the step's
    uint2* xw = reinterpret_cast<uint2*>(xs + g);
    const uint2 x0 = xw[0], x1 = xw[1], x2 = xw[2];
    lvlip_fin_flow x = {};
    x.base = x0.x, x.fin_seq = x0.y, x.expires = x1.x, x.interval = x1.y, x.retries = x2.x;
    x.state = (uint8_t)x2.y, x.flags = (uint8_t)(x2.y >> 8);

    // ---- the states (steps 0, 2-5), the same in every lane of the group
    const flow_fin_out o = flow_fin_step(&x, dead, rcv_nxt, una, nxt, nseg, unsent, rto, hit, again, cl, now);
    const bool fired = live && o.frame != 0u;
    const uint32_t seq = x.fin_seq;
    const uint32_t ack = o.rcv_nxt + g0.x;

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
    h[11] = (h[11] & ~(0x08u << 24)) | (0x11u << 24);             // tcp_queue_fin: FIN, ACK, no PSH (:515-516)
    h[12] = bswap16u(win);                                        // window; tcp.csum = 0, src/tcp_output.c:110
    h[13] &= 0xffffu;                                             // urp; the struct's pad is no frame byte
    h[12] |= (uint32_t)finish(hdr_tcp_seed(h, 20u), hdr_tcp_words(h)) << 16;  // src/tcp_output.c:126

    const uint4 blk[FIN_BLOCKS] = {make_uint4(h[0], h[1], h[2], h[3]), make_uint4(h[4], h[5], h[6], h[7]),
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
        xw[0] = make_uint2(x.base, x.fin_seq);
        xw[1] = make_uint2(x.expires, x.interval);
        xw[2] = make_uint2(x.retries, (x2.y & 0xffff0000u) | x.state | ((uint32_t)x.flags << 8));
        if (o.rcv_nxt != rcv_nxt) f[g].rcv_nxt = o.rcv_nxt;
        if (o.snd_nxt != nxt) s[g].snd_nxt = o.snd_nxt;
        const uint32_t placed = (o.events & LVLIP_FIN_EV_ACK_OWED) && g0.y == 0u ? 1u : g0.y;
        const uint64_t go = reinterpret_cast<uint64_t>(gate + g);
        store_global(go, u32x4{g0.x, placed, g0.z, g0.w});
        store_global(go + 16u, u32x4{g1.x, g1.y, g1.z, g1.w});
        store_global(go + 32u, u32x4{g2.x, g2.y, g2.z, g2.w});
        store_global(reinterpret_cast<uint64_t>(res + g), u32x4{o.events, (uint32_t)x.state, o.frame ? seq : 0u, o.interval});
        store_global(reinterpret_cast<uint64_t>(fd_out + g),
                     u32x4{(uint32_t)off, 0u, o.frame ? (uint32_t)TCP_FRAME_HDR : 0u, 0u});
    }
}

}  // namespace lvlip

extern "C" {

int lvlip_fin_dev(lvlip_lro_flow* f, const lvlip_lro_result* gin, const lvlip_lro_rec* rec, uint32_t n,
                  lvlip_snd_flow* s, const lvlip_push_flow* w, const lvlip_rto_flow* t, lvlip_fin_flow* x,
                  uint32_t nflows, const uint8_t* close, uint32_t now, void* out, lvlip_frame_desc* fd_out,
                  lvlip_lro_result* gate, lvlip_fin_result* res, void* ws, void* stream) {
    if (nflows == 0) return LVLIP_OK;
    if (!f || !gin || !s || !w || !t || !x || !out || !fd_out || !gate || !res || !ws || (!rec && n)) return LVLIP_EINVAL;
    if (gate == gin || nflows > LVLIP_LRO_MAX_FLOWS || n > LVLIP_MAX_BATCH) return LVLIP_EINVAL;
    if (any_misaligned<8>(f, s, w, t, x) || any_misaligned<16>(gin, rec, fd_out, gate, res) || ((uintptr_t)ws & 15u))
        return LVLIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int rc = lvlip_launch_status(hipMemsetAsync(ws, 0, lvlip_fin_workspace_bytes(nflows), st), "lvlip_fin_dev: memset");
    if (rc != LVLIP_OK) return rc;
    if (n) {
        const uint32_t grid = (uint32_t)(((uint64_t)n + 255u) / 256u);
        hipLaunchKernelGGL(lvlip::k_fin_scan, dim3(grid), dim3(256), 0, st, f, gin, rec, n, x, nflows, (uint8_t*)ws);
        rc = lvlip_launched("k_fin_scan");
        if (rc != LVLIP_OK) return rc;
    }
    const uint32_t grid = (nflows + lvlip::FIN_FLOWS - 1u) / lvlip::FIN_FLOWS;
    hipLaunchKernelGGL(lvlip::k_fin, dim3(grid), dim3(256), 0, st, f, gin, s, w, t, x, nflows, close, now, (uint8_t*)out,
                       fd_out, gate, res, (const uint8_t*)ws);
    return lvlip_launched("k_fin");
}

}  // extern "C"
