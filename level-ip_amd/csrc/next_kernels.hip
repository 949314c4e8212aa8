// next_kernels.hip — moving a connection's state on to the next batch on the
// device (include/lvlip_skb.h, "state across batches"): what rcv_cpu.c's
// lvlip_lro_next_cpu and snd_cpu.c's lvlip_snd_next_cpu do, on the caller's
// stream, so that a loop of many rounds needs no host step between them.
//
//   k_lro_next   one lane per flow: d = min(res.delivered, f.rcv_wnd) goes onto
//                rcv_nxt and out_off and off rcv_wnd; res.delivered = 0
//   k_snd_next   one lane per flow: p = min(res.popped, s.nseg) goes onto seg0
//                and off nseg, snd_una = res.snd_una; res.popped = res.acked = 0,
//                res.inflight = nseg
//
// Each is one launch of loads and stores: no workspace, no atomics, no LDS.  A
// lane loads the result's words as 16-B vectors (res is 16-B aligned) and the
// flow's as 8-B vectors (f and s are 8-B aligned), and stores the ones that
// change the same way.
//
// Bounds.  Every index is below nflows (a live test from blockIdx); the values
// read are clamped and never become an address.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lvlip_skb.h"
#include "tcp_hdr_dev.h"  // lvlip_launched, any_misaligned

namespace lvlip {

__global__ __launch_bounds__(256) void k_lro_next(lvlip_lro_flow* f, lvlip_lro_result* res, uint32_t nflows) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;  // nflows <= 65536
    if (k >= nflows) return;
    uint2* fw = reinterpret_cast<uint2*>(f + k);      // [1] ports, rcv_nxt; [2] rcv_wnd, reserved; [3] out_off
    uint4* rw = reinterpret_cast<uint4*>(res + k);    // [0] delivered, placed, nsack, reserved
    uint2 a = fw[1], b = fw[2], o = fw[3];
    uint4 r = rw[0];
    const uint32_t d = r.x < b.x ? r.x : b.x;
    a.y += d;
    b.x -= d;
    const uint64_t off = (((uint64_t)o.y << 32) | o.x) + d;
    o.x = (uint32_t)off, o.y = (uint32_t)(off >> 32);
    r.x = 0u;
    fw[1] = a, fw[2] = b, fw[3] = o;
    rw[0] = r;
}

__global__ __launch_bounds__(256) void k_snd_next(lvlip_snd_flow* s, lvlip_snd_result* res, uint32_t nflows) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= nflows) return;
    uint2* sw = reinterpret_cast<uint2*>(s + k);      // [0] snd_una, snd_nxt; [1] seg0, nseg
    uint4* rw = reinterpret_cast<uint4*>(res + k);    // [0] snd_una, acked, n_new, n_dup; [1] n_old, n_beyond, popped, inflight
    uint2 a = sw[0], q = sw[1];
    uint4 r0 = rw[0], r1 = rw[1];
    const uint32_t p = r1.z < q.y ? r1.z : q.y;
    a.x = r0.x;
    q.x += p;
    q.y -= p;
    r0.y = 0u;
    r1.z = 0u;
    r1.w = q.y;
    sw[0] = a, sw[1] = q;
    rw[0] = r0, rw[1] = r1;
}

}  // namespace lvlip

extern "C" {

int lvlip_lro_next_dev(lvlip_lro_flow* f, lvlip_lro_result* res, uint32_t nflows, void* stream) {
    if (nflows == 0) return LVLIP_OK;
    if (!f || !res || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    if (any_misaligned<8>(f) || any_misaligned<16>(res)) return LVLIP_EINVAL;
    hipLaunchKernelGGL(lvlip::k_lro_next, dim3((nflows + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, f, res,
                       nflows);
    return lvlip_launched("k_lro_next");
}

int lvlip_snd_next_dev(lvlip_snd_flow* s, lvlip_snd_result* res, uint32_t nflows, void* stream) {
    if (nflows == 0) return LVLIP_OK;
    if (!s || !res || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    if (any_misaligned<8>(s) || any_misaligned<16>(res)) return LVLIP_EINVAL;
    hipLaunchKernelGGL(lvlip::k_snd_next, dim3((nflows + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, s, res,
                       nflows);
    return lvlip_launched("k_snd_next");
}

}  // extern "C"
