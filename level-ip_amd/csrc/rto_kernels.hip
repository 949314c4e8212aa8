// rto_kernels.hip — the retransmission timer and the peer's window on the
// device (include/lvlip_skb.h, "f2 on the device: the timer and the peer's
// window").  rto_cpu.c is the same on the calling thread, bit for bit.
//
// lvlip_wnd_dev: res is zeroed on the stream, then two kernels.
//
//   k_wnd_rec   one lane per record, the shape of k_snd_rec (snd_kernels.hip):
//               the rec_ack_flow gather, the class against the flow's snd_una
//               and snd_nxt, then the frame test of lvlip_sack_* on the ACK
//               frame (descriptor, the dword at byte 14 for version and ihl,
//               the dword at 14 + ihl*4 + 12 for hl; both inside the frame
//               once fd.len has been compared).  A counting lane's key is
//               (d + 1) << 32 | i.  The wave reduces BEFORE any atomic
//               (wave_peel, wave_ops.h): for the flow of its first pending
//               lane a butterfly max of the keys and a ballot count, then lane
//               0 issues one 64-bit atomic max into the first 8 bytes of
//               res[flow] and lane 1 one atomic add into its third dword;
//               SND_PEEL flows a wave, after which pending lanes (a wave of
//               many flows, whose addresses do not collide) issue their own
//               two.  Max and add only: the bytes do not depend on the run.
//   k_wnd_fin   one lane per flow: splits the key into winner and d, loads
//               the winner's descriptor and the dword at 14 + ihl*4 + 12 again
//               (hl, flags, window: frame bytes the record pass already
//               proved present), and writes res[k] (one 16-B store),
//               t[k].snd_wnd and, with LVLIP_WND_APPLY, w[k].wnd.
//
// lvlip_rto_dev: ONE launch, k_rto.  A wave per flow, four per workgroup, as
// k_snd_fin.  Lane 0 does the arithmetic of steps 1-4 and stores t[k] (32 B),
// res[k] (16 B) and gate[k] (32 B); the verdict goes to the wave with a
// shuffle, and a flow that timed out has its scoreboard range cleared 64 bytes
// a step, a byte per lane, inside [seg0, seg0 + nseg) only.
//
// The arithmetic per flow (the ACK class, the window's scale and ceiling, the
// timer's steps 1-4) is flow_step.h's, which rto_cpu.c calls too.
//
// No LDS, no workspace, plain C++ stores; no atomics in k_wnd_fin and k_rto.
//
// Bounds.  Flow indices come from rec_ack_flow (below nflows); a frame is read
// only inside the aligned dwords that hold bytes it was proved to have (at
// most three bytes to either side of a field, all within the 20 TCP header
// bytes); the winner index is one a lane of k_wnd_rec wrote, so below n; the
// scoreboard index is seg0 + i with i < nseg, which lvlip_snd_plan keeps below
// 2^32 and inside the caller's *nfd entries.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "csum_dev.h"
#include "flow_step.h"
#include "tcp_hdr_dev.h"
#include "wave_ops.h"

namespace lvlip {

constexpr int RTO_PEEL = 4;                      // SND_PEEL: flows a wave reduces before lanes go alone
constexpr uint32_t RTO_WAVES = 4;                // flows per workgroup of k_rto

// The frame test of lvlip_sack_* on the frame at F of len bytes.  *tw gets the
// dword at 14 + ihl*4 + 12: hl in bits 4-7, the window in the upper half.
__device__ __forceinline__ bool wnd_frame(uint64_t F, uint32_t len, uint32_t* tw) {
    if (len < 34u) return false;
    const uint32_t a = load_u32_any(F + 14u);  // version | ihl, tos, ip.len
    const uint32_t ihl = a & 0xfu;
    if (((a >> 4) & 0xfu) != 4u || ihl < 5u) return false;
    const uint32_t th = 14u + 4u * ihl;
    if (len < th + 20u) return false;
    const uint32_t w = load_u32_any(F + th + 12u);  // hl << 4, flags, window
    const uint32_t hl = (w >> 4) & 0xfu;
    if (hl < 5u || len < th + 4u * hl) return false;
    *tw = w;
    return true;
}

// ------------------------------------------------------------- the window --

__global__ __launch_bounds__(256) void k_wnd_rec(const lvlip_lro_flow* f, const lvlip_snd_flow* s, uint32_t nflows,
                                                 const lvlip_lro_rec* rec, const uint8_t* ack_base,
                                                 const lvlip_frame_desc* ack_fd, uint32_t n, lvlip_wnd_result* res) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t flow = FLOW_NONE;
    uint64_t key = 0;  // 0: the record does not count
    if (i < n) {
        const uint4 r = load_global(reinterpret_cast<uint64_t>(rec + i));  // flow, rel, dlen | status | flags, ack_seq
        flow = rec_ack_flow(r, f, nflows);
        if (flow != FLOW_NONE) {
            const uint32_t una = s[flow].snd_una, span = s[flow].snd_nxt - una;
            const uint32_t d = r.w - una;
            if (flow_ack_class(d, span) <= FLOW_ACK_DUP) {  // new or duplicate
                const uint4 fd = load_global(reinterpret_cast<uint64_t>(ack_fd + i));  // offset lo, hi, len, -
                const uint64_t F = reinterpret_cast<uint64_t>(ack_base) + (((uint64_t)fd.y << 32) | fd.x);
                uint32_t tw;
                if (wnd_frame(F, fd.z, &tw)) key = ((uint64_t)(d + 1u) << 32) | (uint32_t)i;
            }
        }
    }
    const bool pending = wave_peel<RTO_PEEL>(key != 0ull, flow, [=](uint32_t fl, bool mine) {
        const uint32_t cnt = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(mine));
        const uint64_t mx = wave_max_u64(mine ? key : 0ull);
        if (lane == 0u) atomicMax(reinterpret_cast<unsigned long long*>(res + fl), (unsigned long long)mx);
        if (lane == 1u) atomicAdd(reinterpret_cast<uint32_t*>(res + fl) + 2, cnt);
    });
    if (pending) {
        atomicMax(reinterpret_cast<unsigned long long*>(res + flow), (unsigned long long)key);
        atomicAdd(reinterpret_cast<uint32_t*>(res + flow) + 2, 1u);
    }
}

__global__ __launch_bounds__(256) void k_wnd_fin(lvlip_rto_flow* t, lvlip_push_flow* w, uint32_t nflows,
                                                 const uint8_t* ack_base, const lvlip_frame_desc* ack_fd,
                                                 uint32_t flags, lvlip_wnd_result* res) {
    const uint64_t k64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k64 >= nflows) return;
    const uint32_t k = (uint32_t)k64;
    const uint4 a = load_global(reinterpret_cast<uint64_t>(res + k));  // winner, d + 1, count, 0
    uint32_t winner = FLOW_NONE, raw = 0u, wnd = t[k].snd_wnd;
    if (a.y) {
        const uint4 fd = load_global(reinterpret_cast<uint64_t>(ack_fd + a.x));
        const uint64_t F = reinterpret_cast<uint64_t>(ack_base) + (((uint64_t)fd.y << 32) | fd.x);
        uint32_t tw;
        if (wnd_frame(F, fd.z, &tw)) {  // it passed in k_wnd_rec: the same bytes
            winner = a.x;
            raw = bswap16u(tw >> 16);
            wnd = flow_wnd_scale(raw, t[k].wscale);
            t[k].snd_wnd = wnd;
        }
    }
    store_global(reinterpret_cast<uint64_t>(res + k), u32x4{a.z, winner, raw, wnd});
    if ((flags & LVLIP_WND_APPLY) && w) w[k].wnd = flow_wnd_apply(wnd, t[k].wnd_cap);
}

// --------------------------------------------------------------- the timer --

__global__ __launch_bounds__(256) void k_rto(const lvlip_snd_flow* s, const lvlip_snd_result* snd,
                                             const lvlip_push_result* push, lvlip_rto_flow* t, uint32_t nflows,
                                             uint32_t now, uint32_t flags, uint8_t* sacked, lvlip_snd_result* gate,
                                             lvlip_rto_result* res) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k64 = (uint64_t)blockIdx.x * RTO_WAVES + (threadIdx.x >> 6);
    if (k64 >= nflows) return;  // the whole wave
    const uint32_t k = (uint32_t)k64;
    const uint32_t seg0 = s[k].seg0, nseg = s[k].nseg;
    uint32_t fired = 0u;
    if (lane == 0u) {
        lvlip_rto_flow x = t[k];
        const bool live = !x.dead;  // a dead flow's state is not stored
        const flow_rto_out o = flow_rto_step(&x, nseg, push ? push[k].pushed : 0u, snd ? snd[k].n_new : 0u,
                                             snd ? snd[k].n_dup : 0u, now, flags);
        fired = o.fired;
        if (live) t[k] = x;
        store_global(reinterpret_cast<uint64_t>(res + k), u32x4{fired, o.sample, x.rto, (uint32_t)x.backoff});
        const uint64_t g = reinterpret_cast<uint64_t>(gate + k);
        store_global(g, u32x4{0u, 0u, 0u, 0u});                            // snd_una acked n_new n_dup
        store_global(g + 16u, u32x4{0u, 0u, fired ? 0u : nseg, 0u});       // n_old n_beyond popped inflight
    }
    fired = (uint32_t)__shfl((int)fired, 0, 64);
    if (fired == LVLIP_RTO_TIMEOUT && sacked) {
        for (uint64_t c0 = 0; c0 < nseg; c0 += 64u) {
            const uint64_t i = c0 + lane;
            if (i < nseg) sacked[(uint64_t)seg0 + i] = 0;
        }
    }
}

}  // namespace lvlip

extern "C" {

int lvlip_wnd_dev(const lvlip_lro_flow* f, const lvlip_snd_flow* s, lvlip_rto_flow* t, lvlip_push_flow* w,
                  uint32_t nflows, const lvlip_lro_rec* rec, const void* ack_base, const lvlip_frame_desc* ack_fd,
                  uint32_t n, uint32_t flags, lvlip_wnd_result* res, void* stream) {
    if (nflows == 0) return LVLIP_OK;
    if (!f || !s || !t || !res || (n && (!rec || !ack_base || !ack_fd))) return LVLIP_EINVAL;
    if (n > LVLIP_MAX_BATCH || nflows > LVLIP_LRO_MAX_FLOWS || (flags & ~LVLIP_WND_APPLY)) return LVLIP_EINVAL;
    if (any_misaligned<8>(f, s, t, w) || any_misaligned<16>(rec, ack_fd, res)) return LVLIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int rc = lvlip_launch_status(hipMemsetAsync(res, 0, (size_t)nflows * sizeof *res, st), "lvlip_wnd_dev: memset");
    if (rc != LVLIP_OK) return rc;
    if (n) {
        const uint32_t grid = (uint32_t)(((uint64_t)n + 255u) / 256u);
        hipLaunchKernelGGL(lvlip::k_wnd_rec, dim3(grid), dim3(256), 0, st, f, s, nflows, rec, (const uint8_t*)ack_base,
                           ack_fd, n, res);
        rc = lvlip_launched("k_wnd_rec");
        if (rc != LVLIP_OK) return rc;
    }
    const uint32_t fgrid = (nflows + 255u) / 256u;
    hipLaunchKernelGGL(lvlip::k_wnd_fin, dim3(fgrid), dim3(256), 0, st, t, w, nflows, (const uint8_t*)ack_base, ack_fd,
                       flags, res);
    return lvlip_launched("k_wnd_fin");
}

int lvlip_rto_dev(const lvlip_snd_flow* s, const lvlip_snd_result* snd, const lvlip_push_result* push,
                  lvlip_rto_flow* t, uint32_t nflows, uint32_t now, uint32_t flags, uint8_t* sacked,
                  lvlip_snd_result* gate, lvlip_rto_result* res, void* stream) {
    if (nflows == 0) return LVLIP_OK;
    if (!s || !t || !gate || !res) return LVLIP_EINVAL;
    if (nflows > LVLIP_LRO_MAX_FLOWS || (flags & ~LVLIP_RTO_FAST)) return LVLIP_EINVAL;
    if (any_misaligned<8>(s, t) || any_misaligned<16>(snd, push, gate, res)) return LVLIP_EINVAL;
    const uint32_t grid = (nflows + lvlip::RTO_WAVES - 1u) / lvlip::RTO_WAVES;
    hipLaunchKernelGGL(lvlip::k_rto, dim3(grid), dim3(256), 0, (hipStream_t)stream, s, snd, push, t, nflows, now, flags,
                       sacked, gate, res);
    return lvlip_launched("k_rto");
}

}  // extern "C"
