// cc_kernels.hip — the congestion window on the device (include/lvlip_skb.h,
// "f2 on the device: the congestion window").  cc_cpu.c is the same on the
// calling thread, bit for bit.
//
// lvlip_cc_dev: res is zeroed on the stream, then two kernels.
//
//   k_cc_sum   step 3, the hot part: 1 byte of the scoreboard per queue entry
//              and the 16-B descriptor of a marked entry.  The queue lengths
//              are in HBM, so the grid is sized from the flow count as
//              k_sack_mark's is (sack_kernels.hip): a wave per flow and chunk
//              of 64 entries, blockIdx.y striding the queue, so a queue of a
//              million entries is the work of 1024 waves and 65 536 flows
//              still give each queue eight.  A wave takes CC_UNROLL chunks a
//              step: their bytes are requested first, then the descriptors of
//              the marked entries, so the two round trips of a chunk overlap
//              with its neighbours'.  The wave reduces its count and its
//              64-bit byte sum (wave_ops.h) and issues one 64-bit atomic add
//              into the first 8 bytes of res[k] and one 32-bit add into its
//              third dword; a wave without a marked entry issues none.  Dead
//              flows are skipped.  Not launched with a NULL sacked.
//   k_cc_fin   one lane per flow: steps 1, 2 and 4 on the sums, c[k] (32 B),
//              res[k] (one 16-B store) and t[k].wnd_cap.
//
// Integer adds are the only reductions, so the bytes do not depend on the run.
// No LDS, no workspace beyond res, plain C++ and vector stores.
//
// Bounds.  Flow indices are below nflows (a live test from blockIdx).  A queue
// index is seg0 + p + i with i < nseg - p and p <= nseg, formed in 64 bits:
// inside [seg0, seg0 + nseg), which lvlip_snd_plan keeps inside the caller's
// *nfd entries of fd and sacked.  Values read from res, snd and prev are
// clamped and never become an address.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lvlip_skb.h"
#include "tcp_hdr_dev.h"
#include "wave_ops.h"

namespace lvlip {

constexpr uint32_t CC_WAVES = 4;          // waves (flows) per workgroup of k_cc_sum
constexpr uint32_t CC_Y = 1024;           // most chunks a queue is spread over
constexpr uint32_t CC_Y_MIN = 8;          // fewest
constexpr uint32_t CC_GRID = 1u << 17;    // workgroups of k_cc_sum the chunk count aims at
constexpr int CC_UNROLL = 4;              // chunks of 64 entries a wave has in flight
constexpr uint32_t CC_HDR = 54u;          // the header of every frame lvlip_tso_* / lvlip_push_* build
constexpr uint32_t CC_MAX_WND = LVLIP_CC_MAX_WND;

// the sum of the wave's 64 values, in every lane
__device__ __forceinline__ uint64_t wave_add_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_cc_sum(const lvlip_snd_flow* s, const lvlip_snd_result* snd,
                                                const lvlip_rto_flow* t, uint32_t nflows, const lvlip_frame_desc* fd,
                                                const uint8_t* sacked, lvlip_cc_result* res) {
    typedef __attribute__((address_space(1))) const uint8_t gby;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k64 = (uint64_t)blockIdx.x * CC_WAVES + (threadIdx.x >> 6);
    if (k64 >= nflows) return;  // the whole wave
    const uint32_t k = (uint32_t)k64;
    if (t[k].dead) return;
    const uint32_t seg0 = s[k].seg0, nseg = s[k].nseg;
    const uint32_t p = snd ? min(snd[k].popped, nseg) : 0u;
    const uint64_t q0 = (uint64_t)seg0 + p, len = nseg - p;
    const uint64_t first = (uint64_t)blockIdx.y * 64u, stride = (uint64_t)gridDim.y * 64u;
    if (first >= len) return;  // the whole wave
    const uint64_t S = reinterpret_cast<uint64_t>(sacked) + q0, D = reinterpret_cast<uint64_t>(fd + q0);
    uint64_t bytes = 0;
    uint32_t count = 0;
    for (uint64_t c0 = first; c0 < len; c0 += stride * CC_UNROLL) {
        uint32_t mark[CC_UNROLL], flen[CC_UNROLL];
#pragma unroll
        for (int u = 0; u < CC_UNROLL; ++u) {  // no branch: an entry past the end reads the chunk's first byte
            const uint64_t i = c0 + u * stride + lane;
            mark[u] = *reinterpret_cast<gby*>(S + (i < len ? i : first));
            mark[u] = i < len ? mark[u] : 0u;
        }
#pragma unroll
        for (int u = 0; u < CC_UNROLL; ++u) {
            flen[u] = 0u;
            if (mark[u]) flen[u] = load_global(D + 16u * (c0 + u * stride + lane)).z;  // offset lo, hi, len, -
        }
#pragma unroll
        for (int u = 0; u < CC_UNROLL; ++u) {
            count += mark[u] ? 1u : 0u;
            bytes += flen[u] >= CC_HDR ? flen[u] - CC_HDR : 0u;
        }
    }
    count = wave_add_u32(count);
    bytes = wave_add_u64(bytes);
    if (lane == 0u && bytes) atomicAdd(reinterpret_cast<unsigned long long*>(res + k), (unsigned long long)bytes);
    if (lane == 1u && count) atomicAdd(reinterpret_cast<uint32_t*>(res + k) + 2, count);
}

__global__ __launch_bounds__(256) void k_cc_fin(const lvlip_snd_flow* s, const lvlip_snd_result* snd,
                                                const lvlip_rto_result* prev, lvlip_cc_flow* c, lvlip_rto_flow* t,
                                                uint32_t nflows, lvlip_cc_result* res) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;  // nflows <= 65536
    if (k >= nflows) return;
    lvlip_cc_flow x = c[k];
    const uint64_t R = reinterpret_cast<uint64_t>(res + k);
    if (t[k].dead) {
        store_global(R, u32x4{x.cwnd, 0u, 0u, 0u});
        return;
    }
    const uint4 r = load_global(R);  // the byte sum's halves, n_sacked, 0
    const uint32_t mss = x.mss, una = s[k].snd_una, nxt = s[k].snd_nxt;
    const uint32_t flight = nxt - una;
    uint32_t a = 0u, n_new = 0u, fired = 0u, bo = 0u;
    if (snd) {
        const uint4 v = load_global(reinterpret_cast<uint64_t>(snd + k));  // snd_una, acked, n_new, n_dup
        a = v.y, n_new = v.z;
    }
    if (prev) {
        const uint4 v = load_global(reinterpret_cast<uint64_t>(prev + k));  // fired, sample, rto, backoff
        fired = v.x, bo = v.w;
    }
    const uint32_t half = max(flight / 2u, 2u * mss);
    uint32_t event = 0u;
    // 1: loss
    if (fired == LVLIP_RTO_TIMEOUT) {
        if (bo == 1u) x.ssthresh = half;
        x.cwnd = mss, x.acc = 0u, x.in_rec = 0, x.recover = nxt;
        event |= LVLIP_CC_EV_TIMEOUT;
    } else if (fired == LVLIP_RTO_FASTRTX && !x.in_rec) {
        x.ssthresh = half, x.cwnd = half, x.acc = 0u, x.in_rec = 1, x.recover = nxt;
        event |= LVLIP_CC_EV_ENTER;
    }
    // 2: ACKs
    if (n_new && a) {
        uint64_t cwnd = x.cwnd;
        if (x.in_rec) {
            if (a >= x.recover - una) {
                x.in_rec = 0, x.acc = 0u;
                cwnd = x.ssthresh;
                event |= LVLIP_CC_EV_EXIT;
            }
        } else if (cwnd < x.ssthresh) {
            const uint64_t cap = (uint64_t)n_new * mss;
            cwnd += a < cap ? a : cap;
            event |= LVLIP_CC_EV_SLOWSTART;
        } else {
            uint64_t acc = (uint64_t)x.acc + a;
            if (acc >= cwnd) {
                acc -= cwnd;
                cwnd += mss;
                event |= LVLIP_CC_EV_AVOID;
            }
            x.acc = (uint32_t)(acc < cwnd ? acc : cwnd);
        }
        x.cwnd = (uint32_t)(cwnd < x.cwnd_max ? cwnd : x.cwnd_max);
    }
    // 4: output
    uint64_t bytes = ((uint64_t)r.y << 32) | r.x;
    if (bytes > CC_MAX_WND) bytes = CC_MAX_WND;
    const uint64_t cap = (uint64_t)x.cwnd + bytes;
    c[k] = x;
    store_global(R, u32x4{x.cwnd, (uint32_t)bytes, r.z, event});
    t[k].wnd_cap = cap < CC_MAX_WND ? (uint32_t)cap : CC_MAX_WND;
}

}  // namespace lvlip

extern "C" {

int lvlip_cc_dev(const lvlip_snd_flow* s, const lvlip_snd_result* snd, const lvlip_rto_result* prev,
                 lvlip_cc_flow* c, lvlip_rto_flow* t, uint32_t nflows, const lvlip_frame_desc* fd,
                 const uint8_t* sacked, lvlip_cc_result* res, void* stream) {
    using namespace lvlip;
    if (nflows == 0) return LVLIP_OK;
    if (!s || !c || !t || !res || (sacked && !fd)) return LVLIP_EINVAL;
    if (nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    if (((uintptr_t)s & 7u) || ((uintptr_t)c & 7u) || ((uintptr_t)t & 7u) || ((uintptr_t)snd & 15u) ||
        ((uintptr_t)prev & 15u) || ((uintptr_t)fd & 15u) || ((uintptr_t)res & 15u))
        return LVLIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int rc = lvlip_launch_status(hipMemsetAsync(res, 0, (size_t)nflows * sizeof *res, st), "lvlip_cc_dev: memset");
    if (rc != LVLIP_OK) return rc;
    if (sacked) {
        // a queue's chunks, sized from the flow count as lvlip_sack_dev sizes k_sack_mark's: a wave whose chunk
        // lies behind its queue's end leaves after three loads
        const uint32_t fgrid = (nflows + CC_WAVES - 1u) / CC_WAVES;
        uint32_t y = CC_GRID / fgrid;
        y = y > CC_Y ? CC_Y : y < CC_Y_MIN ? CC_Y_MIN : y;
        hipLaunchKernelGGL(k_cc_sum, dim3(fgrid, y), dim3(256), 0, st, s, snd, (const lvlip_rto_flow*)t, nflows, fd,
                           sacked, res);
        if ((rc = lvlip_launched("k_cc_sum")) != LVLIP_OK) return rc;
    }
    hipLaunchKernelGGL(k_cc_fin, dim3((nflows + 255u) / 256u), dim3(256), 0, st, s, snd, prev, c, t, nflows, res);
    return lvlip_launched("k_cc_fin");
}

}  // extern "C"
