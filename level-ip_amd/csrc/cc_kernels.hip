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
//   k_cc_fin   one lane per flow: steps 1, 2 and 4 on the sums (flow_step.h,
//              which cc_cpu.c calls too), c[k] (32 B), res[k] (one 16-B store)
//              and t[k].wnd_cap.
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

#include "flow_step.h"
#include "tcp_hdr_dev.h"
#include "wave_ops.h"

namespace lvlip {

constexpr uint32_t CC_WAVES = 4;          // waves (flows) per workgroup of k_cc_sum
constexpr uint32_t CC_Y = 1024;           // most chunks a queue is spread over
constexpr uint32_t CC_Y_MIN = 8;          // fewest
constexpr uint32_t CC_GRID = 1u << 17;    // workgroups of k_cc_sum the chunk count aims at
constexpr int CC_UNROLL = 4;              // chunks of 64 entries a wave has in flight

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
            // behind TCP_FRAME_HDR, the header of every frame lvlip_tso_* / lvlip_push_* build
            bytes += flen[u] >= (uint32_t)TCP_FRAME_HDR ? flen[u] - (uint32_t)TCP_FRAME_HDR : 0u;
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
    uint32_t a = 0u, n_new = 0u, fired = 0u, bo = 0u;
    if (snd) {
        const uint4 v = load_global(reinterpret_cast<uint64_t>(snd + k));  // snd_una, acked, n_new, n_dup
        a = v.y, n_new = v.z;
    }
    if (prev) {
        const uint4 v = load_global(reinterpret_cast<uint64_t>(prev + k));  // fired, sample, rto, backoff
        fired = v.x, bo = v.w;
    }
    const uint32_t event = flow_cc_step(&x, s[k].snd_una, s[k].snd_nxt, a, n_new, fired, bo);  // 1: loss, 2: ACKs
    uint32_t bytes;
    const uint32_t cap = flow_cc_cap(x.cwnd, ((uint64_t)r.y << 32) | r.x, &bytes);  // 4: output
    c[k] = x;
    store_global(R, u32x4{x.cwnd, bytes, r.z, event});
    t[k].wnd_cap = cap;
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
    if (any_misaligned<8>(s, c, t) || any_misaligned<16>(snd, prev, fd, res)) return LVLIP_EINVAL;
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
