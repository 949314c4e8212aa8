// push_kernels.hip — the write queue on the device (include/lvlip_skb.h, "f2
// on the device: the write queue"): new writes cut into segments, built as
// frames in the flow's slots of the TX ring and appended to its queue, popped
// entries given back.  push_cpu.c is the same on the calling thread, bit for
// bit.  Three launches on the caller's stream, no workspace beyond res:
//
//   k_push_count  one wave per flow.  Step 1: when the queue does not start at
//                 q0 it is moved down there, 64 entries (a 16-B descriptor and
//                 a scoreboard byte per lane) a step in ascending order.  A
//                 step loads all of its entries before it stores one (the
//                 stores take the loads' data), and its stores end below the
//                 next step's loads because q0 < seg0: memmove's result
//                 whatever the distance.  Step 2: lane 0 counts m
//                 (flow_step.h, which push_cpu.c calls too) and writes res
//                 and seg0.
//   k_push        k_tso's mapping and k_tso's row (seg_frame_dev.h): one DPP
//                 row per slot, four slots per wave; slot g -> flow by a binary
//                 search over the flows' slot0 (lvlip_push_plan's running sum);
//                 slot i of a flow is live when i < res.pushed.  The template
//                 gets ack_seq and the window as k_rtx writes them, seq is
//                 snd_nxt + i*mss.  It reads w and s before the step.
//   k_push_step   one lane per flow, as k_snd_next: nseg, snd_nxt, pay_off,
//                 unsent, slot_nxt.
//
// Bounds.  Flow indices are below nflows.  Ring, fd and scoreboard addresses
// come from the planned w and s (lvlip_push_plan: regions disjoint, the queue
// inside [q0, q0 + cap), slot_nxt < cap): m <= cap - nseg keeps every new
// entry inside the region, and a slot index is below cap.  A queue that lies
// below q0, or is longer than cap, is not the plan's: nothing is moved and
// nothing is pushed.  Rows of a slot that is dead, or past nslots, load
// nothing from the payload and store nothing to the ring.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "flow_step.h"
#include "seg_frame_dev.h"

namespace lvlip {

constexpr uint32_t PUSH_WAVES = 4;  // flows per workgroup of k_push_count

__global__ __launch_bounds__(256) void k_push_count(lvlip_snd_flow* s, const lvlip_push_flow* w, uint32_t nflows,
                                                    lvlip_frame_desc* fd, uint8_t* sacked, lvlip_push_result* res) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k64 = (uint64_t)blockIdx.x * PUSH_WAVES + (threadIdx.x >> 6);
    if (k64 >= nflows) return;  // the whole wave
    const uint32_t k = (uint32_t)k64;
    const uint32_t una = s[k].snd_una, nxt = s[k].snd_nxt, seg0 = s[k].seg0, nseg = s[k].nseg;
    const lvlip_push_flow* t = w + k;
    const uint32_t q0 = t->q0, cap = t->cap;

    // ---- 1: the queue down to q0
    const uint32_t moved = seg0 != q0 ? nseg : 0u;
    if (seg0 > q0 && nseg <= cap) {
        for (uint64_t c0 = 0; c0 < nseg; c0 += 64u) {
            const uint64_t i = c0 + lane;
            uint4 d = make_uint4(0u, 0u, 0u, 0u);
            uint8_t b = 0;
            if (i < nseg) {
                d = load_global(reinterpret_cast<uint64_t>(fd + (seg0 + (uint32_t)i)));
                if (sacked) b = sacked[seg0 + (uint32_t)i];
            }
            __builtin_amdgcn_wave_barrier();  // every load of the step is issued before its first store
            if (i < nseg) {
                store_global(reinterpret_cast<uint64_t>(fd + (q0 + (uint32_t)i)), u32x4{d.x, d.y, d.z, d.w});
                if (sacked) sacked[q0 + (uint32_t)i] = b;
            }
        }
    }

    // ---- 2: the count
    if (lane == 0u) {
        // register copies of the words the count reads: the queue where step 1 found it (flow_push_count
        // refuses one below q0), and of w[k] the four words not loaded yet
        lvlip_snd_flow q = {};
        q.snd_una = una, q.snd_nxt = nxt, q.seg0 = seg0, q.nseg = nseg;
        lvlip_push_flow p = {};
        p.q0 = q0, p.cap = cap, p.unsent = t->unsent, p.mss = t->mss, p.wnd = t->wnd, p.push = t->push;
        uint32_t bytes;
        const uint32_t m = flow_push_count(&p, &q, &bytes);
        store_global(reinterpret_cast<uint64_t>(res + k), u32x4{m, bytes, q0 + nseg, moved});
        s[k].seg0 = q0;
    }
}

__global__ __launch_bounds__(256) void k_push(const lvlip_lro_flow* f, const lvlip_lro_result* lro,
                                              const lvlip_snd_flow* s, const lvlip_push_flow* w, uint32_t nflows,
                                              uint32_t nslots, const uint8_t* payload, uint8_t* base,
                                              lvlip_frame_desc* fd, uint8_t* sacked, lvlip_frame_desc* fd_out,
                                              const lvlip_push_result* res) {
    const uint32_t tl = threadIdx.x & (TSO_ROW - 1u);
    const uint64_t g64 = (uint64_t)blockIdx.x * TSO_SEGS + (threadIdx.x / TSO_ROW);
    const bool inside = g64 < nslots;
    const uint32_t g = inside ? (uint32_t)g64 : 0u;

    // the flow of slot g: the last one whose slot0 is <= g (slot0 never falls, w[0].slot0 == 0; among
    // flows that share a slot0 only the last has a slot)
    const uint32_t k = slot_owner<&lvlip_push_flow::slot0>(w, nflows, g);
    const lvlip_push_flow* t = w + k;
    const uint4 r = load_global(reinterpret_cast<uint64_t>(res + k));  // pushed, bytes, first, moved
    const uint32_t i = g - t->slot0;
    const bool live = inside && g >= t->slot0 && i < t->push && i < r.x;
    const uint32_t mss = t->mss, unsent = t->unsent;
    const uint64_t done = (uint64_t)i * mss;
    const uint32_t dlen = live ? (unsent - done < mss ? (uint32_t)(unsent - done) : mss) : 0u;  // i < ceil(unsent / mss)
    const bool last = done + dlen == unsent;

    // slots go round robin: slot_nxt < cap and i < pushed <= cap
    uint64_t slot = (uint64_t)t->slot_nxt + i;
    if (slot >= t->cap) slot -= t->cap;
    const uint64_t off = live ? t->ring_off + slot * t->stride : 0ull;
    const uint64_t F = reinterpret_cast<uint64_t>(base) + off;
    const uint64_t S = reinterpret_cast<uint64_t>(payload) + t->pay_off + done;
    // The template, with tcp_transmit_skb's ack_seq and window (src/tcp_output.c:107-109) as k_rtx writes them,
    // and seq from snd_nxt: all loaded behind the sweep, where the row's registers are free again (with the
    // template held across the sweep the kernel needs 132 VGPRs, a wave per SIMD fewer).
    uint32_t h[14];
    tso_frame(tl, live, h, F, S, dlen, last, [=](uint32_t(&hd)[14]) {
        const uint32_t* hw = reinterpret_cast<const uint32_t*>(t->hdr);  // offset 52 of an 8-B aligned struct
#pragma unroll
        for (int j = 0; j < 14; ++j) hd[j] = hw[j];
        hdr_put_ack(hd, __builtin_bswap32(f[k].rcv_nxt + (lro ? lro[k].delivered : 0u)));
        hd[12] = (hd[12] & 0xffff0000u) | bswap16u(s[k].win);
        return s[k].snd_nxt + (uint32_t)done;
    });

    if (inside && tl == 0u) {
        const u32x4 d = live ? u32x4{(uint32_t)off, (uint32_t)(off >> 32), (uint32_t)TSO_HDR + dlen, 0u}
                             : u32x4{0u, 0u, 0u, 0u};
        store_global(reinterpret_cast<uint64_t>(fd_out + g), d);
        if (live) {
            store_global(reinterpret_cast<uint64_t>(fd + (r.z + i)), d);
            if (sacked) sacked[r.z + i] = 0;
        }
    }
}

__global__ __launch_bounds__(256) void k_push_step(lvlip_snd_flow* s, lvlip_push_flow* w, uint32_t nflows,
                                                   const lvlip_push_result* res) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;  // nflows <= 65536
    if (k >= nflows) return;
    uint2* sw = reinterpret_cast<uint2*>(s + k);  // [0] snd_una, snd_nxt; [1] seg0, nseg
    uint2* ww = reinterpret_cast<uint2*>(w + k);  // [0] pay_off; [2] unsent, stride; [3] cap, q0; [4] slot_nxt, push
    const uint4 r = load_global(reinterpret_cast<uint64_t>(res + k));  // pushed, bytes, first, moved
    uint2 a = sw[0], q = sw[1], p = ww[0], u = ww[2], n = ww[4];
    const uint32_t cap = ww[3].x;
    a.y += r.y;
    q.y += r.x;
    const uint64_t pay = (((uint64_t)p.y << 32) | p.x) + r.y;
    p.x = (uint32_t)pay, p.y = (uint32_t)(pay >> 32);
    u.x -= r.y;
    const uint64_t nx = (uint64_t)n.x + r.x;  // slot_nxt < cap, pushed <= cap
    n.x = (uint32_t)(nx >= cap ? nx - cap : nx);
    sw[0] = a, sw[1] = q;
    ww[0] = p, ww[2] = u, ww[4] = n;
}

}  // namespace lvlip

extern "C" {

int lvlip_push_dev(const lvlip_lro_flow* f, const lvlip_lro_result* lro, lvlip_snd_flow* s, lvlip_push_flow* w,
                   uint32_t nflows, uint32_t nslots, const void* payload, void* base, lvlip_frame_desc* fd,
                   uint8_t* sacked, lvlip_frame_desc* fd_out, lvlip_push_result* res, void* stream) {
    if (nflows > LVLIP_LRO_MAX_FLOWS || nslots > LVLIP_MAX_BATCH) return LVLIP_EINVAL;
    if (nslots && (!payload || !base || !fd_out || nflows == 0)) return LVLIP_EINVAL;
    if (nflows == 0) return LVLIP_OK;
    if (!f || !s || !w || !fd || !res) return LVLIP_EINVAL;
    if (any_misaligned<8>(f, s, w) || any_misaligned<16>(lro, fd, fd_out, res)) return LVLIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t fgrid = (nflows + lvlip::PUSH_WAVES - 1u) / lvlip::PUSH_WAVES;
    hipLaunchKernelGGL(lvlip::k_push_count, dim3(fgrid), dim3(256), 0, st, s, w, nflows, fd, sacked, res);
    int rc = lvlip_launched("k_push_count");
    if (rc != LVLIP_OK) return rc;
    if (nslots) {
        const uint32_t grid = (uint32_t)(((uint64_t)nslots + lvlip::TSO_SEGS - 1u) / lvlip::TSO_SEGS);
        hipLaunchKernelGGL(lvlip::k_push, dim3(grid), dim3(256), 0, st, f, lro, s, w, nflows, nslots,
                           (const uint8_t*)payload, (uint8_t*)base, fd, sacked, fd_out, res);
        rc = lvlip_launched("k_push");
        if (rc != LVLIP_OK) return rc;
    }
    hipLaunchKernelGGL(lvlip::k_push_step, dim3((nflows + 255u) / 256u), dim3(256), 0, st, s, w, nflows, res);
    return lvlip_launched("k_push_step");
}

}  // extern "C"
