// snd_kernels.hip — the ACK side of a coalesced batch and the retransmit on
// the device (include/lvlip_skb.h, "f2 on the device: the ACK side and the
// retransmit").  snd_cpu.c is the same on the calling thread, bit for bit.
//
// lvlip_snd_dev: res is zeroed on the stream, then two kernels.
//
//   k_snd_rec   one lane per record.  The lane classifies its record's ack_seq
//               against its flow's snd_una and snd_nxt (two gathers) and the
//               wave then reduces BEFORE any atomic: it takes the flow of its
//               first pending lane, counts that flow's lanes per class with
//               ballots, takes the largest d with a butterfly max, and five
//               lanes issue the flow's atomics (four class counts, one max);
//               then the next flow, SND_PEEL times (wave_peel, wave_ops.h,
//               which k_sack_parse runs too).  A batch of one flow (a
//               bulk sender's ACK stream) thus costs five atomics per wave
//               instead of 128 on one address.  Lanes still pending after
//               SND_PEEL rounds belong to a wave of many flows, whose
//               addresses do not collide: they issue their own two atomics.
//               Integer add and max are the only reductions, so the 32 bytes
//               do not depend on the order the records arrive or run in.
//   k_snd_fin   one wave per flow: the leading run of tcp_clean_rto_queue
//               (src/tcp_input.c:72-84).  64 queue entries per step, one per
//               lane: descriptor, then the three header dwords that hold
//               ihl, ip.len, seq and hl (unaligned: two aligned loads and a
//               v_alignbyte each, all inside the 54 header bytes); a ballot of
//               "not fully acknowledged" ends the scan at its first set bit,
//               so a flow costs ceil((popped + 1) / 64) steps whatever its
//               queue holds.
//
// lvlip_rtx_dev: ONE launch, k_rtx.  lvlip_rtx_sack_dev ("the scoreboard and the
// selective retransmit") is k_pick, which chooses each slot's queue entry
// from the scoreboard, and then the same k_rtx from the queue entry onwards.
//
// Work mapping.  One DPP row (16 lanes) per slot, four slots per wave, 16 per
// 256-thread workgroup, as k_tso and k_lro map their frames; slot g -> flow by
// a binary search over the flows' slot0 (lvlip_snd_plan's running count).  The
// frame sizes are in device memory, so the host cannot pick a shape per
// launch, and the row is the shape that holds for all of them: a row sweeps
// its frame 16 chunks at a time with RTX_U sweeps (1.5 KiB) in flight, so a
// 55-B frame (four chunks, one of them beyond the header) occupies one row
// for one round, a 1514-B frame (at most 93 chunks behind the header's) is
// one round with every load in flight at once, a 9000-B frame six rounds, and
// a wave always has four frames' streams going.
// A wave per frame would leave 60 of 64 lanes idle on ACK-sized frames and
// gain nothing on MTU frames, which one round of a row already covers.
//
// One pass.  Every lane of the row loads the (at most five) aligned chunks
// that hold the 54 header bytes (the same addresses in all 16 lanes: one
// request) and funnels them into the frame's dwords h[0..13].  The header is
// patched in registers as tcp_transmit_skb patches it (ack_seq, win, csum 0,
// src/tcp_output.c:107-110) and its ten TCP words are summed from the
// registers (tcp_hdr_dev.h); the sweep sums only the bytes behind the header, frame bytes
// [54, 14 + ip.len), each read once, masked to the segment at both ends.  The
// frame's u16 words start at frame byte 34, an even offset, so for a frame at
// an odd address the two bytes of every aligned u16 are swapped before summing
// (v_perm), as in k_tso.  The fold happens once, on (seed + W) mod 2^32
// (src/utils.c:46-54).
//
// Why a full recomputation.  RFC 1624 would update the old field from the
// three changed words without reading the payload.  It is not bit-exact here:
// the reference adds the pseudo header in a u32 and loses the carry out of bit
// 31 (src/tcp.c:92-95), and whether the later (seed + W) wraps depends on W,
// the sum of the whole segment, which the old field no longer determines.  So
// the segment is summed again, which is also what tcp_transmit_skb does
// (src/tcp_output.c:126).
//
// Stores.  The ten rewritten bytes (42-45, 48-51) leave as one byte store from
// lanes 0-7 of the row; nothing else of the ring is written.  fd_out[slot] is
// one 16-B store.
//
// Bounds.  Flow and queue indices come from the planned s (slot0 ascending,
// seg0 + nseg below 2^32).  A frame is read only inside [F & ~15, F + fd.len
// rounded up to 16): the header chunks only when fd.len >= 54, the sweep only
// after 14 + ip.len <= fd.len held.  Lanes of a slot that is dead, or past
// nslots, load nothing from the ring and store nothing to it.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "csum_dev.h"
#include "flow_step.h"
#include "row_copy.h"
#include "tcp_hdr_dev.h"
#include "wave_ops.h"

namespace lvlip {

constexpr int SND_PEEL = 4;                      // flows a wave reduces before lanes go alone
constexpr uint32_t SND_WAVES = 4;                // flows per workgroup of k_snd_fin
constexpr uint32_t RTX_ROW = 16;                 // lanes per slot
constexpr uint32_t RTX_SLOTS = 256 / RTX_ROW;    // slots per workgroup
constexpr int RTX_U = 6;                         // sweeps of a row in flight: an MTU frame in one round
constexpr int RTX_HDR = TCP_FRAME_HDR;

// ------------------------------------------------------------ the ACK side --

__global__ __launch_bounds__(256) void k_snd_rec(const lvlip_lro_flow* f, const lvlip_snd_flow* s, uint32_t nflows,
                                                 const lvlip_lro_rec* rec, uint32_t n, lvlip_snd_result* res) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t flow = FLOW_NONE, cls = 4u, d = 0u;  // cls: flow_ack_class (flow_step.h), or 4: no ACK
    if (i < n) {
        const uint4 r = load_global(reinterpret_cast<uint64_t>(rec + i));  // flow, rel, dlen | status | flags, ack_seq
        flow = rec_ack_flow(r, f, nflows);
        if (flow != FLOW_NONE) {
            const uint32_t una = s[flow].snd_una, span = s[flow].snd_nxt - una;
            d = r.w - una;
            cls = flow_ack_class(d, span);
        }
    }
    const bool pending = wave_peel<SND_PEEL>(cls < 4u, flow, [=](uint32_t fl, bool mine) {
        const uint32_t c0 = __builtin_popcountll(__builtin_amdgcn_ballot_w64(mine && cls == FLOW_ACK_NEW));
        const uint32_t c1 = __builtin_popcountll(__builtin_amdgcn_ballot_w64(mine && cls == FLOW_ACK_DUP));
        const uint32_t c2 = __builtin_popcountll(__builtin_amdgcn_ballot_w64(mine && cls == FLOW_ACK_OLD));
        const uint32_t c3 = __builtin_popcountll(__builtin_amdgcn_ballot_w64(mine && cls == FLOW_ACK_BEYOND));
        const uint32_t mx = wave_max_u32(mine && cls == FLOW_ACK_NEW ? d : 0u);
        uint32_t* w = reinterpret_cast<uint32_t*>(res + fl);  // snd_una acked n_new n_dup n_old n_beyond popped inflight
        const uint32_t cnt = lane == 0u ? c0 : lane == 1u ? c1 : lane == 2u ? c2 : c3;
        if (lane < 4u && cnt) atomicAdd(w + 2u + lane, cnt);
        if (lane == 4u && mx) atomicMax(w + 1, mx);
    });
    if (pending) {
        uint32_t* w = reinterpret_cast<uint32_t*>(res + flow);
        atomicAdd(w + 2u + cls, 1u);
        if (cls == FLOW_ACK_NEW) atomicMax(w + 1, d);
    }
}

__global__ __launch_bounds__(256) void k_snd_fin(const lvlip_snd_flow* s, uint32_t nflows, const uint8_t* base,
                                                 const lvlip_frame_desc* fd, lvlip_snd_result* res) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k64 = (uint64_t)blockIdx.x * SND_WAVES + (threadIdx.x >> 6);
    if (k64 >= nflows) return;  // the whole wave
    const uint32_t k = (uint32_t)k64;
    const uint32_t una = s[k].snd_una, seg0 = s[k].seg0, nseg = s[k].nseg;
    const uint32_t acked = res[k].acked;
    uint32_t popped = nseg;
    for (uint64_t c0 = 0; c0 < nseg; c0 += 64u) {
        const uint64_t i = c0 + lane;
        bool stop = false;
        if (i < nseg) {
            const uint4 d = load_global(reinterpret_cast<uint64_t>(fd + (seg0 + (uint32_t)i)));  // offset lo, hi, len, -
            stop = d.z < (uint32_t)RTX_HDR;
            if (!stop) {
                const uint64_t F = reinterpret_cast<uint64_t>(base) + (((uint64_t)d.y << 32) | d.x);
                const uint32_t a = load_u32_any(F + 14u);  // version | ihl, tos, ip.len
                const uint32_t seq = __builtin_bswap32(load_u32_any(F + 38u));
                const uint32_t hl = (load_u32_any(F + 44u) >> 20) & 0xfu;  // byte 46
                const uint32_t iplen = bswap16u(a >> 16);
                const uint32_t end_seq = seq + iplen - 4u * (a & 0xfu) - 4u * hl;  // src/tcp.c:46-50
                stop = end_seq - una > acked;  // src/tcp_input.c:73, mod 2^32
            }
        }
        const uint64_t b = __builtin_amdgcn_ballot_w64(stop);
        if (b) {
            popped = (uint32_t)c0 + (uint32_t)__builtin_ctzll(b);
            break;
        }
    }
    if (lane == 0u) {
        res[k].snd_una = una + acked;
        res[k].popped = popped;
        res[k].inflight = nseg - popped;
    }
}

// ---------------------------------------------------------- the retransmit --

// The selection pass of lvlip_rtx_sack_dev, one wave per flow: pick[slot0 + j]
// is the j-th queue entry from seg0 + popped whose scoreboard byte is 0 (every
// entry when sacked is NULL).  64 bytes a step, one per lane; a ballot of the
// zero bytes and a popcount of the bits below the lane rank them.  The scan
// ends once rtx entries are found, so a flow costs as many steps as it skips
// marks; the slots left over get 0xFFFFFFFF.
__global__ __launch_bounds__(256) void k_pick(const lvlip_snd_flow* s, const lvlip_snd_result* snd,
                                                  const uint8_t* sacked, uint32_t nflows, uint32_t* pick) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k64 = (uint64_t)blockIdx.x * SND_WAVES + (threadIdx.x >> 6);
    if (k64 >= nflows) return;  // the whole wave
    const uint32_t k = (uint32_t)k64;
    const uint32_t seg0 = s[k].seg0, nseg = s[k].nseg, rtx = s[k].rtx;
    uint32_t* out = pick + s[k].slot0;
    uint32_t found = 0;
    for (uint64_t c0 = snd ? snd[k].popped : 0u; c0 < nseg && found < rtx; c0 += 64u) {
        const uint64_t i = c0 + lane;
        const bool open = i < nseg && (!sacked || sacked[seg0 + (uint32_t)i] == 0);
        const uint64_t b = __builtin_amdgcn_ballot_w64(open);
        const uint32_t rank = found + (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1ull));
        if (open && rank < rtx) out[rank] = seg0 + (uint32_t)i;
        found += (uint32_t)__builtin_popcountll(b);
    }
    for (uint64_t j = (uint64_t)found + lane; j < rtx; j += 64u) out[j] = FLOW_NONE;
}

// with pick, the slot's queue entry is pick[slot] (0xFFFFFFFF: dead), as k_pick left it, not popped + j
__global__ __launch_bounds__(256) void k_rtx(const lvlip_lro_flow* f, const lvlip_lro_result* lro,
                                             const lvlip_snd_flow* s, const lvlip_snd_result* snd, uint32_t nflows,
                                             uint32_t nslots, uint8_t* base, const lvlip_frame_desc* fd,
                                             lvlip_frame_desc* fd_out, const uint32_t* pick) {
    const uint32_t tl = threadIdx.x & (RTX_ROW - 1u);
    const uint64_t g64 = (uint64_t)blockIdx.x * RTX_SLOTS + (threadIdx.x / RTX_ROW);
    const bool inside = g64 < nslots;
    const uint32_t g = inside ? (uint32_t)g64 : 0u;

    // the flow of slot g: the last one whose slot0 is <= g (slot0 never falls, s[0].slot0 == 0; among
    // flows that share a slot0 only the last has a slot)
    const uint32_t slo = slot_owner<&lvlip_snd_flow::slot0>(s, nflows, g);
    const lvlip_snd_flow* t = s + slo;
    uint32_t e = FLOW_NONE;  // the slot's queue entry
    if (pick) {
        if (inside) e = pick[g];
    } else {
        const uint32_t nseg = t->nseg, j = g - t->slot0;
        const uint32_t popped = snd ? snd[slo].popped : 0u;
        if (inside && j < t->rtx && popped < nseg && j < nseg - popped) e = t->seg0 + popped + j;
    }
    bool live = e != FLOW_NONE;

    uint4 d = make_uint4(0u, 0u, 0u, 0u);  // the queue entry: offset lo, hi, len, reserved
    if (live) d = load_global(reinterpret_cast<uint64_t>(fd + e));
    live = live && d.z >= (uint32_t)RTX_HDR;
    const uint64_t F = reinterpret_cast<uint64_t>(base) + (((uint64_t)d.y << 32) | d.x);  // the frame's first byte
    const int fo = (int)(F & 15ull);
    const uint64_t D = F - (uint64_t)fo;  // chunk 0

    // ---- the 54 header bytes: chunks 0 .. (fo + 53) / 16, funnelled to the frame's dwords
    uint4 c[5];
#pragma unroll
    for (int i = 0; i < 5; ++i)
        c[i] = live && 16 * i < fo + RTX_HDR ? load_global(D + 16ull * i) : make_uint4(0u, 0u, 0u, 0u);
    uint32_t h[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint4 b = funnel16(c[i], c[i + 1], (uint32_t)fo);
        h[4 * i] = b.x, h[4 * i + 1] = b.y, h[4 * i + 2] = b.z, h[4 * i + 3] = b.w;
    }
    uint32_t iplen, hl;  // bytes 16-17, byte 46
    live = rtx_frame_ok((h[3] >> 16) | (h[4] << 16), h[11], d.z, &iplen, &hl) && live;
    const int L = 14 + (int)iplen;              // the frame's bytes the segment ends at
    const uint32_t nch = live ? (uint32_t)(fo + L + 15) >> 4 : 0u;
    const uint32_t kb = (uint32_t)(fo + RTX_HDR) >> 4;  // the first chunk with a byte behind the header: 3 or 4
    const uint32_t sel = (F & 1ull) ? 0x02030001u : 0x03020100u;

    // ---- frame bytes [54, L): summed chunk by chunk, masked at both ends
    uint32_t acc = 0;
    for (uint32_t k0 = kb; k0 < nch; k0 += RTX_ROW * RTX_U) {
        uint4 v[RTX_U];
#pragma unroll
        for (int u = 0; u < RTX_U; ++u) {
            const uint32_t k = k0 + (uint32_t)u * RTX_ROW + tl;
            v[u] = k < nch ? load_nt_global(D + 16ull * k) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < RTX_U; ++u) {
            const uint32_t k = k0 + (uint32_t)u * RTX_ROW + tl;
            const int rel = (int)(16u * k) - fo;  // the frame byte chunk k starts at
            const uint4 m = mask_chunk(v[u], min(max(RTX_HDR - rel, 0), 16), min(max(L - rel, 0), 16));
            acc = chunk_acc(m, sel, acc);
        }
    }
    const uint32_t W = row_sum_dpp(acc);  // in every lane of the row

    // ---- the TCP header as tcp_transmit_skb leaves it (every lane of the row the same)
    const uint32_t rcv_nxt = f[slo].rcv_nxt + (lro ? lro[slo].delivered : 0u);
    const uint32_t ack = __builtin_bswap32(rcv_nxt);
    const uint32_t win = bswap16u(t->win);                       // src/tcp_output.c:109,123
    hdr_put_ack(h, ack);
    h[12] = win;                                                 // tcp.csum = 0, :110
    const uint32_t thw = hdr_tcp_words(h);
    const uint32_t csum = finish(hdr_tcp_seed(h, iplen - 20u), thw + W);  // :126

    // ---- bytes 42-45, 48-49, 50-51: lane tl of the row stores one
    if (live && tl < 8u) {
        typedef __attribute__((address_space(1))) uint8_t gby;
        const uint32_t word = tl < 4u ? ack : win | (csum << 16);
        const uint32_t at = tl < 4u ? 42u + tl : 44u + tl;
        *reinterpret_cast<gby*>(F + at) = (uint8_t)(word >> (8u * (tl & 3u)));
    }
    if (inside && tl == 0u)
        store_global(reinterpret_cast<uint64_t>(fd_out + g), live ? u32x4{d.x, d.y, d.z, d.w} : u32x4{0u, 0u, 0u, 0u});
}

}  // namespace lvlip

// lvlip_rtx_dev (pick NULL: slot j of a flow is queue entry popped + j) and
// lvlip_rtx_sack_dev (k_pick fills pick from the scoreboard first)
static int rtx_launch(const lvlip_lro_flow* f, const lvlip_lro_result* lro, const lvlip_snd_flow* s,
                      const lvlip_snd_result* snd, const uint8_t* sacked, uint32_t nflows, uint32_t nslots,
                      void* base, const lvlip_frame_desc* fd, lvlip_frame_desc* fd_out, uint32_t* pick,
                      void* stream) {
    if (nslots == 0) return LVLIP_OK;
    if (!f || !s || !base || !fd || !fd_out) return LVLIP_EINVAL;
    if (nflows == 0 || nflows > LVLIP_LRO_MAX_FLOWS || nslots > LVLIP_MAX_BATCH) return LVLIP_EINVAL;
    if (any_misaligned<8>(f, s) || any_misaligned<16>(lro, snd, fd, fd_out) || any_misaligned<4>(pick))
        return LVLIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (pick) {
        const uint32_t fgrid = (nflows + lvlip::SND_WAVES - 1u) / lvlip::SND_WAVES;
        hipLaunchKernelGGL(lvlip::k_pick, dim3(fgrid), dim3(256), 0, st, s, snd, sacked, nflows, pick);
        const int rc = lvlip_launched("k_pick");
        if (rc != LVLIP_OK) return rc;
    }
    const uint32_t grid = (uint32_t)(((uint64_t)nslots + lvlip::RTX_SLOTS - 1u) / lvlip::RTX_SLOTS);
    hipLaunchKernelGGL(lvlip::k_rtx, dim3(grid), dim3(256), 0, st, f, lro, s, snd, nflows, nslots, (uint8_t*)base, fd,
                       fd_out, (const uint32_t*)pick);
    return lvlip_launched("k_rtx");
}

extern "C" {

int lvlip_snd_dev(const lvlip_lro_flow* f, const lvlip_snd_flow* s, uint32_t nflows, const lvlip_lro_rec* rec,
                  uint32_t n, const void* base, const lvlip_frame_desc* fd, lvlip_snd_result* res, void* stream) {
    if (nflows == 0 || n == 0) return LVLIP_OK;
    if (!f || !s || !rec || !base || !fd || !res) return LVLIP_EINVAL;
    if (n > LVLIP_MAX_BATCH || nflows > LVLIP_LRO_MAX_FLOWS) return LVLIP_EINVAL;
    if (any_misaligned<8>(f, s) || any_misaligned<16>(rec, fd, res)) return LVLIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int rc = lvlip_launch_status(hipMemsetAsync(res, 0, (size_t)nflows * sizeof *res, st), "lvlip_snd_dev: memset");
    if (rc != LVLIP_OK) return rc;
    const uint32_t grid = (uint32_t)(((uint64_t)n + 255u) / 256u);
    hipLaunchKernelGGL(lvlip::k_snd_rec, dim3(grid), dim3(256), 0, st, f, s, nflows, rec, n, res);
    rc = lvlip_launched("k_snd_rec");
    if (rc != LVLIP_OK) return rc;
    const uint32_t fgrid = (nflows + lvlip::SND_WAVES - 1u) / lvlip::SND_WAVES;
    hipLaunchKernelGGL(lvlip::k_snd_fin, dim3(fgrid), dim3(256), 0, st, s, nflows, (const uint8_t*)base, fd, res);
    return lvlip_launched("k_snd_fin");
}

int lvlip_rtx_dev(const lvlip_lro_flow* f, const lvlip_lro_result* lro, const lvlip_snd_flow* s,
                  const lvlip_snd_result* snd, uint32_t nflows, uint32_t nslots, void* base,
                  const lvlip_frame_desc* fd, lvlip_frame_desc* fd_out, void* stream) {
    return rtx_launch(f, lro, s, snd, nullptr, nflows, nslots, base, fd, fd_out, nullptr, stream);
}

int lvlip_rtx_sack_dev(const lvlip_lro_flow* f, const lvlip_lro_result* lro, const lvlip_snd_flow* s,
                       const lvlip_snd_result* snd, const uint8_t* sacked, uint32_t nflows, uint32_t nslots,
                       void* base, const lvlip_frame_desc* fd, lvlip_frame_desc* fd_out, uint32_t* pick,
                       void* stream) {
    if (nslots && !pick) return LVLIP_EINVAL;
    return rtx_launch(f, lro, s, snd, sacked, nflows, nslots, base, fd, fd_out, pick, stream);
}

}  // extern "C"
