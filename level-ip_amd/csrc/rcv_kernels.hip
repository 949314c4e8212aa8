// rcv_kernels.hip — TCP receive coalescing on the device (include/lvlip_skb.h,
// "f1 on the device: receive coalescing"): frames in HBM -> each payload at its
// place in its flow's byte stream, one record per frame.  k_tso
// (seg_kernels.hip) run backwards, out of the same pieces (row_copy.h, and
// tcp_hdr_dev.h for the record's store);
// rcv_cpu.c is the same on the calling thread, bit for bit.
//
// Work mapping.  One DPP row (16 lanes) per frame, four frames per wave, 16
// per 256-thread workgroup.  Every lane of a row parses the frame (the same
// addresses: one request per row) with ip_rcv's decisions as parse_rx takes
// them (flat_src.h), reads the TCP fields, and finds the flow by a binary
// search over the planned flows' 12 key bytes.  A frame with ihl 5 and hl 5
// is decided out of the four-chunk header window (FrWin); options take byte
// loads.
//
// The copy is laid out by DESTINATION chunk of `out`: chunk k of a segment
// that lands at O is the 16 aligned bytes at (O & ~15) + 16 k.  The lane loads
// the one or two aligned frame chunks that hold its bytes (never a chunk
// without a payload byte of this frame), funnels them (v_alignbyte), and
// stores whole chunks as 16-B nontemporal stores, the first and last chunk as
// the dwords and bytes inside [O, O + dlen): a neighbour's bytes are never
// written.
//
// Without LVLIP_RX_VERIFY_L4 that is one pass.  With it the row sums the
// segment first, in the same layout: the funnelled chunks of the first
// LRO_KEEP sweeps (1.5 KiB of payload: a 1460-B segment whole) stay in registers, the TCP header's
// words are added from the header window, and only when the row's sum (one
// DPP reduction every lane waits for) verifies do the kept chunks leave; what
// lies beyond them is read a second time, from lines the row has just pulled
// through L2.  No lane stores a byte before the verdict: the stores depend on
// the reduction.
//
// Parity.  The checksum's u16 words are aligned to the TCP header; the
// payload starts an even number of bytes (hl*4) behind it, so destination
// chunk byte j is at segment offset hl*4 + 16 k - (O & 15) + j: an aligned u16
// of the funnelled data is one TCP word when O is even, and the high byte of
// one word with the low byte of the next when O is odd, where the bytes of
// every u16 are swapped before summing (v_perm).  Either way every even-offset
// byte is added once and every odd-offset byte times 256: the exact word sum,
// whatever the frame's address.  The pseudo header is summed in RFC arithmetic
// (fr_pseudo_rfc), as lvlip_rx_verify_dev does.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "csum_dev.h"
#include "flat_src.h"
#include "row_copy.h"
#include "tcp_hdr_dev.h"

namespace lvlip {

constexpr uint32_t LRO_FRAMES = 256 / ROW;  // frames per workgroup
constexpr int LRO_U = 4;                    // sweeps of a row in flight
constexpr int LRO_KEEP = 6;                 // sweeps kept in registers until the verdict: a round
                                            // of LRO_U and one of the rest, 1.5 KiB of payload
constexpr uint32_t LRO_NONE = 0xFFFFFFFFu;
constexpr uint32_t TCP_CONTROL = 0x26u;     // SYN 0x02, RST 0x04, URG 0x20

// u16 word sum (as stored) of `words` words at p, byte loads: headers with options
__device__ __forceinline__ uint32_t words_sum(const uint8_t* p, uint32_t words) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < words; ++w) s += fr_le16(p + 2u * w);
    return s;
}

// a row's stores of one round: destination chunks k0 + 16 u + tl of nch
template <int U>
__device__ __forceinline__ void row_put(uint64_t D, int o, uint32_t dlen, uint32_t nch, uint32_t k0, uint32_t tl,
                                        const uint4* v) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t k = k0 + (uint32_t)u * ROW + tl;
        if (k < nch) store_chunk(D + 16ull * k, v[u], k == 0u ? o : 0, min(16, o + (int)dlen - (int)(16u * k)));
    }
}

// one round of the summing pass whose chunks stay in registers
template <int U>
__device__ __forceinline__ void sum_keep(uint64_t S, int o, uint32_t len, uint32_t nch, uint32_t k0, uint32_t tl,
                                         uint32_t sel, uint32_t& acc, uint4* kept) {
    uint4 v[U];
    row_gather<U, true>(S, o, len, nch, k0, tl, v);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        acc = chunk_acc(v[u], sel, acc);
        kept[u] = v[u];
    }
}

template <bool L4>
__global__ __launch_bounds__(256) void k_lro(const uint8_t* base, const lvlip_frame_desc* fd, uint32_t n,
                                             const lvlip_lro_flow* fl, uint32_t nflows, uint8_t* out,
                                             lvlip_lro_rec* rec) {
    const uint32_t tl = threadIdx.x & (ROW - 1u);
    const uint64_t g64 = (uint64_t)blockIdx.x * LRO_FRAMES + (threadIdx.x / ROW);
    const bool live = g64 < n;
    const uint32_t g = live ? (uint32_t)g64 : 0u;

    uint64_t foff;
    uint32_t flen;
    {
        typedef __attribute__((address_space(1))) const u32x4 gvec;
        const u32x4 d = *reinterpret_cast<gvec*>(reinterpret_cast<uint64_t>(fd + g));
        foff = ((uint64_t)d.y << 32) | d.x;
        flen = live ? d.z : 0u;
    }
    const uint8_t* h = base + foff;
    FrWin x;
    x.load(h, flen, reinterpret_cast<uint64_t>(fd + g));

    // ---- ip_rcv's decisions, in its order (parse_rx, rx_verdict_one)
    uint32_t st = 0, ihl = 5u, proto = 0u, iplen = 0u;
    bool inside = false;
    if (flen < FR_ETH + 20u) {
        st = LVLIP_RX_SHORT;
    } else if (x.be16(12) != 0x0800u) {
        st = LVLIP_RX_NOT_IP;
    } else {
        const uint32_t ver = x.b(14) >> 4;
        ihl = x.b(14) & 0x0fu;
        if (ver != 4u) {
            st = LVLIP_RX_BAD_VERSION;
        } else if (ihl < 5u) {
            st = LVLIP_RX_BAD_IHL;
        } else if (x.b(22) == 0u) {
            st = LVLIP_RX_TTL0;
        } else if (flen < FR_ETH + ihl * 4u) {
            st = LVLIP_RX_SHORT;
        } else {
            const uint32_t hw = ihl == 5u ? (x.A[0] >> 16) + halves(x.A[1]) + halves(x.A[2]) + halves(x.A[3]) +
                                                halves(x.A[4]) + (x.A[5] & 0xffffu)
                                          : words_sum(h + FR_ETH, ihl * 2u);
            proto = x.b(23);
            iplen = x.be16(16);
            inside = iplen >= ihl * 4u && flen >= FR_ETH + iplen;
            if (finish(0u, hw) != 0) st = LVLIP_RX_BAD_CSUM;
            else if (proto != 6u && proto != 1u) st = LVLIP_RX_UNKNOWN_PROTO;
            else if (L4 && !inside) st = LVLIP_RX_SHORT;
        }
    }
    const bool kept_frame = st == 0u;  // ip_rcv keeps it (the L4 sum still to come)
    const uint32_t l4len = (kept_frame && inside) ? iplen - ihl * 4u : 0u;
    const uint8_t* th = h + FR_ETH + ihl * 4u;

    // ---- tcp_init_segment's fields (src/tcp.c:40-50)
    uint32_t hl = 0u, seq = 0u, ack = 0u, tflags = 0u, ports = 0u;
    bool thdr = false;  // a TCP header that describes a segment inside the frame
    if (kept_frame && proto == 6u && l4len >= 20u) {
        if (ihl == 5u) {
            ports = (x.be16(34) << 16) | x.be16(36);
            seq = (x.be16(38) << 16) | x.be16(40);
            ack = (x.be16(42) << 16) | x.be16(44);
            hl = x.b(46) >> 4;
            tflags = x.b(47);
        } else {
            ports = (fr_be16(th) << 16) | fr_be16(th + 2);
            seq = (fr_be16(th + 4) << 16) | fr_be16(th + 6);
            ack = (fr_be16(th + 8) << 16) | fr_be16(th + 10);
            hl = (uint32_t)th[12] >> 4;
            tflags = th[13];
        }
        thdr = hl >= 5u && hl * 4u <= l4len;
    }
    const uint32_t dlen = thdr ? l4len - hl * 4u : 0u;

    // ---- the flow: the first planned key that is not below the frame's
    uint32_t flow = LRO_NONE, rel = seq, wnd = 0u;
    uint64_t out_off = 0;
    if (thdr) {
        const uint32_t k0 = __builtin_bswap32(x.le32(26)), k1 = __builtin_bswap32(x.le32(30));
        uint32_t lo = 0u, hi = nflows;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            const uint32_t* p = reinterpret_cast<const uint32_t*>(fl + mid);
            const uint32_t a0 = __builtin_bswap32(p[0]), a1 = __builtin_bswap32(p[1]), a2 = __builtin_bswap32(p[2]);
            const bool less = a0 < k0 || (a0 == k0 && (a1 < k1 || (a1 == k1 && a2 < ports)));
            if (less) lo = mid + 1u;
            else hi = mid;
        }
        if (lo < nflows) {
            const lvlip_lro_flow* c = fl + lo;
            const uint32_t* p = reinterpret_cast<const uint32_t*>(c);
            if (__builtin_bswap32(p[0]) == k0 && __builtin_bswap32(p[1]) == k1 && __builtin_bswap32(p[2]) == ports) {
                flow = lo;
                rel = seq - c->rcv_nxt;
                wnd = c->rcv_wnd;
                out_off = c->out_off;
            }
        }
    }

    // ---- what the frame is, unless its checksum says otherwise
    uint32_t st2 = LVLIP_LRO_PLACED;
    if (proto != 6u) st2 = LVLIP_LRO_NOT_TCP;
    else if (!thdr) st2 = LVLIP_LRO_BAD_TCP_HDR;
    else if (flow == LRO_NONE) st2 = LVLIP_LRO_NO_FLOW;
    else if (tflags & TCP_CONTROL) st2 = LVLIP_LRO_CONTROL;
    else if (dlen == 0u) st2 = LVLIP_LRO_NO_DATA;
    else if ((uint64_t)rel + dlen > wnd) st2 = LVLIP_LRO_OUT_OF_WINDOW;
    bool place = kept_frame && st2 == LVLIP_LRO_PLACED;

    const uint64_t O = reinterpret_cast<uint64_t>(out) + out_off + rel;  // the payload's first byte in out
    const int o = place ? (int)(O & 15ull) : 0;
    const uint64_t D = O - (uint64_t)o;                                   // destination chunk 0
    const uint64_t S = reinterpret_cast<uint64_t>(th) + hl * 4u;          // the payload's first byte in the frame
    const uint32_t nch = place ? (uint32_t)(o + (int)dlen + 15) >> 4 : 0u;

    uint4 kept[LRO_KEEP];
    if (L4) {
        // ---- sum first: the payload behind a sound TCP header in the
        // destination's layout (a frame that is not placed: layout 0), any
        // other L4 message (ICMP, a TCP header that does not fit) whole
        const uint64_t SS = thdr ? S : reinterpret_cast<uint64_t>(th);
        const uint32_t sl = thdr ? dlen : l4len;
        const uint32_t nsum = kept_frame ? (uint32_t)(o + (int)sl + 15) >> 4 : 0u;
        const uint32_t sel = (o & 1) ? 0x02030001u : 0x03020100u;
        uint32_t acc = 0;
        sum_keep<LRO_U>(SS, o, sl, nsum, 0u, tl, sel, acc, kept);
        if (ROW * LRO_U < nsum) sum_keep<LRO_KEEP - LRO_U>(SS, o, sl, nsum, ROW * LRO_U, tl, sel, acc, kept + LRO_U);
        // beyond the kept sweeps: plain loads, the lines are read again below
        for (uint32_t k0 = ROW * LRO_KEEP; k0 < nsum; k0 += ROW * LRO_U) {
            uint4 v[LRO_U];
            row_gather<LRO_U, false>(SS, o, sl, nsum, k0, tl, v);
#pragma unroll
            for (int u = 0; u < LRO_U; ++u) acc = chunk_acc(v[u], sel, acc);
        }
        uint32_t hsum = 0u;
        if (thdr)
            hsum = (ihl == 5u && hl == 5u) ? (x.A[5] >> 16) + halves(x.A[6]) + halves(x.A[7]) + halves(x.A[8]) +
                                                 halves(x.A[9]) + (x.A[10] & 0xffffu)
                                           : words_sum(th, hl * 2u);
        const uint32_t W = row_sum_dpp(acc);  // in every lane of the row
        const uint32_t seed = proto == 6u ? fr_pseudo_rfc(x.le32(26), x.le32(30), 6u, l4len) : 0u;
        if (kept_frame && finish(seed, hsum + W) != 0) {
            st = LVLIP_RX_BAD_L4;
            place = false;
        }
        // ---- the verdict is known: the kept chunks leave
        if (place) {
            row_put<LRO_U>(D, o, dlen, nch, 0u, tl, kept);
            row_put<LRO_KEEP - LRO_U>(D, o, dlen, nch, ROW * LRO_U, tl, kept + LRO_U);
        }
    }
    // ---- copy: everything (one pass), or what the registers did not keep
    if (place) {
        for (uint32_t k0 = L4 ? ROW * LRO_KEEP : 0u; k0 < nch; k0 += ROW * LRO_U) {
            uint4 v[LRO_U];
            row_gather<LRO_U, true>(S, o, dlen, nch, k0, tl, v);
            row_put<LRO_U>(D, o, dlen, nch, k0, tl, v);
        }
    }
    if (st == 0u) st = st2;

    if (live && tl == 0u) {
        const bool tcp = st == LVLIP_LRO_PLACED || st >= LVLIP_LRO_NO_FLOW;  // the TCP fields mean something
        store_global(reinterpret_cast<uint64_t>(rec + g), tcp ? u32x4{flow, rel, dlen | (st << 16) | (tflags << 24), ack}
                                                              : u32x4{LRO_NONE, 0u, st << 16, 0u});
    }
}

}  // namespace lvlip

extern "C" {

int lvlip_lro_dev(const void* base, const lvlip_frame_desc* fd, uint32_t n, const lvlip_lro_flow* f,
                  uint32_t nflows, uint32_t flags, void* out, lvlip_lro_rec* rec, void* stream) {
    if (n == 0) return LVLIP_OK;
    if (!base || !fd || !out || !rec || (nflows && !f)) return LVLIP_EINVAL;
    if (n > LVLIP_MAX_BATCH || nflows > LVLIP_LRO_MAX_FLOWS || (flags & ~LVLIP_RX_VERIFY_L4)) return LVLIP_EINVAL;
    const uint32_t grid = (uint32_t)(((uint64_t)n + lvlip::LRO_FRAMES - 1u) / lvlip::LRO_FRAMES);
    if (flags & LVLIP_RX_VERIFY_L4)
        hipLaunchKernelGGL(lvlip::k_lro<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)base,
                           fd, n, f, nflows, (uint8_t*)out, rec);
    else
        hipLaunchKernelGGL(lvlip::k_lro<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)base,
                           fd, n, f, nflows, (uint8_t*)out, rec);
    return lvlip_launch_status(hipGetLastError(), "k_lro");
}

}  // extern "C"
