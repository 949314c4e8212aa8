/*
 * lvlip_skb.h — batch-and-dispatch over level-ip frames.
 *
 * level-ip handles one frame at a time: netdev_rx_loop reads one frame per
 * read(2) (src/netdev.c:86-101) and every checksum is a synchronous per-packet
 * call.  These entry points take N frames at once and run all their checksums
 * as ONE GPU batch through a context (include/lvlip_csum.h, Group 3).
 *
 * A frame is what an sk_buff holds (include/skbuff.h:9-23): `head` points at the
 * Ethernet header, the IPv4 header is at head + 14 (ip_hdr(), include/ip.h:47-50)
 * and the TCP/ICMP header right after it (tcp_hdr(), include/tcp.h:224-227).
 *
 * The device parses every frame (the same kernels as the _dev calls below):
 * the host moves whole frames to the GPU (a gather into a pinned arena, or,
 * for frames inside a registered region, DMA of its spans or in-place reads),
 * and gets back one verdict (RX) or one record of the two fields (TX) per
 * frame.  The plan and apply steps below are the same decisions as plain host
 * logic (no GPU): the CPU tests and the sanitizer harness exercise them.
 * (Round 4's host frame path batched the planned pieces through
 * lvlip_csum_batch_host; round 5 retired it, slower from every source.)
 */
#ifndef LVLIP_SKB_H
#define LVLIP_SKB_H

#include <stdint.h>

#include "lvlip_csum.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

typedef struct lvlip_frame {
    uint8_t *head;  /* Ethernet header (skb->head) */
    uint32_t len;   /* bytes valid from head */
} lvlip_frame;

/* ---- f1: RX ------------------------------------------------------------ */

/* Verdicts, in the order ip_rcv (src/ip_input.c:17-43) takes its decisions. */
#define LVLIP_RX_OK          1  /* ip_rcv hands the packet to icmpv4_incoming/tcp_in */
#define LVLIP_RX_NOT_IP      2  /* ethertype != 0x0800 (netdev_receive, src/netdev.c:67-80) */
#define LVLIP_RX_SHORT       3  /* frame shorter than 14 + 20, 14 + ihl*4, or (with
                                   VERIFY_L4) 14 + the IP total length; the
                                   reference has no such check (it would read past
                                   the frame) */
#define LVLIP_RX_BAD_VERSION 4  /* src/ip_input.c:22-25                          */
#define LVLIP_RX_BAD_IHL     5  /* src/ip_input.c:27-30                          */
#define LVLIP_RX_TTL0        6  /* src/ip_input.c:32-36                          */
#define LVLIP_RX_BAD_CSUM    7  /* checksum(ih, ihl*4, 0) != 0, src/ip_input.c:38-43 */
#define LVLIP_RX_BAD_L4      8  /* only with LVLIP_RX_VERIFY_L4                  */
#define LVLIP_RX_UNKNOWN_PROTO 9 /* not ICMP/TCP, src/ip_input.c:51-60         */

/* Also verify TCP (pseudo header, RFC arithmetic: the seed's carries are folded
 * back in) and ICMP checksums.  The reference never verifies them on RX
 * (src/tcp.c:79-81 is commented out, src/icmpv4.c:11 is a TODO), so this is off
 * by default. */
#define LVLIP_RX_VERIFY_L4   0x1u

/* Verdict per frame; frames are not modified.  Must run before ip_init_pkt's
 * in-place byte swaps (src/ip_input.c:47).  n <= LVLIP_MAX_BATCH / 2 (up to two
 * checksums per frame).  Returns 0 or LVLIP_E* (LVLIP_ERANGE: with
 * LVLIP_RX_VERIFY_L4, a frame longer than the context's arena).  A call of at
 * most the context's cpu_max frames runs on the calling thread
 * (lvlip_csum_ctx_set_cpu_max, include/lvlip_csum.h), with the same results. */
int lvlip_rx_verify(lvlip_csum_ctx *ctx, const lvlip_frame *frames, uint32_t n,
                    uint32_t flags, uint8_t *verdict);

/* Plan: verdict[] gets the header-field decisions, or 0 / 0x80|X = pending on
 * the checksums (X is the verdict if the header checksum passes);
 * iov[]/tag[] (capacity 2n) get the checksums to run, tag = frame << 1 | is_l4.
 * Returns the number of iov entries. */
uint32_t lvlip_rx_plan(const lvlip_frame *frames, uint32_t n, uint32_t flags,
                       uint8_t *verdict, lvlip_csum_iov *iov, uint32_t *tag);
/* Apply: BAD_CSUM if the header checksum fails, else BAD_L4 if an L4 one does,
 * else the deferred verdict (OK for 0). */
void lvlip_rx_apply(uint32_t n, uint8_t *verdict, uint32_t m, const uint32_t *tag,
                    const uint16_t *csum);

/* ---- f2: TX ------------------------------------------------------------ */

/* Frames fully built by tcp_transmit_skb / ip_output / icmpv4_reply except their
 * checksums.  Fills, stored raw as the reference stores them, the values the
 * reference computes with each field zeroed first (whatever the field holds):
 *   TCP  : checksum(tcp, ip.len - ihl*4, pseudo(saddr, daddr, 6, len))
 *          src/tcp_output.c:110,126 -> src/tcp.c:87-98 (u32 seed, carry lost);
 *          saddr/daddr are the header's network-order words, as
 *          tcp_transmit_skb passes htonl(sk->saddr), htonl(sk->daddr)
 *   ICMP : checksum(icmp, ip.len - ihl*4, 0), src/icmpv4.c:46-47
 *   IPv4 : checksum(ih, ihl*4, 0), src/ip_output.c:42,53 (ip_send_check)
 * The IPv4 header checksum does not cover the L4 bytes, so all 2n checksums
 * are one batch; n <= LVLIP_MAX_BATCH / 2.  Returns 0 or LVLIP_E* (frames
 * untouched on error): LVLIP_EINVAL for a malformed frame (not IPv4, ihl < 5,
 * shorter than 14 + its IP length), LVLIP_ERANGE for a frame longer than the
 * context's arena.  A call of at most the context's cpu_max frames runs on the
 * calling thread, with the same results and codes.
 * Each frame may be listed once per call.  A frame listed twice is
 * unsupported: its fields may be stored from two threads at once, and after a
 * failed call it need not get back the bytes it held before the call. */
int lvlip_tx_checksum(lvlip_csum_ctx *ctx, lvlip_frame *frames, uint32_t n);

/* Plan: fills iov[]/field[] (capacity 2n; field = where each result goes),
 * frames unmodified (each seed is compensated for its field's current value).
 * Returns the number of iov entries, or 0xFFFFFFFF if a frame is malformed. */
uint32_t lvlip_tx_plan(lvlip_frame *frames, uint32_t n, lvlip_csum_iov *iov,
                       uint8_t **field);
void lvlip_tx_apply(uint32_t m, uint8_t *const *field, const uint16_t *csum);

/* ---- f4: RFC 1624 incremental update for the echo reply ----------------- */

/* icmpv4_reply (src/icmpv4.c:44-47) turns an echo request into the reply by
 * setting type 8 -> 0 and recomputing the ICMP checksum over the whole
 * message.  Given the request's stored checksum field (raw u16, as loaded
 * from the frame) of a request whose ICMP checksum VERIFIED (checksum over
 * the message == 0, e.g. LVLIP_RX_OK from lvlip_rx_verify with
 * LVLIP_RX_VERIFY_L4), returns the reply's checksum field, bit-identical to
 * the reference's full recomputation, without reading the message; or
 * LVLIP_CSUM_RECOMPUTE in the one case the field cannot decide (the reply's
 * one's-complement sum is 0xffff, which is also what an all-zero reply
 * gives), where the caller recomputes with checksum(). */
#define LVLIP_CSUM_RECOMPUTE 0xFFFFFFFFu
uint32_t lvlip_icmp_echo_reply_csum(uint16_t req_csum);

/* In place over n verified echo-request frames: ICMP type 8 -> 0 and the
 * checksum field updated as above (recomputed with checksum() in the
 * undecidable case).  Returns the number of frames that needed the
 * recomputation, or 0xFFFFFFFF (frames untouched) if one is not an ICMP echo
 * request. */
uint32_t lvlip_icmp_echo_reply_fill(lvlip_frame *frames, uint32_t n);

/* ---- f1/f2 over level-ip's own skb queues -------------------------------- */

/* The same calls over an sk_buff_head (include/skbuff.h:25-29) as level-ip
 * fills it, walked in list order through the intrusive list_head at the start
 * of every sk_buff (include/list.h; LP64 offsets of include/skbuff.h:9-23:
 * len 40, end 56, head 64, data 72).  The queue is only read.
 *
 * RX: skbs as netdev_rx_loop allocates and fills them (src/netdev.c:86-101,
 * alloc_skb src/skbuff.c:5-20): the frame is skb->data .. skb->end (tun_read
 * writes it at skb->data; the rest of the BUFLEN buffer is zero).  verdict[k]
 * is the k-th skb's; cap is verdict's capacity.  Returns the number of skbs,
 * LVLIP_ERANGE if more than cap, or LVLIP_E*. */
struct sk_buff_head;
int lvlip_rx_verify_skb_list(lvlip_csum_ctx *ctx, struct sk_buff_head *q, uint32_t flags,
                             uint8_t *verdict, uint32_t cap);

/* TX: skbs as ip_output leaves them before dst_neigh_output
 * (src/ip_output.c:14-56): skb->data at the IPv4 header, skb->len covering it
 * and the TCP/ICMP segment, the Ethernet header's 14 bytes reserved in front
 * (the frame is skb->data - 14 .. skb->data + skb->len).  Fills the TCP/ICMP
 * and IPv4 checksums as lvlip_tx_checksum, i.e. what tcp_transmit_skb
 * (src/tcp_output.c:126), icmpv4_reply (src/icmpv4.c:47) and ip_send_check
 * (src/ip_output.c:53) would have stored.  Returns the number of skbs or
 * LVLIP_E* (skbs untouched on error). */
int lvlip_tx_checksum_skb_list(lvlip_csum_ctx *ctx, struct sk_buff_head *q);

/* ---- f1/f2 on the calling thread (no context, no GPU) --------------------- */

/* The same calls computed by the library's CPU code on the calling thread,
 * with the same results and return codes (LVLIP_EINVAL on a malformed frame,
 * frames untouched; no arena, so LVLIP_ERANGE only for an RX queue longer than
 * cap).  A context's calls of at
 * most its cpu_max frames run these (lvlip_csum_ctx_set_cpu_max,
 * include/lvlip_csum.h).  A caller that deferred its TX checksums also calls
 * them when the GPU call fails (LVLIP_ENODEV, LVLIP_EHIP, LVLIP_ENOMEM,
 * LVLIP_ERANGE; or no context could be made), so that no frame leaves with a
 * deferred, still-zero field (src/ip_output.c:53-55 sends
 * whatever the fields hold).  Reentrant; one checksum() per field, as the
 * reference's call sites. */
int lvlip_rx_verify_cpu(const lvlip_frame *frames, uint32_t n, uint32_t flags,
                        uint8_t *verdict);
int lvlip_tx_checksum_cpu(lvlip_frame *frames, uint32_t n);
int lvlip_rx_verify_skb_list_cpu(struct sk_buff_head *q, uint32_t flags,
                                 uint8_t *verdict, uint32_t cap);
int lvlip_tx_checksum_skb_list_cpu(struct sk_buff_head *q);

/* ---- f1/f2/f4 on device-resident frames ---------------------------------- */

/* Frames already in HBM (a receive ring filled by a GPU-direct NIC, or frames
 * built on the GPU): one frame = `len` bytes at base + offset, Ethernet header
 * first.  Parse, checksum and apply run as one kernel on the caller's stream;
 * nothing returns to the host.  Pointers are device pointers; `base` is 16-B
 * aligned and readable up to the last frame's end rounded up to 16 B.
 * `workspace` is reserved and may be NULL: lvlip_frames_workspace_bytes()
 * returns 0 (ABI 1 kept the argument from the earlier three-kernel form). */
typedef struct lvlip_frame_desc {
    uint64_t offset;
    uint32_t len;
    uint32_t reserved;  /* 0 */
} lvlip_frame_desc;

size_t lvlip_frames_workspace_bytes(uint32_t n);

/* verdict[i] as lvlip_rx_verify (same decisions, same flags). */
int lvlip_rx_verify_dev(const void *base, const lvlip_frame_desc *frames, uint32_t n,
                        uint32_t flags, uint8_t *verdict, void *workspace, void *stream);

/* Fills the TCP/ICMP and IPv4 checksums in place, as lvlip_tx_checksum.  A
 * malformed frame (not IPv4, short) is left untouched and gets status 0 (1 =
 * filled); status may be NULL. */
int lvlip_tx_checksum_dev(void *base, const lvlip_frame_desc *frames, uint32_t n,
                          uint8_t *status, void *workspace, void *stream);

/* f4 on frames in HBM: lvlip_icmp_echo_reply_fill in one launch, one lane per
 * frame.  Every frame that is an IPv4 ICMP echo request (type 8, code 0, the
 * message inside the frame) becomes the reply's ICMP part: type 0 and the
 * RFC 1624 checksum field derived from the request's field alone; in the one
 * undecidable case (LVLIP_CSUM_RECOMPUTE) the lane sums the message itself.
 * status[i] (may be NULL): 1 updated from the field, 2 recomputed, 0 not an
 * echo request (frame untouched).  Nothing else of the message is read.
 *
 * PRECONDITION: the request's ICMP checksum verified (e.g. the frame got
 * LVLIP_RX_OK from lvlip_rx_verify_dev with LVLIP_RX_VERIFY_L4).  Only then
 * is the field bit-identical to icmpv4_reply's full recomputation
 * (src/icmpv4.c:44-47).  The call does NOT check it: status 1 does not mean
 * the request verified, and for a request whose checksum is wrong the field
 * written differs from the reference's (which answers such requests with a
 * correct checksum, src/icmpv4.c:11 never verifies).  For frames nobody
 * verified, use lvlip_icmp_echo_reply_dev_ex with LVLIP_ECHO_FULL. */
int lvlip_icmp_echo_reply_dev(void *base, const lvlip_frame_desc *frames, uint32_t n,
                              uint8_t *status, void *stream);

/* flags of lvlip_icmp_echo_reply_dev_ex */
#define LVLIP_ECHO_FULL 0x1u /* sum every request's message (one lane per frame)
                                and write icmpv4_reply's field exactly: for
                                any request, verified or not; status 2.  Costs
                                a full read of each message by its one lane
                                (serial 16-B loads), where flags 0 reads one
                                64-B sector per frame (DESIGN.md §9 times
                                both) */

/* lvlip_icmp_echo_reply_dev with flags: 0 is lvlip_icmp_echo_reply_dev (the
 * precondition above holds); LVLIP_ECHO_FULL computes the reply's field as
 * icmpv4_reply does, from the whole message with type and field zeroed
 * (src/icmpv4.c:45-47), bit-identical for every echo request.  Other flag bits
 * are LVLIP_EINVAL. */
int lvlip_icmp_echo_reply_dev_ex(void *base, const lvlip_frame_desc *frames, uint32_t n,
                                 uint32_t flags, uint8_t *status, void *stream);

/* ---- f2 on the device: segmentation ---------------------------------------- */

/* tcp_send (src/tcp_output.c:445-478) cuts one write into ceil(len/mss)
 * segments that differ only in seq, IP length, PSH, the two checksums and the
 * payload slice.  For payload that already lives in HBM these calls do the
 * same from one 54-byte header template, as a NIC's TSO does: payload copy and
 * TCP checksum in one pass, finished Ethernet/IPv4/TCP frames out.
 *
 * A send is a payload range, an MSS and a template in network order: Ethernet
 * 14 B, IPv4 with ihl 5, TCP with hl 5 (no options), holding the fields the
 * first segment would carry; its IP length and both checksum fields are
 * ignored.  Segment i of nseg = ceil(len/mss) carries dlen_i = min(mss,
 * len - i*mss) payload bytes and is the 54 + dlen_i bytes at
 * out + out_off + i*stride:
 *   Ethernet  the template's 14 bytes
 *   IPv4      the template, total length htons(40 + dlen_i), id as given (the
 *             reference never advances it, src/ip_output.c:36), header
 *             checksum checksum(ih, 20, 0) stored raw (src/ip_output.c:42,53)
 *   TCP       the template, seq = htonl(seq0 + i*mss) mod 2^32; PSH and FIN of
 *             the template on the last segment only (src/tcp_output.c:466);
 *             csum = checksum(tcp, 20 + dlen_i, saddr + daddr + htons(6) +
 *             htons(20 + dlen_i)) stored raw, the seed a u32 that wraps
 *             (src/tcp.c:87-98: the carry is lost)
 *   payload   bytes [i*mss, i*mss + dlen_i) of the send
 * and, when fd is given, fd[seg0 + i] = {out_off + i*stride, 54 + dlen_i, 0},
 * which the other _dev calls take as it is.  Nothing outside the frames is
 * written (stride gaps keep their bytes); the payload is only read. */
typedef struct lvlip_tso_send {
    uint64_t payload_off;   /* from the payload base; any alignment            */
    uint64_t out_off;       /* first frame, from the out base; any alignment   */
    uint32_t len;           /* payload bytes, > 0                              */
    uint32_t seg0;          /* index of this send's first segment in the call  */
    uint32_t stride;        /* >= 54 + mss; any value                          */
    uint16_t mss;           /* 1 .. 65495                                      */
    uint16_t reserved;      /* 0                                               */
    uint8_t  hdr[54];
    uint8_t  pad[10];       /* 0; sizeof == 96                                 */
} lvlip_tso_send;

/* Host only: validates every send, fills seg0 with the running segment count
 * and returns the total segment count (nseg of lvlip_tso_dev), or 0xFFFFFFFF
 * for a malformed send (len or mss 0, mss > 65495, stride < 54 + mss, reserved
 * != 0, ethertype != 0x0800, version/ihl != 0x45, protocol != 6, TCP header
 * length != 5) or a total above LVLIP_MAX_BATCH.  *out_bytes (may be NULL) gets
 * the largest out_off + (nseg-1)*stride + 54 + dlen_last: the bytes `out` must
 * hold.  out_off is the caller's; the plan lays nothing out. */
uint32_t lvlip_tso_plan(lvlip_tso_send *s, uint32_t n, uint64_t *out_bytes);

/* The frames on the calling thread, one checksum() per field (the library's
 * CPU code).  s as lvlip_tso_plan left it.  Returns 0, or LVLIP_EINVAL (NULL
 * pointers with n > 0, a malformed or unplanned send) with nothing written.
 * Reentrant; fd may be NULL. */
int lvlip_tso_cpu(const void *payload, const lvlip_tso_send *s, uint32_t n, void *out,
                  lvlip_frame_desc *fd);

/* The same frames, bit for bit, in one launch on the caller's stream
 * (asynchronous; no allocation, copy or synchronisation).  All pointers are
 * device pointers, of any alignment for payload and out (s: 8 B, fd: 16 B);
 * s as lvlip_tso_plan left it, nseg what it returned.  n == 0 is a no-op;
 * NULL payload, s or out with n > 0, or nseg 0 or above LVLIP_MAX_BATCH, is
 * LVLIP_EINVAL before any HIP call; LVLIP_ENODEV without a device; a failed
 * launch is LVLIP_EHIP (lvlip_last_hip_error).  The device does not validate
 * the templates again: the caller planned the sends. */
int lvlip_tso_dev(const void *payload, const lvlip_tso_send *s, uint32_t n, uint32_t nseg,
                  void *out, lvlip_frame_desc *fd, void *stream);

/* ---- f1 on the device: receive coalescing ----------------------------------- */

/* The receive half of the data path: tcp_in sets seq, dlen and payload per skb
 * (src/tcp.c:46-50), tcp_data_queue orders the skbs (src/tcp_data.c:87-128)
 * and tcp_data_dequeue copies them out one memcpy at a time (:49-85).  For a
 * receive ring that already lives in HBM these calls do the same per batch, as
 * a NIC's LRO/GRO does: every frame is parsed as ip_rcv and tcp_in parse it,
 * matched to a flow, and its payload lands where the byte stream wants it, at
 * out + out_off + (seq - rcv_nxt).  One record per frame tells the host what
 * happened; lvlip_lro_advance turns the records into the new rcv_nxt and the
 * SACK blocks.  The state machine (SYN, RST, URG) stays on the host: such
 * frames are reported, not interpreted.  The ACK side of the records is
 * lvlip_snd_* below ("the ACK side and the retransmit").
 *
 * Status of a frame.  2-9 are LVLIP_RX_NOT_IP .. LVLIP_RX_UNKNOWN_PROTO with
 * the meaning and precedence lvlip_rx_verify_dev gives them for the same flags
 * (LVLIP_RX_BAD_L4 only with LVLIP_RX_VERIFY_L4).  A frame ip_rcv would keep
 * gets the lowest of the values below that applies:
 *   NOT_TCP        ICMP
 *   BAD_TCP_HDR    hl < 5 or hl*4 > ip.len - ihl*4; also, without
 *                  LVLIP_RX_VERIFY_L4 (which calls them LVLIP_RX_SHORT), an
 *                  ip.len below ihl*4 or beyond the frame: the segment the
 *                  header describes is not in the frame
 *   NO_FLOW        no planned flow has the frame's addresses and ports
 *   CONTROL        SYN, RST or URG set: left to the state machine
 *   NO_DATA        dlen == 0 (a pure ACK, a bare FIN); rel and ack_seq are valid
 *   OUT_OF_WINDOW  rel + dlen > rcv_wnd in 64-bit arithmetic
 *   PLACED         the dlen payload bytes are at out + out_off + rel.  FIN with
 *                  data is placed; FIN is in tcp_flags, where lvlip_fin_*
 *                  ("the end of a connection") reads it.
 * IPv4 and TCP options are accepted and skipped.
 *
 * The bytes of `out`.  After the call the dlen bytes at out + out_off + rel
 * hold the payload of every PLACED frame; where two PLACED frames of a flow
 * overlap with different bytes the result is either frame's byte (TCP requires
 * them equal).  Every other byte of `out` is untouched.  With
 * LVLIP_RX_VERIFY_L4 no byte of a frame is stored before that frame's verdict
 * is known: a BAD_L4 frame never damages a good one it overlaps.
 *
 * Departures from the reference:
 *   - the window test is mod 2^32 (rel = seq - rcv_nxt); tcp_verify_segment
 *     (src/tcp_input.c:106-107) compares plain u32 values and breaks when
 *     rcv_nxt + rcv_wnd wraps;
 *   - a segment must END inside the window (the reference checks its start
 *     only; the out buffer needs the bound);
 *   - partially overlapping segments are united (src/tcp_data.c:16 is a TODO).
 * For segments that share boundaries, in any arrival order and with
 * duplicates, out[out_off .. out_off + delivered) is what tcp_data_dequeue
 * returns and rcv_nxt + delivered what tcp_data_queue leaves in rcv_nxt. */
#define LVLIP_LRO_PLACED        1
#define LVLIP_LRO_NOT_TCP       16
#define LVLIP_LRO_BAD_TCP_HDR   17
#define LVLIP_LRO_NO_FLOW       18
#define LVLIP_LRO_CONTROL       19
#define LVLIP_LRO_NO_DATA       20
#define LVLIP_LRO_OUT_OF_WINDOW 21
#define LVLIP_LRO_MAX_FLOWS     65536u
#define LVLIP_LRO_MAX_WND       0x40000000u

typedef struct lvlip_lro_flow {      /* one connection's receive side; sizeof == 48 */
    uint32_t saddr, daddr;           /* the words of the frame's IPv4 header (network order) */
    uint16_t sport, dport;           /* as in the TCP header (network order) */
    uint32_t rcv_nxt;                /* host order: the first stream byte wanted */
    uint32_t rcv_wnd;                /* bytes of window = bytes of `out` this flow owns; 1 .. 2^30 */
    uint32_t reserved;               /* 0 */
    uint64_t out_off;                /* where stream byte rcv_nxt lands, from the out base; any alignment */
    uint64_t user;                   /* the caller's cookie; the plan reorders flows */
    uint8_t  pad[8];                 /* 0 */
} lvlip_lro_flow;

typedef struct lvlip_lro_rec {       /* one per frame; sizeof == 16, one vector store */
    uint32_t flow;                   /* index into the planned flows, 0xFFFFFFFF if none */
    uint32_t rel;                    /* (seq - rcv_nxt) mod 2^32; the raw seq for NO_FLOW */
    uint16_t dlen;                   /* ip.len - ihl*4 - hl*4, src/tcp.c:47 */
    uint8_t  status;
    uint8_t  tcp_flags;              /* byte 13 of the TCP header */
    uint32_t ack_seq;                /* host order */
} lvlip_lro_rec;                     /* status below NO_FLOW: flow 0xFFFFFFFF, the rest 0 */

typedef struct lvlip_lro_sack {
    uint32_t left, right;            /* host-order seq numbers, [left, right) */
} lvlip_lro_sack;

typedef struct lvlip_lro_result {    /* one per planned flow; sizeof == 48 */
    uint32_t delivered;              /* contiguous bytes from rel 0: what tcp_data_queue and
                                        tcp_consume_ofo_queue add to rcv_nxt */
    uint32_t placed;                 /* PLACED frames of the flow */
    uint32_t nsack;                  /* islands reported below, 0 .. 4 */
    uint32_t reserved;               /* 0 */
    lvlip_lro_sack sack[4];          /* the first islands beyond the prefix in ascending rel, as
                                        tcp_calculate_sacks walks the ofo queue (src/tcp.c:470-481) */
} lvlip_lro_result;

/* Host only: validates the flows and sorts them in place by their 12 key
 * bytes (saddr, daddr, sport, dport) in memcmp order, which is what the
 * lookup searches.  Returns n, or 0xFFFFFFFF for a duplicate key, rcv_wnd 0 or
 * above 2^30, nonzero reserved or pad, two flows whose [out_off, out_off +
 * rcv_wnd) overlap, n above LVLIP_LRO_MAX_FLOWS, or no memory for the overlap
 * check.  *out_bytes (may be NULL) gets the largest out_off + rcv_wnd: the
 * bytes `out` must hold. */
uint32_t lvlip_lro_plan(lvlip_lro_flow *f, uint32_t n, uint64_t *out_bytes);

/* The batch on the calling thread with the library's CPU checksum.  fd[i]
 * describes frame i inside base, f as lvlip_lro_plan left it; flags 0 or
 * LVLIP_RX_VERIFY_L4.  Returns 0, or LVLIP_EINVAL (NULL base, fd, out or rec
 * with n > 0, NULL f with nflows > 0, n above LVLIP_MAX_BATCH, nflows above
 * LVLIP_LRO_MAX_FLOWS, other flag bits, flows not in plan order) with nothing
 * written.  nflows == 0 is legal: every TCP frame gets NO_FLOW.  Reentrant. */
int lvlip_lro_cpu(const void *base, const lvlip_frame_desc *fd, uint32_t n, const lvlip_lro_flow *f,
                  uint32_t nflows, uint32_t flags, void *out, lvlip_lro_rec *rec);

/* The same records and bytes in one launch on the caller's stream
 * (asynchronous; no allocation, copy or synchronisation).  All pointers are
 * device pointers; base as for lvlip_rx_verify_dev (16-B aligned, readable up
 * to the last frame's end rounded up to 16 B), fd and rec 16-B aligned, f 8-B
 * aligned, out any alignment.  n == 0 is a no-op; the refusals of
 * lvlip_lro_cpu are LVLIP_EINVAL before any HIP call, except the flows' order,
 * which the device does not check: the caller planned them.  LVLIP_ENODEV
 * without a device; a failed launch is LVLIP_EHIP (lvlip_last_hip_error). */
int lvlip_lro_dev(const void *base, const lvlip_frame_desc *fd, uint32_t n, const lvlip_lro_flow *f,
                  uint32_t nflows, uint32_t flags, void *out, lvlip_lro_rec *rec, void *stream);

/* Host only: per flow, the union of the PLACED records' [rel, rel + dlen)
 * (records of other statuses are ignored) -> res[k] for flow k.  Returns 0,
 * LVLIP_EINVAL (NULL f or res with nflows > 0, NULL rec with n > 0) or
 * LVLIP_ENOMEM if its scratch allocation fails. */
int lvlip_lro_advance(const lvlip_lro_flow *f, uint32_t nflows, const lvlip_lro_rec *rec, uint32_t n,
                      lvlip_lro_result *res);

/* Bytes of device workspace lvlip_lro_advance_dev needs for n records and
 * nflows flows (20 n and a little: the sort's keys and lengths twice, a bit per
 * record, the sort's own storage).  Returns 0 for n == 0 or above
 * LVLIP_MAX_BATCH.  May initialise the HIP runtime (the sort's size query asks
 * for the device's architecture); returns 0 when there is no device. */
size_t lvlip_lro_advance_workspace_bytes(uint32_t n, uint32_t nflows);

/* lvlip_lro_advance on the device: res[k] for every planned flow k, all 48
 * bytes of each result equal to the host form's, for ANY record array, not only
 * one lvlip_lro_dev wrote: a record counts when its status is PLACED and its
 * flow is below nflows, whatever its rel and dlen.  f, rec, res and workspace
 * are device pointers (f 8-B, rec and res 16-B, workspace 256-B aligned).
 * Asynchronous on `stream` (a key per record, rocPRIM's radix sort, a scan, one
 * wave per flow): no allocation, no device-to-host copy, no synchronisation.
 * rec and f are only read; the results do not depend on the run.
 * nflows == 0 is a no-op; n == 0 zeroes res on the stream and needs no
 * workspace.  LVLIP_EINVAL before any HIP call: NULL f or res with nflows > 0,
 * NULL rec with n > 0, n above LVLIP_MAX_BATCH, nflows above
 * LVLIP_LRO_MAX_FLOWS, a misaligned f, rec or res, and with n > 0 and
 * nflows > 0 a NULL or misaligned workspace.  workspace_bytes below
 * lvlip_lro_advance_workspace_bytes(n, nflows) is LVLIP_ERANGE with nothing
 * written; LVLIP_ENODEV without a device; a failed launch is LVLIP_EHIP
 * (lvlip_last_hip_error).
 * Measured: 1M records in 0.22-0.28 ms, against roughly 25 ms
 * (in order) to 110 ms (shuffled) for copying them to the host and
 * lvlip_lro_advance there.  The call costs about 30 us however small the batch
 * (its launches): at 256 records that is what the host path takes too, one
 * ahead on one machine and the other on the next; from 4096 records on this
 * call is several times faster.  The library does not choose: a caller with
 * small batches that may leave the stream loses nothing with the host form. */
int lvlip_lro_advance_dev(const lvlip_lro_flow *f, uint32_t nflows, const lvlip_lro_rec *rec, uint32_t n,
                          lvlip_lro_result *res, void *workspace, size_t workspace_bytes, void *stream);

/* ---- f1 on the device: state across batches --------------------------------- */

/* The calls above work on one batch.  These carry a connection over to the
 * next one, so that a transfer of many rounds runs with record arrays of one
 * round's size and, on the device, with no host step between rounds:
 *   lvlip_lro_* -> lvlip_lro_advance_carry* (prev = the results of the round
 *   before) -> lvlip_ack_* -> lvlip_lro_next_*, and on the sender
 *   lvlip_snd_* -> lvlip_sack_* / lvlip_rtx* -> lvlip_snd_next_*.
 *
 * lvlip_lro_advance_carry is lvlip_lro_advance with one more source of
 * intervals.  prev[k] is the result an earlier call left for flow k; its
 * sack[] holds absolute sequence numbers, so it survives a change of rcv_nxt.
 *
 * Carried blocks.  For flow k and j < min(prev[k].nsack, 4), against f[k] as it
 * is AT THE CALL: l = (sack[j].left - f[k].rcv_nxt) mod 2^32, r =
 * (sack[j].right - f[k].rcv_nxt) mod 2^32.  The block counts when l < r <=
 * f[k].rcv_wnd and joins the flow's union as [l, r).  A block that is stale
 * (behind rcv_nxt), empty, straddling rcv_nxt or ending beyond the window is
 * ignored, and so is every other field of prev: a crafted prev (nsack 7, any
 * edges) changes values, never an address.
 *
 * Results.  delivered, nsack and sack[] describe the union of the PLACED
 * records and the carried blocks; placed counts records only.  A flow with a
 * carry and no record still gets its islands.  With n == 0 and a prev the call
 * is not a zero fill: the results are the union of the carried blocks.  With
 * prev == NULL all 48 bytes of every result equal lvlip_lro_advance's, for any
 * record array.  prev == res is allowed (in place).
 *
 * What is remembered.  The carry is the four islands a result reports.  A
 * fifth island of a flow is FORGOTTEN from one call to the next: its bytes stay
 * in `out`, nothing accounts for them, and the peer sends them again (they were
 * never the subject of a SACK block, and RFC 2018 section 8 lets a receiver
 * renege in any case).  Within one call any number of islands is united as
 * before.
 *
 * lvlip_lro_advance_carry: host only.  Returns as lvlip_lro_advance; prev may
 * be NULL.  Reentrant. */
int lvlip_lro_advance_carry(const lvlip_lro_flow *f, uint32_t nflows, const lvlip_lro_rec *rec, uint32_t n,
                            const lvlip_lro_result *prev, lvlip_lro_result *res);

/* Bytes of device workspace lvlip_lro_advance_carry_dev needs: what
 * lvlip_lro_advance_dev's needs, for n + 4 nflows elements with 4-B lengths,
 * and 4 bytes per flow (24 (n + 4 nflows) and a little), and never less than
 * lvlip_lro_advance_workspace_bytes(n, nflows).  Unlike that call it is not 0
 * for n == 0: the carried blocks are elements too.  Returns 0 for nflows == 0
 * or above LVLIP_LRO_MAX_FLOWS, for n + 4 nflows above LVLIP_MAX_BATCH, and when
 * there is no device.  May initialise the HIP runtime. */
size_t lvlip_lro_advance_carry_workspace_bytes(uint32_t n, uint32_t nflows);

/* lvlip_lro_advance_carry on the device, every byte of res equal to the host
 * form's: lvlip_lro_advance_dev's pipeline over n + 4 nflows elements, the key
 * step also turning block j of prev[k] into element n + 4 k + j, with 4-B
 * lengths through the sort and the scans (a carried block is up to 2^30 bytes
 * long).  Asynchronous on `stream`: no allocation, no device-to-host copy, no
 * synchronisation; rec and f are only read, and so is prev unless it is res.
 * Pointers and alignments as for lvlip_lro_advance_dev, prev 16-B aligned.
 * nflows == 0 is a no-op.  LVLIP_EINVAL before any HIP call: the refusals of
 * lvlip_lro_advance_dev, a misaligned prev, n + 4 nflows above LVLIP_MAX_BATCH
 * (the elements are indexed in 32 bits), and with nflows > 0 and either n > 0
 * or a prev, a NULL or misaligned workspace.  workspace_bytes below
 * lvlip_lro_advance_carry_workspace_bytes(n, nflows) is LVLIP_ERANGE with
 * nothing written; LVLIP_ENODEV without a device; a failed launch is LVLIP_EHIP
 * (lvlip_last_hip_error).
 * With prev == NULL the call IS lvlip_lro_advance_dev (the same launches with
 * 2-B lengths, inside the workspace given), so a caller without a carry loses
 * nothing by calling either form; it still needs this form's workspace size.
 * Measured: DESIGN.md section 9h. */
int lvlip_lro_advance_carry_dev(const lvlip_lro_flow *f, uint32_t nflows, const lvlip_lro_rec *rec, uint32_t n,
                                const lvlip_lro_result *prev, lvlip_lro_result *res,
                                void *workspace, size_t workspace_bytes, void *stream);

/* Move the receive side on.  For every flow k: d = min(res[k].delivered,
 * f[k].rcv_wnd); f[k].rcv_nxt += d mod 2^32, f[k].out_off += d, f[k].rcv_wnd -=
 * d; then res[k].delivered = 0.  sack[], nsack and placed stay: they are the
 * next lvlip_lro_advance_carry* call's prev.  The call consumes the result, so
 * applying it twice changes nothing, and lvlip_ack_* or lvlip_rtx* run after it
 * build the frames they would have built before it (rcv_nxt + delivered is the
 * same number).  Keys, the plan's order and the disjointness of the flows' out
 * ranges are preserved: a range only shrinks from its front.
 * rcv_wnd may reach 0.  Such a flow places nothing more (every data frame is
 * OUT_OF_WINDOW, a pure ACK NO_DATA) until the caller gives it a fresh region
 * and plans again; only lvlip_lro_plan refuses a window of 0, the batch calls
 * take it.
 * Only f[k] and res[k] are written.  nflows == 0 is a no-op.  LVLIP_EINVAL: NULL
 * f or res, nflows above LVLIP_LRO_MAX_FLOWS.  _cpu: on the calling thread,
 * reentrant.  _dev: one launch on the caller's stream, a lane per flow
 * (asynchronous; no allocation, copy, workspace or synchronisation); f 8-B and
 * res 16-B aligned device pointers, a misaligned one is LVLIP_EINVAL before any
 * HIP call; LVLIP_ENODEV without a device; a failed launch is LVLIP_EHIP. */
int lvlip_lro_next_cpu(lvlip_lro_flow *f, lvlip_lro_result *res, uint32_t nflows);
int lvlip_lro_next_dev(lvlip_lro_flow *f, lvlip_lro_result *res, uint32_t nflows, void *stream);

/* ---- f1 on the device: the acknowledgement --------------------------------- */

/* What follows the advance step in the reference's receive path is
 * tcp_send_ack (src/tcp_output.c:247-267) -> tcp_transmit_skb (:93-129) ->
 * ip_output (src/ip_output.c:14-56): one pure ACK per connection, with the
 * SACK option tcp_write_options writes (src/tcp_output.c:65-91), the only TCP
 * option the reference writes outside a SYN.  These calls build that frame
 * per planned flow from a 54-byte header template and the flow's
 * lvlip_lro_result, so that lvlip_lro_dev -> lvlip_lro_advance_dev ->
 * lvlip_ack_dev turns frames in HBM into stream bytes and ACK frames in HBM on
 * one stream, with no host step.
 *
 * The frame of flow k.  b = min(res[k].nsack, t[k].max_sack, 4) (the clamp
 * holds for a res no library call wrote), optlen = b ? 4 + 8 b : 0; the frame
 * is the 54 + optlen bytes at out + t[k].out_off:
 *   Ethernet  the template's 14 bytes
 *   IPv4      the template, total length htons(40 + optlen), header checksum
 *             checksum(ih, 20, 0) with the field zeroed first, stored raw
 *             (src/ip_output.c:42,53)
 *   TCP       the template, ack_seq = htonl(f[k].rcv_nxt + res[k].delivered)
 *             mod 2^32 (src/tcp_output.c:107); the data offset nibble
 *             5 + optlen/4 (:261), the low nibble of that byte as the template
 *             has it; when b > 0 the option bytes 01 01 05 (2 + 8 b), then the
 *             blocks sack[b-1], ..., sack[0], each htonl(left), htonl(right):
 *             DESCENDING, as tcp_write_options walks i = sacklen-1 .. 0
 *             (src/tcp_output.c:78-86); csum = checksum(tcp, 20 + optlen,
 *             saddr + daddr + htons(6) + htons(20 + optlen)) stored raw, the
 *             seed a u32 that wraps (src/tcp.c:87-98: the carry is lost, as in
 *             lvlip_pseudo_sum and lvlip_tso_dev)
 * and, when fd is given, fd[k] = {t[k].out_off, 54 + optlen, 0}, which the
 * other _dev calls take as it is.  Without LVLIP_ACK_ALL a flow with
 * res[k].placed == 0 gets no ACK: no byte of `out` is written for it and
 * fd[k] = {t[k].out_off, 0, 0}.  Nothing outside the frames is written (the
 * rest of a 90-byte slot keeps its bytes); t, f and res are only read.
 *
 * Departure from the reference: tcp_write_options and tcp_options_len treat a
 * block whose left edge is sequence number 0 as absent
 * (src/tcp_output.c:69,234).  Here every one of the b blocks is written. */
#define LVLIP_ACK_MAX_FRAME 90u       /* 14 + 20 + 20 + 4 + 4*8 */
#define LVLIP_ACK_ALL       0x1u      /* flags: an ACK for every flow; 0 = only flows with res.placed > 0 */

typedef struct lvlip_ack_tmpl {       /* one per planned flow, index k = flow k in plan order; sizeof == 64 */
    uint64_t out_off;                 /* where the frame goes, from the out base; any alignment */
    uint8_t  hdr[54];                 /* Ethernet, IPv4 (ihl 5), TCP (hl 5), network order: what the stack's
                                         own next pure ACK of this connection would carry (seq = snd_nxt, win,
                                         flags, id, addresses, ports); IP length, ack_seq, data offset and both
                                         checksum fields are ignored */
    uint8_t  max_sack;                /* tsk->sacks_allowed: 0 (SACK not negotiated) .. 4 */
    uint8_t  reserved;                /* 0 */
} lvlip_ack_tmpl;

/* Host only: validates the templates against the planned flows.  Returns
 * nflows, or 0xFFFFFFFF for a template whose ethertype is not 0x0800, whose
 * version/ihl is not 0x45, whose protocol is not 6 or whose TCP header length
 * is not 5; max_sack above 4; nonzero reserved; a template that is not the
 * reverse of its flow (hdr.saddr == f.daddr, hdr.daddr == f.saddr, hdr.sport
 * == f.dport and hdr.dport == f.sport must all hold: lvlip_lro_plan reorders
 * flows, and this catches templates left in the old order); two slots
 * [out_off, out_off + 90) that overlap; nflows above LVLIP_LRO_MAX_FLOWS; or no
 * memory for the overlap check.  *out_bytes (may be NULL) gets the largest
 * out_off + 90: the bytes `out` must hold.  Nothing is modified. */
uint32_t lvlip_ack_plan(const lvlip_ack_tmpl *t, const lvlip_lro_flow *f, uint32_t nflows, uint64_t *out_bytes);

/* The frames on the calling thread, one checksum() per field (the library's
 * CPU code).  Returns 0, or LVLIP_EINVAL (NULL t, f, res or out with
 * nflows > 0, flag bits other than LVLIP_ACK_ALL, nflows above
 * LVLIP_LRO_MAX_FLOWS) with nothing written.  nflows == 0 is a no-op.
 * Reentrant; fd may be NULL. */
int lvlip_ack_cpu(const lvlip_ack_tmpl *t, const lvlip_lro_flow *f, const lvlip_lro_result *res,
                  uint32_t nflows, uint32_t flags, void *out, lvlip_frame_desc *fd);

/* The same frames and fd, bit for bit, in one launch on the caller's stream
 * (asynchronous; no allocation, copy, workspace, atomics or synchronisation).
 * All pointers are device pointers: t and f 8-B aligned, res and fd 16-B
 * aligned, out any alignment; res as lvlip_lro_advance_dev left it on the same
 * stream, or any other.  The refusals of lvlip_ack_cpu, and a misaligned t,
 * f, res or fd, are LVLIP_EINVAL before any HIP call; LVLIP_ENODEV without a
 * device; a failed launch is LVLIP_EHIP (lvlip_last_hip_error).  The device
 * does not validate the templates again: the caller planned them.  Measured:
 * DESIGN.md §9d. */
int lvlip_ack_dev(const lvlip_ack_tmpl *t, const lvlip_lro_flow *f, const lvlip_lro_result *res,
                  uint32_t nflows, uint32_t flags, void *out, lvlip_frame_desc *fd, void *stream);

/* ---- f2 on the device: the ACK side and the retransmit ---------------------- */

/* The sender's half of the loop.  The frames lvlip_tso_dev left in a TX ring
 * are the connection's write queue; the ACK frames the peer's lvlip_ack_dev
 * built come back through a second, reverse-direction lvlip_lro_* plan as
 * records whose ack_seq nothing above consumes.  These calls consume it:
 * lvlip_snd_* is the fifth check of tcp_input_state ("check the ACK field",
 * src/tcp_input.c:311-356) with tcp_clean_rto_queue (:66-92) over a whole
 * batch of records, and lvlip_rtx_* sends the head of the queue again as
 * tcp_retransmission_timeout (src/tcp_output.c:359-381) and tcp_send_next
 * (:198-225) do: skb_reset_header, then tcp_transmit_skb (:93-129), which
 * writes the current rcv_nxt and window into the same segment and computes the
 * TCP checksum afresh over all of it.  With them lvlip_tso_dev -> wire ->
 * lvlip_lro_dev -> lvlip_lro_advance_dev -> lvlip_ack_dev -> wire -> reverse
 * lvlip_lro_dev -> lvlip_snd_dev -> lvlip_rtx_dev runs a transfer with loss
 * and recovery on one stream.  SYN, RST and URG stay on the host (CONTROL).
 *
 * The write queue of flow k is the frames fd[s[k].seg0 .. s[k].seg0 +
 * s[k].nseg) of a TX ring, frame i at base + fd[i].offset, in queue order:
 * what lvlip_tso_dev leaves in `out` and `fd` (Ethernet, IPv4 with ihl 5, TCP).
 * s[k] belongs to planned LRO flow k (of the REVERSE plan: the one that parses
 * the peer's ACKs), as lvlip_ack_tmpl k does.
 *
 * Which records carry an ACK.  A record counts for flow k = rec.flow (below
 * nflows) when its status is PLACED, NO_DATA or OUT_OF_WINDOW, tcp_flags & 0x10
 * is set and rel <= f[k].rcv_wnd: tcp_verify_segment (src/tcp_input.c:100-113)
 * taken mod 2^32, which tests only the START of a segment, so a segment that
 * starts inside the window and ends beyond it (OUT_OF_WINDOW) still has its
 * ACK field read.  SYN and RST are CONTROL already (second and fourth check).
 *
 * The classes.  d = (ack_seq - s[k].snd_una) mod 2^32, span = (s[k].snd_nxt -
 * s[k].snd_una) mod 2^32, both against snd_una AT CALL ENTRY:
 *   new       1 <= d <= span     src/tcp_input.c:330
 *   duplicate d == 0             (falls through every test there)
 *   old       d >= 2^31          :338
 *   beyond    anything else      :343
 *
 * The result of flow k, 32 bytes, all defined:
 *   acked     the largest d among the records classed new (0 if none)
 *   snd_una   s[k].snd_una + acked mod 2^32
 *   n_new, n_dup, n_old, n_beyond   the class counts
 *   popped    the length of the leading run of queue frames with
 *             (end_seq - s[k].snd_una) mod 2^32 <= acked, where end_seq = seq +
 *             ip.len - ihl*4 - hl*4 mod 2^32 read from the frame in the ring
 *             (seq at byte 38, ip.len at 16, ihl in byte 14, hl in byte 46):
 *             the while loop of tcp_clean_rto_queue, which stops at the first
 *             frame that is not fully acknowledged.  A queue entry whose fd.len
 *             is below 54 ends the run.  Only the 54 header bytes are read.
 *   inflight  s[k].nseg - popped
 * The state is carried on by lvlip_snd_next_* below (snd_una = res.snd_una,
 * seg0 += popped, nseg -= popped), or by the caller.
 *
 * Equivalence.  snd_una is monotone in the reference (:330-331 only ever
 * raises it), so the final snd_una and the frames popped are what its
 * frame-by-frame processing leaves, in whatever order the records arrived.
 * Departures:
 *   - the classes are counted against the entry value of snd_una, not the
 *     running one (src/tcp_input.c:330,338 read tcb->snd_una as the frames
 *     before left it: there a second copy of a new ACK is a duplicate, here it
 *     is new twice);
 *   - the comparisons are mod 2^32; :330,338,343 and :73 compare plain u32
 *     values and break when snd_una..snd_nxt wraps;
 *   - tcp_clean_rto_queue's `skb->seq > 0` (:73) is dropped: a segment whose
 *     sequence number is 0 is popped like any other;
 *   - the reference frees a data segment whose ACK is old or beyond
 *     (:338-350, return_tcp_drop) before tcp_data_queue sees it.  lvlip_lro_*
 *     has already placed it; this call does not undo that. */
typedef struct lvlip_snd_flow {       /* one per planned flow, index k = flow k in plan order; sizeof == 32 */
    uint32_t snd_una, snd_nxt;        /* host order; (snd_nxt - snd_una) mod 2^32 <= 2^30 */
    uint32_t seg0, nseg;              /* the write queue: fd[seg0 .. seg0 + nseg) */
    uint32_t slot0;                   /* filled by the plan: the flow's first retransmit slot */
    uint32_t rtx;                     /* frames from the head of the queue a retransmit call may send */
    uint16_t win;                     /* host order: the window to advertise (tcb->rcv_wnd) */
    uint16_t reserved;                /* 0 */
    uint32_t reserved2;               /* 0 */
} lvlip_snd_flow;

typedef struct lvlip_snd_result {     /* one per planned flow; sizeof == 32 */
    uint32_t snd_una, acked;
    uint32_t n_new, n_dup, n_old, n_beyond;
    uint32_t popped, inflight;
} lvlip_snd_result;

/* Host only: validates the flows' send sides and fills slot0 with the running
 * sum of rtx; nothing else is modified.  Returns the total slot count (nslots
 * of lvlip_rtx_*), or 0xFFFFFFFF for nonzero reserved bytes, (snd_nxt -
 * snd_una) mod 2^32 above 2^30, a queue whose seg0 + nseg passes 2^32, queues
 * of two flows that overlap in the fd index space (empty queues overlap
 * nothing), a total of nseg or of rtx above LVLIP_MAX_BATCH, nflows above
 * LVLIP_LRO_MAX_FLOWS, or no memory for the overlap check.  *nfd (may be NULL)
 * gets the largest seg0 + nseg: the entries fd must hold. */
uint32_t lvlip_snd_plan(lvlip_snd_flow *s, uint32_t nflows, uint32_t *nfd);

/* The ACK side of one lvlip_lro_* call's records on the calling thread.  f the
 * planned flows, s as lvlip_snd_plan left it, base and fd the TX ring; only
 * res is written.  Returns 0, or LVLIP_EINVAL (NULL f, s, base, fd or res with
 * nflows > 0 and n > 0, NULL rec with n > 0, n above LVLIP_MAX_BATCH, nflows
 * above LVLIP_LRO_MAX_FLOWS) with nothing written.  nflows == 0 and n == 0 are
 * no-ops: without a record there is nothing to report, and res keeps its
 * bytes.  Reentrant. */
int lvlip_snd_cpu(const lvlip_lro_flow *f, const lvlip_snd_flow *s, uint32_t nflows, const lvlip_lro_rec *rec,
                  uint32_t n, const void *base, const lvlip_frame_desc *fd, lvlip_snd_result *res);

/* The same results, bit for bit, on the caller's stream (asynchronous; no
 * allocation, no device-to-host copy, no synchronisation, no workspace beyond
 * res): res is zeroed, every record adds to its flow's class count and raises
 * `acked` (atomic integer add and max, the only reductions, so the results do
 * not depend on the run; records of one flow are first reduced within their
 * wave, so a batch of one flow does not queue up on one address), and a wave
 * per flow scans the queue's headers.  All pointers are device pointers: f and
 * s 8-B aligned, rec, fd and res 16-B aligned, base any alignment; every frame
 * of a queue readable for its 54 header bytes.  The refusals of lvlip_snd_cpu,
 * and a misaligned f, s, rec, fd or res, are LVLIP_EINVAL before any HIP call;
 * LVLIP_ENODEV without a device; a failed launch is LVLIP_EHIP
 * (lvlip_last_hip_error).  The device does not validate s again: the caller
 * planned it.
 * Measured: 1M records in 0.09 ms over 1K flows and 0.15 ms
 * over 64K flows, against 2.2 ms and 13.7 ms for copying the records to the
 * host and lvlip_snd_cpu there: 24 and 94 times faster.  With every record of
 * one flow it is 0.38 to 0.41 ms. */
int lvlip_snd_dev(const lvlip_lro_flow *f, const lvlip_snd_flow *s, uint32_t nflows, const lvlip_lro_rec *rec,
                  uint32_t n, const void *base, const lvlip_frame_desc *fd, lvlip_snd_result *res, void *stream);

/* Move the send side on (the receive side's twin is lvlip_lro_next_*).  For
 * every flow k: p = min(res[k].popped, s[k].nseg); s[k].snd_una =
 * res[k].snd_una, s[k].seg0 += p, s[k].nseg -= p; then res[k].popped = 0,
 * res[k].acked = 0 and res[k].inflight = s[k].nseg.  The call consumes the
 * result, so applying it twice changes nothing, and lvlip_rtx* run after it
 * re-send the frames they would have re-sent before it (seg0 + popped is the
 * same entry).  slot0, rtx, win and snd_nxt stay, so the plan's nslots still
 * holds; the scoreboard is indexed like fd and needs nothing.  res must be one
 * a lvlip_snd_* call or this call wrote (its snd_una is taken as it is).  A
 * lvlip_snd_* call with n == 0 leaves res as it was; after this step that is
 * harmless, because the result is consumed.  Appending new writes to a queue
 * (snd_nxt, nseg, fresh fd entries) and giving popped entries back is
 * lvlip_push_* below ("the write queue").
 * Only s[k] and res[k] are written.  nflows == 0 is a no-op.  LVLIP_EINVAL: NULL
 * s or res, nflows above LVLIP_LRO_MAX_FLOWS.  _cpu: on the calling thread,
 * reentrant.  _dev: one launch on the caller's stream, a lane per flow
 * (asynchronous; no allocation, copy, workspace or synchronisation); s 8-B and
 * res 16-B aligned device pointers, a misaligned one is LVLIP_EINVAL before any
 * HIP call; LVLIP_ENODEV without a device; a failed launch is LVLIP_EHIP. */
int lvlip_snd_next_cpu(lvlip_snd_flow *s, lvlip_snd_result *res, uint32_t nflows);
int lvlip_snd_next_dev(lvlip_snd_flow *s, lvlip_snd_result *res, uint32_t nflows, void *stream);

/* Send the head of the queue again.  Flow k owns the slots s[k].slot0 ..
 * s[k].slot0 + s[k].rtx; nslots is what lvlip_snd_plan returned.  Slot j of
 * flow k is LIVE when popped_k + j < s[k].nseg, popped_k = snd[k].popped (snd
 * may be NULL: 0, a retransmission timeout without an ACK batch); its frame is
 * queue entry fd[s[k].seg0 + popped_k + j].  A caller who wants only the
 * timed-out flows sets rtx to 0 on the others before the plan.
 *
 * A live frame is rewritten IN PLACE in the ring as tcp_transmit_skb and
 * ip_output rewrite it:
 *   ack_seq  bytes 42-45 = htonl(f[k].rcv_nxt + lro[k].delivered) mod 2^32
 *            (src/tcp_output.c:107,122); lro may be NULL: delivered 0
 *   win      bytes 48-49 = htons(s[k].win) (:109,123)
 *   csum     bytes 50-51 = checksum(tcp, ip.len - 20, saddr + daddr + htons(6)
 *            + htons(ip.len - 20)) over the segment with the field zeroed and
 *            the two fields above in place (:110,126), stored raw; the seed a
 *            u32 that wraps (src/tcp.c:87-98: the carry is lost)
 * and fd_out[slot] = fd[that entry].  Everything else stays as it is, seq
 * included (tcp_retransmission_timeout passes snd_una, which is the head's own
 * seq, src/tcp_output.c:381; tcp_send_next numbers the segments from snd_nxt,
 * :214-218, which is theirs the first time they go out), and the IPv4 header
 * does not change: the reference never
 * advances the id (src/ip_output.c:36).  These ten bytes are the only bytes of
 * the ring that are stored.  A dead slot gets fd_out[slot] = {0, 0, 0}: a
 * length of 0 means no frame, as in lvlip_ack_dev.  So does a live slot whose
 * queue entry is not a frame these calls can rewrite (fd.len below 54, version
 * or ihl not 0x45, 14 + ip.len beyond fd.len, hl below 5 or beyond the
 * segment); its bytes stay.  fd_out must not overlap fd.
 *
 * The checksum is a full recomputation, not an RFC 1624 update of the old
 * field: the reference's seed loses its carry depending on the sum of the
 * WHOLE segment (src/tcp.c:92-95, src/utils.c:46-48), so an incremental update
 * is not bit-exact for every address pair.
 *
 * lvlip_rtx_cpu: on the calling thread.  Returns 0, or LVLIP_EINVAL (NULL f,
 * s, base, fd or fd_out with nslots > 0, nflows 0 or above
 * LVLIP_LRO_MAX_FLOWS with nslots > 0, nslots above LVLIP_MAX_BATCH or not the
 * plan's total) with nothing written.  nslots == 0 is a no-op.  Reentrant. */
int lvlip_rtx_cpu(const lvlip_lro_flow *f, const lvlip_lro_result *lro, const lvlip_snd_flow *s,
                  const lvlip_snd_result *snd, uint32_t nflows, uint32_t nslots, void *base,
                  const lvlip_frame_desc *fd, lvlip_frame_desc *fd_out);

/* The same bytes and fd_out in ONE launch on the caller's stream
 * (asynchronous; no allocation, copy, workspace, atomics or synchronisation):
 * header patch and the sum over header and payload in one pass over the frame.
 * All pointers are device pointers: f and s 8-B aligned, lro, snd, fd and
 * fd_out 16-B aligned, base any alignment, every frame readable from its first
 * byte rounded down to 16 B to its end rounded up to 16 B.  The refusals of
 * lvlip_rtx_cpu (the device cannot check nslots against the plan) and a
 * misaligned pointer are LVLIP_EINVAL before any HIP call; LVLIP_ENODEV
 * without a device; a failed launch is LVLIP_EHIP (lvlip_last_hip_error).
 * Measured: 1M live slots of 1460-B frames in 0.54 ms.  That
 * is SLOWER than the composed alternative, a header patch followed by
 * lvlip_tx_checksum_dev over the same frames, which takes 0.38 ms (ratio
 * 0.70): what this call has for it is one launch with the slot logic (live,
 * dead, popped) on the device, not speed.  A caller who holds the live
 * frames' descriptors anyway loses nothing by composing. */
int lvlip_rtx_dev(const lvlip_lro_flow *f, const lvlip_lro_result *lro, const lvlip_snd_flow *s,
                  const lvlip_snd_result *snd, uint32_t nflows, uint32_t nslots, void *base,
                  const lvlip_frame_desc *fd, lvlip_frame_desc *fd_out, void *stream);

/* ---- f2 on the device: the scoreboard and the selective retransmit ---------- */

/* lvlip_ack_dev writes a SACK option with up to four islands into every ACK it
 * builds; lvlip_snd_* reads only ack_seq, and lvlip_rtx_* re-sends the head of
 * a queue whatever the peer said about it.  These calls read the blocks back:
 * lvlip_sack_* marks, in a scoreboard of one byte per TX ring entry, the queue
 * entries the peer reports it holds, and lvlip_rtx_sack_* re-sends only
 * entries that are not marked.  The loop is then ... -> reverse lvlip_lro_dev
 * -> lvlip_snd_dev -> lvlip_sack_dev -> lvlip_rtx_sack_dev, still on one
 * stream with no host step.
 *
 * The reference never reads an incoming SACK block: tcp_parse_opts
 * (src/tcp_input.c:7-60) handles SACK-permitted only, and
 * tcp_retransmission_timeout (src/tcp_output.c:359-381) sends the head.  What
 * stays tied to it are the frames read, those its tcp_write_options writes
 * (src/tcp_output.c:65-91), and the bytes of every re-sent frame, which are
 * lvlip_rtx_*'s.
 *
 * Arguments of lvlip_sack_*.  f and s are the planned reverse flows and their
 * send sides, exactly as lvlip_snd_* takes them; rec[i] is the record the
 * reverse lvlip_lro_* call wrote for frame ack_fd[i] inside ack_base; base and
 * fd are the TX ring; sacked is the caller's scoreboard, one byte per fd
 * index, any alignment, at least the *nfd entries lvlip_snd_plan reports.
 *
 * Which frames count.  Record i counts for flow k = rec[i].flow under exactly
 * the rule of lvlip_snd_* ("Which records carry an ACK" above).
 *
 * The blocks of a counting frame.  ihl and hl are read from the frame itself;
 * the options are the bytes [14 + ihl*4 + 20, 14 + ihl*4 + hl*4).  A frame has
 * no blocks when fd.len is below that end, its version is not 4, ihl is below
 * 5 or hl is below 5: this holds for ANY record array, a crafted record
 * changes values and never an address.  The options are walked as RFC 793
 * lays them out: kind 0 ends the list, kind 1 is one byte, any other kind has
 * a length byte, and a length below 2 or one that runs past the end ends the
 * walk.  Kind 5 with length 2 + 8 b, b in 1..4, gives b blocks, each
 * ntohl(left), ntohl(right) (RFC 2018 §3); a kind 5 of any other length is
 * skipped by its length.  A frame yields at most the first four blocks across
 * all of its kind-5 options.  Only bytes inside the frame are read.
 *
 * Valid blocks.  l = (left - s[k].snd_una) mod 2^32, r = (right -
 * s[k].snd_una) mod 2^32, span = (s[k].snd_nxt - s[k].snd_una) mod 2^32, all
 * against the values AT CALL ENTRY, as lvlip_snd_* classes its ACKs.  A block
 * is valid when l < r <= span.  Blocks below snd_una (D-SACK, stale), empty
 * blocks and blocks beyond snd_nxt are counted in n_blocks only.
 *
 * Marking.  For queue entry q in [s[k].seg0, s[k].seg0 + s[k].nseg): seq,
 * ip.len, ihl and hl from its 54 header bytes, as `popped` reads them; a =
 * (seq - snd_una) mod 2^32, len = ip.len - ihl*4 - hl*4, e = a + len in 64
 * bits.  sacked[q] becomes 1 when the entry is a frame lvlip_rtx_* could
 * rewrite (its list of refusals), len > 0, and every byte of [a, e) lies in
 * the UNION of the flow's valid blocks of this batch, where blocks that touch
 * or overlap are one island.  Otherwise sacked[q] keeps its byte: the call
 * only ever stores the value 1, and only inside the planned queues, so the
 * scoreboard accumulates over calls: the MARKS do, the blocks do not.  The
 * union is taken per batch, so an entry that only blocks of two different
 * calls cover together (one block ends inside it, a later call's block starts
 * there) is not marked; blocks that belong together go into one call.  The
 * caller forgets by zeroing the scoreboard, and
 * should zero a flow's queue at a retransmission timeout (RFC 2018 §8: the
 * peer may renege).  Because of the union the results depend neither on the
 * order of the records, nor on which frame carried which block, nor on the
 * queue being in sequence order.
 *
 * Departures from the reference: incoming SACK blocks are read at all; an
 * entry is marked by the union of a batch's blocks, not block by block; the
 * comparisons are mod 2^32 against the entry value of snd_una. */
typedef struct lvlip_sack_result {    /* one per planned flow; sizeof == 16 */
    uint32_t n_blocks;                /* SACK blocks read from the flow's counting records */
    uint32_t n_valid;                 /* of those, valid (above) */
    uint32_t n_sacked;                /* entries of the flow's queue whose sacked byte is 1 after the call */
    uint32_t high;                    /* the largest r among the valid blocks (relative to snd_una), 0 if none */
} lvlip_sack_result;

/* On the calling thread.  Returns 0, or LVLIP_EINVAL (NULL f, s, base, fd,
 * sacked or res with nflows > 0 and n > 0, NULL rec, ack_base or ack_fd with
 * n > 0, n above LVLIP_MAX_BATCH, nflows above LVLIP_LRO_MAX_FLOWS) or
 * LVLIP_ENOMEM (its block list) with nothing written.  nflows == 0 and n == 0
 * are no-ops: res and sacked keep their bytes.  Reentrant. */
int lvlip_sack_cpu(const lvlip_lro_flow *f, const lvlip_snd_flow *s, uint32_t nflows, const lvlip_lro_rec *rec,
                   const void *ack_base, const lvlip_frame_desc *ack_fd, uint32_t n, const void *base,
                   const lvlip_frame_desc *fd, uint8_t *sacked, lvlip_sack_result *res);

/* Bytes of device workspace lvlip_sack_dev needs for n records (96 n and a
 * little: a key and an end per possible block, twice, and rocPRIM's storage).
 * Returns 0 for n == 0 and for n above 2^30 - 1, which no workspace serves
 * (the element indices are 32 bits; lvlip_sack_dev returns LVLIP_ERANGE).  May
 * initialise the HIP runtime; returns 0 when there is no device. */
size_t lvlip_sack_workspace_bytes(uint32_t n, uint32_t nflows);

/* The same bytes of res and sacked on the caller's stream (asynchronous; no
 * allocation, no device-to-host copy, no synchronisation): a lane per ACK
 * frame parses the options into up to four keys flow << 32 | l with the end r
 * as value, rocPRIM's radix sort and two max-scans unite them per flow, and a
 * lane per queue entry searches its flow's range of the sorted blocks.  The
 * queue lengths are in device memory, so the waves a queue is spread over come
 * from the flow count: min(1024, max(8, 131072 / ceil(nflows / 4))), each wave
 * taking every such chunk of 64 entries; beyond 16 384 flows a queue of q
 * entries costs its eight waves q / 512 steps each.  All
 * pointers are device pointers: f and s 8-B aligned, rec, ack_fd, fd and res
 * 16-B aligned, workspace 256-B aligned, ack_base, base and sacked any
 * alignment; frames readable as for the other _dev frame calls.  The refusals
 * of lvlip_sack_cpu, a NULL workspace and a misaligned pointer are
 * LVLIP_EINVAL before any HIP call; workspace_bytes below
 * lvlip_sack_workspace_bytes(n, nflows) is LVLIP_ERANGE with nothing written;
 * LVLIP_ENODEV without a device; a failed launch is LVLIP_EHIP
 * (lvlip_last_hip_error).
 * Measured: 1M ACK frames with 2.6M blocks in 0.80 ms over 1K
 * flows, 0.84 ms over 64K flows and 1.14 ms with every record of one flow over
 * a queue of 65 536 entries, against 207, 263 and 302 ms for copying records
 * and frames to the host, lvlip_sack_cpu there and the scoreboard back: 260 to
 * 312 times faster. */
int lvlip_sack_dev(const lvlip_lro_flow *f, const lvlip_snd_flow *s, uint32_t nflows, const lvlip_lro_rec *rec,
                   const void *ack_base, const lvlip_frame_desc *ack_fd, uint32_t n, const void *base,
                   const lvlip_frame_desc *fd, uint8_t *sacked, lvlip_sack_result *res, void *workspace,
                   size_t workspace_bytes, void *stream);

/* lvlip_rtx_* with a scoreboard.  Slot j of flow k is the j-th queue entry,
 * counted from 0 and from s[k].seg0 + popped_k up to the queue's end, whose
 * sacked byte is 0; without such an entry the slot is dead.  pick[slot] gets
 * that fd index, or 0xFFFFFFFF for a dead slot (pick 4-B aligned, nslots
 * entries).  A live slot's frame is rewritten in place exactly as lvlip_rtx_*
 * rewrites it: the same ten bytes, the same refusals, the same fd_out; a dead
 * slot gets fd_out = {0, 0, 0}.  With sacked == NULL ring and fd_out equal
 * lvlip_rtx_*'s and pick is the plain mapping.  Other arguments, refusals and
 * return codes as for lvlip_rtx_cpu / lvlip_rtx_dev; a NULL pick with
 * nslots > 0 is LVLIP_EINVAL, and so is a misaligned pick on the device.  The
 * device form is two launches on the stream: a wave per flow scans the
 * scoreboard (a ballot and a popcount prefix) and writes pick, then
 * lvlip_rtx_dev's kernel runs from the queue entry onwards.
 * Measured: with no mark set, so that it re-sends the frames
 * lvlip_rtx_dev does, this call is SLOWER than lvlip_rtx_dev by its selection
 * pass: 0.148 against 0.139 ms at 262 144 slots of 1460-B frames, 0.513
 * against 0.512 ms at 1M.  lvlip_rtx_dev itself costs what it cost before its
 * kernel took the pick argument (0.139 against 0.138 ms, 0.5115 against
 * 0.5112 ms). */
int lvlip_rtx_sack_cpu(const lvlip_lro_flow *f, const lvlip_lro_result *lro, const lvlip_snd_flow *s,
                       const lvlip_snd_result *snd, const uint8_t *sacked, uint32_t nflows, uint32_t nslots,
                       void *base, const lvlip_frame_desc *fd, lvlip_frame_desc *fd_out, uint32_t *pick);
int lvlip_rtx_sack_dev(const lvlip_lro_flow *f, const lvlip_lro_result *lro, const lvlip_snd_flow *s,
                       const lvlip_snd_result *snd, const uint8_t *sacked, uint32_t nflows, uint32_t nslots,
                       void *base, const lvlip_frame_desc *fd, lvlip_frame_desc *fd_out, uint32_t *pick,
                       void *stream);

/* ---- f2 on the device: the write queue -------------------------------------- */

/* tcp_send + tcp_queue_transmit_skb (src/tcp_output.c:131-156, 445-478) per
 * round: bytes the application has made ready are cut into segments, built as
 * frames in the flow's slots of the TX ring and appended to its write queue,
 * and the entries lvlip_snd_next_* popped are given back.  A connection that
 * keeps writing then needs a ring and an fd region of `cap` slots, not of
 * everything it will ever send, and no host step per write: the loop is
 * ... -> lvlip_snd_next_* -> lvlip_push_* -> lvlip_rtx_sack_* -> ...
 *
 * lvlip_push_flow k is the write side of flow k of the reverse plan, as
 * lvlip_snd_flow k is.  Its frame slot j (0 <= j < cap) is the stride bytes at
 * ring_off + j*stride of the ring; its fd / scoreboard region is the indices
 * [q0, q0 + cap).  Slots are filled round robin from slot_nxt.
 *
 * One call does for flow k, from the values at entry:
 *   1 compact  if s[k].seg0 != q0: fd[q0 + i] = fd[seg0 + i] for i < nseg, and
 *              likewise sacked[], as memmove does (entries that are not
 *              overwritten keep their bytes); seg0 = q0, res.moved = nseg
 *              (else 0).  Frames do not move: fd holds their offsets.
 *   2 count    span = (snd_nxt - snd_una) mod 2^32; m is the largest count with
 *              m <= cap - nseg, m <= push, m <= ceil(unsent / mss) and
 *              span + min(m*mss, unsent) <= wnd.  Only whole segments are
 *              pushed; a short one is only the one that ends `unsent`.
 *   3 build    segment i < m carries dlen_i = min(mss, unsent - i*mss) bytes; its
 *              frame, at ring_off + ((slot_nxt + i) mod cap)*stride, holds
 *              exactly the bytes lvlip_tso_* writes for segment i of a send
 *              {payload_off = pay_off, len = unsent, mss, hdr} whose template
 *              has seq = htonl(snd_nxt), ack_seq = htonl(f[k].rcv_nxt +
 *              lro[k].delivered) and window = htons(s[k].win) in place of its
 *              own (lvlip_rtx_*'s two fields, src/tcp_output.c:107-109); PSH
 *              thus goes only on the segment that empties `unsent` (:466).
 *              fd[q0 + nseg + i] = fd_out[slot0 + i] = {offset, 54 + dlen_i, 0}
 *              and sacked[q0 + nseg + i] = 0.  Slots i >= m of the flow's
 *              `push` get fd_out = {0, 0, 0}.  No byte of the ring outside the
 *              m frames is stored: stride gaps keep their bytes.
 *   4 step     nseg += m, snd_nxt += bytes, pay_off += bytes, unsent -= bytes,
 *              slot_nxt = (slot_nxt + m) mod cap; res[k] = {m, bytes, q0 + nseg
 *              (the first new entry's fd index), moved}.
 *
 * Contract.  The call runs after lvlip_snd_next_* has consumed the last
 * lvlip_snd_result; it ignores `popped`.  The queue's entries hold the cap
 * slots first in, first out, starting from an empty queue (every entry of a
 * queue was appended by these calls), so a slot being filled never holds a
 * live frame.  `pick` values of an earlier lvlip_rtx_sack_* call are stale
 * after a compaction.  Refilling pay_off / unsent / wnd is the application's
 * step, as reopening rcv_wnd is.  wnd is the hook for a peer's or a congestion
 * window: the reference never limits the bytes in flight (snd_wnd is written
 * once, src/tcp_output.c:429); 2^30 means "no limit".  A FIN has to
 * advance snd_nxt: the plan refuses it in a template, and lvlip_fin_* below
 * ("the end of a connection") sends it once `unsent` is 0. */
typedef struct lvlip_push_flow {      /* one per planned flow; sizeof == 112 */
    uint64_t pay_off;                 /* the next unsent byte, from the payload base; any alignment */
    uint64_t ring_off;                /* frame slot 0, from the ring base; any alignment */
    uint32_t unsent;                  /* bytes ready to send, 0 .. 2^30 */
    uint32_t stride;                  /* >= 54 + mss; any value */
    uint32_t cap;                     /* frame slots = fd entries of the flow, > 0 */
    uint32_t q0;                      /* the flow's fd / scoreboard region is [q0, q0 + cap) */
    uint32_t slot_nxt;                /* the next frame slot to fill, < cap */
    uint32_t push;                    /* the most segments one call may append */
    uint32_t slot0;                   /* filled by the plan: the running sum of push */
    uint32_t wnd;                     /* bytes allowed between snd_una and snd_nxt, 0 .. 2^30 */
    uint16_t mss;                     /* 1 .. 65495 */
    uint16_t reserved;                /* 0 */
    uint8_t  hdr[54];                 /* as lvlip_tso_send.hdr; seq, ack_seq and window are ignored */
    uint8_t  pad[6];                  /* 0 */
} lvlip_push_flow;

typedef struct lvlip_push_result {    /* one per planned flow; sizeof == 16 */
    uint32_t pushed;                  /* m */
    uint32_t bytes;                   /* payload bytes of the m segments */
    uint32_t first;                   /* the fd index of the first new entry */
    uint32_t moved;                   /* queue entries moved down to q0 */
} lvlip_push_result;

/* Host only: validates the write sides against the send sides and fills slot0
 * with the running sum of push; nothing else is modified.  Returns the total
 * slot count (nslots of lvlip_push_*), or 0xFFFFFFFF with w unwritten for: a
 * template lvlip_tso_plan refuses, or one with FIN, SYN, RST or URG set; cap 0,
 * slot_nxt >= cap, mss 0 or above 65495, stride < 54 + mss, unsent or wnd above
 * 2^30, nonzero reserved or pad; a region [q0, q0 + cap) that passes 2^32 or a
 * ring range that passes 2^64; two flows whose [q0, q0 + cap) overlap, or whose
 * [ring_off, ring_off + cap*stride) overlap; a non-empty queue of s[k] that is
 * not inside [q0, q0 + cap); a total of push or of cap above LVLIP_MAX_BATCH;
 * nflows above LVLIP_LRO_MAX_FLOWS; NULL w or s; or no memory for the overlap
 * checks.  *ring_bytes (may be NULL) gets the largest ring_off + (cap - 1)*stride
 * + 54 + mss, the bytes the ring must hold, and *nfd (may be NULL) the largest
 * q0 + cap, the entries fd, sacked and the scoreboard calls' arrays must hold. */
uint32_t lvlip_push_plan(lvlip_push_flow *w, const lvlip_snd_flow *s, uint32_t nflows, uint64_t *ring_bytes,
                         uint32_t *nfd);

/* On the calling thread, one checksum() per field (seg_cpu.c's frame writer, so
 * the frames are lvlip_tso_cpu's by construction).  f, lro (may be NULL:
 * delivered 0) and s exactly as lvlip_rtx_* takes them; payload is only read;
 * base is the ring; sacked may be NULL; s, w, fd, sacked, fd_out and res are
 * written.  nslots is what lvlip_push_plan returned.  Returns 0, or
 * LVLIP_EINVAL with nothing written: NULL f, s, w, fd or res with nflows > 0;
 * NULL payload, base or fd_out, or nflows 0, with nslots > 0; nflows above
 * LVLIP_LRO_MAX_FLOWS, nslots above LVLIP_MAX_BATCH; w not as the plan left it
 * (slot0, nslots) or a flow the plan would refuse for its own fields or its
 * queue.  nflows == 0 is a no-op; with nslots == 0 the call still compacts and
 * writes res.  Reentrant. */
int lvlip_push_cpu(const lvlip_lro_flow *f, const lvlip_lro_result *lro, lvlip_snd_flow *s, lvlip_push_flow *w,
                   uint32_t nflows, uint32_t nslots, const void *payload, void *base, lvlip_frame_desc *fd,
                   uint8_t *sacked, lvlip_frame_desc *fd_out, lvlip_push_result *res);

/* The same bytes of every output on the caller's stream (asynchronous; no
 * allocation, copy, atomics or synchronisation, no workspace beyond res), in
 * three launches: a wave per flow moves the queue down in ascending chunks of
 * 64 entries, each read completely before it is written, and one lane counts m
 * and writes res; lvlip_tso_dev's kernel body, a 16-lane row per slot, builds
 * the frames of the live slots (payload copy and TCP checksum in one pass); a
 * lane per flow does the step.  All pointers are device pointers: f, s and w
 * 8-B aligned, lro, fd, fd_out and res 16-B aligned, payload, base and sacked
 * any alignment.  The NULL and limit refusals of lvlip_push_cpu and a
 * misaligned pointer are LVLIP_EINVAL before any HIP call; LVLIP_ENODEV without
 * a device; a failed launch is LVLIP_EHIP (lvlip_last_hip_error).  The device
 * does not validate w again: the caller planned it.  Measured: DESIGN.md
 * section 9i. */
int lvlip_push_dev(const lvlip_lro_flow *f, const lvlip_lro_result *lro, lvlip_snd_flow *s, lvlip_push_flow *w,
                   uint32_t nflows, uint32_t nslots, const void *payload, void *base, lvlip_frame_desc *fd,
                   uint8_t *sacked, lvlip_frame_desc *fd_out, lvlip_push_result *res, void *stream);

/* ---- f2 on the device: the timer and the peer's window ----------------------- */

/* The two decisions of the sender's loop that the calls above leave to the
 * host: WHEN a flow re-sends (lvlip_rto_*) and HOW FAR it may run ahead of the
 * peer (lvlip_wnd_*).  With them the loop is ... -> reverse lvlip_lro_* ->
 * lvlip_snd_* -> lvlip_sack_* -> lvlip_wnd_* -> lvlip_snd_next_* ->
 * lvlip_push_* -> lvlip_rto_* -> lvlip_rtx_sack_* -> ..., and the application
 * supplies bytes and one clock value per round.
 *
 * lvlip_rto_flow k is the timer and window state of flow k of the reverse
 * plan, as lvlip_snd_flow k is its send side.  The struct has no padding: every
 * byte is a field.
 *
 * lvlip_rto_* restates, per flow and per round:
 *   tcp_rtt                      src/tcp.c:424-452 (RFC 6298 2.2, 2.3; the 200 ms
 *                                floor of :449), with Karn's rule of :426
 *   tcp_retransmission_timeout   src/tcp_output.c:359-401: the empty queue
 *                                (:371-375), the 60 s cut-off (:384-391, tcp_done
 *                                and -ETIMEDOUT), doubling and backoff (:394-396)
 *   tcp_rearm_rto_timer          on the first skb of an empty queue
 *                                (src/tcp_output.c:138-140, :417)
 *   tcp_stop_rto_timer           when the queue empties (src/tcp_input.c:86-89)
 *   the timer's test             t->expires < tick, src/timer.c:71: strict, and
 *                                unsigned (expires is a uint32_t there)
 * The caller starts a flow with rto = 1000 (src/tcp_input.c:196), everything
 * else 0 but wnd_cap and wscale.
 *
 * One call, for flow k, in this fixed order, with nseg = s[k].nseg (the queue
 * as it now stands), pushed = min(push[k].pushed, nseg) (push may be NULL: 0)
 * and before = nseg - pushed, the queue before the push:
 *   1 ACKs   n_new = snd[k].n_new, n_dup = snd[k].n_dup (they survive
 *            lvlip_snd_next_*; snd may be NULL: both 0).
 *            n_new > 0: tcp_rtt, then dupacks = 0, then, if before == 0,
 *            armed = 0 and backoff = 0.  tcp_rtt returns at once when
 *            backoff > 0 or the timer is not armed; else r = (int32_t)(now -
 *            (expires - rto)) with the CURRENT rto, which after the first sample
 *            is no longer the one the timer was armed with: the reference's
 *            quirk, kept; r < 0 returns.  srtt == 0 (:434, the reference's test
 *            for "first") : srtt = r, rttvar = r / 2.  Else rttvar = (3 rttvar +
 *            |srtt - r|) / 4, then srtt = (7 srtt + r) / 8, both truncated
 *            towards 0.  These equal the reference's double arithmetic for
 *            every int32_t input: the products by 0.75, 0.25, 0.875 and 0.125
 *            are exact in a double and its conversion to int truncates the
 *            same way.  Then k = max(4 rttvar, 200) and rto = srtt + k.
 *            n_new == 0: dupacks += n_dup.
 *   2 push   pushed > 0 and before == 0: armed = 1, expires = now + rto.
 *   3 timer  armed and expires < now: with nseg == 0, armed = 0 and
 *            backoff = 0 and nothing fires; else the flow FIRES (timeout) and
 *            either rto > 60000: dead = 1, armed = 0, backoff = 0 (tcp_done
 *            stops the timer, src/tcp.c:313-334; the head is sent first there
 *            too), or rto *= 2, backoff++ (a uint8_t, as there),
 *            expires = now + rto.
 *   4 fast   only with LVLIP_RTO_FAST and when step 3 did not fire: dupacks was
 *            below 3 at entry, is at least 3 now, and nseg > 0: the flow FIRES
 *            (fast).  No timer state changes.  The reference has no fast
 *            retransmit; this is RFC 5681 section 3.2.
 * A flow that is dead at entry never fires and nothing of it changes.
 *
 * Outputs.  res[k] = {fired, sample, rto, backoff}: fired 0, LVLIP_RTO_TIMEOUT
 * or LVLIP_RTO_FASTRTX; sample the r that tcp_rtt took, 0xFFFFFFFF when it took
 * none; rto and backoff as the call leaves them.  gate[k] is a whole
 * lvlip_snd_result, all zero but popped: 0 for a flow that fired, s[k].nseg for
 * one that did not.  Passed as `snd` to the unchanged lvlip_rtx_* /
 * lvlip_rtx_sack_* it makes every slot of a silent flow dead by their own rule
 * (popped_k + j < nseg), so rtx needs no host step per round.  With a non-NULL
 * sacked a flow that TIMED OUT has sacked[seg0 .. seg0 + nseg) zeroed (RFC 2018
 * section 8, the peer may renege; see lvlip_sack_* above); a fast retransmit
 * keeps the marks; no other byte of the scoreboard is stored.
 *
 * Departures from the reference: one `now` per call, with a round's ACKs
 * ordered before its timer (there each runs when it happens); the dupack count
 * and the fast retransmit; `dead` stands for tcp_done, which stays on the host.
 *
 * lvlip_wnd_* reads the window field of the ACKs.  The reference never does:
 * src/tcp_input.c:352-354 is a TODO and snd_wnd is written once
 * (src/tcp_output.c:429).  Reading it is a departure, as reading SACK blocks is.
 *
 * Which records count.  Record i counts for flow k = rec[i].flow under the rule
 * of lvlip_snd_* ("Which records carry an ACK"), when besides d = (ack_seq -
 * s[k].snd_una) mod 2^32 is at most span = (s[k].snd_nxt - s[k].snd_una) mod
 * 2^32 (new or duplicate, against the values at call entry), and when its
 * frame ack_fd[i] passes the test lvlip_sack_* applies before it reads
 * options: fd.len at least 34, version 4, ihl at least 5, fd.len at least 14 +
 * ihl*4 + 20, hl at least 5 and fd.len at least 14 + ihl*4 + hl*4.  Only bytes
 * inside the frame are read: a crafted record changes values, never an address.
 *
 * The winner of flow k is the counting record with the largest (d, i), i the
 * record index: RFC 793's SND.WL1 / SND.WL2 rule (take the window of the
 * segment that acknowledges most, the later one among equals) reduced to what
 * a batch can order.  It does not depend on the order the records run in.
 *
 * res[k] = {n_counting, winner (0xFFFFFFFF if none), raw, snd_wnd}: raw =
 * ntohs of the two bytes at 14 + ihl*4 + 14 of the winner's frame (0 without a
 * winner), and t[k].snd_wnd = min(raw << t[k].wscale, 2^30); a flow without a
 * winner keeps its snd_wnd; res[k].snd_wnd is t[k].snd_wnd as the call leaves
 * it.  With LVLIP_WND_APPLY and a non-NULL w, w[k].wnd = min(t[k].snd_wnd,
 * t[k].wnd_cap) for EVERY flow; nothing else of w and t is written.  wnd_cap is
 * where a congestion window plugs in.  n == 0 is not a no-op: no flow has a
 * winner, res is written and the window applied.  A flow whose peer closes the
 * window waits for the next ACK that opens it; the zero-window persist timer
 * (RFC 1122 4.2.2.17) that covers the loss of that ACK is lvlip_persist_*
 * below. */
#define LVLIP_RTO_FAST    0x1u        /* flags of lvlip_rto_*: step 4 */
#define LVLIP_RTO_TIMEOUT 1u          /* lvlip_rto_result.fired */
#define LVLIP_RTO_FASTRTX 2u
#define LVLIP_RTO_DEAD_MS 60000u      /* src/tcp_output.c:384 */
#define LVLIP_WND_APPLY   0x1u        /* flags of lvlip_wnd_*: write w[k].wnd */
#define LVLIP_WSCALE_MAX  14u         /* RFC 7323 2.3 */

typedef struct lvlip_rto_flow {       /* one per planned flow, index k = flow k in plan order; sizeof == 32 */
    int32_t  srtt, rttvar;            /* tsk->srtt, tsk->rttvar, ms */
    uint32_t rto;                     /* ms; the caller starts it at 1000 */
    uint32_t expires;                 /* timer->expires; meaningful while armed */
    uint32_t dupacks;                 /* duplicate ACKs since the last new one, carried across batches */
    uint32_t snd_wnd;                 /* the peer's window in bytes, as lvlip_wnd_* last left it; 0 .. 2^30 */
    uint32_t wnd_cap;                 /* the caller's ceiling on w.wnd, 0 .. 2^30 */
    uint8_t  armed;                   /* tsk->retransmit != NULL; 0 or 1 */
    uint8_t  backoff;                 /* tsk->backoff */
    uint8_t  dead;                    /* sticky, 0 or 1: a timeout found rto > 60000 */
    uint8_t  wscale;                  /* the peer's window scale, 0 .. 14 */
} lvlip_rto_flow;

typedef struct lvlip_rto_result {     /* one per planned flow; sizeof == 16 */
    uint32_t fired, sample, rto, backoff;
} lvlip_rto_result;

typedef struct lvlip_wnd_result {     /* one per planned flow; sizeof == 16 */
    uint32_t n_counting, winner, raw, snd_wnd;
} lvlip_wnd_result;

/* Host only: 0 when every t[k] is a state these calls take, LVLIP_EINVAL for a
 * wscale above 14, snd_wnd or wnd_cap above 2^30, armed or dead other than 0
 * and 1, a NULL t with nflows > 0 or nflows above LVLIP_LRO_MAX_FLOWS.  The
 * _dev forms cannot look: the state is in HBM; the caller checks it here before
 * it uploads it, as the plans check theirs.  Nothing is written. */
int lvlip_rto_check(const lvlip_rto_flow *t, uint32_t nflows);

/* On the calling thread.  f, s: the planned reverse flows and their send sides
 * as lvlip_snd_* takes them (read only); t, w (may be NULL) and res are
 * written as above; rec[i] is the record of frame ack_fd[i] inside ack_base.
 * Returns 0, or LVLIP_EINVAL with nothing written: NULL f, s, t or res with
 * nflows > 0, NULL rec, ack_base or ack_fd with n > 0, n above LVLIP_MAX_BATCH,
 * nflows above LVLIP_LRO_MAX_FLOWS, flag bits other than LVLIP_WND_APPLY, or a
 * t lvlip_rto_check refuses.  nflows == 0 is a no-op.  Reentrant. */
int lvlip_wnd_cpu(const lvlip_lro_flow *f, const lvlip_snd_flow *s, lvlip_rto_flow *t, lvlip_push_flow *w,
                  uint32_t nflows, const lvlip_lro_rec *rec, const void *ack_base, const lvlip_frame_desc *ack_fd,
                  uint32_t n, uint32_t flags, lvlip_wnd_result *res);

/* The same bytes of res, t and w on the caller's stream (asynchronous; no
 * allocation, copy, synchronisation or LDS, no workspace beyond res): res is
 * zeroed, a lane per record raises its flow's 64-bit key (d + 1) << 32 | i
 * with one atomic max and counts with one atomic add (records of one flow are
 * first reduced within their wave, as in lvlip_snd_dev; max and add only, so
 * the bytes do not depend on the run), and a lane per flow reads the winner's
 * window and writes res, t and w.  All pointers are device pointers: f, s, t
 * and w 8-B aligned, rec, ack_fd and res 16-B aligned, ack_base any alignment.
 * The NULL, limit and flag refusals of lvlip_wnd_cpu and a misaligned pointer
 * are LVLIP_EINVAL before any HIP call (t is not looked at: lvlip_rto_check);
 * LVLIP_ENODEV without a device; a failed launch is LVLIP_EHIP
 * (lvlip_last_hip_error).  Measured: DESIGN.md section 9j. */
int lvlip_wnd_dev(const lvlip_lro_flow *f, const lvlip_snd_flow *s, lvlip_rto_flow *t, lvlip_push_flow *w,
                  uint32_t nflows, const lvlip_lro_rec *rec, const void *ack_base, const lvlip_frame_desc *ack_fd,
                  uint32_t n, uint32_t flags, lvlip_wnd_result *res, void *stream);

/* On the calling thread, once per round, after lvlip_snd_next_* and
 * lvlip_push_*.  s, snd (may be NULL) and push (may be NULL) are read; t,
 * gate, res and, if given, sacked (one byte per fd index, any alignment) are
 * written as above.  Returns 0, or LVLIP_EINVAL with nothing written: NULL s,
 * t, gate or res with nflows > 0, nflows above LVLIP_LRO_MAX_FLOWS, flag bits
 * other than LVLIP_RTO_FAST, or a t lvlip_rto_check refuses.  nflows == 0 is a
 * no-op.  Reentrant. */
int lvlip_rto_cpu(const lvlip_snd_flow *s, const lvlip_snd_result *snd, const lvlip_push_result *push,
                  lvlip_rto_flow *t, uint32_t nflows, uint32_t now, uint32_t flags, uint8_t *sacked,
                  lvlip_snd_result *gate, lvlip_rto_result *res);

/* The same bytes in ONE launch on the caller's stream (asynchronous; no
 * allocation, copy, atomics, LDS, workspace or synchronisation): a wave per
 * flow, four per workgroup; lane 0 does the arithmetic and the 16- and 32-byte
 * stores, and the wave clears a timed-out flow's scoreboard range 64 bytes a
 * step.  All pointers are device pointers: s and t 8-B aligned, snd, push, gate
 * and res 16-B aligned, sacked any alignment.  The NULL, limit and flag
 * refusals of lvlip_rto_cpu and a misaligned pointer are LVLIP_EINVAL before
 * any HIP call (t is not looked at: lvlip_rto_check); LVLIP_ENODEV without a
 * device; a failed launch is LVLIP_EHIP (lvlip_last_hip_error).  Measured:
 * DESIGN.md section 9j. */
int lvlip_rto_dev(const lvlip_snd_flow *s, const lvlip_snd_result *snd, const lvlip_push_result *push,
                  lvlip_rto_flow *t, uint32_t nflows, uint32_t now, uint32_t flags, uint8_t *sacked,
                  lvlip_snd_result *gate, lvlip_rto_result *res, void *stream);

/* ---- f2 on the device: the congestion window --------------------------------
 *
 * lvlip_push_* sends up to w.wnd bytes past snd_una and lvlip_wnd_* sets that
 * to min(snd_wnd, t.wnd_cap).  lvlip_cc_* writes t[k].wnd_cap once per round:
 * the congestion window of RFC 5681 (slow start, congestion avoidance, the
 * cut on a timeout) with RFC 3465's byte counting, the recovery point of RFC
 * 6582 and the pipe of RFC 6675, from what the other calls already leave on the
 * device: lvlip_snd_result.acked / n_new, lvlip_rto_result.fired / backoff,
 * the scoreboard of lvlip_sack_* and the queue's fd[].  The reference has a
 * cwnd field (include/tcp.h:211) that it never reads or writes: like reading
 * SACK blocks and the window field, this is a departure that follows the RFCs.
 *
 * lvlip_cc_flow k is the congestion state of flow k of the reverse plan, as
 * lvlip_rto_flow k is its timer.  The struct has no padding.  The caller starts
 * a flow with cwnd at the initial window (RFC 5681 3.1: min(4 mss, max(2 mss,
 * 4380))), ssthresh = 2^30, its mss and ceiling, everything else 0.
 *
 * Where it sits in the loop.  After lvlip_sack_* and before lvlip_wnd_* and
 * lvlip_snd_next_*: snd[k].acked and popped are still unconsumed there; s[k] is
 * as the previous round's lvlip_rto_* saw it, because nothing between them
 * writes s; prev is the previous round's lvlip_rto_result array.  lvlip_wnd_*
 * with LVLIP_WND_APPLY then carries t[k].wnd_cap into w[k].wnd, unchanged.
 *
 * One call, for flow k, in this fixed order, with
 *   flight = (s.snd_nxt - s.snd_una) mod 2^32
 *   a = snd[k].acked, n_new = snd[k].n_new      (snd may be NULL: both 0)
 *   fired = prev[k].fired, bo = prev[k].backoff (prev may be NULL: both 0)
 *   half = max(flight / 2, 2 mss)
 * A flow with t[k].dead set: c[k] and t[k] do not change, res[k] = {c.cwnd, 0,
 * 0, 0}.  Otherwise:
 *   1 loss   from the previous round's timer.
 *            fired == LVLIP_RTO_TIMEOUT: ssthresh = half only when bo == 1 (RFC
 *            5681 3.1: a segment that times out again does not halve twice);
 *            always cwnd = mss, acc = 0, in_rec = 0, recover = s.snd_nxt; event
 *            TIMEOUT.
 *            fired == LVLIP_RTO_FASTRTX and in_rec == 0: ssthresh = half, cwnd =
 *            ssthresh, acc = 0, in_rec = 1, recover = s.snd_nxt; event ENTER (RFC
 *            6675 5, step 4.2).  FASTRTX while in_rec == 1 changes nothing.
 *   2 ACKs   only when n_new > 0 and a > 0.
 *            in_rec == 1: a full ACK, a >= (recover - s.snd_una) mod 2^32, sets
 *            in_rec = 0, cwnd = ssthresh, acc = 0; event EXIT.  A partial ACK
 *            changes nothing: the pipe of step 3 governs what goes out.
 *            in_rec == 0 and cwnd < ssthresh: cwnd += min(a, n_new * mss),
 *            formed in 64 bits (RFC 5681 eq. 2 summed over the batch's ACKs);
 *            event SLOWSTART.
 *            in_rec == 0 otherwise: acc += a (64 bits); if acc >= cwnd then
 *            acc -= cwnd, cwnd += mss, event AVOID, once per call (a batch is
 *            a round and RFC 5681 allows one mss per RTT); then acc = min(acc,
 *            cwnd).
 *            Finally cwnd = min(cwnd, cwnd_max), whichever of the three ran and
 *            whether it changed anything.  No loops: the step takes the same
 *            time for every input.
 *   3 pipe   p = min(snd[k].popped, s.nseg).  Over the queue entries q in
 *            [seg0 + p, seg0 + nseg), the index formed in 64 bits: n_sacked
 *            counts the entries with sacked[q] != 0 (the test of
 *            lvlip_rtx_sack_*), sacked_bytes sums fd[q].len - 54 over those of
 *            them with fd[q].len >= 54, in 64 bits, clamped to 2^30.  A NULL
 *            sacked gives both 0.
 *   4 output t[k].wnd_cap = min(cwnd + sacked_bytes, 2^30): the bytes the peer
 *            reports holding are not in the network, so bounding snd_nxt -
 *            snd_una by this bounds RFC 6675's pipe by cwnd.  res[k] = {cwnd,
 *            sacked_bytes, n_sacked, event}.  Nothing else of t is written.
 *
 * Limits.  Step 3 reads fd and sacked only, never the ring: an entry's payload
 * is taken as fd.len - 54, the header of every frame lvlip_tso_* and
 * lvlip_push_* build; a queue of frames with IP or TCP options is overcounted
 * by their length.  s is not validated again (the caller planned it), and
 * neither is what the arithmetic leaves: a caller who hands in in_rec = 1 with
 * ssthresh below mss gets that back as cwnd on the full ACK, and step 1 does
 * not apply cwnd_max; lvlip_cc_check says so before the next call.
 *
 * Departures.  The reference has no congestion control.  One step per batch,
 * not per ACK.  No retransmit of the next hole on a partial ACK:
 * lvlip_rtx_sack_* with rtx > 1 re-sends several holes when the flow fires, and
 * the timer covers the rest.  No ECN, no pacing.  The persist timer is
 * lvlip_persist_* below. */
#define LVLIP_CC_MAX_WND 0x40000000u
/* event bits of lvlip_cc_result.event */
#define LVLIP_CC_EV_TIMEOUT   0x01u   /* step 1 cut cwnd to one mss */
#define LVLIP_CC_EV_ENTER     0x02u   /* entered fast recovery */
#define LVLIP_CC_EV_EXIT      0x04u   /* full ACK: left fast recovery */
#define LVLIP_CC_EV_SLOWSTART 0x08u   /* cwnd grew in slow start */
#define LVLIP_CC_EV_AVOID     0x10u   /* cwnd grew in congestion avoidance */

typedef struct lvlip_cc_flow {        /* one per planned reverse flow; sizeof == 32, no padding */
    uint32_t cwnd;                    /* bytes, mss .. 2^30 */
    uint32_t ssthresh;                /* bytes, 0 .. 2^30; the caller starts it at 2^30 */
    uint32_t recover;                 /* host order: snd_nxt when recovery was entered (RFC 6582) */
    uint32_t acc;                     /* bytes acknowledged since cwnd last grew in avoidance (RFC 3465 2.1) */
    uint32_t cwnd_max;                /* the caller's ceiling, mss .. 2^30 */
    uint16_t mss;                     /* 1 .. 65495 */
    uint8_t  in_rec;                  /* 0 or 1 */
    uint8_t  reserved;                /* 0 */
    uint32_t reserved2[2];            /* 0 */
} lvlip_cc_flow;

typedef struct lvlip_cc_result {      /* one per planned flow; sizeof == 16 */
    uint32_t cwnd, sacked_bytes, n_sacked, event;
} lvlip_cc_result;

/* Host only: 0 when every c[k] is a state these calls take, LVLIP_EINVAL for
 * mss == 0 or above 65495, cwnd or cwnd_max outside [mss, 2^30], ssthresh above
 * 2^30, in_rec other than 0 and 1, nonzero reserved bytes, a NULL c with
 * nflows > 0 or nflows above LVLIP_LRO_MAX_FLOWS.  The _dev form cannot look:
 * the state is in HBM; the caller checks it here before it uploads it.  Nothing
 * is written. */
int lvlip_cc_check(const lvlip_cc_flow *c, uint32_t nflows);

/* On the calling thread.  s, snd (may be NULL), prev (may be NULL), fd and
 * sacked (one byte per fd index, any alignment; may be NULL, and then fd may
 * be) are read; c, t[k].wnd_cap and res are written as above.  Returns 0, or
 * LVLIP_EINVAL with nothing written: NULL s, c, t or res with nflows > 0, NULL
 * fd with a non-NULL sacked, nflows above LVLIP_LRO_MAX_FLOWS, or a c
 * lvlip_cc_check refuses.  nflows == 0 is a no-op.  Reentrant. */
int lvlip_cc_cpu(const lvlip_snd_flow *s, const lvlip_snd_result *snd, const lvlip_rto_result *prev,
                 lvlip_cc_flow *c, lvlip_rto_flow *t, uint32_t nflows, const lvlip_frame_desc *fd,
                 const uint8_t *sacked, lvlip_cc_result *res);

/* The same bytes of c, t and res on the caller's stream (asynchronous; no
 * allocation, copy, synchronisation or LDS, no workspace beyond res): res is
 * zeroed; with a non-NULL sacked a wave per flow and chunk of its queue (a
 * queue is spread over 8 to 1024 waves by the flow count, as in lvlip_sack_dev)
 * reads one scoreboard byte per lane and the descriptor of a marked entry
 * only, and adds its sums to res[k] with one 64-bit and one 32-bit atomic add
 * (integer adds only, so the bytes do not depend on the run); then a lane per
 * flow does steps 1, 2 and 4.  All pointers are device pointers: s, c and t
 * 8-B aligned, snd, prev, fd and res 16-B aligned, sacked any alignment.  The
 * NULL and limit refusals of lvlip_cc_cpu and a misaligned pointer are
 * LVLIP_EINVAL before any HIP call (c is not looked at: lvlip_cc_check);
 * LVLIP_ENODEV without a device; a failed launch is LVLIP_EHIP
 * (lvlip_last_hip_error).  Measured: DESIGN.md section 9k. */
int lvlip_cc_dev(const lvlip_snd_flow *s, const lvlip_snd_result *snd, const lvlip_rto_result *prev,
                 lvlip_cc_flow *c, lvlip_rto_flow *t, uint32_t nflows, const lvlip_frame_desc *fd,
                 const uint8_t *sacked, lvlip_cc_result *res, void *stream);

/* ---- f2 on the device: the persist timer -------------------------------------
 *
 * When the peer advertises a window below one segment lvlip_push_* appends
 * nothing; once the queue has drained lvlip_rto_* stops its timer (steps 1 and
 * 3), and from then on nothing on the sender produces a frame.  If the one ACK
 * that reopens the window is lost the connection hangs for good.  RFC 1122
 * 4.2.2.17 makes the zero-window probe a MUST for this reason; lvlip_persist_*
 * is that timer and that probe.  The reference has no persist timer and never
 * reads the window field: like lvlip_wnd_* and lvlip_cc_*, a departure that
 * follows the RFCs.
 *
 * lvlip_persist_flow k is the persist state of flow k of the reverse plan, as
 * lvlip_rto_flow k is its retransmission timer.  The struct has no padding.
 * The caller starts a flow all zero.
 *
 * Where it sits in the loop.  Once per round, after lvlip_push_* and
 * lvlip_rto_* and before the retransmit, with the `now` lvlip_rto_* got; s and
 * w are as the push left them; out and fd_out go to the wire beside the
 * push's and the retransmit's frames.
 *
 * One call, for flow k, from the values at entry, in this fixed order:
 *   0 dead     t[k].dead set: p[k] and t[k] do not change, res[k] is all zero,
 *              fd_out[k] = {64 k, 0, 0} and no byte of out is written.
 *   1 stalled  s.nseg == 0 and w.unsent > 0 and w.wnd < min(w.unsent, w.mss):
 *              nothing is in flight (so the retransmission timer is stopped
 *              and no ACK is owed), there are bytes to send, and the window,
 *              not cap or push, keeps the first segment back.  A window of
 *              1 .. mss - 1 against a full segment counts: lvlip_push_* sends
 *              whole segments only.
 *   2 not stalled.  If p.armed: p[k] becomes all zero and t[k].dupacks = 0.
 *              The answers to probes raise n_dup in lvlip_snd_* and so dupacks
 *              in lvlip_rto_* step 1; they are not duplicate ACKs in RFC
 *              5681's sense, because no data was outstanding, and left in
 *              place they would keep step 4 there ("below 3 at entry") from
 *              ever firing for the first loss after the window reopens.
 *              Nothing else of t is ever written.  No probe; res[k] is zero.
 *   3 stalled and not armed.  armed = 1, probes = 0, interval = max(1,
 *              min(t.rto, 60000)), expires = now + interval.  No probe;
 *              res[k] = {0, interval, 0, 0}.
 *   4 stalled and armed.  The timer's test is expires < now: strict and
 *              unsigned, the test of lvlip_rto_* step 3 (src/timer.c:71).  If
 *              it holds the flow FIRES: probes += 1 (it stops at 2^32 - 1),
 *              interval = min(2 * interval, 60000) formed in 64 bits, expires =
 *              now + interval, res[k] = {1, interval, probes, snd_una - 1}.
 *              Otherwise res[k] = {0, interval, probes, 0}.  There is no
 *              cut-off: RFC 1122 requires probing for as long as the peer
 *              answers; giving up is lvlip_rto_*'s `dead` and the host's.
 * Arming and firing never happen in one call.
 *
 * The probe of a fired flow is the Linux form: zero length, seq one below
 * snd_una.  It takes no sequence space and touches no queue entry, no fd
 * region and no scoreboard byte.  It is the 54 bytes at out + 64 k; bytes
 * 54 .. 63 of the slot keep their contents.  Ethernet and IPv4 are w[k].hdr's
 * with total length htons(40), the id as given and the header checksum
 * checksum(ih, 20, 0), stored raw.  TCP is w[k].hdr's with seq = htonl(s.snd_una
 * - 1), ack_seq = htonl(f[k].rcv_nxt + lro[k].delivered) (lro may be NULL: 0),
 * window = htons(s[k].win) (the fields lvlip_push_* and lvlip_rtx_* patch),
 * byte 13 the template's with PSH and FIN cleared (what a segment that is not
 * the last gets, src/tcp_output.c:466) and csum = checksum(tcp, 20, saddr +
 * daddr + htons(6) + htons(20)) with the wrapping u32 seed of every other
 * frame writer here.  fd_out[k] = {64 k, 54, 0}; a flow that did not fire gets
 * {64 k, 0, 0} and no byte of out.
 *
 * Out of scope.  The receiver's side of a probe stays as it is: lvlip_lro_*
 * reports it as NO_DATA with rel == 0xFFFFFFFF, lvlip_ack_* answers it only
 * under LVLIP_ACK_ALL; RFC 793 says an unacceptable segment elicits an ACK, and
 * arranging that is the receiving caller's step.  Also out of scope: the
 * one-byte BSD probe, sender-side SWS override timers, advertising rcv_wnd
 * from the device.  FIN is lvlip_fin_* below ("the end of a connection"). */
#define LVLIP_PERSIST_MAX_MS 60000u
#define LVLIP_PERSIST_SLOT   64u      /* probe k is the 54 bytes at out + 64 k */

typedef struct lvlip_persist_flow {   /* one per planned reverse flow; sizeof == 16, no padding */
    uint32_t expires;                 /* meaningful while armed */
    uint32_t interval;                /* ms, 1 .. 60000 while armed, else 0 */
    uint32_t probes;                  /* probes sent since the timer was armed; saturates */
    uint8_t  armed;                   /* 0 or 1 */
    uint8_t  reserved[3];             /* 0 */
} lvlip_persist_flow;

typedef struct lvlip_persist_result { /* one per planned flow; sizeof == 16 */
    uint32_t fired, interval, probes, seq;   /* seq: the probe's sequence number, host order; 0 if none */
} lvlip_persist_result;

/* Host only: 0 when every p[k] is a state these calls take, LVLIP_EINVAL for
 * armed other than 0 and 1, nonzero reserved bytes, interval above 60000 or
 * interval 0 while armed, a NULL p with nflows > 0 or nflows above
 * LVLIP_LRO_MAX_FLOWS.  The _dev form cannot look: the state is in HBM; the
 * caller checks it here before it uploads it.  Nothing is written. */
int lvlip_persist_check(const lvlip_persist_flow *p, uint32_t nflows);

/* On the calling thread, the frame through the writer lvlip_push_cpu uses.  f,
 * lro (may be NULL), s and w are read; t[k].dupacks, p, out (64 bytes per
 * flow, any alignment), fd_out and res are written as above.  Returns 0, or
 * LVLIP_EINVAL with nothing written: NULL f, s, w, t, p, out, fd_out or res
 * with nflows > 0, nflows above LVLIP_LRO_MAX_FLOWS, or a p
 * lvlip_persist_check refuses.  nflows == 0 is a no-op.  Reentrant. */
int lvlip_persist_cpu(const lvlip_lro_flow *f, const lvlip_lro_result *lro, const lvlip_snd_flow *s,
                      const lvlip_push_flow *w, lvlip_rto_flow *t, lvlip_persist_flow *p, uint32_t nflows,
                      uint32_t now, void *out, lvlip_frame_desc *fd_out, lvlip_persist_result *res);

/* The same bytes in ONE launch on the caller's stream (asynchronous; no
 * allocation, copy, atomics, LDS, workspace or synchronisation): eight lanes
 * per flow all load the flow's words, build the 54 bytes in registers and each
 * keep one aligned 16-byte chunk of the frame, so that no byte outside it is
 * stored; the first lane stores p[k], res[k], fd_out[k] and, only when step 2
 * asks for it, the four bytes of t[k].dupacks.  All pointers are device
 * pointers: f, s, w, t and p 8-B aligned, lro, fd_out and res 16-B aligned, out
 * any alignment.  The NULL and limit refusals of lvlip_persist_cpu and a
 * misaligned pointer are LVLIP_EINVAL before any HIP call (p and w are not
 * looked at: the caller checked and planned them); LVLIP_ENODEV without a
 * device; a failed launch is LVLIP_EHIP (lvlip_last_hip_error).  Measured:
 * DESIGN.md section 9m. */
int lvlip_persist_dev(const lvlip_lro_flow *f, const lvlip_lro_result *lro, const lvlip_snd_flow *s,
                      const lvlip_push_flow *w, lvlip_rto_flow *t, lvlip_persist_flow *p, uint32_t nflows,
                      uint32_t now, void *out, lvlip_frame_desc *fd_out, lvlip_persist_result *res, void *stream);

/* ---- f1: the receive buffer --------------------------------------------------- */

/* The receiver's half of the loop, closed.  lvlip_lro_next_* only ever shrinks
 * a flow's region of `out` from its front, and the window lvlip_ack_*
 * advertises is whatever the host wrote into the template; a connection that
 * outlives its region needed a host step.  lvlip_rbuf_* is what the reference's
 * tcp_data_dequeue (src/tcp_data.c:49-85, the recv() side of tcp_data_queue)
 * and the window field of tcp_transmit_skb (src/tcp_output.c:109) do, once per
 * round: the application reads from the front of the
 * flow's buffer, the buffer is used again once what was read outweighs what is
 * left, the window that follows is advertised with RFC 1122 4.2.3.3's
 * receiver-side silly-window avoidance, and a flow whose window opened with no
 * data to acknowledge is marked as owing a window update.  So far these calls
 * have a CPU form only: the state and the plan's piece0 are laid out for a
 * device form that is not in the library yet.
 *
 * lvlip_rbuf_flow k is the buffer of flow k of the forward plan.  The buffer is
 * the cap bytes at out + base_off; f[k]'s region [out_off, out_off + rcv_wnd) is
 * its tail, the used = out_off - base_off bytes in front of it are stream bytes
 * delivered in order, and the first `head` of those the application has read.
 * Invariants against f[k], which lvlip_rbuf_plan and lvlip_rbuf_check test:
 *   base_off <= f.out_off,  f.out_off + f.rcv_wnd == base_off + cap,
 *   head <= f.out_off - base_off,  1 <= cap <= 2^30,  mss >= 1,  wscale <= 14,
 *   reserved all zero, and the buffers [base_off, base_off + cap) pairwise
 *   disjoint.
 * A fresh flow has base_off = out_off, cap = rcv_wnd, head = 0 and adv_edge =
 * rcv_nxt + rcv_wnd.  The struct has no padding.
 *
 * Where it sits in the loop.  lvlip_lro_* -> lvlip_lro_advance_carry* ->
 * lvlip_lro_next_* -> lvlip_rbuf_* -> lvlip_ack_*.  The ACK after `next` builds
 * the frame it would have built before it (above); it is given `gate` as its
 * res and the t this call patched.
 *
 * One call, for flow k, from the values at entry, in this fixed order, with
 * used = out_off - base_off and unread = used - head:
 *   1 read     r = min(nread[k], unread) (nread NULL: 0).  With a sink the r
 *              bytes at out + base_off + head are copied to sink + sink_off and
 *              sink_off += r: tcp_data_dequeue's copy.  head += r.
 *   2 live     span = the largest r_j over the blocks j < min(res[k].nsack, 4)
 *              that count under lvlip_lro_advance_carry's rule against f[k] as
 *              it stands (l < r_j <= rcv_wnd; "Carried blocks" above), 0 if
 *              none does.  live = (used - head) + span: the unread bytes and
 *              everything up to the end of the last island.
 *   3 reuse    if head > 0 and live <= head: the live bytes at base_off + head
 *              move to base_off (the two ranges cannot overlap), out_off -=
 *              head, rcv_wnd += head, head = 0.  What is copied is at most
 *              what was read since the last move, so reuse costs at most one
 *              more copy per stream byte; with live == 0 it is a rewind and
 *              copies nothing.  Islands keep their sequence numbers: res[k]'s
 *              sack[] stays valid as the next carry.
 *   4 window   edge = rcv_nxt + rcv_wnd, grow = (edge - adv_edge) mod 2^32.  If
 *              grow >= min(ceil(cap / 2), mss) then adv_edge = edge (RFC 1122
 *              4.2.3.3 with Fr = 1/2); otherwise the edge stays (RFC 793: never
 *              shrink).  a = (adv_edge - rcv_nxt) mod 2^32 are the advertised
 *              bytes; min(a >> wscale, 65535) is stored htons into bytes 48-49
 *              of t[k].hdr.  No other byte of t is written.
 *   5 update   gate[k] = all 48 bytes of res[k]; when step 4 moved the edge and
 *              res[k].placed == 0, gate[k].placed = 1, so that lvlip_ack_*
 *              without LVLIP_ACK_ALL sends the window update.  res is only read.
 * rres[k] = {r, unread and head as the call leaves them, the bytes step 3
 * moved, a, the field, LVLIP_RBUF_* bits, 0}.
 * Only f[k].out_off, f[k].rcv_wnd, p[k], t[k].hdr[48..49], gate, rres, the moved
 * bytes inside the flow's own buffer and sink are written.
 *
 * Departures from the reference.  tcp_data_dequeue frees the skbs it has
 * copied out; here the bytes that are left move to the buffer's front.  The
 * reference advertises a constant window (src/tcp_output.c:109, tcb.rcv_wnd is
 * set once) and so never shrinks or reopens one.  lvlip_snd_flow.win, the window
 * on this host's own data frames, is not written: it lives in the reverse
 * plan's index space, and copying rres[k].field there is the caller's.  The ACK
 * RFC 793 owes an unacceptable segment (a probe among them) stays the caller's
 * step, as in the persist section. */
#define LVLIP_RBUF_PIECE    16384u    /* bytes of a flow's range that make one copy piece (piece0) */
#define LVLIP_RBUF_MOVED    0x1u      /* lvlip_rbuf_result.flags: step 3 reused the buffer */
#define LVLIP_RBUF_ADVANCED 0x2u      /* step 4 moved the advertised edge */
#define LVLIP_RBUF_UPDATE   0x4u      /* step 5 raised gate.placed: a window update is owed */

typedef struct lvlip_rbuf_flow {      /* one per planned forward flow; sizeof == 48, no padding */
    uint64_t base_off;                /* start of the flow's buffer, from the out base; any alignment */
    uint64_t sink_off;                /* where the next byte read goes, from the sink base */
    uint32_t cap;                     /* bytes of the buffer, 1 .. 2^30 */
    uint32_t head;                    /* offset from base_off of the first unread byte */
    uint32_t adv_edge;                /* host order: the right edge last advertised */
    uint32_t piece0;                  /* written by lvlip_rbuf_plan: the first of the flow's copy pieces */
    uint16_t mss;                     /* >= 1: the peer's segment size, for step 4 */
    uint8_t  wscale;                  /* 0 .. 14: the shift this host announced (RFC 7323) */
    uint8_t  reserved[13];            /* 0 */
} lvlip_rbuf_flow;

typedef struct lvlip_rbuf_result {    /* one per planned flow; sizeof == 32 */
    uint32_t read, unread, head, moved, adv, field, flags, reserved;
} lvlip_rbuf_result;

/* Host only: validates p against the planned flows f (the invariants above)
 * and writes p[k].piece0 = the sum of ceil(p[j].cap / LVLIP_RBUF_PIECE) over
 * j < k, the index space the copy kernel's workgroups stride over.  Returns
 * nflows, or 0xFFFFFFFF for a broken invariant, a NULL p or f with nflows > 0,
 * nflows above LVLIP_LRO_MAX_FLOWS, more than 2^31 pieces, or no memory for the
 * overlap check, with nothing written.  *npieces (may be NULL) gets the sum
 * over all flows. */
uint32_t lvlip_rbuf_plan(lvlip_rbuf_flow *p, const lvlip_lro_flow *f, uint32_t nflows, uint64_t *npieces);

/* Host only: 0 when p is a state these calls take against f (the invariants
 * and the piece0 of lvlip_rbuf_plan), LVLIP_EINVAL otherwise and for a NULL p or
 * f with nflows > 0 or nflows above LVLIP_LRO_MAX_FLOWS, LVLIP_ENOMEM if the
 * overlap check's allocation fails.  Every call leaves a state the check
 * takes.  Nothing is written. */
int lvlip_rbuf_check(const lvlip_rbuf_flow *p, const lvlip_lro_flow *f, uint32_t nflows);

/* On the calling thread, the copies with memcpy.  res and nread (may be NULL)
 * are read; f, p, t, gate, rres, out and sink (may be NULL: what is read is
 * dropped and sink_off stays) are written as above.  gate must not be res.
 * Returns 0, or with nothing written LVLIP_EINVAL: NULL f, res, p, t, out, gate
 * or rres with nflows > 0, gate == res, nflows above LVLIP_LRO_MAX_FLOWS, or a p
 * lvlip_rbuf_check refuses (LVLIP_ENOMEM as there).  nflows == 0 is a no-op.
 * Reentrant. */
int lvlip_rbuf_cpu(lvlip_lro_flow *f, const lvlip_lro_result *res, lvlip_rbuf_flow *p, lvlip_ack_tmpl *t,
                   uint32_t nflows, const uint32_t *nread, void *out, void *sink, lvlip_lro_result *gate,
                   lvlip_rbuf_result *rres);

/* ---- the end of a connection: FIN and TIME-WAIT ------------------------------ */

/* What ends a connection in the reference: tcp_close -> tcp_queue_fin
 * (src/tcp.c:255-285, src/tcp_output.c:506-523), the fifth and the eighth check
 * of tcp_input_state (src/tcp_input.c:359-389, :417-467) and
 * tcp_enter_time_wait (src/tcp.c:402-411).  lvlip_fin_* is that state machine
 * per planned flow and round: it sees the peer's FIN in the round's records,
 * sends this host's FIN once the application has asked for it and everything
 * written has been segmented, re-sends it on a timer of its own, follows the
 * states of RFC 793 down to CLOSED and owes the ACK of the peer's FIN through
 * the `gate` mechanism of lvlip_rbuf_* above.
 *
 * lvlip_fin_flow k belongs to connection k: f[k] is its receive side, s[k],
 * w[k] and t[k] its send side, write side and retransmission timer (the
 * forward and the reverse plan of one endpoint list the connections in the
 * same order).  A fresh flow is {base = f[k].rcv_nxt, state =
 * LVLIP_TCP_ESTABLISHED, the rest 0}.  The struct has no padding.
 *
 * Where it sits in the loop.  Once per round at each endpoint: after the
 * round's lvlip_lro_* -> lvlip_lro_advance_carry* -> lvlip_lro_next_* (and
 * lvlip_rbuf_* where used), after lvlip_snd_next_*, lvlip_push_*, lvlip_rto_*
 * and lvlip_persist_*, with the `now` these got; before lvlip_ack_*, which is
 * given `gate` as its res, and before the retransmit.  rec are the round's
 * records, gin is the result lvlip_ack_* would have been given.
 *
 * One call, for flow k, from the values at entry, in this fixed order:
 *   0 dead or closed.  t[k].dead set or x.state == LVLIP_TCP_CLOSED: x.base =
 *              f.rcv_nxt and nothing else of x changes; gate[k] = gin[k],
 *              fd_out[k] = {64 k, 0, 0}, res[k] = {0, x.state, 0, 0}, no byte
 *              of out.
 *   1 FIN records.  A record counts for flow k when rec.flow == k, its status
 *              is PLACED or NO_DATA and tcp_flags & 0x01; its key is (rel +
 *              dlen) mod 2^32, the stream offset of the FIN from x.base.
 *              target = (f.rcv_nxt + gin.delivered - x.base) mod 2^32 is where
 *              the stream stands now, whether lvlip_lro_next_* has run or not.
 *              hit: some record has key == target.  again: some record has
 *              key == target - 1, a FIN already counted.  Nothing is kept
 *              across rounds: a FIN in front of a hole is ignored and the
 *              peer sends it again, as the reference's `th->fin && expected`
 *              (src/tcp_input.c:418) has it; a FIN whose hole the same batch
 *              fills IS taken, which the reference, a frame at a time, would
 *              not do.
 *   2 our FIN acknowledged.  x.state FIN_WAIT_1, CLOSING or LAST_ACK and
 *              s.snd_una == x.fin_seq + 1: ACKED.  FIN_WAIT_1 -> FIN_WAIT_2;
 *              CLOSING -> TIME_WAIT with interval = LVLIP_FIN_2MSL_MS and
 *              expires = now + interval (TCP_2MSL, src/tcp.c:410); LAST_ACK ->
 *              CLOSED.
 *   3 the peer's FIN.  hit in ESTABLISHED, FIN_WAIT_1 or FIN_WAIT_2:
 *              f[k].rcv_nxt += 1, PEER_FIN | ACK_OWED; ESTABLISHED ->
 *              CLOSE_WAIT, FIN_WAIT_1 -> CLOSING, FIN_WAIT_2 -> TIME_WAIT,
 *              armed as in step 2.  A FIN_WAIT_1 flow with hit and ACKED in
 *              one call so ends in TIME_WAIT (src/tcp_input.c:441-449).
 *              again in CLOSE_WAIT, CLOSING, LAST_ACK or TIME_WAIT: ACK_OWED,
 *              and TIME_WAIT starts its timer afresh (RFC 793; a TODO at
 *              src/tcp_input.c:463).
 *   4 close.   close[k] != 0 (close may be NULL) sets LVLIP_FIN_CLOSE_REQ in
 *              x.flags, where it stays.  With it, in ESTABLISHED or CLOSE_WAIT
 *              and with w.unsent == 0: fin_seq = s.snd_nxt, s[k].snd_nxt += 1,
 *              ESTABLISHED -> FIN_WAIT_1, CLOSE_WAIT -> LAST_ACK, interval =
 *              max(1, min(t.rto, 60000)), expires = now + interval, retries =
 *              0, SENT, and the frame below is written.  Data may still be in
 *              flight: the FIN follows the last segment on the wire.
 *   5 timers, for a flow that did not send in step 4.  In FIN_WAIT_1, CLOSING
 *              or LAST_ACK: with s.nseg > 0 the timer is held at expires =
 *              now + interval (the data's timer is lvlip_rto_*'s); otherwise,
 *              if expires < now (strict and unsigned, the test of
 *              lvlip_persist_* step 4) the frame is written again, retries +=
 *              1 (it stops at 2^32 - 1), interval = min(2 * interval, 60000)
 *              formed in 64 bits, expires = now + interval, RESENT.  In
 *              TIME_WAIT, expires < now: CLOSED, TW_DONE.
 *   6 stores.  x.base = f.rcv_nxt.  gate[k] = all 48 bytes of gin[k], with
 *              placed = 1 when ACK_OWED is set and gin.placed == 0: the
 *              unchanged lvlip_ack_* without LVLIP_ACK_ALL then sends the ACK
 *              of the FIN (ack_seq = rcv_nxt + delivered covers it).  res[k] =
 *              {events, x.state, the frame's seq or 0, x.interval}.
 *              LATE_WRITE is set when the flow ends the call in FIN_WAIT_1,
 *              FIN_WAIT_2, CLOSING, LAST_ACK or TIME_WAIT with w.unsent > 0: a
 *              write behind our FIN.  It is reported; nothing is done.
 *
 * The frame is the 54 bytes at out + 64 k, lvlip_persist_*'s slot and writer:
 * w[k].hdr with total length htons(40), both checksums as there, window =
 * htons(s[k].win), seq = htonl(x.fin_seq), ack_seq = htonl(f.rcv_nxt +
 * gin.delivered) as step 3 left rcv_nxt, and byte 13 the template's with PSH
 * cleared and FIN and ACK set: what tcp_queue_fin leaves there
 * (src/tcp_output.c:515-516).  fd_out[k] = {64 k, 54, 0}, or {64 k, 0, 0} and
 * no byte of out when no frame is written.  Bytes 54 .. 63 of a slot are never
 * written.
 *
 * Only f[k].rcv_nxt, s[k].snd_nxt, x, gate, res, fd_out and the frames are
 * written.  The FIN is no queue entry: nseg, `popped` and the scoreboard never
 * see it, and with span = snd_nxt - snd_una = 1 its ACK classes as new in
 * lvlip_snd_*.
 *
 * Departures from the reference.  tcp_close leaves a CLOSE_WAIT socket in
 * CLOSE_WAIT (src/tcp.c:278-282); here it enters LAST_ACK, as RFC 793 has it.
 * The reference takes an empty write queue for "our FIN was acknowledged" and
 * enters TIME_WAIT from CLOSING without a timer (src/tcp_input.c:360-371);
 * here the test is on snd_una and the timer is armed.  The FIN's timer is this
 * call's own: lvlip_rto_* stops with the empty queue.  lvlip_cc_* sees one
 * acknowledged byte more than was sent as data.  The sequence number on the
 * ACKs lvlip_ack_* builds is the template's: after SENT the caller's template
 * has to carry fin_seq + 1. */
#define LVLIP_TCP_ESTABLISHED 3u      /* x.state: the numbers of the reference's enum tcp_states */
#define LVLIP_TCP_FIN_WAIT_1  4u
#define LVLIP_TCP_FIN_WAIT_2  5u
#define LVLIP_TCP_CLOSED      6u
#define LVLIP_TCP_CLOSE_WAIT  7u
#define LVLIP_TCP_CLOSING     8u
#define LVLIP_TCP_LAST_ACK    9u
#define LVLIP_TCP_TIME_WAIT   10u
#define LVLIP_FIN_CLOSE_REQ   0x1u    /* x.flags: the application has closed; sticky */
#define LVLIP_FIN_MAX_MS      60000u  /* the ceiling of the FIN's interval */
#define LVLIP_FIN_2MSL_MS     60000u  /* TCP_2MSL, include/tcp.h:32 */
#define LVLIP_FIN_EV_PEER_FIN   0x01u /* res.events */
#define LVLIP_FIN_EV_ACK_OWED   0x02u
#define LVLIP_FIN_EV_SENT       0x04u
#define LVLIP_FIN_EV_RESENT     0x08u
#define LVLIP_FIN_EV_ACKED      0x10u
#define LVLIP_FIN_EV_TW_DONE    0x20u
#define LVLIP_FIN_EV_LATE_WRITE 0x40u

typedef struct lvlip_fin_flow {       /* one per connection; sizeof == 32, no padding */
    uint32_t base;                    /* f[k].rcv_nxt as the last call left it */
    uint32_t fin_seq;                 /* host order: the sequence number of our FIN */
    uint32_t expires;                 /* the running timer's deadline (FIN re-send or 2 MSL) */
    uint32_t interval;                /* ms, 0 .. 60000 */
    uint32_t retries;                 /* FIN re-sends so far; saturates */
    uint8_t  state;                   /* LVLIP_TCP_* */
    uint8_t  flags;                   /* LVLIP_FIN_CLOSE_REQ */
    uint8_t  reserved[10];            /* 0 */
} lvlip_fin_flow;

typedef struct lvlip_fin_result {     /* one per connection; sizeof == 16 */
    uint32_t events, state, seq, interval;
} lvlip_fin_result;

/* Host only, between rounds: 0 when every x[k] is a state these calls take and
 * x[k].base == f[k].rcv_nxt (every call leaves that), LVLIP_EINVAL for a state
 * that is no LVLIP_TCP_* value, nonzero reserved bytes, an interval above
 * 60000, a base that is not f[k].rcv_nxt, a NULL x or f with nflows > 0 or
 * nflows above LVLIP_LRO_MAX_FLOWS.  Nothing is written. */
int lvlip_fin_check(const lvlip_fin_flow *x, const lvlip_lro_flow *f, uint32_t nflows);

/* On the calling thread, the frame through the writer lvlip_persist_cpu uses.
 * gin, rec (may be NULL with n == 0), w, t and close (may be NULL) are read; f,
 * s, x, out (64 bytes per flow, any alignment), fd_out, gate and res are
 * written as above.  gate must not be gin.  Returns 0, or LVLIP_EINVAL with
 * nothing written: NULL f, gin, s, w, t, x, out, fd_out, gate or res with
 * nflows > 0, NULL rec with n > 0, gate == gin, nflows above
 * LVLIP_LRO_MAX_FLOWS, n above LVLIP_MAX_BATCH, or an x lvlip_fin_check would
 * refuse for its state, reserved bytes or interval (base is not tested: inside
 * a round rcv_nxt has moved on).  nflows == 0 is a no-op.  Reentrant. */
int lvlip_fin_cpu(lvlip_lro_flow *f, const lvlip_lro_result *gin, const lvlip_lro_rec *rec, uint32_t n,
                  lvlip_snd_flow *s, const lvlip_push_flow *w, const lvlip_rto_flow *t, lvlip_fin_flow *x,
                  uint32_t nflows, const uint8_t *close, uint32_t now, void *out, lvlip_frame_desc *fd_out,
                  lvlip_lro_result *gate, lvlip_fin_result *res);

/* Bytes of workspace lvlip_fin_dev needs for nflows connections: two bytes per
 * flow, in whole 16-B units, at least 16. */
size_t lvlip_fin_workspace_bytes(uint32_t nflows);

/* The same bytes on the caller's stream (asynchronous; no allocation, copy,
 * atomics, LDS or synchronisation): the workspace is cleared with a memset on
 * the stream, a lane per record marks its flow's `hit` or `again` byte (plain
 * stores of the constant 1), and eight lanes per flow run the steps, build
 * the 54 bytes in registers and each keep one aligned 16-byte chunk of the
 * frame; the first lane stores x[k], res[k], fd_out[k], gate[k] and, only when
 * they change, the four bytes of f[k].rcv_nxt and of s[k].snd_nxt.  All
 * pointers are device pointers: f, s, w, t and x 8-B aligned, gin, rec, fd_out,
 * gate, res and ws 16-B aligned, close and out any alignment; ws holds
 * lvlip_fin_workspace_bytes(nflows) bytes and its contents afterwards are
 * unspecified.  The NULL and limit refusals of lvlip_fin_cpu, a NULL ws and a
 * misaligned pointer are LVLIP_EINVAL before any HIP call (x is not looked at:
 * the caller checked it); LVLIP_ENODEV without a device; a failed launch is
 * LVLIP_EHIP (lvlip_last_hip_error).  Measured: DESIGN.md section 9o. */
int lvlip_fin_dev(lvlip_lro_flow *f, const lvlip_lro_result *gin, const lvlip_lro_rec *rec, uint32_t n,
                  lvlip_snd_flow *s, const lvlip_push_flow *w, const lvlip_rto_flow *t, lvlip_fin_flow *x,
                  uint32_t nflows, const uint8_t *close, uint32_t now, void *out, lvlip_frame_desc *fd_out,
                  lvlip_lro_result *gate, lvlip_fin_result *res, void *ws, void *stream);

/* RFC 1071 pseudo-header seed with the carries folded back (for RX verify of
 * checksums produced by RFC-correct peers). */
uint32_t lvlip_pseudo_sum_rfc(uint32_t saddr, uint32_t daddr, uint8_t proto,
                              uint16_t len);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* LVLIP_SKB_H */
