/*
 * flow_step.h — one flow's step of the protocol state machines, once for both
 * sides: the retransmission timer, the congestion window, the peer's window,
 * the push count, the class of an ACK, the persist timer, the receive buffer
 * and the connection's close.  The CPU forms (rto_cpu.c, cc_cpu.c, push_cpu.c,
 * snd_cpu.c, persist_cpu.c, rbuf_cpu.c, fin_cpu.c) call these on the flow in
 * the caller's array, the kernels (rto_, cc_, push_, snd_, persist_ and
 * fin_kernels.hip) on a flow in registers; the receive buffer has no kernel
 * yet.
 * Every function takes scalars and one flow; none sees a batch.  How a flow's
 * words travel between HBM and registers, which lane runs the step and what is
 * reduced around it stays in the kernels.  Plain C99, not installed.
 */
#ifndef LVLIP_FLOW_STEP_H
#define LVLIP_FLOW_STEP_H

#include <stdint.h>

#include "lvlip_skb.h"

#ifdef __HIPCC__
#define FLOW_FN __host__ __device__ __forceinline__
#else
#define FLOW_FN static inline
#endif

#define FLOW_NONE 0xFFFFFFFFu    /* no flow, no queue entry, no sample, no winner; a plan's refusal */
#define FLOW_WND_MAX 0x40000000u /* the largest window: 0xFFFF << 14 is below it (RFC 7323 2.3) */

#define FLOW_ACK_NEW 0u    /* src/tcp_input.c:330-331: snd_una only ever rises */
#define FLOW_ACK_DUP 1u
#define FLOW_ACK_OLD 2u    /* :338 */
#define FLOW_ACK_BEYOND 3u /* :343 */

/* The fifth check (src/tcp_input.c:311-356) on d = ack_seq - snd_una against
 * span = snd_nxt - snd_una, both mod 2^32.  The classes are numbered in the
 * order of lvlip_snd_result's counters (n_new, n_dup, n_old, n_beyond), which
 * k_snd_rec indexes with them.  A record counts for the window when its class
 * is at most FLOW_ACK_DUP, which is d <= span. */
FLOW_FN uint32_t flow_ack_class(uint32_t d, uint32_t span)
{
    return d == 0u ? FLOW_ACK_DUP : d <= span ? FLOW_ACK_NEW : d >= 0x80000000u ? FLOW_ACK_OLD : FLOW_ACK_BEYOND;
}

/* the window field raw of the winning ACK as bytes; the mask is a no-op for a
 * wscale lvlip_rto_check accepts and keeps the shift defined for any other */
FLOW_FN uint32_t flow_wnd_scale(uint32_t raw, uint32_t wscale)
{
    const uint64_t v = (uint64_t)raw << (wscale & 15u);
    return v > FLOW_WND_MAX ? FLOW_WND_MAX : (uint32_t)v;
}

/* LVLIP_WND_APPLY: what the write queue may have in flight */
FLOW_FN uint32_t flow_wnd_apply(uint32_t snd_wnd, uint32_t wnd_cap) { return snd_wnd < wnd_cap ? snd_wnd : wnd_cap; }

typedef struct flow_rto_out {
    uint32_t fired;  /* 0, LVLIP_RTO_TIMEOUT or LVLIP_RTO_FASTRTX */
    uint32_t sample; /* the round-trip sample in ms, FLOW_NONE when none was taken */
} flow_rto_out;

/* Steps 1-4 of lvlip_rto_* on *x, for a queue of nseg entries of which this
 * round pushed the last `pushed`, n_new new and n_dup duplicate ACKs, at time
 * now.  A dead flow is left as it is. */
FLOW_FN flow_rto_out flow_rto_step(lvlip_rto_flow *x, uint32_t nseg, uint32_t pushed, uint32_t n_new, uint32_t n_dup,
                                   uint32_t now, uint32_t flags)
{
    flow_rto_out o = {0u, FLOW_NONE};
    if (x->dead) return o;
    if (pushed > nseg) pushed = nseg;
    const uint32_t before = nseg - pushed;
    const uint32_t dup0 = x->dupacks;
    if (n_new) { /* src/tcp_input.c:330-334: tcp_rtt, then tcp_clean_rto_queue */
        if (x->backoff == 0 && x->armed) { /* Karn, src/tcp.c:426 */
            const int32_t r = (int32_t)(now - (x->expires - x->rto));
            if (r >= 0) {
                /* tcp_rtt, src/tcp.c:431-451.  The integer forms equal the reference's double arithmetic (include/
                 * lvlip_skb.h); 64-bit intermediates, so no product overflows whatever state the caller hands in. */
                o.sample = (uint32_t)r;
                if (!x->srtt) { /* RFC 6298 2.2 */
                    x->srtt = r;
                    x->rttvar = r / 2;
                } else { /* 2.3 */
                    const int64_t e = (int64_t)x->srtt - r;
                    x->rttvar = (int32_t)(uint32_t)(uint64_t)((3 * (int64_t)x->rttvar + (e < 0 ? -e : e)) / 4);
                    x->srtt = (int32_t)(uint32_t)(uint64_t)((7 * (int64_t)x->srtt + r) / 8);
                }
                int64_t k = 4 * (int64_t)x->rttvar;
                if (k < 200) k = 200; /* :449 */
                x->rto = (uint32_t)(uint64_t)(x->srtt + k);
            }
        }
        x->dupacks = 0;
        if (before == 0) x->armed = 0, x->backoff = 0; /* tcp_stop_rto_timer, src/tcp_input.c:86-89 */
    } else {
        x->dupacks += n_dup;
    }
    if (pushed && before == 0) { /* src/tcp_output.c:138-140 */
        x->armed = 1;
        x->expires = now + x->rto;
    }
    if (x->armed && x->expires < now) { /* src/timer.c:71 */
        if (nseg == 0) { /* src/tcp_output.c:371-375 */
            x->armed = 0, x->backoff = 0;
        } else {
            o.fired = LVLIP_RTO_TIMEOUT;
            if (x->rto > LVLIP_RTO_DEAD_MS) { /* :384-391; tcp_done stops the timer, src/tcp.c:313-334 */
                x->dead = 1, x->armed = 0, x->backoff = 0;
            } else { /* :394-396 */
                x->rto *= 2u;
                x->backoff++;
                x->expires = now + x->rto;
            }
        }
    }
    if ((flags & LVLIP_RTO_FAST) && !o.fired && dup0 < 3u && x->dupacks >= 3u && nseg) o.fired = LVLIP_RTO_FASTRTX;
    return o;
}

/* Steps 1 and 2 of lvlip_cc_* on *x of a live flow: the cut after the loss the
 * last lvlip_rto_* call reported (fired, backoff), then the round's n_new new
 * ACKs for `acked` bytes.  Returns the LVLIP_CC_EV_* bits. */
FLOW_FN uint32_t flow_cc_step(lvlip_cc_flow *x, uint32_t una, uint32_t nxt, uint32_t acked, uint32_t n_new,
                              uint32_t fired, uint32_t backoff)
{
    const uint32_t mss = x->mss, flight = nxt - una;
    const uint32_t half = flight / 2u > 2u * mss ? flight / 2u : 2u * mss;
    uint32_t event = 0;
    /* 1: loss */
    if (fired == LVLIP_RTO_TIMEOUT) {
        if (backoff == 1u) x->ssthresh = half;
        x->cwnd = mss, x->acc = 0, x->in_rec = 0, x->recover = nxt;
        event |= LVLIP_CC_EV_TIMEOUT;
    } else if (fired == LVLIP_RTO_FASTRTX && !x->in_rec) {
        x->ssthresh = half, x->cwnd = half, x->acc = 0, x->in_rec = 1, x->recover = nxt;
        event |= LVLIP_CC_EV_ENTER;
    }
    /* 2: ACKs */
    if (n_new && acked) {
        uint64_t cwnd = x->cwnd;
        if (x->in_rec) {
            if (acked >= (uint32_t)(x->recover - una)) {
                x->in_rec = 0, x->acc = 0;
                cwnd = x->ssthresh;
                event |= LVLIP_CC_EV_EXIT;
            }
        } else if (cwnd < x->ssthresh) {
            const uint64_t cap = (uint64_t)n_new * mss;
            cwnd += acked < cap ? acked : cap;
            event |= LVLIP_CC_EV_SLOWSTART;
        } else {
            uint64_t acc = (uint64_t)x->acc + acked;
            if (acc >= cwnd) {
                acc -= cwnd;
                cwnd += mss;
                event |= LVLIP_CC_EV_AVOID;
            }
            x->acc = (uint32_t)(acc < cwnd ? acc : cwnd);
        }
        x->cwnd = (uint32_t)(cwnd < x->cwnd_max ? cwnd : x->cwnd_max);
    }
    return event;
}

/* Step 4: wnd_cap from cwnd and the pipe sum of step 3; *bytes gets the sum as
 * the result reports it.  Both stop at LVLIP_CC_MAX_WND. */
FLOW_FN uint32_t flow_cc_cap(uint32_t cwnd, uint64_t sum, uint32_t *bytes)
{
    *bytes = sum < LVLIP_CC_MAX_WND ? (uint32_t)sum : LVLIP_CC_MAX_WND;
    const uint64_t cap = (uint64_t)cwnd + *bytes;
    return cap < LVLIP_CC_MAX_WND ? (uint32_t)cap : LVLIP_CC_MAX_WND;
}

/* Step 2 of lvlip_push_*: the segments flow *w may append now to the queue *s,
 * and their payload bytes.  The device cannot refuse its input, so a zero mss
 * and a queue that is not the plan's (longer than cap, or below q0) push
 * nothing.  For a flow lvlip_push_plan accepted, whose queue step 1 has moved
 * to q0 or will, these guards always hold: mss > 0, nseg <= cap and
 * seg0 >= q0. */
FLOW_FN uint32_t flow_push_count(const lvlip_push_flow *w, const lvlip_snd_flow *s, uint32_t *bytes)
{
    const uint32_t unsent = w->unsent, mss = w->mss, wnd = w->wnd, push = w->push;
    const uint32_t span = s->snd_nxt - s->snd_una;
    const uint32_t need = mss ? (uint32_t)(((uint64_t)unsent + mss - 1u) / mss) : 0u;
    uint32_t m = s->nseg < w->cap && (s->seg0 >= w->q0 || s->nseg == 0u) ? w->cap - s->nseg : 0u;
    if (push < m) m = push;
    if (need < m) m = need;
    /* span + min(m*mss, unsent) <= wnd: everything that is ready fits, or whole segments of the room */
    const uint32_t room = span <= wnd ? wnd - span : 0u;
    const uint32_t fit = span <= wnd && unsent <= room ? need : (mss ? room / mss : 0u);
    if (fit < m) m = fit;
    const uint64_t b = (uint64_t)m * mss;
    *bytes = b < unsent ? (uint32_t)b : unsent;
    return m;
}

typedef struct flow_persist_out {
    uint32_t fired;    /* 0 or 1: a probe goes out */
    uint32_t interval; /* lvlip_persist_result's interval and probes */
    uint32_t probes;
    uint32_t clear; /* 0 or 1: the timer's dupacks are to be zeroed */
} flow_persist_out;

/* Steps 0-4 of lvlip_persist_* on *x, for a flow whose queue holds nseg
 * entries, whose write side has `unsent` bytes ready, a window of wnd and
 * segments of mss, and whose retransmission timer stands at rto (and is dead
 * or not), at time now.  A dead flow is left as it is. */
FLOW_FN flow_persist_out flow_persist_step(lvlip_persist_flow *x, uint32_t dead, uint32_t nseg, uint32_t unsent,
                                           uint32_t wnd, uint32_t mss, uint32_t rto, uint32_t now)
{
    flow_persist_out o = {0u, 0u, 0u, 0u};
    if (dead) return o;
    const uint32_t first = unsent < mss ? unsent : mss; /* the segment lvlip_push_* would send next */
    if (!(nseg == 0u && unsent > 0u && wnd < first)) {  /* 2: not stalled */
        if (x->armed) {
            x->expires = 0u, x->interval = 0u, x->probes = 0u;
            x->armed = 0, x->reserved[0] = 0, x->reserved[1] = 0, x->reserved[2] = 0;
            o.clear = 1u; /* the answers to probes are no duplicate ACKs of RFC 5681 */
        }
        return o;
    }
    if (!x->armed) { /* 3: the timer starts; the first probe waits one interval */
        const uint32_t iv = rto < LVLIP_PERSIST_MAX_MS ? rto : LVLIP_PERSIST_MAX_MS;
        x->armed = 1, x->probes = 0u;
        x->interval = iv ? iv : 1u;
        x->expires = now + x->interval;
    } else if (x->expires < now) { /* 4: src/timer.c:71, as flow_rto_step */
        const uint64_t twice = 2ull * x->interval;
        o.fired = 1u;
        if (x->probes != 0xFFFFFFFFu) x->probes++;
        x->interval = twice < LVLIP_PERSIST_MAX_MS ? (uint32_t)twice : LVLIP_PERSIST_MAX_MS;
        x->expires = now + x->interval;
    }
    o.interval = x->interval, o.probes = x->probes;
    return o;
}

typedef struct flow_rbuf_out {
    uint32_t read, unread, moved, adv, field, flags; /* lvlip_rbuf_result's; head is x->head */
    uint32_t rd_from;                                /* the read's source, from base_off; its length is `read` */
    uint32_t mv_from;                                /* the move's source, from base_off; its length is `moved` */
    uint64_t rd_to;                                  /* the read's destination, from the sink base */
} flow_rbuf_out;

/* step 2's largest right edge so far, with block b if it is reported and counts
 * (constant indices at the call: a kernel keeps the blocks in registers) */
FLOW_FN uint32_t flow_rbuf_span(uint32_t span, lvlip_lro_sack b, int reported, uint32_t rcv_nxt, uint32_t rcv_wnd)
{
    const uint32_t l = b.left - rcv_nxt, r = b.right - rcv_nxt;
    return reported && l < r && r <= rcv_wnd && r > span ? r : span;
}

/* Steps 1-4 of lvlip_rbuf_* and step 5's verdict on *x, for a flow whose
 * region starts at *out_off with *rcv_wnd bytes and wants rcv_nxt, whose
 * application asks for nread bytes (into a sink or not) and whose last result
 * has the islands sack[0 .. nsack) and `placed` frames.  For a state
 * lvlip_rbuf_check accepts used <= cap and head <= used; a block counts only
 * when it ends inside rcv_wnd, so head + live <= cap whatever the islands say:
 * both copies stay inside the flow's buffer. */
FLOW_FN flow_rbuf_out flow_rbuf_step(lvlip_rbuf_flow *x, uint64_t *out_off, uint32_t *rcv_wnd, uint32_t rcv_nxt,
                                     uint32_t nread, uint32_t have_sink, const lvlip_lro_sack *sack, uint32_t nsack,
                                     uint32_t placed)
{
    flow_rbuf_out o = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const uint32_t used = (uint32_t)(*out_off - x->base_off);
    /* 1: read (tcp_data_dequeue's copy, src/tcp_data.c:49-85) */
    const uint32_t unread = used - x->head;
    o.read = nread < unread ? nread : unread;
    o.rd_from = x->head, o.rd_to = x->sink_off;
    if (have_sink) x->sink_off += o.read;
    x->head += o.read;
    o.unread = used - x->head;
    /* 2: live bytes, the carried blocks under lvlip_lro_advance_carry's rule */
    uint32_t span = 0;
    span = flow_rbuf_span(span, sack[0], nsack > 0u, rcv_nxt, *rcv_wnd);
    span = flow_rbuf_span(span, sack[1], nsack > 1u, rcv_nxt, *rcv_wnd);
    span = flow_rbuf_span(span, sack[2], nsack > 2u, rcv_nxt, *rcv_wnd);
    span = flow_rbuf_span(span, sack[3], nsack > 3u, rcv_nxt, *rcv_wnd);
    const uint64_t live = (uint64_t)o.unread + span;
    /* 3: reuse */
    if (x->head > 0u && live <= x->head) {
        o.moved = (uint32_t)live, o.mv_from = x->head;
        *out_off -= x->head, *rcv_wnd += x->head;
        x->head = 0u;
        o.flags |= LVLIP_RBUF_MOVED;
    }
    /* 4: window (RFC 1122 4.2.3.3, Fr = 1/2; RFC 793: the edge never moves left) */
    const uint32_t edge = rcv_nxt + *rcv_wnd;
    const uint32_t half = x->cap / 2u + (x->cap & 1u);
    if ((uint32_t)(edge - x->adv_edge) >= (half < x->mss ? half : x->mss)) {
        x->adv_edge = edge;
        o.flags |= LVLIP_RBUF_ADVANCED;
        if (placed == 0u) o.flags |= LVLIP_RBUF_UPDATE; /* 5 */
    }
    o.adv = x->adv_edge - rcv_nxt;
    const uint32_t fld = o.adv >> (x->wscale & 15u);
    o.field = fld < 65535u ? fld : 65535u;
    return o;
}

typedef struct flow_fin_out {
    uint32_t events;  /* LVLIP_FIN_EV_* */
    uint32_t frame;   /* 0 or 1: the FIN goes out, with sequence number x->fin_seq */
    uint32_t rcv_nxt; /* the receive side's rcv_nxt as step 3 leaves it */
    uint32_t snd_nxt; /* the send side's snd_nxt as step 4 leaves it */
    uint32_t interval; /* lvlip_fin_result's interval: 0 from step 0 */
} flow_fin_out;

/* our FIN is out and the connection is not yet over */
FLOW_FN int flow_fin_sent(uint32_t state)
{
    return state == LVLIP_TCP_FIN_WAIT_1 || state == LVLIP_TCP_FIN_WAIT_2 || state == LVLIP_TCP_CLOSING ||
           state == LVLIP_TCP_LAST_ACK || state == LVLIP_TCP_TIME_WAIT;
}

/* Steps 0 and 2-5 of lvlip_fin_* on *x and step 6's x.base, for a connection
 * whose receive side wants rcv_nxt, whose send side stands at snd_una ..
 * snd_nxt with nseg queue entries and `unsent` bytes not yet segmented, whose
 * retransmission timer stands at rto (and is dead or not), whose records of
 * this round hold the peer's FIN at the stream's end (hit) or one byte before
 * it (again), and whose application has closed or not, at time now. */
FLOW_FN flow_fin_out flow_fin_step(lvlip_fin_flow *x, uint32_t dead, uint32_t rcv_nxt, uint32_t snd_una,
                                   uint32_t snd_nxt, uint32_t nseg, uint32_t unsent, uint32_t rto, uint32_t hit,
                                   uint32_t again, uint32_t close, uint32_t now)
{
    flow_fin_out o = {0u, 0u, rcv_nxt, snd_nxt, 0u};
    x->base = rcv_nxt;
    if (dead || x->state == LVLIP_TCP_CLOSED) return o; /* 0 */
    uint32_t st = x->state;
    /* 2: our FIN acknowledged (src/tcp_input.c:359-376) */
    if ((st == LVLIP_TCP_FIN_WAIT_1 || st == LVLIP_TCP_CLOSING || st == LVLIP_TCP_LAST_ACK) &&
        snd_una == x->fin_seq + 1u) {
        o.events |= LVLIP_FIN_EV_ACKED;
        if (st == LVLIP_TCP_FIN_WAIT_1) {
            st = LVLIP_TCP_FIN_WAIT_2;
        } else if (st == LVLIP_TCP_CLOSING) {
            st = LVLIP_TCP_TIME_WAIT;
            x->interval = LVLIP_FIN_2MSL_MS, x->expires = now + LVLIP_FIN_2MSL_MS; /* src/tcp.c:410 */
        } else {
            st = LVLIP_TCP_CLOSED;
        }
    }
    /* 3: the peer's FIN (src/tcp_input.c:417-467) */
    if (hit && (st == LVLIP_TCP_ESTABLISHED || st == LVLIP_TCP_FIN_WAIT_1 || st == LVLIP_TCP_FIN_WAIT_2)) {
        o.rcv_nxt = rcv_nxt + 1u; /* :429 */
        o.events |= LVLIP_FIN_EV_PEER_FIN | LVLIP_FIN_EV_ACK_OWED;
        if (st == LVLIP_TCP_ESTABLISHED) {
            st = LVLIP_TCP_CLOSE_WAIT;
        } else if (st == LVLIP_TCP_FIN_WAIT_1) {
            st = LVLIP_TCP_CLOSING;
        } else {
            st = LVLIP_TCP_TIME_WAIT;
            x->interval = LVLIP_FIN_2MSL_MS, x->expires = now + LVLIP_FIN_2MSL_MS;
        }
    }
    if (again && (st == LVLIP_TCP_CLOSE_WAIT || st == LVLIP_TCP_CLOSING || st == LVLIP_TCP_LAST_ACK ||
                  st == LVLIP_TCP_TIME_WAIT)) {
        o.events |= LVLIP_FIN_EV_ACK_OWED;
        if (st == LVLIP_TCP_TIME_WAIT) x->interval = LVLIP_FIN_2MSL_MS, x->expires = now + LVLIP_FIN_2MSL_MS;
    }
    x->base = o.rcv_nxt;
    /* 4: close (tcp_close, src/tcp.c:271-282; tcp_queue_fin) */
    if (close) x->flags |= (uint8_t)LVLIP_FIN_CLOSE_REQ;
    if ((x->flags & LVLIP_FIN_CLOSE_REQ) && (st == LVLIP_TCP_ESTABLISHED || st == LVLIP_TCP_CLOSE_WAIT) &&
        unsent == 0u) {
        const uint32_t iv = rto < LVLIP_FIN_MAX_MS ? rto : LVLIP_FIN_MAX_MS;
        x->fin_seq = snd_nxt;
        o.snd_nxt = snd_nxt + 1u; /* src/tcp_output.c:150 */
        st = st == LVLIP_TCP_ESTABLISHED ? LVLIP_TCP_FIN_WAIT_1 : LVLIP_TCP_LAST_ACK;
        x->interval = iv ? iv : 1u;
        x->expires = now + x->interval;
        x->retries = 0u;
        o.events |= LVLIP_FIN_EV_SENT;
        o.frame = 1u;
    } else if (st == LVLIP_TCP_FIN_WAIT_1 || st == LVLIP_TCP_CLOSING || st == LVLIP_TCP_LAST_ACK) { /* 5 */
        if (nseg > 0u) {
            x->expires = now + x->interval;
        } else if (x->expires < now) { /* src/timer.c:71, as flow_persist_step */
            const uint64_t twice = 2ull * x->interval;
            if (x->retries != 0xFFFFFFFFu) x->retries++;
            x->interval = twice < LVLIP_FIN_MAX_MS ? (uint32_t)twice : LVLIP_FIN_MAX_MS;
            x->expires = now + x->interval;
            o.events |= LVLIP_FIN_EV_RESENT;
            o.frame = 1u;
        }
    } else if (st == LVLIP_TCP_TIME_WAIT && x->expires < now) {
        st = LVLIP_TCP_CLOSED;
        o.events |= LVLIP_FIN_EV_TW_DONE;
    }
    if (flow_fin_sent(st) && unsent > 0u) o.events |= LVLIP_FIN_EV_LATE_WRITE;
    x->state = (uint8_t)st;
    o.interval = x->interval;
    return o;
}

#endif
