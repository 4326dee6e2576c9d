/*
 * cts_tcp_senders.h — TCP senders on the device-resident path: many connections' buffer sends written into an arena
 * of slots from a small state entry per connection, with no host descriptor per buffer.
 *
 * cts_fill (cts_engine.h) writes buffers whose offset, length and pattern offset the host has prepared one by one.
 * What a TCP sender does per send is determined by three numbers per connection: the transfer size, the buffer size
 * and the bytes already sent (ctsIOPattern.cpp:550-575, 676-697). So here a sender is a slot c of a table in device
 * memory (cts_tcp_sender_state below), as a receiver is in cts_connections.h:
 *
 *   per tick   cts_tcp_senders_send(ids, max_buffers, ...)  -> up to max_buffers buffers of every listed connection:
 *                                                              the arena's bytes, their descriptors, the entries, a
 *                                                              tick block
 *
 * and the receiving half consumes what it wrote, unchanged: cts_verify_at, cts_refview_accumulate_conns and
 * cts_conns_close (cts_connections.h) over dev_descs.
 *
 * How many buffers a tick writes is known without reading anything back: total = min(capacity, sum of w) with w =
 * min(max_buffers, ceil((transfer_bytes - bytes_sent) / buffer_size)) of the running listed connections, all of which
 * the caller knows from the settings. The receive pass's n is that total.
 *
 * Ordinals: the slots are handed out in listed order, so a caller that passes base_index to cts_verify_at and
 * advances it by the tick's total gives every connection increasing stream ordinals in stream order, which is what
 * the first-failure slots need.
 *
 * Send pacing (-RateLimit with its TcpBytesPerSecondPeriod quanta, -BurstCount / -BurstDelay) runs in the tick too:
 *
 *   per tick   cts_tcp_senders_send_paced(..., dev_pace, now_ms, ...)  -> the same, but every listed connection sends
 *                                                              what CreateNewTask's send branch
 *                                                              (ctsIOPattern.cpp:593-674) lets it send at now_ms, from
 *                                                              a 64-byte pace entry per connection; the tick block
 *                                                              ends with the time of the next deferred send
 *
 * so a rate-limited run lists every connection in every tick and its one host timer sleeps until next_due_ms.
 *
 * Out of scope:
 *   - -Buffer:[lo,hi] random buffer sizes: an entry has one buffer_size
 *   - a ring that wraps: a tick writes the slots first_slot .. first_slot + total of one flat arena
 *   - handing the slots to sockets
 *   - Pull, PushPull and Duplex: cts_tcp_exchange_send and cts_tcp_exchange_send_paced (cts_tcp_exchange.h) run all
 *     four patterns, paced or not; the two ticks of this header stay -Pattern:Push
 *
 * Conventions as cts_media_stream_servers.h: noexcept, int status, device pointers from hipMalloc, stream =
 * hipStream_t as void*. Every argument check comes before the engine is used, so a bad argument is CTS_E_INVALID with
 * nothing launched; n == 0 is CTS_OK.
 */
#ifndef CTS_TCP_SENDERS_H
#define CTS_TCP_SENDERS_H

#include <stddef.h>

#include "cts_connections.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One per connection slot, device memory, 8-byte aligned, 32 bytes. Filled by cts_tcp_sender_init on the host and
 * copied to the device by the caller; afterwards only the tick writes it. m_sendPatternOffset is not stored: the
 * reference starts it at 0 and adds every send's length mod c_bufferPatternSize, so it is bytes_sent mod 65536. */
typedef struct cts_tcp_sender_state {
    uint64_t bytes_sent;     /* TcpStatusDetails.m_bytesSent of this connection */
    uint64_t transfer_bytes; /* -Transfer */
    uint64_t buffers_sent;
    uint32_t buffer_size;    /* -Buffer */
    uint32_t finished;       /* 0 running, 1 every byte of the transfer has been sent */
} cts_tcp_sender_state;      /* 32 bytes */

/* A fresh entry. CTS_E_INVALID for a null out, transfer_bytes == 0 or buffer_size == 0. Host only. */
int cts_tcp_sender_init(uint64_t transfer_bytes, uint32_t buffer_size, cts_tcp_sender_state* out);

/* dev_codes[i] of a tick */
#define CTS_TCP_SENDER_SENT 0u     /* sent at least one buffer, more to come */
#define CTS_TCP_SENDER_FINISHED 1u /* sent the last byte of its transfer */
#define CTS_TCP_SENDER_ENDED 2u    /* finished earlier (or bytes_sent >= transfer_bytes): nothing sent */
#define CTS_TCP_SENDER_NO_ROOM 3u  /* running, but no slot was left: nothing sent */
#define CTS_TCP_SENDER_SKIPPED 4u  /* id >= n_conns, buffer_size == 0 or buffer_size > stride: nothing sent */

/* What one tick did; written (not accumulated) by the tick. 32 bytes, 8-byte aligned. */
typedef struct cts_tcp_sender_tick {
    uint64_t bytes;                /* sum of the written buffers' lengths */
    uint32_t buffers;              /* slots written: first_slot .. first_slot + buffers */
    uint32_t connections_sent;     /* connections that took at least one slot */
    uint32_t connections_finished; /* of those, how many sent their last byte */
    uint32_t connections_no_room;  /* running, but no slot was left for them */
    uint32_t connections_skipped;  /* codes 2 and 4 */
    uint32_t reserved;
} cts_tcp_sender_tick;

/* A device counter block (cts_counters_device_bytes(), cts_counters_reset) as the senders feed it: bytes_sent is the
 * TcpStatusDetails.m_bytesSent delta (ctsIOPattern.cpp:510). Laid out like cts_counters_ex: six u64. */
typedef struct cts_counters_sent {
    uint64_t bytes_sent;
    uint64_t buffers_sent;
    uint64_t connections_finished;
    uint64_t reserved[3]; /* 0 */
} cts_counters_sent;

/* Bytes of dev_scratch a tick over n listed connections needs (8-byte aligned device memory; its content means
 * nothing between ticks, and two ticks in flight on different streams need one each). */
size_t cts_tcp_senders_scratch_bytes(uint32_t n);

/* One tick: up to max_buffers buffers of each of the distinct connections dev_conn_ids[0..n), in listed order. For c =
 * dev_conn_ids[i] with entry E = dev_senders[c], B = E.buffer_size and R = E.transfer_bytes - E.bytes_sent:
 *   c >= n_conns, B == 0 or B > stride          nothing sent, E untouched (code 4)
 *   E.finished != 0 (or R <= 0)                 nothing sent, E untouched (code 2)
 *   otherwise the connection wants w = min(max_buffers, ceil(R / B)) consecutive slots (64-bit arithmetic), handed
 *   out by an exclusive prefix sum (64-bit) p over the listed order, and takes t = min(w, capacity - min(p, capacity))
 *   of them. p only grows, so at most one connection per tick takes fewer slots than it wants and more than none, and
 *   every running connection listed after it takes none (code 3, E untouched). Buffer j < t goes to tick-local slot
 *   g = p + j, arena slot first_slot + g:
 *     the bytes P[(E.bytes_sent + j B + x) mod 65536] for x < len, len = min(B, R - j B): byte for byte what cts_fill
 *     writes for the descriptor
 *     dev_descs[g] = {byte_offset = (first_slot + g) x stride, length = len, expected_pattern_offset =
 *                     (E.bytes_sent + j B) mod 65536, conn_index = c, skip_head = 0}
 *   then E.bytes_sent += the taken bytes, E.buffers_sent += t, and E.finished = 1 once bytes_sent == transfer_bytes
 *   (code 1, else 0).
 * The written slots are first_slot .. first_slot + total with no gap, total = min(capacity, sum of w) =
 * tick.buffers. Nothing else is written: not the bytes between a buffer's end and the next slot, not the slots from
 * total on, not dev_descs[total .. capacity).
 *
 * dev_descs is required: `capacity` elements, 8-byte aligned. It is what the receive half consumes: cts_verify_at,
 * cts_refview_accumulate_conns and cts_conns_close run over it unchanged. dev_codes[i] (n elements, may be NULL) takes
 * the code, dev_tick (may be NULL) the tick block. dev_sent_counters (may be NULL) is a cts_counters_sent block: it
 * takes the tick's bytes, buffers and finished connections.
 *
 * Arguments: stride a multiple of 16 in [16, 16 MiB]; dev_arena non-null and 16-byte aligned; (first_slot + capacity)
 * x stride <= arena_bytes with no wrap-around; max_buffers >= 1; dev_conn_ids non-null; dev_senders non-null when
 * n_conns != 0; dev_descs non-null (whatever the capacity); dev_senders, dev_descs, dev_tick, dev_sent_counters and
 * dev_scratch 8-byte aligned, dev_conn_ids and dev_codes 4-byte; dev_scratch non-null with scratch_bytes >=
 * cts_tcp_senders_scratch_bytes(n) (CTS_E_INVALID otherwise, nothing launched).
 * Ordering: on one stream, a tick's outputs are ready for the receive pass that follows. Two ticks listing the same
 * connection must be stream-ordered. A connection listed twice in one tick is the caller's error (its entry is then
 * undefined; no write leaves the entries, the capacity's slots or the output arrays). */
int cts_tcp_senders_send(cts_engine* engine, void* dev_arena, uint64_t arena_bytes, uint32_t stride,
                         uint64_t first_slot, uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n,
                         uint32_t max_buffers, cts_tcp_sender_state* dev_senders, uint32_t n_conns,
                         cts_buf_desc* dev_descs, uint32_t* dev_codes, cts_tcp_sender_tick* dev_tick,
                         void* dev_sent_counters, void* dev_scratch, size_t scratch_bytes, void* stream);

/* ---- send pacing ---------------------------------------------------------------------------------------------------
 * One per connection slot, device memory, 8-byte aligned, 64 bytes: a table parallel to dev_senders. Filled by
 * cts_tcp_sender_pace_init on the host and copied to the device by the caller; afterwards only the paced tick writes
 * it. The members are CreateNewTask's pacing state (ctsIOPattern.h:204-205, 273-275) plus the one send that a task
 * with a time offset leaves waiting. */
typedef struct cts_tcp_sender_pace {
    int64_t bytes_per_quantum;  /* m_bytesSendingPerQuantum = bytes_per_second x period_ms / 1000; 0 = no rate limit */
    int64_t bytes_this_quantum; /* m_bytesSendingThisQuantum */
    int64_t quantum_start_ms;   /* m_quantumStartTimeMs */
    int64_t due_ms;             /* when the pending send may go out; meaningful only while pending != 0 */
    uint32_t quantum_period_ms; /* TcpBytesPerSecondPeriod */
    uint32_t burst_count;       /* -BurstCount, the setting; 0 = none */
    uint32_t burst_left;        /* m_burstCount */
    uint32_t burst_delay_ms;    /* -BurstDelay */
    uint32_t pending;           /* 1: a task has been created whose send waits for due_ms */
    uint32_t reserved[3];       /* 0 */
} cts_tcp_sender_pace;          /* 64 bytes */

/* A fresh pace entry whose first quantum starts at start_ms. period_ms == 0 means 100. A rate whose bytes per quantum
 * come to 0 leaves the burst settings in charge; otherwise a rate limit takes precedence over them
 * (ctsIOPattern.cpp:593, 657). CTS_E_INVALID for a null out, a negative start_ms, or bytes_per_second x period_ms that
 * does not fit an int64. Host only. */
int cts_tcp_sender_pace_init(uint64_t bytes_per_second, uint32_t period_ms, uint32_t burst_count,
                             uint32_t burst_delay_ms, int64_t start_ms, cts_tcp_sender_pace* out);

#define CTS_TCP_SENDER_WAITING 5u /* running, but pacing lets no send out at now_ms: nothing sent */

/* What one paced tick did. 48 bytes, 8-byte aligned. Its first 32 bytes are the plain tick's block. */
typedef struct cts_tcp_sender_paced_tick {
    cts_tcp_sender_tick tick;
    int64_t next_due_ms;          /* the smallest due_ms of the listed running connections (codes 0, 1, 3 and 5) that
                                     the tick leaves with pending != 0; INT64_MAX when there is none: the one number a
                                     host timer needs */
    uint32_t connections_waiting; /* code 5 */
    uint32_t connections_pending; /* the listed running connections left with pending != 0, those that sent included */
} cts_tcp_sender_paced_tick;

/* Bytes of dev_scratch a paced tick over n listed connections needs (the plain tick's, with the larger tick block). */
size_t cts_tcp_senders_paced_scratch_bytes(uint32_t n);

/* One paced tick at the time now_ms: cts_tcp_senders_send, with every listed running connection's wanted slots cut to
 * what its pace entry Q = dev_pace[c] lets out. Let step(now, size) be CreateNewTask's send branch
 * (ctsIOPattern.cpp:593-674) over Q: it moves the quantum or the burst count and returns the task's time offset. With
 * limit = min(max_buffers, ceil(R / B)):
 *
 *   run(cap):  count = 0
 *     while count < cap:
 *         if Q.pending:  if now_ms < Q.due_ms: break;  Q.pending = 0            the waiting send goes out first
 *         else:          off = step(now_ms, min(B, R - count B))
 *                        if off > 0: Q.pending = 1; Q.due_ms = now_ms + off; break   task created, send deferred
 *         count += 1
 *     return count
 *
 * This models a caller that stops asking a connection for tasks once one has come back with a time offset, until that
 * send has gone out: the reference's scheduler would go on and queue further timers, which needs a timer per task.
 *
 * The connection wants w = run(limit) slots; p and t are the plain tick's (t = min(w, capacity - min(p, capacity))):
 *   w == 0                       nothing sent (code 5), E untouched, Q as run(limit) leaves it (a first step may
 *                                have created the pending task)
 *   w > 0, t == 0                nothing sent (code 3), E and Q untouched
 *   0 < t < w                    t buffers sent, Q as run(t) leaves it (no task beyond the t-th is created)
 *   t == w                       w buffers sent, Q as run(limit) leaves it
 * Codes 0-4, the buffers' bytes, the descriptors, E's update, the sent block and the no-gap rule are the plain tick's;
 * tick.buffers = min(capacity, sum of w). Connections with codes 2 and 4 have neither entry read past what decides
 * the code, and do not count for next_due_ms or connections_pending. A table whose pace entries all have
 * bytes_per_quantum == 0, burst_count == 0 and pending == 0 gives, byte for byte and field for field, what
 * cts_tcp_senders_send gives.
 *
 * Arguments: cts_tcp_senders_send's, and dev_pace non-null when n_conns != 0 and 8-byte aligned, n_conns entries;
 * now_ms >= 0; dev_tick (may be NULL) a cts_tcp_sender_paced_tick; scratch_bytes >=
 * cts_tcp_senders_paced_scratch_bytes(n). The caller's duties: now_ms does not decrease from tick to tick of a table
 * and stays below 2^62, and bytes_per_quantum x the quanta a tick skips fits an int64; a pace entry comes from
 * cts_tcp_sender_pace_init. Outside them the values of the pace entries, the wanted counts and the tick's tail are
 * unspecified, but no write leaves the entries, the capacity's slots or the output arrays. */
int cts_tcp_senders_send_paced(cts_engine* engine, void* dev_arena, uint64_t arena_bytes, uint32_t stride,
                               uint64_t first_slot, uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n,
                               uint32_t max_buffers, cts_tcp_sender_state* dev_senders, cts_tcp_sender_pace* dev_pace,
                               uint32_t n_conns, int64_t now_ms, cts_buf_desc* dev_descs, uint32_t* dev_codes,
                               cts_tcp_sender_paced_tick* dev_tick, void* dev_sent_counters, void* dev_scratch,
                               size_t scratch_bytes, void* stream);

/* The three counter reads over sent blocks: the same fold, and for the all-reduce the same ncclAllReduce of count 6,
 * with the six words named as cts_counters_sent. */
int cts_counters_read_sent(cts_engine* engine, const void* dev_sent_counters, cts_counters_sent* out, void* stream);
int cts_counters_read_multi_sent(cts_engine* const* engines, const void* const* dev_sent_counters,
                                 void* const* streams, uint32_t n, cts_counters_sent* out);
int cts_counters_allreduce_sent(cts_engine* const* engines, const void* const* dev_sent_counters,
                                void* const* streams, uint32_t n, cts_counters_sent* out);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* CTS_TCP_SENDERS_H */
