/*
 * cts_tcp_exchange.h — all four TCP patterns on the device-resident path: Push, Pull, PushPull and Duplex connections
 * whose buffers, in both directions, a tick writes into an arena of slots from a small state entry per connection,
 * with no host descriptor per buffer and no host decision about whose turn it is.
 *
 * cts_tcp_senders_send (cts_tcp_senders.h) runs a one-way stream. Here a connection has two directions, d = 0 client
 * -> server and d = 1 server -> client, and each direction is a stream of its own: its pattern offset is that
 * direction's bytes sent mod 65536 (m_sendPatternOffset of the sending side, m_recvPatternOffset of the other). With
 * the buffer size B, the transfer T and the pattern, the connection's buffers form one fixed sequence m = 0 .. N-1:
 *
 *   Push      every buffer has d = 0 and len = min(B, bytes left)                 (ctsIOPattern.cpp:849-893)
 *   Pull      every buffer has d = 1 and the same len                             (ctsIOPattern.cpp:796-840)
 *   PushPull  segments of P (-PushBytes, d = 0) and Q (-PullBytes, d = 1) bytes alternate, push first; len = min(B,
 *             bytes left of T, segment - intra), intra += len after each buffer, and when intra reaches the segment
 *             size the direction flips and intra = 0. T counts both directions.   (ctsIOPattern.cpp:906-992)
 *   Duplex    T is rounded up to even and each direction sends H = T / 2. The reference's interleaving depends on
 *             timing; the tick fixes it: buffer m has d = m & 1, stream position (m >> 1) B and len = min(B, H -
 *             (m >> 1) B). Per direction this is the reference's sequence of sends. (ctsIOPattern.cpp:1000-1095)
 *
 * PushPull in closed form, all in 64 bits: kp = ceil(P / B), kq = ceil(Q / B), K = kp + kq, C = P + Q, y = m / K, r = m
 * mod K.
 *   r < kp       d = 0, s = r B, stream position y P + s, the buffer starts at G = y C + s of the transfer,
 *                len = min(B, P - s, T - G)
 *   otherwise    r' = r - kp, d = 1, s = r' B, stream position y Q + s, G = y C + P + s, len = min(B, Q - s, T - G)
 *   N = (T / C) K + tail; with rem = T mod C, tail = ceil(rem / B) when rem <= P, else kp + ceil((rem - P) / B).
 * So everything a tick decides per buffer follows from the entry's constants and one number, the connection's buffer
 * index: the turn (m_sending, m_intraSegmentTransfer) is not stored.
 *
 *   per tick   cts_tcp_exchange_send(ids, max_buffers, ...)  -> up to max_buffers buffers of every listed connection,
 *                                                               whichever side sends them: the arena's bytes, their
 *                                                               descriptors, the entries, a tick block
 *
 * Send pacing (-RateLimit, -BurstCount / -BurstDelay; cts_tcp_senders.h) runs in the tick for every pattern:
 *
 *   per tick   cts_tcp_exchange_send_paced(..., dev_pace, now_ms, ...)  -> the same, but every listed connection sends
 *                                                               what CreateNewTask's send branch of the side whose turn
 *                                                               it is lets out at now_ms, from two 64-byte pace entries
 *                                                               per connection; the tick block ends with the time of
 *                                                               the next deferred send
 *
 * The receiving half consumes the descriptors unchanged (cts_verify_at, cts_refview_accumulate_conns, cts_conns_close
 * of cts_connections.h) over receiver tables of 2 x n_conns slots: the receiver of direction d of connection c is slot
 * c + d x n_conns, the direction-0 receivers (the servers) first, then the direction-1 receivers (the clients).
 *
 * A tick may carry a connection across segment ends: with max_buffers > 1 it writes a pull segment's first buffers in
 * the same launch as the push segment's last, before anything of the push segment has been verified. A Push tick
 * likewise writes ahead of its verification; what orders the two halves is the stream.
 *
 * Out of scope:
 *   - closed forms for the runs of sends inside a quantum: the paced tick walks a paced connection's buffers one by one
 *   - -Buffer:[lo,hi] random buffer sizes: an entry has one buffer_size
 *   - a ring that wraps: a tick writes the slots first_slot .. first_slot + total of one flat arena
 *   - the connection-id and completion messages that frame a TCP connection (ctsIOPattern.cpp:330-470)
 *   - handing the slots to sockets
 *
 * Conventions as cts_tcp_senders.h: noexcept, int status, device pointers from hipMalloc, stream = hipStream_t as
 * void*. Every argument check comes before the engine is used, so a bad argument is CTS_E_INVALID with nothing
 * launched; n == 0 is CTS_OK.
 */
#ifndef CTS_TCP_EXCHANGE_H
#define CTS_TCP_EXCHANGE_H

#include <stddef.h>

#include "cts_tcp_senders.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CTS_TCP_EXCHANGE_PUSH 0u
#define CTS_TCP_EXCHANGE_PULL 1u
#define CTS_TCP_EXCHANGE_PUSHPULL 2u
#define CTS_TCP_EXCHANGE_DUPLEX 3u

/* One per connection slot, device memory, 8-byte aligned, 64 bytes. Filled by cts_tcp_exchange_init (and
 * cts_tcp_exchange_seek) on the host and copied to the device by the caller; afterwards only the tick writes it. */
typedef struct cts_tcp_exchange_state {
    uint64_t transfer_bytes; /* -Transfer, both directions together; Duplex: rounded up to even */
    uint64_t total_buffers;  /* N, the length of the connection's buffer sequence */
    uint64_t buffers_sent;   /* m, the connection's position in that sequence */
    uint64_t bytes_sent[2];  /* per direction: m_bytesSent of its sender, m_bytesRecv of its receiver */
    uint32_t buffer_size;    /* -Buffer */
    uint32_t pattern;        /* CTS_TCP_EXCHANGE_* */
    uint32_t push_bytes;     /* -PushBytes (PushPull) */
    uint32_t pull_bytes;     /* -PullBytes (PushPull) */
    uint32_t finished;       /* 0 running, 1 every buffer of the sequence has been sent */
    uint32_t reserved;       /* 0 */
} cts_tcp_exchange_state;

/* A fresh entry with its N. push_bytes and pull_bytes are stored as given and matter to PushPull only.
 * CTS_E_INVALID for a null out, transfer_bytes == 0, buffer_size == 0, an unknown pattern, PushPull with push_bytes ==
 * 0 or pull_bytes == 0, or a Duplex transfer of 2^64 - 1 (it has no even successor). Host only. */
int cts_tcp_exchange_init(uint32_t pattern, uint64_t transfer_bytes, uint32_t buffer_size, uint32_t push_bytes,
                          uint32_t pull_bytes, cts_tcp_exchange_state* out);

/* Sets the entry to the state after its first m buffers: buffers_sent, both bytes_sent and finished. It serves a
 * resumed transfer and a test's preset. CTS_E_INVALID for a null entry, an entry that cts_tcp_exchange_init would not
 * have made, or m > total_buffers. Host only; closed forms, whatever m. */
int cts_tcp_exchange_seek(cts_tcp_exchange_state* entry, uint64_t m);

/* The reference's turn at the entry's position: *direction = the direction of the next buffer (for a PushPull client
 * m_sending == (direction == 0), for its server m_sending == (direction == 1)) and *intra = m_intraSegmentTransfer.
 * Push and Pull give their one direction and 0; Duplex gives buffers_sent & 1 and 0. At the end of the sequence the
 * values are those the last completion left (PushPull: a full last segment has flipped the direction). Either output
 * may be NULL. CTS_E_INVALID for a null or malformed entry. Host only. */
int cts_tcp_exchange_where(const cts_tcp_exchange_state* entry, uint32_t* direction, uint32_t* intra);

/* What direction d (0 or 1) of the entry's connection carries in total: the dev_expected_bytes of that receiver's
 * cts_conns_close. 0 for a null or malformed entry or d > 1. Host only. */
uint64_t cts_tcp_exchange_direction_bytes(const cts_tcp_exchange_state* entry, uint32_t direction);

/* What one tick did; written (not accumulated) by the tick. 48 bytes, 8-byte aligned. Its first 32 bytes are the
 * senders' tick block. */
typedef struct cts_tcp_exchange_tick {
    cts_tcp_sender_tick tick;
    uint64_t bytes_dir[2]; /* tick.bytes by direction */
} cts_tcp_exchange_tick;

/* Bytes of dev_scratch a tick over n listed connections needs (8-byte aligned device memory; its content means
 * nothing between ticks, and two ticks in flight on different streams need one each). */
size_t cts_tcp_exchange_scratch_bytes(uint32_t n);

/* One tick: up to max_buffers buffers of each of the distinct connections dev_conn_ids[0..n), in listed order. For c =
 * dev_conn_ids[i] with entry E = dev_entries[c] and B = E.buffer_size:
 *   c >= n_conns, B == 0, B > stride, E.pattern > 3, or a PushPull E with push_bytes == 0 or pull_bytes == 0
 *                                                 nothing sent, E untouched (code 4)
 *   E.finished != 0 (or E.buffers_sent >= N)      nothing sent, E untouched (code 2)
 *   otherwise the connection wants w = min(max_buffers, N - E.buffers_sent) consecutive slots, handed out by an
 *   exclusive prefix sum (64-bit) p over the listed order, and takes t = min(w, capacity - min(p, capacity)) of them.
 *   p only grows, so at most one connection per tick takes fewer slots than it wants and more than none, and every
 *   running connection listed after it takes none (code 3, E untouched). Buffer j < t goes to tick-local slot g = p +
 *   j, arena slot first_slot + g, and is element m = E.buffers_sent + j of the connection's sequence, with direction
 *   d, stream position s and length len as above:
 *     the bytes P[(s + x) mod 65536] for x < len: byte for byte what cts_fill writes for the descriptor
 *     dev_descs[g] = {byte_offset = (first_slot + g) x stride, length = len, expected_pattern_offset = s mod 65536,
 *                     conn_index = c + d x n_conns, skip_head = 0}
 *   then E.bytes_sent[d] += the taken buffers' bytes of direction d, E.buffers_sent += t, and E.finished = 1 once
 *   buffers_sent == N (code 1, else 0).
 * The codes are the senders' (CTS_TCP_SENDER_SENT .. CTS_TCP_SENDER_SKIPPED). The written slots are first_slot ..
 * first_slot + total with no gap, total = min(capacity, sum of w) = tick.buffers, which the caller knows from the
 * settings without reading anything back. Nothing else is written: not the bytes between a buffer's end and the next
 * slot, not the slots from total on, not dev_descs[total .. capacity).
 *
 * A table of Push entries gives, byte for byte, what cts_tcp_senders_send gives over the same transfers: the arena,
 * the descriptors, the codes, the tick's first 32 bytes and the sent block.
 *
 * dev_descs is required: `capacity` elements, 8-byte aligned. dev_codes[i] (n elements, may be NULL) takes the code,
 * dev_tick (may be NULL) the tick block. dev_sent_counters (may be NULL) is a cts_counters_sent block: it takes the
 * tick's bytes (both directions), buffers and finished connections.
 *
 * Arguments: cts_tcp_senders_send's, with dev_entries for dev_senders, and n_conns <= 2^31 (the receiver index c +
 * n_conns is a uint32); scratch_bytes >= cts_tcp_exchange_scratch_bytes(n). CTS_E_INVALID otherwise, nothing launched.
 * An entry comes from cts_tcp_exchange_init or _seek; with any other content the lengths and offsets are unspecified,
 * but no write leaves the entries, the capacity's slots or the output arrays and no buffer is longer than its slot.
 * Ordering: on one stream, a tick's outputs are ready for the receive pass that follows. Two ticks listing the same
 * connection must be stream-ordered. A connection listed twice in one tick is the caller's error (its entry is then
 * undefined; no write leaves the entries, the capacity's slots or the output arrays). */
int cts_tcp_exchange_send(cts_engine* engine, void* dev_arena, uint64_t arena_bytes, uint32_t stride,
                          uint64_t first_slot, uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n,
                          uint32_t max_buffers, cts_tcp_exchange_state* dev_entries, uint32_t n_conns,
                          cts_buf_desc* dev_descs, uint32_t* dev_codes, cts_tcp_exchange_tick* dev_tick,
                          void* dev_sent_counters, void* dev_scratch, size_t scratch_bytes, void* stream);

/* ---- send pacing ---------------------------------------------------------------------------------------------------
 * What one paced tick did. 64 bytes, 8-byte aligned. Its first 48 bytes are the plain exchange tick's block, its tail
 * is cts_tcp_sender_paced_tick's. */
typedef struct cts_tcp_exchange_paced_tick {
    cts_tcp_exchange_tick tick;
    int64_t next_due_ms;          /* the smallest due_ms among the listed running connections (codes 0, 1, 3 and 5) that
                                     the tick leaves with a pending send; INT64_MAX when there is none */
    uint32_t connections_waiting; /* code 5 */
    uint32_t connections_pending; /* the listed running connections left with a pending send, each counted once */
} cts_tcp_exchange_paced_tick;

/* Bytes of dev_scratch a paced tick over n listed connections needs (the plain tick's, with the larger tick block). */
size_t cts_tcp_exchange_paced_scratch_bytes(uint32_t n);

/* One paced tick at the time now_ms: cts_tcp_exchange_send, with every listed running connection's wanted slots cut to
 * what pacing lets out.
 *
 * The pace table: dev_pace holds 2 x n_conns cts_tcp_sender_pace entries (cts_tcp_sender_pace_init). Entry c + d x
 * n_conns is the pacing state of the side that sends direction d of connection c, the client for d = 0, the server for
 * d = 1: the receivers' indexing. Each side of a reference connection is a ctsIoPattern of its own with its own
 * m_bytesSendingThisQuantum, m_quantumStartTimeMs and m_burstCount. Push uses entry c only, Pull entry c + n_conns
 * only, PushPull and Duplex both; the entries a pattern does not use are never read or written.
 *
 * The walk: with limit = min(max_buffers, N - E.buffers_sent), m = E.buffers_sent and step(Q, now, size) the step of
 * cts_tcp_senders.h (CreateNewTask's send branch, ctsIOPattern.cpp:593-674) over the pace entry Q,
 *
 *   run_x(cap):  count = 0
 *     while count < cap:
 *         (d, len) = element m + count of the sequence;  Q = dev_pace[c + d x n_conns]
 *         if Q.pending:  if now_ms < Q.due_ms: break;  Q.pending = 0            the waiting send goes out first
 *         else:          off = step(Q, now_ms, len)
 *                        if off > 0: Q.pending = 1; Q.due_ms = now_ms + off; break   task created, send deferred
 *         count += 1
 *     return count
 *
 * which is run() of cts_tcp_senders.h with every step taken on the pace entry of the next buffer's direction. The
 * connection wants w = run_x(limit) slots; p and t are the plain tick's:
 *   w == 0                       nothing sent (code 5, CTS_TCP_SENDER_WAITING), E untouched, the pace entries as
 *                                run_x(limit) leaves them (a first step may have created the pending task)
 *   w > 0, t == 0                nothing sent (code 3), E and both pace entries untouched
 *   0 < t < w                    t buffers sent, the pace entries as run_x(t) from the stored entries leaves them (no
 *                                task beyond the t-th is created)
 *   t == w                       w buffers sent, the pace entries as run_x(limit) leaves them
 * Codes 0-4, the buffers' bytes, the descriptors (receiver c + d x n_conns), E's move, bytes_dir, the sent block and
 * the no-gap rule are cts_tcp_exchange_send's; tick.buffers = min(capacity, sum of w). Connections with codes 2 and 4
 * have no pace entry read, and do not count for next_due_ms or connections_pending.
 *
 * A deferred buffer holds the connection's sequence: nothing after it goes out before it. So of a connection's two
 * pace entries at most one is ever pending, the one of the next buffer's direction, and next_due_ms and
 * connections_pending count a connection once, with that entry's due_ms. (Should a caller's table hold both pending,
 * the connection still counts once, with the smaller due_ms.)
 *
 * Duplex: as the interleaving of the two directions is fixed (buffer m has d = m & 1), a deferred buffer also holds the
 * other direction's next buffer, which the reference's other side, a pattern of its own, could send meanwhile. No send
 * leaves earlier than the reference's CreateNewTask on that side would release it; a send may leave later. Per side,
 * the calls to step (their times and sizes) are what the reference's side would see if asked at those times. The same
 * holds at a PushPull segment end, where the reference waits for the segment anyway.
 *
 * Two equalities:
 *   - a table whose used pace entries all have bytes_per_quantum == 0, burst_count == 0 and pending == 0 gives what
 *     cts_tcp_exchange_send gives, byte for byte and field for field, with the tail {INT64_MAX, 0, 0}. Such a
 *     connection is not walked: max_buffers = 2^31 is no loop.
 *   - a table of Push entries gives what cts_tcp_senders_send_paced gives over the same transfers and pace settings:
 *     the arena, the descriptors, the codes, the pace entries [0, n_conns), the tick's first 32 bytes, its three tail
 *     fields and the sent block.
 *
 * Arguments: cts_tcp_exchange_send's, and dev_pace non-null when n_conns != 0 and 8-byte aligned, 2 x n_conns entries;
 * now_ms >= 0; dev_tick (may be NULL) a cts_tcp_exchange_paced_tick; scratch_bytes >=
 * cts_tcp_exchange_paced_scratch_bytes(n). CTS_E_INVALID otherwise, nothing launched; n == 0 is CTS_OK. The caller's
 * duties are the paced senders' tick's: now_ms does not decrease from tick to tick of a table and stays below 2^62,
 * bytes_per_quantum x the quanta a tick skips fits an int64, and a pace entry comes from cts_tcp_sender_pace_init.
 * Outside them, or with an entry that cts_tcp_exchange_init or _seek did not make, the values of the pace entries, the
 * wanted counts, the lengths and the tick's tail are unspecified, but no write leaves the entries, the capacity's
 * slots or the output arrays. A paced connection costs a loop of up to max_buffers steps in each of two launches. */
int cts_tcp_exchange_send_paced(cts_engine* engine, void* dev_arena, uint64_t arena_bytes, uint32_t stride,
                                uint64_t first_slot, uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n,
                                uint32_t max_buffers, cts_tcp_exchange_state* dev_entries,
                                cts_tcp_sender_pace* dev_pace, uint32_t n_conns, int64_t now_ms,
                                cts_buf_desc* dev_descs, uint32_t* dev_codes, cts_tcp_exchange_paced_tick* dev_tick,
                                void* dev_sent_counters, void* dev_scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* CTS_TCP_EXCHANGE_H */
