/*
 * cts_media_stream_servers.h — MediaStream (UDP) servers on the device-resident path: many connections' frame sends
 * written into a datagram ring from a small state entry per connection, with no host metadata per datagram.
 *
 * cts_media_stream_fill and cts_media_stream_fill_strided (cts_media_stream.h) write datagrams whose length and
 * header the host has prepared one by one. What ctsIoPatternMediaStreamServer does per frame is determined by four
 * numbers per connection (ctsIOPattern.cpp:1110-1174, ctsMediaStreamProtocol.hpp:171-244), so here a server is a
 * slot c of a table in device memory (cts_ms_server_state below), as a client is in cts_media_stream_conns.h:
 *
 *   per tick   cts_media_stream_servers_send(ids, ...)  -> one frame of every listed connection: the ring's datagrams,
 *                                                          their descriptors and lengths, the entries, a tick block
 *        or    cts_media_stream_servers_send_at(ids, ..., now_ms)
 *                                                       -> the frames of every listed connection that the reference's
 *                                                          schedule (ctsIOPattern.cpp:1136-1150, the "< 2" rule of
 *                                                          ctsMediaStreamServerConnectedSocket.cpp:62-74) releases at
 *                                                          now_ms, from a 16-byte schedule entry per connection; the
 *                                                          tick block ends with the time of the next frame
 *
 * so a run lists every connection in every tick and its one host timer sleeps until next_due_ms.
 *
 * and the receiving half consumes what it wrote: cts_media_stream_verify_status_at and
 * cts_media_stream_conns_accumulate over the descriptors, cts_media_stream_conns_render, cts_media_stream_conns_close.
 *
 * How many datagrams a tick writes is known without reading anything back: a running connection sends
 * cts_media_stream_split(frame_size_bytes, datagram_max_size, NULL, 0) datagrams per tick, for final_frame ticks, as
 * long as the capacity holds the listed connections' sum. The receive pass's n is that sum, computed on the host
 * from the settings.
 *
 * Out of scope:
 *   - the connection-id datagram and the START exchange (39 bytes once per connection): they stay with the caller;
 *     CTS_PATTERN_MEDIA_STREAM (cts_pattern.h) makes them
 *   - a ring that wraps: a tick writes the slots first_slot .. first_slot + datagrams of one flat arena
 *   - a qpc per connection: one tick carries one timestamp
 *   - handing the written slots to sockets: the ring is the caller's to drain
 *
 * Conventions as cts_media_stream_conns.h: noexcept, int status, device pointers from hipMalloc, stream = hipStream_t
 * as void*. Every argument check comes before the engine is used, so a bad argument is CTS_E_INVALID with nothing
 * launched; n == 0 is CTS_OK.
 */
#ifndef CTS_MEDIA_STREAM_SERVERS_H
#define CTS_MEDIA_STREAM_SERVERS_H

#include <stddef.h>

#include "cts_media_stream_conns.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The smallest datagram_max_size a device server takes. The device's own rule: below it the reference's shortened
 * last-but-one datagram (ctsMediaStreamProtocol.hpp:188-199: it gives up to 26 bytes to a last datagram that would
 * not hold a header and one byte) no longer holds a header and one byte itself. The reference does not check this
 * (ctsConfig.cpp:1232). */
#define CTS_MS_SERVER_MIN_DATAGRAM 53u

/* One per connection slot, device memory, 8-byte aligned, 48 bytes. Filled by cts_ms_server_init on the host and
 * copied to the device by the caller; afterwards only the tick writes it. */
typedef struct cts_ms_server_state {
    uint64_t bits_sent;           /* ctsIOPattern.cpp:1160-1163: 8 x the bytes of every completed frame send */
    uint64_t datagrams_sent;
    int64_t current_frame;        /* m_currentFrame: starts at 1; the sequence number of the next frame */
    int64_t final_frame;          /* stream_length_frames */
    uint32_t frame_size_bytes;
    uint32_t datagram_max_size;
    uint32_t datagrams_per_frame; /* ceil(frame_size_bytes / datagram_max_size) */
    uint32_t finished;            /* 0 running, 1 the final frame has been sent */
} cts_ms_server_state;            /* 48 bytes */

/* A fresh entry from the server's settings. CTS_E_INVALID for a null argument, frame_size_bytes <= 26 (the reference
 * FAIL_FASTs, ctsMediaStreamProtocol.hpp:225-227), frames_per_second == 0, stream_length_frames <= 0 or > UINT32_MAX,
 * or datagram_max_size < CTS_MS_SERVER_MIN_DATAGRAM (the device's own rule, above). buffered_frames is the client's
 * and is not read. Host only. */
int cts_ms_server_init(const cts_media_stream_settings* settings, cts_ms_server_state* out);

/* cts_ms_server_tick codes, dev_codes[i] of a tick */
#define CTS_MS_SERVER_SENT 0u      /* sent a frame, more to come */
#define CTS_MS_SERVER_FINISHED 1u  /* sent its final frame */
#define CTS_MS_SERVER_ENDED 2u     /* finished earlier: nothing sent */
#define CTS_MS_SERVER_NO_ROOM 3u   /* running, but its frame did not fit into the capacity: nothing sent */
#define CTS_MS_SERVER_SKIPPED 4u   /* id >= n_conns, or datagram_max_size > stride: nothing sent */

/* What one tick did; written (not accumulated) by the tick. 32 bytes, 8-byte aligned. */
typedef struct cts_ms_server_tick {
    uint64_t bytes;                /* sum of the sent frames' frame_size_bytes */
    uint32_t datagrams;            /* slots written: first_slot .. first_slot + datagrams */
    uint32_t connections_sent;
    uint32_t connections_finished; /* of those sent, how many sent their final frame */
    uint32_t connections_no_room;  /* running, but their frame did not fit into `capacity` */
    uint32_t connections_skipped;  /* finished earlier, id >= n_conns, or datagram_max_size > stride */
    uint32_t reserved;
} cts_ms_server_tick;

/* Bytes of dev_scratch a tick over n listed connections needs (8-byte aligned device memory; its content means
 * nothing between ticks, and two ticks in flight on different streams need one each). */
size_t cts_media_stream_servers_scratch_bytes(uint32_t n);

/* One tick: one frame of each of the distinct connections dev_conn_ids[0..n), in listed order. For c =
 * dev_conn_ids[i] with entry E = dev_servers[c], F = E.frame_size_bytes, M = E.datagram_max_size and k =
 * E.datagrams_per_frame:
 *   c >= n_conns, E.finished != 0 or M > stride   nothing sent, E untouched (code 4, 2, 4)
 *   otherwise the connection wants k consecutive slots, handed out by an exclusive prefix sum (64-bit) p over the
 *   listed order:
 *   p + k > capacity                              nothing sent, E untouched (code 3); since p only grows, so it is for
 *                                                 every running connection listed after it
 *   otherwise                                     datagram j of the frame goes to slot first_slot + p + j: the
 *                                                 26-byte header {u16 0, i64 E.current_frame, i64 qpc, i64 qpf} and
 *                                                 the payload P[0 .. len_j - 26), byte for byte what
 *                                                 cts_media_stream_fill_strided writes for that length and header,
 *                                                 with the lengths of cts_media_stream_split(F, M). Then
 *                                                 E.bits_sent += 8 F, E.datagrams_sent += k, E.current_frame += 1,
 *                                                 and E.finished = 1 once current_frame > final_frame (code 1, else 0)
 * The written slots are first_slot .. first_slot + tick.datagrams with no gap; bytes between a datagram's end and
 * the next slot, and slots from first_slot + tick.datagrams on, are never written. For the written slot s with
 * tick-local index g = s - first_slot:
 *   dev_descs[g]   = {byte_offset = s x stride, length = len, expected_pattern_offset = 0, conn_index = c,
 *                     skip_head = 26}: the array serves cts_media_stream_verify_status_at,
 *                     cts_media_stream_conns_accumulate and a plain cts_verify of the payloads
 *   dev_lengths[g] = len
 * Both hold `capacity` elements; either may be NULL. dev_codes[i] (n elements, may be NULL) takes the code, dev_tick
 * (may be NULL) the tick block. dev_udp_counters (may be NULL) is a cts_counters_udp block: it takes bits_received +
 * 8 F and datagrams + k per sent frame (the reference's server adds its sent bits to UdpStatusDetails.m_bitsReceived,
 * ctsIOPattern.cpp:1162).
 *
 * Arguments: stride a multiple of 16 in [32, 1 MiB]; dev_arena non-null and 16-byte aligned; (first_slot + capacity)
 * x stride <= arena_bytes with no wrap-around; dev_conn_ids non-null; dev_servers non-null when n_conns != 0;
 * dev_servers, dev_descs, dev_tick, dev_udp_counters and dev_scratch 8-byte aligned, dev_conn_ids, dev_lengths and
 * dev_codes 4-byte; dev_scratch non-null with scratch_bytes >= cts_media_stream_servers_scratch_bytes(n)
 * (CTS_E_INVALID otherwise, nothing launched).
 * Ordering: on one stream, a tick's outputs are ready for the receive pass that follows. Two ticks listing the same
 * connection must be stream-ordered. A connection listed twice in one tick is the caller's error (its entry is then
 * undefined; no write leaves the entries, the ring's slots or the output arrays). */
int cts_media_stream_servers_send(cts_engine* engine, void* dev_arena, uint64_t arena_bytes, uint32_t stride,
                                  uint64_t first_slot, uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n,
                                  cts_ms_server_state* dev_servers, uint32_t n_conns, int64_t qpc, int64_t qpf,
                                  cts_buf_desc* dev_descs, uint32_t* dev_lengths, uint32_t* dev_codes,
                                  cts_ms_server_tick* dev_tick, void* dev_udp_counters, void* dev_scratch,
                                  size_t scratch_bytes, void* stream);

/* ---- The frame schedule on the device ----------------------------------------------------------------------------
 * ctsIoPatternMediaStreamServer gives every frame send the time offset m_baseTimeMilliseconds + m_currentFrame x
 * 1000LL / m_frameRateFps - now (ctsIOPattern.cpp:1136-1150), and ctsMediaStreamServerConnectedSocket sends at once
 * when that offset is below 2 and arms a timer for it otherwise (.cpp:62-74, :125-133). The schedule has no state of
 * its own: which frames are out at now_ms follows from the two numbers below and the entry's current_frame. */

/* One per connection slot, beside dev_servers: device memory, 8-byte aligned, 16 bytes. The host writes it
 * (cts_ms_server_schedule_init) and no tick ever writes it. */
typedef struct cts_ms_server_schedule {
    int64_t base_time_ms;       /* m_baseTimeMilliseconds: the time of frame 0, on the clock of now_ms; in [0, 2^62) */
    uint32_t frames_per_second; /* m_frameRateFps, not 0 */
    uint32_t reserved;
} cts_ms_server_schedule;

/* A schedule entry from the server's settings and the time its stream starts. CTS_E_INVALID for a null argument,
 * frames_per_second == 0, or base_time_ms outside [0, 2^62). Host only. */
int cts_ms_server_schedule_init(const cts_media_stream_settings* settings, int64_t base_time_ms,
                                cts_ms_server_schedule* out);

#define CTS_MS_SERVER_WAITING 5u /* running, but no frame is due at now_ms: nothing sent */

/* What one timed tick did. 48 bytes, 8-byte aligned. Its first 32 bytes are the plain tick's block. */
typedef struct cts_ms_server_timed_tick {
    cts_ms_server_tick tick;
    int64_t next_due_ms;          /* the smallest due(current_frame) of the listed connections that the tick leaves
                                     running (codes 0, 3 and 5), after the tick; INT64_MAX when there is none. A value
                                     <= now_ms + 1 means: tick again once the ring is drained */
    uint32_t connections_waiting; /* code 5 */
    uint32_t frames;              /* frames sent, all connections */
} cts_ms_server_timed_tick;

/* Bytes of dev_scratch a timed tick over n listed connections needs: the plain tick's (with the larger tick block) and
 * a 64-bit word per listed connection, its current_frame from before the move. */
size_t cts_media_stream_servers_timed_scratch_bytes(uint32_t n);

/* The closed form on the host, for the caller's own bookkeeping: how many frames of entry E the schedule S releases at
 * now_ms, at most max_frames, and when the first frame after those is due (INT64_MAX when E is finished or they are
 * its last). E is not moved. frames and next_due_ms may each be NULL. CTS_E_INVALID for a null entry or schedule,
 * max_frames == 0, S.frames_per_second == 0, or now_ms or S.base_time_ms outside [0, 2^62). Host only. */
int cts_ms_server_frames_due(const cts_ms_server_state* state, const cts_ms_server_schedule* schedule, int64_t now_ms,
                             uint32_t max_frames, uint32_t* frames, int64_t* next_due_ms);

/* One timed tick: cts_media_stream_servers_send with every listed connection's frames released by its schedule entry
 * at now_ms, up to max_frames of them (a connection that has fallen behind catches up in one tick). For c =
 * dev_conn_ids[i] with E = dev_servers[c], S = dev_schedule[c], F, M and k as above, and
 *   due(f) = S.base_time_ms + f x 1000 / S.frames_per_second     (the integer division of the product, the
 *                                                                 reference's expression)
 * frame f is released at now_ms when due(f) - now_ms < 2. The frames released are E.current_frame .. last, where with
 * d = now_ms + 1 - S.base_time_ms
 *   d < 0                                  none
 *   d >= E.final_frame x 1000 / fps        last = E.final_frame
 *   otherwise                              last = ((d + 1) x fps - 1) / 1000    (here (d + 1) x fps <= final_frame x
 *                                          1000 + fps < 2^43: nothing overflows)
 * m = max(0, last - E.current_frame + 1) of them, and the connection asks for wf = min(m, max_frames) frames.
 *   code 4 or 2 (the plain tick's, decided first)   nothing sent, E untouched, S not read
 *   wf == 0                                nothing sent, E untouched (code 5)
 *   otherwise it wants w = min(wf x k, UINT32_MAX) consecutive slots, handed out by the exclusive prefix sum (64-bit) p
 *   over the listed order, and takes t = min(wf, (capacity - min(p, capacity)) / k) whole frames:
 *   t == 0                                 nothing sent, E untouched (code 3)
 *   otherwise                              with `before` = E.current_frame, datagram q % k of frame before + q / k goes
 *                                          to slot first_slot + p + q for q in [0, t x k): header, payload, descriptor
 *                                          and length byte for byte what the plain tick writes for that frame. Then
 *                                          E.bits_sent += 8 t F, E.datagrams_sent += t k, E.current_frame += t, and
 *                                          E.finished = 1 once current_frame > final_frame (code 1, else 0)
 * The written slots are first_slot .. first_slot + tick.datagrams with no gap: a connection cut by the capacity (t <
 * wf) has pushed every later prefix past the capacity, so every running connection with a frame out that is listed
 * after it has code 3. The tick block: the plain fields as for the plain tick (bytes = the sum of t F), frames = the
 * sum of t, connections_waiting and next_due_ms as above. dev_udp_counters takes bits_received + 8 t F and datagrams +
 * t k per connection.
 * With max_frames == 1 and a frame of every listed running connection out, the entries, the ring, the descriptors,
 * the lengths, the codes, the UDP block and the first 32 bytes of the tick block are exactly what
 * cts_media_stream_servers_send leaves.
 *
 * Arguments: cts_media_stream_servers_send's, and dev_schedule non-null when n_conns != 0 and 8-byte aligned, n_conns
 * entries; max_frames >= 1; now_ms >= 0; dev_tick (may be NULL) a cts_ms_server_timed_tick; scratch_bytes >=
 * cts_media_stream_servers_timed_scratch_bytes(n). The caller's duties: now_ms is below 2^62 and does not decrease
 * from tick to tick of a table, and a schedule entry comes from cts_ms_server_schedule_init (base_time_ms in [0,
 * 2^62), frames_per_second != 0). Outside them the frame counts and the tick's tail are unspecified, but no write
 * leaves the entries, the capacity's slots or the output arrays. */
int cts_media_stream_servers_send_at(cts_engine* engine, void* dev_arena, uint64_t arena_bytes, uint32_t stride,
                                     uint64_t first_slot, uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n,
                                     cts_ms_server_state* dev_servers, const cts_ms_server_schedule* dev_schedule,
                                     uint32_t n_conns, uint32_t max_frames, int64_t now_ms, int64_t qpc, int64_t qpf,
                                     cts_buf_desc* dev_descs, uint32_t* dev_lengths, uint32_t* dev_codes,
                                     cts_ms_server_timed_tick* dev_tick, void* dev_udp_counters, void* dev_scratch,
                                     size_t scratch_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* CTS_MEDIA_STREAM_SERVERS_H */
