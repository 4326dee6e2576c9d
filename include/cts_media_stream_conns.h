/*
 * cts_media_stream_conns.h — MediaStream (UDP) connections on the device-resident path: many clients' jitter windows
 * and statistics in device memory, fed by the receive pass, advanced at a render tick and closed with the reference's
 * ctsUdpStatistics and status, with no host round trip per batch.
 *
 * On the host one cts_media_stream_client (cts_media_stream.h) holds one stream; cts_media_stream_verify_frames serves
 * one of them per launch and its sums go back through the host before the next batch. Here a connection is a slot c,
 * as in cts_connections.h: dev_conn_first_fail[c] (the first datagram that failed the stream, as a stream ordinal),
 * dev_conns[c] (cts_ms_conn_state below) and the connection's ring of frame bytes inside one uint64_t array.
 *
 *   per batch   cts_media_stream_verify_status_at(...)  -> statuses; lowers the slots of connections with an exception
 *               cts_media_stream_conns_accumulate(...)  -> each connection's books, its ring, the node-wide UDP block
 *   per tick    cts_media_stream_conns_render(ids, ...) -> TimerCallback + RenderFrame of every listed connection
 *   per close   cts_media_stream_conns_close(ids, ...)  -> results, the close block, slots and rings emptied
 *   now and then cts_conn_slots_rebase(delta)           -> as for TCP connections (cts_connections.h)
 *
 * The semantics are those of ctsIoPatternMediaStreamClient (ctsIOPatternMediaStream.cpp:46-96, 140-318, 360-530) as
 * cts_media_stream_client_complete_status and cts_media_stream_client_render restate them, one client per slot.
 *
 * Conventions as cts_connections.h: noexcept, int status, device pointers from hipMalloc, stream = hipStream_t as
 * void*. Every argument check comes before the engine is used, so a bad argument is CTS_E_INVALID with nothing
 * launched; n == 0 is CTS_OK.
 */
#ifndef CTS_MEDIA_STREAM_CONNS_H
#define CTS_MEDIA_STREAM_CONNS_H

#include "cts_connections.h"
#include "cts_media_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cts_ms_conn_state.finished */
#define CTS_MS_CONN_RUNNING 0u     /* the renderer has not ended the stream */
#define CTS_MS_CONN_FINISHED 1u    /* rendered to its final frame (Abort -> status 0) */
#define CTS_MS_CONN_FATAL 2u       /* FatalAbort: nothing was ever received */
#define CTS_MS_CONN_CLOSED 3u      /* closed before the renderer ended it (cts_media_stream_conns_close) */

/* One per connection slot, device memory, 8-byte aligned, 112 bytes. Filled by cts_ms_conn_init on the host and
 * copied to the device by the caller; afterwards only the kernels write it. With g a datagram's stream ordinal and F
 * the connection's slot in dev_conn_first_fail: */
typedef struct cts_ms_conn_state {
    uint64_t bits_received;         /* ctsUdpStatistics: clean DATA datagrams with g < F, completed bytes x 8 */
    uint64_t successful_frames;     /* ... frames rendered with exactly frame_size_bytes */
    uint64_t dropped_frames;        /* ... with fewer (and final_frame of them at a FatalAbort) */
    uint64_t duplicate_frames;      /* ... with more */
    uint64_t error_frames;          /* clean DATA datagrams outside the window or past the final frame */
    uint64_t datagrams;             /* datagrams completed into the pattern: g <= F while the stream ran */
    uint64_t datagrams_after_end;   /* g > F, or after the renderer or a close ended the stream: applied nowhere */
    int64_t head_sequence_number;   /* the jitter queue's head frame; starts at 1, moves only at a render tick */
    int64_t final_frame;            /* m_finalFrame = stream_length_frames */
    uint64_t frame_base;            /* the ring: dev_frame_bytes[frame_base .. frame_base + frames); sequence number s
                                     * sits at frame_base + (s - 1) mod frames, always */
    uint32_t frames;                /* the queue's size, 2 x min(final_frame, buffered_frames) */
    uint32_t frame_size_bytes;
    uint32_t initial_buffer_frames; /* min(final_frame, buffered_frames) */
    uint32_t timer_wheel_offset;    /* m_timerWheelOffsetFrames; starts at initial_buffer_frames */
    uint32_t last_error;            /* CTS_STATUS_IO_RUNNING, 0, or the protocol error that ended the stream */
    uint32_t finished;              /* CTS_MS_CONN_* */
    uint32_t received_any;          /* sticky: some datagram's bytes reached the ring (ReceivedBufferedFrames: no byte
                                     * is cleared before the first render, and then the head has moved) */
    uint32_t has_failure;           /* a datagram latched last_error: fail_datagram = datagrams - 1 */
} cts_ms_conn_state;                /* 112 bytes */

/* A fresh entry from the client's settings, with cts_media_stream_client_create's validation and arithmetic
 * (ctsIOPatternMediaStream.cpp:46-96): final_frame = stream_length_frames, the queue 2 x min(final_frame,
 * buffered_frames) frames. CTS_E_INVALID for a null argument, frame_size_bytes == 0, frames_per_second == 0,
 * stream_length_frames <= 0 or > UINT32_MAX, or a queue below 2 frames. Host only; the caller lays the rings out in
 * one uint64_t array (frame_base, out->frames elements each, zeroed) and copies the entries to the device. */
int cts_ms_conn_init(const cts_media_stream_settings* settings, uint64_t frame_base, cts_ms_conn_state* out);

#define CTS_MS_CONN_RESULT_FLAG_BAD_CONN 0x1u     /* conn_index >= n_conns: nothing read, counted or reset */
#define CTS_MS_CONN_RESULT_FLAG_HAS_FAILURE 0x2u  /* a datagram failed the stream: fail_datagram is valid */
#define CTS_MS_CONN_RESULT_FLAG_RUNNING 0x4u      /* still running at close: reported as NOT_ALL_DATA_TRANSFERRED */

/* What a close reports for one connection: its ctsUdpStatistics, the datagram counts and the status. */
typedef struct cts_ms_conn_result {
    uint64_t bits_received;
    uint64_t successful_frames;
    uint64_t dropped_frames;
    uint64_t duplicate_frames;
    uint64_t error_frames;
    uint64_t datagrams;
    uint64_t datagrams_after_end;
    int64_t head_sequence_number;
    uint32_t fail_datagram;  /* index, in completion order, of the datagram that failed the stream (flag HAS_FAILURE);
                              * 0xFFFFFFFF otherwise */
    uint32_t first_fail;     /* the slot at close */
    uint32_t status;         /* 0, CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN or _NOT_ALL_DATA_TRANSFERRED */
    uint32_t conn_index;     /* dev_conn_ids[i] */
    uint32_t flags;          /* CTS_MS_CONN_RESULT_FLAG_* */
    uint32_t finished;       /* the entry's at close: 0, CTS_MS_CONN_FINISHED or _FATAL */
} cts_ms_conn_result;        /* 88 bytes */

/* The node-wide UdpStatusDetails (ctsConfig.h:417) as a view of an ordinary device counter block
 * (cts_counters_device_bytes(), cts_counters_reset): the accounting pass adds bits, error frames and datagrams, the
 * tick the three frame outcomes (the final_frame drops of a FatalAbort included). It folds and all-reduces like the
 * other blocks. The UDP status line prints from it through cts_status.h: the difference of two reads fills a
 * cts_udp_status time slice (bits_received and the four frame counts) for cts_status_udp_line, and the last read
 * cts_status_udp_summary. */
typedef struct cts_counters_udp {
    uint64_t bits_received;
    uint64_t successful_frames;
    uint64_t dropped_frames;
    uint64_t duplicate_frames;
    uint64_t error_frames;
    uint64_t datagrams;
} cts_counters_udp;

/* cts_media_stream_verify_status with stream ordinals: datagram i of the launch is ordinal base_index + i, and every
 * exception does atomicMin(dev_conn_first_fail[d.conn_index], base_index + i) when d.conn_index < n_conns. An
 * exception is a datagram that fails the stream: kind SHORT, UNKNOWN, BAD_DESC or ZERO (NotAllDataTransferred), or
 * DATA whose payload does not verify (DataDidNotMatchBitPattern); an ID datagram is none. Statuses and the
 * verify-counter block as cts_media_stream_verify_status (connections_failed is not fed). Launches holding datagrams
 * of one connection may run in any order: the slot ends at the lowest exception ordinal.
 * Ordinal limit and alignment as cts_verify_at: base_index + n <= 0xFFFFFFFF, dev_descs 8-byte and dev_arena 16-byte
 * aligned, dev_status and dev_conn_first_fail 4-byte, dev_counters 8-byte; dev_conn_first_fail non-null when n_conns
 * != 0 (CTS_E_INVALID otherwise, nothing launched). Only the descriptor form exists: cts_buf_desc.conn_index carries
 * the connection. */
int cts_media_stream_verify_status_at(cts_engine* engine, const void* dev_arena, uint64_t arena_bytes,
                                      const cts_buf_desc* dev_descs, uint32_t n, uint32_t base_index,
                                      cts_datagram_status* dev_status, void* dev_counters,
                                      uint32_t* dev_conn_first_fail, uint32_t n_conns, void* stream);

/* The accounting pass: 40 bytes of metadata per datagram (descriptor + status), no arena reads. For datagram i with
 * ordinal g = base_index + i, connection c = dev_descs[i].conn_index, entry E = dev_conns[c] and F =
 * dev_conn_first_fail[c]:
 *   c >= n_conns      counts in dev_udp_counters only, as a connection that never fails and has no window:
 *                     datagrams + 1, and bits_received for clean DATA
 *   E.finished != 0   E.datagrams_after_end + 1, nothing else (the renderer or a close ended the stream)
 *   g < F             E.datagrams + 1; clean DATA: bits_received + 8 x completed, then error_frames + 1 when seq >
 *                     final_frame, seq < head or seq > head + frames - 1, else ring[(seq - 1) mod frames] += completed
 *                     and received_any is set; an ID datagram counts in datagrams only
 *   g == F            E.datagrams + 1 and E.last_error is latched from the datagram (one datagram per connection)
 *   g > F             E.datagrams_after_end + 1
 * dev_udp_counters takes what the entries take of bits_received, error_frames and datagrams. The window (head) is
 * the one the last tick left: it does not move inside a batch. Runs of one connection's datagrams are summed on the
 * chip before they reach the entry (one set of adds per run, as cts_refview_accumulate_conns); the ring takes one add
 * per in-window datagram. A ring index at or beyond frame_elems is never written (the datagram then counts as an
 * error frame).
 * Ordering contract as cts_refview_accumulate: after every receive pass holding ordinals <= the batch's own for its
 * connections, and before the next tick or close that lists them.
 * dev_descs, dev_status (read as 8-byte words), dev_conns, dev_frame_bytes and dev_udp_counters 8-byte aligned,
 * dev_conn_first_fail 4-byte;
 * dev_descs, dev_status and dev_udp_counters non-null; dev_conn_first_fail and dev_conns non-null when n_conns != 0,
 * dev_frame_bytes when frame_elems != 0; base_index + n <= 0xFFFFFFFF (CTS_E_INVALID otherwise). */
int cts_media_stream_conns_accumulate(cts_engine* engine, uint64_t arena_bytes, const cts_buf_desc* dev_descs,
                                      const cts_datagram_status* dev_status, uint32_t n, uint32_t base_index,
                                      const uint32_t* dev_conn_first_fail, cts_ms_conn_state* dev_conns,
                                      uint64_t* dev_frame_bytes, uint64_t frame_elems, uint32_t n_conns,
                                      void* dev_udp_counters, void* stream);

/* One render tick (TimerCallback, then RenderFrame: ctsIOPatternMediaStream.cpp:360-530) of each of the distinct
 * connections dev_conn_ids[0..n) whose last_error is still CTS_STATUS_IO_RUNNING:
 *   ++timer_wheel_offset; then, when timer_wheel_offset >= initial_buffer_frames and head <= final_frame:
 *     received_any clear and head == 1  -> dropped_frames += final_frame, finished = CTS_MS_CONN_FATAL, last_error =
 *                                          NOT_ALL_DATA_TRANSFERRED (code 2)
 *     otherwise                          -> the head frame's bytes against frame_size_bytes: successful, dropped
 *                                          (fewer) or duplicate (more); its ring element zeroed, head += 1
 *   then head > final_frame              -> finished = CTS_MS_CONN_FINISHED, last_error = 0 (code 1)
 * dev_udp_counters takes the frame outcomes. dev_codes[i] (may be NULL): 0 keep rendering, 1 finished, 2 fatal; a
 * connection that is not rendered (failed, ended or closed earlier) reports its entry's finished, an id >= n_conns 0
 * and is skipped. A failed connection is not rendered again: the reference has closed its socket.
 * Ordering: after the accounting passes of the batches the tick follows, before those of the batches after it.
 * dev_conn_ids and dev_codes 4-byte aligned, dev_conns, dev_frame_bytes and dev_udp_counters 8-byte; dev_conn_ids and
 * dev_udp_counters non-null, dev_conns and dev_frame_bytes non-null when n_conns != 0 (CTS_E_INVALID otherwise). */
int cts_media_stream_conns_render(cts_engine* engine, const uint32_t* dev_conn_ids, uint32_t n,
                                  cts_ms_conn_state* dev_conns, uint64_t* dev_frame_bytes, uint32_t n_conns,
                                  void* dev_udp_counters, uint32_t* dev_codes, void* stream);

/* Closes the distinct connections dev_conn_ids[0..n). For each id c < n_conns the status is the entry's last_error;
 * a connection still CTS_STATUS_IO_RUNNING is reported and counted as CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED with
 * CTS_MS_CONN_RESULT_FLAG_RUNNING (the device's own rule: the reference never closes a running client normally, its
 * renderer ends every stream). dev_results[i] (may be NULL) takes the statistics, and the close block
 * (cts_counters_close, which may be the block the TCP closes use) takes connections_closed + 1, one of successful,
 * data_errors and not_all_data, and bits_received / 8 to bytes_recv. Then the slot is emptied (0xFFFFFFFF), the
 * connection's ring zeroed, and the entry left ended (finished = CTS_MS_CONN_CLOSED unless the renderer ended it,
 * last_error = the status): datagrams that arrive late count as datagrams_after_end until the caller writes a fresh
 * entry over it. An id >= n_conns gets CTS_MS_CONN_RESULT_FLAG_BAD_CONN and an otherwise zero result.
 * Ordering as cts_conns_close. dev_conn_ids and dev_conn_first_fail 4-byte aligned, the others 8-byte; dev_conn_ids
 * and dev_close_counters non-null; dev_conn_first_fail, dev_conns and dev_frame_bytes non-null when n_conns != 0. */
int cts_media_stream_conns_close(cts_engine* engine, const uint32_t* dev_conn_ids, uint32_t n,
                                 uint32_t* dev_conn_first_fail, cts_ms_conn_state* dev_conns,
                                 uint64_t* dev_frame_bytes, uint32_t n_conns, cts_ms_conn_result* dev_results,
                                 void* dev_close_counters, void* stream);

/* The three counter reads over UDP blocks: the same fold, and for the all-reduce the same ncclAllReduce of count 6,
 * with the six words named as cts_counters_udp. */
int cts_counters_read_udp(cts_engine* engine, const void* dev_udp_counters, cts_counters_udp* out, void* stream);
int cts_counters_read_multi_udp(cts_engine* const* engines, const void* const* dev_udp_counters,
                                void* const* streams, uint32_t n, cts_counters_udp* out);
int cts_counters_allreduce_udp(cts_engine* const* engines, const void* const* dev_udp_counters,
                               void* const* streams, uint32_t n, cts_counters_udp* out);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* CTS_MEDIA_STREAM_CONNS_H */
