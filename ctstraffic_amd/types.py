"""numpy mirrors of the C ABI structs (include/cts_engine.h)."""
import numpy as np

# cts_buf_desc: the ctsTask fields the hot path reads (ctsIOTask.hpp:37-60)
DESC_DTYPE = np.dtype(
    [
        ("byte_offset", "<u8"),
        ("length", "<u4"),
        ("expected_pattern_offset", "<u4"),
        ("conn_index", "<u4"),
        ("skip_head", "<u4"),
    ]
)
# cts_verify_result
RESULT_DTYPE = np.dtype(
    [
        ("first_mismatch", "<u4"),
        ("mismatch_bytes", "<u4"),
        ("expected", "u1"),
        ("actual", "u1"),
        ("pass", "u1"),
        ("flags", "u1"),
    ]
)
COUNTER_FIELDS = ("bytes_checked", "bytes_ok", "buffers_checked", "buffers_failed", "mismatched_bytes")
# cts_counters_ex: plus the DataError count (ctsSocketState.cpp:221-228), slot 5 of a device counter shard
COUNTER_FIELDS_EX = COUNTER_FIELDS + ("connections_failed",)
RESULT_FLAG_BAD_DESC = 0x1

assert DESC_DTYPE.itemsize == 24 and RESULT_DTYPE.itemsize == 12
# cts_datagram_record (include/cts_media_stream.h)
DGRAM_RECORD_DTYPE = np.dtype(
    [
        ("sequence_number", "<i8"),
        ("sender_qpc", "<i8"),
        ("sender_qpf", "<i8"),
        ("flag", "<u2"),
        ("kind", "u1"),
        ("reserved", "u1"),
        ("completed_bytes", "<u4"),
    ]
)
# cts_datagram_status (compact receive output)
DGRAM_STATUS_DTYPE = np.dtype(
    [
        ("sequence_number", "<i8"),
        ("completed_bytes", "<u4"),
        ("flag", "<u2"),
        ("kind", "u1"),
        ("pass", "u1"),
    ]
)
assert DGRAM_STATUS_DTYPE.itemsize == 16
# cts_datagram_header
DGRAM_HEADER_DTYPE = np.dtype([("sequence_number", "<i8"), ("qpc", "<i8"), ("qpf", "<i8")])
RESULT_FLAG_NOT_DATA = 0x2
assert DGRAM_RECORD_DTYPE.itemsize == 32 and DGRAM_HEADER_DTYPE.itemsize == 24
# cts_conn_state (include/cts_connections.h): one connection's share of the reference view; all-zero = fresh
CONN_STATE_DTYPE = np.dtype(
    [
        ("bytes_recv", "<u8"),
        ("buffers_recv", "<u8"),
        ("bytes_after_failure", "<u8"),
        ("buffers_after_failure", "<u8"),
    ]
)
# cts_conn_result: what cts_conns_close reports for one connection
CONN_RESULT_DTYPE = np.dtype(
    [
        ("bytes_recv", "<u8"),
        ("buffers_recv", "<u8"),
        ("bytes_after_failure", "<u8"),
        ("buffers_after_failure", "<u8"),
        ("first_fail", "<u4"),
        ("status", "<u4"),
        ("conn_index", "<u4"),
        ("flags", "<u4"),
    ]
)
CONN_RESULT_FLAG_BAD_CONN = 0x1
# cts_counters_close: the six words of a close block
CLOSE_FIELDS = ("connections_closed", "successful", "data_errors", "not_all_data", "too_much_data", "bytes_recv")
assert CONN_STATE_DTYPE.itemsize == 32 and CONN_RESULT_DTYPE.itemsize == 48
# cts_ms_conn_state (include/cts_media_stream_conns.h): one MediaStream connection's device entry
MS_CONN_STATE_DTYPE = np.dtype(
    [
        ("bits_received", "<u8"),
        ("successful_frames", "<u8"),
        ("dropped_frames", "<u8"),
        ("duplicate_frames", "<u8"),
        ("error_frames", "<u8"),
        ("datagrams", "<u8"),
        ("datagrams_after_end", "<u8"),
        ("head_sequence_number", "<i8"),
        ("final_frame", "<i8"),
        ("frame_base", "<u8"),
        ("frames", "<u4"),
        ("frame_size_bytes", "<u4"),
        ("initial_buffer_frames", "<u4"),
        ("timer_wheel_offset", "<u4"),
        ("last_error", "<u4"),
        ("finished", "<u4"),
        ("received_any", "<u4"),
        ("has_failure", "<u4"),
    ]
)
# cts_ms_conn_result: what cts_media_stream_conns_close reports for one connection
MS_CONN_RESULT_DTYPE = np.dtype(
    [
        ("bits_received", "<u8"),
        ("successful_frames", "<u8"),
        ("dropped_frames", "<u8"),
        ("duplicate_frames", "<u8"),
        ("error_frames", "<u8"),
        ("datagrams", "<u8"),
        ("datagrams_after_end", "<u8"),
        ("head_sequence_number", "<i8"),
        ("fail_datagram", "<u4"),
        ("first_fail", "<u4"),
        ("status", "<u4"),
        ("conn_index", "<u4"),
        ("flags", "<u4"),
        ("finished", "<u4"),
    ]
)
MS_CONN_RESULT_FLAG_BAD_CONN, MS_CONN_RESULT_FLAG_HAS_FAILURE, MS_CONN_RESULT_FLAG_RUNNING = 0x1, 0x2, 0x4
MS_CONN_RUNNING, MS_CONN_FINISHED, MS_CONN_FATAL, MS_CONN_CLOSED = 0, 1, 2, 3
# cts_counters_udp: the six words of a UDP block
UDP_FIELDS = ("bits_received", "successful_frames", "dropped_frames", "duplicate_frames", "error_frames", "datagrams")
assert MS_CONN_STATE_DTYPE.itemsize == 112 and MS_CONN_RESULT_DTYPE.itemsize == 88
# cts_ms_server_state (include/cts_media_stream_servers.h): one MediaStream server's device entry
MS_SERVER_STATE_DTYPE = np.dtype(
    [
        ("bits_sent", "<u8"),
        ("datagrams_sent", "<u8"),
        ("current_frame", "<i8"),
        ("final_frame", "<i8"),
        ("frame_size_bytes", "<u4"),
        ("datagram_max_size", "<u4"),
        ("datagrams_per_frame", "<u4"),
        ("finished", "<u4"),
    ]
)
# cts_ms_server_tick: what one cts_media_stream_servers_send did
MS_SERVER_TICK_DTYPE = np.dtype(
    [
        ("bytes", "<u8"),
        ("datagrams", "<u4"),
        ("connections_sent", "<u4"),
        ("connections_finished", "<u4"),
        ("connections_no_room", "<u4"),
        ("connections_skipped", "<u4"),
        ("reserved", "<u4"),
    ]
)
# a tick's per-connection codes
MS_SERVER_SENT, MS_SERVER_FINISHED, MS_SERVER_ENDED, MS_SERVER_NO_ROOM, MS_SERVER_SKIPPED = 0, 1, 2, 3, 4
MS_SERVER_MIN_DATAGRAM = 53  # CTS_MS_SERVER_MIN_DATAGRAM
assert MS_SERVER_STATE_DTYPE.itemsize == 48 and MS_SERVER_TICK_DTYPE.itemsize == 32
# cts_ms_server_schedule: one MediaStream server's frame schedule, beside its entry; the host writes it, no tick does
MS_SERVER_SCHEDULE_DTYPE = np.dtype([("base_time_ms", "<i8"), ("frames_per_second", "<u4"), ("reserved", "<u4")])
# cts_ms_server_timed_tick: what one cts_media_stream_servers_send_at did; its first 32 bytes are the plain tick's
MS_SERVER_TIMED_TICK_DTYPE = np.dtype(
    MS_SERVER_TICK_DTYPE.descr + [("next_due_ms", "<i8"), ("connections_waiting", "<u4"), ("frames", "<u4")]
)
MS_SERVER_WAITING = 5  # CTS_MS_SERVER_WAITING: running, but no frame is due at now_ms
assert MS_SERVER_SCHEDULE_DTYPE.itemsize == 16 and MS_SERVER_TIMED_TICK_DTYPE.itemsize == 48
assert MS_SERVER_TIMED_TICK_DTYPE.fields["next_due_ms"][1] == 32
# cts_tcp_sender_state (include/cts_tcp_senders.h): one TCP sender's device entry
TCP_SENDER_DTYPE = np.dtype(
    [
        ("bytes_sent", "<u8"),
        ("transfer_bytes", "<u8"),
        ("buffers_sent", "<u8"),
        ("buffer_size", "<u4"),
        ("finished", "<u4"),
    ]
)
# cts_tcp_sender_tick: what one cts_tcp_senders_send did
TCP_SENDER_TICK_DTYPE = np.dtype(
    [
        ("bytes", "<u8"),
        ("buffers", "<u4"),
        ("connections_sent", "<u4"),
        ("connections_finished", "<u4"),
        ("connections_no_room", "<u4"),
        ("connections_skipped", "<u4"),
        ("reserved", "<u4"),
    ]
)
# a tick's per-connection codes
TCP_SENDER_SENT, TCP_SENDER_FINISHED, TCP_SENDER_ENDED, TCP_SENDER_NO_ROOM, TCP_SENDER_SKIPPED = 0, 1, 2, 3, 4
# cts_counters_sent: the six words of a sent block (the last three stay 0)
SENT_FIELDS = ("bytes_sent", "buffers_sent", "connections_finished", "reserved0", "reserved1", "reserved2")
assert TCP_SENDER_DTYPE.itemsize == 32 and TCP_SENDER_TICK_DTYPE.itemsize == 32
# cts_tcp_sender_pace: one TCP sender's pacing state (a table parallel to the entries)
TCP_SENDER_PACE_DTYPE = np.dtype(
    [
        ("bytes_per_quantum", "<i8"),
        ("bytes_this_quantum", "<i8"),
        ("quantum_start_ms", "<i8"),
        ("due_ms", "<i8"),
        ("quantum_period_ms", "<u4"),
        ("burst_count", "<u4"),
        ("burst_left", "<u4"),
        ("burst_delay_ms", "<u4"),
        ("pending", "<u4"),
        ("reserved", "<u4", (3,)),
    ]
)
# cts_tcp_sender_paced_tick: what one cts_tcp_senders_send_paced did; its first 32 bytes are a cts_tcp_sender_tick
TCP_SENDER_PACED_TICK_DTYPE = np.dtype(
    TCP_SENDER_TICK_DTYPE.descr + [("next_due_ms", "<i8"), ("connections_waiting", "<u4"),
                                   ("connections_pending", "<u4")]
)
TCP_SENDER_WAITING = 5
TCP_SENDER_NO_DUE = (1 << 63) - 1  # next_due_ms when nothing is pending
assert TCP_SENDER_PACE_DTYPE.itemsize == 64 and TCP_SENDER_PACED_TICK_DTYPE.itemsize == 48
# cts_tcp_exchange_state (include/cts_tcp_exchange.h): one Push, Pull, PushPull or Duplex connection's device entry
TCP_EXCHANGE_DTYPE = np.dtype(
    [
        ("transfer_bytes", "<u8"),
        ("total_buffers", "<u8"),
        ("buffers_sent", "<u8"),
        ("bytes_sent", "<u8", (2,)),
        ("buffer_size", "<u4"),
        ("pattern", "<u4"),
        ("push_bytes", "<u4"),
        ("pull_bytes", "<u4"),
        ("finished", "<u4"),
        ("reserved", "<u4"),
    ]
)
TCP_EXCHANGE_PUSH, TCP_EXCHANGE_PULL, TCP_EXCHANGE_PUSHPULL, TCP_EXCHANGE_DUPLEX = 0, 1, 2, 3
# cts_tcp_exchange_tick: what one cts_tcp_exchange_send did; its first 32 bytes are a cts_tcp_sender_tick
TCP_EXCHANGE_TICK_DTYPE = np.dtype(TCP_SENDER_TICK_DTYPE.descr + [("bytes_dir", "<u8", (2,))])
assert TCP_EXCHANGE_DTYPE.itemsize == 64 and TCP_EXCHANGE_TICK_DTYPE.itemsize == 48
# cts_tcp_exchange_paced_tick: what one cts_tcp_exchange_send_paced did; its first 48 bytes are a cts_tcp_exchange_tick,
# its tail is the paced senders' tick's
TCP_EXCHANGE_PACED_TICK_DTYPE = np.dtype(
    TCP_EXCHANGE_TICK_DTYPE.descr + [("next_due_ms", "<i8"), ("connections_waiting", "<u4"),
                                     ("connections_pending", "<u4")]
)
assert TCP_EXCHANGE_PACED_TICK_DTYPE.itemsize == 64
