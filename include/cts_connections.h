/*
 * cts_connections.h — connections on the device-resident path: the reference view per connection, a close that
 * classifies, reports and recycles a connection slot, and a rebase that keeps the ordinal space alive.
 *
 * ctsTraffic opens connections, closes each with a result (its bytes and its status, which feed Completed and
 * DataError in the status line: ctsSocketState.cpp:221-228, ctsIOPattern.h:46-77) and opens the next one in its
 * place, for as long as the process runs (-Connections:N -Iterations:M, or a server until stopped). On the
 * device a connection is a slot c: dev_conn_first_fail[c] (cts_verify_at) and dev_conn_state[c] (below).
 *
 *   per batch   cts_verify_at(...)                   -> lowers the slots of failing connections
 *               cts_refview_accumulate_conns(...)    -> node-wide reference view + each connection's entry
 *   per close   cts_conns_close(ids, expected, ...)  -> results, the close block, slots and entries emptied
 *   now and then cts_conn_slots_rebase(delta)        -> ordinals restart low; the caller lowers its base_index
 *
 * Conventions as cts_engine.h: noexcept, int status, device pointers from hipMalloc, stream = hipStream_t as void*.
 * Every argument check comes before the engine is used, so a bad argument is CTS_E_INVALID with nothing launched.
 */
#ifndef CTS_CONNECTIONS_H
#define CTS_CONNECTIONS_H

#include "cts_engine.h"
#include "cts_pattern.h" /* CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED / _TOO_MUCH_DATA_TRANSFERRED */

#ifdef __cplusplus
extern "C" {
#endif

/* One per connection slot, device memory, 8-byte aligned; all-zero = a fresh connection (hipMemset 0). The
 * connection's share of cts_counters_ref: with g a buffer's stream ordinal, F the connection's first failing ordinal
 * and vlen = length - skip_head, bad descriptors excluded. */
typedef struct cts_conn_state {
    uint64_t bytes_recv;            /* sum of vlen over g <= F: what the connection's m_bytesRecv would hold */
    uint64_t buffers_recv;          /* # buffers with g <= F */
    uint64_t bytes_after_failure;   /* sum of vlen over g > F: verified here, never received by the reference */
    uint64_t buffers_after_failure; /* # buffers with g > F */
} cts_conn_state;                   /* 32 bytes */

#define CTS_CONN_RESULT_FLAG_BAD_CONN 0x1u /* conn_index >= n_conns: nothing read, counted or reset */

/* What a close reports for one connection (ctsSocket::CloseSocket's status and the connection's statistics). */
typedef struct cts_conn_result {
    uint64_t bytes_recv;            /* the entry at close */
    uint64_t buffers_recv;
    uint64_t bytes_after_failure;
    uint64_t buffers_after_failure;
    uint32_t first_fail;            /* the slot at close: first failing stream ordinal, 0xFFFFFFFF = none */
    uint32_t status;                /* 0, CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN,
                                     * CTS_STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED or _NOT_ALL_DATA_TRANSFERRED */
    uint32_t conn_index;            /* dev_conn_ids[i] */
    uint32_t flags;                 /* CTS_CONN_RESULT_FLAG_* */
} cts_conn_result;                  /* 48 bytes */

/* The close block: a third device counter block (cts_counters_device_bytes(), cts_counters_reset; it folds and
 * all-reduces like the other two). Per closed connection with a slot: 1 to connections_closed, 1 to exactly one of the
 * four classes, its entry's bytes_recv to bytes_recv. successful feeds
 * ConnectionStatusDetails.m_successfulCompletionCount and data_errors + not_all_data + too_much_data feeds
 * m_protocolErrorCount (IsProtocolError, ctsIOPattern.h:55-58; ctsSocketState.cpp:221-228);
 * cts_counters_ex.connections_failed is the data_errors part alone, counted when the verify sees the failure. */
typedef struct cts_counters_close {
    uint64_t connections_closed;
    uint64_t successful;
    uint64_t data_errors;   /* c_statusErrorDataDidNotMatchBitPattern */
    uint64_t not_all_data;  /* c_statusErrorNotAllDataTransferred */
    uint64_t too_much_data; /* c_statusErrorTooMuchDataTransferred */
    uint64_t bytes_recv;
} cts_counters_close;

/* cts_refview_accumulate / _strided that also keep each connection's books. One pass over the descriptors adds to
 * dev_ref_counters exactly what cts_refview_accumulate adds, and each buffer's share to dev_conn_state[conn_index]
 * (n_conns entries): g <= F to bytes_recv and buffers_recv, g > F to the two *_after_failure fields. Bad descriptors
 * count nowhere; a buffer whose conn_index >= n_conns counts in the block, as in cts_refview_accumulate, and in no
 * entry. Consecutive descriptors of one connection are summed on the chip before they reach its entry, so a strided
 * ring or a connection-major batch costs a handful of atomic adds per connection and wave, not one per buffer; a
 * batch whose neighbours all differ in connection (buffer-major order) costs one set per buffer, spread over the
 * entries.
 * Contract, argument checks, n == 0 and the ordinal limit: those of cts_refview_accumulate. In addition
 * dev_conn_state must be non-null and 8-byte aligned when n_conns != 0 (CTS_E_INVALID). */
int cts_refview_accumulate_conns(cts_engine* engine, uint64_t arena_bytes, const cts_buf_desc* dev_descs, uint32_t n,
                                 uint32_t base_index, const uint32_t* dev_conn_first_fail, uint32_t n_conns,
                                 void* dev_ref_counters, cts_conn_state* dev_conn_state, void* stream);
int cts_refview_accumulate_conns_strided(cts_engine* engine, uint64_t arena_bytes, uint32_t stride,
                                         const uint32_t* dev_lengths, uint32_t n, uint32_t skip_head,
                                         uint32_t conn_index, uint32_t base_index, const uint32_t* dev_conn_first_fail,
                                         uint32_t n_conns, void* dev_ref_counters, cts_conn_state* dev_conn_state,
                                         void* stream);

/* Closes the n connections dev_conn_ids[0..n) (distinct ids; one id twice in a call is undefined). For each id c <
 * n_conns, with F = dev_conn_first_fail[c] and S = dev_conn_state[c]:
 *   status = F != 0xFFFFFFFF                 ? CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN
 *          : S.bytes_recv > expected_bytes[i] ? CTS_STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED
 *          : S.bytes_recv < expected_bytes[i] ? CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED
 *          : 0
 * dev_results[i] = {S, F, status, c, 0}, the close block takes the connection (cts_counters_close), and then the slot
 * is emptied (0xFFFFFFFF) and the entry zeroed: slot c is ready for the next connection. The data error wins over the
 * byte-count errors: it happened inside the stream, and the reference records only the first error
 * (ctsIOPattern.h:155, :346). dev_expected_bytes[i] is the connection's -Transfer size in verified bytes; NULL turns
 * the byte-count check off ("Udp just tracks bytes", ctsIOPatternState.hpp:346-354). The reference raises the two
 * byte-count errors at a completion (ctsIOPatternState.hpp:357-370, 398-404, 491-501); the device judges them at
 * close, from the bytes received up to and including the first failing buffer.
 * An id >= n_conns gets CTS_CONN_RESULT_FLAG_BAD_CONN, its conn_index and an otherwise zero result; it is counted
 * nowhere and resets nothing. dev_results may be NULL: only the counters and the reset happen.
 * Ordering contract: the close runs after every verify and every reference-view pass that holds a buffer of the
 * closed connections (the same stream, or an event); a verify of the slot's next connection runs after the close.
 * dev_conn_ids 4-byte aligned and non-null; dev_expected_bytes, dev_conn_state, dev_results and dev_close_counters
 * 8-byte aligned; dev_conn_first_fail 4-byte aligned; dev_conn_first_fail and dev_conn_state non-null when n_conns
 * != 0; dev_close_counters non-null (CTS_E_INVALID otherwise). n == 0 is CTS_OK. */
int cts_conns_close(cts_engine* engine, const uint32_t* dev_conn_ids, const uint64_t* dev_expected_bytes, uint32_t n,
                    uint32_t* dev_conn_first_fail, cts_conn_state* dev_conn_state, uint32_t n_conns,
                    cts_conn_result* dev_results, void* dev_close_counters, void* stream);

/* Keeps the ordinal space alive: every non-empty slot F becomes F - delta, or 0 where F < delta; empty slots stay
 * empty. The caller subtracts delta from its next base_index. Preconditions:
 *  - every buffer with an ordinal below delta has been through its verify and its reference-view pass (and this call
 *    is ordered after them, and before the launches that use the lowered base_index);
 *  - delta is strictly below the lowest ordinal still to be handed in.
 * Every later ordinal is then at least 1, so a connection that failed before the rebase sits at or above slot 0 and
 * below all its later buffers: they stay "after failure". n_conns == 0 or delta == 0 is CTS_OK and does nothing;
 * dev_conn_first_fail non-null and 4-byte aligned otherwise. */
int cts_conn_slots_rebase(cts_engine* engine, uint32_t* dev_conn_first_fail, uint32_t n_conns, uint32_t delta,
                          void* stream);

/* The three counter reads over close blocks: the same fold, and for the all-reduce the same ncclAllReduce of count
 * 6, with the six words named as cts_counters_close. */
int cts_counters_read_close(cts_engine* engine, const void* dev_close_counters, cts_counters_close* out, void* stream);
int cts_counters_read_multi_close(cts_engine* const* engines, const void* const* dev_close_counters,
                                  void* const* streams, uint32_t n, cts_counters_close* out);
int cts_counters_allreduce_close(cts_engine* const* engines, const void* const* dev_close_counters,
                                 void* const* streams, uint32_t n, cts_counters_close* out);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* CTS_CONNECTIONS_H */
