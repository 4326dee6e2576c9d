// cts_tcp_senders.cpp — TCP senders on the device-resident path (cts_tcp_senders.h): the host-side entry initialiser
// (cts_tcp_sender_init), the scratch size, the tick (cts_tcp_senders_send), the pace entry's initialiser and the paced
// tick (cts_tcp_sender_pace_init, cts_tcp_senders_send_paced), and the three reads of a sent block.
//
// A translation unit of its own, like cts_media_stream_servers.cpp: nothing else in the library references these
// entry points or their launchers. No threads, no allocation.
#include <hip/hip_runtime_api.h>

#include "cts_internal.hpp"
#include "cts_tcp_senders.h"
#include "cts_tcp_tick.hpp"

static_assert(sizeof(cts_tcp_sender_state) == 32 && alignof(cts_tcp_sender_state) == 8, "cts_tcp_sender_state: 32 bytes");
static_assert(sizeof(cts_tcp_sender_tick) == 32 && alignof(cts_tcp_sender_tick) == 8, "cts_tcp_sender_tick: 32 bytes");
static_assert(sizeof(cts_tcp_sender_pace) == 64 && alignof(cts_tcp_sender_pace) == 8, "cts_tcp_sender_pace: 64 bytes");
static_assert(sizeof(cts_tcp_sender_paced_tick) == 48 && alignof(cts_tcp_sender_paced_tick) == 8,
              "cts_tcp_sender_paced_tick: 48 bytes");
static_assert(sizeof(cts_counters_sent) == 6 * sizeof(uint64_t), "a sent block's six words are a counter block's");

namespace {

// The descriptor pass of both ticks, the plain tick's: it reads the tick block's first 32 bytes.
auto sender_descs(const cts::TcpTickArgs& a, const cts_tcp_sender_state* senders)
{
    return [&a, senders](const auto& scratch, auto* tick, hipStream_t s, const cts::LaunchGeometry& geo) {
        return cts::launch_tcp_sender_descs(a.stride, a.first_slot, a.capacity, a.conn_ids, a.n, senders, a.n_conns,
                                            scratch.prefix, scratch.before, cts::plain_tick(tick), a.descs, s, geo);
    };
}

inline cts_counters_sent sent_of(const cts_counters_ex& x)
{
    return cts_counters_sent{x.bytes_checked, x.bytes_ok, x.buffers_checked, {0, 0, 0}};
}

}  // namespace

extern "C" {

int cts_tcp_sender_init(uint64_t transfer_bytes, uint32_t buffer_size, cts_tcp_sender_state* out)
{
    if (out == nullptr || transfer_bytes == 0 || buffer_size == 0) return CTS_E_INVALID;
    *out = cts_tcp_sender_state{};
    out->transfer_bytes = transfer_bytes;
    out->buffer_size = buffer_size;
    return CTS_OK;
}

size_t cts_tcp_senders_scratch_bytes(uint32_t n) { return cts::TcpTickScratch<cts_tcp_sender_tick>::bytes(n); }

int cts_tcp_senders_send(cts_engine* e, void* dev_arena, uint64_t arena_bytes, uint32_t stride, uint64_t first_slot,
                         uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n, uint32_t max_buffers,
                         cts_tcp_sender_state* dev_senders, uint32_t n_conns, cts_buf_desc* dev_descs,
                         uint32_t* dev_codes, cts_tcp_sender_tick* dev_tick, void* dev_sent_counters,
                         void* dev_scratch, size_t scratch_bytes, void* stream)
{
    const cts::TcpTickArgs a{dev_arena, arena_bytes, stride, first_slot, capacity, dev_conn_ids, n, max_buffers, n_conns,
                             dev_descs, dev_codes, dev_sent_counters, dev_scratch, scratch_bytes, stream, nullptr, 0};
    return cts::tcp_tick_send(e, a, dev_senders, dev_tick, [] { return true; }, sender_descs(a, dev_senders));
}

int cts_tcp_sender_pace_init(uint64_t bytes_per_second, uint32_t period_ms, uint32_t burst_count,
                             uint32_t burst_delay_ms, int64_t start_ms, cts_tcp_sender_pace* out)
{
    if (out == nullptr || start_ms < 0) return CTS_E_INVALID;
    // m_quantumPeriodMs and m_bytesSendingPerQuantum as the pattern's constructor sets them (ctsIOPattern.cpp:258-262)
    const uint32_t period = period_ms != 0u ? period_ms : 100u;
    if (bytes_per_second > (uint64_t)INT64_MAX / period) return CTS_E_INVALID;
    *out = cts_tcp_sender_pace{};
    out->bytes_per_quantum = (int64_t)(bytes_per_second * period / 1000u);
    out->quantum_start_ms = start_ms;
    out->quantum_period_ms = period;
    out->burst_count = burst_count;
    out->burst_left = burst_count;
    out->burst_delay_ms = burst_delay_ms;
    return CTS_OK;
}

size_t cts_tcp_senders_paced_scratch_bytes(uint32_t n)
{
    return cts::TcpTickScratch<cts_tcp_sender_paced_tick>::bytes(n);
}

int cts_tcp_senders_send_paced(cts_engine* e, void* dev_arena, uint64_t arena_bytes, uint32_t stride,
                               uint64_t first_slot, uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n,
                               uint32_t max_buffers, cts_tcp_sender_state* dev_senders, cts_tcp_sender_pace* dev_pace,
                               uint32_t n_conns, int64_t now_ms, cts_buf_desc* dev_descs, uint32_t* dev_codes,
                               cts_tcp_sender_paced_tick* dev_tick, void* dev_sent_counters, void* dev_scratch,
                               size_t scratch_bytes, void* stream)
{
    const cts::TcpTickArgs a{dev_arena, arena_bytes, stride, first_slot, capacity, dev_conn_ids, n, max_buffers, n_conns,
                             dev_descs, dev_codes, dev_sent_counters, dev_scratch, scratch_bytes, stream, dev_pace, now_ms};
    return cts::tcp_tick_send(e, a, dev_senders, dev_tick, [&] { return cts::pace_args_ok(a); },
                              sender_descs(a, dev_senders));
}

// The reads are the *_ex reads: the same fold (and the same ncclAllReduce of count 6) over a block of the same
// layout, its first three words named as cts_counters_sent.
int cts_counters_read_sent(cts_engine* e, const void* dev_sent_counters, cts_counters_sent* out, void* stream)
{
    if (out == nullptr) return CTS_E_INVALID;
    cts_counters_ex x{};
    const int rc = cts_counters_read_ex(e, dev_sent_counters, &x, stream);
    if (rc == CTS_OK) *out = sent_of(x);
    return rc;
}

int cts_counters_read_multi_sent(cts_engine* const* engines, const void* const* dev_sent_counters,
                                 void* const* streams, uint32_t n, cts_counters_sent* out)
{
    if (out == nullptr) return CTS_E_INVALID;
    cts_counters_ex x{};
    const int rc = cts_counters_read_multi_ex(engines, dev_sent_counters, streams, n, &x);
    if (rc == CTS_OK) *out = sent_of(x);
    return rc;
}

int cts_counters_allreduce_sent(cts_engine* const* engines, const void* const* dev_sent_counters,
                                void* const* streams, uint32_t n, cts_counters_sent* out)
{
    if (out == nullptr) return CTS_E_INVALID;
    cts_counters_ex x{};
    const int rc = cts_counters_allreduce_ex(engines, dev_sent_counters, streams, n, &x);
    if (rc == CTS_OK) *out = sent_of(x);
    return rc;
}

}  // extern "C"
