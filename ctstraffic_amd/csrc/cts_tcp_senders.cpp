// cts_tcp_senders.cpp — TCP senders on the device-resident path (cts_tcp_senders.h): the host-side entry initialiser
// (cts_tcp_sender_init), the scratch size, the tick (cts_tcp_senders_send), the pace entry's initialiser and the paced
// tick (cts_tcp_sender_pace_init, cts_tcp_senders_send_paced), and the three reads of a sent block.
//
// A translation unit of its own, like cts_media_stream_servers.cpp: nothing else in the library references these
// entry points or their launchers. No threads, no allocation.
#include <hip/hip_runtime_api.h>

#include "cts_internal.hpp"
#include "cts_tcp_senders.h"

static_assert(sizeof(cts_tcp_sender_state) == 32 && alignof(cts_tcp_sender_state) == 8, "cts_tcp_sender_state: 32 bytes");
static_assert(sizeof(cts_tcp_sender_tick) == 32 && alignof(cts_tcp_sender_tick) == 8, "cts_tcp_sender_tick: 32 bytes");
static_assert(sizeof(cts_tcp_sender_pace) == 64 && alignof(cts_tcp_sender_pace) == 8, "cts_tcp_sender_pace: 64 bytes");
static_assert(sizeof(cts_tcp_sender_paced_tick) == 48 && alignof(cts_tcp_sender_paced_tick) == 8,
              "cts_tcp_sender_paced_tick: 48 bytes");
static_assert(sizeof(cts_counters_sent) == 6 * sizeof(uint64_t), "a sent block's six words are a counter block's");

namespace {

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (prev == dev) || (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline int hip_status(hipError_t e) { return e == hipSuccess ? CTS_OK : CTS_E_HIP; }

using cts::misaligned;
using cts::tick_args_ok;

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

size_t cts_tcp_senders_scratch_bytes(uint32_t n) { return cts::TcpSenderScratch::bytes(n); }

int cts_tcp_senders_send(cts_engine* e, void* dev_arena, uint64_t arena_bytes, uint32_t stride, uint64_t first_slot,
                         uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n, uint32_t max_buffers,
                         cts_tcp_sender_state* dev_senders, uint32_t n_conns, cts_buf_desc* dev_descs,
                         uint32_t* dev_codes, cts_tcp_sender_tick* dev_tick, void* dev_sent_counters,
                         void* dev_scratch, size_t scratch_bytes, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (!tick_args_ok(dev_arena, arena_bytes, stride, first_slot, capacity, dev_conn_ids, max_buffers, dev_senders,
                      n_conns, dev_descs, dev_codes, dev_tick, dev_sent_counters, dev_scratch, scratch_bytes,
                      cts::TcpSenderScratch::bytes(n)))
        return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    const cts::TcpSenderScratch scratch(dev_scratch, n);
    // the descriptor pass and the fill read the tick's buffer count: a caller that wants no tick block gets the
    // scratch's
    cts_tcp_sender_tick* const tick = dev_tick != nullptr ? dev_tick : scratch.tick;
    hipStream_t const s = static_cast<hipStream_t>(stream);
    hipError_t rc = cts::launch_tcp_sender_plan(dev_conn_ids, n, max_buffers, dev_senders, n_conns, stride, capacity,
                                                dev_codes, tick, static_cast<uint64_t*>(dev_sent_counters), scratch, s);
    if (rc != hipSuccess) return CTS_E_HIP;
    rc = cts::launch_tcp_sender_descs(stride, first_slot, capacity, dev_conn_ids, n, dev_senders, n_conns, scratch,
                                      tick, dev_descs, s, geo);
    if (rc != hipSuccess) return CTS_E_HIP;
    return hip_status(cts::launch_tcp_sender_fill(static_cast<uint8_t*>(dev_arena), arena_bytes, stride, capacity,
                                                  dev_descs, tick, s, geo));
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

size_t cts_tcp_senders_paced_scratch_bytes(uint32_t n) { return cts::TcpPacedScratch::bytes(n); }

int cts_tcp_senders_send_paced(cts_engine* e, void* dev_arena, uint64_t arena_bytes, uint32_t stride,
                               uint64_t first_slot, uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n,
                               uint32_t max_buffers, cts_tcp_sender_state* dev_senders, cts_tcp_sender_pace* dev_pace,
                               uint32_t n_conns, int64_t now_ms, cts_buf_desc* dev_descs, uint32_t* dev_codes,
                               cts_tcp_sender_paced_tick* dev_tick, void* dev_sent_counters, void* dev_scratch,
                               size_t scratch_bytes, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (!tick_args_ok(dev_arena, arena_bytes, stride, first_slot, capacity, dev_conn_ids, max_buffers, dev_senders,
                      n_conns, dev_descs, dev_codes, dev_tick, dev_sent_counters, dev_scratch, scratch_bytes,
                      cts::TcpPacedScratch::bytes(n)))
        return CTS_E_INVALID;
    if (now_ms < 0) return CTS_E_INVALID;
    if ((n_conns != 0 && dev_pace == nullptr) || misaligned(dev_pace, 8)) return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    const cts::TcpPacedScratch scratch(dev_scratch, n);
    cts_tcp_sender_paced_tick* const tick = dev_tick != nullptr ? dev_tick : scratch.tick;
    hipStream_t const s = static_cast<hipStream_t>(stream);
    hipError_t rc = cts::launch_tcp_paced_plan(dev_conn_ids, n, max_buffers, dev_senders, dev_pace, n_conns, now_ms,
                                               stride, capacity, dev_codes, tick,
                                               static_cast<uint64_t*>(dev_sent_counters), scratch, s);
    if (rc != hipSuccess) return CTS_E_HIP;
    // the descriptor pass and the fill are the plain tick's: they read the block's first 32 bytes
    rc = cts::launch_tcp_sender_descs(stride, first_slot, capacity, dev_conn_ids, n, dev_senders, n_conns,
                                      scratch.plain, &tick->tick, dev_descs, s, geo);
    if (rc != hipSuccess) return CTS_E_HIP;
    return hip_status(cts::launch_tcp_sender_fill(static_cast<uint8_t*>(dev_arena), arena_bytes, stride, capacity,
                                                  dev_descs, &tick->tick, s, geo));
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
