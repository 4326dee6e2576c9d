// cts_connections.cpp — connections on the device-resident path (cts_connections.h): the reference view per connection
// (cts_refview_accumulate_conns / _strided), the close that classifies, reports and recycles connection slots
// (cts_conns_close), the slot rebase (cts_conn_slots_rebase) and the *_close reads.
//
// A translation unit of its own, like cts_refview.cpp: cts_engine.cpp and cts_collective.cpp reference none of the
// launchers used here, so whatever links those two against its own launchers keeps linking.
#include <hip/hip_runtime_api.h>

#include "cts_connections.h"
#include "cts_internal.hpp"

namespace {

using cts::DeviceGuard;
using cts::hip_status;

// ordinal 0xFFFFFFFF is the empty slot: the launch's last ordinal, base_index + n - 1, must stay below it
inline bool ordinals_overflow(uint32_t base_index, uint32_t n) { return (uint64_t)base_index + n > 0xFFFFFFFFull; }

inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0; }

// the slot array and the entry table of n_conns connections: both there (unless there are no connections), both aligned
inline bool tables_bad(const uint32_t* conn_first_fail, const cts_conn_state* conn_state, uint32_t n_conns)
{
    if (n_conns != 0 && (conn_first_fail == nullptr || conn_state == nullptr)) return true;
    return misaligned(conn_first_fail, 4) || misaligned(conn_state, 8);
}

inline cts_counters_close close_of(const cts_counters_ex& x)
{
    // a close block has a counter block's layout: slot k of one is slot k of the other
    return cts_counters_close{x.bytes_checked,  x.bytes_ok,         x.buffers_checked,
                              x.buffers_failed, x.mismatched_bytes, x.connections_failed};
}

}  // namespace

extern "C" {

int cts_refview_accumulate_conns(cts_engine* e, uint64_t arena_bytes, const cts_buf_desc* dev_descs, uint32_t n,
                                 uint32_t base_index, const uint32_t* dev_conn_first_fail, uint32_t n_conns,
                                 void* dev_ref_counters, cts_conn_state* dev_conn_state, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (dev_descs == nullptr || misaligned(dev_descs, 8)) return CTS_E_INVALID;
    if (tables_bad(dev_conn_first_fail, dev_conn_state, n_conns)) return CTS_E_INVALID;
    if (dev_ref_counters == nullptr || misaligned(dev_ref_counters, 8)) return CTS_E_INVALID;
    if (ordinals_overflow(base_index, n)) return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    return hip_status(cts::launch_conn_accumulate(arena_bytes, dev_descs, n, base_index, dev_conn_first_fail, n_conns,
                                                  static_cast<uint64_t*>(dev_ref_counters), dev_conn_state,
                                                  static_cast<hipStream_t>(stream), geo));
}

int cts_refview_accumulate_conns_strided(cts_engine* e, uint64_t arena_bytes, uint32_t stride,
                                         const uint32_t* dev_lengths, uint32_t n, uint32_t skip_head,
                                         uint32_t conn_index, uint32_t base_index, const uint32_t* dev_conn_first_fail,
                                         uint32_t n_conns, void* dev_ref_counters, cts_conn_state* dev_conn_state,
                                         void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (dev_lengths == nullptr || stride == 0 || arena_bytes < 16 || misaligned(dev_lengths, 4)) return CTS_E_INVALID;
    if (tables_bad(dev_conn_first_fail, dev_conn_state, n_conns)) return CTS_E_INVALID;
    if (dev_ref_counters == nullptr || misaligned(dev_ref_counters, 8)) return CTS_E_INVALID;
    if (ordinals_overflow(base_index, n)) return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    return hip_status(cts::launch_conn_accumulate_strided(
        arena_bytes, stride, dev_lengths, n, skip_head, conn_index, base_index, dev_conn_first_fail, n_conns,
        static_cast<uint64_t*>(dev_ref_counters), dev_conn_state, static_cast<hipStream_t>(stream), geo));
}

int cts_conns_close(cts_engine* e, const uint32_t* dev_conn_ids, const uint64_t* dev_expected_bytes, uint32_t n,
                    uint32_t* dev_conn_first_fail, cts_conn_state* dev_conn_state, uint32_t n_conns,
                    cts_conn_result* dev_results, void* dev_close_counters, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (dev_conn_ids == nullptr || misaligned(dev_conn_ids, 4) || misaligned(dev_expected_bytes, 8))
        return CTS_E_INVALID;
    if (tables_bad(dev_conn_first_fail, dev_conn_state, n_conns)) return CTS_E_INVALID;
    if (misaligned(dev_results, 8) || dev_close_counters == nullptr || misaligned(dev_close_counters, 8))
        return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    return hip_status(cts::launch_conn_close(dev_conn_ids, dev_expected_bytes, n, dev_conn_first_fail, dev_conn_state,
                                             n_conns, dev_results, static_cast<uint64_t*>(dev_close_counters),
                                             static_cast<hipStream_t>(stream), geo));
}

int cts_conn_slots_rebase(cts_engine* e, uint32_t* dev_conn_first_fail, uint32_t n_conns, uint32_t delta, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n_conns == 0 || delta == 0) return CTS_OK;
    if (dev_conn_first_fail == nullptr || misaligned(dev_conn_first_fail, 4)) return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    return hip_status(
        cts::launch_conn_slots_rebase(dev_conn_first_fail, n_conns, delta, static_cast<hipStream_t>(stream), geo));
}

// The reads are the *_ex reads: the same fold (and the same ncclAllReduce of count 6) over a block of the same
// layout, its six words named as cts_counters_close.
int cts_counters_read_close(cts_engine* e, const void* dev_close_counters, cts_counters_close* out, void* stream)
{
    if (out == nullptr) return CTS_E_INVALID;
    cts_counters_ex x{};
    const int rc = cts_counters_read_ex(e, dev_close_counters, &x, stream);
    if (rc == CTS_OK) *out = close_of(x);
    return rc;
}

int cts_counters_read_multi_close(cts_engine* const* engines, const void* const* dev_close_counters,
                                  void* const* streams, uint32_t n, cts_counters_close* out)
{
    if (out == nullptr) return CTS_E_INVALID;
    cts_counters_ex x{};
    const int rc = cts_counters_read_multi_ex(engines, dev_close_counters, streams, n, &x);
    if (rc == CTS_OK) *out = close_of(x);
    return rc;
}

int cts_counters_allreduce_close(cts_engine* const* engines, const void* const* dev_close_counters,
                                 void* const* streams, uint32_t n, cts_counters_close* out)
{
    if (out == nullptr) return CTS_E_INVALID;
    cts_counters_ex x{};
    const int rc = cts_counters_allreduce_ex(engines, dev_close_counters, streams, n, &x);
    if (rc == CTS_OK) *out = close_of(x);
    return rc;
}

}  // extern "C"
