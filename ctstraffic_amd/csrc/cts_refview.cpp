// cts_refview.cpp — stream ordinals in the DataError slots (cts_verify_at / cts_verify_strided_at) and the
// reference view of the device counters (cts_refview_accumulate, the *_ref reads): the counters as ctsTraffic
// itself would hold them, every connection stopped at its first failing buffer (ctsIOPattern.cpp:486-489).
//
// A translation unit of its own: cts_engine.cpp and cts_collective.cpp reference none of the launchers used here, so
// whatever links those two against its own launchers keeps linking.
#include <hip/hip_runtime_api.h>

#include "cts_engine.h"
#include "cts_internal.hpp"

namespace {

using cts::DeviceGuard;
using cts::hip_status;

// ordinal 0xFFFFFFFF is the empty slot: the launch's last ordinal, base_index + n - 1, must stay below it
inline bool ordinals_overflow(uint32_t base_index, uint32_t n) { return (uint64_t)base_index + n > 0xFFFFFFFFull; }

inline cts_counters_ref ref_of(const cts_counters_ex& x)
{
    // a reference-view block has a counter block's layout: slot k of one is slot k of the other
    return cts_counters_ref{x.bytes_checked,  x.bytes_ok,         x.buffers_checked,
                            x.buffers_failed, x.mismatched_bytes, x.connections_failed};
}

}  // namespace

extern "C" {

int cts_verify_at(cts_engine* e, const void* dev_arena, uint64_t arena_bytes, const cts_buf_desc* dev_descs, uint32_t n,
                  uint32_t max_length_hint, uint32_t base_index, cts_verify_result* dev_results, void* dev_counters,
                  uint32_t* dev_conn_first_fail, uint32_t n_conns, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (dev_arena == nullptr || dev_descs == nullptr || ((uintptr_t)dev_descs & 7u) != 0 ||
        ((uintptr_t)dev_arena & 15u) != 0)
        return CTS_E_INVALID;
    if (dev_conn_first_fail == nullptr && n_conns != 0) return CTS_E_INVALID;
    if (((uintptr_t)dev_results & 3u) != 0 || ((uintptr_t)dev_counters & 7u) != 0 ||
        ((uintptr_t)dev_conn_first_fail & 3u) != 0)
        return CTS_E_INVALID;
    if (ordinals_overflow(base_index, n)) return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    return hip_status(cts::launch_verify_at(static_cast<const uint8_t*>(dev_arena), arena_bytes, dev_descs, n,
                                            max_length_hint, dev_results, static_cast<uint64_t*>(dev_counters),
                                            dev_conn_first_fail, n_conns, base_index,
                                            static_cast<hipStream_t>(stream), geo));
}

int cts_verify_strided_at(cts_engine* e, const void* dev_arena, uint64_t arena_bytes, uint32_t stride,
                          const uint32_t* dev_lengths, uint32_t n, uint32_t skip_head, uint32_t expected_offset,
                          uint32_t conn_index, uint32_t base_index, cts_verify_result* dev_results, void* dev_counters,
                          uint32_t* dev_conn_first_fail, uint32_t n_conns, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (dev_arena == nullptr || dev_lengths == nullptr || stride == 0 || arena_bytes < 16 ||
        ((uintptr_t)dev_arena & 15u) != 0 || ((uintptr_t)dev_lengths & 3u) != 0)
        return CTS_E_INVALID;
    if (expected_offset >= CTS_PATTERN_PERIOD) return CTS_E_INVALID;
    if (dev_conn_first_fail == nullptr && n_conns != 0) return CTS_E_INVALID;
    if (((uintptr_t)dev_results & 3u) != 0 || ((uintptr_t)dev_counters & 7u) != 0 ||
        ((uintptr_t)dev_conn_first_fail & 3u) != 0)
        return CTS_E_INVALID;
    if (ordinals_overflow(base_index, n)) return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    return hip_status(cts::launch_verify_strided_at(
        static_cast<const uint8_t*>(dev_arena), arena_bytes, stride, dev_lengths, n, skip_head, expected_offset,
        conn_index, dev_results, static_cast<uint64_t*>(dev_counters), dev_conn_first_fail, n_conns, base_index,
        static_cast<hipStream_t>(stream), geo));
}

int cts_refview_accumulate(cts_engine* e, uint64_t arena_bytes, const cts_buf_desc* dev_descs, uint32_t n,
                           uint32_t base_index, const uint32_t* dev_conn_first_fail, uint32_t n_conns,
                           void* dev_ref_counters, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (dev_descs == nullptr || ((uintptr_t)dev_descs & 7u) != 0) return CTS_E_INVALID;
    if (dev_conn_first_fail == nullptr && n_conns != 0) return CTS_E_INVALID;
    if (dev_ref_counters == nullptr || ((uintptr_t)dev_ref_counters & 7u) != 0 ||
        ((uintptr_t)dev_conn_first_fail & 3u) != 0)
        return CTS_E_INVALID;
    if (ordinals_overflow(base_index, n)) return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    return hip_status(cts::launch_refview(arena_bytes, dev_descs, n, base_index, dev_conn_first_fail, n_conns,
                                          static_cast<uint64_t*>(dev_ref_counters), static_cast<hipStream_t>(stream),
                                          geo));
}

int cts_refview_accumulate_strided(cts_engine* e, uint64_t arena_bytes, uint32_t stride, const uint32_t* dev_lengths,
                                   uint32_t n, uint32_t skip_head, uint32_t conn_index, uint32_t base_index,
                                   const uint32_t* dev_conn_first_fail, uint32_t n_conns, void* dev_ref_counters,
                                   void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (dev_lengths == nullptr || stride == 0 || arena_bytes < 16 || ((uintptr_t)dev_lengths & 3u) != 0)
        return CTS_E_INVALID;
    if (dev_conn_first_fail == nullptr && n_conns != 0) return CTS_E_INVALID;
    if (dev_ref_counters == nullptr || ((uintptr_t)dev_ref_counters & 7u) != 0 ||
        ((uintptr_t)dev_conn_first_fail & 3u) != 0)
        return CTS_E_INVALID;
    if (ordinals_overflow(base_index, n)) return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    return hip_status(cts::launch_refview_strided(arena_bytes, stride, dev_lengths, n, skip_head, conn_index, base_index,
                                                  dev_conn_first_fail, n_conns,
                                                  static_cast<uint64_t*>(dev_ref_counters),
                                                  static_cast<hipStream_t>(stream), geo));
}

// The reads are the *_ex reads: the same fold (and the same ncclAllReduce of count 6) over a block of the same
// layout, its six words named as cts_counters_ref.
int cts_counters_read_ref(cts_engine* e, const void* dev_ref_counters, cts_counters_ref* out, void* stream)
{
    if (out == nullptr) return CTS_E_INVALID;
    cts_counters_ex x{};
    const int rc = cts_counters_read_ex(e, dev_ref_counters, &x, stream);
    if (rc == CTS_OK) *out = ref_of(x);
    return rc;
}

int cts_counters_read_multi_ref(cts_engine* const* engines, const void* const* dev_ref_counters, void* const* streams,
                                uint32_t n, cts_counters_ref* out)
{
    if (out == nullptr) return CTS_E_INVALID;
    cts_counters_ex x{};
    const int rc = cts_counters_read_multi_ex(engines, dev_ref_counters, streams, n, &x);
    if (rc == CTS_OK) *out = ref_of(x);
    return rc;
}

int cts_counters_allreduce_ref(cts_engine* const* engines, const void* const* dev_ref_counters, void* const* streams,
                               uint32_t n, cts_counters_ref* out)
{
    if (out == nullptr) return CTS_E_INVALID;
    cts_counters_ex x{};
    const int rc = cts_counters_allreduce_ex(engines, dev_ref_counters, streams, n, &x);
    if (rc == CTS_OK) *out = ref_of(x);
    return rc;
}

}  // extern "C"
