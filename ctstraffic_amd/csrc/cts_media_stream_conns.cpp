// cts_media_stream_conns.cpp — MediaStream connections on the device-resident path (cts_media_stream_conns.h): the
// host-side entry initialiser (cts_ms_conn_init), the ordinal receive pass (cts_media_stream_verify_status_at), the
// accounting pass (cts_media_stream_conns_accumulate), the render tick (cts_media_stream_conns_render), the close
// (cts_media_stream_conns_close) and the *_udp reads.
//
// A translation unit of its own, like cts_connections.cpp: nothing else in the library references these entry points
// or their launchers, so whatever links the other files against its own launchers keeps linking.
#include <hip/hip_runtime_api.h>

#include <algorithm>

#include "cts_internal.hpp"
#include "cts_media_stream_conns.h"

static_assert(sizeof(cts_ms_conn_state) == 112 && alignof(cts_ms_conn_state) == 8, "cts_ms_conn_state: 112 bytes");
static_assert(sizeof(cts_ms_conn_result) == 88 && alignof(cts_ms_conn_result) == 8, "cts_ms_conn_result: 88 bytes");
static_assert(sizeof(cts_datagram_status) == 16, "the accounting pass reads a status as two 8-byte words");

namespace {

using cts::DeviceGuard;
using cts::hip_status;

// ordinal 0xFFFFFFFF is the empty slot: the launch's last ordinal, base_index + n - 1, must stay below it
inline bool ordinals_overflow(uint32_t base_index, uint32_t n) { return (uint64_t)base_index + n > 0xFFFFFFFFull; }

inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0; }

// the entry table and the ring array of n_conns connections: both there (unless there are no connections), both aligned
inline bool tables_bad(const cts_ms_conn_state* conns, const uint64_t* frame_bytes, uint32_t n_conns)
{
    if (n_conns != 0 && (conns == nullptr || frame_bytes == nullptr)) return true;
    return misaligned(conns, 8) || misaligned(frame_bytes, 8);
}

inline cts_counters_udp udp_of(const cts_counters_ex& x)
{
    // a UDP block has a counter block's layout: slot k of one is slot k of the other
    return cts_counters_udp{x.bytes_checked,  x.bytes_ok,         x.buffers_checked,
                            x.buffers_failed, x.mismatched_bytes, x.connections_failed};
}

}  // namespace

extern "C" {

int cts_ms_conn_init(const cts_media_stream_settings* s, uint64_t frame_base, cts_ms_conn_state* out)
{
    if (s == nullptr || out == nullptr) return CTS_E_INVALID;
    // cts_media_stream_client_create's checks (ctsIOPatternMediaStream.cpp:46-96)
    if (s->frame_size_bytes == 0 || s->frames_per_second == 0 || s->stream_length_frames <= 0 ||
        s->stream_length_frames > (int64_t)UINT32_MAX)
        return CTS_E_INVALID;  // FAIL_FAST_IF(m_finalFrame > UINT32_MAX), :53
    const uint32_t initial = std::min<uint32_t>((uint32_t)s->stream_length_frames, s->buffered_frames);
    const uint64_t queue = 2 * (uint64_t)initial;  // extraBufferDepthFactor
    if (queue < 2 || queue > UINT32_MAX) return CTS_E_INVALID;
    *out = cts_ms_conn_state{};
    out->head_sequence_number = 1;
    out->final_frame = s->stream_length_frames;
    out->frame_base = frame_base;
    out->frames = (uint32_t)queue;
    out->frame_size_bytes = s->frame_size_bytes;
    out->initial_buffer_frames = initial;
    out->timer_wheel_offset = initial;
    out->last_error = CTS_STATUS_IO_RUNNING;
    return CTS_OK;
}

int cts_media_stream_verify_status_at(cts_engine* e, const void* dev_arena, uint64_t arena_bytes,
                                      const cts_buf_desc* dev_descs, uint32_t n, uint32_t base_index,
                                      cts_datagram_status* dev_status, void* dev_counters,
                                      uint32_t* dev_conn_first_fail, uint32_t n_conns, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (dev_arena == nullptr || dev_descs == nullptr || misaligned(dev_descs, 8) || misaligned(dev_arena, 16))
        return CTS_E_INVALID;
    if (dev_conn_first_fail == nullptr && n_conns != 0) return CTS_E_INVALID;
    if (misaligned(dev_status, 4) || misaligned(dev_counters, 8) || misaligned(dev_conn_first_fail, 4))
        return CTS_E_INVALID;
    if (ordinals_overflow(base_index, n)) return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    return hip_status(cts::launch_media_stream_status_at(static_cast<const uint8_t*>(dev_arena), arena_bytes, dev_descs,
                                                         n, base_index, dev_status,
                                                         static_cast<uint64_t*>(dev_counters), dev_conn_first_fail,
                                                         n_conns, static_cast<hipStream_t>(stream), geo));
}

int cts_media_stream_conns_accumulate(cts_engine* e, uint64_t arena_bytes, const cts_buf_desc* dev_descs,
                                      const cts_datagram_status* dev_status, uint32_t n, uint32_t base_index,
                                      const uint32_t* dev_conn_first_fail, cts_ms_conn_state* dev_conns,
                                      uint64_t* dev_frame_bytes, uint64_t frame_elems, uint32_t n_conns,
                                      void* dev_udp_counters, void* stream)
{
    (void)arena_bytes;  // a datagram outside the arena is CTS_DGRAM_BAD_DESC in its status already
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (dev_descs == nullptr || misaligned(dev_descs, 8) || dev_status == nullptr || misaligned(dev_status, 8))
        return CTS_E_INVALID;
    if (n_conns != 0 && (dev_conn_first_fail == nullptr || dev_conns == nullptr)) return CTS_E_INVALID;
    if (frame_elems != 0 && dev_frame_bytes == nullptr) return CTS_E_INVALID;
    if (misaligned(dev_conn_first_fail, 4) || misaligned(dev_conns, 8) || misaligned(dev_frame_bytes, 8))
        return CTS_E_INVALID;
    if (dev_udp_counters == nullptr || misaligned(dev_udp_counters, 8)) return CTS_E_INVALID;
    if (ordinals_overflow(base_index, n)) return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    return hip_status(cts::launch_ms_conn_accumulate(dev_descs, dev_status, n, base_index, dev_conn_first_fail,
                                                     dev_conns, dev_frame_bytes, frame_elems, n_conns,
                                                     static_cast<uint64_t*>(dev_udp_counters),
                                                     static_cast<hipStream_t>(stream), geo));
}

int cts_media_stream_conns_render(cts_engine* e, const uint32_t* dev_conn_ids, uint32_t n,
                                  cts_ms_conn_state* dev_conns, uint64_t* dev_frame_bytes, uint32_t n_conns,
                                  void* dev_udp_counters, uint32_t* dev_codes, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (dev_conn_ids == nullptr || misaligned(dev_conn_ids, 4) || misaligned(dev_codes, 4)) return CTS_E_INVALID;
    if (tables_bad(dev_conns, dev_frame_bytes, n_conns)) return CTS_E_INVALID;
    if (dev_udp_counters == nullptr || misaligned(dev_udp_counters, 8)) return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    return hip_status(cts::launch_ms_conn_render(dev_conn_ids, n, dev_conns, dev_frame_bytes, n_conns,
                                                 static_cast<uint64_t*>(dev_udp_counters), dev_codes,
                                                 static_cast<hipStream_t>(stream), geo));
}

int cts_media_stream_conns_close(cts_engine* e, const uint32_t* dev_conn_ids, uint32_t n,
                                 uint32_t* dev_conn_first_fail, cts_ms_conn_state* dev_conns,
                                 uint64_t* dev_frame_bytes, uint32_t n_conns, cts_ms_conn_result* dev_results,
                                 void* dev_close_counters, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (dev_conn_ids == nullptr || misaligned(dev_conn_ids, 4)) return CTS_E_INVALID;
    if (n_conns != 0 && dev_conn_first_fail == nullptr) return CTS_E_INVALID;
    if (misaligned(dev_conn_first_fail, 4) || tables_bad(dev_conns, dev_frame_bytes, n_conns)) return CTS_E_INVALID;
    if (misaligned(dev_results, 8) || dev_close_counters == nullptr || misaligned(dev_close_counters, 8))
        return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    return hip_status(cts::launch_ms_conn_close(dev_conn_ids, n, dev_conn_first_fail, dev_conns, dev_frame_bytes,
                                                n_conns, dev_results, static_cast<uint64_t*>(dev_close_counters),
                                                static_cast<hipStream_t>(stream), geo));
}

// The reads are the *_ex reads: the same fold (and the same ncclAllReduce of count 6) over a block of the same
// layout, its six words named as cts_counters_udp.
int cts_counters_read_udp(cts_engine* e, const void* dev_udp_counters, cts_counters_udp* out, void* stream)
{
    if (out == nullptr) return CTS_E_INVALID;
    cts_counters_ex x{};
    const int rc = cts_counters_read_ex(e, dev_udp_counters, &x, stream);
    if (rc == CTS_OK) *out = udp_of(x);
    return rc;
}

int cts_counters_read_multi_udp(cts_engine* const* engines, const void* const* dev_udp_counters,
                                void* const* streams, uint32_t n, cts_counters_udp* out)
{
    if (out == nullptr) return CTS_E_INVALID;
    cts_counters_ex x{};
    const int rc = cts_counters_read_multi_ex(engines, dev_udp_counters, streams, n, &x);
    if (rc == CTS_OK) *out = udp_of(x);
    return rc;
}

int cts_counters_allreduce_udp(cts_engine* const* engines, const void* const* dev_udp_counters,
                               void* const* streams, uint32_t n, cts_counters_udp* out)
{
    if (out == nullptr) return CTS_E_INVALID;
    cts_counters_ex x{};
    const int rc = cts_counters_allreduce_ex(engines, dev_udp_counters, streams, n, &x);
    if (rc == CTS_OK) *out = udp_of(x);
    return rc;
}

}  // extern "C"
