// cts_media_stream_servers.cpp — MediaStream servers on the device-resident path (cts_media_stream_servers.h): the
// host-side entry initialiser (cts_ms_server_init), the scratch size and the tick (cts_media_stream_servers_send).
//
// A translation unit of its own, like cts_media_stream_conns.cpp: nothing else in the library references these entry
// points or their launchers, so whatever links the other files against its own launchers keeps linking. No threads,
// no allocation.
#include <hip/hip_runtime_api.h>

#include "cts_internal.hpp"
#include "cts_media_stream_servers.h"

static_assert(sizeof(cts_ms_server_state) == 48 && alignof(cts_ms_server_state) == 8, "cts_ms_server_state: 48 bytes");
static_assert(sizeof(cts_ms_server_tick) == 32 && alignof(cts_ms_server_tick) == 8, "cts_ms_server_tick: 32 bytes");
static_assert(sizeof(cts_counters_udp) == 6 * sizeof(uint64_t), "a UDP block's six words are a counter block's");

namespace {

using cts::DeviceGuard;
using cts::hip_status;

inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0; }

}  // namespace

extern "C" {

int cts_ms_server_init(const cts_media_stream_settings* s, cts_ms_server_state* out)
{
    if (s == nullptr || out == nullptr) return CTS_E_INVALID;
    // ctsMediaStreamSendRequests FAIL_FASTs on a frame that holds no payload byte (ctsMediaStreamProtocol.hpp:225-227)
    if (s->frame_size_bytes <= CTS_UDP_DATA_HEADER_LENGTH) return CTS_E_INVALID;
    if (s->frames_per_second == 0 || s->stream_length_frames <= 0 || s->stream_length_frames > (int64_t)UINT32_MAX)
        return CTS_E_INVALID;
    // the device's own rule (the reference does not check, ctsConfig.cpp:1232): see CTS_MS_SERVER_MIN_DATAGRAM
    if (s->datagram_max_size < CTS_MS_SERVER_MIN_DATAGRAM) return CTS_E_INVALID;
    *out = cts_ms_server_state{};
    out->current_frame = 1;
    out->final_frame = s->stream_length_frames;
    out->frame_size_bytes = s->frame_size_bytes;
    out->datagram_max_size = s->datagram_max_size;
    out->datagrams_per_frame =
        (uint32_t)(((uint64_t)s->frame_size_bytes + s->datagram_max_size - 1) / s->datagram_max_size);
    return CTS_OK;
}

size_t cts_media_stream_servers_scratch_bytes(uint32_t n) { return cts::MsServerScratch::bytes(n); }

int cts_media_stream_servers_send(cts_engine* e, void* dev_arena, uint64_t arena_bytes, uint32_t stride,
                                  uint64_t first_slot, uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n,
                                  cts_ms_server_state* dev_servers, uint32_t n_conns, int64_t qpc, int64_t qpf,
                                  cts_buf_desc* dev_descs, uint32_t* dev_lengths, uint32_t* dev_codes,
                                  cts_ms_server_tick* dev_tick, void* dev_udp_counters, void* dev_scratch,
                                  size_t scratch_bytes, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if ((stride & 15u) != 0u || stride < 32u || stride > (1u << 20)) return CTS_E_INVALID;
    if (dev_arena == nullptr || misaligned(dev_arena, 16)) return CTS_E_INVALID;
    // (first_slot + capacity) x stride <= arena_bytes, without wrap-around: compared in slots
    if (first_slot > arena_bytes / stride || (uint64_t)capacity > arena_bytes / stride - first_slot)
        return CTS_E_INVALID;
    if (dev_conn_ids == nullptr || misaligned(dev_conn_ids, 4)) return CTS_E_INVALID;
    if ((n_conns != 0 && dev_servers == nullptr) || misaligned(dev_servers, 8)) return CTS_E_INVALID;
    if (misaligned(dev_descs, 8) || misaligned(dev_lengths, 4) || misaligned(dev_codes, 4) ||
        misaligned(dev_tick, 8) || misaligned(dev_udp_counters, 8))
        return CTS_E_INVALID;
    if (dev_scratch == nullptr || misaligned(dev_scratch, 8) || scratch_bytes < cts::MsServerScratch::bytes(n))
        return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    const cts::MsServerScratch scratch(dev_scratch, n);
    // the fill reads the tick's datagram count: a caller that wants no tick block gets the scratch's
    cts_ms_server_tick* const tick = dev_tick != nullptr ? dev_tick : scratch.tick;
    hipStream_t const s = static_cast<hipStream_t>(stream);
    const hipError_t rc = cts::launch_ms_server_plan(dev_conn_ids, n, dev_servers, n_conns, stride, capacity, dev_codes,
                                                     tick, static_cast<uint64_t*>(dev_udp_counters), scratch, s);
    if (rc != hipSuccess) return CTS_E_HIP;
    return hip_status(cts::launch_ms_server_fill(static_cast<uint8_t*>(dev_arena), arena_bytes, stride, first_slot,
                                                 capacity, dev_conn_ids, n, dev_servers, n_conns, scratch.prefix, tick,
                                                 qpc, qpf, dev_descs, dev_lengths, s, geo));
}

}  // extern "C"
