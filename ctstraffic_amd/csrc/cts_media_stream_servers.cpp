// cts_media_stream_servers.cpp — MediaStream servers on the device-resident path (cts_media_stream_servers.h): the
// host-side entry initialisers (cts_ms_server_init, cts_ms_server_schedule_init), the scratch sizes, the tick
// (cts_media_stream_servers_send), the timed tick (cts_media_stream_servers_send_at) and the schedule's closed form for
// the host (cts_ms_server_frames_due).
//
// A translation unit of its own, like cts_media_stream_conns.cpp: nothing else in the library references these entry
// points or their launchers, so whatever links the other files against its own launchers keeps linking. No threads,
// no allocation.
#include <hip/hip_runtime_api.h>

#include "cts_internal.hpp"
#include "cts_media_stream_servers.h"
#include "cts_ms_server_schedule_math.hpp"

static_assert(sizeof(cts_ms_server_state) == 48 && alignof(cts_ms_server_state) == 8, "cts_ms_server_state: 48 bytes");
static_assert(sizeof(cts_ms_server_tick) == 32 && alignof(cts_ms_server_tick) == 8, "cts_ms_server_tick: 32 bytes");
static_assert(sizeof(cts_counters_udp) == 6 * sizeof(uint64_t), "a UDP block's six words are a counter block's");

namespace {

using cts::DeviceGuard;
using cts::hip_status;

inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0; }

// a time the schedule's arithmetic takes: [0, 2^62)
inline bool time_ok(int64_t ms) { return ms >= 0 && ms < ((int64_t)1 << 62); }

// What both ticks check of the arguments they share, before the engine is used.
bool tick_args_ok(const void* dev_arena, uint64_t arena_bytes, uint32_t stride, uint64_t first_slot, uint32_t capacity,
                  const uint32_t* dev_conn_ids, const void* dev_servers, uint32_t n_conns, const void* dev_descs,
                  const void* dev_lengths, const void* dev_codes, const void* dev_tick, const void* dev_udp_counters,
                  const void* dev_scratch, size_t scratch_bytes, size_t scratch_needed)
{
    if ((stride & 15u) != 0u || stride < 32u || stride > (1u << 20)) return false;
    if (dev_arena == nullptr || misaligned(dev_arena, 16)) return false;
    // (first_slot + capacity) x stride <= arena_bytes, without wrap-around: compared in slots
    if (first_slot > arena_bytes / stride || (uint64_t)capacity > arena_bytes / stride - first_slot) return false;
    if (dev_conn_ids == nullptr || misaligned(dev_conn_ids, 4)) return false;
    if ((n_conns != 0 && dev_servers == nullptr) || misaligned(dev_servers, 8)) return false;
    if (misaligned(dev_descs, 8) || misaligned(dev_lengths, 4) || misaligned(dev_codes, 4) ||
        misaligned(dev_tick, 8) || misaligned(dev_udp_counters, 8))
        return false;
    return dev_scratch != nullptr && !misaligned(dev_scratch, 8) && scratch_bytes >= scratch_needed;
}

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
    if (!tick_args_ok(dev_arena, arena_bytes, stride, first_slot, capacity, dev_conn_ids, dev_servers, n_conns,
                      dev_descs, dev_lengths, dev_codes, dev_tick, dev_udp_counters, dev_scratch, scratch_bytes,
                      cts::MsServerScratch::bytes(n)))
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

int cts_ms_server_schedule_init(const cts_media_stream_settings* s, int64_t base_time_ms, cts_ms_server_schedule* out)
{
    if (s == nullptr || out == nullptr) return CTS_E_INVALID;
    if (s->frames_per_second == 0 || !time_ok(base_time_ms)) return CTS_E_INVALID;
    *out = cts_ms_server_schedule{};
    out->base_time_ms = base_time_ms;
    out->frames_per_second = s->frames_per_second;
    return CTS_OK;
}

size_t cts_media_stream_servers_timed_scratch_bytes(uint32_t n) { return cts::MsServerTimedScratch::bytes(n); }

int cts_ms_server_frames_due(const cts_ms_server_state* state, const cts_ms_server_schedule* schedule, int64_t now_ms,
                             uint32_t max_frames, uint32_t* frames, int64_t* next_due_ms)
{
    if (state == nullptr || schedule == nullptr || max_frames == 0) return CTS_E_INVALID;
    if (schedule->frames_per_second == 0 || !time_ok(schedule->base_time_ms) || !time_ok(now_ms)) return CTS_E_INVALID;
    uint32_t wf = 0;
    int64_t due = INT64_MAX;
    if (state->finished == 0u) {
        wf = cts::ms_schedule_frames(schedule->base_time_ms, schedule->frames_per_second, state->current_frame,
                                     state->final_frame, now_ms, max_frames);
        const int64_t next = state->current_frame + (int64_t)wf;
        if (next <= state->final_frame)
            due = cts::ms_schedule_due(schedule->base_time_ms, schedule->frames_per_second, next);
    }
    if (frames != nullptr) *frames = wf;
    if (next_due_ms != nullptr) *next_due_ms = due;
    return CTS_OK;
}

int cts_media_stream_servers_send_at(cts_engine* e, void* dev_arena, uint64_t arena_bytes, uint32_t stride,
                                     uint64_t first_slot, uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n,
                                     cts_ms_server_state* dev_servers, const cts_ms_server_schedule* dev_schedule,
                                     uint32_t n_conns, uint32_t max_frames, int64_t now_ms, int64_t qpc, int64_t qpf,
                                     cts_buf_desc* dev_descs, uint32_t* dev_lengths, uint32_t* dev_codes,
                                     cts_ms_server_timed_tick* dev_tick, void* dev_udp_counters, void* dev_scratch,
                                     size_t scratch_bytes, void* stream)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (n == 0) return CTS_OK;
    if (!tick_args_ok(dev_arena, arena_bytes, stride, first_slot, capacity, dev_conn_ids, dev_servers, n_conns,
                      dev_descs, dev_lengths, dev_codes, dev_tick, dev_udp_counters, dev_scratch, scratch_bytes,
                      cts::MsServerTimedScratch::bytes(n)))
        return CTS_E_INVALID;
    if ((n_conns != 0 && dev_schedule == nullptr) || misaligned(dev_schedule, 8)) return CTS_E_INVALID;
    if (max_frames == 0 || now_ms < 0) return CTS_E_INVALID;
    int device = 0;
    const cts::LaunchGeometry& geo = cts::engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    const cts::MsServerTimedScratch scratch(dev_scratch, n);
    // the fill reads the tick's datagram count: a caller that wants no tick block gets the scratch's
    cts_ms_server_timed_tick* const tick = dev_tick != nullptr ? dev_tick : scratch.tick;
    hipStream_t const s = static_cast<hipStream_t>(stream);
    const hipError_t rc = cts::launch_ms_server_timed_plan(dev_conn_ids, n, dev_servers, dev_schedule, n_conns, stride,
                                                           capacity, max_frames, now_ms, dev_codes, tick,
                                                           static_cast<uint64_t*>(dev_udp_counters), scratch, s);
    if (rc != hipSuccess) return CTS_E_HIP;
    return hip_status(cts::launch_ms_server_timed_fill(static_cast<uint8_t*>(dev_arena), arena_bytes, stride,
                                                       first_slot, capacity, dev_conn_ids, n, dev_servers, n_conns,
                                                       scratch.prefix, scratch.before, &tick->tick, qpc, qpf,
                                                       dev_descs, dev_lengths, s, geo));
}

}  // extern "C"
