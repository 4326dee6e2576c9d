// device_ms_servers_timed.cpp — MediaStream servers sending by the clock on the device from C++, through the C ABI only
// (include/cts_media_stream_servers.h; INTEGRATION.md "The frame schedule on the device-resident path"): entries from
// cts_ms_server_init, schedule entries from cts_ms_server_schedule_init, then the host loop of one timer: every
// connection listed in every tick, cts_media_stream_servers_send_at at the clock's now_ms, the clock moved on to the
// tick's next_due_ms. The clock is the program's own, so the run takes no wall time. After every tick the codes, the
// tick block, the entries and the sequence number of every written datagram are held against a restatement of the
// reference's rule, one frame after the other (base + frame * 1000 / fps - now < 2, ctsIOPattern.cpp:1136-1150), and
// against cts_ms_server_frames_due. Built by `make` (ctstraffic_amd/build/device_ms_servers_timed) and run by
// tests/test_cpp_ms_servers_timed.py on the GPU box. Exits non-zero on a failed check.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "cts_media_stream_servers.h"

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) {                                                                     \
            std::fprintf(stderr, "%s:%d CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

namespace {
constexpr uint32_t kConns = 5, kStride = 1472, kCapacity = 24, kMaxFrames = 3;
// frame size, datagram size, frames per second, buffered frames, stream length
const cts_media_stream_settings kSettings[kConns] = {{3000, 1472, 60, 2, 9},
                                                     {1472, 1472, 30, 1, 4},
                                                     {2 * 1400 + 13, 1400, 1000, 3, 40},
                                                     {27, 53, 1, 1, 2},
                                                     {5 * 700, 700, 24, 2, 6}};
const int64_t kBase[kConns] = {10000, 10007, 10100, 9500, 10250};

int64_t due_of(uint32_t c, int64_t frame) { return kBase[c] + frame * 1000LL / kSettings[c].frames_per_second; }
}  // namespace

int main()
{
    cts_engine* e = nullptr;
    CHECK(cts_engine_create(0, &e) == CTS_OK);
    void* stream = nullptr;
    CHECK(cts_engine_stream_create(e, &stream) == CTS_OK);
    hipStream_t s = static_cast<hipStream_t>(stream);

    std::vector<cts_ms_server_state> servers(kConns), model(kConns);
    std::vector<cts_ms_server_schedule> schedule(kConns);
    for (uint32_t c = 0; c < kConns; ++c) {
        CHECK(cts_ms_server_init(&kSettings[c], &servers[c]) == CTS_OK);
        CHECK(cts_ms_server_schedule_init(&kSettings[c], kBase[c], &schedule[c]) == CTS_OK);
        CHECK(schedule[c].base_time_ms == kBase[c] && schedule[c].frames_per_second == kSettings[c].frames_per_second);
    }
    model = servers;
    cts_ms_server_schedule refused{};
    const cts_media_stream_settings still{3000, 1472, 0, 2, 4};
    CHECK(cts_ms_server_schedule_init(&still, 0, &refused) == CTS_E_INVALID);
    CHECK(cts_ms_server_schedule_init(&kSettings[0], -1, &refused) == CTS_E_INVALID);
    CHECK(cts_ms_server_schedule_init(&kSettings[0], (int64_t)1 << 62, &refused) == CTS_E_INVALID);

    const uint64_t arena_bytes = (uint64_t)kCapacity * kStride;
    const size_t scratch_bytes = cts_media_stream_servers_timed_scratch_bytes(kConns);
    CHECK(scratch_bytes >= cts_media_stream_servers_scratch_bytes(kConns) + kConns * sizeof(uint64_t));
    void *arena = nullptr, *descs = nullptr, *lengths = nullptr, *udp = nullptr, *dservers = nullptr,
         *dschedule = nullptr, *ids = nullptr, *codes = nullptr, *tick = nullptr, *scratch = nullptr;
    CHECK(hipMalloc(&arena, arena_bytes) == hipSuccess);
    CHECK(hipMalloc(&descs, kCapacity * sizeof(cts_buf_desc)) == hipSuccess);
    CHECK(hipMalloc(&lengths, kCapacity * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&udp, cts_counters_device_bytes()) == hipSuccess);
    CHECK(hipMalloc(&dservers, kConns * sizeof(cts_ms_server_state)) == hipSuccess);
    CHECK(hipMalloc(&dschedule, kConns * sizeof(cts_ms_server_schedule)) == hipSuccess);
    CHECK(hipMalloc(&ids, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&codes, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&tick, sizeof(cts_ms_server_timed_tick)) == hipSuccess);
    CHECK(hipMalloc(&scratch, scratch_bytes) == hipSuccess);
    CHECK(hipMemsetAsync(arena, 0xA5, arena_bytes, s) == hipSuccess);
    CHECK(hipMemcpyAsync(dservers, servers.data(), kConns * sizeof(cts_ms_server_state), hipMemcpyHostToDevice, s) ==
          hipSuccess);
    CHECK(hipMemcpyAsync(dschedule, schedule.data(), kConns * sizeof(cts_ms_server_schedule), hipMemcpyHostToDevice,
                         s) == hipSuccess);
    CHECK(cts_counters_reset(e, udp, stream) == CTS_OK);
    const uint32_t order[kConns] = {3, 0, 4, 1, 2};  // the listed order is the ring's order
    CHECK(hipMemcpyAsync(ids, order, sizeof(order), hipMemcpyHostToDevice, s) == hipSuccess);

    cts_buf_desc* dd = static_cast<cts_buf_desc*>(descs);
    uint32_t* dids = static_cast<uint32_t*>(ids);
    cts_ms_server_state* sv = static_cast<cts_ms_server_state*>(dservers);
    cts_ms_server_schedule* sc = static_cast<cts_ms_server_schedule*>(dschedule);
    cts_ms_server_timed_tick* dtick = static_cast<cts_ms_server_timed_tick*>(tick);

    // a refused argument launches nothing
    CHECK(cts_media_stream_servers_send_at(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, sv, nullptr, kConns,
                                           kMaxFrames, 0, 1, 2, dd, static_cast<uint32_t*>(lengths),
                                           static_cast<uint32_t*>(codes), dtick, udp, scratch, scratch_bytes,
                                           stream) == CTS_E_INVALID);
    CHECK(cts_media_stream_servers_send_at(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, sv, sc, kConns, 0,
                                           0, 1, 2, dd, static_cast<uint32_t*>(lengths), static_cast<uint32_t*>(codes),
                                           dtick, udp, scratch, scratch_bytes, stream) == CTS_E_INVALID);
    CHECK(cts_media_stream_servers_send_at(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, sv, sc, kConns,
                                           kMaxFrames, -1, 1, 2, dd, static_cast<uint32_t*>(lengths),
                                           static_cast<uint32_t*>(codes), dtick, udp, scratch, scratch_bytes,
                                           stream) == CTS_E_INVALID);
    CHECK(cts_media_stream_servers_send_at(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, sv, sc, kConns,
                                           kMaxFrames, 0, 1, 2, dd, static_cast<uint32_t*>(lengths),
                                           static_cast<uint32_t*>(codes), dtick, udp, scratch,
                                           cts_media_stream_servers_scratch_bytes(kConns), stream) == CTS_E_INVALID);

    // ---- the host loop: one timer, every connection listed in every tick ----
    int64_t now = 0;
    uint64_t sent_bits = 0, sent_datagrams = 0, ticks = 0, idle_ticks = 0;
    std::vector<uint8_t> ring(arena_bytes);
    std::vector<uint32_t> got_codes(kConns);
    for (;; ++ticks) {
        CHECK(ticks < 500);
        CHECK(cts_media_stream_servers_send_at(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, sv, sc, kConns,
                                               kMaxFrames, now, 1000 + now, 10000000, dd,
                                               static_cast<uint32_t*>(lengths), static_cast<uint32_t*>(codes), dtick, udp,
                                               scratch, scratch_bytes, stream) == CTS_OK);
        cts_ms_server_timed_tick t{};
        CHECK(hipMemcpyAsync(&t, tick, sizeof(t), hipMemcpyDeviceToHost, s) == hipSuccess);
        CHECK(hipMemcpyAsync(got_codes.data(), codes, kConns * sizeof(uint32_t), hipMemcpyDeviceToHost, s) == hipSuccess);
        CHECK(hipMemcpyAsync(servers.data(), dservers, kConns * sizeof(cts_ms_server_state), hipMemcpyDeviceToHost, s) ==
              hipSuccess);
        CHECK(hipMemcpyAsync(ring.data(), arena, arena_bytes, hipMemcpyDeviceToHost, s) == hipSuccess);
        CHECK(hipStreamSynchronize(s) == hipSuccess);

        // the restatement: one connection after the other in listed order, one frame after the other
        uint32_t slot = 0, frames = 0, waiting = 0, sent = 0, finished = 0, no_room = 0, skipped = 0;
        uint64_t bytes = 0;
        int64_t next_due = INT64_MAX;
        bool cut = false;  // a connection cut by the capacity leaves no room to those after it
        for (uint32_t i = 0; i < kConns; ++i) {
            const uint32_t c = order[i];
            cts_ms_server_state& m = model[c];
            uint32_t code = CTS_MS_SERVER_ENDED;
            if (m.finished != 0) {
                ++skipped;
            } else {
                uint32_t out = 0;
                while (m.current_frame + out <= m.final_frame && out < kMaxFrames &&
                       due_of(c, m.current_frame + out) - now < 2)
                    ++out;
                uint32_t by_closed_form = 0;
                int64_t then = 0;
                CHECK(cts_ms_server_frames_due(&m, &schedule[c], now, kMaxFrames, &by_closed_form, &then) == CTS_OK);
                CHECK(by_closed_form == out);
                CHECK(then == (m.current_frame + out <= m.final_frame ? due_of(c, m.current_frame + out) : INT64_MAX));
                const uint32_t k = m.datagrams_per_frame;
                uint32_t take = 0;
                while (!cut && take < out && slot + (take + 1) * k <= kCapacity) ++take;
                if (out == 0) {
                    code = CTS_MS_SERVER_WAITING;
                    ++waiting;
                } else if (take == 0) {
                    code = CTS_MS_SERVER_NO_ROOM;
                    ++no_room;
                } else {
                    for (uint32_t q = 0; q < take * k; ++q) {
                        int64_t seq = 0, qpc = 0;
                        std::memcpy(&seq, &ring[(uint64_t)(slot + q) * kStride + 2], 8);
                        std::memcpy(&qpc, &ring[(uint64_t)(slot + q) * kStride + 10], 8);
                        CHECK(seq == m.current_frame + q / k && qpc == 1000 + now);
                    }
                    slot += take * k;
                    frames += take;
                    bytes += (uint64_t)take * m.frame_size_bytes;
                    m.bits_sent += 8ull * take * m.frame_size_bytes;
                    m.datagrams_sent += (uint64_t)take * k;
                    m.current_frame += take;
                    ++sent;
                    code = CTS_MS_SERVER_SENT;
                    if (m.current_frame > m.final_frame) {
                        m.finished = 1;
                        ++finished;
                        code = CTS_MS_SERVER_FINISHED;
                    }
                }
                if (take < out) cut = true;
                if (m.finished == 0 && due_of(c, m.current_frame) < next_due) next_due = due_of(c, m.current_frame);
            }
            CHECK(got_codes[i] == code);
            CHECK(std::memcmp(&servers[c], &m, sizeof(m)) == 0);
        }
        CHECK(t.tick.datagrams == slot && t.tick.bytes == bytes && t.frames == frames);
        CHECK(t.tick.connections_sent == sent && t.tick.connections_finished == finished);
        CHECK(t.tick.connections_no_room == no_room && t.tick.connections_skipped == skipped);
        CHECK(t.connections_waiting == waiting && t.next_due_ms == next_due);
        sent_bits += 8 * bytes;
        sent_datagrams += slot;
        idle_ticks += slot == 0;
        if (t.next_due_ms == INT64_MAX) break;  // every stream has ended
        // the timer: a value <= now + 1 means "tick again once the ring is drained" (here: at once)
        if (t.next_due_ms - 1 > now) now = t.next_due_ms - 1;
    }
    uint64_t all_bits = 0;
    for (uint32_t c = 0; c < kConns; ++c) {
        CHECK(servers[c].finished == 1 && servers[c].current_frame == kSettings[c].stream_length_frames + 1);
        all_bits += 8ull * kSettings[c].frame_size_bytes * (uint64_t)kSettings[c].stream_length_frames;
    }
    cts_counters_udp from_servers{};
    CHECK(cts_counters_read_udp(e, udp, &from_servers, stream) == CTS_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    CHECK(sent_bits == all_bits && from_servers.bits_received == all_bits && from_servers.datagrams == sent_datagrams);
    CHECK(idle_ticks >= 1);  // the first tick, before any base

    for (void* p : {arena, descs, lengths, udp, dservers, dschedule, ids, codes, tick, scratch})
        CHECK(hipFree(p) == hipSuccess);
    CHECK(cts_engine_stream_destroy(e, stream) == CTS_OK);
    CHECK(cts_engine_destroy(e) == CTS_OK);
    std::printf("device_ms_servers_timed: ok (%llu ticks)\n", (unsigned long long)ticks + 1);
    return 0;
}
