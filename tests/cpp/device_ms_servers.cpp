// device_ms_servers.cpp — a whole MediaStream exchange on the device from C++, through the C ABI only
// (include/cts_media_stream_servers.h; INTEGRATION.md "MediaStream servers on the device-resident path"): servers from
// cts_ms_server_init, clients from cts_ms_conn_init, and per tick cts_media_stream_servers_send ->
// cts_media_stream_verify_status_at -> cts_media_stream_conns_accumulate -> cts_media_stream_conns_render over the
// descriptors the servers wrote, with the receive pass's n computed from the settings and nothing read back inside the
// loop; then cts_media_stream_conns_close. One tick's ring is also written by cts_media_stream_fill_strided from
// host-built lengths and headers and compared byte for byte. Built by `make` (ctstraffic_amd/build/device_ms_servers)
// and run by tests/test_cpp_ms_servers.py on the GPU box. Exits non-zero on a failed check.
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
constexpr uint32_t kConns = 5, kStride = 1472;
// frame size, datagram size, frames per second, buffered frames, stream length
const cts_media_stream_settings kSettings[kConns] = {{3000, 1472, 60, 2, 4},
                                                     {1472, 1472, 60, 1, 2},
                                                     {2 * 1400 + 13, 1400, 60, 3, 3},
                                                     {27, 53, 60, 1, 1},
                                                     {5 * 700, 700, 60, 2, 4}};
}  // namespace

int main()
{
    cts_engine* e = nullptr;
    CHECK(cts_engine_create(0, &e) == CTS_OK);
    void* stream = nullptr;
    CHECK(cts_engine_stream_create(e, &stream) == CTS_OK);
    hipStream_t s = static_cast<hipStream_t>(stream);

    std::vector<cts_ms_server_state> servers(kConns);
    std::vector<cts_ms_conn_state> clients(kConns);
    std::vector<std::vector<uint32_t>> lens(kConns);
    uint64_t frame_elems = 0;
    uint32_t capacity = 0;
    int64_t ticks = 0;
    for (uint32_t c = 0; c < kConns; ++c) {
        CHECK(cts_ms_server_init(&kSettings[c], &servers[c]) == CTS_OK);
        CHECK(cts_ms_conn_init(&kSettings[c], frame_elems, &clients[c]) == CTS_OK);
        frame_elems += clients[c].frames;
        lens[c].resize(cts_media_stream_split(kSettings[c].frame_size_bytes, kSettings[c].datagram_max_size, nullptr, 0));
        CHECK(cts_media_stream_split(kSettings[c].frame_size_bytes, kSettings[c].datagram_max_size, lens[c].data(),
                                     lens[c].size()) == lens[c].size());
        CHECK(servers[c].datagrams_per_frame == lens[c].size() && servers[c].current_frame == 1);
        capacity += servers[c].datagrams_per_frame;
        if (kSettings[c].stream_length_frames > ticks) ticks = kSettings[c].stream_length_frames;
    }
    cts_ms_server_state refused{};
    const cts_media_stream_settings tiny{3000, CTS_MS_SERVER_MIN_DATAGRAM - 1, 60, 2, 4}, empty{26, 1400, 60, 2, 4};
    CHECK(cts_ms_server_init(&tiny, &refused) == CTS_E_INVALID && cts_ms_server_init(&empty, &refused) == CTS_E_INVALID);

    const uint64_t arena_bytes = (uint64_t)capacity * kStride;
    const size_t scratch_bytes = cts_media_stream_servers_scratch_bytes(kConns);
    void *arena = nullptr, *arena2 = nullptr, *descs = nullptr, *lengths = nullptr, *headers = nullptr,
         *status = nullptr, *udp_s = nullptr, *udp_c = nullptr, *closes = nullptr, *cff = nullptr, *dservers = nullptr,
         *dclients = nullptr, *ring = nullptr, *ids = nullptr, *codes = nullptr, *tick = nullptr, *scratch = nullptr,
         *results = nullptr, *payload = nullptr;
    CHECK(hipMalloc(&arena, arena_bytes) == hipSuccess && hipMalloc(&arena2, arena_bytes) == hipSuccess);
    CHECK(hipMalloc(&descs, capacity * sizeof(cts_buf_desc)) == hipSuccess);
    CHECK(hipMalloc(&lengths, capacity * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&headers, capacity * sizeof(cts_datagram_header)) == hipSuccess);
    CHECK(hipMalloc(&status, capacity * sizeof(cts_datagram_status)) == hipSuccess);
    for (void** p : {&udp_s, &udp_c, &closes, &payload}) CHECK(hipMalloc(p, cts_counters_device_bytes()) == hipSuccess);
    CHECK(hipMalloc(&cff, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&dservers, kConns * sizeof(cts_ms_server_state)) == hipSuccess);
    CHECK(hipMalloc(&dclients, kConns * sizeof(cts_ms_conn_state)) == hipSuccess);
    CHECK(hipMalloc(&ring, frame_elems * sizeof(uint64_t)) == hipSuccess);
    CHECK(hipMalloc(&ids, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&codes, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&tick, sizeof(cts_ms_server_tick)) == hipSuccess);
    CHECK(hipMalloc(&scratch, scratch_bytes) == hipSuccess);
    CHECK(hipMalloc(&results, kConns * sizeof(cts_ms_conn_result)) == hipSuccess);
    CHECK(hipMemsetAsync(arena, 0xA5, arena_bytes, s) == hipSuccess);
    CHECK(hipMemsetAsync(arena2, 0xA5, arena_bytes, s) == hipSuccess);
    CHECK(hipMemsetAsync(cff, 0xFF, kConns * sizeof(uint32_t), s) == hipSuccess);  // every slot empty
    CHECK(hipMemsetAsync(ring, 0, frame_elems * sizeof(uint64_t), s) == hipSuccess);
    CHECK(hipMemcpyAsync(dservers, servers.data(), kConns * sizeof(cts_ms_server_state), hipMemcpyHostToDevice, s) ==
          hipSuccess);
    CHECK(hipMemcpyAsync(dclients, clients.data(), kConns * sizeof(cts_ms_conn_state), hipMemcpyHostToDevice, s) ==
          hipSuccess);
    for (void* p : {udp_s, udp_c, closes, payload}) CHECK(cts_counters_reset(e, p, stream) == CTS_OK);
    const uint32_t order[kConns] = {3, 0, 4, 1, 2};  // the listed order is the ring's order
    CHECK(hipMemcpyAsync(ids, order, sizeof(order), hipMemcpyHostToDevice, s) == hipSuccess);

    cts_buf_desc* dd = static_cast<cts_buf_desc*>(descs);
    cts_datagram_status* dstatus = static_cast<cts_datagram_status*>(status);
    uint32_t* dids = static_cast<uint32_t*>(ids);
    cts_ms_server_state* sv = static_cast<cts_ms_server_state*>(dservers);
    cts_ms_conn_state* cl = static_cast<cts_ms_conn_state*>(dclients);

    // a refused argument launches nothing
    CHECK(cts_media_stream_servers_send(e, arena, arena_bytes, kStride + 8, 0, capacity, dids, kConns, sv, kConns, 1, 2,
                                        dd, static_cast<uint32_t*>(lengths), static_cast<uint32_t*>(codes),
                                        static_cast<cts_ms_server_tick*>(tick), udp_s, scratch, scratch_bytes,
                                        stream) == CTS_E_INVALID);
    CHECK(cts_media_stream_servers_send(e, arena, arena_bytes, kStride, 1, capacity, dids, kConns, sv, kConns, 1, 2, dd,
                                        static_cast<uint32_t*>(lengths), static_cast<uint32_t*>(codes),
                                        static_cast<cts_ms_server_tick*>(tick), udp_s, scratch, scratch_bytes,
                                        stream) == CTS_E_INVALID);

    // ---- the exchange: nothing is read back inside the loop ----
    uint32_t ordinal = 0;
    uint64_t sent_bytes = 0, payload_bytes = 0;
    for (int64_t t = 0; t < ticks; ++t) {
        uint32_t n = 0;  // from the settings: a running connection sends its split's datagrams per tick
        for (uint32_t c = 0; c < kConns; ++c) {
            if (t >= kSettings[c].stream_length_frames) continue;
            n += (uint32_t)lens[c].size();
            sent_bytes += kSettings[c].frame_size_bytes;
            payload_bytes += kSettings[c].frame_size_bytes - CTS_UDP_DATA_HEADER_LENGTH * lens[c].size();
        }
        CHECK(cts_media_stream_servers_send(e, arena, arena_bytes, kStride, 0, capacity, dids, kConns, sv, kConns,
                                            1000 + t, 10000000, dd, static_cast<uint32_t*>(lengths),
                                            static_cast<uint32_t*>(codes), static_cast<cts_ms_server_tick*>(tick),
                                            udp_s, scratch, scratch_bytes, stream) == CTS_OK);
        if (t == 0) {
            // the same tick through the host-fed ring fill: lengths and headers built here, one by one
            std::vector<uint32_t> hl;
            std::vector<cts_datagram_header> hh;
            for (uint32_t c : order)
                for (uint32_t len : lens[c]) {
                    hl.push_back(len);
                    hh.push_back(cts_datagram_header{1, 1000, 10000000});
                }
            CHECK(hl.size() == n && n == capacity);
            void* hlen = nullptr;
            CHECK(hipMalloc(&hlen, n * sizeof(uint32_t)) == hipSuccess);
            CHECK(hipMemcpyAsync(hlen, hl.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s) == hipSuccess);
            CHECK(hipMemcpyAsync(headers, hh.data(), n * sizeof(cts_datagram_header), hipMemcpyHostToDevice, s) ==
                  hipSuccess);
            CHECK(cts_media_stream_fill_strided(e, arena2, arena_bytes, kStride, static_cast<uint32_t*>(hlen),
                                                static_cast<cts_datagram_header*>(headers), n, stream) == CTS_OK);
            std::vector<uint8_t> a(arena_bytes), b(arena_bytes);
            std::vector<uint32_t> dl(n);
            CHECK(hipMemcpyAsync(a.data(), arena, arena_bytes, hipMemcpyDeviceToHost, s) == hipSuccess);
            CHECK(hipMemcpyAsync(b.data(), arena2, arena_bytes, hipMemcpyDeviceToHost, s) == hipSuccess);
            CHECK(hipMemcpyAsync(dl.data(), lengths, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s) == hipSuccess);
            CHECK(hipStreamSynchronize(s) == hipSuccess);
            CHECK(a == b && dl == hl);
            CHECK(hipFree(hlen) == hipSuccess);
        }
        CHECK(cts_media_stream_verify_status_at(e, arena, arena_bytes, dd, n, ordinal, dstatus, nullptr,
                                                static_cast<uint32_t*>(cff), kConns, stream) == CTS_OK);
        CHECK(cts_media_stream_conns_accumulate(e, arena_bytes, dd, dstatus, n, ordinal, static_cast<uint32_t*>(cff), cl,
                                                static_cast<uint64_t*>(ring), frame_elems, kConns, udp_c,
                                                stream) == CTS_OK);
        CHECK(cts_verify(e, arena, arena_bytes, dd, n, 0, nullptr, payload, nullptr, 0, stream) == CTS_OK);
        CHECK(cts_media_stream_conns_render(e, dids, kConns, cl, static_cast<uint64_t*>(ring), kConns, udp_c, nullptr,
                                            stream) == CTS_OK);
        ordinal += n;
    }
    // one tick more: every server has finished and sends nothing
    CHECK(cts_media_stream_servers_send(e, arena, arena_bytes, kStride, 0, capacity, dids, kConns, sv, kConns, 0, 1, dd,
                                        static_cast<uint32_t*>(lengths), static_cast<uint32_t*>(codes),
                                        static_cast<cts_ms_server_tick*>(tick), udp_s, scratch, scratch_bytes,
                                        stream) == CTS_OK);
    CHECK(cts_media_stream_conns_close(e, dids, kConns, static_cast<uint32_t*>(cff), cl, static_cast<uint64_t*>(ring),
                                       kConns, static_cast<cts_ms_conn_result*>(results), closes, stream) == CTS_OK);

    std::vector<cts_ms_conn_result> r(kConns);
    std::vector<uint32_t> got_codes(kConns);
    cts_ms_server_tick last{};
    CHECK(hipMemcpyAsync(r.data(), results, kConns * sizeof(cts_ms_conn_result), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipMemcpyAsync(servers.data(), dservers, kConns * sizeof(cts_ms_server_state), hipMemcpyDeviceToHost, s) ==
          hipSuccess);
    CHECK(hipMemcpyAsync(got_codes.data(), codes, kConns * sizeof(uint32_t), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipMemcpyAsync(&last, tick, sizeof(last), hipMemcpyDeviceToHost, s) == hipSuccess);
    cts_counters_udp from_servers{}, from_clients{};
    cts_counters_close closed{};
    cts_counters clean{};
    CHECK(cts_counters_read_udp(e, udp_s, &from_servers, stream) == CTS_OK);
    CHECK(cts_counters_read_udp(e, udp_c, &from_clients, stream) == CTS_OK);
    CHECK(cts_counters_read_close(e, closes, &closed, stream) == CTS_OK);
    CHECK(cts_counters_read(e, payload, &clean, stream) == CTS_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    uint64_t frames = 0;
    for (uint32_t i = 0; i < kConns; ++i) {
        const uint32_t c = order[i];
        const cts_media_stream_settings& cfg = kSettings[c];
        CHECK(r[i].conn_index == c && r[i].status == 0 && r[i].flags == 0 && r[i].finished == CTS_MS_CONN_FINISHED);
        CHECK(r[i].successful_frames == (uint64_t)cfg.stream_length_frames);
        CHECK(r[i].dropped_frames == 0 && r[i].duplicate_frames == 0 && r[i].error_frames == 0);
        CHECK(r[i].datagrams_after_end == 0 && r[i].datagrams == servers[c].datagrams_sent);
        CHECK(r[i].bits_received == servers[c].bits_sent);
        CHECK(servers[c].bits_sent == 8ull * cfg.frame_size_bytes * (uint64_t)cfg.stream_length_frames);
        CHECK(servers[c].finished == 1 && servers[c].current_frame == cfg.stream_length_frames + 1);
        CHECK(got_codes[i] == CTS_MS_SERVER_ENDED);
        frames += (uint64_t)cfg.stream_length_frames;
    }
    CHECK(last.datagrams == 0 && last.bytes == 0 && last.connections_sent == 0 && last.connections_skipped == kConns);
    CHECK(from_servers.bits_received == 8 * sent_bytes && from_servers.datagrams == ordinal);
    CHECK(from_clients.bits_received == from_servers.bits_received && from_clients.datagrams == ordinal);
    CHECK(from_clients.successful_frames == frames && from_clients.dropped_frames == 0 &&
          from_clients.duplicate_frames == 0 && from_clients.error_frames == 0);
    CHECK(closed.connections_closed == kConns && closed.successful == kConns && closed.bytes_recv == sent_bytes);
    CHECK(clean.bytes_checked == payload_bytes && clean.bytes_ok == payload_bytes && clean.buffers_failed == 0 &&
          clean.buffers_checked == ordinal);

    for (void* p : {arena, arena2, descs, lengths, headers, status, udp_s, udp_c, closes, cff, dservers, dclients, ring,
                    ids, codes, tick, scratch, results, payload})
        CHECK(hipFree(p) == hipSuccess);
    CHECK(cts_engine_stream_destroy(e, stream) == CTS_OK);
    CHECK(cts_engine_destroy(e) == CTS_OK);
    std::printf("device_ms_servers: ok\n");
    return 0;
}
