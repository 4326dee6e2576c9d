// device_ms_connections.cpp — MediaStream connections on the device-resident path from C++, through the C ABI only
// (include/cts_media_stream_conns.h; INTEGRATION.md "MediaStream connections on the device-resident path"): entries
// from cts_ms_conn_init, cts_media_stream_fill as the sender, a flipped byte, two batches through
// cts_media_stream_verify_status_at and cts_media_stream_conns_accumulate, a render tick, cts_media_stream_conns_close,
// every result, the UDP block and the close block checked against one host cts_media_stream_client per connection fed
// with the same statuses, then a second stream through every recycled slot. Built by `make`
// (ctstraffic_amd/build/device_ms_connections) and run by tests/test_cpp_ms_connections.py on the GPU box. Exits
// non-zero on a failed check.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "cts_media_stream_conns.h"

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) {                                                                     \
            std::fprintf(stderr, "%s:%d CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

namespace {
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kConns = 6, kMaxDatagram = 1472, kFrame = 3000;
constexpr uint32_t kSilent = 4;   // receives nothing: FatalAbort at the tick
constexpr uint32_t kCorrupt = 2;  // a flipped payload byte in its second datagram

struct Batch {
    std::vector<cts_buf_desc> descs;
    std::vector<cts_datagram_header> headers;
};

// frame `seq` of every connection but the silent one, connection-major; `extra_seq` != 0: one more datagram with that
// sequence number for the last connection
Batch make_batch(const std::vector<uint32_t>& lens, int64_t seq, int64_t extra_seq, uint64_t* off)
{
    Batch b;
    for (uint32_t c = 0; c < kConns; ++c) {
        if (c == kSilent) continue;
        for (uint32_t len : lens) {
            b.descs.push_back(cts_buf_desc{*off, len, 0, c, CTS_UDP_DATA_HEADER_LENGTH});
            b.headers.push_back(cts_datagram_header{seq, 0, 0});
            *off += (len + 15u) & ~15u;
        }
    }
    if (extra_seq != 0) {
        b.descs.push_back(cts_buf_desc{*off, lens[0], 0, kConns - 1, CTS_UDP_DATA_HEADER_LENGTH});
        b.headers.push_back(cts_datagram_header{extra_seq, 0, 0});
        *off += (lens[0] + 15u) & ~15u;
    }
    return b;
}
}  // namespace

int main()
{
    cts_engine* e = nullptr;
    CHECK(cts_engine_create(0, &e) == CTS_OK);
    void* stream = nullptr;
    CHECK(cts_engine_stream_create(e, &stream) == CTS_OK);
    hipStream_t s = static_cast<hipStream_t>(stream);

    // six clients: frames of 3000 bytes as three datagrams (1472, 1472, 56), four frames long, two buffered: a window
    // of four frames each, the rings one after the other
    const cts_media_stream_settings cfg{kFrame, kMaxDatagram, 60, 2, 4};
    std::vector<uint32_t> lens(cts_media_stream_split(kFrame, kMaxDatagram, nullptr, 0));
    CHECK(lens.size() == 3 && cts_media_stream_split(kFrame, kMaxDatagram, lens.data(), lens.size()) == 3);
    std::vector<cts_ms_conn_state> fresh(kConns);
    uint64_t frame_elems = 0;
    for (uint32_t c = 0; c < kConns; ++c) {
        CHECK(cts_ms_conn_init(&cfg, frame_elems, &fresh[c]) == CTS_OK);
        CHECK(fresh[c].frames == 4 && fresh[c].last_error == CTS_STATUS_IO_RUNNING);
        frame_elems += fresh[c].frames;
    }
    cts_ms_conn_state refused{};
    const cts_media_stream_settings none{kFrame, kMaxDatagram, 60, 0, 4};  // nothing buffered: no queue
    CHECK(cts_ms_conn_init(&none, 0, &refused) == CTS_E_INVALID);

    uint64_t arena_bytes = 0;
    // two batches of the first streams (frame 1 with a stray sequence number 99, then frame 2), one of the second
    Batch b[3] = {make_batch(lens, 1, 99, &arena_bytes), make_batch(lens, 2, 0, &arena_bytes),
                  make_batch(lens, 1, 0, &arena_bytes)};
    const uint32_t n_max = (uint32_t)b[0].descs.size();
    const uint32_t n_ids = kConns + 1;  // every connection and one id without a slot

    void *arena = nullptr, *descs = nullptr, *headers = nullptr, *status = nullptr, *ctr = nullptr, *udp = nullptr,
         *closes = nullptr, *cff = nullptr, *conns = nullptr, *ring = nullptr, *ids = nullptr, *codes = nullptr,
         *results = nullptr;
    CHECK(hipMalloc(&arena, arena_bytes) == hipSuccess);
    CHECK(hipMalloc(&descs, n_max * sizeof(cts_buf_desc)) == hipSuccess);
    CHECK(hipMalloc(&headers, n_max * sizeof(cts_datagram_header)) == hipSuccess);
    CHECK(hipMalloc(&status, n_max * sizeof(cts_datagram_status)) == hipSuccess);
    CHECK(hipMalloc(&ctr, cts_counters_device_bytes()) == hipSuccess);
    CHECK(hipMalloc(&udp, cts_counters_device_bytes()) == hipSuccess);
    CHECK(hipMalloc(&closes, cts_counters_device_bytes()) == hipSuccess);
    CHECK(hipMalloc(&cff, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&conns, kConns * sizeof(cts_ms_conn_state)) == hipSuccess);
    CHECK(hipMalloc(&ring, frame_elems * sizeof(uint64_t)) == hipSuccess);
    CHECK(hipMalloc(&ids, n_ids * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&codes, n_ids * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&results, n_ids * sizeof(cts_ms_conn_result)) == hipSuccess);
    cts_buf_desc* dd = static_cast<cts_buf_desc*>(descs);
    cts_datagram_status* dstatus = static_cast<cts_datagram_status*>(status);
    uint32_t* slots = static_cast<uint32_t*>(cff);
    cts_ms_conn_state* entries = static_cast<cts_ms_conn_state*>(conns);
    uint64_t* frame_bytes = static_cast<uint64_t*>(ring);
    CHECK(hipMemsetAsync(arena, 0, arena_bytes, s) == hipSuccess);
    CHECK(hipMemsetAsync(cff, 0xFF, kConns * sizeof(uint32_t), s) == hipSuccess);  // every slot empty
    CHECK(hipMemsetAsync(ring, 0, frame_elems * sizeof(uint64_t), s) == hipSuccess);
    CHECK(hipMemcpyAsync(conns, fresh.data(), kConns * sizeof(cts_ms_conn_state), hipMemcpyHostToDevice, s) ==
          hipSuccess);
    CHECK(cts_counters_reset(e, ctr, stream) == CTS_OK && cts_counters_reset(e, udp, stream) == CTS_OK &&
          cts_counters_reset(e, closes, stream) == CTS_OK);
    std::vector<uint32_t> all_ids(n_ids);
    for (uint32_t i = 0; i < n_ids; ++i) all_ids[i] = i;  // the last one, kConns, has no slot
    CHECK(hipMemcpyAsync(ids, all_ids.data(), n_ids * sizeof(uint32_t), hipMemcpyHostToDevice, s) == hipSuccess);

    // the checkers: one host client per connection, fed with the statuses the device wrote
    std::vector<cts_media_stream_client*> client(kConns, nullptr);
    for (auto& c : client) CHECK(cts_media_stream_client_create(&cfg, &c) == CTS_OK);
    cts_udp_status_details_reset();

    uint32_t ordinal = 100;
    uint64_t after_end[kConns] = {};
    auto run_batch = [&](const Batch& bt, bool corrupt) -> int {
        const uint32_t n = (uint32_t)bt.descs.size();
        CHECK(hipMemcpyAsync(descs, bt.descs.data(), n * sizeof(cts_buf_desc), hipMemcpyHostToDevice, s) == hipSuccess);
        CHECK(hipMemcpyAsync(headers, bt.headers.data(), n * sizeof(cts_datagram_header), hipMemcpyHostToDevice, s) ==
              hipSuccess);
        CHECK(cts_media_stream_fill(e, arena, arena_bytes, dd, static_cast<cts_datagram_header*>(headers), n, stream) ==
              CTS_OK);
        if (corrupt) {  // the second datagram of connection kCorrupt: one payload byte flipped
            const cts_buf_desc& d = bt.descs[kCorrupt * 3 + 1];
            uint8_t* at = static_cast<uint8_t*>(arena) + d.byte_offset + 700;
            uint8_t v = 0;
            CHECK(hipMemcpyAsync(&v, at, 1, hipMemcpyDeviceToHost, s) == hipSuccess);
            CHECK(hipStreamSynchronize(s) == hipSuccess);
            v ^= 0x5A;
            CHECK(hipMemcpyAsync(at, &v, 1, hipMemcpyHostToDevice, s) == hipSuccess);
        }
        CHECK(cts_media_stream_verify_status_at(e, arena, arena_bytes, dd, n, ordinal, dstatus, ctr, slots, kConns,
                                                stream) == CTS_OK);
        CHECK(cts_media_stream_conns_accumulate(e, arena_bytes, dd, dstatus, n, ordinal, slots, entries, frame_bytes,
                                                frame_elems, kConns, udp, stream) == CTS_OK);
        ordinal += n;
        std::vector<cts_datagram_status> st(n);
        CHECK(hipMemcpyAsync(st.data(), status, n * sizeof(cts_datagram_status), hipMemcpyDeviceToHost, s) ==
              hipSuccess);
        CHECK(hipStreamSynchronize(s) == hipSuccess);
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t consumed = 0;
            const uint32_t c = bt.descs[i].conn_index;
            CHECK(cts_media_stream_client_complete_status(client[c], &st[i], 1, 0, 0, &consumed) >= 0);
            after_end[c] += 1u - consumed;
        }
        return 0;
    };
    auto tick = [&](std::vector<uint32_t>* got) -> int {
        CHECK(cts_media_stream_conns_render(e, static_cast<uint32_t*>(ids), n_ids, entries, frame_bytes, kConns, udp,
                                            static_cast<uint32_t*>(codes), stream) == CTS_OK);
        got->assign(n_ids, 77u);
        CHECK(hipMemcpyAsync(got->data(), codes, n_ids * sizeof(uint32_t), hipMemcpyDeviceToHost, s) == hipSuccess);
        CHECK(hipStreamSynchronize(s) == hipSuccess);
        return 0;
    };

    // ---- the first streams: two batches, a tick, the close ----
    if (run_batch(b[0], true) != 0 || run_batch(b[1], false) != 0) return 1;
    std::vector<uint32_t> got_codes;
    if (tick(&got_codes) != 0) return 1;
    for (uint32_t c = 0; c < kConns; ++c) {
        cts_media_stream_stats st{};
        CHECK(cts_media_stream_client_stats(client[c], &st) == CTS_OK);
        const int code = st.last_error == CTS_STATUS_IO_RUNNING ? cts_media_stream_client_render(client[c]) : 0;
        CHECK(got_codes[c] == (uint32_t)code);
    }
    CHECK(got_codes[kSilent] == 2 && got_codes[kCorrupt] == 0 && got_codes[kConns] == 0);
    CHECK(cts_media_stream_conns_close(e, static_cast<uint32_t*>(ids), n_ids, slots, entries, frame_bytes, kConns,
                                       static_cast<cts_ms_conn_result*>(results), closes, stream) == CTS_OK);
    std::vector<cts_ms_conn_result> r(n_ids);
    std::vector<uint32_t> slots_now(kConns);
    std::vector<uint64_t> ring_now(frame_elems);
    CHECK(hipMemcpyAsync(r.data(), results, n_ids * sizeof(cts_ms_conn_result), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipMemcpyAsync(slots_now.data(), cff, kConns * sizeof(uint32_t), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipMemcpyAsync(ring_now.data(), ring, frame_elems * sizeof(uint64_t), hipMemcpyDeviceToHost, s) ==
          hipSuccess);
    cts_counters_udp node{};
    cts_counters_close closed{};
    CHECK(cts_counters_read_udp(e, udp, &node, stream) == CTS_OK);
    CHECK(cts_counters_read_close(e, closes, &closed, stream) == CTS_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    uint64_t datagrams = 0, bytes = 0, ok = 0, data_errors = 0, not_all = 0;
    for (uint32_t c = 0; c < kConns; ++c) {
        cts_media_stream_stats st{};
        CHECK(cts_media_stream_client_stats(client[c], &st) == CTS_OK);
        CHECK(r[c].conn_index == c);
        CHECK(r[c].bits_received == (uint64_t)st.bits_received && r[c].successful_frames == (uint64_t)st.successful_frames);
        CHECK(r[c].dropped_frames == (uint64_t)st.dropped_frames && r[c].duplicate_frames == (uint64_t)st.duplicate_frames);
        CHECK(r[c].error_frames == (uint64_t)st.error_frames && r[c].datagrams == st.datagrams);
        CHECK(r[c].datagrams_after_end == after_end[c] && r[c].head_sequence_number == st.head_sequence_number);
        CHECK(r[c].finished == st.finished);
        const bool running = st.last_error == CTS_STATUS_IO_RUNNING;
        CHECK(r[c].status == (running ? CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED : st.last_error));
        CHECK(((r[c].flags & CTS_MS_CONN_RESULT_FLAG_RUNNING) != 0) == running);
        CHECK(((r[c].flags & CTS_MS_CONN_RESULT_FLAG_HAS_FAILURE) != 0) == (st.has_failure != 0));
        CHECK(r[c].fail_datagram == (st.has_failure ? st.fail_datagram : kEmpty));
        CHECK(slots_now[c] == kEmpty);
        datagrams += st.datagrams;
        bytes += (uint64_t)st.bits_received / 8;
        ok += r[c].status == 0;
        data_errors += r[c].status == CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN;
        not_all += r[c].status == CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED;
    }
    // the corrupt one stopped at its second datagram (ordinal 100 + 3 * kCorrupt + 1), the silent one was aborted, the
    // last one took an error frame for sequence number 99, the others rendered frame 1 and hold frame 2
    CHECK(r[kCorrupt].status == CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN && r[kCorrupt].fail_datagram == 1);
    CHECK(r[kCorrupt].first_fail == 100 + 3 * kCorrupt + 1 && r[kCorrupt].datagrams_after_end == 4);
    CHECK(r[kSilent].finished == CTS_MS_CONN_FATAL && r[kSilent].dropped_frames == 4 && r[kSilent].datagrams == 0);
    CHECK(r[kConns - 1].error_frames == 1 && r[0].successful_frames == 1 && r[0].head_sequence_number == 2);
    CHECK(r[kConns].flags == CTS_MS_CONN_RESULT_FLAG_BAD_CONN && r[kConns].conn_index == kConns &&
          r[kConns].datagrams == 0);
    for (uint64_t v : ring_now) CHECK(v == 0);
    cts_udp_status_details host{};
    CHECK(cts_udp_status_details_read(&host) == CTS_OK);
    CHECK(node.bits_received == (uint64_t)host.bits_received && node.successful_frames == (uint64_t)host.successful_frames);
    CHECK(node.dropped_frames == (uint64_t)host.dropped_frames && node.duplicate_frames == (uint64_t)host.duplicate_frames);
    CHECK(node.error_frames == (uint64_t)host.error_frames && node.datagrams == datagrams);
    CHECK(closed.connections_closed == kConns && closed.successful == ok && closed.data_errors == data_errors);
    CHECK(closed.not_all_data == not_all && closed.too_much_data == 0 && closed.bytes_recv == bytes);
    CHECK(ok == 0 && data_errors == 1 && not_all == kConns - 1);

    // ---- reuse: a datagram that arrives before the fresh entry counts after the end; then a second stream ----
    Batch late;
    late.descs.assign(1, b[2].descs[0]);
    late.headers.assign(1, b[2].headers[0]);
    if (run_batch(late, false) != 0) return 1;
    cts_ms_conn_state e0{};
    CHECK(hipMemcpy(&e0, conns, sizeof(e0), hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(e0.datagrams_after_end == r[0].datagrams_after_end + 1 && e0.datagrams == r[0].datagrams);
    CHECK(e0.finished == CTS_MS_CONN_CLOSED && e0.last_error == CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED);
    CHECK(hipMemcpyAsync(conns, fresh.data(), kConns * sizeof(cts_ms_conn_state), hipMemcpyHostToDevice, s) ==
          hipSuccess);
    for (auto& c : client) {
        CHECK(cts_media_stream_client_destroy(c) == CTS_OK);
        CHECK(cts_media_stream_client_create(&cfg, &c) == CTS_OK);
    }
    std::memset(after_end, 0, sizeof(after_end));
    if (run_batch(b[2], false) != 0) return 1;
    if (tick(&got_codes) != 0) return 1;
    CHECK(got_codes[0] == 0 && got_codes[kSilent] == 2);
    CHECK(cts_media_stream_conns_close(e, static_cast<uint32_t*>(ids), kConns, slots, entries, frame_bytes, kConns,
                                       static_cast<cts_ms_conn_result*>(results), closes, stream) == CTS_OK);
    CHECK(hipMemcpyAsync(r.data(), results, kConns * sizeof(cts_ms_conn_result), hipMemcpyDeviceToHost, s) ==
          hipSuccess);
    CHECK(cts_counters_read_close(e, closes, &closed, stream) == CTS_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    for (uint32_t c = 0; c < kConns; ++c) {
        if (c == kSilent) continue;
        CHECK(r[c].successful_frames == 1 && r[c].datagrams == 3 && r[c].datagrams_after_end == 0);
        CHECK(r[c].bits_received == 8ull * kFrame && r[c].first_fail == kEmpty && r[c].head_sequence_number == 2);
        CHECK(r[c].flags == CTS_MS_CONN_RESULT_FLAG_RUNNING);
    }
    CHECK(closed.connections_closed == 2 * kConns && closed.data_errors == 1);

    for (auto& c : client) CHECK(cts_media_stream_client_destroy(c) == CTS_OK);
    for (void* p : {arena, descs, headers, status, ctr, udp, closes, cff, conns, ring, ids, codes, results})
        CHECK(hipFree(p) == hipSuccess);
    CHECK(cts_engine_stream_destroy(e, stream) == CTS_OK);
    CHECK(cts_engine_destroy(e) == CTS_OK);
    std::printf("device_ms_connections: ok\n");
    return 0;
}
