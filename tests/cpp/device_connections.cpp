// device_connections.cpp — the connection lifecycle on the device-resident path from C++, through the C ABI only
// (include/cts_connections.h; INTEGRATION.md "Connection close on the device-resident path"): cts_fill as the
// sender, a few flipped bytes, cts_verify_at, cts_refview_accumulate_conns, a slot rebase, cts_conns_close, every
// result, the close block and the emptied slots checked against values computed here, then a second connection
// through each recycled slot. Built by `make` (ctstraffic_amd/build/device_connections) and run by
// tests/test_cpp_connections.py on the GPU box. Exits non-zero on a failed check.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "cts_connections.h"

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) {                                                                     \
            std::fprintf(stderr, "%s:%d CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

namespace {
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kConns = 24, kPer = 12, kN = kConns * kPer;
}  // namespace

int main()
{
    cts_engine* e = nullptr;
    CHECK(cts_engine_create(0, &e) == CTS_OK);
    void* stream = nullptr;
    CHECK(cts_engine_stream_create(e, &stream) == CTS_OK);
    hipStream_t s = static_cast<hipStream_t>(stream);

    // 24 connections x 12 buffers of ragged lengths, connection-major; expected offsets = per-connection prefix sums
    std::vector<cts_buf_desc> d(kN);
    uint64_t off = 0;
    for (uint32_t c = 0; c < kConns; ++c) {
        uint32_t stream_off = 0;
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t i = c * kPer + k;
            const uint32_t len = 1 + (i * 2654435761u) % 70000u;
            d[i] = cts_buf_desc{off, len, stream_off, c, 0};
            stream_off = (stream_off + len) % CTS_PATTERN_PERIOD;
            off += (len + 15u) & ~15u;
        }
    }
    const uint64_t arena_bytes = off;
    void *arena = nullptr, *descs = nullptr, *ctr = nullptr, *ref = nullptr, *blk = nullptr, *cff = nullptr,
         *state = nullptr, *ids = nullptr, *expect = nullptr, *results = nullptr;
    const uint32_t n_ids = kConns + 1;  // every connection and one id without a slot
    CHECK(hipMalloc(&arena, arena_bytes) == hipSuccess);
    CHECK(hipMalloc(&descs, kN * sizeof(cts_buf_desc)) == hipSuccess);
    CHECK(hipMalloc(&ctr, cts_counters_device_bytes()) == hipSuccess);
    CHECK(hipMalloc(&ref, cts_counters_device_bytes()) == hipSuccess);
    CHECK(hipMalloc(&blk, cts_counters_device_bytes()) == hipSuccess);
    CHECK(hipMalloc(&cff, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&state, kConns * sizeof(cts_conn_state)) == hipSuccess);
    CHECK(hipMalloc(&ids, n_ids * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&expect, n_ids * sizeof(uint64_t)) == hipSuccess);
    CHECK(hipMalloc(&results, n_ids * sizeof(cts_conn_result)) == hipSuccess);
    cts_buf_desc* dd = static_cast<cts_buf_desc*>(descs);
    uint32_t* slots = static_cast<uint32_t*>(cff);
    cts_conn_state* entries = static_cast<cts_conn_state*>(state);
    CHECK(hipMemcpyAsync(descs, d.data(), kN * sizeof(cts_buf_desc), hipMemcpyHostToDevice, s) == hipSuccess);
    CHECK(hipMemsetAsync(cff, 0xFF, kConns * sizeof(uint32_t), s) == hipSuccess);      // every slot empty
    CHECK(hipMemsetAsync(state, 0, kConns * sizeof(cts_conn_state), s) == hipSuccess);  // every connection fresh
    CHECK(cts_counters_reset(e, ctr, stream) == CTS_OK && cts_counters_reset(e, ref, stream) == CTS_OK &&
          cts_counters_reset(e, blk, stream) == CTS_OK);
    CHECK(cts_fill(e, arena, arena_bytes, dd, kN, 0, stream) == CTS_OK);

    // corrupt one byte of every 37th buffer from buffer 5 on: eight connections fail, at different buffers
    std::vector<uint8_t> bad(kN, 0);
    for (uint32_t i = 5; i < kN; i += 37) {
        uint8_t* b = static_cast<uint8_t*>(arena) + d[i].byte_offset + (i * 40503u) % d[i].length;
        uint8_t v = 0;
        CHECK(hipMemcpyAsync(&v, b, 1, hipMemcpyDeviceToHost, s) == hipSuccess);
        CHECK(hipStreamSynchronize(s) == hipSuccess);
        v ^= 0x5A;
        CHECK(hipMemcpyAsync(b, &v, 1, hipMemcpyHostToDevice, s) == hipSuccess);
        bad[i] = 1;
    }

    // what the device must hold: each connection stops at its first failing buffer
    const uint32_t base = 1000, delta = 700;  // ordinals 1000.., rebased by 700 before the close
    std::vector<cts_conn_state> want(kConns, cts_conn_state{0, 0, 0, 0});
    std::vector<uint32_t> want_first(kConns, kEmpty);
    std::vector<uint64_t> total(kConns, 0);
    cts_counters_ref want_ref{};
    uint64_t failed_conns = 0;
    for (uint32_t i = 0; i < kN; ++i) {
        const uint32_t c = d[i].conn_index, g = base + i;
        total[c] += d[i].length;
        if (g <= want_first[c]) {
            want[c].bytes_recv += d[i].length;
            want[c].buffers_recv += 1;
            want_ref.bytes_recv += d[i].length;
            want_ref.buffers_recv += 1;
            if (bad[i]) {
                want_first[c] = g;
                want_ref.buffers_failed += 1;
                ++failed_conns;
            } else {
                want_ref.bytes_ok += d[i].length;
            }
        } else {
            want[c].bytes_after_failure += d[i].length;
            want[c].buffers_after_failure += 1;
            want_ref.bytes_after_failure += d[i].length;
            want_ref.buffers_after_failure += 1;
        }
    }
    CHECK(failed_conns > 3 && failed_conns < kConns - 6);

    // per batch: verify, then the pass that keeps the node's and every connection's books (same stream)
    CHECK(cts_verify_at(e, arena, arena_bytes, dd, kN, 65536, base, nullptr, ctr, slots, kConns, stream) == CTS_OK);
    CHECK(cts_refview_accumulate_conns(e, arena_bytes, dd, kN, base, slots, kConns, ref, entries, stream) == CTS_OK);
    cts_counters_ref got_ref{};
    CHECK(cts_counters_read_ref(e, ref, &got_ref, stream) == CTS_OK);
    CHECK(std::memcmp(&got_ref, &want_ref, sizeof(want_ref)) == 0);
    std::vector<cts_conn_state> got_state(kConns);
    std::vector<uint32_t> got_first(kConns);
    CHECK(hipMemcpyAsync(got_state.data(), state, kConns * sizeof(cts_conn_state), hipMemcpyDeviceToHost, s) ==
          hipSuccess);
    CHECK(hipMemcpyAsync(got_first.data(), cff, kConns * sizeof(uint32_t), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    CHECK(std::memcmp(got_state.data(), want.data(), kConns * sizeof(cts_conn_state)) == 0);
    CHECK(got_first == want_first);

    // the ordinal space restarts low: every buffer below ordinal 700 is through, the next base_index drops by 700
    CHECK(cts_conn_slots_rebase(e, slots, kConns, delta, stream) == CTS_OK);
    for (uint32_t c = 0; c < kConns; ++c)
        if (want_first[c] != kEmpty) want_first[c] -= delta;
    uint32_t next_base = base + kN - delta;

    // close every connection (and one id that has no slot): sizes are the connections' totals, except that clean
    // connections 3k get one byte more than they sent and clean connections 3k + 1 one byte less
    std::vector<uint32_t> h_ids(n_ids);
    std::vector<uint64_t> h_expect(n_ids);
    cts_counters_close want_close{};
    std::vector<uint32_t> want_status(n_ids, 0);
    for (uint32_t i = 0; i < n_ids; ++i) {
        const uint32_t c = i < 10 ? i : i == 10 ? kConns + 5 : i - 1;  // the bad id in the middle of the list
        h_ids[i] = c;
        h_expect[i] = 0;
        if (c >= kConns) continue;
        h_expect[i] = total[c] + (c % 3 == 0 ? 1 : 0) - (c % 3 == 1 ? 1 : 0);
        want_close.connections_closed += 1;
        want_close.bytes_recv += want[c].bytes_recv;
        if (want_first[c] != kEmpty) {
            want_status[i] = CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN;
            want_close.data_errors += 1;
        } else if (want[c].bytes_recv > h_expect[i]) {
            want_status[i] = CTS_STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED;
            want_close.too_much_data += 1;
        } else if (want[c].bytes_recv < h_expect[i]) {
            want_status[i] = CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED;
            want_close.not_all_data += 1;
        } else {
            want_close.successful += 1;
        }
    }
    CHECK(want_close.successful > 0 && want_close.data_errors == failed_conns && want_close.not_all_data > 0 &&
          want_close.too_much_data > 0);
    CHECK(hipMemcpyAsync(ids, h_ids.data(), n_ids * sizeof(uint32_t), hipMemcpyHostToDevice, s) == hipSuccess);
    CHECK(hipMemcpyAsync(expect, h_expect.data(), n_ids * sizeof(uint64_t), hipMemcpyHostToDevice, s) == hipSuccess);
    CHECK(cts_conns_close(e, static_cast<uint32_t*>(ids), static_cast<uint64_t*>(expect), n_ids, slots, entries,
                          kConns, static_cast<cts_conn_result*>(results), blk, stream) == CTS_OK);
    std::vector<cts_conn_result> r(n_ids);
    CHECK(hipMemcpyAsync(r.data(), results, n_ids * sizeof(cts_conn_result), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipMemcpyAsync(got_state.data(), state, kConns * sizeof(cts_conn_state), hipMemcpyDeviceToHost, s) ==
          hipSuccess);
    CHECK(hipMemcpyAsync(got_first.data(), cff, kConns * sizeof(uint32_t), hipMemcpyDeviceToHost, s) == hipSuccess);
    cts_counters_close got_close{};
    CHECK(cts_counters_read_close(e, blk, &got_close, stream) == CTS_OK);  // synchronises the stream
    CHECK(std::memcmp(&got_close, &want_close, sizeof(want_close)) == 0);
    for (uint32_t i = 0; i < n_ids; ++i) {
        const uint32_t c = h_ids[i];
        CHECK(r[i].conn_index == c);
        if (c >= kConns) {
            CHECK(r[i].flags == CTS_CONN_RESULT_FLAG_BAD_CONN && r[i].status == 0 && r[i].first_fail == 0 &&
                  r[i].bytes_recv == 0 && r[i].buffers_recv == 0 && r[i].bytes_after_failure == 0 &&
                  r[i].buffers_after_failure == 0);
            continue;
        }
        CHECK(r[i].flags == 0 && r[i].status == want_status[i] && r[i].first_fail == want_first[c]);
        CHECK(r[i].bytes_recv == want[c].bytes_recv && r[i].buffers_recv == want[c].buffers_recv &&
              r[i].bytes_after_failure == want[c].bytes_after_failure &&
              r[i].buffers_after_failure == want[c].buffers_after_failure);
    }
    for (uint32_t c = 0; c < kConns; ++c) {
        CHECK(got_first[c] == kEmpty);
        CHECK(got_state[c].bytes_recv == 0 && got_state[c].buffers_recv == 0 &&
              got_state[c].bytes_after_failure == 0 && got_state[c].buffers_after_failure == 0);
    }

    // the next connections take the slots: the first half of every stream again (the fill repairs the arena first, so
    // only connection 2's new third buffer is corrupt), ordinals going on from the rebased count
    CHECK(cts_fill(e, arena, arena_bytes, dd, kN, 0, stream) == CTS_OK);
    std::vector<cts_buf_desc> d2;
    for (uint32_t c = 0; c < kConns; ++c)
        for (uint32_t k = 0; k < kPer / 2; ++k) d2.push_back(d[c * kPer + k]);
    const uint32_t n2 = (uint32_t)d2.size(), bad2 = 2 * (kPer / 2) + 2;
    {
        uint8_t* b = static_cast<uint8_t*>(arena) + d2[bad2].byte_offset + d2[bad2].length / 2;
        uint8_t v = 0;
        CHECK(hipMemcpyAsync(&v, b, 1, hipMemcpyDeviceToHost, s) == hipSuccess);
        CHECK(hipStreamSynchronize(s) == hipSuccess);
        v ^= 0xFF;
        CHECK(hipMemcpyAsync(b, &v, 1, hipMemcpyHostToDevice, s) == hipSuccess);
    }
    CHECK(hipMemcpyAsync(descs, d2.data(), n2 * sizeof(cts_buf_desc), hipMemcpyHostToDevice, s) == hipSuccess);
    CHECK(cts_verify_at(e, arena, arena_bytes, dd, n2, 65536, next_base, nullptr, ctr, slots, kConns, stream) == CTS_OK);
    CHECK(cts_refview_accumulate_conns(e, arena_bytes, dd, n2, next_base, slots, kConns, ref, entries, stream) ==
          CTS_OK);
    // close connections 0..3 with no sizes (a UDP-style close: only data errors are judged)
    const uint32_t n_close2 = 4;
    CHECK(cts_conns_close(e, static_cast<uint32_t*>(ids), nullptr, n_close2, slots, entries, kConns,
                          static_cast<cts_conn_result*>(results), blk, stream) == CTS_OK);
    CHECK(hipMemcpyAsync(r.data(), results, n_close2 * sizeof(cts_conn_result), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipMemcpyAsync(got_state.data(), state, kConns * sizeof(cts_conn_state), hipMemcpyDeviceToHost, s) ==
          hipSuccess);
    CHECK(hipMemcpyAsync(got_first.data(), cff, kConns * sizeof(uint32_t), hipMemcpyDeviceToHost, s) == hipSuccess);
    cts_counters_close after{};
    CHECK(cts_counters_read_close(e, blk, &after, stream) == CTS_OK);
    uint64_t bytes2 = 0;
    for (uint32_t c = 0; c < n_close2; ++c) {
        uint64_t recv = 0, later = 0, nrecv = 0, nlater = 0;
        for (uint32_t k = 0; k < kPer / 2; ++k) {
            const uint32_t i = c * (kPer / 2) + k;
            const bool received = c != 2 || i <= bad2;
            (received ? recv : later) += d2[i].length;
            (received ? nrecv : nlater) += 1;
        }
        bytes2 += recv;
        CHECK(r[c].conn_index == c && r[c].flags == 0);
        CHECK(r[c].first_fail == (c == 2 ? next_base + bad2 : kEmpty));
        CHECK(r[c].status == (c == 2 ? CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN : 0u));
        CHECK(r[c].bytes_recv == recv && r[c].buffers_recv == nrecv && r[c].bytes_after_failure == later &&
              r[c].buffers_after_failure == nlater);
        CHECK(got_first[c] == kEmpty && got_state[c].buffers_recv == 0);
    }
    for (uint32_t c = n_close2; c < kConns; ++c)  // still open: their entries hold the second connections' buffers
        CHECK(got_first[c] == kEmpty && got_state[c].buffers_recv == kPer / 2 && got_state[c].buffers_after_failure == 0);
    CHECK(after.connections_closed == want_close.connections_closed + n_close2);
    CHECK(after.successful == want_close.successful + 3 && after.data_errors == want_close.data_errors + 1);
    CHECK(after.not_all_data == want_close.not_all_data && after.too_much_data == want_close.too_much_data);
    CHECK(after.bytes_recv == want_close.bytes_recv + bytes2);
    // the DataError count of the verifies: the first generation's failed connections and the one recycled slot
    cts_counters_ex cx{};
    CHECK(cts_counters_read_ex(e, ctr, &cx, stream) == CTS_OK);
    CHECK(cx.connections_failed == failed_conns + 1);
    // the same close block through the node-wide host fold
    cts_engine* const engines[1] = {e};
    const void* const blocks[1] = {blk};
    void* const streams[1] = {stream};
    cts_counters_close folded{};
    CHECK(cts_counters_read_multi_close(engines, blocks, streams, 1, &folded) == CTS_OK);
    CHECK(std::memcmp(&folded, &after, sizeof(after)) == 0);

    CHECK(hipFree(arena) == hipSuccess && hipFree(descs) == hipSuccess && hipFree(ctr) == hipSuccess);
    CHECK(hipFree(ref) == hipSuccess && hipFree(blk) == hipSuccess && hipFree(cff) == hipSuccess);
    CHECK(hipFree(state) == hipSuccess && hipFree(ids) == hipSuccess && hipFree(expect) == hipSuccess);
    CHECK(hipFree(results) == hipSuccess);
    CHECK(cts_engine_stream_destroy(e, stream) == CTS_OK);
    CHECK(cts_engine_destroy(e) == CTS_OK);
    std::printf("device_connections: ok (%u buffers, %llu connections closed, %llu data errors, %llu short, %llu long)\n",
                kN, (unsigned long long)after.connections_closed, (unsigned long long)after.data_errors,
                (unsigned long long)after.not_all_data, (unsigned long long)after.too_much_data);
    return 0;
}
