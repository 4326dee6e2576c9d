// device_tcp_paced_senders.cpp — a paced TCP exchange on the device from C++, through the C ABI only
// (include/cts_tcp_senders.h; INTEGRATION.md "Send pacing on the device-resident path"): senders from
// cts_tcp_sender_init, their pace entries from cts_tcp_sender_pace_init, and per tick cts_tcp_senders_send_paced ->
// cts_verify_at -> cts_refview_accumulate_conns over the descriptors the senders wrote. Every tick lists every
// connection; the host keeps no pacing state: it reads the 48-byte tick block, takes the receive pass's n from it and
// moves its (simulated) clock to next_due_ms. Then cts_conns_close against the transfer sizes. Built by `make`
// (ctstraffic_amd/build/device_tcp_paced_senders) and run by tests/test_cpp_tcp_paced_senders.py on the GPU box. Exits
// non-zero on a failed check.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "cts_tcp_senders.h"

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) {                                                                     \
            std::fprintf(stderr, "%s:%d CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

namespace {
constexpr uint32_t kConns = 6, kStride = 9008, kMaxBuffers = 4, kCapacity = kConns * kMaxBuffers;
constexpr int64_t kStart = 10000;
struct Setting {
    uint64_t transfer;
    uint32_t buffer;
    uint64_t bytes_per_second;  // -RateLimit
    uint32_t period_ms;         // TcpBytesPerSecondPeriod, 0 = 100
    uint32_t burst_count, burst_delay_ms;
};
// unpaced; one buffer per 100 ms quantum; 2.5 buffers per 10 ms quantum; bursts of 3 every 50 ms; a rate that rounds
// to nothing over a burst setting; a rate over a burst setting (the rate wins)
const Setting kSettings[kConns] = {{20 * 9000ull, 9000, 0, 0, 0, 0},          {10 * 9000ull + 1, 9000, 90000, 0, 0, 0},
                                   {28 * 1000ull, 1000, 250000, 10, 0, 0},    {9 * 8193ull + 5, 8193, 0, 0, 3, 50},
                                   {7 * 33ull, 33, 999, 1, 2, 7},             {12 * 1000ull, 1000, 400000, 10, 1, 500}};
}  // namespace

int main()
{
    cts_engine* e = nullptr;
    CHECK(cts_engine_create(0, &e) == CTS_OK);
    void* stream = nullptr;
    CHECK(cts_engine_stream_create(e, &stream) == CTS_OK);
    hipStream_t s = static_cast<hipStream_t>(stream);

    std::vector<cts_tcp_sender_state> senders(kConns);
    std::vector<cts_tcp_sender_pace> pace(kConns);
    std::vector<uint64_t> expected(kConns);
    std::vector<uint32_t> order(kConns);
    for (uint32_t c = 0; c < kConns; ++c) {
        const Setting& cfg = kSettings[c];
        CHECK(cts_tcp_sender_init(cfg.transfer, cfg.buffer, &senders[c]) == CTS_OK);
        CHECK(cts_tcp_sender_pace_init(cfg.bytes_per_second, cfg.period_ms, cfg.burst_count, cfg.burst_delay_ms, kStart,
                                       &pace[c]) == CTS_OK);
        CHECK(pace[c].quantum_start_ms == kStart && pace[c].pending == 0 && pace[c].burst_left == cfg.burst_count);
        CHECK(pace[c].quantum_period_ms == (cfg.period_ms ? cfg.period_ms : 100u));
        order[c] = c;
        expected[c] = cfg.transfer;
    }
    CHECK(pace[1].bytes_per_quantum == 9000 && pace[2].bytes_per_quantum == 2500 && pace[4].bytes_per_quantum == 0);
    cts_tcp_sender_pace refused{};
    CHECK(cts_tcp_sender_pace_init(1, 1, 0, 0, -1, &refused) == CTS_E_INVALID &&
          cts_tcp_sender_pace_init(1, 1, 0, 0, 0, nullptr) == CTS_E_INVALID &&
          cts_tcp_sender_pace_init(UINT64_MAX, 1000, 0, 0, 0, &refused) == CTS_E_INVALID);

    const uint64_t arena_bytes = (uint64_t)kCapacity * kStride;
    const size_t scratch_bytes = cts_tcp_senders_paced_scratch_bytes(kConns);
    CHECK(scratch_bytes > cts_tcp_senders_scratch_bytes(kConns));
    void *arena = nullptr, *descs = nullptr, *sent = nullptr, *verify = nullptr, *ref = nullptr, *closes = nullptr,
         *cff = nullptr, *dsenders = nullptr, *dpace = nullptr, *state = nullptr, *ids = nullptr, *codes = nullptr,
         *tick = nullptr, *scratch = nullptr, *results = nullptr, *dexpected = nullptr;
    CHECK(hipMalloc(&arena, arena_bytes) == hipSuccess);
    CHECK(hipMalloc(&descs, kCapacity * sizeof(cts_buf_desc)) == hipSuccess);
    for (void** p : {&sent, &verify, &ref, &closes}) CHECK(hipMalloc(p, cts_counters_device_bytes()) == hipSuccess);
    CHECK(hipMalloc(&cff, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&dsenders, kConns * sizeof(cts_tcp_sender_state)) == hipSuccess);
    CHECK(hipMalloc(&dpace, kConns * sizeof(cts_tcp_sender_pace)) == hipSuccess);
    CHECK(hipMalloc(&state, kConns * sizeof(cts_conn_state)) == hipSuccess);
    CHECK(hipMalloc(&ids, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&codes, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&tick, sizeof(cts_tcp_sender_paced_tick)) == hipSuccess);
    CHECK(hipMalloc(&scratch, scratch_bytes) == hipSuccess);
    CHECK(hipMalloc(&results, kConns * sizeof(cts_conn_result)) == hipSuccess);
    CHECK(hipMalloc(&dexpected, kConns * sizeof(uint64_t)) == hipSuccess);
    CHECK(hipMemsetAsync(arena, 0xA5, arena_bytes, s) == hipSuccess);
    CHECK(hipMemsetAsync(cff, 0xFF, kConns * sizeof(uint32_t), s) == hipSuccess);  // every slot empty
    CHECK(hipMemsetAsync(state, 0, kConns * sizeof(cts_conn_state), s) == hipSuccess);
    CHECK(hipMemcpyAsync(dsenders, senders.data(), kConns * sizeof(cts_tcp_sender_state), hipMemcpyHostToDevice, s) ==
          hipSuccess);
    CHECK(hipMemcpyAsync(dpace, pace.data(), kConns * sizeof(cts_tcp_sender_pace), hipMemcpyHostToDevice, s) == hipSuccess);
    for (void* p : {sent, verify, ref, closes}) CHECK(cts_counters_reset(e, p, stream) == CTS_OK);
    CHECK(hipMemcpyAsync(ids, order.data(), kConns * sizeof(uint32_t), hipMemcpyHostToDevice, s) == hipSuccess);
    CHECK(hipMemcpyAsync(dexpected, expected.data(), kConns * sizeof(uint64_t), hipMemcpyHostToDevice, s) == hipSuccess);

    cts_buf_desc* dd = static_cast<cts_buf_desc*>(descs);
    uint32_t* dids = static_cast<uint32_t*>(ids);
    cts_tcp_sender_state* sv = static_cast<cts_tcp_sender_state*>(dsenders);
    cts_tcp_sender_pace* pv = static_cast<cts_tcp_sender_pace*>(dpace);
    cts_tcp_sender_paced_tick* dtick = static_cast<cts_tcp_sender_paced_tick*>(tick);
    uint32_t* dcodes = static_cast<uint32_t*>(codes);

    // a refused argument launches nothing
    CHECK(cts_tcp_senders_send_paced(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, kMaxBuffers, sv, nullptr,
                                     kConns, kStart, dd, dcodes, dtick, sent, scratch, scratch_bytes,
                                     stream) == CTS_E_INVALID);
    CHECK(cts_tcp_senders_send_paced(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, kMaxBuffers, sv, pv,
                                     kConns, -1, dd, dcodes, dtick, sent, scratch, scratch_bytes,
                                     stream) == CTS_E_INVALID);
    CHECK(cts_tcp_senders_send_paced(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, kMaxBuffers, sv, pv,
                                     kConns, kStart, dd, dcodes, dtick, sent, scratch,
                                     cts_tcp_senders_scratch_bytes(kConns), stream) == CTS_E_INVALID);

    // ---- the exchange: the tick block is all the host reads ----
    int64_t now = kStart;
    uint32_t ordinal = 0, ticks = 0, idle_ticks = 0, finished = 0;
    uint64_t total_bytes = 0;
    std::vector<int64_t> last_sent_ms(kConns, -1);
    while (finished < kConns) {
        CHECK(cts_tcp_senders_send_paced(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, kMaxBuffers, sv, pv,
                                         kConns, now, dd, dcodes, dtick, sent, scratch, scratch_bytes,
                                         stream) == CTS_OK);
        cts_tcp_sender_paced_tick t{};
        std::vector<uint32_t> got_codes(kConns);
        CHECK(hipMemcpyAsync(&t, tick, sizeof(t), hipMemcpyDeviceToHost, s) == hipSuccess);
        CHECK(hipMemcpyAsync(got_codes.data(), codes, kConns * sizeof(uint32_t), hipMemcpyDeviceToHost, s) == hipSuccess);
        CHECK(hipStreamSynchronize(s) == hipSuccess);
        const uint32_t n = t.tick.buffers;
        CHECK(n <= kCapacity && t.tick.connections_no_room == 0 && t.tick.reserved == 0);
        CHECK(t.connections_waiting + t.tick.connections_sent + t.tick.connections_skipped == kConns);
        CHECK((t.connections_pending == 0) == (t.next_due_ms == INT64_MAX));
        for (uint32_t c = 0; c < kConns; ++c)
            if (got_codes[c] == CTS_TCP_SENDER_SENT || got_codes[c] == CTS_TCP_SENDER_FINISHED) last_sent_ms[c] = now;
        if (n != 0) {
            CHECK(cts_verify_at(e, arena, arena_bytes, dd, n, kStride, ordinal, nullptr, verify,
                                static_cast<uint32_t*>(cff), kConns, stream) == CTS_OK);
            CHECK(cts_refview_accumulate_conns(e, arena_bytes, dd, n, ordinal, static_cast<uint32_t*>(cff), kConns, ref,
                                               static_cast<cts_conn_state*>(state), stream) == CTS_OK);
        } else {
            ++idle_ticks;
        }
        ordinal += n;
        total_bytes += t.tick.bytes;
        finished += t.tick.connections_finished;
        // the one host timer: nothing went out, so sleep until the next deferred send is due
        if (t.tick.connections_sent == 0 && finished < kConns) {
            CHECK(t.next_due_ms != INT64_MAX && t.next_due_ms > now);
            now = t.next_due_ms;
        }
        CHECK(++ticks < 1000);
    }
    CHECK(cts_conns_close(e, dids, static_cast<uint64_t*>(dexpected), kConns, static_cast<uint32_t*>(cff),
                          static_cast<cts_conn_state*>(state), kConns, static_cast<cts_conn_result*>(results), closes,
                          stream) == CTS_OK);

    std::vector<cts_conn_result> r(kConns);
    CHECK(hipMemcpyAsync(r.data(), results, kConns * sizeof(cts_conn_result), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipMemcpyAsync(senders.data(), dsenders, kConns * sizeof(cts_tcp_sender_state), hipMemcpyDeviceToHost, s) ==
          hipSuccess);
    CHECK(hipMemcpyAsync(pace.data(), dpace, kConns * sizeof(cts_tcp_sender_pace), hipMemcpyDeviceToHost, s) == hipSuccess);
    cts_counters_sent from_senders{};
    cts_counters_close closed{};
    cts_counters clean{};
    CHECK(cts_counters_read_sent(e, sent, &from_senders, stream) == CTS_OK);
    CHECK(cts_counters_read_close(e, closes, &closed, stream) == CTS_OK);
    CHECK(cts_counters_read(e, verify, &clean, stream) == CTS_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    uint64_t transfers = 0, buffers = 0;
    for (uint32_t c = 0; c < kConns; ++c) {
        const Setting& cfg = kSettings[c];
        CHECK(r[c].conn_index == c && r[c].status == 0 && r[c].flags == 0 && r[c].first_fail == 0xFFFFFFFFu);
        CHECK(r[c].bytes_recv == cfg.transfer && r[c].buffers_recv == (cfg.transfer + cfg.buffer - 1) / cfg.buffer);
        CHECK(senders[c].finished == 1 && senders[c].bytes_sent == cfg.transfer && pace[c].pending == 0);
        transfers += cfg.transfer;
        buffers += r[c].buffers_recv;
    }
    // the clock the pacing imposed: the unpaced connection ends at the start; one buffer per 100 ms puts the 11th
    // buffer 1 000 ms later; 28 buffers at 2.5 per 10 ms end in the 11th quantum; 10 buffers in bursts of 3 every
    // 50 ms end after the third delay; 7 buffers in bursts of 2 every 7 ms after the third; the rate of 4 buffers per
    // 10 ms quantum, not the burst delay of 500 ms, paces the last
    CHECK(last_sent_ms[0] == kStart && last_sent_ms[1] == kStart + 1000 && last_sent_ms[2] == kStart + 100);
    CHECK(last_sent_ms[3] == kStart + 150 && last_sent_ms[4] == kStart + 21 && last_sent_ms[5] == kStart + 20);
    CHECK(idle_ticks > 0 && total_bytes == transfers && ordinal == buffers);
    CHECK(from_senders.bytes_sent == transfers && from_senders.buffers_sent == buffers &&
          from_senders.connections_finished == kConns);
    CHECK(closed.connections_closed == kConns && closed.successful == kConns && closed.bytes_recv == transfers);
    CHECK(clean.bytes_checked == transfers && clean.bytes_ok == transfers && clean.buffers_failed == 0 &&
          clean.buffers_checked == buffers);

    for (void* p : {arena, descs, sent, verify, ref, closes, cff, dsenders, dpace, state, ids, codes, tick, scratch, results,
                    dexpected})
        CHECK(hipFree(p) == hipSuccess);
    CHECK(cts_engine_stream_destroy(e, stream) == CTS_OK);
    CHECK(cts_engine_destroy(e) == CTS_OK);
    std::printf("device_tcp_paced_senders: ok\n");
    return 0;
}
