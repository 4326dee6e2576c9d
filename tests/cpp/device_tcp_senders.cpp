// device_tcp_senders.cpp — a whole TCP exchange on the device from C++, through the C ABI only
// (include/cts_tcp_senders.h; INTEGRATION.md "TCP senders on the device-resident path"): senders from
// cts_tcp_sender_init, and per tick cts_tcp_senders_send -> cts_verify_at -> cts_refview_accumulate_conns over the
// descriptors the senders wrote, with the receive pass's n computed from the settings and nothing read back inside the
// loop; then cts_conns_close against the transfer sizes. One tick's arena is also written by cts_fill from host-built
// descriptors and compared byte for byte. Built by `make` (ctstraffic_amd/build/device_tcp_senders) and run by
// tests/test_cpp_tcp_senders.py on the GPU box. Exits non-zero on a failed check.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
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
constexpr uint32_t kConns = 6, kStride = 65536, kMaxBuffers = 3, kCapacity = 11;
struct Setting {
    uint64_t transfer;
    uint32_t buffer;
};
// multiples and non-multiples of the buffer size, odd sizes, one byte, one connection longer than the others
const Setting kSettings[kConns] = {{5 * 65536, 65536}, {200000, 65531}, {1, 1024}, {7 * 8193 + 5, 8193},
                                   {12 * 9000ull, 9000},  {33 * 20 + 1, 33}};
}  // namespace

int main()
{
    cts_engine* e = nullptr;
    CHECK(cts_engine_create(0, &e) == CTS_OK);
    void* stream = nullptr;
    CHECK(cts_engine_stream_create(e, &stream) == CTS_OK);
    hipStream_t s = static_cast<hipStream_t>(stream);

    std::vector<cts_tcp_sender_state> senders(kConns);
    std::vector<uint64_t> expected(kConns);
    for (uint32_t c = 0; c < kConns; ++c) {
        CHECK(cts_tcp_sender_init(kSettings[c].transfer, kSettings[c].buffer, &senders[c]) == CTS_OK);
        CHECK(senders[c].bytes_sent == 0 && senders[c].finished == 0 && senders[c].transfer_bytes == kSettings[c].transfer);
    }
    cts_tcp_sender_state refused{};
    CHECK(cts_tcp_sender_init(0, 1024, &refused) == CTS_E_INVALID && cts_tcp_sender_init(1024, 0, &refused) == CTS_E_INVALID &&
          cts_tcp_sender_init(1024, 1024, nullptr) == CTS_E_INVALID);

    const uint64_t arena_bytes = (uint64_t)kCapacity * kStride;
    const size_t scratch_bytes = cts_tcp_senders_scratch_bytes(kConns);
    void *arena = nullptr, *arena2 = nullptr, *descs = nullptr, *descs2 = nullptr, *sent = nullptr, *verify = nullptr,
         *ref = nullptr, *closes = nullptr, *cff = nullptr, *dsenders = nullptr, *state = nullptr, *ids = nullptr,
         *codes = nullptr, *tick = nullptr, *scratch = nullptr, *results = nullptr, *dexpected = nullptr;
    CHECK(hipMalloc(&arena, arena_bytes) == hipSuccess && hipMalloc(&arena2, arena_bytes) == hipSuccess);
    CHECK(hipMalloc(&descs, kCapacity * sizeof(cts_buf_desc)) == hipSuccess);
    CHECK(hipMalloc(&descs2, kCapacity * sizeof(cts_buf_desc)) == hipSuccess);
    for (void** p : {&sent, &verify, &ref, &closes}) CHECK(hipMalloc(p, cts_counters_device_bytes()) == hipSuccess);
    CHECK(hipMalloc(&cff, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&dsenders, kConns * sizeof(cts_tcp_sender_state)) == hipSuccess);
    CHECK(hipMalloc(&state, kConns * sizeof(cts_conn_state)) == hipSuccess);
    CHECK(hipMalloc(&ids, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&codes, kConns * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&tick, sizeof(cts_tcp_sender_tick)) == hipSuccess);
    CHECK(hipMalloc(&scratch, scratch_bytes) == hipSuccess);
    CHECK(hipMalloc(&results, kConns * sizeof(cts_conn_result)) == hipSuccess);
    CHECK(hipMalloc(&dexpected, kConns * sizeof(uint64_t)) == hipSuccess);
    CHECK(hipMemsetAsync(arena, 0xA5, arena_bytes, s) == hipSuccess);
    CHECK(hipMemsetAsync(arena2, 0xA5, arena_bytes, s) == hipSuccess);
    CHECK(hipMemsetAsync(cff, 0xFF, kConns * sizeof(uint32_t), s) == hipSuccess);  // every slot empty
    CHECK(hipMemsetAsync(state, 0, kConns * sizeof(cts_conn_state), s) == hipSuccess);
    CHECK(hipMemcpyAsync(dsenders, senders.data(), kConns * sizeof(cts_tcp_sender_state), hipMemcpyHostToDevice, s) ==
          hipSuccess);
    for (void* p : {sent, verify, ref, closes}) CHECK(cts_counters_reset(e, p, stream) == CTS_OK);
    const uint32_t order[kConns] = {3, 0, 5, 1, 4, 2};  // the listed order is the slots' order
    for (uint32_t i = 0; i < kConns; ++i) expected[i] = kSettings[order[i]].transfer;
    CHECK(hipMemcpyAsync(ids, order, sizeof(order), hipMemcpyHostToDevice, s) == hipSuccess);
    CHECK(hipMemcpyAsync(dexpected, expected.data(), kConns * sizeof(uint64_t), hipMemcpyHostToDevice, s) == hipSuccess);

    cts_buf_desc* dd = static_cast<cts_buf_desc*>(descs);
    uint32_t* dids = static_cast<uint32_t*>(ids);
    cts_tcp_sender_state* sv = static_cast<cts_tcp_sender_state*>(dsenders);
    cts_tcp_sender_tick* dtick = static_cast<cts_tcp_sender_tick*>(tick);
    uint32_t* dcodes = static_cast<uint32_t*>(codes);

    // a refused argument launches nothing
    CHECK(cts_tcp_senders_send(e, arena, arena_bytes, kStride + 8, 0, kCapacity, dids, kConns, kMaxBuffers, sv, kConns, dd,
                               dcodes, dtick, sent, scratch, scratch_bytes, stream) == CTS_E_INVALID);
    CHECK(cts_tcp_senders_send(e, arena, arena_bytes, kStride, 1, kCapacity, dids, kConns, kMaxBuffers, sv, kConns, dd,
                               dcodes, dtick, sent, scratch, scratch_bytes, stream) == CTS_E_INVALID);
    CHECK(cts_tcp_senders_send(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, 0, sv, kConns, dd, dcodes,
                               dtick, sent, scratch, scratch_bytes, stream) == CTS_E_INVALID);
    CHECK(cts_tcp_senders_send(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, kMaxBuffers, sv, kConns,
                               nullptr, dcodes, dtick, sent, scratch, scratch_bytes, stream) == CTS_E_INVALID);

    // ---- the exchange: the host keeps the books of the settings only; nothing is read back inside the loop ----
    std::vector<uint64_t> done(kConns, 0);  // bytes each connection has sent, by the settings' arithmetic
    uint32_t ordinal = 0, ticks = 0;
    uint64_t total_bytes = 0, total_buffers = 0;
    for (;; ++ticks) {
        // this tick's buffers, from the settings: w per running connection in listed order, cut at the capacity
        std::vector<cts_buf_desc> host;
        for (uint32_t i = 0; i < kConns && host.size() < kCapacity; ++i) {
            const uint32_t c = order[i];
            const uint64_t B = kSettings[c].buffer, left = kSettings[c].transfer - done[c];
            const uint64_t w = std::min<uint64_t>(kMaxBuffers, (left + B - 1) / B);
            for (uint64_t j = 0; j < w && host.size() < kCapacity; ++j) {
                const uint64_t len = std::min(B, kSettings[c].transfer - done[c]);
                host.push_back(cts_buf_desc{host.size() * (uint64_t)kStride, (uint32_t)len, (uint32_t)(done[c] % 65536), c, 0});
                done[c] += len;
                total_bytes += len;
            }
        }
        const uint32_t n = (uint32_t)host.size();
        if (n == 0) break;
        total_buffers += n;
        if (ticks < 2) CHECK(hipMemsetAsync(arena, 0xA5, arena_bytes, s) == hipSuccess);  // compared whole below
        CHECK(cts_tcp_senders_send(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, kMaxBuffers, sv, kConns, dd,
                                   dcodes, dtick, sent, scratch, scratch_bytes, stream) == CTS_OK);
        if (ticks < 2) {
            // the same tick through the host-fed fill: descriptors built here, one by one
            CHECK(hipMemsetAsync(arena2, 0xA5, arena_bytes, s) == hipSuccess);
            CHECK(hipMemcpyAsync(descs2, host.data(), n * sizeof(cts_buf_desc), hipMemcpyHostToDevice, s) == hipSuccess);
            CHECK(cts_fill(e, arena2, arena_bytes, static_cast<cts_buf_desc*>(descs2), n, kStride, stream) == CTS_OK);
            std::vector<uint8_t> a(arena_bytes), b(arena_bytes);
            std::vector<cts_buf_desc> got(n);
            CHECK(hipMemcpyAsync(a.data(), arena, arena_bytes, hipMemcpyDeviceToHost, s) == hipSuccess);
            CHECK(hipMemcpyAsync(b.data(), arena2, arena_bytes, hipMemcpyDeviceToHost, s) == hipSuccess);
            CHECK(hipMemcpyAsync(got.data(), descs, n * sizeof(cts_buf_desc), hipMemcpyDeviceToHost, s) == hipSuccess);
            CHECK(hipStreamSynchronize(s) == hipSuccess);
            CHECK(ticks != 0 || n == kCapacity);  // the first tick fills the capacity and cuts a burst
            CHECK(a == b);
            CHECK(std::memcmp(got.data(), host.data(), n * sizeof(cts_buf_desc)) == 0);
        }
        CHECK(cts_verify_at(e, arena, arena_bytes, dd, n, kStride, ordinal, nullptr, verify, static_cast<uint32_t*>(cff),
                            kConns, stream) == CTS_OK);
        CHECK(cts_refview_accumulate_conns(e, arena_bytes, dd, n, ordinal, static_cast<uint32_t*>(cff), kConns, ref,
                                           static_cast<cts_conn_state*>(state), stream) == CTS_OK);
        ordinal += n;
        CHECK(ticks < 100);
    }
    // one tick more: every sender has finished and sends nothing
    CHECK(cts_tcp_senders_send(e, arena, arena_bytes, kStride, 0, kCapacity, dids, kConns, kMaxBuffers, sv, kConns, dd,
                               dcodes, dtick, sent, scratch, scratch_bytes, stream) == CTS_OK);
    CHECK(cts_conns_close(e, dids, static_cast<uint64_t*>(dexpected), kConns, static_cast<uint32_t*>(cff),
                          static_cast<cts_conn_state*>(state), kConns, static_cast<cts_conn_result*>(results), closes,
                          stream) == CTS_OK);

    std::vector<cts_conn_result> r(kConns);
    std::vector<uint32_t> got_codes(kConns);
    cts_tcp_sender_tick last{};
    CHECK(hipMemcpyAsync(r.data(), results, kConns * sizeof(cts_conn_result), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipMemcpyAsync(senders.data(), dsenders, kConns * sizeof(cts_tcp_sender_state), hipMemcpyDeviceToHost, s) ==
          hipSuccess);
    CHECK(hipMemcpyAsync(got_codes.data(), codes, kConns * sizeof(uint32_t), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipMemcpyAsync(&last, tick, sizeof(last), hipMemcpyDeviceToHost, s) == hipSuccess);
    cts_counters_sent from_senders{};
    cts_counters_close closed{};
    cts_counters_ref seen{};
    cts_counters clean{};
    CHECK(cts_counters_read_sent(e, sent, &from_senders, stream) == CTS_OK);
    CHECK(cts_counters_read_close(e, closes, &closed, stream) == CTS_OK);
    CHECK(cts_counters_read_ref(e, ref, &seen, stream) == CTS_OK);
    CHECK(cts_counters_read(e, verify, &clean, stream) == CTS_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    uint64_t transfers = 0;
    for (uint32_t i = 0; i < kConns; ++i) {
        const uint32_t c = order[i];
        const Setting& cfg = kSettings[c];
        CHECK(r[i].conn_index == c && r[i].status == 0 && r[i].flags == 0 && r[i].first_fail == 0xFFFFFFFFu);
        CHECK(r[i].bytes_recv == cfg.transfer && r[i].buffers_recv == (cfg.transfer + cfg.buffer - 1) / cfg.buffer);
        CHECK(r[i].bytes_after_failure == 0 && r[i].buffers_after_failure == 0);
        CHECK(senders[c].finished == 1 && senders[c].bytes_sent == cfg.transfer && senders[c].buffers_sent == r[i].buffers_recv);
        CHECK(got_codes[i] == CTS_TCP_SENDER_ENDED);
        transfers += cfg.transfer;
    }
    CHECK(ticks > 4 && total_bytes == transfers && ordinal == total_buffers);
    CHECK(last.buffers == 0 && last.bytes == 0 && last.connections_sent == 0 && last.connections_skipped == kConns);
    CHECK(from_senders.bytes_sent == transfers && from_senders.buffers_sent == total_buffers &&
          from_senders.connections_finished == kConns);
    CHECK(closed.connections_closed == kConns && closed.successful == kConns && closed.bytes_recv == transfers);
    CHECK(seen.bytes_recv == transfers && seen.buffers_recv == total_buffers && seen.buffers_failed == 0);
    CHECK(clean.bytes_checked == transfers && clean.bytes_ok == transfers && clean.buffers_failed == 0 &&
          clean.buffers_checked == total_buffers);

    for (void* p : {arena, arena2, descs, descs2, sent, verify, ref, closes, cff, dsenders, state, ids, codes, tick, scratch,
                    results, dexpected})
        CHECK(hipFree(p) == hipSuccess);
    CHECK(cts_engine_stream_destroy(e, stream) == CTS_OK);
    CHECK(cts_engine_destroy(e) == CTS_OK);
    std::printf("device_tcp_senders: ok\n");
    return 0;
}
