// device_tcp_exchange.cpp — one PushPull exchange on the device from C++, through the C ABI only
// (include/cts_tcp_exchange.h; INTEGRATION.md "Pull, PushPull and Duplex on the device-resident path"): an entry from
// cts_tcp_exchange_init, and per tick cts_tcp_exchange_send -> cts_verify_at -> cts_refview_accumulate_conns over the
// descriptors the tick wrote, with the receive pass's n computed from the settings and nothing read back inside the
// loop; then cts_conns_close of both receivers (the server, slot c, and the client, slot c + n_conns) against
// cts_tcp_exchange_direction_bytes. The host walks the pattern one buffer at a time beside it, as the reference's
// GetNextTaskFromPattern / CompleteTaskBackToPattern do, and the first ticks' descriptors are compared with that walk
// one by one. Built by `make` (ctstraffic_amd/build/device_tcp_exchange) and run by tests/test_cpp_tcp_exchange.py on
// the GPU box. Exits non-zero on a failed check.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cts_tcp_exchange.h"

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) {                                                                     \
            std::fprintf(stderr, "%s:%d CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

namespace {
// one connection (slot 1 of a table of 2: slot 0 stays a finished Push entry), -PushBytes and -PullBytes no multiples
// of the buffer size, the transfer ending inside the fourth pull segment
constexpr uint32_t kConns = 2, kConn = 1, kReceivers = 2 * kConns, kStride = 65536, kMaxBuffers = 3, kCapacity = 3;
constexpr uint32_t kBuffer = 65531, kPush = 200000, kPull = 70001;
constexpr uint64_t kTransfer = 3ull * (kPush + kPull) + kPush + 1234;

// The pattern, one buffer at a time (ctsIOPattern.cpp:920-992 from the client's side).
struct Walk {
    bool sending = true;
    uint32_t intra = 0;
    uint64_t left = kTransfer, sent[2] = {0, 0};
    bool next(cts_buf_desc* d, uint64_t slot)
    {
        if (left == 0) return false;
        const uint32_t segment = sending ? kPush : kPull, dir = sending ? 0u : 1u;
        const uint32_t len = (uint32_t)std::min<uint64_t>({kBuffer, left, segment - intra});
        *d = cts_buf_desc{slot * kStride, len, (uint32_t)(sent[dir] % 65536), kConn + dir * kConns, 0};
        sent[dir] += len;
        left -= len;
        intra += len;
        if (intra == segment) {
            sending = !sending;
            intra = 0;
        }
        return true;
    }
};
}  // namespace

int main()
{
    cts_engine* e = nullptr;
    CHECK(cts_engine_create(0, &e) == CTS_OK);
    void* stream = nullptr;
    CHECK(cts_engine_stream_create(e, &stream) == CTS_OK);
    hipStream_t s = static_cast<hipStream_t>(stream);

    std::vector<cts_tcp_exchange_state> entries(kConns);
    CHECK(cts_tcp_exchange_init(CTS_TCP_EXCHANGE_PUSH, 1000, 1000, 0, 0, &entries[0]) == CTS_OK);
    CHECK(cts_tcp_exchange_seek(&entries[0], 1) == CTS_OK && entries[0].finished == 1);
    CHECK(cts_tcp_exchange_init(CTS_TCP_EXCHANGE_PUSHPULL, kTransfer, kBuffer, kPush, kPull, &entries[kConn]) == CTS_OK);
    const cts_tcp_exchange_state fresh = entries[kConn];
    CHECK(fresh.total_buffers == 3 * (4 + 2) + 4 + 1 && fresh.buffers_sent == 0 && fresh.finished == 0);
    cts_tcp_exchange_state refused{};
    CHECK(cts_tcp_exchange_init(CTS_TCP_EXCHANGE_PUSHPULL, 1, 1, 0, 1, &refused) == CTS_E_INVALID &&
          cts_tcp_exchange_init(4, 1, 1, 1, 1, &refused) == CTS_E_INVALID &&
          cts_tcp_exchange_init(CTS_TCP_EXCHANGE_PULL, 1, 1, 0, 0, nullptr) == CTS_E_INVALID);
    const uint64_t expected[kReceivers] = {1000, cts_tcp_exchange_direction_bytes(&fresh, 0), 0,
                                           cts_tcp_exchange_direction_bytes(&fresh, 1)};
    CHECK(expected[1] == 4ull * kPush && expected[3] == 3ull * kPull + 1234 && expected[1] + expected[3] == kTransfer);

    const uint64_t arena_bytes = (uint64_t)kCapacity * kStride;
    const size_t scratch_bytes = cts_tcp_exchange_scratch_bytes(1);
    void *arena = nullptr, *descs = nullptr, *sent = nullptr, *verify = nullptr, *ref = nullptr, *closes = nullptr,
         *cff = nullptr, *dentries = nullptr, *state = nullptr, *ids = nullptr, *rids = nullptr, *codes = nullptr,
         *tick = nullptr, *scratch = nullptr, *results = nullptr, *dexpected = nullptr;
    CHECK(hipMalloc(&arena, arena_bytes) == hipSuccess);
    CHECK(hipMalloc(&descs, kCapacity * sizeof(cts_buf_desc)) == hipSuccess);
    for (void** p : {&sent, &verify, &ref, &closes}) CHECK(hipMalloc(p, cts_counters_device_bytes()) == hipSuccess);
    CHECK(hipMalloc(&cff, kReceivers * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&dentries, kConns * sizeof(cts_tcp_exchange_state)) == hipSuccess);
    CHECK(hipMalloc(&state, kReceivers * sizeof(cts_conn_state)) == hipSuccess);
    CHECK(hipMalloc(&ids, sizeof(uint32_t)) == hipSuccess && hipMalloc(&rids, 2 * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&codes, sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&tick, sizeof(cts_tcp_exchange_tick)) == hipSuccess);
    CHECK(hipMalloc(&scratch, scratch_bytes) == hipSuccess);
    CHECK(hipMalloc(&results, 2 * sizeof(cts_conn_result)) == hipSuccess);
    CHECK(hipMalloc(&dexpected, 2 * sizeof(uint64_t)) == hipSuccess);
    CHECK(hipMemsetAsync(arena, 0xA5, arena_bytes, s) == hipSuccess);
    CHECK(hipMemsetAsync(cff, 0xFF, kReceivers * sizeof(uint32_t), s) == hipSuccess);  // every slot empty
    CHECK(hipMemsetAsync(state, 0, kReceivers * sizeof(cts_conn_state), s) == hipSuccess);
    CHECK(hipMemcpyAsync(dentries, entries.data(), kConns * sizeof(cts_tcp_exchange_state), hipMemcpyHostToDevice, s) ==
          hipSuccess);
    for (void* p : {sent, verify, ref, closes}) CHECK(cts_counters_reset(e, p, stream) == CTS_OK);
    const uint32_t listed[1] = {kConn}, receivers[2] = {kConn, kConn + kConns};
    const uint64_t receiver_bytes[2] = {expected[kConn], expected[kConn + kConns]};
    CHECK(hipMemcpyAsync(ids, listed, sizeof(listed), hipMemcpyHostToDevice, s) == hipSuccess);
    CHECK(hipMemcpyAsync(rids, receivers, sizeof(receivers), hipMemcpyHostToDevice, s) == hipSuccess);
    CHECK(hipMemcpyAsync(dexpected, receiver_bytes, sizeof(receiver_bytes), hipMemcpyHostToDevice, s) == hipSuccess);

    cts_buf_desc* dd = static_cast<cts_buf_desc*>(descs);
    uint32_t* dids = static_cast<uint32_t*>(ids);
    cts_tcp_exchange_state* ev = static_cast<cts_tcp_exchange_state*>(dentries);
    cts_tcp_exchange_tick* dtick = static_cast<cts_tcp_exchange_tick*>(tick);
    uint32_t* dcodes = static_cast<uint32_t*>(codes);
    uint32_t* dcff = static_cast<uint32_t*>(cff);
    cts_conn_state* dstate = static_cast<cts_conn_state*>(state);

    // a refused argument launches nothing
    CHECK(cts_tcp_exchange_send(e, arena, arena_bytes, kStride + 8, 0, kCapacity, dids, 1, kMaxBuffers, ev, kConns, dd,
                                dcodes, dtick, sent, scratch, scratch_bytes, stream) == CTS_E_INVALID);
    CHECK(cts_tcp_exchange_send(e, arena, arena_bytes, kStride, 0, kCapacity, dids, 1, kMaxBuffers, ev, kConns, dd,
                                dcodes, dtick, sent, scratch, scratch_bytes - 1, stream) == CTS_E_INVALID);
    CHECK(cts_tcp_exchange_send(e, arena, arena_bytes, kStride, 0, kCapacity, dids, 1, kMaxBuffers, ev, 0x80000001u, dd,
                                dcodes, dtick, sent, scratch, scratch_bytes, stream) == CTS_E_INVALID);

    // ---- the exchange: the host keeps the books of the settings only; nothing is read back inside the loop ----
    Walk walk;
    cts_tcp_exchange_state at = fresh;  // the host's copy of the entry, moved by cts_tcp_exchange_seek
    uint32_t ordinal = 0, ticks = 0, turns = 0;
    for (;; ++ticks) {
        // this tick's buffers, from the settings: the entry's next min(max_buffers, N - m)
        std::vector<cts_buf_desc> host;
        cts_buf_desc d{};
        while (host.size() < kMaxBuffers && walk.next(&d, host.size())) host.push_back(d);
        const uint32_t n = (uint32_t)host.size();
        if (n == 0) break;
        CHECK(n == std::min<uint64_t>(kMaxBuffers, at.total_buffers - at.buffers_sent));
        for (uint32_t g = 1; g < n; ++g) turns += host[g].conn_index != host[g - 1].conn_index;
        CHECK(cts_tcp_exchange_send(e, arena, arena_bytes, kStride, 0, kCapacity, dids, 1, kMaxBuffers, ev, kConns, dd,
                                    dcodes, dtick, sent, scratch, scratch_bytes, stream) == CTS_OK);
        if (ticks < 4) {
            std::vector<cts_buf_desc> got(n);
            CHECK(hipMemcpyAsync(got.data(), descs, n * sizeof(cts_buf_desc), hipMemcpyDeviceToHost, s) == hipSuccess);
            CHECK(hipStreamSynchronize(s) == hipSuccess);
            CHECK(std::memcmp(got.data(), host.data(), n * sizeof(cts_buf_desc)) == 0);
        }
        CHECK(cts_verify_at(e, arena, arena_bytes, dd, n, kStride, ordinal, nullptr, verify, dcff, kReceivers, stream) ==
              CTS_OK);
        CHECK(cts_refview_accumulate_conns(e, arena_bytes, dd, n, ordinal, dcff, kReceivers, ref, dstate, stream) ==
              CTS_OK);
        ordinal += n;
        // the host's entry follows by the closed form, and names the reference's turn
        CHECK(cts_tcp_exchange_seek(&at, at.buffers_sent + n) == CTS_OK);
        uint32_t direction = 9, intra = 9;
        CHECK(cts_tcp_exchange_where(&at, &direction, &intra) == CTS_OK);
        CHECK(at.bytes_sent[0] == walk.sent[0] && at.bytes_sent[1] == walk.sent[1]);
        CHECK(direction == (walk.sending ? 0u : 1u) && intra == walk.intra);
        CHECK(ticks < 100);
    }
    CHECK(turns > 0);  // some tick carried the connection across a segment end
    // one tick more: the connection has finished and sends nothing
    CHECK(cts_tcp_exchange_send(e, arena, arena_bytes, kStride, 0, kCapacity, dids, 1, kMaxBuffers, ev, kConns, dd, dcodes,
                                dtick, sent, scratch, scratch_bytes, stream) == CTS_OK);
    CHECK(cts_conns_close(e, static_cast<uint32_t*>(rids), static_cast<uint64_t*>(dexpected), 2, dcff, dstate, kReceivers,
                          static_cast<cts_conn_result*>(results), closes, stream) == CTS_OK);

    std::vector<cts_conn_result> r(2);
    uint32_t code = 9;
    cts_tcp_exchange_tick last{};
    CHECK(hipMemcpyAsync(r.data(), results, 2 * sizeof(cts_conn_result), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipMemcpyAsync(entries.data(), dentries, kConns * sizeof(cts_tcp_exchange_state), hipMemcpyDeviceToHost, s) ==
          hipSuccess);
    CHECK(hipMemcpyAsync(&code, codes, sizeof(code), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipMemcpyAsync(&last, tick, sizeof(last), hipMemcpyDeviceToHost, s) == hipSuccess);
    cts_counters_sent from_ticks{};
    cts_counters_close closed{};
    cts_counters_ref seen{};
    cts_counters clean{};
    CHECK(cts_counters_read_sent(e, sent, &from_ticks, stream) == CTS_OK);
    CHECK(cts_counters_read_close(e, closes, &closed, stream) == CTS_OK);
    CHECK(cts_counters_read_ref(e, ref, &seen, stream) == CTS_OK);
    CHECK(cts_counters_read(e, verify, &clean, stream) == CTS_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    for (uint32_t i = 0; i < 2; ++i) {
        CHECK(r[i].conn_index == receivers[i] && r[i].status == 0 && r[i].flags == 0 && r[i].first_fail == 0xFFFFFFFFu);
        CHECK(r[i].bytes_recv == receiver_bytes[i] && r[i].bytes_after_failure == 0);
    }
    CHECK(r[0].buffers_recv + r[1].buffers_recv == fresh.total_buffers && r[0].buffers_recv == 4 * 4 && ordinal == 23);
    CHECK(std::memcmp(&entries[kConn], &at, sizeof(at)) == 0 && at.finished == 1 && at.buffers_sent == at.total_buffers);
    CHECK(entries[0].finished == 1 && entries[0].buffers_sent == 1);  // never listed
    CHECK(code == CTS_TCP_SENDER_ENDED && last.tick.buffers == 0 && last.tick.connections_skipped == 1);
    CHECK(last.bytes_dir[0] == 0 && last.bytes_dir[1] == 0);
    CHECK(from_ticks.bytes_sent == kTransfer && from_ticks.buffers_sent == 23 && from_ticks.connections_finished == 1);
    CHECK(closed.connections_closed == 2 && closed.successful == 2 && closed.bytes_recv == kTransfer);
    CHECK(seen.bytes_recv == kTransfer && seen.buffers_recv == 23 && seen.buffers_failed == 0);
    CHECK(clean.bytes_checked == kTransfer && clean.bytes_ok == kTransfer && clean.buffers_failed == 0);

    for (void* p : {arena, descs, sent, verify, ref, closes, cff, dentries, state, ids, rids, codes, tick, scratch,
                    results, dexpected})
        CHECK(hipFree(p) == hipSuccess);
    CHECK(cts_engine_stream_destroy(e, stream) == CTS_OK);
    CHECK(cts_engine_destroy(e) == CTS_OK);
    std::printf("device_tcp_exchange: ok\n");
    return 0;
}
