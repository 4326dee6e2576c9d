// device_tcp_paced_exchange.cpp — one rate-limited PushPull exchange on the device from C++, through the C ABI only
// (include/cts_tcp_exchange.h; INTEGRATION.md "Send pacing for every pattern on the device-resident path"): an entry
// from cts_tcp_exchange_init, a pace entry per side from cts_tcp_sender_pace_init (the client's at c, the server's at
// c + n_conns), and per tick cts_tcp_exchange_send_paced -> cts_verify_at -> cts_refview_accumulate_conns over the
// descriptors the tick wrote; the host's one timer is the tick block's next_due_ms. Then cts_conns_close of both
// receivers against cts_tcp_exchange_direction_bytes. Beside it the host walks the pattern one buffer at a time with
// CreateNewTask's send branch (ctsIOPattern.cpp:593-674) per side, and every tick's count, descriptors and due time
// are compared with that walk. Built by `make` (ctstraffic_amd/build/device_tcp_paced_exchange) and run by
// tests/test_cpp_tcp_paced_exchange.py on the GPU box. Exits non-zero on a failed check.
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
// one connection (slot 1 of a table of 2: slot 0 stays a finished Push entry): -PushBytes 2500 -PullBytes 1500 in
// buffers of 1000, the client at 30 000 B/s in 100 ms quanta, the server two sends and then 15 ms
constexpr uint32_t kConns = 2, kConn = 1, kReceivers = 2 * kConns, kStride = 1008, kMaxBuffers = 8, kCapacity = 8;
constexpr uint32_t kBuffer = 1000, kPush = 2500, kPull = 1500;
constexpr uint64_t kTransfer = 5ull * (kPush + kPull) + kPush + 700;
constexpr int64_t kStart = 1000;

// CreateNewTask's send branch over one side's pacing state: the task's time offset.
int64_t step(cts_tcp_sender_pace& q, int64_t now, int64_t size)
{
    int64_t offset = 0;
    if (q.bytes_per_quantum > 0) {
        const int64_t period = q.quantum_period_ms;
        if (q.bytes_this_quantum < q.bytes_per_quantum) {
            q.bytes_this_quantum += size;
            if (now > q.quantum_start_ms + period) {
                const int64_t skipped = (now - q.quantum_start_ms) / period;
                q.quantum_start_ms += skipped * period;
                const int64_t adjust = q.bytes_per_quantum * skipped;
                q.bytes_this_quantum = adjust > q.bytes_this_quantum ? 0 : q.bytes_this_quantum - adjust;
            }
        } else {
            const int64_t ahead = q.bytes_this_quantum / q.bytes_per_quantum;
            q.bytes_this_quantum += size - q.bytes_per_quantum * ahead;
            if (now < q.quantum_start_ms + period) offset = q.quantum_start_ms + period - now;
            offset += (ahead - 1) * period;
            q.quantum_start_ms += ahead * period;
        }
    } else if (q.burst_count != 0) {
        if (q.burst_left == 0) q.burst_left = q.burst_count;
        if (--q.burst_left == 0) offset = q.burst_delay_ms;
    }
    return offset;
}

// The pattern, one buffer at a time (ctsIOPattern.cpp:920-992 from the client's side), each send through its side's
// pacing; a send with a time offset waits, and nothing is asked for behind it.
struct Walk {
    bool sending = true;
    uint32_t intra = 0;
    uint64_t left = kTransfer, sent[2] = {0, 0};
    cts_tcp_sender_pace pace[2];
    bool next(int64_t now, cts_buf_desc* d, uint64_t slot)
    {
        if (left == 0) return false;
        const uint32_t segment = sending ? kPush : kPull, dir = sending ? 0u : 1u;
        const uint32_t len = (uint32_t)std::min<uint64_t>({kBuffer, left, segment - intra});
        cts_tcp_sender_pace& q = pace[dir];
        if (q.pending) {
            if (now < q.due_ms) return false;
            q.pending = 0;
        } else {
            const int64_t off = step(q, now, len);
            if (off > 0) {
                q.pending = 1;
                q.due_ms = now + off;
                return false;
            }
        }
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
    CHECK(fresh.total_buffers == 5 * 5 + 3 + 1);
    // the pace table: 2 x n_conns entries, the client's at c, the server's at c + n_conns
    std::vector<cts_tcp_sender_pace> pace(2 * kConns);
    for (auto& q : pace) CHECK(cts_tcp_sender_pace_init(0, 0, 0, 0, kStart, &q) == CTS_OK);
    CHECK(cts_tcp_sender_pace_init(30000, 100, 0, 0, kStart, &pace[kConn]) == CTS_OK);
    CHECK(cts_tcp_sender_pace_init(0, 0, 2, 15, kStart, &pace[kConn + kConns]) == CTS_OK);
    CHECK(pace[kConn].bytes_per_quantum == 3000 && pace[kConn + kConns].burst_left == 2);
    const uint64_t receiver_bytes[2] = {cts_tcp_exchange_direction_bytes(&fresh, 0),
                                        cts_tcp_exchange_direction_bytes(&fresh, 1)};
    CHECK(receiver_bytes[0] == 6ull * kPush && receiver_bytes[1] == 5ull * kPull + 700);

    const uint64_t arena_bytes = (uint64_t)kCapacity * kStride;
    const size_t scratch_bytes = cts_tcp_exchange_paced_scratch_bytes(1);
    CHECK(scratch_bytes == cts_tcp_exchange_scratch_bytes(1) + 16);
    void *arena = nullptr, *descs = nullptr, *sent = nullptr, *verify = nullptr, *ref = nullptr, *closes = nullptr,
         *cff = nullptr, *dentries = nullptr, *dpace = nullptr, *state = nullptr, *ids = nullptr, *rids = nullptr,
         *codes = nullptr, *tick = nullptr, *scratch = nullptr, *results = nullptr, *dexpected = nullptr;
    CHECK(hipMalloc(&arena, arena_bytes) == hipSuccess);
    CHECK(hipMalloc(&descs, kCapacity * sizeof(cts_buf_desc)) == hipSuccess);
    for (void** p : {&sent, &verify, &ref, &closes}) CHECK(hipMalloc(p, cts_counters_device_bytes()) == hipSuccess);
    CHECK(hipMalloc(&cff, kReceivers * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&dentries, kConns * sizeof(cts_tcp_exchange_state)) == hipSuccess);
    CHECK(hipMalloc(&dpace, 2 * kConns * sizeof(cts_tcp_sender_pace)) == hipSuccess);
    CHECK(hipMalloc(&state, kReceivers * sizeof(cts_conn_state)) == hipSuccess);
    CHECK(hipMalloc(&ids, sizeof(uint32_t)) == hipSuccess && hipMalloc(&rids, 2 * sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&codes, sizeof(uint32_t)) == hipSuccess);
    CHECK(hipMalloc(&tick, sizeof(cts_tcp_exchange_paced_tick)) == hipSuccess);
    CHECK(hipMalloc(&scratch, scratch_bytes) == hipSuccess);
    CHECK(hipMalloc(&results, 2 * sizeof(cts_conn_result)) == hipSuccess);
    CHECK(hipMalloc(&dexpected, 2 * sizeof(uint64_t)) == hipSuccess);
    CHECK(hipMemsetAsync(arena, 0xA5, arena_bytes, s) == hipSuccess);
    CHECK(hipMemsetAsync(cff, 0xFF, kReceivers * sizeof(uint32_t), s) == hipSuccess);  // every slot empty
    CHECK(hipMemsetAsync(state, 0, kReceivers * sizeof(cts_conn_state), s) == hipSuccess);
    CHECK(hipMemcpyAsync(dentries, entries.data(), kConns * sizeof(cts_tcp_exchange_state), hipMemcpyHostToDevice, s) ==
          hipSuccess);
    CHECK(hipMemcpyAsync(dpace, pace.data(), 2 * kConns * sizeof(cts_tcp_sender_pace), hipMemcpyHostToDevice, s) ==
          hipSuccess);
    for (void* p : {sent, verify, ref, closes}) CHECK(cts_counters_reset(e, p, stream) == CTS_OK);
    const uint32_t listed[1] = {kConn}, receivers[2] = {kConn, kConn + kConns};
    CHECK(hipMemcpyAsync(ids, listed, sizeof(listed), hipMemcpyHostToDevice, s) == hipSuccess);
    CHECK(hipMemcpyAsync(rids, receivers, sizeof(receivers), hipMemcpyHostToDevice, s) == hipSuccess);
    CHECK(hipMemcpyAsync(dexpected, receiver_bytes, sizeof(receiver_bytes), hipMemcpyHostToDevice, s) == hipSuccess);

    cts_buf_desc* dd = static_cast<cts_buf_desc*>(descs);
    uint32_t* dids = static_cast<uint32_t*>(ids);
    cts_tcp_exchange_state* ev = static_cast<cts_tcp_exchange_state*>(dentries);
    cts_tcp_sender_pace* pv = static_cast<cts_tcp_sender_pace*>(dpace);
    cts_tcp_exchange_paced_tick* dtick = static_cast<cts_tcp_exchange_paced_tick*>(tick);
    uint32_t* dcodes = static_cast<uint32_t*>(codes);
    uint32_t* dcff = static_cast<uint32_t*>(cff);
    cts_conn_state* dstate = static_cast<cts_conn_state*>(state);

    // a refused argument launches nothing
    CHECK(cts_tcp_exchange_send_paced(e, arena, arena_bytes, kStride, 0, kCapacity, dids, 1, kMaxBuffers, ev, nullptr,
                                      kConns, kStart, dd, dcodes, dtick, sent, scratch, scratch_bytes, stream) ==
          CTS_E_INVALID);
    CHECK(cts_tcp_exchange_send_paced(e, arena, arena_bytes, kStride, 0, kCapacity, dids, 1, kMaxBuffers, ev, pv, kConns,
                                      -1, dd, dcodes, dtick, sent, scratch, scratch_bytes, stream) == CTS_E_INVALID);
    CHECK(cts_tcp_exchange_send_paced(e, arena, arena_bytes, kStride, 0, kCapacity, dids, 1, kMaxBuffers, ev, pv, kConns,
                                      kStart, dd, dcodes, dtick, sent, scratch, scratch_bytes - 1, stream) ==
          CTS_E_INVALID);

    // ---- the exchange: one tick per due time; the only thing read back inside the loop is the tick block ----
    Walk walk;
    walk.pace[0] = pace[kConn];
    walk.pace[1] = pace[kConn + kConns];
    int64_t now = kStart;
    uint32_t ordinal = 0, ticks = 0, waited = 0, server_waited = 0;
    while (walk.left != 0) {
        std::vector<cts_buf_desc> host;
        cts_buf_desc d{};
        while (host.size() < kMaxBuffers && walk.next(now, &d, host.size())) host.push_back(d);
        const uint32_t n = (uint32_t)host.size();
        CHECK(cts_tcp_exchange_send_paced(e, arena, arena_bytes, kStride, 0, kCapacity, dids, 1, kMaxBuffers, ev, pv,
                                          kConns, now, dd, dcodes, dtick, sent, scratch, scratch_bytes, stream) == CTS_OK);
        if (n != 0) {
            CHECK(cts_verify_at(e, arena, arena_bytes, dd, n, kStride, ordinal, nullptr, verify, dcff, kReceivers,
                                stream) == CTS_OK);
            CHECK(cts_refview_accumulate_conns(e, arena_bytes, dd, n, ordinal, dcff, kReceivers, ref, dstate, stream) ==
                  CTS_OK);
        }
        ordinal += n;
        cts_tcp_exchange_paced_tick t{};
        std::vector<cts_buf_desc> got(n);
        CHECK(hipMemcpyAsync(&t, tick, sizeof(t), hipMemcpyDeviceToHost, s) == hipSuccess);
        if (n != 0)
            CHECK(hipMemcpyAsync(got.data(), descs, n * sizeof(cts_buf_desc), hipMemcpyDeviceToHost, s) == hipSuccess);
        CHECK(hipStreamSynchronize(s) == hipSuccess);
        CHECK(t.tick.tick.buffers == n && t.connections_waiting == (n == 0 ? 1u : 0u));
        CHECK(n == 0 || std::memcmp(got.data(), host.data(), n * sizeof(cts_buf_desc)) == 0);
        // at most one side holds a task, and its due time is the tick's
        CHECK(walk.pace[0].pending + walk.pace[1].pending <= 1);
        const bool pending = walk.pace[0].pending + walk.pace[1].pending != 0;
        CHECK(t.connections_pending == (pending ? 1u : 0u));
        if (pending) {
            const int64_t due = walk.pace[0].pending ? walk.pace[0].due_ms : walk.pace[1].due_ms;
            CHECK(t.next_due_ms == due && due > now);
            now = due;  // the host's one timer
            ++waited;
            server_waited += walk.pace[1].pending;
        } else {
            CHECK(t.next_due_ms == INT64_MAX);
        }
        CHECK(++ticks < 200);
    }
    CHECK(waited > 5 && server_waited > 0 && server_waited < waited);  // both sides have held the connection
    CHECK(cts_conns_close(e, static_cast<uint32_t*>(rids), static_cast<uint64_t*>(dexpected), 2, dcff, dstate, kReceivers,
                          static_cast<cts_conn_result*>(results), closes, stream) == CTS_OK);

    std::vector<cts_conn_result> r(2);
    std::vector<cts_tcp_sender_pace> after(2 * kConns);
    CHECK(hipMemcpyAsync(r.data(), results, 2 * sizeof(cts_conn_result), hipMemcpyDeviceToHost, s) == hipSuccess);
    CHECK(hipMemcpyAsync(entries.data(), dentries, kConns * sizeof(cts_tcp_exchange_state), hipMemcpyDeviceToHost, s) ==
          hipSuccess);
    CHECK(hipMemcpyAsync(after.data(), dpace, 2 * kConns * sizeof(cts_tcp_sender_pace), hipMemcpyDeviceToHost, s) ==
          hipSuccess);
    cts_counters_sent from_ticks{};
    cts_counters_close closed{};
    cts_counters clean{};
    CHECK(cts_counters_read_sent(e, sent, &from_ticks, stream) == CTS_OK);
    CHECK(cts_counters_read_close(e, closes, &closed, stream) == CTS_OK);
    CHECK(cts_counters_read(e, verify, &clean, stream) == CTS_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    for (uint32_t i = 0; i < 2; ++i) {
        CHECK(r[i].conn_index == receivers[i] && r[i].status == 0 && r[i].flags == 0 && r[i].first_fail == 0xFFFFFFFFu);
        CHECK(r[i].bytes_recv == receiver_bytes[i] && r[i].bytes_after_failure == 0);
    }
    CHECK(entries[kConn].finished == 1 && entries[kConn].buffers_sent == fresh.total_buffers && ordinal == 29);
    CHECK(entries[kConn].bytes_sent[0] == walk.sent[0] && entries[kConn].bytes_sent[1] == walk.sent[1]);
    // both sides' pace entries are the walk's; the unused slot's two entries have not been touched
    CHECK(std::memcmp(&after[kConn], &walk.pace[0], sizeof(cts_tcp_sender_pace)) == 0);
    CHECK(std::memcmp(&after[kConn + kConns], &walk.pace[1], sizeof(cts_tcp_sender_pace)) == 0);
    CHECK(std::memcmp(&after[0], &pace[0], sizeof(cts_tcp_sender_pace)) == 0);
    CHECK(std::memcmp(&after[kConns], &pace[kConns], sizeof(cts_tcp_sender_pace)) == 0);
    CHECK(from_ticks.bytes_sent == kTransfer && from_ticks.buffers_sent == 29 && from_ticks.connections_finished == 1);
    CHECK(closed.connections_closed == 2 && closed.successful == 2 && closed.bytes_recv == kTransfer);
    CHECK(clean.bytes_checked == kTransfer && clean.bytes_ok == kTransfer && clean.buffers_failed == 0);

    for (void* p : {arena, descs, sent, verify, ref, closes, cff, dentries, dpace, state, ids, rids, codes, tick, scratch,
                    results, dexpected})
        CHECK(hipFree(p) == hipSuccess);
    CHECK(cts_engine_stream_destroy(e, stream) == CTS_OK);
    CHECK(cts_engine_destroy(e) == CTS_OK);
    std::printf("device_tcp_paced_exchange: ok\n");
    return 0;
}
