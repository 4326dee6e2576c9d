// cts_tcp_exchange.cpp — Push, Pull, PushPull and Duplex connections on the device-resident path
// (cts_tcp_exchange.h): the host-side entry helpers (cts_tcp_exchange_init, _seek, _where, _direction_bytes), the
// scratch sizes, the tick (cts_tcp_exchange_send) and the paced tick (cts_tcp_exchange_send_paced).
//
// A translation unit of its own, like cts_tcp_senders.cpp: nothing else in the library references these entry points.
// The helpers are the closed forms of cts_tcp_exchange_math.hpp, the ones the kernels run: no loop over buffers, so a
// seek past 2^33 costs what a seek to 0 costs. No threads, no allocation.
#include <hip/hip_runtime_api.h>

#include "cts_internal.hpp"
#include "cts_tcp_exchange.h"
#include "cts_tcp_exchange_math.hpp"
#include "cts_tcp_tick.hpp"

static_assert(sizeof(cts_tcp_exchange_state) == 64 && alignof(cts_tcp_exchange_state) == 8,
              "cts_tcp_exchange_state: 64 bytes");
static_assert(sizeof(cts_tcp_exchange_tick) == 48 && alignof(cts_tcp_exchange_tick) == 8 &&
                  offsetof(cts_tcp_exchange_tick, bytes_dir) == 32,
              "cts_tcp_exchange_tick: a plain tick and 16 bytes");
static_assert(sizeof(cts_tcp_exchange_paced_tick) == 64 && alignof(cts_tcp_exchange_paced_tick) == 8 &&
                  offsetof(cts_tcp_exchange_paced_tick, next_due_ms) == 48,
              "cts_tcp_exchange_paced_tick: an exchange tick and 16 bytes");

namespace {

// the direction-1 receiver, and a paced tick's direction-1 pace entry, of connection c is c + n_conns
bool receivers_ok(const cts::TcpTickArgs& a) { return a.n_conns <= (1u << 31); }

// The descriptor pass of both ticks, the plain exchange tick's: it reads the tick block's first 48 bytes.
auto exchange_descs(const cts::TcpTickArgs& a, const cts_tcp_exchange_state* entries)
{
    return [&a, entries](const auto& scratch, auto* tick, hipStream_t s, const cts::LaunchGeometry& geo) {
        return cts::launch_tcp_exchange_descs(a.stride, a.first_slot, a.capacity, a.conn_ids, a.n, entries, a.n_conns,
                                              scratch.prefix, scratch.before, cts::exchange_tick(tick), a.descs, s,
                                              geo);
    };
}

// An entry as cts_tcp_exchange_init makes it, wherever it has been moved since.
bool well_formed(const cts_tcp_exchange_state* e)
{
    if (e == nullptr || e->transfer_bytes == 0) return false;
    const cts::ExchangeShape s = cts::exchange_shape(e);
    if (!cts::exchange_shape_ok(s)) return false;
    if (s.pattern == CTS_TCP_EXCHANGE_DUPLEX && (s.T & 1u) != 0u) return false;
    return s.N == cts::exchange_total_buffers(s);
}

}  // namespace

extern "C" {

int cts_tcp_exchange_init(uint32_t pattern, uint64_t transfer_bytes, uint32_t buffer_size, uint32_t push_bytes,
                          uint32_t pull_bytes, cts_tcp_exchange_state* out)
{
    if (out == nullptr || transfer_bytes == 0 || buffer_size == 0 || pattern > CTS_TCP_EXCHANGE_DUPLEX)
        return CTS_E_INVALID;
    if (pattern == CTS_TCP_EXCHANGE_PUSHPULL && (push_bytes == 0 || pull_bytes == 0)) return CTS_E_INVALID;
    if (pattern == CTS_TCP_EXCHANGE_DUPLEX && (transfer_bytes & 1u) != 0u) {
        // max transfer bytes must be even so that send bytes and recv bytes balance (ctsIOPattern.cpp:1004-1009)
        if (transfer_bytes == UINT64_MAX) return CTS_E_INVALID;
        transfer_bytes += 1u;
    }
    *out = cts_tcp_exchange_state{};
    out->transfer_bytes = transfer_bytes;
    out->buffer_size = buffer_size;
    out->pattern = pattern;
    out->push_bytes = push_bytes;
    out->pull_bytes = pull_bytes;
    out->total_buffers = cts::exchange_total_buffers(cts::exchange_shape(out));
    return CTS_OK;
}

int cts_tcp_exchange_seek(cts_tcp_exchange_state* entry, uint64_t m)
{
    if (!well_formed(entry) || m > entry->total_buffers) return CTS_E_INVALID;
    cts::exchange_position(cts::exchange_shape(entry), m, entry->bytes_sent);
    entry->buffers_sent = m;
    entry->finished = m == entry->total_buffers ? 1u : 0u;
    return CTS_OK;
}

int cts_tcp_exchange_where(const cts_tcp_exchange_state* entry, uint32_t* direction, uint32_t* intra)
{
    if (!well_formed(entry) || entry->buffers_sent > entry->total_buffers) return CTS_E_INVALID;
    const cts::ExchangeShape s = cts::exchange_shape(entry);
    const uint64_t m = entry->buffers_sent;
    uint32_t d = 0u, in_seg = 0u;
    if (s.pattern == CTS_TCP_EXCHANGE_PUSHPULL) {
        // what the segments before the position leave of the cycle it is in: below P the push segment is open, from P
        // on the pull segment (a segment that has just filled has flipped the turn, ctsIOPattern.cpp:985-989)
        uint64_t sent[2];
        cts::exchange_position(s, m, sent);
        const uint64_t in_cycle = (sent[0] + sent[1]) % ((uint64_t)s.P + s.Q);
        d = in_cycle < s.P ? 0u : 1u;
        in_seg = (uint32_t)(d == 0u ? in_cycle : in_cycle - s.P);
    } else if (s.pattern == CTS_TCP_EXCHANGE_DUPLEX) {
        d = (uint32_t)(m & 1u);
    } else {
        d = s.pattern == CTS_TCP_EXCHANGE_PULL ? 1u : 0u;
    }
    if (direction != nullptr) *direction = d;
    if (intra != nullptr) *intra = in_seg;
    return CTS_OK;
}

uint64_t cts_tcp_exchange_direction_bytes(const cts_tcp_exchange_state* entry, uint32_t direction)
{
    if (!well_formed(entry) || direction > 1u) return 0u;
    return cts::exchange_direction_total(cts::exchange_shape(entry), direction);
}

size_t cts_tcp_exchange_scratch_bytes(uint32_t n) { return cts::TcpTickScratch<cts_tcp_exchange_tick>::bytes(n); }

int cts_tcp_exchange_send(cts_engine* e, void* dev_arena, uint64_t arena_bytes, uint32_t stride, uint64_t first_slot,
                          uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n, uint32_t max_buffers,
                          cts_tcp_exchange_state* dev_entries, uint32_t n_conns, cts_buf_desc* dev_descs,
                          uint32_t* dev_codes, cts_tcp_exchange_tick* dev_tick, void* dev_sent_counters,
                          void* dev_scratch, size_t scratch_bytes, void* stream)
{
    const cts::TcpTickArgs a{dev_arena, arena_bytes, stride, first_slot, capacity, dev_conn_ids, n, max_buffers, n_conns,
                             dev_descs, dev_codes, dev_sent_counters, dev_scratch, scratch_bytes, stream, nullptr, 0};
    return cts::tcp_tick_send(e, a, dev_entries, dev_tick, [&] { return receivers_ok(a); },
                              exchange_descs(a, dev_entries));
}

size_t cts_tcp_exchange_paced_scratch_bytes(uint32_t n)
{
    return cts::TcpTickScratch<cts_tcp_exchange_paced_tick>::bytes(n);
}

int cts_tcp_exchange_send_paced(cts_engine* e, void* dev_arena, uint64_t arena_bytes, uint32_t stride,
                                uint64_t first_slot, uint32_t capacity, const uint32_t* dev_conn_ids, uint32_t n,
                                uint32_t max_buffers, cts_tcp_exchange_state* dev_entries,
                                cts_tcp_sender_pace* dev_pace, uint32_t n_conns, int64_t now_ms,
                                cts_buf_desc* dev_descs, uint32_t* dev_codes, cts_tcp_exchange_paced_tick* dev_tick,
                                void* dev_sent_counters, void* dev_scratch, size_t scratch_bytes, void* stream)
{
    const cts::TcpTickArgs a{dev_arena, arena_bytes, stride, first_slot, capacity, dev_conn_ids, n, max_buffers, n_conns,
                             dev_descs, dev_codes, dev_sent_counters, dev_scratch, scratch_bytes, stream, dev_pace, now_ms};
    return cts::tcp_tick_send(e, a, dev_entries, dev_tick, [&] { return receivers_ok(a) && cts::pace_args_ok(a); },
                              exchange_descs(a, dev_entries));
}

}  // extern "C"
