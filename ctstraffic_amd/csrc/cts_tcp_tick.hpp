// cts_tcp_tick.hpp — the body of the four device-resident TCP ticks' entry points (cts_tcp_senders_send, _send_paced in
// cts_tcp_senders.cpp; cts_tcp_exchange_send, _send_paced in cts_tcp_exchange.cpp), written once: the argument checks,
// the engine's device, the scratch view, the caller's tick block or the scratch's, then the planning, the descriptor
// pass and the fill. An entry point supplies its tick and entry types, its own checks and its descriptor pass.
#pragma once

#include "cts_internal.hpp"

namespace cts {

// What the arguments of a TCP tick must satisfy once n != 0; dev_entries = the connections' table, need = the scratch
// size of that tick.
inline bool tick_args_ok(const TcpTickArgs& a, const void* dev_entries, const void* dev_tick, size_t need)
{
    if ((a.stride & 15u) != 0u || a.stride < 16u || a.stride > (16u << 20)) return false;
    if (a.max_buffers == 0u) return false;
    if (a.arena == nullptr || misaligned(a.arena, 16)) return false;
    // (first_slot + capacity) x stride <= arena_bytes, without wrap-around: compared in slots
    if (a.first_slot > a.arena_bytes / a.stride || (uint64_t)a.capacity > a.arena_bytes / a.stride - a.first_slot)
        return false;
    if (a.conn_ids == nullptr || misaligned(a.conn_ids, 4)) return false;
    if ((a.n_conns != 0 && dev_entries == nullptr) || misaligned(dev_entries, 8)) return false;
    if (a.descs == nullptr || misaligned(a.descs, 8)) return false;
    if (misaligned(a.codes, 4) || misaligned(dev_tick, 8) || misaligned(a.sent_counters, 8)) return false;
    return a.scratch != nullptr && !misaligned(a.scratch, 8) && a.scratch_bytes >= need;
}

// A paced tick's own arguments: the time and the pace table.
inline bool pace_args_ok(const TcpTickArgs& a)
{
    if (a.now_ms < 0) return false;
    return !((a.n_conns != 0 && a.pace == nullptr) || misaligned(a.pace, 8));
}

// One tick. extra_ok() = the entry point's own checks, made after the shared ones; launch_descs(scratch, tick, stream,
// geo) = its descriptor pass. The fill is the plain senders' for all four: it reads the block's first 32 bytes.
template <typename Tick, typename Entry, typename Extra, typename Descs>
int tcp_tick_send(cts_engine* e, const TcpTickArgs& a, Entry* dev_entries, Tick* dev_tick, Extra extra_ok,
                  Descs launch_descs)
{
    if (e == nullptr) return CTS_E_INVALID;
    if (a.n == 0) return CTS_OK;
    if (!tick_args_ok(a, dev_entries, dev_tick, TcpTickScratch<Tick>::bytes(a.n)) || !extra_ok()) return CTS_E_INVALID;
    int device = 0;
    const LaunchGeometry& geo = engine_geometry(e, &device);
    DeviceGuard g(device);
    if (!g.ok) return CTS_E_HIP;
    const TcpTickScratch<Tick> scratch(a.scratch, a.n);
    // the descriptor pass and the fill read the tick's buffer count: a caller that wants no tick block gets the
    // scratch's
    Tick* const tick = dev_tick != nullptr ? dev_tick : scratch.tick;
    hipStream_t const s = static_cast<hipStream_t>(a.stream);
    hipError_t rc = launch_tcp_plan(a, dev_entries, tick, scratch, s);
    if (rc != hipSuccess) return CTS_E_HIP;
    rc = launch_descs(scratch, tick, s, geo);
    if (rc != hipSuccess) return CTS_E_HIP;
    return hip_status(launch_tcp_sender_fill(static_cast<uint8_t*>(a.arena), a.arena_bytes, a.stride, a.capacity,
                                             a.descs, plain_tick(tick), s, geo));
}

}  // namespace cts
