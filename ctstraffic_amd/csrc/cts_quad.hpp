// cts_quad.hpp — four buffers per wave: the machinery that verify_quad_kernel (cts_verify.hip) and the MediaStream
// receive (cts_media_stream_recv.hip) share.
//
// 16-lane teams, one buffer each (datagram-sized spans).
// A whole wave per 1472-byte datagram issues its per-buffer scalar work (descriptor,
// span set-up, edge lanes, record, counters) once per datagram, and a third of its
// lanes' loads fall past the span (4.71 against 5.95 TB/s of payload for this form on
// config 3, tools/rounds/r04/media_stream_probe.py). Here a wave's instructions serve four datagrams at once: the span fields live in VGPRs (one
// descriptor per team), each load instruction fetches four 256-byte runs, and
// U loads per lane cover 16*U chunks per round (U = 6: 1536 B, one round for a
// 1446-byte payload at any alignment). Loads are global (per-lane 64-bit
// addresses: a buffer resource must be wave-uniform); addresses of chunks outside
// a span are clamped into it (same lines, no extra traffic) and their compare is
// discarded. The rounds start on the 128-byte line of chunk 0 (the line-aligned
// interior of scan_buffer), so a team's run covers 2 lines, not 3.
// A team whose OR is nonzero (rare; the verdict is a wave ballot) re-reads its own
// chunks exactly and reduces (first, count) over its 16 lanes.
#pragma once

#include <type_traits>

#include "cts_chunks.hpp"

namespace cts {

__device__ __forceinline__ void take_diff_at(uint32_t c, uint32_t lo, u32x4 x, uint32_t& first, uint32_t& count)
{
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t nz = nonzero_bytes(x[w]);
        if (nz) {
            const uint32_t pos = 16u * c + 4u * (uint32_t)w + ((uint32_t)__builtin_ctz(nz) >> 3) - lo;
            first = pos < first ? pos : first;
            count += (uint32_t)__builtin_popcount(nz);
        }
    }
}

constexpr int kQuadTeam = 16;  // lanes per buffer in the four-buffers-per-wave kernels

// A team's span, all fields per lane (VGPRs): the four teams of a wave hold four buffers.
struct QSpan {
    const u32x4* p;     // chunk 0 (16-byte aligned)
    const uint8_t* sp;  // first verified byte
    uint32_t len, nch, hi_last, lo, q0, sh;
    int last;  // address clamp: the last chunk (0 for an empty span)
    int cs;    // first chunk of round 0: the first chunk of chunk 0's 128-byte line (-7..0)
    int c_hi;  // last interior chunk (nch - 2)
};

// Span of [sp, sp + len) at pattern offset `expected`; an empty span (len 0: an idle
// team, a bad descriptor, a non-DATA datagram) points at `dummy`, 16-byte-aligned
// memory the clamped loads may read (every compare of an empty span is discarded).
__device__ __forceinline__ QSpan quad_span(const uint8_t* sp, uint32_t len, uint32_t expected, const void* dummy)
{
    QSpan q;
    q.sp = len ? sp : reinterpret_cast<const uint8_t*>(dummy);
    q.len = len;
    q.lo = (uint32_t)((uintptr_t)q.sp & 15u);
    q.nch = len == 0u ? 0u : (uint32_t)(((uint64_t)q.lo + len + 15u) >> 4);
    q.hi_last = len == 0u ? 0u : (uint32_t)((uint64_t)q.lo + len - 16ull * (q.nch - 1u));
    q.q0 = (expected - q.lo) & 0xFFFFu;
    q.sh = q.q0 & 1u;
    q.p = reinterpret_cast<const u32x4*>(q.sp - q.lo);
    q.last = q.nch == 0u ? 0 : (int)q.nch - 1;
    q.cs = -(int)(((uintptr_t)q.p >> 4) & 7u);
    q.c_hi = (int)q.nch - 2;
    return q;
}

// Edge chunk of a team lane: lane 0 chunk 0, lane 1 the last chunk (others: none).
__device__ __forceinline__ bool quad_edge_used(const QSpan& q, uint32_t lane)
{
    return (lane == 0u && q.nch >= 1u) || (lane == 1u && q.nch >= 2u);
}
__device__ __forceinline__ uint32_t quad_edge_chunk(const QSpan& q, uint32_t lane) { return lane == 1u ? (uint32_t)q.last : 0u; }
__device__ __forceinline__ u32x4 quad_edge_xor(const QSpan& q, uint32_t ce, u32x4 data)
{
    return (data ^ expected_chunk((q.q0 + 16u * ce) & 0xFFFFu, q.sh)) &
           range_mask(ce == 0u ? q.lo : 0u, ce == (uint32_t)q.last ? q.hi_last : 16u);
}

// Interior [1, nch-1) in rounds of U loads per lane starting at chunk cs (the wave loops
// while any of its teams has chunks left); returns the OR of this lane's differences.
// Chunks outside the span are clamped to its first / last chunk.
template <int U, bool NT>
__device__ __forceinline__ uint32_t quad_scan_interior(const QSpan& q, uint32_t lane)
{
    constexpr int ROUND = kQuadTeam * U;
    uint32_t acc = 0;
    for (int r = 0; __any(q.cs + r * ROUND <= q.c_hi); ++r) {
        const int cb = q.cs + r * ROUND + (int)lane;
        u32x4 dd[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int c = cb + u * kQuadTeam;
            c = c < 0 ? 0 : (c > q.last ? q.last : c);
            dd[u] = load_chunk_g<NT>(q.p + c);
        }
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t k = ((q.q0 + 16u * (uint32_t)cb) & 0xFFFFu) >> 1;
        const uint32_t B = __umul24(k, 0x10001u) + 0x10000u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = cb + u * kQuadTeam;
            const uint32_t any = or4(dd[u] ^ expected_step<kQuadTeam, U>(B, u, q.sh));
            acc |= (c >= 1 && c <= q.c_hi) ? any : 0u;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    return acc;
}

// Exact re-read of exactly the chunks this lane owns (interior chunks = cs + lane mod 16,
// plus its edge chunk): first differing byte (span-relative) and differing-byte count.
template <bool NT>
__device__ __forceinline__ void quad_scan_exact(const QSpan& q, uint32_t lane, uint32_t& first, uint32_t& count)
{
    for (int c = q.cs + (int)lane; c <= q.c_hi; c += kQuadTeam) {
        if (c >= 1)
            take_diff_at((uint32_t)c, q.lo,
                         load_chunk_g<NT>(q.p + c) ^ expected_chunk((q.q0 + 16u * (uint32_t)c) & 0xFFFFu, q.sh), first,
                         count);
    }
    if (quad_edge_used(q, lane)) {
        const uint32_t ce = quad_edge_chunk(q, lane);
        take_diff_at(ce, q.lo, quad_edge_xor(q, ce, load_chunk_g<NT>(q.p + ce)), first, count);
    }
}

// min / sum over the 16 lanes of each team (all lanes of the wave take part)
__device__ __forceinline__ void quad_team_reduce(uint32_t& first, uint32_t& count)
{
#pragma unroll
    for (int off = kQuadTeam / 2; off > 0; off >>= 1) {
        const uint32_t of = (uint32_t)__shfl_xor((int)first, off, kQuadTeam);
        first = of < first ? of : first;
        count += (uint32_t)__shfl_xor((int)count, off, kQuadTeam);
    }
}

// Team-leader running counters (registers), written to LDS once at the end.
struct QCounters {
    uint64_t bytes = 0, ok = 0, mism = 0;
    uint32_t bufs = 0, fail = 0, conns = 0;
    __device__ __forceinline__ void add(uint32_t len, bool pass, uint32_t count)
    {
        bytes += len;
        bufs += 1u;
        if (pass) {
            ok += len;
        } else {
            fail += 1u;
            mism += count;
        }
    }
    template <int TEAMS>
    __device__ __forceinline__ void flush(uint64_t (*ctr)[kCounterCount], uint32_t team, uint32_t lane,
                                          uint64_t* counters) const
    {
        if (lane == 0u) {
            ctr[team][kBytesChecked] = bytes;
            ctr[team][kBytesOk] = ok;
            ctr[team][kBuffersChecked] = bufs;
            ctr[team][kBuffersFailed] = fail;
            ctr[team][kMismatchedBytes] = mism;
            ctr[team][kConnectionsFailed] = conns;
        }
        flush_counters<TEAMS>(counters, ctr);
    }
};

// Per-wave output staging for the four-buffers-per-wave kernels. Each team leader puts its
// 12-byte result (and, for MediaStream, its 32-byte record) in LDS as whole dwords; the wave
// then writes the four teams' outputs from consecutive lanes: one coalesced dword store covers
// 4 x 12 = 48 contiguous result bytes, one covers 4 x 32 = 128 record bytes. Written directly,
// each leader's struct became 4-lane sub-dword and unaligned stores (global_store_short/byte,
// dword at +7): on 4 M datagrams the records alone added 265 us to a 920 us launch
// (tools/rounds/r04/media_stream_probe.py). Nontemporal stores here measured 2-4 % slower; write-through
// (sc1) stores helped the records and hurt the results, and deferring the stores until the next
// buffer's loads were in flight changed nothing (+-0.5 %).
struct QuadOut {
    uint32_t res[4][3];
    uint32_t rec[4][8];
};

__device__ __forceinline__ uint32_t result_dw2(uint32_t expected, uint32_t actual, uint32_t pass, uint32_t flags)
{
    return (expected & 0xFFu) | ((actual & 0xFFu) << 8) | (pass << 16) | (flags << 24);  // bytes 8..11
}

template <typename O>
__device__ __forceinline__ void quad_stage_result(O& o, uint32_t t, uint32_t first_mismatch,
                                                  uint32_t mismatch_bytes, uint32_t dw2)
{
    o.res[t][0] = first_mismatch;
    o.res[t][1] = mismatch_bytes;
    o.res[t][2] = dw2;
}

// All 64 lanes of the wave call this after the leaders staged their results; i = this lane's buffer index
// (the wave's four teams hold i0 .. i0 + 3, i0 = lane 0's), n = buffers in the launch.
__device__ __forceinline__ void quad_flush_results(const QuadOut& o, uint32_t i, uint32_t n, cts_verify_result* results)
{
    __builtin_amdgcn_wave_barrier();
    // (64-bit: i0 + t may pass 2^32 on the wave's last round when n is close to it)
    const uint64_t i0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)i);
    const uint32_t l = threadIdx.x & 63u;
    if (results != nullptr && l < 12u) {
        const uint32_t t = l / 3u;
        const uint32_t v = o.res[t][l - 3u * t];
        if (i0 + t < n) reinterpret_cast<uint32_t*>(results)[3ull * i0 + l] = v;
    }
    __builtin_amdgcn_wave_barrier();
}

// The MediaStream receive writes its records + results every kMsRing rounds from the per-wave ring: for config 3
// (1 024 datagrams per workgroup, 64 rounds per wave) once, at the workgroup's end. 4.25 vs 4.30 ms per 16 M
// datagrams written every round (two boxes, profiles/r02/ms_records_ring/); 45 KB of LDS per workgroup.
constexpr int kMsRing = 64;

// Per-wave output ring: the staged outputs of K rounds (QuadOut slots) and each round's first buffer
// index, written by the wave every K rounds instead of every round. A read stream slows down with the
// FREQUENCY of the writes mixed into it, not with their bytes (tools/rw_mix_probe.hip: one dword per wave
// per 4 KiB round costs the read 18 %, the same store on every 16th round 5 %, on every 64th round
// nothing measurable; 4 to 120 bytes per store cost the same).
// A ring slot of the compact receive: four cts_datagram_status entries (4 dwords each), no result records.
struct QuadStatusOut {
    uint32_t rec[4][4];
};

template <int K, typename SlotT = QuadOut>
struct QuadRing {
    SlotT slot[K];
    uint32_t i0[K];
};

// All 64 lanes: write rounds [0, m) of the ring (round j's four buffers start at i0[j]); n = buffers in
// the launch. Records go as agent-scope relaxed atomic dwords, RECDW x 4 per round, results as plain dwords,
// 12 per round.
// RECDW = dwords per record: 8 (cts_datagram_record) or 4 (cts_datagram_status, staged in rec[t][0..3]).
template <int K, int RECDW = 8, typename SlotT = QuadOut>
__device__ __forceinline__ void quad_ring_flush(const QuadRing<K, SlotT>& g, uint32_t m, uint32_t n,
                                                cts_verify_result* results, void* records)
{
    __builtin_amdgcn_wave_barrier();
    const uint32_t l = threadIdx.x & 63u;
    if (records != nullptr) {
#pragma unroll 1  // (unrolled, the LDS reads are hoisted into ~80 VGPRs: occupancy 4 -> 2 waves/SIMD)
        for (uint32_t k = 0; k < (K * 4u * RECDW + 63u) / 64u; ++k) {
            const uint32_t e = k * 64u + l, j = e / (4u * RECDW), d = e % (4u * RECDW);
            if (j < m) {
                const uint64_t i0 = g.i0[j];
                if (i0 + d / RECDW < n)
                    __hip_atomic_store(reinterpret_cast<uint32_t*>(records) + (uint64_t)RECDW * i0 + d,
                                       g.slot[j].rec[d / RECDW][d % RECDW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if constexpr (!std::is_same<SlotT, QuadStatusOut>::value)
    if (results != nullptr) {
#pragma unroll 1
        for (uint32_t k = 0; k < (K * 12u + 63u) / 64u; ++k) {
            const uint32_t e = k * 64u + l, j = e / 12u, d = e - 12u * j;
            if (j < m) {
                const uint64_t i0 = g.i0[j];
                const uint32_t t = d / 3u;
                if (i0 + t < n) reinterpret_cast<uint32_t*>(results)[3ull * i0 + d] = g.slot[j].res[t][d - 3u * t];
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// Which buffers a team visits: the buffers are cut into chunks of `per` consecutive buffers (a multiple of
// TEAMS); block b walks chunks b, b + grid, ... TEAMS buffers at a time, so the rounds of a wave write adjacent
// outputs and a 128-byte line of 12-byte results fills up in ONE CU's L2 (a grid-stride walk spreads a line over
// workgroups on different XCDs: partial-line writes, 0-5 % slower, tools/rounds/r04/media_stream_probe.py). One chunk per
// block (contig_grid's default) is a fully block-contiguous walk.
template <int TEAMS>
struct QuadWalk {
    uint32_t i, end;
    uint64_t cbase;  // first buffer of the current chunk
    uint32_t per, team;
    __device__ __forceinline__ QuadWalk(uint32_t n, uint32_t per_, uint32_t team_) : end(n), per(per_), team(team_)
    {
        cbase = (uint64_t)blockIdx.x * per;
        i = cbase + team < (uint64_t)n ? (uint32_t)(cbase + team) : n;
    }
    // the buffer after i (end when none); moves to the block's next chunk at a chunk's end
    __device__ __forceinline__ uint32_t next()
    {
        uint64_t nx = (uint64_t)i + TEAMS;
        if (nx - cbase >= per) {
            cbase += (uint64_t)gridDim.x * per;
            nx = cbase + team;
        }
        return nx < (uint64_t)end ? (uint32_t)nx : end;
    }
};

// A quad-team walk's buffer i from its source (VSource, cts_device_util.hpp): a descriptor, or a strided ring's slot.
template <bool STRIDED>
__device__ __forceinline__ cts_buf_desc vs_desc(const VSource& src, uint32_t i)
{
    if constexpr (STRIDED) {
        const uint32_t len = src.lens[i];
        // a completion longer than its slot would overlap the next one: flagged (an out-of-range
        // expected offset makes desc_bad reject it) rather than read
        return cts_buf_desc{(uint64_t)i * src.stride, len, len <= src.stride ? src.expected : 65536u, src.conn_index,
                            src.skip_head};
    } else {
        return src.descs[i];
    }
}

// U = 6 loads per lane per round: 1536 B per team, one round for a 1446-byte payload at any alignment.
// The two edge chunks are loaded first with the default (L2-allocating) policy, so the lines they bring into L2
// stay there for the round loads that request them again (nontemporal, they sat at L2's LRU position and were
// often gone: config 3, 4 M datagrams, 8 M extra L2 requests and FETCH_SIZE 1.7 % over the arena,
// profiles/r03/dg_probe/).
constexpr int kQuadLoads = 6;

}  // namespace cts
