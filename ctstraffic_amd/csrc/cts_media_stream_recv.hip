// cts_media_stream_recv.hip — the MediaStream (UDP) receive for gfx950: header + payload, four datagrams per wave
// (16-lane teams, cts_quad.hpp; see verify_quad_kernel in cts_verify.hip).
//   media_stream_verify_quad_kernel   cts_media_stream_verify / _status / _frames and their strided forms
//   ms_verify_status_ordinal          cts_media_stream_verify_status_at: the status form that also lowers the DataError
//                                     slots of the device-resident connections
// Both are one body (ms_verify_quad_body), so all their instantiations stay in this unit (DESIGN.md §File layout).
// Receive: parse + validate the header (ctsMediaStreamProtocol.hpp:284-329), then verify the payload of
// DATA datagrams at pattern offset 0 after the 26-byte header (ctsIOPatternMediaStream.cpp:185-192).
// Team lanes 0..2 load the 16-byte chunks holding the header alongside the speculative DATA payload
// stream; the header dwords reach the team leader through DPP row shifts, with no dependent memory round
// trip (header bytes by byte loads and lane shuffles, one wave per datagram, and two-pass receives measured slower:
// tools/rounds/r04/media_stream_probe.py).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cts_chunks.hpp"
#include "cts_launch.hpp"
#include "cts_quad.hpp"

namespace cts {

// Team lane 0 receives dword c of lane `from`'s u32x4 (from = 1, 2) within its 16-lane DPP
// row (row_shl:from; a VALU move, no LDS round trip).
template <int FROM>
__device__ __forceinline__ uint32_t row_shl(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 | FROM, 0xF, 0xF, true);
}

// Header dwords: team lanes 0..2 each hold one 16-byte chunk of
// the 48-byte window starting at the datagram's 16-byte-aligned base; header byte b sits at
// window byte ho + b. Returns dwords H[0..5] = header bytes 0..23 on team lane 0.
__device__ __forceinline__ void header_dwords_hdr16(u32x4 own, uint32_t ho, uint32_t (&H)[6])
{
    uint32_t W[12];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        W[c] = own[c];
        W[4 + c] = row_shl<1>(own[c]);
        W[8 + c] = row_shl<2>(own[c]);
    }
    // the 7 dwords starting at ho / 4 (a 4-way select each), then a byte funnel by ho % 4
    const uint32_t j0 = ho >> 2, s = ho & 3u;
    uint32_t V[7];
#pragma unroll
    for (int m = 0; m < 7; ++m)
        V[m] = j0 == 0u ? W[m] : (j0 == 1u ? W[m + 1] : (j0 == 2u ? W[m + 2] : W[m + 3]));
#pragma unroll
    for (int k = 0; k < 6; ++k) H[k] = __builtin_amdgcn_alignbyte(V[k + 1], V[k], s);
}

// Where a received datagram sits: a descriptor (cts_media_stream_verify), or slot i of a uniformly
// strided receive ring with its completed length in lens[i] (STRIDED: cts_media_stream_verify_strided,
// 4 B of metadata per datagram instead of a 24-B descriptor).
struct MsSource {
    const cts_buf_desc* descs;  // !STRIDED
    const uint32_t* lens;       // STRIDED
    uint32_t stride;
};

template <bool STRIDED>
__device__ __forceinline__ void ms_datagram(const MsSource& src, uint32_t i, uint64_t& off, uint32_t& len)
{
    if constexpr (STRIDED) {
        off = (uint64_t)i * src.stride;
        len = src.lens[i];
    } else {
        const cts_buf_desc d = src.descs[i];
        off = d.byte_offset;
        len = d.length;
    }
}

// The team leader's staging of its datagram's outputs into slot o (a QuadOut, or a ring slot).
#define CTS_MS_STAGE(o)                                                                                           \
    do {                                                                                                          \
            const uint32_t t = team & 3u;                                                                         \
            if constexpr (STATUS) {                                                                               \
                if (records != nullptr) {                                                                         \
                    /* cts_datagram_status as dwords: seq, completed bytes, flag | kind | pass */ \
                    o.rec[t][0] = data ? (H[0] >> 16) | (H[1] << 16) : 0u;                                        \
                    o.rec[t][1] = data ? (H[1] >> 16) | (H[2] << 16) : 0u;                                        \
                    o.rec[t][2] = completed;                                                                      \
                    o.rec[t][3] = (flag & 0xFFFFu) | (kind << 16) | ((data && first == kNone) ? 1u << 24 : 0u);   \
                }                                                                                                 \
            } else if (records != nullptr) {                                                                      \
                /* cts_datagram_record as dwords: seq = header bytes 2..9 (GetSequenceNumberFromTask); */ \
                /* ctsIOPatternMediaStream.cpp:218-219 read the sender qpc / qpf at bytes 8 and 16 */ \
                o.rec[t][0] = data ? (H[0] >> 16) | (H[1] << 16) : 0u;                                            \
                o.rec[t][1] = data ? (H[1] >> 16) | (H[2] << 16) : 0u;                                            \
                o.rec[t][2] = data ? H[2] : 0u;                                                                   \
                o.rec[t][3] = data ? H[3] : 0u;                                                                   \
                o.rec[t][4] = data ? H[4] : 0u;                                                                   \
                o.rec[t][5] = data ? H[5] : 0u;                                                                   \
                o.rec[t][6] = (flag & 0xFFFFu) | (kind << 16);  /* flag, kind, reserved = 0 */ \
                o.rec[t][7] = completed;                                                                          \
            }                                                                                                     \
            if (!data) {                                                                                          \
                if constexpr (!STATUS)                                                                            \
                quad_stage_result(o, t, 0u, 0u,                                                                   \
                                  result_dw2(0u, 0u, 0u, kind == CTS_DGRAM_BAD_DESC ? CTS_RESULT_FLAG_BAD_DESC    \
                                                                                   : CTS_RESULT_FLAG_NOT_DATA));  \
            } else {                                                                                              \
                const bool pass = first == kNone;                                                                 \
                if constexpr (!STATUS)                                                                            \
                if (results != nullptr)                                                                           \
                    quad_stage_result(o, t, pass ? q.len : first, pass ? 0u : count,                              \
                                      pass ? result_dw2(0u, 0u, 1u, 0u)                                           \
                                           : result_dw2(pattern_byte_dev(first), q.sp[first], 0u, 0u));           \
                qc.add(q.len, pass, count);                                                                       \
            }                                                                                                     \
    } while (0)

// RING: outputs staged in a per-wave ring of RING rounds and written every RING rounds (QuadRing); 0 only with
// FRAMES, which writes no per-datagram outputs.
// STATUS: records points at 16-byte cts_datagram_status entries (results unused).
// FRAMES (cts_media_stream_verify_frames): the client's accounting of the batch, summed on the GPU. The jitter window
// does not move between two render ticks, so CompleteTaskBackToPattern (ctsIOPatternMediaStream.cpp:150-272) over a
// batch is a sum over its clean DATA datagrams: bits received, the bytes of each frame in the window, an error frame
// for each one outside it. Every other datagram is an exception (its lowest index is kept): the client replays such a
// batch datagram by datagram.
constexpr uint32_t kFramesLds = 512;  // window slots summed in LDS per workgroup (larger windows: global atomics)
struct MsFrames {
    int64_t head;         // the window's first sequence number (the jitter queue's head)
    int64_t final_frame;  // m_finalFrame
    uint32_t frames;      // the window's size
    uint32_t finished;    // the stream finished: a zero-byte datagram is no exception
    uint64_t* totals;     // CTS_FRAME_TOTAL_SHARDS x {bits, error frames, datagrams, ~first exception | count << 32}
    uint64_t* frame_bytes;  // [frames]
};

// The header chunks and the payload's edge chunks are loaded ahead of the rounds with the default (L2-allocating)
// policy, as verify_quad_kernel's edges (nontemporal, their lines were often gone from L2 when the rounds asked again).
// ORD (cts_media_stream_verify_status_at): the first-failure slots of the device-resident connections. The leader of
// a team whose datagram is an exception (it fails the stream: anything but clean DATA and ID) reads the descriptor's
// conn_index and lowers the connection's slot to the datagram's stream ordinal; the common path gains no load.
struct MsOrdinals {
    uint32_t* conn_first_fail;
    uint32_t n_conns;
    uint32_t base_index;  // ordinal of datagram 0; base_index + n <= 0xFFFFFFFF (checked by the entry point)
};

template <bool NT, bool STRIDED, int RING, bool STATUS, bool FRAMES, bool ORD>
__device__ __forceinline__ void ms_verify_quad_body(const uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                    MsSource src, uint32_t n, void* __restrict__ records,
                                                    cts_verify_result* __restrict__ results,
                                                    uint64_t* __restrict__ counters, uint32_t per, MsFrames fr,
                                                    MsOrdinals ord)
{
    static_assert(RING > 0 || FRAMES, "per-datagram outputs go through the per-wave ring");
    static_assert(!ORD || (STATUS && !STRIDED), "ordinals: the status form over descriptors");
    constexpr int U = kQuadLoads;
    constexpr int TEAMS = kBlock / kQuadTeam;
    __shared__ uint64_t s_fbytes[FRAMES ? kFramesLds : 1];  // FRAMES: this workgroup's bytes per window slot
    __shared__ uint64_t s_ftot[4];                          // FRAMES: bits, error frames, datagrams, exceptions
    uint64_t f_bits = 0;
    uint32_t f_err = 0, f_data = 0, f_exc = 0, f_inv_first = 0;
    const bool f_lds = FRAMES && fr.frames <= kFramesLds;
    if constexpr (FRAMES) {
        for (uint32_t k = threadIdx.x; k < kFramesLds; k += kBlock) s_fbytes[k] = 0;
        if (threadIdx.x < 4) s_ftot[threadIdx.x] = 0;
        __syncthreads();
    }
    __shared__ uint64_t ctr[TEAMS][kCounterCount];
    using RingSlot = typename std::conditional<STATUS, QuadStatusOut, QuadOut>::type;
    __shared__ QuadRing<RING ? RING : 1, RingSlot> qring[RING ? kBlock / 64 : 1];
    uint32_t rs = 0;  // RING: this wave's next ring slot (wave-uniform)
    const uint32_t lane = threadIdx.x & (kQuadTeam - 1);
    const uint32_t team = threadIdx.x / kQuadTeam;
    // dummy target of an empty span's clamped loads: 16-byte-aligned bytes the launch owns
    const void* dummy = STRIDED ? reinterpret_cast<const void*>(arena)
                                : reinterpret_cast<const void*>(((uintptr_t)src.descs + 15u) & ~(uintptr_t)15u);
    QCounters qc;
    QuadWalk<TEAMS> w(n, per, team);
    uint64_t noff;
    uint32_t nlen;
    ms_datagram<STRIDED>(src, w.i < n ? w.i : n - 1u, noff, nlen);
    while (__any(w.i < w.end)) {
        const uint32_t i = w.i;
        const uint64_t doff = noff;
        const uint32_t completed = nlen;
        const uint32_t inext = w.next();
        ms_datagram<STRIDED>(src, inext < n ? inext : n - 1u, noff, nlen);  // clamped: no load under a branch
        const bool live = i < w.end;
        const bool bad = doff > arena_bytes || arena_bytes - doff < (uint64_t)completed ||
                         (STRIDED && completed > src.stride);
        const bool in = live && !bad;
        const uint8_t* dg = arena + (in ? doff : 0u);
        u32x4 hch = u32x4{0u, 0u, 0u, 0u};
        const uint32_t ho = (uint32_t)((uintptr_t)dg & 15u);
        // header chunks: the 16-byte-aligned chunks holding bytes [0, min(completed, 26)); a
        // chunk is loaded only if it holds one of those bytes (never past the datagram's page)
        const uint32_t hbytes = completed < CTS_UDP_DATA_HEADER_LENGTH ? completed : CTS_UDP_DATA_HEADER_LENGTH;
        if (in && 16u * lane < ho + hbytes) hch = load_chunk_g<false>(reinterpret_cast<const u32x4*>(dg - ho) + lane);
        // speculative DATA payload: [26, completed) at pattern offset 0
        const bool maybe_data = in && completed >= CTS_UDP_DATA_HEADER_LENGTH;
        const QSpan q = quad_span(dg + CTS_UDP_DATA_HEADER_LENGTH, maybe_data ? completed - CTS_UDP_DATA_HEADER_LENGTH : 0u,
                                  0u, dummy);
        const uint32_t ce = quad_edge_chunk(q, lane);
        const u32x4 edge = load_chunk_g<false>(q.p + ce);
        uint32_t acc = quad_scan_interior<U, NT>(q, lane);
        acc |= quad_edge_used(q, lane) ? or4(quad_edge_xor(q, ce, edge)) : 0u;
        // header dwords, valid on team lane 0; bytes past the completed length are never read (the flag needs
        // completed >= 2, the DATA fields completed >= 26)
        uint32_t H[6];
        header_dwords_hdr16(hch, ho, H);
        // header: ctsMediaStreamMessage::ValidateBufferLengthFromTask (ctsMediaStreamProtocol.hpp:284-329)
        uint32_t flag = 0, kind;
        if (bad) {
            kind = CTS_DGRAM_BAD_DESC;
        } else if (completed == 0u) {
            kind = CTS_DGRAM_ZERO;
        } else if (completed < CTS_UDP_FLAG_LENGTH) {
            kind = CTS_DGRAM_SHORT;
        } else {
            flag = H[0] & 0xFFFFu;
            if (flag == CTS_UDP_FLAG_DATA)
                kind = completed < CTS_UDP_DATA_HEADER_LENGTH ? CTS_DGRAM_SHORT : CTS_DGRAM_DATA;
            else if (flag == CTS_UDP_FLAG_ID)
                kind = completed < CTS_UDP_CONNECTION_ID_HEADER_LENGTH ? CTS_DGRAM_SHORT : CTS_DGRAM_ID;
            else
                kind = CTS_DGRAM_UNKNOWN;
        }
        kind = (uint32_t)__shfl((int)kind, 0, kQuadTeam);  // lane 0's verdict, for every lane
        const bool data = kind == CTS_DGRAM_DATA;
        uint32_t first = kNone, count = 0;
        if (__any(acc != 0u && data)) {  // rare: exact re-read (non-DATA teams' differences are discarded)
            if (acc != 0u && data) quad_scan_exact<NT>(q, lane, first, count);
            quad_team_reduce(first, count);
        }
        if constexpr (FRAMES) {
            if (lane == 0u && live) {
                if (data && first == kNone) {
                    // GetSequenceNumberFromTask: header bytes 2..9; found in the window -> bytes to its frame
                    // (ctsIOPatternMediaStream.cpp:195-265)
                    const int64_t seq = (int64_t)((uint64_t)((H[0] >> 16) | (H[1] << 16)) |
                                                  ((uint64_t)((H[1] >> 16) | (H[2] << 16)) << 32));
                    const uint64_t k = (uint64_t)seq - (uint64_t)fr.head;
                    f_bits += (uint64_t)completed * 8u;
                    ++f_data;
                    if (seq > fr.final_frame || seq < fr.head || k >= fr.frames) {
                        ++f_err;
                    } else if (f_lds) {
                        __hip_atomic_fetch_add(&s_fbytes[k], (uint64_t)completed, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else {
                        atomicAdd((unsigned long long*)&fr.frame_bytes[k], (unsigned long long)completed);
                    }
                    qc.add(q.len, true, 0u);
                } else {
                    if (data) qc.add(q.len, false, count);  // a corrupt payload: CorruptedBytes
                    if (!(kind == CTS_DGRAM_ZERO && fr.finished)) {
                        ++f_exc;
                        f_inv_first = f_inv_first > ~i ? f_inv_first : ~i;  // the lowest index: the largest ~i
                    }
                }
            }
            w.i = inext;
            continue;
        }
        if constexpr (RING > 0) {
            if (lane == 0u && live) {
                auto& o_ = qring[team >> 2].slot[rs];
                CTS_MS_STAGE(o_);
                if constexpr (ORD) {
                    if (data ? first != kNone : kind != CTS_DGRAM_ID) {  // rare: the datagram fails its stream
                        const uint32_t conn = src.descs[i].conn_index;
                        if (conn < ord.n_conns) atomicMin(&ord.conn_first_fail[conn], ord.base_index + i);
                    }
                }
            }
            auto& g = qring[team >> 2];
            const uint32_t i0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)i);
            if ((threadIdx.x & 63u) == 0u) g.i0[rs] = i0;
            if (++rs == (uint32_t)RING) {
                quad_ring_flush<RING, STATUS ? 4 : 8, RingSlot>(g, RING, w.end, STATUS ? nullptr : results, records);
                rs = 0;
            }
        }
        w.i = inext;
    }
    if constexpr (RING > 0)
        if (rs)
            quad_ring_flush<RING, STATUS ? 4 : 8, RingSlot>(qring[team >> 2], rs, w.end, STATUS ? nullptr : results,
                                                           records);
    if constexpr (FRAMES) {
        // the team leaders' sums -> the workgroup's (LDS) -> one shard of the launch's totals
        uint64_t* const sh = fr.totals + (size_t)(blockIdx.x % CTS_FRAME_TOTAL_SHARDS) * 4u;
        if (lane == 0u) {
            if (f_bits) __hip_atomic_fetch_add(&s_ftot[0], f_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (f_err) __hip_atomic_fetch_add(&s_ftot[1], (uint64_t)f_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (f_data) __hip_atomic_fetch_add(&s_ftot[2], (uint64_t)f_data, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (f_exc) {  // rare: straight to the shard (u32 ~first exception, then u32 count)
                uint32_t* const w3 = reinterpret_cast<uint32_t*>(&sh[3]);
                atomicMax(&w3[0], f_inv_first);
                atomicAdd(&w3[1], f_exc);
            }
        }
        __syncthreads();
        if (f_lds)
            for (uint32_t k = threadIdx.x; k < fr.frames; k += kBlock)
                if (s_fbytes[k]) atomicAdd((unsigned long long*)&fr.frame_bytes[k], (unsigned long long)s_fbytes[k]);
        if (threadIdx.x < 3 && s_ftot[threadIdx.x])
            atomicAdd((unsigned long long*)&sh[threadIdx.x], (unsigned long long)s_ftot[threadIdx.x]);
    }
    qc.flush<TEAMS>(ctr, team, lane, counters);
}

// The receive pass of cts_media_stream_verify / _status / _frames and their strided forms. Its name and arguments are
// what tests/test_abi.py and the profiling tools look the MediaStream kernels up by, so they stay as they are.
template <bool NT, bool STRIDED, int RING, bool STATUS = false, bool FRAMES = false>
__global__ void __launch_bounds__(kBlock)
    media_stream_verify_quad_kernel(const uint8_t* __restrict__ arena, uint64_t arena_bytes, MsSource src, uint32_t n,
                                    void* __restrict__ records, cts_verify_result* __restrict__ results,
                                    uint64_t* __restrict__ counters, uint32_t per, MsFrames fr = MsFrames{})
{
    ms_verify_quad_body<NT, STRIDED, RING, STATUS, FRAMES, false>(arena, arena_bytes, src, n, records, results,
                                                                  counters, per, fr, MsOrdinals{nullptr, 0u, 0u});
}

// cts_media_stream_verify_status_at: the status form over descriptors, the same body, with the slot claim.
template <bool NT>
__global__ void __launch_bounds__(kBlock)
    ms_verify_status_ordinal(const uint8_t* __restrict__ arena, uint64_t arena_bytes, MsSource src, uint32_t n,
                             void* __restrict__ status, uint64_t* __restrict__ counters, uint32_t per, MsOrdinals ord)
{
    ms_verify_quad_body<NT, false, 64, true, false, true>(arena, arena_bytes, src, n, status, nullptr, counters, per,
                                                          MsFrames{}, ord);
}

static_assert(kGridBlock == (uint32_t)kBlock && kGridQuadTeams == (uint32_t)(kBlock / kQuadTeam),
              "cts_grids.hpp sizes the launches of these kernels");

// The MediaStream receive: four datagrams per wave walking block-contiguous ranges (contig_grid), records + results
// staged in a per-wave LDS ring and written every kMsRing rounds (for config 3 once, at the workgroup's end).
hipError_t launch_media_stream_verify(const uint8_t* arena, uint64_t arena_bytes, const cts_buf_desc* descs, uint32_t n,
                                     cts_datagram_record* records, cts_verify_result* results, uint64_t* counters,
                                     hipStream_t stream, const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    const ContigGrid cg = contig_grid(n, geo);
    const MsSource src{descs, nullptr, 0u};
    with_flags(
        [&](auto NT) {
            media_stream_verify_quad_kernel<NT.value, false, kMsRing><<<cg.grid, kBlock, 0, stream>>>(
                arena, arena_bytes, src, n, records, results, counters, cg.per);
        },
        geo.nontemporal);
    return hipGetLastError();
}

hipError_t launch_media_stream_verify_strided(const uint8_t* arena, uint64_t arena_bytes, uint32_t stride,
                                             const uint32_t* lengths, uint32_t n, cts_datagram_record* records,
                                             cts_verify_result* results, uint64_t* counters, hipStream_t stream,
                                             const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    // the same walk over the ring's slots
    const ContigGrid cg = contig_grid(n, geo);
    const MsSource src{nullptr, lengths, stride};
    with_flags(
        [&](auto NT) {
            media_stream_verify_quad_kernel<NT.value, true, kMsRing><<<cg.grid, kBlock, 0, stream>>>(
                arena, arena_bytes, src, n, records, results, counters, cg.per);
        },
        geo.nontemporal);
    return hipGetLastError();
}

hipError_t launch_media_stream_status(const uint8_t* arena, uint64_t arena_bytes, const cts_buf_desc* descs,
                                     const uint32_t* lengths, uint32_t stride, uint32_t n, cts_datagram_status* status,
                                     uint64_t* counters, hipStream_t stream, const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    // one pass over descriptors, or (descs == nullptr) the strided ring: the receive walk, each wave staging its
    // datagrams' 16-byte statuses in an LDS ring and writing 64 rounds of them at a time -- for config 3 (1024
    // datagrams per workgroup) once, at the workgroup's end. Per 16 M datagrams 4.30-4.31 ms against 4.44 with 32
    // rounds and 4.54 written every round, one box (profiles/r02/ms_status/); a two-pass form (headers -> statuses,
    // then the payload clearing pass on failures) measured 4.25 against 4.08 ms (the header gather's scattered
    // 16-byte reads cost more than the writes it takes out of the payload pass)
    const ContigGrid cg = contig_grid(n, geo);
    const MsSource src{descs, lengths, stride};
    with_flags(
        [&](auto NT, auto STRIDED) {
            media_stream_verify_quad_kernel<NT.value, STRIDED.value, 64, true><<<cg.grid, kBlock, 0, stream>>>(
                arena, arena_bytes, src, n, status, nullptr, counters, cg.per);
        },
        geo.nontemporal, descs == nullptr);
    return hipGetLastError();
}

// cts_media_stream_verify_status_at: launch_media_stream_status's walk over descriptors, with the slot claim
hipError_t launch_media_stream_status_at(const uint8_t* arena, uint64_t arena_bytes, const cts_buf_desc* descs,
                                        uint32_t n, uint32_t base_index, cts_datagram_status* status,
                                        uint64_t* counters, uint32_t* conn_first_fail, uint32_t n_conns,
                                        hipStream_t stream, const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    const ContigGrid cg = contig_grid(n, geo);
    const MsSource src{descs, nullptr, 0u};
    const MsOrdinals ord{conn_first_fail, n_conns, base_index};
    with_flags(
        [&](auto NT) {
            ms_verify_status_ordinal<NT.value><<<cg.grid, kBlock, 0, stream>>>(arena, arena_bytes, src, n, status,
                                                                               counters, cg.per, ord);
        },
        geo.nontemporal);
    return hipGetLastError();
}

hipError_t launch_media_stream_frames(const uint8_t* arena, uint64_t arena_bytes, const cts_buf_desc* descs,
                                     const uint32_t* lengths, uint32_t stride, uint32_t n, const cts_frame_window& win,
                                     uint64_t* totals, uint64_t* frame_bytes, uint64_t* counters, hipStream_t stream,
                                     const LaunchGeometry& geo)
{
    // the sums start from zero on the launch's stream (a batch's totals, not a running sum); frame bytes placed right
    // after the totals (the pattern's layout) are cleared with them in one call
    const size_t tb = (size_t)CTS_FRAME_TOTAL_SHARDS * 4u * sizeof(uint64_t);
    const bool adjacent = frame_bytes == totals + CTS_FRAME_TOTAL_SHARDS * 4u;
    hipError_t err = hipMemsetAsync(totals, 0, tb + (adjacent ? (size_t)win.frames * 8u : 0u), stream);
    if (err == hipSuccess && win.frames != 0 && !adjacent)
        err = hipMemsetAsync(frame_bytes, 0, (size_t)win.frames * 8u, stream);
    if (err != hipSuccess || n == 0) return err;
    // descs == nullptr: the strided-ring form; the variant-3 walk without per-datagram outputs
    const ContigGrid cg = contig_grid(n, geo);
    const MsSource src{descs, lengths, stride};
    const MsFrames fr{win.head_sequence_number, win.final_frame, win.frames, win.finished, totals, frame_bytes};
    with_flags(
        [&](auto NT, auto STRIDED) {
            media_stream_verify_quad_kernel<NT.value, STRIDED.value, 0, false, true><<<cg.grid, kBlock, 0, stream>>>(
                arena, arena_bytes, src, n, nullptr, nullptr, counters, cg.per, fr);
        },
        geo.nontemporal, descs == nullptr);
    return hipGetLastError();
}

}  // namespace cts
