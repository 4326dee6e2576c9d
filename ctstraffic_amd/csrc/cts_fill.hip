// cts_fill.hip — the sender side for gfx950: the write-bound twins of the verify kernels.
//   fill_kernel / fill_pieces_kernel / fill_span_kernel   the pattern into buffers (cts_fill) and one long span
//   fill_batched_kernel / media_stream_fill_ring_kernel   whole MediaStream datagrams: descriptors, or a ring
//   ms_server_fill                    the MediaStream servers' tick: the ring fill with media_stream_fill_ring_kernel's
//                                     store loop (cts_ring_store_loop.hpp) and no per-datagram metadata
//   tcp_sender_descs, tcp_sender_fill_pieces / _small   the TCP senders' tick: a descriptor per written slot, then
//                                     fill_pieces_kernel's or fill_kernel's loop (cts_fill_pieces_loop.hpp,
//                                     cts_fill_team_loop.hpp) over a count read on the device
//   tcp_exchange_descs                the exchange tick (Push, Pull, PushPull, Duplex): a descriptor per written slot
//                                     by closed form from the buffer's index; the fill is the senders'
// The slots of the ticks are planned in cts_tick_plan.hip, which writes no pattern byte.
// The expected chunk is regenerated in registers as in the verify (cts_chunks.hpp); the verify kernels are in
// cts_verify.hip, the MediaStream receive in cts_media_stream_recv.hip. The alternatives that lost are in DESIGN.md §10.
#include <hip/hip_runtime.h>

#include "cts_chunks.hpp"
#include "cts_launch.hpp"
#include "cts_tcp_exchange_math.hpp"

namespace cts {

// ---------------------------------------------------------------------------------------------
// fill: the write-bound twin. Interior chunks are 16-byte stores; the (at most
// two) edge chunks of a span write only their own bytes, so neighbouring buffers
// sharing a 16-byte line are never touched.

// Bytes [b0, b1) of the 16-byte chunk e at dst: whole dwords as dword stores, a partial dword as one
// aligned short and/or one byte store (at most 6 stores; a byte loop took up to 15).
__device__ __forceinline__ void store_chunk_bytes(uint8_t* dst, const u32x4& e, uint32_t b0, uint32_t b1)
{
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) {
        const uint32_t lo = b0 > 4u * w ? b0 - 4u * w : 0u, hi = b1 < 4u * w + 4u ? (b1 > 4u * w ? b1 - 4u * w : 0u) : 4u;
        if (lo >= hi) continue;
        uint8_t* q = dst + 4u * w;
        const uint32_t v = e[w];
        if (lo == 0u && hi == 4u) {
            *reinterpret_cast<uint32_t*>(q) = v;
            continue;
        }
        uint32_t b = lo;
        if ((b & 1u) && b < hi) {  // odd start: one byte
            q[b] = (uint8_t)(v >> (8u * b));
            ++b;
        }
        if (b + 2u <= hi) {  // an aligned pair
            *reinterpret_cast<uint16_t*>(q + b) = (uint16_t)(v >> (8u * b));
            b += 2u;
        }
        if (b < hi) q[b] = (uint8_t)(v >> (8u * b));  // one byte left
    }
}

template <bool NTS = false>
__device__ __forceinline__ void fill_chunk(u32x4* a0, uint32_t c, uint32_t nchunks, uint32_t q0, uint32_t lo,
                                           uint32_t hi_last)
{
    const u32x4 e = expected_chunk((q0 + 16u * c) & 0xFFFFu, q0 & 1u);
    const bool first_c = (c == 0u);
    const bool last_c = (c == nchunks - 1u);
    const uint32_t b0 = first_c ? lo : 0u;
    const uint32_t b1 = last_c ? hi_last : 16u;
    if (b0 == 0u && b1 == 16u) {
        if constexpr (NTS) __builtin_nontemporal_store(e, a0 + c);
        else a0[c] = e;
    } else {
        store_chunk_bytes(reinterpret_cast<uint8_t*>(a0 + c), e, b0, b1);
    }
}

// A span of whole 16-byte chunks (lo == 0, last chunk full): straight-line rounds of
// U 16-byte buffer stores per lane, the expected words stepped like the verify
// stream; the tail round needs no mask (stores past num_records are dropped).
template <int TEAM, int U, bool EVEN, bool NTS>
__device__ __forceinline__ void fill_whole_rounds(u32x4* p, uint32_t nchunks, uint32_t q0, uint32_t lane)
{
    const uint32_t sh = q0 & 1u;
    typedef u32x4 __attribute__((address_space(1)))* gstore_ptr;
    uint32_t cb = 0;
    for (; cb + (uint32_t)(TEAM * U) <= nchunks; cb += (uint32_t)(TEAM * U)) {  // full rounds: global stores
        const uint32_t k = ((q0 + 16u * (cb + lane)) & 0xFFFFu) >> 1;
        const uint32_t B = __umul24(k, 0x10001u) + 0x10000u;
        const gstore_ptr g = (gstore_ptr)(p + cb + lane);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32x4 e = expected_step<TEAM, U, EVEN>(B, u, sh);
            if constexpr (NTS) __builtin_nontemporal_store(e, g + u * TEAM);
            else g[u * TEAM] = e;
        }
    }
    if (cb < nchunks) {  // tail round: buffer stores past num_records are dropped
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(p, (short)0, (int)(nchunks * 16u), 0x00020000);
        const uint32_t k = ((q0 + 16u * (cb + lane)) & 0xFFFFu) >> 1;
        const uint32_t B = __umul24(k, 0x10001u) + 0x10000u;
#pragma unroll
        for (int u = 0; u < U; ++u)
            __builtin_amdgcn_raw_buffer_store_b128(expected_step<TEAM, U, EVEN>(B, u, sh), r,
                                                   (cb + (uint32_t)(u * TEAM) + lane) * 16u, 0u, NTS ? 2 : 0);
    }
}

// NTS: nontemporal stores. Plain stores measured faster for whole 64 KiB buffers (tools/hbm_read_ceiling
// writes: 5.51-5.60 TB/s plain vs 4.98-5.35 nt on the same slab shape), nontemporal for datagrams.
// One buffer's payload (descriptor d: bytes [skip_head, length) at pattern offset expected_pattern_offset) by a team of
// TEAM lanes, FU stores per lane per whole-span round.
template <int TEAM, int FU, bool NTS>
__device__ __forceinline__ void fill_one(uint8_t* arena, uint64_t arena_bytes, const cts_buf_desc& d, uint32_t lane)
{
    if (desc_bad(d, arena_bytes)) return;
    const uint32_t len = d.length - d.skip_head;
    if (len == 0) return;
    uint8_t* sp = arena + d.byte_offset + d.skip_head;
    const uint32_t lo = (uint32_t)((uintptr_t)sp & 15u);
    const uint32_t nchunks = (uint32_t)(((uint64_t)lo + len + 15u) >> 4);
    const uint32_t hi_last = (uint32_t)((uint64_t)lo + len - 16ull * (nchunks - 1u));
    const uint32_t q0 = (d.expected_pattern_offset - lo) & 0xFFFFu;
    u32x4* p = reinterpret_cast<u32x4*>(sp - lo);
    // (whole-chunk spans stream buffer stores: 32-bit offsets, so spans >= 2 GiB take the pointer loop)
    if (__builtin_amdgcn_readfirstlane((lo == 0u && hi_last == 16u && nchunks < kGiantChunks) ? 1u : 0u)) {
        if (__builtin_amdgcn_readfirstlane(q0 & 1u) == 0u) fill_whole_rounds<TEAM, FU, true, NTS>(p, nchunks, q0, lane);
        else fill_whole_rounds<TEAM, FU, false, NTS>(p, nchunks, q0, lane);
        return;
    }
    for (uint32_t c = lane; c < nchunks; c += TEAM) fill_chunk<NTS>(p, c, nchunks, q0, lo, hi_last);
}

template <int TEAM, bool NTS = false>
__global__ void __launch_bounds__(kBlock) fill_kernel(uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                      const cts_buf_desc* __restrict__ descs, uint32_t n)
{
#include "cts_fill_team_loop.hpp"
}

// The workgroup path's fill in piece order. Every buffer is cut into ppb pieces of kFillPiece bytes (the last
// piece of a buffer also takes whatever lies past ppb pieces, so any length is filled whatever the hint said);
// pieces are numbered buffer-major and dealt to the workgroups round robin, so at any moment the grid's stores
// cover adjacent pieces -- adjacent buffers of an arena that holds them in order -- rather than one 64 KiB slab per
// workgroup spread over the arena. Rotated over 4 GiB of arenas at one workgroup per CU, plain 16-B stores of the
// pattern write 6.4-6.5 TB/s in this order against 5.5-5.6 in the slab order (tools/write_ceiling_rot.hip,
// profiles/r06/). One workgroup per CU leaves nothing to hide a wave's scalar work between its stores, so the
// pieces of a batch are decoded together: lane m of every wave loads piece m's descriptor and works out its span
// (checks, alignment, chunk range, pattern phase) in vector registers, the next batch's load is issued before this
// batch's stores, and each piece then costs a few readlanes and its stores. (Decoded piece by piece on the scalar
// unit, the same order wrote 3.9 TB/s at one workgroup per CU.)
constexpr uint32_t kFillPiece = 8192;
constexpr int kPieceBatch = 16;

struct PieceJob {   // one piece, decoded by its lane of the batch
    uint64_t base;  // 16-B-aligned address of the span's chunk 0
    uint32_t q0;    // pattern position of chunk 0's first byte
    uint32_t cb, ce;  // chunk range of the piece
    uint32_t nchunks, lo, hi_last;
    uint32_t kind;  // 0 nothing to write, 1 whole 16-B chunks, 2 edge chunks in the range
};

template <uint32_t PIECE>
__device__ __forceinline__ PieceJob decode_piece(uint8_t* arena, uint64_t arena_bytes, const cts_buf_desc* descs,
                                                 uint64_t v, uint64_t total, uint32_t ppb, bool mine)
{
    constexpr uint32_t kChunks = PIECE / 16;
    PieceJob j{};
    if (!mine || v >= total) return j;
    const uint32_t i = (uint32_t)(v / ppb), pc = (uint32_t)(v - (uint64_t)i * ppb);
    const cts_buf_desc d = descs[i];
    if (desc_bad(d, arena_bytes) || d.length == d.skip_head) return j;
    const uint32_t len = d.length - d.skip_head;
    const uint64_t sp = (uint64_t)(uintptr_t)arena + d.byte_offset + d.skip_head;
    j.lo = (uint32_t)(sp & 15u);
    j.nchunks = (uint32_t)(((uint64_t)j.lo + len + 15u) >> 4);
    j.hi_last = (uint32_t)((uint64_t)j.lo + len - 16ull * (j.nchunks - 1u));
    j.q0 = (d.expected_pattern_offset - j.lo) & 0xFFFFu;
    j.base = sp - j.lo;
    const uint64_t cb = (uint64_t)pc * kChunks;
    if (cb >= j.nchunks) return j;
    j.cb = (uint32_t)cb;
    j.ce = pc + 1u == ppb ? j.nchunks : (uint32_t)(cb + kChunks < j.nchunks ? cb + kChunks : j.nchunks);
    j.kind = (j.lo == 0u && j.hi_last == 16u) ? 1u : 2u;
    return j;
}

__device__ __forceinline__ uint32_t lane_u32(uint32_t x, int m) { return (uint32_t)__builtin_amdgcn_readlane((int)x, m); }

// (PIECE and BATCH other than the defaults: tools/write_ceiling_rot.hip's sweep only)
template <bool NTS, uint32_t PIECE = kFillPiece, int BATCH = kPieceBatch>
__global__ void __launch_bounds__(kBlock) fill_pieces_kernel(uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                             const cts_buf_desc* __restrict__ descs, uint32_t n,
                                                             uint32_t ppb)
{
#include "cts_fill_pieces_loop.hpp"
}

// One long span, all workgroups cooperating (sender buffer materialisation).
__global__ void __launch_bounds__(kBlock) fill_span_kernel(uint8_t* __restrict__ dst, uint64_t bytes, uint32_t e)
{
    const uint32_t lo = (uint32_t)((uintptr_t)dst & 15u);
    const uint32_t nchunks = (uint32_t)((lo + bytes + 15u) >> 4);
    const uint32_t hi_last = (uint32_t)(lo + bytes - 16ull * (nchunks - 1u));
    const uint32_t q0 = (e - lo) & 0xFFFFu;
    u32x4* p = reinterpret_cast<u32x4*>(dst - lo);
    for (uint32_t c = blockIdx.x * kBlock + threadIdx.x; c < nchunks; c += gridDim.x * kBlock)
        fill_chunk(p, c, nchunks, q0, lo, hi_last);
}

// ---------------------------------------------------------------------------------------------
// MediaStream send: header {u16 0, i64 seq, i64 qpc, i64 qpf} + P[0 .. length-26) per datagram
// (ctsMediaStreamSendRequests' WSABUF array, ctsMediaStreamProtocol.hpp:230-243).
// A datagram starting on a 16-byte boundary (every slot of a receive-ring-shaped arena, 1472 = 92 x 16) is written
// as whole 16-byte chunks: chunk c holds datagram bytes [16c, 16c + 16), i.e. pattern positions 16c - 26 on, with
// the header's 26 bytes assembled in registers into chunks 0 and 1. Only a partial last chunk writes bytes. (The
// header written bytewise by 26 lanes beside nontemporal payload chunks and 6 byte stores for payload bytes 26..31
// left the first line of every datagram written in pieces: 8.4 -> 7.0 ms for 16 M x 1472 B, tools/rounds/r04/media_stream_probe.py.)
// What still bounds this kernel is latency, not bytes: each datagram's descriptor and header are loaded before its
// stores, one datagram per wave at a time (a one-datagram prefetch was slower: 9.3 ms, tools/ring_fill_probe.hip).
// A ring of datagrams goes through media_stream_fill_ring_kernel instead (cts_media_stream_fill_strided: 4.3 ms).
// One whole datagram (header {0, seq, qpc, qpf} + payload) of descriptor d by one wave.
template <bool NTS>
__device__ __forceinline__ void ms_fill_one(uint8_t* arena, uint64_t arena_bytes, const cts_buf_desc& d, uint64_t seq,
                                            uint64_t qpc, uint64_t qpf, uint32_t lane)
{
    if (d.length < CTS_UDP_DATA_HEADER_LENGTH || d.byte_offset > arena_bytes ||
        arena_bytes - d.byte_offset < (uint64_t)d.length)
        return;
    uint8_t* dg = arena + d.byte_offset;
    if (__builtin_amdgcn_readfirstlane(((uintptr_t)dg & 15u) == 0u ? 1u : 0u)) {
        const uint32_t nchunks = (d.length + 15u) >> 4;
        const uint32_t hi_last = d.length - 16u * (nchunks - 1u);
        u32x4* p = reinterpret_cast<u32x4*>(dg);
        for (uint32_t c = lane; c < nchunks; c += 64u) {
            u32x4 e = expected_chunk((16u * c - CTS_UDP_DATA_HEADER_LENGTH) & 0xFFFFu, 0u);
            if (c == 0u)  // flag 0 | seq | qpc bytes 0..5
                e = u32x4{(uint32_t)(seq << 16), (uint32_t)(seq >> 16), (uint32_t)(seq >> 48) | (uint32_t)(qpc << 16),
                          (uint32_t)(qpc >> 16)};
            else if (c == 1u)  // qpc bytes 6..7 | qpf | payload bytes 0..5
                e = u32x4{(uint32_t)(qpc >> 48) | (uint32_t)(qpf << 16), (uint32_t)(qpf >> 16),
                          (uint32_t)(qpf >> 48) | (e[2] & 0xFFFF0000u), e[3]};
            if (c == nchunks - 1u && hi_last != 16u) {
                store_chunk_bytes(reinterpret_cast<uint8_t*>(p + c), e, 0u, hi_last);
            } else {
                if constexpr (NTS) __builtin_nontemporal_store(e, p + c);
                else p[c] = e;
            }
        }
        return;
    }
    if (lane < CTS_UDP_DATA_HEADER_LENGTH) {
        uint8_t b = 0;
        if (lane >= 2u && lane < 10u) b = (uint8_t)(seq >> (8 * (lane - 2u)));
        else if (lane >= 10u && lane < 18u) b = (uint8_t)(qpc >> (8 * (lane - 10u)));
        else if (lane >= 18u) b = (uint8_t)(qpf >> (8 * (lane - 18u)));
        dg[lane] = b;  // flag bytes 0..1 = c_udpDatagramProtocolHeaderFlagData = 0
    }
    const uint32_t len = d.length - CTS_UDP_DATA_HEADER_LENGTH;
    if (len == 0) return;
    uint8_t* sp = dg + CTS_UDP_DATA_HEADER_LENGTH;
    const uint32_t lo = (uint32_t)((uintptr_t)sp & 15u);
    const uint32_t nchunks = (uint32_t)(((uint64_t)lo + len + 15u) >> 4);
    const uint32_t hi_last = (uint32_t)((uint64_t)lo + len - 16ull * (nchunks - 1u));
    const uint32_t q0 = (0u - lo) & 0xFFFFu;
    u32x4* p = reinterpret_cast<u32x4*>(sp - lo);
    for (uint32_t c = lane; c < nchunks; c += 64u) fill_chunk<NTS>(p, c, nchunks, q0, lo, hi_last);
}

// Whole MediaStream datagrams through descriptors (cts_media_stream_fill), batched: each workgroup walks one
// contiguous range of descriptors in batches of kFillBatch, staged in LDS with their headers, and each wave fills a
// contiguous quarter of the batch, one datagram at a time. Nothing is loaded inside the per-datagram loop: the
// wave-per-datagram form waits for a descriptor (a scalar load of a far-away line: ~1 us) before every datagram's
// stores, which bounded it at 3.4-3.9 TB/s on 16 M x 1472 B (6.8-7.0 ms, tools/rounds/r04/media_stream_probe.py). (The same
// batching measured slower for cts_fill's payload-only small buffers, whose first chunk is a partial write either
// way: 6.9 against 6.1-6.8 ms per 16 M x 1446 B, tools/ring_fill_probe.hip.)
constexpr uint32_t kFillBatch = kBlock;

template <bool NTS>
__global__ void __launch_bounds__(kBlock)
    fill_batched_kernel(uint8_t* __restrict__ arena, uint64_t arena_bytes, const cts_buf_desc* __restrict__ descs,
                        const cts_datagram_header* __restrict__ headers, uint32_t n)
{
    constexpr uint32_t WAVES = kBlock / 64;
    __shared__ cts_buf_desc ds[kFillBatch];
    __shared__ cts_datagram_header hs[kFillBatch];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t per_wg = (uint32_t)(((uint64_t)n + gridDim.x - 1u) / gridDim.x);
    const uint64_t g0 = (uint64_t)blockIdx.x * per_wg;
    const uint64_t g1 = g0 + per_wg < n ? g0 + per_wg : n;
    for (uint64_t d0 = g0; d0 < g1; d0 += kFillBatch) {
        const uint32_t nb = (uint32_t)(g1 - d0 < kFillBatch ? g1 - d0 : kFillBatch);
        __syncthreads();  // every wave is done with the previous batch
        if (threadIdx.x < nb) {
            ds[threadIdx.x] = descs[d0 + threadIdx.x];
            hs[threadIdx.x] = headers[d0 + threadIdx.x];
        }
        __syncthreads();
        const uint32_t q = (nb + WAVES - 1u) / WAVES;
        const uint32_t t1 = (wave + 1u) * q < nb ? (wave + 1u) * q : nb;
        for (uint32_t t = wave * q; t < t1; ++t) {
            const cts_datagram_header h = hs[t];
            ms_fill_one<NTS>(arena, arena_bytes, ds[t], (uint64_t)h.sequence_number, (uint64_t)h.qpc, (uint64_t)h.qpf,
                             lane);
        }
    }
}


// MediaStream sender over a ring (cts_media_stream_fill_strided): datagram i occupies [i * stride, i * stride +
// lengths[i]) of a 16-byte aligned arena, stride a multiple of 16, so the ring is a flat array of 16-byte chunks and
// chunk k is chunk c = k mod (stride / 16) of datagram k / (stride / 16). A datagram with a length below the header,
// above the stride or past the arena is not written; nor are the bytes between a datagram's end and the next slot.
//
// Each workgroup walks one contiguous range of datagrams in batches of kRingBatch: the batch's headers and lengths
// are loaded into LDS (one vector load per thread, then one wait), and its chunks are cut into four contiguous runs,
// one per wave, written 64 consecutive chunks (1 KiB) per round across datagram boundaries. In the loop nothing is
// loaded from memory: a store never waits on a load (vmcnt counts loads and stores in issue order, so a vector load
// in the loop would wait for every store before it; scalar header loads wait for K$ misses at ~1 us each, and every
// SMEM wait is lgkmcnt(0), so they cannot be prefetched). A round of whole datagrams (the common case) writes its
// header chunks through two lane selects and checks nothing per lane. Measured on 16 M x 1472 B
// (tools/ring_fill_probe.hip, profiles/r03/fill_ring/): 4.6-4.9 ms (5.1-5.4 TB/s) at 4 workgroups per CU; scalar
// per-round header loads 4.4-5.8 ms by form; the descriptor fill 5.1-5.4 ms batched, 6.8-9.0 ms wave per datagram; the
// bare pattern as one span 4.0-4.3 ms.
constexpr uint32_t kRingBatch = 512;

struct RingHeader {
    uint64_t seq, qpc, qpf;
};

__device__ __forceinline__ u32x4 datagram_chunk(uint32_t c, const u32x4& pattern, uint64_t seq, uint64_t qpc,
                                                uint64_t qpf)
{
    if (c == 0u)  // flag 0 | seq | qpc bytes 0..5
        return u32x4{(uint32_t)(seq << 16), (uint32_t)(seq >> 16), (uint32_t)(seq >> 48) | (uint32_t)(qpc << 16),
                     (uint32_t)(qpc >> 16)};
    if (c == 1u)  // qpc bytes 6..7 | qpf | payload bytes 0..5
        return u32x4{(uint32_t)(qpc >> 48) | (uint32_t)(qpf << 16), (uint32_t)(qpf >> 16),
                     (uint32_t)(qpf >> 48) | (pattern[2] & 0xFFFF0000u), pattern[3]};
    return pattern;
}

// e with header h in lanes l0 (chunk 0) and l0 + 1 (chunk 1, whose bytes 10..15 are payload: the pattern e already
// holds there). l0 is wave-uniform and may be outside [0, 64) (wrapped), then no lane matches.
__device__ __forceinline__ u32x4 header_lanes(u32x4 e, uint32_t lane, uint32_t l0, const RingHeader& h)
{
    if (lane == l0) {
        e = u32x4{(uint32_t)(h.seq << 16), (uint32_t)(h.seq >> 16), (uint32_t)(h.seq >> 48) | (uint32_t)(h.qpc << 16),
                  (uint32_t)(h.qpc >> 16)};
    } else if (lane == l0 + 1u) {
        e[0] = (uint32_t)(h.qpc >> 48) | (uint32_t)(h.qpf << 16);
        e[1] = (uint32_t)(h.qpf >> 16);
        e[2] = (uint32_t)(h.qpf >> 48) | (e[2] & 0xFFFF0000u);
    }
    return e;
}

// One chunk with every check: chunk c of datagram j (batch slot t) at ring chunk k.
template <bool NTS>
__device__ __forceinline__ void ring_chunk_checked(u32x4* ring, uint64_t k, uint64_t j, uint32_t c, uint32_t len,
                                                   const RingHeader& h, uint32_t stride, uint64_t arena_bytes)
{
    if (len < CTS_UDP_DATA_HEADER_LENGTH || len > stride || 16u * c >= len || j * stride + len > arena_bytes) return;
    const u32x4 e = datagram_chunk(c, expected_chunk((16u * c - CTS_UDP_DATA_HEADER_LENGTH) & 0xFFFFu, 0u), h.seq,
                                   h.qpc, h.qpf);
    if (16u * c + 16u > len) {
        store_chunk_bytes(reinterpret_cast<uint8_t*>(ring + k), e, 0u, len - 16u * c);
    } else {
        if constexpr (NTS) __builtin_nontemporal_store(e, ring + k);
        else ring[k] = e;
    }
}

// SCALAR: stride >= 1024 (the two forms of the store loop, cts_ring_store_loop.hpp). full_slots: slots wholly inside
// the arena (clamped to 2^32-1).
template <bool NTS, bool SCALAR>
__global__ void __launch_bounds__(kBlock)
    media_stream_fill_ring_kernel(uint8_t* __restrict__ arena, uint64_t arena_bytes, uint32_t stride,
                                  const uint32_t* __restrict__ lengths, const cts_datagram_header* __restrict__ headers,
                                  uint32_t n, uint32_t full_slots)
{
    constexpr uint32_t WAVES = kBlock / 64;
    __shared__ RingHeader hs[kRingBatch];
    __shared__ uint32_t ls[kRingBatch];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t cps = stride >> 4;  // chunks per slot
    const uint32_t per_wg = (uint32_t)(((uint64_t)n + gridDim.x - 1u) / gridDim.x);
    const uint64_t g0 = (uint64_t)blockIdx.x * per_wg;
    const uint64_t g1 = g0 + per_wg < n ? g0 + per_wg : n;
    u32x4* const ring = reinterpret_cast<u32x4*>(arena);
    for (uint64_t d0 = g0; d0 < g1; d0 += kRingBatch) {
        const uint32_t nb = (uint32_t)(g1 - d0 < kRingBatch ? g1 - d0 : kRingBatch);
        __syncthreads();  // every wave is done with the previous batch's LDS
        for (uint32_t t = threadIdx.x; t < nb; t += kBlock) {
            const cts_datagram_header h = headers[d0 + t];
            hs[t] = RingHeader{(uint64_t)h.sequence_number, (uint64_t)h.qpc, (uint64_t)h.qpf};
            ls[t] = lengths[d0 + t];
        }
        __syncthreads();
#include "cts_ring_store_loop.hpp"
    }
}

// ---------------------------------------------------------------------------------------------
// MediaStream servers on the device (cts_media_stream_servers_send): the ring fill of a tick that cts_tick_plan.hip
// has planned, with no per-datagram metadata from the host. prefix[i] is listed connection i's first tick-local slot
// (prefix[n] the total), the tick block holds the datagram count, and the entries have been moved.

// The last i in [lo, hi) with prefix[i] <= g; prefix[lo] <= g.
__device__ __forceinline__ uint64_t ms_server_listed(const uint64_t* __restrict__ prefix, uint64_t lo, uint64_t hi,
                                                     uint64_t g)
{
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (prefix[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Datagram j of a frame of F bytes in datagrams of at most M, k = ceil(F / M) of them: cts_media_stream_split's
// lengths in closed form (ctsMediaStreamProtocol.hpp:171-205: a remainder of 1..26 bytes would not hold a header and
// a byte, so the last datagram takes 27 and the one before it gives them up).
__device__ __forceinline__ uint32_t ms_server_length(uint32_t F, uint32_t M, uint32_t k, uint32_t j)
{
    const uint32_t r = F % (M != 0u ? M : 1u);
    const bool tiny = r != 0u && r <= CTS_UDP_DATA_HEADER_LENGTH;
    if (j + 1u == k) return r == 0u ? M : (tiny && k > 1u ? CTS_UDP_DATA_HEADER_LENGTH + 1u : r);
    if (j + 2u == k && tiny) return M - (CTS_UDP_DATA_HEADER_LENGTH + 1u - r);
    return M;
}

// The tick's ring fill: tick-local datagram g goes to slot g of `ring` (the arena from first_slot on). The grid comes
// from the capacity; the total is read here, and workgroups past it leave at once. Each workgroup takes one contiguous
// range of datagrams in batches of kRingBatch, as media_stream_fill_ring_kernel does. It finds the listed connection of
// its first datagram by a binary search of prefix[] and walks forward: every batch loads the kRingBatch + 1 prefixes
// from its first datagram's connection on into LDS, each thread finds its datagram's connection among them (beyond
// them, behind a run of connections that send nothing, in prefix[] itself), and the batch's last datagram leaves its
// connection for the next batch. The batch's lengths and sequence numbers come from the entries by the closed form
// (apply has moved the entry: the frame sent is current_frame - 1); the descriptors and lengths are written here as
// coalesced stores, and the store loop loads nothing.
template <bool NTS, bool SCALAR>
__global__ void __launch_bounds__(kBlock)
    ms_server_fill(uint8_t* __restrict__ ring_base, uint64_t arena_bytes, uint32_t stride, uint64_t first_slot,
                          const uint32_t* __restrict__ ids, uint32_t n,
                          const cts_ms_server_state* __restrict__ servers, const uint64_t* __restrict__ prefix,
                          const cts_ms_server_tick* __restrict__ tick, uint64_t qpc, uint64_t qpf,
                          cts_buf_desc* __restrict__ descs, uint32_t* __restrict__ lengths, uint32_t full_slots,
                          uint32_t capacity, uint32_t n_conns)
{
    constexpr bool TIMED = false;
    const uint64_t* const before = nullptr;  // (the fragment names it in the branch this kernel does not have)
#include "cts_ms_server_fill_body.hpp"
}

// The timed tick's ring fill (cts_media_stream_servers_send_at): the same body over a connection's several frames.
// before[i] is listed connection i's current_frame from before the planning moved its entry.
template <bool NTS, bool SCALAR>
__global__ void __launch_bounds__(kBlock)
    ms_server_timed_fill(uint8_t* __restrict__ ring_base, uint64_t arena_bytes, uint32_t stride, uint64_t first_slot,
                         const uint32_t* __restrict__ ids, uint32_t n,
                         const cts_ms_server_state* __restrict__ servers, const uint64_t* __restrict__ prefix,
                         const uint64_t* __restrict__ before, const cts_ms_server_tick* __restrict__ tick,
                         uint64_t qpc, uint64_t qpf, cts_buf_desc* __restrict__ descs, uint32_t* __restrict__ lengths,
                         uint32_t full_slots, uint32_t capacity, uint32_t n_conns)
{
    constexpr bool TIMED = true;
#include "cts_ms_server_fill_body.hpp"
}

// ---------------------------------------------------------------------------------------------
// TCP senders on the device (cts_tcp_senders_send, cts_tcp_senders_send_paced): what follows a tick's planning
// (cts_tick_plan.hip), with no host descriptor per buffer. tcp_sender_descs writes one descriptor per written slot from
// prefix[], before[] (every listed connection's bytes_sent from before the move) and the tick block; the fill runs over
// those descriptors with the existing loops (cts_fill_pieces_loop.hpp, cts_fill_team_loop.hpp), its buffer count read
// from the tick block.

// One lane per tick-local slot g < total, grid-stride over the capacity: the descriptor of buffer j = g - prefix[i] of
// listed connection i, the last one with prefix[i] <= g (prefix[] stays in L2). A launch of its own: at the fill's one
// workgroup per CU nothing hides a chain of dependent loads in the piece decode, and a thread per connection writing
// its t descriptors would serialise a one-connection tick.
__global__ void __launch_bounds__(kBlock)
    tcp_sender_descs(uint32_t stride, uint64_t first_slot, uint32_t capacity, const uint32_t* __restrict__ ids,
                     uint32_t n, const cts_tcp_sender_state* __restrict__ senders, uint32_t n_conns,
                     const uint64_t* __restrict__ prefix, const uint64_t* __restrict__ before,
                     const cts_tcp_sender_tick* __restrict__ tick, cts_buf_desc* __restrict__ descs)
{
    // (the clamps only matter to a caller who lists a connection twice: nothing is written outside the capacity or
    // read outside the table then either, and no descriptor is longer than its slot)
    const uint32_t total = tick->buffers < capacity ? tick->buffers : capacity;
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < total; g += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = ms_server_listed(prefix, 0u, n, g);
        const uint64_t j = g - prefix[i];
        const uint32_t c = ids[i];
        uint32_t len = 0u, off = 0u;
        if (c < n_conns) {
            const uint32_t B = senders[c].buffer_size;
            const uint64_t was = before[i], start = was + j * B;  // j < capacity: the product stays in 64 bits
            const uint64_t end = senders[c].transfer_bytes;
            const uint64_t left = start < end ? end - start : 0u;
            len = left < (uint64_t)B ? (uint32_t)left : B;
            if (len > stride) len = 0u;
            off = (uint32_t)(start & 0xFFFFu);
        }
        descs[g] = cts_buf_desc{(first_slot + g) * stride, len, off, c, 0u};
    }
}

// The fill over the tick's descriptors: the existing loops, their buffer count read from the tick block (the grid
// comes from the capacity; workgroups past the count find nothing to do).
template <bool NTS>
__global__ void __launch_bounds__(kBlock)
    tcp_sender_fill_pieces(uint8_t* __restrict__ arena, uint64_t arena_bytes, const cts_buf_desc* __restrict__ descs,
                           const cts_tcp_sender_tick* __restrict__ tick, uint32_t capacity, uint32_t ppb)
{
    constexpr uint32_t PIECE = kFillPiece;
    constexpr int BATCH = kPieceBatch;
    const uint32_t n = tick->buffers < capacity ? tick->buffers : capacity;
#include "cts_fill_pieces_loop.hpp"
}

template <bool NTS>
__global__ void __launch_bounds__(kBlock)
    tcp_sender_fill_small(uint8_t* __restrict__ arena, uint64_t arena_bytes, const cts_buf_desc* __restrict__ descs,
                          const cts_tcp_sender_tick* __restrict__ tick, uint32_t capacity)
{
    constexpr int TEAM = 64;
    const uint32_t n = tick->buffers < capacity ? tick->buffers : capacity;
#include "cts_fill_team_loop.hpp"
}

// ---------------------------------------------------------------------------------------------
// The exchange tick (cts_tcp_exchange_send): tcp_sender_descs over 64-byte entries whose buffers go either way.
// before[] holds every listed connection's buffers_sent from before the move, so tick-local slot g is element m =
// before[i] + j of connection ids[i]'s sequence, and its direction, stream position and length are the closed form of
// cts_tcp_exchange_math.hpp: one 64-bit division (by K, PushPull only) per slot, no loop over buffers or segments.
// The receiver of direction d is slot c + d x n_conns (n_conns <= 2^31). The fill that follows is the senders'.
__global__ void __launch_bounds__(kBlock)
    tcp_exchange_descs(uint32_t stride, uint64_t first_slot, uint32_t capacity, const uint32_t* __restrict__ ids,
                       uint32_t n, const cts_tcp_exchange_state* __restrict__ entries, uint32_t n_conns,
                       const uint64_t* __restrict__ prefix, const uint64_t* __restrict__ before,
                       const cts_tcp_exchange_tick* __restrict__ tick, cts_buf_desc* __restrict__ descs)
{
    // (the clamps only matter to a caller who lists a connection twice or passes an entry of its own making: nothing
    // is written outside the capacity or read outside the table then either, and no descriptor is longer than its
    // slot)
    const uint32_t total = tick->tick.buffers < capacity ? tick->tick.buffers : capacity;
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < total; g += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = ms_server_listed(prefix, 0u, n, g);
        const uint64_t j = g - prefix[i];
        const uint32_t c = ids[i];
        uint32_t len = 0u, off = 0u, receiver = c;
        if (c < n_conns) {
            const ExchangeShape S = exchange_shape(entries + c);
            if (exchange_shape_ok(S)) {
                uint32_t d;
                uint64_t pos;
                exchange_element(S, before[i] + j, d, pos, len);
                if (len > stride) len = 0u;
                off = (uint32_t)(pos & 0xFFFFu);
                receiver = c + d * n_conns;
            }
        }
        descs[g] = cts_buf_desc{(first_slot + g) * stride, len, off, receiver, 0u};
    }
}

// ---------------------------------------------------------------------------------------------
static_assert(kGridBlock == (uint32_t)kBlock && kGridFillPiece == kFillPiece && kGridFillBatch == kFillBatch &&
                  kGridRingBatch == kRingBatch,
              "cts_grids.hpp sizes the launches of these kernels");

hipError_t launch_fill(uint8_t* arena, uint64_t arena_bytes, const cts_buf_desc* descs, uint32_t n,
                       uint32_t max_length_hint, hipStream_t stream, const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    const bool small = max_length_hint != 0 && max_length_hint <= (uint32_t)geo.small_threshold;
    // store policy: fill_nt 0 = plain, 1 = nontemporal, 2 = by path (plain for the workgroup path:
    // config 2 48.7 vs 51.1 us; nontemporal for datagrams: 1.46 vs 1.68 ms per 4 M; tools/rounds/r04/tune_verify.py --op fill)
    const bool nts = geo.fill_nt == 2 ? small : geo.fill_nt != 0;
    with_flags(
        [&](auto NTS) {
            if (!small && max_length_hint != 0) {  // the workgroup path in piece order (fill_pieces_kernel)
                const PieceGrid pg = piece_fill_grid(n, max_length_hint, geo.num_cus, geo.fill_blocks_per_cu);
                fill_pieces_kernel<NTS.value><<<pg.grid, kBlock, 0, stream>>>(arena, arena_bytes, descs, n, pg.ppb);
            } else if (small) {
                fill_kernel<64, NTS.value><<<grid_for(n, kBlock / 64, geo), kBlock, 0, stream>>>(arena, arena_bytes,
                                                                                                 descs, n);
            } else {
                fill_kernel<kBlock, NTS.value><<<grid_for(n, 1, geo, geo.fill_blocks_per_cu), kBlock, 0, stream>>>(
                    arena, arena_bytes, descs, n);
            }
        },
        nts);
    return hipGetLastError();
}

hipError_t launch_media_stream_fill(uint8_t* arena, uint64_t arena_bytes, const cts_buf_desc* descs,
                                   const cts_datagram_header* headers, uint32_t n, hipStream_t stream,
                                   const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    // store policy: fill_nt 0 or 2 (by path) = plain, 1 = nontemporal (batched: 5.08 ms plain vs 5.37 nt per 16 M x
    // 1472 B, tools/ring_fill_probe.hip)
    const uint32_t grid = batched_fill_grid(n, geo.num_cus, geo.ring_fill_blocks_per_cu);
    with_flags(
        [&](auto NTS) {
            fill_batched_kernel<NTS.value><<<grid, kBlock, 0, stream>>>(arena, arena_bytes, descs, headers, n);
        },
        geo.fill_nt == 1);
    return hipGetLastError();
}

hipError_t launch_media_stream_fill_strided(uint8_t* arena, uint64_t arena_bytes, uint32_t stride, const uint32_t* lengths,
                                           const cts_datagram_header* headers, uint32_t n, hipStream_t stream,
                                           const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    // (stride <= 1 MiB keeps a batch's chunk count, 512 x stride / 16, in 32 bits; a UDP datagram is < 64 KiB)
    if ((stride & 15u) != 0u || stride < 32u || stride > (1u << 20) || ((uintptr_t)arena & 15u) != 0u)
        return hipErrorInvalidValue;
    // every workgroup gets at least a batch's worth of datagrams, or the whole ring
    const uint32_t grid = ring_fill_grid(n, geo.num_cus, geo.ring_fill_blocks_per_cu);
    const uint64_t slots = arena_bytes / stride;
    const uint32_t full_slots = (uint32_t)(slots < 0xFFFFFFFFull ? slots : 0xFFFFFFFFull);
    with_flags(
        [&](auto NTS, auto SCALAR) {
            media_stream_fill_ring_kernel<NTS.value, SCALAR.value><<<grid, kBlock, 0, stream>>>(
                arena, arena_bytes, stride, lengths, headers, n, full_slots);
        },
        geo.fill_nt != 0, stride >= 1024u);
    return hipGetLastError();
}

// the tick's ring fill: launch_media_stream_fill_strided's grid rule over the capacity (the total is on the device);
// before == nullptr is the plain tick's kernel, otherwise the timed tick's
static hipError_t launch_ms_server_fill_of(uint8_t* arena, uint64_t arena_bytes, uint32_t stride, uint64_t first_slot,
                                           uint32_t capacity, const uint32_t* conn_ids, uint32_t n,
                                           const cts_ms_server_state* servers, uint32_t n_conns,
                                           const uint64_t* prefix, const uint64_t* before,
                                           const cts_ms_server_tick* tick, int64_t qpc, int64_t qpf,
                                           cts_buf_desc* descs, uint32_t* lengths, hipStream_t stream,
                                           const LaunchGeometry& geo)
{
    if (n == 0 || capacity == 0) return hipSuccess;
    if ((stride & 15u) != 0u || stride < 32u || stride > (1u << 20) || ((uintptr_t)arena & 15u) != 0u ||
        first_slot > arena_bytes / stride)
        return hipErrorInvalidValue;
    const uint32_t grid = ring_fill_grid(capacity, geo.num_cus, geo.ring_fill_blocks_per_cu);
    // the ring the kernel sees starts at first_slot: its slot g is the tick's datagram g
    uint8_t* const ring = arena + first_slot * stride;
    const uint64_t ring_bytes = arena_bytes - first_slot * stride;
    const uint64_t slots = ring_bytes / stride;
    const uint32_t full_slots = (uint32_t)(slots < 0xFFFFFFFFull ? slots : 0xFFFFFFFFull);
    with_flags(
        [&](auto NTS, auto SCALAR) {
            if (before == nullptr)
                ms_server_fill<NTS.value, SCALAR.value><<<grid, kBlock, 0, stream>>>(
                    ring, ring_bytes, stride, first_slot, conn_ids, n, servers, prefix, tick, (uint64_t)qpc,
                    (uint64_t)qpf, descs, lengths, full_slots, capacity, n_conns);
            else
                ms_server_timed_fill<NTS.value, SCALAR.value><<<grid, kBlock, 0, stream>>>(
                    ring, ring_bytes, stride, first_slot, conn_ids, n, servers, prefix, before, tick, (uint64_t)qpc,
                    (uint64_t)qpf, descs, lengths, full_slots, capacity, n_conns);
        },
        geo.fill_nt != 0, stride >= 1024u);
    return hipGetLastError();
}

hipError_t launch_ms_server_fill(uint8_t* arena, uint64_t arena_bytes, uint32_t stride, uint64_t first_slot,
                                 uint32_t capacity, const uint32_t* conn_ids, uint32_t n,
                                 const cts_ms_server_state* servers, uint32_t n_conns, const uint64_t* prefix,
                                 const cts_ms_server_tick* tick, int64_t qpc, int64_t qpf, cts_buf_desc* descs,
                                 uint32_t* lengths, hipStream_t stream, const LaunchGeometry& geo)
{
    return launch_ms_server_fill_of(arena, arena_bytes, stride, first_slot, capacity, conn_ids, n, servers, n_conns,
                                    prefix, nullptr, tick, qpc, qpf, descs, lengths, stream, geo);
}

hipError_t launch_ms_server_timed_fill(uint8_t* arena, uint64_t arena_bytes, uint32_t stride, uint64_t first_slot,
                                       uint32_t capacity, const uint32_t* conn_ids, uint32_t n,
                                       const cts_ms_server_state* servers, uint32_t n_conns, const uint64_t* prefix,
                                       const uint64_t* before, const cts_ms_server_tick* tick, int64_t qpc, int64_t qpf,
                                       cts_buf_desc* descs, uint32_t* lengths, hipStream_t stream,
                                       const LaunchGeometry& geo)
{
    if (before == nullptr) return hipErrorInvalidValue;
    return launch_ms_server_fill_of(arena, arena_bytes, stride, first_slot, capacity, conn_ids, n, servers, n_conns,
                                    prefix, before, tick, qpc, qpf, descs, lengths, stream, geo);
}

// the tick's descriptors: one lane per slot of the capacity, at most the verify path's grid (the total is on the device)
hipError_t launch_tcp_sender_descs(uint32_t stride, uint64_t first_slot, uint32_t capacity, const uint32_t* conn_ids,
                                   uint32_t n, const cts_tcp_sender_state* senders, uint32_t n_conns,
                                   const uint64_t* prefix, const uint64_t* before, const cts_tcp_sender_tick* tick,
                                   cts_buf_desc* descs, hipStream_t stream, const LaunchGeometry& geo)
{
    if (n == 0 || capacity == 0) return hipSuccess;
    const uint32_t grid = grid_for((uint32_t)(((uint64_t)capacity + kBlock - 1) / kBlock), 1, geo);
    tcp_sender_descs<<<grid, kBlock, 0, stream>>>(stride, first_slot, capacity, conn_ids, n, senders, n_conns,
                                                  prefix, before, tick, descs);
    return hipGetLastError();
}

// the exchange tick's descriptors: launch_tcp_sender_descs' grid
hipError_t launch_tcp_exchange_descs(uint32_t stride, uint64_t first_slot, uint32_t capacity, const uint32_t* conn_ids,
                                     uint32_t n, const cts_tcp_exchange_state* entries, uint32_t n_conns,
                                     const uint64_t* prefix, const uint64_t* before, const cts_tcp_exchange_tick* tick,
                                     cts_buf_desc* descs, hipStream_t stream, const LaunchGeometry& geo)
{
    if (n == 0 || capacity == 0) return hipSuccess;
    const uint32_t grid = grid_for((uint32_t)(((uint64_t)capacity + kBlock - 1) / kBlock), 1, geo);
    tcp_exchange_descs<<<grid, kBlock, 0, stream>>>(stride, first_slot, capacity, conn_ids, n, entries, n_conns,
                                                    prefix, before, tick, descs);
    return hipGetLastError();
}

// the tick's fill: launch_fill's grids, kernels' loops and store policy with `capacity` buffers and the stride as the
// length hint (the buffer count is on the device)
hipError_t launch_tcp_sender_fill(uint8_t* arena, uint64_t arena_bytes, uint32_t stride, uint32_t capacity,
                                  const cts_buf_desc* descs, const cts_tcp_sender_tick* tick, hipStream_t stream,
                                  const LaunchGeometry& geo)
{
    if (capacity == 0) return hipSuccess;
    const bool small = stride <= (uint32_t)geo.small_threshold;
    const bool nts = geo.fill_nt == 2 ? small : geo.fill_nt != 0;
    with_flags(
        [&](auto NTS) {
            if (!small) {
                const PieceGrid pg = piece_fill_grid(capacity, stride, geo.num_cus, geo.fill_blocks_per_cu);
                tcp_sender_fill_pieces<NTS.value><<<pg.grid, kBlock, 0, stream>>>(arena, arena_bytes, descs, tick,
                                                                                 capacity, pg.ppb);
            } else {
                tcp_sender_fill_small<NTS.value><<<grid_for(capacity, kBlock / 64, geo), kBlock, 0, stream>>>(
                    arena, arena_bytes, descs, tick, capacity);
            }
        },
        nts);
    return hipGetLastError();
}

hipError_t launch_fill_span(uint8_t* dst, uint64_t bytes, uint32_t pattern_offset, hipStream_t stream,
                            const LaunchGeometry& geo)
{
    if (bytes == 0) return hipSuccess;
    const uint64_t chunks = (bytes + 30) / 16 + 1;
    const uint32_t grid = grid_for((uint32_t)((chunks + kBlock - 1) / kBlock), 1, geo);
    fill_span_kernel<<<grid, kBlock, 0, stream>>>(dst, bytes, pattern_offset & 0xFFFFu);
    return hipGetLastError();
}

}  // namespace cts
