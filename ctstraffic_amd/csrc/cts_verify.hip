// cts_verify.hip — CDNA4 (gfx950) verify kernels of ctsTraffic's data-integrity path, the SYNC mailbox and the
// counter fold.
//
// Reference semantics (microsoft/ctsTraffic):
//   verify   ctsTraffic/ctsIOPattern.cpp:745-775 — RtlCompareMemory(S + expected,
//            buf + bufferOffset, n): matching-prefix length; pass iff == n.
//
// Design: a pure HBM-read stream, no MFMA. A buffer's
// verified span is cut into 16-byte chunks aligned in memory (cts_chunks.hpp).
// Chunk 0 and the last chunk may be partial ("edges") and are
// checked with byte masks by two lanes; the interior chunks are streamed by a
// branch-free fast pass that only ORs (received ^ expected). Only when a team's OR
// is nonzero (rare) does an exact re-scan
// compute the first differing byte and the differing-byte count.
//
// Paths (one kernel per path; nontemporal and plain-load forms of each):
//   verify_wg_kernel                  one 256-lane workgroup per buffer (64 KiB TCP buffers); verify_wg_ordinal is the
//                                     same body with cts_verify_at's base_index argument
//   verify_quad_kernel                four buffers per wave (datagram-sized buffers; descriptors or a strided ring)
//   mailbox_kernel                    SYNC-mode VerifyBuffer without a launch per call (resident grid)
//   counters_fold_kernel              cts_counters_allreduce's fold of a counter block's shards
// The MediaStream receive is in cts_media_stream_recv.hip, the sender side and the MediaStream servers' tick in
// cts_fill.hip, the descriptor-only accounting passes in cts_accounting.hip. Kernels that share a body or a
// function-local __shared__ array (all of verify_wg_*, through block_reduce_mismatch) stay in one unit, and the
// mailbox stays beside them: cut apart, their instructions change (DESIGN.md §File layout).
// Every alternative measured on the way to these (other unroll depths, barrier-free and wave-per-buffer
// workgroups, windowed and rotated walks, staged records, speculative first loads, LDS-DMA, line policies)
// was removed from the source once it lost; DESIGN.md §10 lists them with
// their numbers, and git history (up to round 4, commit fe0efda) holds their code.
#include <hip/hip_runtime.h>

#include "cts_chunks.hpp"
#include "cts_launch.hpp"
#include "cts_quad.hpp"

namespace cts {

// A buffer's verified span [sp, sp + len) as 16-byte chunks of p = sp - lo.
struct Span {
    const u32x4* p;
    const uint8_t* sp;
    uint32_t len;
    uint32_t nchunks;  // chunks covering [lo, lo + len)
    uint32_t q0;       // pattern position of the byte at p (mod 65536)
    uint32_t sh;       // q0 & 1 (byte phase), uniform over the span
    uint32_t lo;       // bytes of chunk 0 before the span
    uint32_t hi_last;  // bytes of the last chunk inside the span (1..16)
    uint32_t expected; // ctsTask::m_expectedPatternOffset
    uint32_t cb0;      // first interior chunk on a 128-byte line boundary (1..8)
};

__device__ __forceinline__ Span make_span(const uint8_t* __restrict__ arena, const cts_buf_desc& d)
{
    Span s;
    s.len = d.length - d.skip_head;
    // pointer arithmetic from the kernel argument keeps the global address
    // space (global_load_dwordx4, not flat_load: flat loads also count in
    // lgkmcnt and force full drains)
    s.sp = arena + d.byte_offset + d.skip_head;
    s.lo = (uint32_t)((uintptr_t)s.sp & 15u);
    s.nchunks = s.len == 0 ? 0u : (uint32_t)(((uint64_t)s.lo + s.len + 15u) >> 4);
    s.hi_last = s.len == 0 ? 0u : (uint32_t)((uint64_t)s.lo + s.len - 16ull * (s.nchunks - 1u));
    s.q0 = (d.expected_pattern_offset - s.lo) & 0xFFFFu;
    s.sh = s.q0 & 1u;
    s.p = reinterpret_cast<const u32x4*>(s.sp - s.lo);
    s.expected = d.expected_pattern_offset;
    // Interior rounds start on a 128-byte line: a wave's 1 KiB load then covers 8
    // lines instead of straddling 9 (chunks [1, cb0) are head chunks, see scan_buffer).
    const uint32_t a = (uint32_t)(((uintptr_t)s.p >> 4) & 7u);  // chunk 0's slot in its line
    s.cb0 = 8u - a;                                             // (a + cb0) % 8 == 0, cb0 in [1, 8]
    return s;
}

__device__ __forceinline__ u32x4 chunk_xor(const Span& s, uint32_t c, u32x4 data)
{
    return data ^ expected_chunk((s.q0 + 16u * c) & 0xFFFFu, s.sh);
}

// Buffer resource over the span's chunks [0, nchunks): 16-byte buffer loads
// address it with ONE lane offset VGPR (+ an SGPR offset per unrolled load)
// instead of a 64-bit address per load, and the hardware range check returns 0
// for any byte past num_records instead of faulting.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_rsrc(const Span& s)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(s.p), (short)0, (int)(s.nchunks * 16u), 0x00020000);
}

// packed base (k*0x10001 + 0x10000) of the chunk at index c
__device__ __forceinline__ uint32_t chunk_base(const Span& s, uint32_t c)
{
    const uint32_t k = ((s.q0 + 16u * c) & 0xFFFFu) >> 1;
    return __umul24(k, 0x10001u) + 0x10000u;
}

// Fast pass over the interior chunks [1, nchunks-1) (all 16 bytes valid): OR
// of (received ^ expected) over this lane's chunks. Straight-line rounds of U
// buffer loads per lane, all issued before the first compare (sched_barrier
// keeps the scheduler from interleaving them with the compares); no load under
// a branch (a load under an exec branch makes hipcc drain vmcnt(0) at every
// join). Full rounds use SGPR offsets; the tail round puts the whole offset in
// the VGPR so the range check (which covers voffset + imm) zero-fills the
// excess lanes, which are then masked out.
template <int TEAM, int U, bool NT, bool EVEN>
__device__ __forceinline__ uint32_t scan_rounds(const Span& s, __amdgpu_buffer_rsrc_t r, uint32_t lane, uint32_t cb,
                                                uint32_t c_end)
{
    uint32_t acc = 0;
    const uint32_t voff = lane * 16u;
    for (; cb + (uint32_t)(TEAM * U) <= c_end; cb += (uint32_t)(TEAM * U)) {
        u32x4 d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) d[u] = buf_load<NT>(r, voff, (cb + (uint32_t)(u * TEAM)) * 16u);
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t B = chunk_base(s, cb + lane);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            acc |= or4(d[u] ^ expected_step<TEAM, U, EVEN>(B, u, s.sh));
            // one chunk's expected words live at a time (else hipcc hoists all
            // U*5 of them ahead of the compares: +40 VGPRs, half the occupancy)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (cb < c_end) {
        u32x4 d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) d[u] = buf_load<NT>(r, (cb + (uint32_t)(u * TEAM) + lane) * 16u, 0u);
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t B = chunk_base(s, cb + lane);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t any = or4(d[u] ^ expected_step<TEAM, U, EVEN>(B, u, s.sh));
            acc |= (cb + (uint32_t)(u * TEAM) + lane < c_end) ? any : 0u;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    return acc;
}

// interior = [cb0, nchunks-1); [1, cb0) are head chunks
template <int TEAM, int U, bool NT, bool EVEN>
__device__ __forceinline__ uint32_t scan_interior_impl(const Span& s, __amdgpu_buffer_rsrc_t r, uint32_t lane)
{
    if (s.nchunks < 3u) return 0;
    return scan_rounds<TEAM, U, NT, EVEN>(s, r, lane, s.cb0, s.nchunks - 1u);
}

// SPLIT: a span-uniform (scalar) branch on the byte phase selects the
// funnel-shift-free even-phase stream.
template <int TEAM, int U, bool NT, bool SPLIT>
__device__ __forceinline__ uint32_t scan_interior(const Span& s, __amdgpu_buffer_rsrc_t r, uint32_t lane)
{
    if constexpr (SPLIT) {
        if (__builtin_amdgcn_readfirstlane(s.sh) == 0u) return scan_interior_impl<TEAM, U, NT, true>(s, r, lane);
    }
    return scan_interior_impl<TEAM, U, NT, false>(s, r, lane);
}

// A span of whole chunks starting on a 128-byte line (lo == 0, hi_last == 16,
// chunk 0 line-aligned: every buffer of a 64 KiB-strided arena or recv ring
// whose completion is a multiple of 16 bytes) has no partial chunk to mask: all
// of [0, nchunks) streams in rounds, with no edge/head load and, for 64 KiB, no
// tail round (4096 chunks = 8 full rounds of 256 lanes x U2; scan_whole_exact).
__device__ __forceinline__ bool span_whole_lines(const Span& s)
{
    return s.lo == 0u && s.hi_last == 16u && s.cb0 == 8u;
}

// Fast pass over a whole span: OR of (received ^ expected) over this lane's
// share. The two edge chunks (first and last, possibly partial) are loaded
// FIRST by every lane (lane 1 the last chunk, the others chunk 0: the same
// lines, no extra traffic), so their latency hides under the interior stream
// instead of adding a dependent round trip per buffer; their byte-masked
// compare runs at the end, branch-free, on registers. For an empty span the
// edge offset is out of the resource's range and reads 0.
// Edge/head chunk of a lane: lane 0 = chunk 0, lane 1 = the last chunk, lanes
// 2..8 = head chunks 1..7 (those below cb0 and the last chunk); other lanes
// re-load chunk 0 (same line, no extra traffic) and discard it.
__device__ __forceinline__ uint32_t edge_chunk_of(const Span& s, uint32_t lane)
{
    return lane == 1u ? s.nchunks - 1u : ((lane >= 2u && lane <= 8u) ? lane - 1u : 0u);
}
__device__ __forceinline__ bool edge_chunk_used(const Span& s, uint32_t lane)
{
    if (s.nchunks == 0u) return false;
    if (lane == 0u) return true;
    if (lane == 1u) return s.nchunks > 1u;
    const uint32_t h = s.nchunks - 1u < s.cb0 ? s.nchunks - 1u : s.cb0;  // head = [1, min(cb0, nchunks-1))
    return lane >= 2u && lane <= 8u && lane - 1u < h;
}

template <int TEAM, int U, bool NT, bool SPLIT = false>
__device__ __forceinline__ uint32_t scan_buffer(const Span& s, uint32_t lane)
{
    const __amdgpu_buffer_rsrc_t r = span_rsrc(s);
    const uint32_t ce = edge_chunk_of(s, lane);
    // lanes without an edge/head chunk address past the resource: the range check
    // returns 0 without a memory request (waves 1..3 of a workgroup fetch nothing)
    const u32x4 edge = buf_load<NT>(r, edge_chunk_used(s, lane) ? ce * 16u : 0x7FFFFFF0u, 0u);
    uint32_t acc = scan_interior<TEAM, U, NT, SPLIT>(s, r, lane);
    const u32x4 x = chunk_xor(s, ce, edge) & range_mask(ce == 0u ? s.lo : 0u, ce == s.nchunks - 1u ? s.hi_last : 16u);
    acc |= edge_chunk_used(s, lane) ? or4(x) : 0u;
    return acc;
}

// Exact diff of one chunk's XOR: first differing byte (span-relative) and count.
__device__ __forceinline__ void take_diff(const Span& s, uint32_t c, u32x4 x, uint32_t& first, uint32_t& count)
{
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t nz = nonzero_bytes(x[w]);
        if (nz) {
            const uint32_t idx = 4u * (uint32_t)w + ((uint32_t)__builtin_ctz(nz) >> 3);
            const uint32_t pos = 16u * c + idx - s.lo;
            first = pos < first ? pos : first;
            count += (uint32_t)__builtin_popcount(nz);
        }
    }
}

// Exact re-scan of exactly the chunks this lane owns in scan_buffer (interior
// chunk c in [cb0, nchunks-1) -> lane (c-cb0) % TEAM; edge/head chunks -> lanes
// 0..8, edge_chunk_of). Only lanes whose fast pass saw a difference call it, so
// a corrupt buffer costs one lane's re-read, not the team's; the loads go out U
// at a time like the fast pass, so the re-read is a few round trips, not one per
// chunk. Yields the lane's first differing byte and differing-byte count.
template <int TEAM, int U, bool NT>
__device__ __forceinline__ void scan_exact_owned(const Span& s, uint32_t lane, uint32_t& first, uint32_t& count)
{
    if (s.nchunks == 0) return;
    const __amdgpu_buffer_rsrc_t r = span_rsrc(s);
    if (s.nchunks >= 3u) {
        const uint32_t c_end = s.nchunks - 1u;
        for (uint32_t cb = s.cb0; cb < c_end; cb += (uint32_t)(TEAM * U)) {
            u32x4 d[U];
#pragma unroll
            for (int u = 0; u < U; ++u) d[u] = buf_load<NT>(r, (cb + (uint32_t)(u * TEAM) + lane) * 16u, 0u);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t c = cb + (uint32_t)(u * TEAM) + lane;
                if (c < c_end) take_diff(s, c, chunk_xor(s, c, d[u]), first, count);
            }
        }
    }
    if (edge_chunk_used(s, lane)) {
        const uint32_t c = edge_chunk_of(s, lane);
        const u32x4 x = chunk_xor(s, c, buf_load<NT>(r, c * 16u, 0u)) &
                        range_mask(c == 0u ? s.lo : 0u, c == s.nchunks - 1u ? s.hi_last : 16u);
        take_diff(s, c, x, first, count);
    }
}

// The whole-span stream with the exact diff done in registers: a lane whose round
// saw a difference computes its first differing byte and differing-byte count from
// the XORs it still holds, so a corrupt buffer costs no re-read. (A re-read is 8
// dependent rounds for a 64 KiB buffer: several microseconds during which the
// workgroup's next buffer waits, and with one corrupt buffer in a thousand that
// workgroup is the launch's last to finish.) The clean-path cost is one compare and
// branch per round.
// One whole round: XOR the U loaded chunks with the expected words, then the exact diff of a round that differs.
template <int TEAM, int U, bool EVEN>
__device__ __forceinline__ void whole_exact_round(const Span& s, u32x4 (&d)[U], uint32_t cb, uint32_t lane,
                                                  uint32_t& first, uint32_t& count)
{
    const uint32_t B = chunk_base(s, cb + lane);
    uint32_t any = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        d[u] ^= expected_step<TEAM, U, EVEN>(B, u, s.sh);
        any |= or4(d[u]);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (any != 0u) {
#pragma unroll
        for (int u = 0; u < U; ++u) take_diff(s, cb + (uint32_t)(u * TEAM) + lane, d[u], first, count);
    }
}

template <int TEAM, int U, bool NT, bool EVEN>
__device__ __forceinline__ void scan_whole_exact_impl(const Span& s, __amdgpu_buffer_rsrc_t r, uint32_t lane,
                                                      uint32_t& first, uint32_t& count)
{
    const uint32_t voff = lane * 16u;
    uint32_t cb = 0;
    const uint32_t c_end = s.nchunks;
    for (; cb + (uint32_t)(TEAM * U) <= c_end; cb += (uint32_t)(TEAM * U)) {
        u32x4 d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) d[u] = buf_load<NT>(r, voff, (cb + (uint32_t)(u * TEAM)) * 16u);
        __builtin_amdgcn_sched_barrier(0);
        whole_exact_round<TEAM, U, EVEN>(s, d, cb, lane, first, count);
    }
    if (cb < c_end) {
        u32x4 d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) d[u] = buf_load<NT>(r, (cb + (uint32_t)(u * TEAM) + lane) * 16u, 0u);
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t B = chunk_base(s, cb + lane);
        uint32_t any = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = cb + (uint32_t)(u * TEAM) + lane < c_end;
            d[u] = in ? (d[u] ^ expected_step<TEAM, U, EVEN>(B, u, s.sh)) : u32x4{0u, 0u, 0u, 0u};
            any |= or4(d[u]);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (any != 0u) {
#pragma unroll
            for (int u = 0; u < U; ++u) take_diff(s, cb + (uint32_t)(u * TEAM) + lane, d[u], first, count);
        }
    }
}

// SPLIT: a span-uniform branch on the byte phase selects the funnel-shift-free even-phase stream
template <int TEAM, int U, bool NT, bool SPLIT>
__device__ __forceinline__ void scan_whole_exact(const Span& s, uint32_t lane, uint32_t& first, uint32_t& count)
{
    const __amdgpu_buffer_rsrc_t r = span_rsrc(s);
    if constexpr (SPLIT) {
        if (__builtin_amdgcn_readfirstlane(s.sh) == 0u) {
            scan_whole_exact_impl<TEAM, U, NT, true>(s, r, lane, first, count);
            return;
        }
    }
    scan_whole_exact_impl<TEAM, U, NT, false>(s, r, lane, first, count);
}

// Spans of 2 GiB or more (a u32 ctsTask length allows 4 GiB - 1; kGiantChunks). The buffer-resource streams above
// address a span with 32-bit byte offsets and a 32-bit num_records (and use 0x7FFFFFF0 as an
// out-of-range offset), so such spans take this plain pass instead: 64-bit pointers, exact from the
// start (first differing byte and count, RtlCompareMemory semantics), TEAM lanes striding the chunks
// G loads at a time (2: the pass must not raise the hot kernels' register count). Positions are span-relative u32 (16c + idx - lo < 2^32 even when 16c wraps).
__device__ __forceinline__ bool span_giant(const Span& s)
{
    return __builtin_amdgcn_readfirstlane(s.nchunks >= kGiantChunks ? 1u : 0u) != 0u;
}

template <int TEAM, bool NT, uint32_t G = 2>
__device__ __forceinline__ void scan_giant_exact(const Span& s, uint32_t lane, uint32_t& first, uint32_t& count)
{
    for (uint32_t cb = 0; cb < s.nchunks; cb += G * TEAM) {
        u32x4 d[G];
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t c = cb + g * TEAM + lane;
            d[g] = load_chunk_g<NT>(s.p + (c < s.nchunks ? c : 0u));
        }
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t c = cb + g * TEAM + lane;
            if (c < s.nchunks) {
                u32x4 x = chunk_xor(s, c, d[g]);
                if (c == 0u || c == s.nchunks - 1u)
                    x &= range_mask(c == 0u ? s.lo : 0u, c == s.nchunks - 1u ? s.hi_last : 16u);
                take_diff(s, c, x, first, count);
            }
        }
    }
}

__device__ __forceinline__ void write_bad(cts_verify_result* results, uint32_t i)
{
    if (results != nullptr) {
        cts_verify_result r;
        r.first_mismatch = 0;
        r.mismatch_bytes = 0;
        r.expected = 0;
        r.actual = 0;
        r.pass = 0;
        r.flags = CTS_RESULT_FLAG_BAD_DESC;
        results[i] = r;
    }
}

// Record one verified buffer (called by the team leader).
// base_index: the stream ordinal of the launch's buffer 0 (cts_verify_at); only the DataError slot takes
// base_index + i, the record stays at the launch-local i.
__device__ __forceinline__ void finish_buffer(const Span& s, const cts_buf_desc& d, uint32_t i, uint32_t first,
                                              uint32_t count, cts_verify_result* results, uint64_t* tc,
                                              uint32_t* conn_first_fail, uint32_t n_conns, uint32_t base_index = 0u)
{
    const bool pass = (first == kNone);
    if (results != nullptr) {
        cts_verify_result r;
        r.first_mismatch = pass ? s.len : first;
        r.mismatch_bytes = pass ? 0u : count;
        r.expected = pass ? 0 : (uint8_t)pattern_byte_dev(s.expected + first);
        r.actual = pass ? 0 : s.sp[first];
        r.pass = pass ? 1 : 0;
        r.flags = 0;
        results[i] = r;
    }
    // the team's running counters live in LDS (tc[kCounterCount]), not in 12 VGPRs across the stream loop
    tc[kBytesChecked] += s.len;
    tc[kBuffersChecked] += 1;
    if (pass) {
        tc[kBytesOk] += s.len;
    } else {
        tc[kBuffersFailed] += 1;
        tc[kMismatchedBytes] += count;
        if (conn_first_fail != nullptr && d.conn_index < n_conns &&
            atomicMin(&conn_first_fail[d.conn_index], base_index + i) == 0xFFFFFFFFu)
            tc[kConnectionsFailed] += 1;
    }
}

// Workgroup-wide reduction of (first, count) when some lane saw a mismatch.
__device__ __forceinline__ void block_reduce_mismatch(uint32_t& first, uint32_t& count)
{
    __shared__ uint32_t red[2 * (kBlock / 64)];
    const uint32_t wave = threadIdx.x / 64;
    first = wave_min(first);
    count = wave_sum(count);
    if ((threadIdx.x & 63) == 0) {
        red[wave] = first;
        red[kBlock / 64 + wave] = count;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) {
            first = red[w] < first ? red[w] : first;
            count += red[kBlock / 64 + w];
        }
    }
    __syncthreads();  // red reused by the next buffer
}

// ---------------------------------------------------------------------------------------------
// One 256-lane workgroup per buffer (64 KiB TCP buffers; grid-strides over the descriptors). The next
// buffer's descriptor is fetched while the current one streams. A whole-line span (every buffer of a
// 64 KiB-strided arena whose completion is a multiple of 16 bytes) streams in rounds of kWgLoads 16-byte
// buffer loads per lane with the exact diff in registers (scan_whole_exact); any other span takes the
// edge-first fast pass (scan_buffer) and, when it differs, an exact re-read by the lanes that saw it. The
// per-buffer verdict is workgroup-uniform (__syncthreads_or); only a corrupt buffer reduces (first, count)
// over the workgroup. Registers are allocated for 4 waves per SIMD, the 4 workgroups per CU the launch runs
// at (LaunchGeometry::blocks_per_cu): no SGPR spills in the per-buffer set-up (41.18-41.27 against 41.42-41.45
// us per config-2 launch for the 8-wave allocation, profiles/r04/h/wpe.jsonl).
constexpr int kWgLoads = 2;  // loads per lane per round: 4 workgroups x 4 waves x 2 = 32 KiB in flight per CU

template <bool NT>
__device__ __forceinline__ void verify_wg_body(const uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                               const cts_buf_desc* __restrict__ descs, uint32_t n,
                                               cts_verify_result* __restrict__ results, uint64_t* __restrict__ counters,
                                               uint32_t* __restrict__ conn_first_fail, uint32_t n_conns,
                                               uint32_t base_index)
{
    __shared__ uint64_t ctr[1][kCounterCount];
    const uint32_t lane = threadIdx.x;
    zero_counters<1>(ctr);
    const uint32_t step = gridDim.x;
    uint32_t i = blockIdx.x;
    cts_buf_desc dn;
    if (i < n) dn = descs[i];
    for (; i < n; i = (uint64_t)i + step < n ? i + step : n) {
        const cts_buf_desc d = dn;
        if ((uint64_t)i + step < n) dn = descs[i + step];
        if (desc_bad(d, arena_bytes)) {
            if (lane == 0) write_bad(results, i);
            continue;
        }
        const Span s = make_span(arena, d);
        uint32_t first = kNone, count = 0;
        bool dirty;
        if (span_giant(s)) {  // >= 2 GiB: 64-bit exact pass
            scan_giant_exact<kBlock, NT>(s, lane, first, count);
            dirty = __builtin_amdgcn_readfirstlane(__syncthreads_or(first != kNone)) != 0;
            if (dirty) block_reduce_mismatch(first, count);
        } else if (__builtin_amdgcn_readfirstlane(span_whole_lines(s) ? 1u : 0u)) {
            // whole-line span, exact diff in registers: only the reduction is left
            scan_whole_exact<kBlock, kWgLoads, NT, true>(s, lane, first, count);
            dirty = __builtin_amdgcn_readfirstlane(__syncthreads_or(first != kNone)) != 0;
            if (dirty) block_reduce_mismatch(first, count);
        } else {
            const uint32_t acc = scan_buffer<kBlock, kWgLoads, NT, true>(s, lane);
            dirty = __builtin_amdgcn_readfirstlane(__syncthreads_or(acc != 0u)) != 0;
            if (dirty) {  // rare: exact re-scan by the dirty lanes + reduction
                if (acc != 0u) scan_exact_owned<kBlock, 2, NT>(s, lane, first, count);
                block_reduce_mismatch(first, count);
            }
        }
        if (lane == 0) finish_buffer(s, d, i, first, count, results, ctr[0], conn_first_fail, n_conns, base_index);
    }
    flush_counters<1>(counters, ctr);
}

// cts_verify: the DataError slots take launch-local indices. Its name and its eight arguments are what the
// profiling tools and tests/test_abi.py look the headline kernel up by, so they stay as they are.
template <bool NT>
__global__ void __launch_bounds__(kBlock, 4)
    verify_wg_kernel(const uint8_t* __restrict__ arena, uint64_t arena_bytes, const cts_buf_desc* __restrict__ descs,
                     uint32_t n, cts_verify_result* __restrict__ results, uint64_t* __restrict__ counters,
                     uint32_t* __restrict__ conn_first_fail, uint32_t n_conns)
{
    verify_wg_body<NT>(arena, arena_bytes, descs, n, results, counters, conn_first_fail, n_conns, 0u);
}

// cts_verify_at with a nonzero base: the same body, the slots take base_index + i (stream ordinals). 15 argument
// dwords, still inside the 16 preloaded SGPRs; base_index is read on the failing branch only.
template <bool NT>
__global__ void __launch_bounds__(kBlock, 4)
    verify_wg_ordinal(const uint8_t* __restrict__ arena, uint64_t arena_bytes, const cts_buf_desc* __restrict__ descs,
                      uint32_t n, cts_verify_result* __restrict__ results, uint64_t* __restrict__ counters,
                      uint32_t* __restrict__ conn_first_fail, uint32_t n_conns, uint32_t base_index)
{
    verify_wg_body<NT>(arena, arena_bytes, descs, n, results, counters, conn_first_fail, n_conns, base_index);
}

// ---------------------------------------------------------------------------------------------
// Four buffers per wave (cts_quad.hpp): datagram-sized buffers from descriptors or a strided ring.
template <bool NT, bool STRIDED>
__global__ void __launch_bounds__(kBlock)
    verify_quad_kernel(const uint8_t* __restrict__ arena, uint64_t arena_bytes, VSource src, uint32_t n,
                       cts_verify_result* __restrict__ results, uint64_t* __restrict__ counters,
                       uint32_t* __restrict__ conn_first_fail, uint32_t n_conns, uint32_t per, uint32_t base_index)
{
    constexpr int TEAMS = kBlock / kQuadTeam;
    __shared__ uint64_t ctr[TEAMS][kCounterCount];
    __shared__ QuadOut qout[kBlock / 64];
    const uint32_t lane = threadIdx.x & (kQuadTeam - 1);
    const uint32_t team = threadIdx.x / kQuadTeam;
    // the dummy target of an empty span's clamped loads: the descriptor array (>= 24 bytes) or, for a
    // strided ring, the arena (>= 16 bytes, 16-aligned), rounded up to 16 bytes
    const void* dummy = STRIDED ? static_cast<const void*>(arena)
                                : reinterpret_cast<const void*>(((uintptr_t)src.descs + 15u) & ~(uintptr_t)15u);
    QCounters qc;
    QuadWalk<TEAMS> w(n, per, team);
    cts_buf_desc dn = vs_desc<STRIDED>(src, w.i < n ? w.i : n - 1u);  // n >= 1 (launch_verify returns early on 0)
    while (__any(w.i < w.end)) {
        const uint32_t i = w.i;
        const cts_buf_desc d = dn;
        const uint32_t inext = w.next();
        dn = vs_desc<STRIDED>(src, inext < n ? inext : n - 1u);  // clamped: no load under a branch
        const bool live = i < w.end;
        const bool ok = live && !desc_bad(d, arena_bytes);
        const QSpan q = quad_span(arena + d.byte_offset + d.skip_head, ok ? d.length - d.skip_head : 0u,
                                  d.expected_pattern_offset, dummy);
        // edge chunks first (their latency hides under the interior rounds)
        const uint32_t ce = quad_edge_chunk(q, lane);
        const u32x4 edge = load_chunk_g<false>(q.p + ce);
        uint32_t acc = quad_scan_interior<kQuadLoads, NT>(q, lane);
        acc |= quad_edge_used(q, lane) ? or4(quad_edge_xor(q, ce, edge)) : 0u;
        uint32_t first = kNone, count = 0;
        if (__any(acc != 0u)) {  // rare: exact re-read of the dirty lanes' own chunks
            if (acc != 0u) quad_scan_exact<NT>(q, lane, first, count);
            quad_team_reduce(first, count);
        }
        if (lane == 0u && live) {
            QuadOut& o = qout[team >> 2];
            if (!ok) {
                quad_stage_result(o, team & 3u, 0u, 0u, result_dw2(0u, 0u, 0u, CTS_RESULT_FLAG_BAD_DESC));
            } else {
                const bool pass = first == kNone;
                if (results != nullptr)
                    quad_stage_result(o, team & 3u, pass ? q.len : first, pass ? 0u : count,
                                      pass ? result_dw2(0u, 0u, 1u, 0u)
                                           : result_dw2(pattern_byte_dev(d.expected_pattern_offset + first),
                                                        q.sp[first], 0u, 0u));
                qc.add(q.len, pass, count);
                if (!pass && conn_first_fail != nullptr && d.conn_index < n_conns &&
                    atomicMin(&conn_first_fail[d.conn_index], base_index + i) == 0xFFFFFFFFu)
                    qc.conns += 1u;  // this connection's first recorded failure (kConnectionsFailed)
            }
        }
        quad_flush_results(qout[team >> 2], i, w.end, results);
        w.i = inext;
    }
    qc.flush<TEAMS>(ctr, team, lane, counters);
}

static_assert(kGridBlock == (uint32_t)kBlock && kGridQuadTeams == (uint32_t)(kBlock / kQuadTeam),
              "cts_grids.hpp sizes the launches of these kernels");

// ---- SYNC mailbox: VerifyBuffer (ctsIOPattern.cpp:745-775) per completion without a launch per call ----
// A resident grid of G groups x kMailGroup workgroups; group g serves its own ring of S job slots.
// Every workgroup of the group sees each job itself (no inter-workgroup hand-off on the critical
// path), splits the job's buffer into 4 KiB pieces (one 16-B system-scope load per lane: the host
// rewrites a reused recv slot between jobs, so nothing may come from a cache), compares them with the
// pattern regenerated in registers, and posts one tagged part record to host memory; the caller folds
// the parts.
//
// Each workgroup is four data waves and one polling wave. Lane 0 of the poller reads the next job's
// slot (one 16-B system-scope load in flight) while the data waves still verify the current one, and
// publishes the job to them through LDS (job, then tag); the data waves fold their results with LDS
// atomics and the last one posts the part record. Pollers never join a barrier, and a publication
// slot is reused (two, by job parity) only after its job was folded. More pollers per workgroup, their
// phases spread over the PCIe round trip, were slower: 2 or 4 polling waves (each on its own copy of
// the slot) gave 9.5 us per 64 KiB verify against 6.3 with one, on the same box (tools/sync_probe) --
// the poll reads compete with the data reads. After kMailHotTicks without a job the poller slows
// down, which keeps idle groups' PCIe reads low (a caller's job goes to the least busy group).
constexpr int kMailAux = 1 | 16;                 // sc0 sc1: system scope
constexpr uint32_t kMailThreads = kBlock + 64;   // four data waves + the polling wave
constexpr uint64_t kMailHotTicks = 5000;         // 50 us (s_memrealtime, 100 MHz)

#if defined(CTS_MAILBOX_TRACE)
// diagnostic builds only (tools/mailbox_bisect.hip): per (job mod 1024, workgroup) the s_memrealtime
// stamps of the publication, the data compared (wave 0), the part record stored, the poll's start, and
// each data wave's compare (4 + wave)
__device__ uint64_t* cts_mail_trace;
#define CTS_MAIL_STAMP(which)                                                                      \
    do {                                                                                           \
        if (cts_mail_trace != nullptr)                                                             \
            cts_mail_trace[((j % 1024u) * kMailGroup + gi) * 8u + (which)] = wall_clock64();       \
    } while (0)
#else
#define CTS_MAIL_STAMP(which) \
    do {                      \
    } while (0)
#endif

// The poller keeps one read of the job slot in flight (two reads half a PCIe round trip apart measured 6.72-6.79 us
// per 64 KiB at one caller against 6.32-6.51 with one, and no gain at 8 / 16 callers: profiles/r03/mailbox_polls_ab/).
__global__ __launch_bounds__(kMailThreads) void mailbox_kernel(const MailSlot* slots, MailPart* parts, uint32_t per_group,
                                                               MailStarts starts, uint64_t idle_ticks,
                                                               uint64_t delay_ticks)
{
    __shared__ uint64_t s_job[2][2];              // published job by parity: ptr_exp, len_seq
    __shared__ uint32_t s_tag[2];                 // its tag, written after the job
    __shared__ uint32_t s_first[2], s_count[2], s_arrive[2];
    __shared__ uint32_t s_done;                   // jobs folded
    const uint32_t g = blockIdx.x / kMailGroup, gi = blockIdx.x % kMailGroup;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t j0 = starts.j[g];
    const MailSlot* const ring = slots + (size_t)g * per_group;
    if (tid == 0) {
        s_tag[0] = s_tag[1] = (uint32_t)j0;  // j0's tag is j0 + 1: neither parity starts published
        s_first[0] = s_first[1] = kNone;
        s_count[0] = s_count[1] = s_arrive[0] = s_arrive[1] = 0;
        s_done = 0;
    }
    __syncthreads();  // the kernel's only barrier
    // LDS words shared with waves that never meet at a barrier: relaxed workgroup-scope atomics (ds_read /
    // ds_write), ordered by lds_order() -- one wave's LDS operations execute in issue order, so only the
    // compiler has to be kept from reordering them (no fence: a fence would wait for outstanding loads)
#define LDS_LD(x) __hip_atomic_load(&(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define LDS_ST(x, v) __hip_atomic_store(&(x), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
    const auto lds_order = [] { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };

    if (wave == kBlock / 64) {  // ---- the poller ----
        if (lane != 0) return;
        if (delay_ticks != 0 && g == 0 && gi == kMailGroup - 1) {  // test hook (CTS_MAILBOX_DELAY_MS): a late poller
            const uint64_t t0 = wall_clock64();
            while (wall_clock64() - t0 < delay_ticks) __builtin_amdgcn_s_sleep(127);
        }
        for (uint32_t i = 0;; ++i) {
            const uint64_t j = j0 + i;
            const uint32_t tag = (uint32_t)(j + 1), par = i & 1u;
            while (LDS_LD(s_done) + 1u < i) __builtin_amdgcn_s_sleep(1);  // job i-2 folded: its parity is free
            const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<MailSlot*>(ring + (uint32_t)(j % per_group)), (short)0, 16, 0x00020000);
            const uint64_t start = wall_clock64();
            CTS_MAIL_STAMP(3);
            u32x4 v;
            // this slot's job arrived (or a later one holds it); idle: no job within idle_ticks
            const auto seen = [&](const u32x4& x) { return x[3] == tag || (int32_t)(x[3] - tag) > 0; };
            const auto idle = [&](bool& leave) {
                const uint64_t waited = wall_clock64() - start;
                leave = waited > idle_ticks;
                if (waited > kMailHotTicks) __builtin_amdgcn_s_sleep(40);
            };
            bool leave = false;
            for (;;) {
                v = __builtin_amdgcn_raw_buffer_load_b128(r, 0u, 0u, kMailAux);
                if (seen(v)) break;
                idle(leave);
                if (leave) break;
                __builtin_amdgcn_s_sleep(2);
            }
            if (leave) {
                v = u32x4{0u, 0u, 0u, ~tag};  // no job within idle_ticks: publish one whose tag word is not the tag
            } else if (v[3] != tag) {
                // a later job already holds this slot: the host reuses a slot only once every part record of its
                // job was folded (or at once for a no-op), so job j needed nothing from this workgroup; take it as a
                // no-op and catch up (a workgroup that fell per_group jobs behind would otherwise wait for a tag
                // that never comes back)
                v = u32x4{0u, 0u, kMailSkip, tag};
            }
            LDS_ST(s_job[par][0], (uint64_t)v[0] | ((uint64_t)v[1] << 32));
            LDS_ST(s_job[par][1], (uint64_t)v[2] | ((uint64_t)v[3] << 32));
            lds_order();
            LDS_ST(s_tag[par], tag);
            CTS_MAIL_STAMP(0);
            if (v[3] != tag || v[2] == 0u) return;  // idle leave or stop
        }
    }

    // ---- data waves ----
    for (uint32_t i = 0;; ++i) {
        const uint64_t j = j0 + i;
        const uint32_t tag = (uint32_t)(j + 1), par = i & 1u;
        while (LDS_LD(s_tag[par]) != tag) __builtin_amdgcn_s_sleep(1);
        lds_order();
        const uint64_t ptr_exp = LDS_LD(s_job[par][0]), len_seq = LDS_LD(s_job[par][1]);
        if ((uint32_t)(len_seq >> 32) != tag) return;  // idle leave
        const uint64_t ptr = ptr_exp & 0xFFFFFFFFFFFFull;
        const uint32_t expected = (uint32_t)(ptr_exp >> 48), len = (uint32_t)len_seq;
        const bool mine = len != kMailSkip && gi < mail_parts(ptr, len);
        const uint32_t d = (uint32_t)ptr & 15u;
        const uint8_t* const base = reinterpret_cast<const uint8_t*>(ptr - d);
        uint32_t first = kNone, count = 0;
        if (mine && len != 0) {
            const uint64_t nchunks = ((uint64_t)d + len + 15u) >> 4;
            const uint32_t pieces = (uint32_t)((nchunks * 16u + kMailPieceBytes - 1) / kMailPieceBytes);
            const uint32_t q_base = (expected + 65536u - d) & 0xFFFFu;  // pattern position of base[0]
            const uint32_t hi_last = ((d + len - 1u) & 15u) + 1u;
            for (uint32_t u0 = gi; u0 < pieces; u0 += 4 * kMailGroup) {
                u32x4 v[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {  // four pieces' loads in flight before any compare
                    const uint32_t u = u0 + jj * kMailGroup;
                    const uint64_t off = (uint64_t)u * kMailPieceBytes;
                    const uint64_t rem = u < pieces ? nchunks * 16u - off : 0u;
                    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
                        const_cast<uint8_t*>(base + (u < pieces ? off : 0u)), (short)0,
                        (int)(rem < kMailPieceBytes ? rem : kMailPieceBytes), 0x00020000);
                    v[jj] = __builtin_amdgcn_raw_buffer_load_b128(r, tid * 16u, 0u, kMailAux);
                }
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const uint64_t c = (uint64_t)(u0 + jj * kMailGroup) * (kMailPieceBytes / 16u) + tid;
                    if (u0 + jj * kMailGroup >= pieces || c >= nchunks) continue;
                    const uint32_t q = (uint32_t)((q_base + c * 16u) & 0xFFFFu);
                    u32x4 x = v[jj] ^ expected_chunk(q, q & 1u);
                    if (c == 0 || c == nchunks - 1) x &= range_mask(c == 0 ? d : 0u, c == nchunks - 1 ? hi_last : 16u);
                    if (or4(x) == 0u) continue;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const uint32_t nz = nonzero_bytes(x[w]);
                        if (nz == 0u) continue;
                        const uint32_t pos = (uint32_t)(c * 16u - d) + 4u * w + ((uint32_t)__builtin_ctz(nz) >> 3);
                        first = pos < first ? pos : first;
                        count += (uint32_t)__builtin_popcount(nz);
                    }
                }
            }
        }
        first = wave_min(first);
        count = wave_sum(count);
        if (tid == 0) CTS_MAIL_STAMP(1);
        if (lane == 0) CTS_MAIL_STAMP(4 + wave);
        if (lane == 0) {
            __hip_atomic_fetch_min(&s_first[par], first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(&s_count[par], count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            lds_order();
            if (__hip_atomic_fetch_add(&s_arrive[par], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) ==
                kBlock / 64 - 1) {  // the last data wave: post the part record, free the parity
                lds_order();
                const uint32_t f = LDS_LD(s_first[par]);
                const uint32_t n = LDS_LD(s_count[par]);
                if (mine) {
                    MailPart* const out = parts + ((size_t)g * per_group + (uint32_t)(j % per_group)) * kMailGroup + gi;
                    uint64_t g0 = 0xFFFFFFFFull | ((uint64_t)tag << 32), g1 = (uint64_t)(tag & 0xFFFFFFu) << 40;
                    if (len != 0) {
                        uint32_t actual = 0;
                        if (f != kNone) {  // the received byte there (ctsIOPattern.cpp:761-772 prints it)
                            const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
                                const_cast<uint8_t*>(base + d + f), (short)0, 1, 0x00020000);
                            actual = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(r, 0u, 0u, kMailAux);
                        }
                        g0 = (uint64_t)f | ((uint64_t)tag << 32);
                        g1 |= (uint64_t)n | ((uint64_t)actual << 32);
                    }
                    __hip_atomic_store(&out->g0, g0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(&out->g1, g1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    CTS_MAIL_STAMP(2);
                }
                LDS_ST(s_first[par], kNone);
                LDS_ST(s_count[par], 0u);
                LDS_ST(s_arrive[par], 0u);
                lds_order();
                LDS_ST(s_done, i + 1u);
            }
        }
        if (len == 0) return;  // stop: acknowledged above
    }
#undef LDS_LD
#undef LDS_ST
}

hipError_t launch_mailbox(const MailSlot* slots, MailPart* parts, uint32_t per_group, const MailStarts& starts,
                          uint32_t groups, uint64_t idle_ticks, hipStream_t stream, uint64_t delay_ticks)
{
    if (slots == nullptr || parts == nullptr || per_group == 0 || groups == 0 || groups > kMailMaxGroups)
        return hipErrorInvalidValue;
    mailbox_kernel<<<groups * kMailGroup, kMailThreads, 0, stream>>>(slots, parts, per_group, starts, idle_ticks,
                                                                     delay_ticks);
    return hipGetLastError();
}

// ---- counter fold (cts_counters_allreduce): one lane per shard, the kCounterCount sums by lanes 0.. ----
static_assert(CTS_COUNTER_SHARDS == 64, "one lane per counter shard");
__global__ void __launch_bounds__(64) counters_fold_kernel(const uint64_t* __restrict__ block, uint64_t* __restrict__ out,
                                                           int accumulate)
{
    __shared__ uint64_t part[CTS_COUNTER_SHARDS][kCounterCount];
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kCounterCount; ++k) part[t][k] = block[t * kCounterSlots + k];
    __syncthreads();
    if (t < (uint32_t)kCounterCount) {
        uint64_t s = accumulate ? out[t] : 0u;
        for (uint32_t sh = 0; sh < CTS_COUNTER_SHARDS; ++sh) s += part[sh][t];
        out[t] = s;
    }
}

hipError_t launch_counters_fold(const void* block, uint64_t* out, bool accumulate, hipStream_t stream)
{
    if (block == nullptr || out == nullptr) return hipErrorInvalidValue;
    counters_fold_kernel<<<1, 64, 0, stream>>>(static_cast<const uint64_t*>(block), out, accumulate ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_verify_at(const uint8_t* arena, uint64_t arena_bytes, const cts_buf_desc* descs, uint32_t n,
                            uint32_t max_length_hint, cts_verify_result* results, uint64_t* counters,
                            uint32_t* conn_first_fail, uint32_t n_conns, uint32_t base_index, hipStream_t stream,
                            const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    const bool small = max_length_hint != 0 && max_length_hint <= (uint32_t)geo.small_threshold;
    with_flags(
        [&](auto NT) {
            if (small) {
                const ContigGrid cg = contig_grid(n, geo);
                verify_quad_kernel<NT.value, false><<<cg.grid, kBlock, 0, stream>>>(
                    arena, arena_bytes, VSource{descs, nullptr, 0u, 0u, 0u, 0u}, n, results, counters, conn_first_fail,
                    n_conns, cg.per, base_index);
            } else if (base_index == 0u) {
                verify_wg_kernel<NT.value><<<grid_for(n, 1, geo), kBlock, 0, stream>>>(
                    arena, arena_bytes, descs, n, results, counters, conn_first_fail, n_conns);
            } else {
                verify_wg_ordinal<NT.value><<<grid_for(n, 1, geo), kBlock, 0, stream>>>(
                    arena, arena_bytes, descs, n, results, counters, conn_first_fail, n_conns, base_index);
            }
        },
        geo.nontemporal);
    return hipGetLastError();
}

hipError_t launch_verify(const uint8_t* arena, uint64_t arena_bytes, const cts_buf_desc* descs, uint32_t n,
                         uint32_t max_length_hint, cts_verify_result* results, uint64_t* counters,
                         uint32_t* conn_first_fail, uint32_t n_conns, hipStream_t stream,
                         const LaunchGeometry& geo)
{
    return launch_verify_at(arena, arena_bytes, descs, n, max_length_hint, results, counters, conn_first_fail, n_conns,
                            0u, stream, geo);
}

// cts_verify_strided: the small-buffer walk (verify_quad_kernel) over a uniformly strided ring
hipError_t launch_verify_strided_at(const uint8_t* arena, uint64_t arena_bytes, uint32_t stride, const uint32_t* lens,
                                    uint32_t n, uint32_t skip_head, uint32_t expected, uint32_t conn_index,
                                    cts_verify_result* results, uint64_t* counters, uint32_t* conn_first_fail,
                                    uint32_t n_conns, uint32_t base_index, hipStream_t stream,
                                    const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    const VSource src{nullptr, lens, stride, skip_head, expected, conn_index};
    const ContigGrid cg = contig_grid(n, geo);
    with_flags(
        [&](auto NT) {
            verify_quad_kernel<NT.value, true><<<cg.grid, kBlock, 0, stream>>>(
                arena, arena_bytes, src, n, results, counters, conn_first_fail, n_conns, cg.per, base_index);
        },
        geo.nontemporal);
    return hipGetLastError();
}

hipError_t launch_verify_strided(const uint8_t* arena, uint64_t arena_bytes, uint32_t stride, const uint32_t* lens,
                                 uint32_t n, uint32_t skip_head, uint32_t expected, uint32_t conn_index,
                                 cts_verify_result* results, uint64_t* counters, uint32_t* conn_first_fail,
                                 uint32_t n_conns, hipStream_t stream, const LaunchGeometry& geo)
{
    return launch_verify_strided_at(arena, arena_bytes, stride, lens, n, skip_head, expected, conn_index, results,
                                    counters, conn_first_fail, n_conns, 0u, stream, geo);
}

}  // namespace cts
