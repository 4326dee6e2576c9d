// write_ceiling_rot.hip — the HBM write ceiling on a rotated footprint, beside the product fill kernel.
//
// Every launch writes a different 256 MiB arena of a 4 GiB set (16 arenas, far past the 256 MB Infinity
// Cache, so no launch rewrites lines the MALL still holds), with the ctsTraffic pattern's u16 ramp as data.
// Shapes (all plain stores):
//   dword_slab   : the guide's store shape (MI355X_MICROARCH.md, "plain stores of the same shape": one dword per
//                  lane, 256 B per wave-instruction), each workgroup writing whole contiguous 64 KiB slabs;
//                  8 waves per CU = 2 workgroups of 256 per CU; also at 4 and 16 waves per CU
//   dword_flat   : the same stores, grid-strided over the arena (consecutive waves on adjacent 256 B)
//   b16_slab     : 16 B per lane (1 KiB per wave-instruction), whole 64 KiB slabs, 4/8/16 waves per CU
//   product_fill : cts::fill_kernel<256> (cts_fill.hip, included verbatim) on config 2's 4096 descriptors, at
//                  the product's grid (1 workgroup of 4 waves per CU) and at 2 and 4 per CU
//   b16_flat     : 16-B stores grid-strided (second pass)
//   fill_pieces  : the candidate fill order, buffers cut in 4/8/16 KiB pieces dealt round robin (second pass)
//   SWEEP=2      : the batched piece order beside the product's fill_pieces_kernel, with the stores waited for
//                  every 1-8 pieces or never (profiles/r06/l/)
// Each (shape, waves) is timed over 32 launches (HIP events), the whole sweep three times, interleaved; one JSON
// line per measurement. Diagnostic only (profiles/r06/a/write_ceiling_rotated.jsonl: SWEEP=0; SWEEP=1 the second).
#include "../ctstraffic_amd/csrc/cts_fill.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

using cts::u32x4;
constexpr uint64_t kArena = 256ull << 20;
constexpr int kArenas = 16;
constexpr int kIters = 32;

// u16 ramp of the pattern: dword w of a 64 KiB slab holds u16 values 2w, 2w+1 (mod 32768, as the sender buffer)
__device__ __forceinline__ uint32_t ramp_dword(uint32_t w)
{
    const uint32_t k = (2u * w) & 0x7FFFu;
    return k | ((k + 1u) << 16);
}

template <int U>
__global__ void __launch_bounds__(256) dword_slab_kernel(uint32_t* __restrict__ p, uint64_t bytes)
{
    typedef uint32_t __attribute__((address_space(1)))* gptr;
    const uint64_t nslabs = bytes >> 16;
    for (uint64_t sl = blockIdx.x; sl < nslabs; sl += gridDim.x) {
        const gptr q = (gptr)(p + (sl << 14));
        for (uint32_t r = 0; r < 16384u; r += 256u * U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t w = r + (uint32_t)u * 256u + threadIdx.x;
                q[w] = ramp_dword(w);
            }
        }
    }
}

template <int U>
__global__ void __launch_bounds__(256) dword_flat_kernel(uint32_t* __restrict__ p, uint64_t bytes)
{
    typedef uint32_t __attribute__((address_space(1)))* gptr;
    const uint64_t words = bytes >> 2;
    const uint64_t per_round = (uint64_t)gridDim.x * 256u * U;
    for (uint64_t base = (uint64_t)blockIdx.x * 256u * U; base < words; base += per_round) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t w = base + (uint64_t)u * 256u + threadIdx.x;
            ((gptr)p)[w] = ramp_dword((uint32_t)w);
        }
    }
}

template <int U>
__global__ void __launch_bounds__(256) b16_slab_kernel(u32x4* __restrict__ p, uint64_t bytes)
{
    typedef u32x4 __attribute__((address_space(1)))* gptr;
    const uint64_t nslabs = bytes >> 16;
    for (uint64_t sl = blockIdx.x; sl < nslabs; sl += gridDim.x) {
        const gptr q = (gptr)(p + (sl << 12));
        for (uint32_t r = 0; r < 4096u; r += 256u * U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t c = r + (uint32_t)u * 256u + threadIdx.x;
                q[c] = u32x4{ramp_dword(4u * c), ramp_dword(4u * c + 1u), ramp_dword(4u * c + 2u),
                             ramp_dword(4u * c + 3u)};
            }
        }
    }
}

template <int U>
__global__ void __launch_bounds__(256) b16_flat_kernel(u32x4* __restrict__ p, uint64_t bytes)
{
    typedef u32x4 __attribute__((address_space(1)))* gptr;
    const uint64_t chunks = bytes >> 4;
    const uint64_t per_round = (uint64_t)gridDim.x * 256u * U;
    for (uint64_t base = (uint64_t)blockIdx.x * 256u * U; base < chunks; base += per_round) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t c = base + (uint64_t)u * 256u + threadIdx.x;
            const uint32_t w = 4u * (uint32_t)c;
            ((gptr)p)[c] = u32x4{ramp_dword(w), ramp_dword(w + 1u), ramp_dword(w + 2u), ramp_dword(w + 3u)};
        }
    }
}

// The candidate product order: every buffer cut into pieces of PIECE bytes, pieces numbered buffer-major and dealt
// to the workgroups round robin, so the grid's concurrent stores cover adjacent pieces (of adjacent buffers, when
// the arena holds them in order) instead of one 64 KiB slab per workgroup. 16-B stores of the product's pattern
// words (cts::expected_chunk); whole-line spans only (config 2), ppb = pieces per buffer.
template <int PIECE>
__global__ void __launch_bounds__(256) fill_pieces_kernel(uint8_t* __restrict__ arena, const cts_buf_desc* __restrict__ d,
                                                          uint32_t n, uint32_t ppb)
{
    typedef u32x4 __attribute__((address_space(1)))* gptr;
    constexpr uint32_t kChunks = PIECE / 16, kU = kChunks / 256;
    const uint64_t total = (uint64_t)n * ppb;
    for (uint64_t v = blockIdx.x; v < total; v += gridDim.x) {
        const uint32_t i = (uint32_t)(v / ppb), pc = (uint32_t)(v % ppb);
        const cts_buf_desc dd = d[i];
        const uint32_t nchunks = dd.length >> 4;
        const gptr q = (gptr)(arena + dd.byte_offset);
        const uint32_t q0 = dd.expected_pattern_offset, sh = q0 & 1u;
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) {
            const uint32_t c = pc * kChunks + u * 256u + threadIdx.x;
            if (c < nchunks) q[c] = cts::expected_chunk((q0 + 16u * c) & 0xFFFFu, sh);
        }
    }
}

// fill_pieces with the descriptors of M pieces fetched per batch (lane m loads piece m's, one round trip per batch,
// the next batch's fetched before this batch's stores) and broadcast by readlane: the per-piece dependent
// descriptor load that starved fill_pieces at one workgroup per CU is gone.
template <int PIECE, int M, int DRAIN = 0>
__global__ void __launch_bounds__(256) fill_pieces_batched_kernel(uint8_t* __restrict__ arena,
                                                                  const cts_buf_desc* __restrict__ d, uint32_t n,
                                                                  uint32_t ppb)
{
    typedef u32x4 __attribute__((address_space(1)))* gptr;
    constexpr uint32_t kChunks = PIECE / 16, kU = kChunks / 256;
    const uint64_t total = (uint64_t)n * ppb;
    const uint32_t lane = threadIdx.x;
    const uint64_t G = gridDim.x;
    auto fetch = [&](uint64_t v0) {  // (every wave its own copy: readlane reads the own wave's lanes)
        const uint64_t v = v0 + (uint64_t)(lane & 63u & (M - 1)) * G;
        return d[(uint32_t)((v < total ? v : total - 1) / ppb)];
    };
    cts_buf_desc cur = fetch(blockIdx.x);
    for (uint64_t v0 = blockIdx.x; v0 < total; v0 += (uint64_t)M * G) {
        const cts_buf_desc nxt = fetch(v0 + (uint64_t)M * G < total ? v0 + (uint64_t)M * G : v0);
#pragma unroll 1
        for (int m = 0; m < M; ++m) {
            const uint64_t v = v0 + (uint64_t)m * G;
            if (v >= total) break;
            const uint32_t off_lo = __builtin_amdgcn_readlane((int)(uint32_t)cur.byte_offset, m);
            const uint32_t off_hi = __builtin_amdgcn_readlane((int)(uint32_t)(cur.byte_offset >> 32), m);
            const uint32_t len = __builtin_amdgcn_readlane((int)cur.length, m);
            const uint32_t q0 = __builtin_amdgcn_readlane((int)cur.expected_pattern_offset, m);
            const uint32_t pc = (uint32_t)(v % ppb);
            const gptr q = (gptr)(arena + (((uint64_t)off_hi << 32) | off_lo));
            const uint32_t nchunks = len >> 4, sh = q0 & 1u;
#pragma unroll
            for (uint32_t u = 0; u < kU; ++u) {
                const uint32_t c = pc * kChunks + u * 256u + lane;
                if (c < nchunks) q[c] = cts::expected_chunk((q0 + 16u * c) & 0xFFFFu, sh);
            }
            // DRAIN > 0: every DRAIN pieces, wait for this wave's stores (the batch start drains them anyway)
            if constexpr (DRAIN > 0)
                if ((m + 1) % DRAIN == 0) __builtin_amdgcn_s_waitcnt(0x0F70);
        }
        cur = nxt;
    }
}

// fill_pieces_batched with the batch's pieces unrolled and every store unconditional (whole full batches; the
// rest of the pieces one by one after them): the waitcnt pass can then count the stores issued after the next
// batch's descriptor load and wait for that load alone (vmcnt(N) with N stores still in flight) instead of draining
// them (vmcnt(0)), as it must when a runtime loop or a branch sits between the load and its use.
template <int PIECE, int M>
__global__ void __launch_bounds__(256) fill_pieces_nodrain_kernel(uint8_t* __restrict__ arena,
                                                                  const cts_buf_desc* __restrict__ d, uint32_t n,
                                                                  uint32_t ppb)
{
    typedef u32x4 __attribute__((address_space(1)))* gptr;
    constexpr uint32_t kChunks = PIECE / 16, kU = kChunks / 256;
    const uint64_t total = (uint64_t)n * ppb;
    const uint32_t lane = threadIdx.x;
    const uint64_t G = gridDim.x;
    auto fetch = [&](uint64_t v0) {
        const uint64_t v = v0 + (uint64_t)(lane & 63u & (M - 1)) * G;
        return d[(uint32_t)((v < total ? v : total - 1) / ppb)];
    };
    auto piece = [&](const cts_buf_desc& c, int m, uint64_t v) {
        const uint32_t off_lo = __builtin_amdgcn_readlane((int)(uint32_t)c.byte_offset, m);
        const uint32_t off_hi = __builtin_amdgcn_readlane((int)(uint32_t)(c.byte_offset >> 32), m);
        const uint32_t q0 = __builtin_amdgcn_readlane((int)c.expected_pattern_offset, m);
        const uint32_t pc = (uint32_t)v % ppb;  // (pieces < 2^32 here; a 64-bit remainder branches per piece)
        const gptr q = (gptr)(arena + (((uint64_t)off_hi << 32) | off_lo));
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) {
            const uint32_t ch = pc * kChunks + u * 256u + lane;
            q[ch] = cts::expected_chunk((q0 + 16u * ch) & 0xFFFFu, q0 & 1u);
        }
    };
    uint64_t v0 = blockIdx.x;
    cts_buf_desc cur = fetch(v0);
    // the first batch's load complete before the loop: otherwise the loop header merges "that load pending, nothing
    // after it" with the back edge's "32 stores pending" and waits as for the first, draining the stores every batch
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt and lgkmcnt unconstrained (gfx9 encoding)
    for (; v0 + (uint64_t)(M - 1) * G < total; v0 += (uint64_t)M * G) {
        const cts_buf_desc nxt = fetch(v0 + (uint64_t)M * G < total ? v0 + (uint64_t)M * G : v0);
#pragma unroll
        for (int m = 0; m < M; ++m) piece(cur, m, v0 + (uint64_t)m * G);
        cur = nxt;
    }
    for (int m = 0; m < M && v0 + (uint64_t)m * G < total; ++m) piece(cur, m, v0 + (uint64_t)m * G);
}

// The product's fill_pieces_kernel with the next batch's decode moved off the batch start: the descriptors are
// loaded and waited for at the batch start as in the product (the once-per-batch wait that keeps the waves' stores
// adjacent, profiles/r06/l/), but the ~60 VALU of the decode run after piece 0's stores are issued instead of between
// the wait and the first store. (Probe copy of the product kernel; WAIT = false drops the explicit wait, so the
// compiler places it at the decode.)
template <bool WAIT>
__global__ void __launch_bounds__(256) fill_pieces_deferred_kernel(uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                                   const cts_buf_desc* __restrict__ descs, uint32_t n,
                                                                   uint32_t ppb)
{
    typedef u32x4 __attribute__((address_space(1)))* gstore_ptr;
    constexpr uint32_t kChunks = cts::kFillPiece / 16;
    constexpr int BATCH = cts::kPieceBatch;
    constexpr uint32_t kBlk = 256;
    const uint64_t total = (uint64_t)n * ppb;
    const uint32_t lane = threadIdx.x;
    const uint32_t m_own = lane & 63u;
    const uint64_t G = gridDim.x;
    const bool mine = m_own < (uint32_t)BATCH;
    struct Raw {
        cts_buf_desc d;
        uint64_t v;
    };
    auto load = [&](uint64_t v) {
        Raw r{};
        r.v = v;
        if (mine && v < total) r.d = descs[(uint32_t)(v / ppb)];
        return r;
    };
    auto decode = [&](const Raw& r) {
        cts::PieceJob j{};
        if (!mine || r.v >= total) return j;
        const uint32_t i = (uint32_t)(r.v / ppb), pc = (uint32_t)(r.v - (uint64_t)i * ppb);
        const cts_buf_desc& d = r.d;
        if (cts::desc_bad(d, arena_bytes) || d.length == d.skip_head) return j;
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
    };
    auto piece = [&](const cts::PieceJob& cur, int m) {
        const uint32_t kind = cts::lane_u32(cur.kind, m);
        if (kind == 0u) return;
        const uint64_t base = ((uint64_t)cts::lane_u32((uint32_t)(cur.base >> 32), m) << 32) |
                              cts::lane_u32((uint32_t)cur.base, m);
        const uint32_t q0 = cts::lane_u32(cur.q0, m), cb = cts::lane_u32(cur.cb, m), ce = cts::lane_u32(cur.ce, m);
        if (kind == 1u) {
            const gstore_ptr g = (gstore_ptr)base;
            const uint32_t sh = q0 & 1u;
            if (ce <= cb + kChunks) {
#pragma unroll
                for (uint32_t u = 0; u < kChunks / kBlk; ++u) {
                    const uint32_t c = cb + u * kBlk + lane;
                    if (c < ce) g[c] = cts::expected_chunk((q0 + 16u * c) & 0xFFFFu, sh);
                }
            } else {
                for (uint32_t c = cb + lane; c < ce; c += kBlk) g[c] = cts::expected_chunk((q0 + 16u * c) & 0xFFFFu, sh);
            }
        } else {
            const uint32_t nchunks = cts::lane_u32(cur.nchunks, m), lo = cts::lane_u32(cur.lo, m),
                           hi_last = cts::lane_u32(cur.hi_last, m);
            u32x4* p = reinterpret_cast<u32x4*>((uintptr_t)base);
            for (uint32_t c = cb + lane; c < ce; c += kBlk) cts::fill_chunk<false>(p, c, nchunks, q0, lo, hi_last);
        }
    };
    cts::PieceJob cur = decode(load(blockIdx.x + (uint64_t)m_own * G));
    for (uint64_t v0 = blockIdx.x; v0 < total; v0 += (uint64_t)BATCH * G) {
        const Raw raw = load(v0 + (uint64_t)(BATCH + m_own) * G);
        if constexpr (WAIT) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the product's cadence
        piece(cur, 0);
        const cts::PieceJob nxt = decode(raw);
#pragma unroll 1
        for (int m = 1; m < BATCH; ++m) piece(cur, m);
        cur = nxt;
    }
}

// bytes of p[0, bytes) that differ from the ctsTraffic pattern P(j mod 65536) (every shape writes it)
__global__ void __launch_bounds__(256) count_bad_kernel(const uint8_t* __restrict__ p, uint64_t bytes,
                                                        unsigned long long* bad)
{
    uint32_t c = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < bytes; j += (uint64_t)gridDim.x * 256u)
        c += p[j] != (uint8_t)cts::pattern_byte_dev((uint32_t)j);
    if (c) atomicAdd(bad, (unsigned long long)c);
}

unsigned long long* g_bad = nullptr;
uint8_t* g_check = nullptr;  // the arena the last timed launch writes

template <typename F>
double time_rot_us(F launch)
{
    (void)hipMemset(g_check, 0xA5, kArena);  // not the pattern: a shape that skips bytes leaves them
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    for (int i = 0; i < kArenas; ++i) launch(i);  // untimed: every arena touched once
    (void)hipEventRecord(a);
    for (int i = 0; i < kIters; ++i) launch(i % kArenas);
    (void)hipEventRecord(b);
    (void)hipEventSynchronize(b);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return ms * 1e3 / kIters;
}

void emit(const char* shape, int waves_per_cu, int grid, int rep, double us)
{
    unsigned long long bad = ~0ull;
    if (hipMemset(g_bad, 0, sizeof(*g_bad)) == hipSuccess) {
        count_bad_kernel<<<1024, 256>>>(g_check, kArena, g_bad);
        (void)hipMemcpy(&bad, g_bad, sizeof(bad), hipMemcpyDeviceToHost);
    }
    std::printf("{\"shape\": \"%s\", \"waves_per_cu\": %d, \"grid\": %d, \"rep\": %d, \"bytes\": %llu, "
                "\"footprint_bytes\": %llu, \"us\": %.2f, \"GBps\": %.1f, \"bad_bytes\": %llu}\n",
                shape, waves_per_cu, grid, rep, (unsigned long long)kArena, (unsigned long long)(kArena * kArenas), us,
                (double)kArena / (us * 1e3), bad);
    std::fflush(stdout);
}

}  // namespace

int main()
{
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus <= 0) return 1;
    uint8_t* big = nullptr;
    if (hipMalloc((void**)&big, kArena * kArenas) != hipSuccess) return 1;
    if (hipMalloc((void**)&g_bad, sizeof(*g_bad)) != hipSuccess) return 1;
    g_check = big + (uint64_t)((kIters - 1) % kArenas) * kArena;
    const uint32_t n = (uint32_t)(kArena >> 16);
    std::vector<cts_buf_desc> h(n);
    for (uint32_t i = 0; i < n; ++i) h[i] = cts_buf_desc{(uint64_t)i << 16, 65536u, 0u, i, 0u};
    cts_buf_desc* d = nullptr;
    if (hipMalloc((void**)&d, n * sizeof(cts_buf_desc)) != hipSuccess ||
        hipMemcpy(d, h.data(), n * sizeof(cts_buf_desc), hipMemcpyHostToDevice) != hipSuccess)
        return 1;
    auto arena = [&](int i) { return big + (uint64_t)i * kArena; };
    // SWEEP=1 (default): the round-6 second pass (store width and order at 8 waves per CU, and the piece order of
    // the candidate fill); SWEEP=0: the first pass (slab vs grid-strided at 4/8/16 waves per CU)
    const char* sw = std::getenv("SWEEP");
    const int sweep = sw != nullptr ? std::atoi(sw) : 1;
    for (int rep = 0; rep < 3; ++rep) {
        if (sweep == 0) {
            for (int wpc : {4, 8, 16}) {  // waves per CU: workgroups of 4 waves, wpc / 4 per CU
                const int grid = cus * wpc / 4;
                emit("dword_slab_u8", wpc, grid, rep, time_rot_us([&](int i) {
                         dword_slab_kernel<8><<<grid, 256>>>(reinterpret_cast<uint32_t*>(arena(i)), kArena);
                     }));
                emit("dword_flat_u8", wpc, grid, rep, time_rot_us([&](int i) {
                         dword_flat_kernel<8><<<grid, 256>>>(reinterpret_cast<uint32_t*>(arena(i)), kArena);
                     }));
                emit("b16_slab_u4", wpc, grid, rep, time_rot_us([&](int i) {
                         b16_slab_kernel<4><<<grid, 256>>>(reinterpret_cast<u32x4*>(arena(i)), kArena);
                     }));
                emit("product_fill_kernel", wpc, grid, rep, time_rot_us([&](int i) {
                         cts::fill_kernel<256, false><<<grid, 256>>>(arena(i), kArena, d, n);
                     }));
            }
            continue;
        }
        const int g4 = cus, g8 = cus * 2, g16 = cus * 4;
        emit("product_fill_kernel", 4, g4, rep, time_rot_us([&](int i) {
                 cts::fill_kernel<256, false><<<g4, 256>>>(arena(i), kArena, d, n);
             }));
        emit("dword_flat_u8", 8, g8, rep, time_rot_us([&](int i) {
                 dword_flat_kernel<8><<<g8, 256>>>(reinterpret_cast<uint32_t*>(arena(i)), kArena);
             }));
        emit("dword_flat_u2", 8, g8, rep, time_rot_us([&](int i) {
                 dword_flat_kernel<2><<<g8, 256>>>(reinterpret_cast<uint32_t*>(arena(i)), kArena);
             }));
        if (sweep == 2) {  // the batched-descriptor piece order beside the flat stores it imitates
            for (int wpc : {4, 8, 16}) {
                const int g = cus * wpc / 4;
                emit("b16_flat_u1", wpc, g, rep, time_rot_us([&](int i) {
                         b16_flat_kernel<1><<<g, 256>>>(reinterpret_cast<u32x4*>(arena(i)), kArena);
                     }));
                emit("fill_pieces_batched_8k_m16", wpc, g, rep, time_rot_us([&](int i) {
                         fill_pieces_batched_kernel<8192, 16><<<g, 256>>>(arena(i), d, n, 8u);
                     }));
                emit("product_fill_pieces_deferred_decode", wpc, g, rep, time_rot_us([&](int i) {
                         fill_pieces_deferred_kernel<true><<<g, 256>>>(arena(i), kArena, d, n, 8u);
                     }));
                emit("product_fill_pieces_deferred_decode_nowait", wpc, g, rep, time_rot_us([&](int i) {
                         fill_pieces_deferred_kernel<false><<<g, 256>>>(arena(i), kArena, d, n, 8u);
                     }));
                emit("fill_pieces_batched_8k_m16_drain1", wpc, g, rep, time_rot_us([&](int i) {
                         fill_pieces_batched_kernel<8192, 16, 1><<<g, 256>>>(arena(i), d, n, 8u);
                     }));
                emit("fill_pieces_batched_8k_m16_drain2", wpc, g, rep, time_rot_us([&](int i) {
                         fill_pieces_batched_kernel<8192, 16, 2><<<g, 256>>>(arena(i), d, n, 8u);
                     }));
                emit("fill_pieces_batched_8k_m16_drain4", wpc, g, rep, time_rot_us([&](int i) {
                         fill_pieces_batched_kernel<8192, 16, 4><<<g, 256>>>(arena(i), d, n, 8u);
                     }));
                emit("fill_pieces_batched_8k_m16_drain8", wpc, g, rep, time_rot_us([&](int i) {
                         fill_pieces_batched_kernel<8192, 16, 8><<<g, 256>>>(arena(i), d, n, 8u);
                     }));
                emit("fill_pieces_nodrain_8k_m16", wpc, g, rep, time_rot_us([&](int i) {
                         fill_pieces_nodrain_kernel<8192, 16><<<g, 256>>>(arena(i), d, n, 8u);
                     }));
                emit("fill_pieces_nodrain_8k_m8", wpc, g, rep, time_rot_us([&](int i) {
                         fill_pieces_nodrain_kernel<8192, 8><<<g, 256>>>(arena(i), d, n, 8u);
                     }));
                emit("product_fill_pieces_kernel", wpc, g, rep, time_rot_us([&](int i) {
                         cts::fill_pieces_kernel<false><<<g, 256>>>(arena(i), kArena, d, n, 8u);
                     }));
            }
            continue;
        }
        for (int wpc : {4, 8, 16}) {
            const int g = cus * wpc / 4;
            emit("b16_flat_u1", wpc, g, rep, time_rot_us([&](int i) {
                     b16_flat_kernel<1><<<g, 256>>>(reinterpret_cast<u32x4*>(arena(i)), kArena);
                 }));
            emit("b16_flat_u2", wpc, g, rep, time_rot_us([&](int i) {
                     b16_flat_kernel<2><<<g, 256>>>(reinterpret_cast<u32x4*>(arena(i)), kArena);
                 }));
            emit("fill_pieces_4k", wpc, g, rep, time_rot_us([&](int i) {
                     fill_pieces_kernel<4096><<<g, 256>>>(arena(i), d, n, 16u);
                 }));
            emit("fill_pieces_8k", wpc, g, rep, time_rot_us([&](int i) {
                     fill_pieces_kernel<8192><<<g, 256>>>(arena(i), d, n, 8u);
                 }));
            emit("fill_pieces_16k", wpc, g, rep, time_rot_us([&](int i) {
                     fill_pieces_kernel<16384><<<g, 256>>>(arena(i), d, n, 4u);
                 }));
        }
        (void)g16;
    }
    const hipError_t e = hipDeviceSynchronize();
    (void)hipFree(d);
    (void)hipFree(big);
    return e == hipSuccess ? 0 : 1;
}
