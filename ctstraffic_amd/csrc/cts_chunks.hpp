// cts_chunks.hpp — the 16-byte chunk of the data path: what the verify, MediaStream receive and fill units
// (cts_verify.hip, cts_media_stream_recv.hip, cts_fill.hip) share on the device.
//
// Reference semantics (microsoft/ctsTraffic):
//   pattern  ctsTraffic/ctsIOPattern.cpp:35-36,55-80 — byte at stream position j
//            (mod 65536) is P(j) = (j & 1) ? j >> 9 : (j >> 1) & 0xFF, i.e. the
//            little-endian u16 ramp 0..32767 repeated every 64 KiB.
// A buffer's span is cut into 16-byte chunks aligned in memory (1 KiB per wave-instruction). The expected chunk
// is regenerated in registers from the stream position (no pattern table is read): one v_mad_u32_u24 + add/and
// per u16 pair, one v_alignbyte per dword for the byte phase.
// Here: the expected chunk and its stepped form, the byte masks, the chunk loads, wave_min and the per-team LDS
// counters with their flush to a counter shard.
#pragma once

#include <hip/hip_runtime.h>

#include "cts_device_util.hpp"
#include "cts_internal.hpp"

namespace cts {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t pattern_byte_dev(uint32_t pos)
{
    pos &= 0xFFFFu;
    return (pos & 1u) ? (pos >> 9) : ((pos >> 1) & 0xFFu);
}

// Expected 16 bytes for a chunk whose first byte sits at pattern position q
// (0 <= q < 65536); sh = q & 1. The chunk is bytes sh..sh+15 of the u16 values
// k..k+8 (k = q >> 1, mod 32768). Packed: dword j = (k+2j) | (k+2j+1) << 16 =
// base + j*0x20002 with base = k*0x10001 + 0x10000; & 0x7FFF7FFF wraps
// 32768 -> 0 in each half (the low half never exceeds 32775: no carry crosses).
// v_alignbyte with a register shift handles both phases without a branch.
__device__ __forceinline__ u32x4 expected_chunk(uint32_t q, uint32_t sh)
{
    const uint32_t k = q >> 1;
    const uint32_t base = __umul24(k, 0x10001u) + 0x10000u;
    const uint32_t w0 = base & 0x7FFF7FFFu;
    const uint32_t w1 = (base + 0x20002u) & 0x7FFF7FFFu;
    const uint32_t w2 = (base + 0x40004u) & 0x7FFF7FFFu;
    const uint32_t w3 = (base + 0x60006u) & 0x7FFF7FFFu;
    const uint32_t w4 = (base + 0x80008u) & 0x7FFF7FFFu;
    return u32x4{__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                 __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh)};
}

// 0x80 in every byte of x that is nonzero.
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x)
{
    return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

__device__ __forceinline__ uint32_t low_bytes_mask(int nb)  // nb in [0,4]
{
    return (uint32_t)((1ull << (8 * nb)) - 1ull);
}

// Mask keeping bytes [lo, hi) of a 16-byte chunk (0 <= lo <= hi <= 16).
__device__ __forceinline__ u32x4 range_mask(uint32_t lo, uint32_t hi)
{
    u32x4 m;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        int a = (int)lo - 4 * w;
        int b = (int)hi - 4 * w;
        a = a < 0 ? 0 : (a > 4 ? 4 : a);
        b = b < 0 ? 0 : (b > 4 ? 4 : b);
        m[w] = (b > a) ? (low_bytes_mask(b) & ~low_bytes_mask(a)) : 0u;
    }
    return m;
}

__device__ __forceinline__ uint32_t or4(u32x4 x) { return x[0] | x[1] | x[2] | x[3]; }

// A chunk load through an explicitly global (address space 1) pointer: a pointer that
// went through a select or a phi can lose its address space and become a flat load,
// which also counts in lgkmcnt and forces full drains
typedef const u32x4 __attribute__((address_space(1)))* gchunk_ptr;
template <bool NT>
__device__ __forceinline__ u32x4 load_chunk_g(const u32x4* p)
{
    const gchunk_ptr g = (gchunk_ptr)p;
    if constexpr (NT) {
        return __builtin_nontemporal_load(g);
    } else {
        return *g;
    }
}

template <bool NT>
__device__ __forceinline__ u32x4 buf_load(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff)
{
    return __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, NT ? 2 : 0);  // aux 2 = nt
}

// Buffer resources address a span with 32-bit byte offsets and a 32-bit num_records, so spans of this many chunks
// (2 GiB) or more take 64-bit pointers instead (scan_giant_exact in cts_verify.hip, fill_one in cts_fill.hip).
constexpr uint32_t kGiantChunks = 1u << 27;

// Expected chunk u of a round: k advances by TEAM*8 per unrolled step (16*TEAM
// bytes / 2), added to the packed base before the per-half wrap mask. The low
// half stays below 65536 (k <= 32767 + 8*TEAM*(U-1) + 8), so no carry crosses.
template <int TEAM, int U, bool EVEN = false>
__device__ __forceinline__ u32x4 expected_step(uint32_t B, int u, uint32_t sh)
{
    static_assert(32767 + 8 * TEAM * (U - 1) + 8 < 65536, "packed k must not carry");
    // B is made opaque so each word is v_add(literal) + v_and: left visible,
    // hipcc folds the adds into v_mad_u32_u24 whose 32-bit addends (VOP3 takes
    // no literal on gfx950) it then parks in ~40 VGPRs, halving occupancy.
    uint32_t bb = B;
    asm volatile("" : "+v"(bb));
    const uint32_t b = bb + (uint32_t)u * (uint32_t)(8 * TEAM) * 0x10001u;
    const uint32_t w0 = b & 0x7FFF7FFFu;
    const uint32_t w1 = (b + 0x20002u) & 0x7FFF7FFFu;
    const uint32_t w2 = (b + 0x40004u) & 0x7FFF7FFFu;
    const uint32_t w3 = (b + 0x60006u) & 0x7FFF7FFFu;
    if constexpr (EVEN) {
        // byte phase 0 (every 16-aligned expected offset, 75 % of config 2): the chunk IS
        // the four packed pairs, no funnel shift and no fifth word
        return u32x4{w0, w1, w2, w3};
    } else {
        const uint32_t w4 = (b + 0x80008u) & 0x7FFF7FFFu;
        return u32x4{__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                     __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh)};
    }
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// Per-team running counters in LDS: ctr[team][kCounterCount], zeroed at kernel start.
template <int TEAMS>
__device__ __forceinline__ void zero_counters(uint64_t (*ctr)[kCounterCount])
{
    if (threadIdx.x < (unsigned)(TEAMS * kCounterCount)) ctr[threadIdx.x / kCounterCount][threadIdx.x % kCounterCount] = 0;
    __syncthreads();
}

// Fold the per-team counters of a workgroup and add them to the counter shard
// of this workgroup (one 64-byte line per shard, CTS_COUNTER_SHARDS shards).
template <int TEAMS>
__device__ __forceinline__ void flush_counters(uint64_t* counters, uint64_t (*ctr)[kCounterCount])
{
    __syncthreads();
    if (counters == nullptr) return;
    if (threadIdx.x < (unsigned)kCounterCount) {
        uint64_t sum = 0;
#pragma unroll
        for (int t = 0; t < TEAMS; ++t) sum += ctr[t][threadIdx.x];
        if (sum)
            atomicAdd((unsigned long long*)&counters[(blockIdx.x % CTS_COUNTER_SHARDS) * kCounterSlots + threadIdx.x],
                      (unsigned long long)sum);
    }
}

}  // namespace cts
