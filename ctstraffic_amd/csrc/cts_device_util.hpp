// cts_device_util.hpp — the few device-side definitions that every kernel unit (cts_verify.hip,
// cts_media_stream_recv.hip, cts_fill.hip, cts_tick_plan.hip, cts_accounting.hip) needs: the block size, the empty-slot value, the descriptor check, a batch's source and the wave sums.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cts_engine.h"

namespace cts {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kBlock = 256;

__device__ __forceinline__ bool desc_bad(const cts_buf_desc& d, uint64_t arena_bytes)
{
    // FAIL_FAST conditions of the reference (offset >= c_bufferPatternSize,
    // ctsIOPattern.cpp:723-725) and buffers outside the arena are flagged, not read.
    return d.expected_pattern_offset >= 65536u || d.length < d.skip_head || d.byte_offset > arena_bytes ||
           arena_bytes - d.byte_offset < (uint64_t)d.length;
}

// Where the buffers of a quad-team walk come from: a descriptor array, or (STRIDED) a uniformly strided
// receive ring -- buffer i at i * stride, completed length lens[i], one skip / expected offset /
// connection for the whole ring (a UDP socket's datagrams: skip 26, expected 0), read as 4 bytes of
// metadata per buffer instead of a 24-byte descriptor.
struct VSource {
    const cts_buf_desc* descs;  // !STRIDED
    const uint32_t* lens;       // STRIDED
    uint32_t stride, skip_head, expected, conn_index;
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    return v;
}

}  // namespace cts
