// cts_spans.hpp — the grid and the per-wave span of the accounting passes (host side, no device code).
//
// conn_accumulate (cts_refview_accumulate_conns / _strided) and ms_conn_accumulate
// (cts_media_stream_conns_accumulate) do not walk a batch grid-stride: every wave of the grid takes one contiguous
// span of it, so runs of equal conn_index lie in neighbouring lanes and tiles. The grid is the reference view's (one
// descriptor per lane, at most kSpanBlocksPerCu workgroups per CU); the span is the batch divided over the grid's
// waves, rounded up to whole tiles of 64 descriptors. The waves past ceil(n / span) get an empty span.
// tests/cpp/spans_check.cpp prints this function's answers; tests/accounting_plans.py states the same arithmetic in
// Python and the tests hold the two together.
#pragma once

#include <stdint.h>

namespace cts {

constexpr uint32_t kSpanBlock = 256;       // lanes of a workgroup (kBlock of the kernels)
constexpr uint32_t kSpanTile = 64;         // descriptors per wave and step
constexpr uint32_t kSpanBlocksPerCu = 8;   // 2048 lanes per CU: every wave slot of the CU holds one

struct SpanGeometry {
    uint32_t grid;  // workgroups
    uint32_t span;  // descriptors per wave, a multiple of kSpanTile
};

// n > 0 descriptors on a device of num_cus compute units (below 1 counts as 1).
inline SpanGeometry span_geometry(uint32_t n, int num_cus)
{
    const uint64_t want = ((uint64_t)n + kSpanBlock - 1) / kSpanBlock;
    const uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 1) * kSpanBlocksPerCu;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const uint64_t waves = (uint64_t)grid * (kSpanBlock / kSpanTile);
    const uint32_t span = (uint32_t)((((uint64_t)n + waves - 1) / waves + kSpanTile - 1) / kSpanTile * kSpanTile);
    return SpanGeometry{grid, span};
}

}  // namespace cts
