// cts_spans.hpp — the grids and the per-wave span of the accounting passes (host side, no device code).
//
// Every accounting launch takes one grid rule (item_grid): enough workgroups for its items, at most kSpanBlocksPerCu
// per CU; the kernels go grid-stride beyond the cap.
// conn_accumulate (cts_refview_accumulate_conns / _strided) and ms_conn_accumulate
// (cts_media_stream_conns_accumulate) do not walk a batch grid-stride: every wave of the grid takes one contiguous
// span of it, so runs of equal conn_index lie in neighbouring lanes and tiles. The grid is the reference view's (one
// descriptor per lane); the span is the batch divided over the grid's waves, rounded up to whole tiles of 64
// descriptors. The waves past ceil(n / span) get an empty span.
// tests/cpp/spans_check.cpp prints span_geometry's answers; tests/accounting_plans.py states the same arithmetic in
// Python and the tests hold the two together.
#pragma once

#include <stdint.h>

namespace cts {

constexpr uint32_t kSpanBlock = 256;       // lanes of a workgroup (kBlock of the kernels)
constexpr uint32_t kSpanTile = 64;         // descriptors per wave and step
constexpr uint32_t kSpanBlocksPerCu = 8;   // 2048 lanes per CU: every wave slot of the CU holds one

// Workgroups for `items` items at items_per_block each, on a device of num_cus compute units (below 1 counts as 1).
inline uint32_t item_grid(uint64_t items, uint32_t items_per_block, int num_cus)
{
    const uint64_t want = (items + items_per_block - 1) / items_per_block;
    const uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 1) * kSpanBlocksPerCu;
    return (uint32_t)(want < cap ? want : cap);
}

struct SpanGeometry {
    uint32_t grid;  // workgroups
    uint32_t span;  // descriptors per wave, a multiple of kSpanTile
};

// n > 0 descriptors on a device of num_cus compute units (below 1 counts as 1).
inline SpanGeometry span_geometry(uint32_t n, int num_cus)
{
    const uint32_t grid = item_grid(n, kSpanBlock, num_cus);
    const uint64_t waves = (uint64_t)grid * (kSpanBlock / kSpanTile);
    const uint32_t span = (uint32_t)((((uint64_t)n + waves - 1) / waves + kSpanTile - 1) / kSpanTile * kSpanTile);
    return SpanGeometry{grid, span};
}

}  // namespace cts
