// cts_grids.hpp — the grids of the data-path launches: verify, fill and the MediaStream receive and fills (host side,
// no device code).
//
// Every rule takes plain integers: the launch's item count, the device's compute units and the blocks-per-CU cap of
// its path (LaunchGeometry's values, cts_internal.hpp; cts_launch.hpp's wrappers pick them). The launchers of
// cts_verify.hip, cts_media_stream_recv.hip and cts_fill.hip call them; how deep a
// kernel's outer loop runs (batches per workgroup, rounds per wave, ring flushes) follows from the grid alone.
// tests/cpp/grids_check.cpp prints the rules' answers; tests/launch_depths.py states the same arithmetic in Python
// with the loop depths on top, and tests/test_launch_depths_cpu.py holds the two together.
#pragma once

#include <stdint.h>

namespace cts {

constexpr uint32_t kGridBlock = 256;       // lanes of a workgroup (kBlock of the kernels)
constexpr uint32_t kGridQuadTeams = 16;    // buffers per workgroup and round of the four-buffers-per-wave kernels
constexpr uint32_t kGridFillPiece = 8192;  // bytes per piece of the fill in piece order (kFillPiece)
constexpr uint32_t kGridFillBatch = 256;   // datagrams per LDS batch of fill_batched_kernel (kFillBatch)
constexpr uint32_t kGridRingBatch = 512;   // datagrams per LDS batch of the ring fills (kRingBatch)

// Grid-stride launches (verify_wg_kernel, fill_kernel, fill_span_kernel): n items, teams_per_block of them per
// workgroup and pass, at most num_cus * bpc workgroups (bpc below 1 counts as 8).
inline uint32_t grid_for(uint32_t n, int teams_per_block, int num_cus, int bpc)
{
    const uint64_t want = ((uint64_t)n + teams_per_block - 1) / teams_per_block;
    const uint64_t cap = (uint64_t)num_cus * (uint64_t)(bpc > 0 ? bpc : 8);
    // grid-stride with the same number of teams' worth of work per workgroup: past the cap
    // the grid shrinks to ceil(want / per) so no workgroup runs one buffer more than the
    // rest (an uneven split, e.g. 4096 buffers over 1280 workgroups, leaves a tail of
    // workgroups with an extra buffer that alone sets the launch's end)
    const uint64_t per = want <= cap ? 1 : (want + cap - 1) / cap;
    const uint64_t g = (want + per - 1) / per;
    return (uint32_t)(g == 0 ? 1 : g);
}

// Chunked launch of a four-buffers-per-wave kernel (QuadWalk): small_chunk buffers per chunk (rounded up to the
// block's 16 teams); 0 = one block-contiguous range per block, every block but the last with the same count.
struct ContigGrid {
    uint32_t grid, per;
};
inline ContigGrid contig_grid(uint32_t n, int num_cus, int small_bpc, int small_chunk)
{
    const uint32_t teams = kGridQuadTeams;
    const uint32_t g = grid_for(n, (int)teams, num_cus, small_bpc);
    if (small_chunk > 0) {
        const uint64_t per = ((uint64_t)small_chunk + teams - 1) / teams * teams;
        const uint64_t chunks = ((uint64_t)n + per - 1) / per;
        return ContigGrid{(uint32_t)(chunks < g ? chunks : g), (uint32_t)per};
    }
    const uint64_t groups = ((uint64_t)n + teams - 1) / teams;
    const uint64_t per = (groups + g - 1) / g * teams;
    return ContigGrid{(uint32_t)(((uint64_t)n + per - 1) / per), (uint32_t)per};
}

// Whole LDS batches of `batch` datagrams per workgroup, at most num_cus * ring_bpc workgroups (ring_bpc below 1
// counts as 4): fill_batched_kernel (kGridFillBatch), media_stream_fill_ring_kernel and ms_server_fill
// (kGridRingBatch, n = the tick's capacity).
inline uint32_t batch_fill_grid(uint32_t n, uint32_t batch, int num_cus, int ring_bpc)
{
    const uint64_t cap = (uint64_t)num_cus * (uint64_t)(ring_bpc > 0 ? ring_bpc : 4);
    const uint64_t want = ((uint64_t)n + batch - 1) / batch;
    return (uint32_t)(want < cap ? want : cap);
}
inline uint32_t batched_fill_grid(uint32_t n, int num_cus, int ring_bpc)
{
    return batch_fill_grid(n, kGridFillBatch, num_cus, ring_bpc);
}
inline uint32_t ring_fill_grid(uint32_t n, int num_cus, int ring_bpc)
{
    return batch_fill_grid(n, kGridRingBatch, num_cus, ring_bpc);
}

// The fill in piece order (fill_pieces_kernel): ppb pieces of kGridFillPiece bytes per buffer by the hint, one
// workgroup per piece up to num_cus * fill_bpc (fill_bpc below 1 counts as 1).
struct PieceGrid {
    uint32_t grid, ppb;
};
inline PieceGrid piece_fill_grid(uint32_t n, uint32_t max_length_hint, int num_cus, int fill_bpc)
{
    const uint32_t ppb = (uint32_t)(((uint64_t)max_length_hint + kGridFillPiece - 1) / kGridFillPiece);
    const uint64_t total = (uint64_t)n * ppb;
    const uint64_t cap = (uint64_t)num_cus * (uint64_t)(fill_bpc > 0 ? fill_bpc : 1);
    return PieceGrid{(uint32_t)(total < cap ? total : cap), ppb};
}

}  // namespace cts
