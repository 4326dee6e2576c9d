// cts_launch.hpp — what the launchers of the kernel units share on the host: cts_grids.hpp's rules (plain integers,
// shared with the tests' model of the loop depths) fed from the launch geometry, and the turn from run-time flags to
// template arguments.
#pragma once

#include <type_traits>

#include "cts_grids.hpp"
#include "cts_internal.hpp"

namespace cts {

// Grid-stride launches: the path's blocks-per-CU value out of the launch geometry (bpc_cap > 0 overrides it).
inline uint32_t grid_for(uint32_t n, int teams_per_block, const LaunchGeometry& geo, int bpc_cap = 0)
{
    const int bpc = bpc_cap > 0 ? bpc_cap : (teams_per_block > 1 ? geo.small_blocks_per_cu : geo.blocks_per_cu);
    return grid_for(n, teams_per_block, geo.num_cus, bpc);
}

// Chunked launch of a four-buffers-per-wave kernel (QuadWalk): chunk = geo.small_chunk buffers
inline ContigGrid contig_grid(uint32_t n, const LaunchGeometry& geo)
{
    return contig_grid(n, geo.num_cus, geo.small_blocks_per_cu, geo.small_chunk);
}

// f(std::bool_constant<flag>{}...) for run-time flags: each becomes an argument whose .value is a constant, so
//   with_flags([&](auto NT, auto STRIDED) { kernel<NT.value, STRIDED.value><<<...>>>(...); }, nontemporal, strided);
// launches one of the four instantiations.
template <bool... Bs, typename F>
inline void with_flags(F&& f)
{
    f(std::bool_constant<Bs>{}...);
}
template <bool... Bs, typename F, typename... Rest>
inline void with_flags(F&& f, bool flag, Rest... rest)
{
    if (flag) with_flags<Bs..., true>(f, rest...);
    else with_flags<Bs..., false>(f, rest...);
}

}  // namespace cts
