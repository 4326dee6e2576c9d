// cts_fill_team_loop.hpp — the body of the fill by teams of TEAM lanes, one buffer per team and pass, included (not a
// function: see DESIGN.md §3 "File layout") by its two entry points in cts_fill.hip: fill_kernel, whose buffer count
// is a launch argument, and tcp_sender_fill_small, which reads it from the tick block. In scope: arena, arena_bytes,
// descs, n (buffers), the constant TEAM, and NTS.
    constexpr int TEAMS = kBlock / TEAM;
    constexpr int FU = TEAM == kBlock ? 4 : 2;  // stores per lane per whole-span round
    const uint32_t lane = threadIdx.x % TEAM;
    const uint32_t team = (TEAM == kBlock) ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x / TEAM);
    const uint32_t step = gridDim.x * TEAMS;
    uint32_t i = blockIdx.x * TEAMS + team;
    // the next buffer's descriptor is loaded while this one's stores go out: with one workgroup per CU
    // nothing else hides a dependent descriptor load per buffer (49.4 -> see DESIGN §3 fill)
    cts_buf_desc dn;
    if (i < n) dn = descs[i];
    for (; i < n; i = (uint64_t)i + step < n ? i + step : n) {
        const cts_buf_desc d = dn;
        if ((uint64_t)i + step < n) dn = descs[i + step];
        fill_one<TEAM, FU, NTS>(arena, arena_bytes, d, lane);
    }
