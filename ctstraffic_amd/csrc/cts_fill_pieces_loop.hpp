// cts_fill_pieces_loop.hpp — the body of the fill in piece order, included (not a function: see DESIGN.md §3 "File
// layout") by its two entry points in cts_fill.hip: fill_pieces_kernel, whose buffer count is a launch argument, and
// tcp_sender_fill_pieces, which reads it from the tick block. In scope: arena, arena_bytes, descs, n (buffers), ppb,
// the constants PIECE and BATCH, and NTS.
    typedef u32x4 __attribute__((address_space(1)))* gstore_ptr;
    constexpr uint32_t kChunks = PIECE / 16;
    static_assert(PIECE % (16 * kBlock) == 0 && BATCH <= 64, "whole rounds per piece; one lane per piece");
    const uint64_t total = (uint64_t)n * ppb;
    const uint32_t lane = threadIdx.x;
    const uint32_t m_own = lane & 63u;  // every wave decodes the batch for itself (readlane reads the own wave)
    const uint64_t G = gridDim.x;
    PieceJob cur = decode_piece<PIECE>(arena, arena_bytes, descs, blockIdx.x + (uint64_t)m_own * G, total, ppb,
                                       m_own < (uint32_t)BATCH);
    for (uint64_t v0 = blockIdx.x; v0 < total; v0 += (uint64_t)BATCH * G) {
        // the next batch, decoded before this batch's stores. Its load is waited for at once, which also waits for
        // the previous batch's stores (vector loads and stores share one in-order counter): once per batch, the wave
        // cadence that keeps the grid's stores adjacent (no wait 5.6 TB/s, a wait every 1-4 pieces 5.1-6.2, the
        // decode after the stores 5.7, against 6.2 here: profiles/r06/j, l)
        const PieceJob nxt = decode_piece<PIECE>(arena, arena_bytes, descs, v0 + (uint64_t)(BATCH + m_own) * G, total,
                                                 ppb, m_own < (uint32_t)BATCH);
#pragma unroll 1
        for (int m = 0; m < BATCH; ++m) {
            const uint32_t kind = lane_u32(cur.kind, m);
            if (kind == 0u) continue;
            const uint64_t base = ((uint64_t)lane_u32((uint32_t)(cur.base >> 32), m) << 32) | lane_u32((uint32_t)cur.base, m);
            const uint32_t q0 = lane_u32(cur.q0, m), cb = lane_u32(cur.cb, m), ce = lane_u32(cur.ce, m);
            if (kind == 1u) {  // whole 16-byte chunks: straight stores
                const gstore_ptr g = (gstore_ptr)base;
                const uint32_t sh = q0 & 1u;
                if (ce <= cb + kChunks) {  // one piece: kChunks / kBlock stores per lane, unrolled
#pragma unroll
                    for (uint32_t u = 0; u < kChunks / kBlock; ++u) {
                        const uint32_t c = cb + u * kBlock + lane;
                        if (c < ce) {
                            const u32x4 e = expected_chunk((q0 + 16u * c) & 0xFFFFu, sh);
                            if constexpr (NTS) __builtin_nontemporal_store(e, g + c);
                            else g[c] = e;
                        }
                    }
                } else {  // the last piece of a buffer longer than the hint said
                    for (uint32_t c = cb + lane; c < ce; c += kBlock) {
                        const u32x4 e = expected_chunk((q0 + 16u * c) & 0xFFFFu, sh);
                        if constexpr (NTS) __builtin_nontemporal_store(e, g + c);
                        else g[c] = e;
                    }
                }
            } else {  // the edge chunks write only their own bytes
                const uint32_t nchunks = lane_u32(cur.nchunks, m), lo = lane_u32(cur.lo, m),
                               hi_last = lane_u32(cur.hi_last, m);
                u32x4* p = reinterpret_cast<u32x4*>((uintptr_t)base);
                for (uint32_t c = cb + lane; c < ce; c += kBlock) fill_chunk<NTS>(p, c, nchunks, q0, lo, hi_last);
            }
        }
        cur = nxt;
    }
