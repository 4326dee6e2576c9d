// cts_ring_store_loop.hpp — the store loop of one staged batch of a datagram ring. A fragment, not a header: it is
// included inside the batch loop of media_stream_fill_ring_kernel (cts_fill.hip) and of ms_server_fill and
// ms_server_timed_fill (cts_ms_server_fill_body.hpp), so
// that these kernels run one loop and the compiler sees, in each of them, the text it saw before the second one
// existed (a function taking the LDS arrays changed the first kernel's instructions).
//
// In scope where it is included:
//   template parameters  NTS, SCALAR
//   constexpr            WAVES (kBlock / 64)
//   hs[kRingBatch], ls[kRingBatch]   the batch's headers (RingHeader) and lengths, in LDS, staged and synchronised
//   ring                 u32x4*, chunk 0 of datagram 0
//   d0, nb               the batch: datagrams [d0, d0 + nb), nb <= kRingBatch
//   cps, stride, arena_bytes, full_slots, lane, wave
// It may `continue` the batch loop (a wave with no chunks of this batch).
//
// SCALAR: stride >= 1024, so a round holds at most two datagram starts and the wave tracks its datagram and chunk as
// wave-uniform values; otherwise each lane finds its own.

        // this wave's run of the batch's chunks, whole 64-chunk rounds (the last run may end inside one)
        const uint32_t nk = nb * cps;
        const uint32_t per_w = ((nk + WAVES - 1u) / WAVES + 63u) & ~63u;
        uint32_t kl = wave * per_w;
        const uint32_t kl1 = kl + per_w < nk ? kl + per_w : nk;
        const uint64_t kbase = d0 * cps;  // the batch's first ring chunk
        if constexpr (SCALAR) {
            if (kl >= kl1) continue;
            uint32_t ib = kl / cps, cb = kl - ib * cps;  // lane 0's datagram (in the batch) and chunk
            for (; kl < kl1; kl += 64u) {
                const bool crosses = cb + 63u >= cps;
                const uint32_t i1 = ib + 1u < nb ? ib + 1u : ib;
                const uint32_t l0 = ls[ib], l1 = ls[i1];
                const bool whole = kl + 64u <= kl1 && l0 == stride && d0 + ib < full_slots &&
                                   (!crosses || (ib + 1u < nb && l1 == stride && d0 + ib + 1u < full_slots));
                uint32_t c = cb + lane;
                const bool second = c >= cps;
                if (second) c -= cps;
                if (__builtin_amdgcn_readfirstlane(whole ? 1 : 0)) {
                    u32x4 e = expected_chunk((16u * c - CTS_UDP_DATA_HEADER_LENGTH) & 0xFFFFu, 0u);
                    if (cb < 2u) e = header_lanes(e, lane, 0u - cb, hs[ib]);
                    if (crosses) e = header_lanes(e, lane, cps - cb, hs[i1]);
                    if constexpr (NTS) __builtin_nontemporal_store(e, ring + kbase + kl + lane);
                    else ring[kbase + kl + lane] = e;
                } else if (kl + lane < kl1) {
                    const uint32_t t = second ? i1 : ib;
                    ring_chunk_checked<NTS>(ring, kbase + kl + lane, d0 + t, c, ls[t], hs[t], stride, arena_bytes);
                }
                cb += 64u;
                if (cb >= cps) {
                    cb -= cps;
                    ++ib;
                }
            }
        } else {  // stride < 1024: several datagrams per round, each lane finds its own
            for (uint32_t k = kl + lane; k < kl1; k += 64u) {
                const uint32_t t = k / cps, c = k - t * cps;
                ring_chunk_checked<NTS>(ring, kbase + k, d0 + t, c, ls[t], hs[t], stride, arena_bytes);
            }
        }
