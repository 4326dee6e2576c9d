// cts_ms_server_fill_body.hpp — the body of the servers' ring fill: a workgroup's range of the tick's datagrams in
// batches of kRingBatch, each staged from prefix[] and the entries and stored by cts_ring_store_loop.hpp. A fragment,
// not a header: it is the whole body of ms_server_fill and of ms_server_timed_fill (cts_fill.hip), so that both kernels
// run one batch loop and the first keeps, instruction for instruction, the text it had before the second existed.
//
// In scope where it is included:
//   template parameters  NTS, SCALAR
//   the kernel's arguments: ring_base, arena_bytes, stride, first_slot, ids, n, servers, prefix, tick, qpc, qpf, descs,
//                        lengths, full_slots, capacity, n_conns
//   constexpr bool TIMED false: every listed connection sent one frame, current_frame - 1
//                        true:  a connection sent t >= 1 frames from `before[i]` on (const uint64_t*, the planning's
//                               word per listed connection); tick-local datagram q of its take is datagram q % k of
//                               frame before[i] + q / k: one 32-bit division per datagram, in the staging step only

    constexpr uint32_t WAVES = kBlock / 64;
    __shared__ RingHeader hs[kRingBatch];
    __shared__ uint32_t ls[kRingBatch];
    __shared__ uint64_t ps[kRingBatch + 1];
    __shared__ uint64_t first_listed;
    // (the clamp, and the id check below, only matter to a caller who lists a connection twice: nothing is written
    // outside the capacity or read outside the table then either)
    const uint32_t total = tick->datagrams < capacity ? tick->datagrams : capacity;
    if (total == 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t cps = stride >> 4;  // chunks per slot
    // at least a batch's worth of datagrams per workgroup, or all of them
    const uint32_t even = (uint32_t)(((uint64_t)total + gridDim.x - 1u) / gridDim.x);
    const uint32_t least = total < kRingBatch ? total : kRingBatch;
    const uint32_t per_wg = even > least ? even : least;
    const uint64_t g0 = (uint64_t)blockIdx.x * per_wg;
    if (g0 >= total) return;
    const uint64_t g1 = g0 + per_wg < total ? g0 + per_wg : total;
    if (threadIdx.x == 0u) first_listed = ms_server_listed(prefix, 0u, n, g0);
    u32x4* const ring = reinterpret_cast<u32x4*>(ring_base);
    for (uint64_t d0 = g0; d0 < g1; d0 += kRingBatch) {
        const uint32_t nb = (uint32_t)(g1 - d0 < kRingBatch ? g1 - d0 : kRingBatch);
        __syncthreads();  // every wave is done with the previous batch's LDS
        const uint64_t i0 = first_listed;
        for (uint32_t t = threadIdx.x; t <= kRingBatch; t += kBlock) ps[t] = prefix[i0 + t < n ? i0 + t : n];
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < nb; t += kBlock) {
            const uint64_t g = d0 + t;
            uint32_t lo = 0u, hi = kRingBatch + 1u;  // the last w with ps[w] <= g; ps[0] <= d0
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (ps[mid] <= g) lo = mid;
                else hi = mid;
            }
            uint64_t i = i0 + lo, p = ps[lo];
            if (lo == kRingBatch && i + 1u < n) {
                i = ms_server_listed(prefix, i, n, g);
                p = prefix[i];
            }
            if (i >= n) i = n - 1u;  // (never, unless a connection is listed twice)
            const uint32_t c = ids[i];
            const cts_ms_server_state* e = servers + (c < n_conns ? c : 0u);
            uint32_t j = (uint32_t)(g - p), f = 0u;
            if constexpr (TIMED) {
                // datagram q of the connection's take is datagram q % k of frame before + q / k: the one division
                const uint32_t k = e->datagrams_per_frame;
                f = j / (k != 0u ? k : 1u);
                j -= f * k;
            }
            const uint32_t len = c >= n_conns ? 0u
                                              : ms_server_length(e->frame_size_bytes, e->datagram_max_size,
                                                                 e->datagrams_per_frame, j);
            if constexpr (TIMED) hs[t] = RingHeader{before[i] + f, qpc, qpf};
            else hs[t] = RingHeader{(uint64_t)(e->current_frame - 1), qpc, qpf};
            ls[t] = len;
            if (descs != nullptr)
                descs[g] = cts_buf_desc{(first_slot + g) * stride, len, 0u, c, CTS_UDP_DATA_HEADER_LENGTH};
            if (lengths != nullptr) lengths[g] = len;
            if (t == nb - 1u) first_listed = i;
        }
        __syncthreads();
#include "cts_ring_store_loop.hpp"
    }
