// cts_accounting.hip — the descriptor-only accounting passes for gfx950; none of them reads the arena.
//   refview_accumulate   the reference view of a verified batch: descriptors and DataError slots only
//   conn_accumulate      the same pass keeping each connection's entry too; conn_close, conn_slots_rebase
//   ms_conn_accumulate   the MediaStream connections' pass over descriptors and statuses; ms_conn_render, ms_conn_close
// conn_accumulate sums what shares a connection's entry with walk_runs; ms_conn_accumulate still has that walk written
// out (see there). The receive pass that lowers the DataError slots (ms_verify_status_ordinal) is in
// cts_media_stream_recv.hip.
#include <hip/hip_runtime.h>

#include "cts_device_util.hpp"
#include "cts_internal.hpp"
#include "cts_spans.hpp"

namespace cts {

// ---------------------------------------------------------------------------------------------
// The reference view of a verified batch (cts_refview_accumulate): what ctsTraffic would have counted, which
// fails a connection on its first failing VerifyBuffer (ctsIOPattern.cpp:486-489 -> FailedIo) and receives
// nothing of it afterwards. Descriptors only, the arena is never read: buffer i has the stream ordinal
// g = base_index + i, its connection's DataError slot F holds the first failing ordinal (cts_verify_at), and
// the buffer counts as received when g <= F, as clean when g < F, as the failing one when g == F and as
// never received when g > F. Bad descriptors (the verify's desc_bad) count nowhere, as in the verify.
// One descriptor per lane per step, grid-stride: a wave's loads cover 64 x 24 contiguous bytes (or 64 x 4 of a
// strided ring's lengths), read once (nontemporal with CTS_ATTR_NT_LOADS); the slot reads are plain gathers
// that stay in L2 (connection-major batches make them near-broadcasts). The six per-lane sums are reduced by
// wave shuffles, then over the four waves in LDS, then added to the workgroup's counter shard, the route of
// flush_counters.
enum RefSlot {
    kRefBytesRecv = 0,
    kRefBytesOk = 1,
    kRefBuffersRecv = 2,
    kRefBuffersFailed = 3,
    kRefBytesAfterFailure = 4,
    kRefBuffersAfterFailure = 5
};
static_assert(kRefBuffersAfterFailure + 1 == kCounterCount, "a reference-view block folds like a counter block");

// Six wave-reduced sums (lane 0 of each wave holds them) over the workgroup's waves in LDS, then one add per word to
// the workgroup's shard of a counter block: the route of flush_counters. Every kernel of this file ends here.
__device__ __forceinline__ void block_add_six(const uint64_t (&v)[kCounterCount], uint64_t (*red)[kCounterCount],
                                              uint64_t* __restrict__ block)
{
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < kCounterCount; ++k) red[threadIdx.x / 64][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)kCounterCount) {
        uint64_t sum = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) sum += red[w][threadIdx.x];
        if (sum)
            atomicAdd((unsigned long long*)&block[(blockIdx.x % CTS_COUNTER_SHARDS) * kCounterSlots + threadIdx.x],
                      (unsigned long long)sum);
    }
}

// A lane's six sums of the reference view.
struct RefSums {
    uint64_t bytes_recv = 0, bytes_ok = 0, bytes_after = 0;
    uint32_t bufs_recv = 0, bufs_failed = 0, bufs_after = 0;  // per lane: fewer than 2^32 buffers per launch

    // A good buffer of vlen verified bytes with stream ordinal g, whose connection's slot holds `first`; true when
    // it counts as received (g <= first), false when it came after the failure.
    __device__ __forceinline__ bool count(uint32_t g, uint32_t first, uint32_t vlen)
    {
        if (g <= first) {
            bytes_recv += vlen;
            bufs_recv += 1u;
            if (g < first) bytes_ok += vlen;
            else bufs_failed += 1u;
            return true;
        }
        bytes_after += vlen;
        bufs_after += 1u;
        return false;
    }

    // The six sums over the wave, in a reference-view block's order.
    __device__ __forceinline__ void reduce(uint64_t (&v)[kCounterCount]) const
    {
        v[kRefBytesRecv] = wave_sum64(bytes_recv);
        v[kRefBytesOk] = wave_sum64(bytes_ok);
        v[kRefBuffersRecv] = wave_sum(bufs_recv);  // a wave's 64 lanes of one launch: still below 2^32
        v[kRefBuffersFailed] = wave_sum(bufs_failed);
        v[kRefBytesAfterFailure] = wave_sum64(bytes_after);
        v[kRefBuffersAfterFailure] = wave_sum(bufs_after);
    }
};

template <bool NT, bool STRIDED>
__device__ __forceinline__ cts_buf_desc refview_desc(const VSource& src, uint64_t i)
{
    if constexpr (STRIDED) {
        const uint32_t len = NT ? __builtin_nontemporal_load(src.lens + i) : src.lens[i];
        // vs_desc's rule: a completion longer than its slot is a bad descriptor
        return cts_buf_desc{i * src.stride, len, len <= src.stride ? src.expected : 65536u, src.conn_index,
                            src.skip_head};
    } else {
        // 24 bytes, 8-byte aligned: three 8-byte loads
        const uint64_t* p = reinterpret_cast<const uint64_t*>(src.descs + i);
        const uint64_t a = NT ? __builtin_nontemporal_load(p) : p[0];
        const uint64_t b = NT ? __builtin_nontemporal_load(p + 1) : p[1];
        const uint64_t c = NT ? __builtin_nontemporal_load(p + 2) : p[2];
        return cts_buf_desc{a, (uint32_t)b, (uint32_t)(b >> 32), (uint32_t)c, (uint32_t)(c >> 32)};
    }
}

template <bool NT, bool STRIDED>
__global__ void __launch_bounds__(kBlock)
    refview_accumulate(uint64_t arena_bytes, VSource src, uint32_t n, uint32_t base_index,
                       const uint32_t* __restrict__ conn_first_fail, uint32_t n_conns, uint64_t* __restrict__ ref)
{
    __shared__ uint64_t red[kBlock / 64][kCounterCount];
    RefSums sums;
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
        const cts_buf_desc d = refview_desc<NT, STRIDED>(src, i);
        if (desc_bad(d, arena_bytes)) continue;
        // a connection without a slot never fails
        const uint32_t first = d.conn_index < n_conns ? conn_first_fail[d.conn_index] : kNone;
        // base_index + n <= 0xFFFFFFFF (checked by the entry point)
        sums.count(base_index + (uint32_t)i, first, d.length - d.skip_head);
    }
    uint64_t v[kCounterCount];
    sums.reduce(v);
    block_add_six(v, red, ref);
}

// ---------------------------------------------------------------------------------------------
// The run-aggregation walk of conn_accumulate (ms_conn_accumulate has it written out). An entry would take one set of
// atomics per buffer, and a strided ring or a connection-major batch sends them all to one entry; so everything that
// shares an entry is summed on the chip first. Each wave walks a contiguous span of the batch (`span` items, a
// multiple of 64; not a grid-stride interleave), 64 items per step, so its loads stay contiguous and runs of equal key
// (conn_index) lie in neighbouring lanes. In a tile, a lane whose key differs from the lane below heads a run; the runs
// are summed by a segmented inclusive scan (shuffles, six steps); the tail lane of every run that ends inside the tile
// adds it to the entry, and the run that reaches lane 63 is carried in registers into the wave's next tile, where it
// either goes on (same key in lane 0) or is added by lane 0. A tile that is nothing but the open run is "parked": its
// per-lane sums wait, without a shuffle, until the run is next needed. The run a wave still holds at the end of its
// span goes to LDS, where runs that go on across the workgroup's four waves are joined before they are added. An entry
// therefore takes at most one set of adds per run and wave, and a one-connection batch one set per workgroup of the
// grid, whatever n is: adds to one address serialise in L2, 32 768 of them (one set per wave, 16 Mi-datagram ring)
// took about 215 us. Lanes that count nowhere (bad descriptors, the tail of a partial tile) carry the key kNone, which
// has no entry.

// The sums of one run: W 64-bit sums and C counts. Inside a tile the counts share one 32-bit word, 32 / C bits each.
template <int W, int C>
struct RunSums {
    static_assert(C >= 1 && C <= 4, "a count is at most 64 per tile and needs 7 bits of the packed word");
    uint64_t wide[W];
    uint32_t count[C];
    __device__ __forceinline__ void operator+=(const RunSums& o)
    {
        for (int k = 0; k < W; ++k) wide[k] += o.wide[k];
        for (int k = 0; k < C; ++k) count[k] += o.count[k];
    }
};

// What a pass gives the walk:
//   kWide, kCounts, Item                       the sums of a run and what is loaded per item
//   Item load(uint64_t i) const                item i of the batch
//   uint32_t judge(item, i, in_span, sums)     the lane's key (kNone where it counts nowhere) and its own sums; also
//                                              the pass's node-wide per-lane sums and per-item side effects
//   void add(uint32_t key, sums) const         one finished run into the entry of `key`
template <class Pass>
__device__ __forceinline__ void walk_runs(Pass& pass, uint32_t n, uint32_t span)
{
    constexpr int W = Pass::kWide, C = Pass::kCounts;
    constexpr uint32_t kBits = 32u / C, kMask = kBits == 32u ? ~0u : (1u << kBits) - 1u;
    using Sums = RunSums<W, C>;
    __shared__ uint64_t tail_sum[kBlock / 64][W + C];
    __shared__ uint32_t tail_key[kBlock / 64][2];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lo = ((uint64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64) * span;
    const uint64_t hi = lo + span < (uint64_t)n ? lo + span : (uint64_t)n;  // lo >= n: an empty span
    // the open run: the one that reached lane 63 of the previous tile (wave-uniform)
    uint32_t ckey = kNone;
    Sums open = {};
    bool whole = true;  // the span so far is one run (wave-uniform)
    // per-lane sums of the tiles that were nothing but the open run, not yet in `open`
    Sums park = {};
    bool parked = false;
    const auto unpark = [&]() {
        for (int k = 0; k < W; ++k) open.wide[k] += wave_sum64(park.wide[k]);
        for (int k = 0; k < C; ++k) open.count[k] += wave_sum(park.count[k]);
    };
    typename Pass::Item next = {};
    if (lo < hi) next = pass.load(lo + lane < hi ? lo + lane : hi - 1);
    for (uint64_t t = lo; t < hi; t += 64) {
        const uint64_t i = t + lane;
        const typename Pass::Item item = next;
        if (t + 64 < hi) next = pass.load(i + 64 < hi ? i + 64 : hi - 1);  // the next tile, early
        Sums s;
        const uint32_t key = pass.judge(item, i, i < hi, s);
        // run heads, and for every lane the head of its run
        const uint32_t below = (uint32_t)__shfl_up((int)key, 1, 64);
        const bool head = lane == 0u || key != below;
        const uint64_t heads = __ballot(head);
        const uint32_t h = 63u - (uint32_t)__builtin_clzll(heads & (~0ull >> (63u - lane)));
        const bool merge = (uint32_t)__shfl((int)key, 0, 64) == ckey;
        if (heads == 1ull && merge) {
            // the whole tile goes on the open run: per-lane sums, no shuffle (they join the run when it is next needed)
            park += s;
            parked = true;
            continue;
        }
        if (parked) {
            unpark();
            park = {};
            parked = false;
        }
        // segmented inclusive scan: the wide sums, and the counts packed into one word (each <= 64)
        uint32_t c = 0;
        for (int k = 0; k < C; ++k) c |= s.count[k] << (k * kBits);
#pragma unroll
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            uint64_t up[W];
            for (int k = 0; k < W; ++k) up[k] = (uint64_t)__shfl_up((unsigned long long)s.wide[k], off, 64);
            const uint32_t uc = (uint32_t)__shfl_up((int)c, off, 64);
            if (lane >= h + off) {
                for (int k = 0; k < W; ++k) s.wide[k] += up[k];
                c += uc;
            }
        }
        for (int k = 0; k < C; ++k) s.count[k] = (c >> (k * kBits)) & kMask;
        // the open run goes on in lane 0's run, or ends here
        whole = whole && heads == 1ull && (merge || t == lo);
        if (merge && h == 0u) s += open;
        if (!merge && lane == 0u) pass.add(ckey, open);
        const bool tail = lane == 63u || ((heads >> (lane + 1u)) & 1ull) != 0ull;
        if (tail && lane != 63u) pass.add(key, s);
        ckey = (uint32_t)__shfl((int)key, 63, 64);
        for (int k = 0; k < W; ++k) open.wide[k] = (uint64_t)__shfl((unsigned long long)s.wide[k], 63, 64);
        for (int k = 0; k < C; ++k) open.count[k] = (uint32_t)__shfl((int)s.count[k], 63, 64);
    }
    if (parked) unpark();
    // The waves' last open runs meet in LDS: the spans of a workgroup's waves follow one another, so a wave whose
    // whole span was one run goes on the run the wave before it left open, and a one-connection batch costs one set of
    // adds per workgroup.
    if (lane == 0u) {
        for (int k = 0; k < W; ++k) tail_sum[threadIdx.x / 64][k] = open.wide[k];
        for (int k = 0; k < C; ++k) tail_sum[threadIdx.x / 64][W + k] = open.count[k];
        tail_key[threadIdx.x / 64][0] = ckey;
        tail_key[threadIdx.x / 64][1] = whole ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        const auto left = [&](int w) {  // the run wave w left open
            Sums r;
            for (int k = 0; k < W; ++k) r.wide[k] = tail_sum[w][k];
            for (int k = 0; k < C; ++k) r.count[k] = (uint32_t)tail_sum[w][W + k];
            return r;
        };
        uint32_t key = tail_key[0][0];
        Sums acc = left(0);
        for (int w = 1; w < kBlock / 64; ++w) {
            if (tail_key[w][1] == 0u || tail_key[w][0] != key) {
                pass.add(key, acc);
                key = tail_key[w][0];
                acc = {};
            }
            acc += left(w);
        }
        pass.add(key, acc);
    }
}

// ---------------------------------------------------------------------------------------------
// Connections on the device (cts_connections.h): the reference-view pass that also keeps each connection's entry
// (conn_accumulate), the close (conn_close) and the slot rebase (conn_slots_rebase).

// One finished run of a connection's buffers into its entry: at most four 64-bit adds.
__device__ __forceinline__ void conn_run_add(cts_conn_state* __restrict__ state, uint32_t conn, uint32_t n_conns,
                                             uint64_t recv, uint64_t after, uint32_t nrecv, uint32_t nafter)
{
    if (conn >= n_conns) return;  // a connection without an entry (and kNone, the key of lanes that count nowhere)
    unsigned long long* p = reinterpret_cast<unsigned long long*>(state + conn);
    if (recv) atomicAdd(p + 0, (unsigned long long)recv);
    if (nrecv) atomicAdd(p + 1, (unsigned long long)nrecv);
    if (after) atomicAdd(p + 2, (unsigned long long)after);
    if (nafter) atomicAdd(p + 3, (unsigned long long)nafter);
}

// What conn_accumulate gives walk_runs: a descriptor per item, judged as in refview_accumulate; a run carries the
// bytes received and after the failure (64-bit) and the two buffer counts.
template <bool NT, bool STRIDED>
struct ConnPass {
    static constexpr int kWide = 2, kCounts = 2;
    using Item = cts_buf_desc;
    using Sums = RunSums<kWide, kCounts>;

    uint64_t arena_bytes;
    const VSource& src;
    uint32_t base_index;
    const uint32_t* __restrict__ conn_first_fail;
    uint32_t n_conns;
    cts_conn_state* __restrict__ state;
    uint32_t ring_first;  // a ring is one connection: its slot is read once (STRIDED)
    RefSums node;         // the node-wide six sums, refview_accumulate's

    __device__ __forceinline__ Item load(uint64_t i) const { return refview_desc<NT, STRIDED>(src, i); }

    __device__ __forceinline__ uint32_t judge(const Item& d, uint64_t i, bool in_span, Sums& s)
    {
        const bool ok = in_span && !desc_bad(d, arena_bytes);
        const uint32_t key = ok ? d.conn_index : kNone;
        // a connection without a slot never fails
        const uint32_t first = STRIDED ? ring_first : (key < n_conns ? conn_first_fail[key] : kNone);
        const uint32_t g = base_index + (uint32_t)i;  // base_index + n <= 0xFFFFFFFF (checked by the entry point)
        const uint32_t vlen = ok ? d.length - d.skip_head : 0u;
        const bool recv = ok && node.count(g, first, vlen);  // counted only where ok
        const bool after = ok && !recv;
        s.wide[0] = recv ? vlen : 0u;
        s.wide[1] = after ? vlen : 0u;
        s.count[0] = recv ? 1u : 0u;
        s.count[1] = after ? 1u : 0u;
        return key;
    }

    __device__ __forceinline__ void add(uint32_t key, const Sums& s) const
    {
        conn_run_add(state, key, n_conns, s.wide[0], s.wide[1], s.count[0], s.count[1]);
    }
};

// refview_accumulate plus the per-connection entries: the node-wide six sums take refview_accumulate's route
// unchanged, the entries walk_runs'. A connection's entry takes at most four adds per run and wave, and a
// one-connection batch 4 x (workgroups in the grid) adds.
template <bool NT, bool STRIDED>
__global__ void __launch_bounds__(kBlock)
    conn_accumulate(uint64_t arena_bytes, VSource src, uint32_t n, uint32_t base_index,
                    const uint32_t* __restrict__ conn_first_fail, uint32_t n_conns, uint64_t* __restrict__ ref,
                    cts_conn_state* __restrict__ state, uint32_t span)
{
    __shared__ uint64_t red[kBlock / 64][kCounterCount];
    uint32_t ring_first = kNone;
    if constexpr (STRIDED) ring_first = src.conn_index < n_conns ? conn_first_fail[src.conn_index] : kNone;
    ConnPass<NT, STRIDED> pass{arena_bytes, src, base_index, conn_first_fail, n_conns, state, ring_first, RefSums{}};
    walk_runs(pass, n, span);
    uint64_t v[kCounterCount];
    pass.node.reduce(v);
    block_add_six(v, red, ref);
}

// cts_conns_close: one lane per closed connection. Plain loads of the slot and the entry, the status, the result,
// then the empty slot and the zero entry; the class counts and the byte sum go to the close block's shard by the
// route of flush_counters. The ids and the expected sizes are read once (nontemporal with CTS_ATTR_NT_LOADS).
enum CloseSlot {
    kCloseClosed = 0,
    kCloseSuccessful = 1,
    kCloseDataErrors = 2,
    kCloseNotAllData = 3,
    kCloseTooMuchData = 4,
    kCloseBytesRecv = 5
};
static_assert(kCloseBytesRecv + 1 == kCounterCount, "a close block folds like a counter block");

template <bool NT>
__global__ void __launch_bounds__(kBlock)
    conn_close(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ expected, uint32_t n,
               uint32_t* __restrict__ conn_first_fail, cts_conn_state* __restrict__ state, uint32_t n_conns,
               cts_conn_result* __restrict__ results, uint64_t* __restrict__ block)
{
    __shared__ uint64_t red[kBlock / 64][kCounterCount];
    uint32_t closed = 0, successful = 0, data_errors = 0, not_all = 0, too_much = 0;
    uint64_t bytes = 0;
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
        const uint32_t c = NT ? __builtin_nontemporal_load(ids + i) : ids[i];
        cts_conn_result r = cts_conn_result{0, 0, 0, 0, 0u, 0u, c, 0u};
        if (c >= n_conns) {
            r.flags = CTS_CONN_RESULT_FLAG_BAD_CONN;
        } else {
            const uint32_t first = conn_first_fail[c];
            const cts_conn_state s = state[c];
            uint32_t status = 0u;
            if (first != kNone) {
                status = CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN;
                data_errors += 1u;
            } else if (expected != nullptr) {
                const uint64_t want = NT ? __builtin_nontemporal_load(expected + i) : expected[i];
                if (s.bytes_recv > want) {
                    status = CTS_STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED;
                    too_much += 1u;
                } else if (s.bytes_recv < want) {
                    status = CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED;
                    not_all += 1u;
                }
            }
            if (status == 0u) successful += 1u;
            closed += 1u;
            bytes += s.bytes_recv;
            r.bytes_recv = s.bytes_recv;
            r.buffers_recv = s.buffers_recv;
            r.bytes_after_failure = s.bytes_after_failure;
            r.buffers_after_failure = s.buffers_after_failure;
            r.first_fail = first;
            r.status = status;
            // the slot's next connection starts fresh
            conn_first_fail[c] = kNone;
            state[c] = cts_conn_state{0, 0, 0, 0};
        }
        if (results != nullptr) results[i] = r;
    }
    uint64_t v[kCounterCount];
    v[kCloseClosed] = wave_sum(closed);  // fewer than 2^32 ids per launch
    v[kCloseSuccessful] = wave_sum(successful);
    v[kCloseDataErrors] = wave_sum(data_errors);
    v[kCloseNotAllData] = wave_sum(not_all);
    v[kCloseTooMuchData] = wave_sum(too_much);
    v[kCloseBytesRecv] = wave_sum64(bytes);
    block_add_six(v, red, block);
}

// cts_conn_slots_rebase: one lane per slot, grid-stride. F -> F - delta, clamped at 0; empty slots stay empty.
__global__ void __launch_bounds__(kBlock) conn_slots_rebase(uint32_t* __restrict__ conn_first_fail, uint32_t n_conns,
                                                            uint32_t delta)
{
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_conns; i += step) {
        const uint32_t first = conn_first_fail[i];
        if (first != kNone) conn_first_fail[i] = first < delta ? 0u : first - delta;
    }
}

// ---------------------------------------------------------------------------------------------
// MediaStream connections on the device (cts_media_stream_conns.h): the accounting pass over a batch's descriptors
// and statuses (ms_conn_accumulate), the render tick (ms_conn_render) and the close (ms_conn_close). The receive pass
// that lowers the slots is ms_verify_status_ordinal, beside the MediaStream receive kernels below.
enum UdpSlot {
    kUdpBits = 0,
    kUdpSuccessful = 1,
    kUdpDropped = 2,
    kUdpDuplicate = 3,
    kUdpErrorFrames = 4,
    kUdpDatagrams = 5
};
static_assert(kUdpDatagrams + 1 == kCounterCount, "a UDP block folds like a counter block");

// What the accounting pass reads of one datagram: its connection (the descriptor's third 8 bytes) and its status.
struct MsMeta {
    uint32_t conn;
    int64_t seq;
    uint32_t completed;
    uint32_t fkp;  // flag | kind << 16 | pass << 24
};

template <bool NT>
__device__ __forceinline__ MsMeta ms_meta(const cts_buf_desc* __restrict__ descs,
                                          const cts_datagram_status* __restrict__ status, uint64_t i)
{
    const uint64_t* dp = reinterpret_cast<const uint64_t*>(descs + i) + 2;
    const uint64_t* sp = reinterpret_cast<const uint64_t*>(status + i);
    const uint64_t c = NT ? __builtin_nontemporal_load(dp) : dp[0];
    const uint64_t a = NT ? __builtin_nontemporal_load(sp) : sp[0];
    const uint64_t b = NT ? __builtin_nontemporal_load(sp + 1) : sp[1];
    return MsMeta{(uint32_t)c, (int64_t)a, (uint32_t)b, (uint32_t)(b >> 32)};
}

// One finished run of a connection's datagrams into its entry: at most four 64-bit adds and the sticky flag.
__device__ __forceinline__ void ms_run_add(cts_ms_conn_state* state, uint32_t conn, uint32_t n_conns, uint64_t bits,
                                           uint32_t dg, uint32_t after, uint32_t err, uint32_t in)
{
    if (conn >= n_conns) return;  // a connection without an entry (and kNone, the key of lanes that count nowhere)
    cts_ms_conn_state* e = state + conn;
    if (bits) atomicAdd((unsigned long long*)&e->bits_received, (unsigned long long)bits);
    if (err) atomicAdd((unsigned long long*)&e->error_frames, (unsigned long long)err);
    if (dg) atomicAdd((unsigned long long*)&e->datagrams, (unsigned long long)dg);
    if (after) atomicAdd((unsigned long long*)&e->datagrams_after_end, (unsigned long long)after);
    if (in) e->received_any = 1u;
}

// The walk, the segmented scan and the LDS join are walk_runs', written out here: as a pass of walk_runs (one 64-bit
// sum, four counts) this kernel's one-connection launch with the streams stopped measured 1-2 % above this form (192.4
// against 188.9 us over 16 Mi datagrams, profiles/ms_connections/README.md), so the copy stays until that is found.
// What is summed per
// run: the bits (64-bit) and four counts, packed a byte each inside a tile (each at most 64): datagrams, datagrams
// after the end, error frames, datagrams booked to the ring. Every datagram is judged against its connection's entry
// as the last tick left it (finished, head) and against the final slot; the one datagram with g == F stores the
// stream's error. Frame bytes go to the ring with one add per in-window datagram.
template <bool NT>
__global__ void __launch_bounds__(kBlock)
    ms_conn_accumulate(const cts_buf_desc* __restrict__ descs, const cts_datagram_status* __restrict__ status,
                       uint32_t n, uint32_t base_index, const uint32_t* __restrict__ conn_first_fail,
                       cts_ms_conn_state* state, uint64_t* __restrict__ frame_bytes, uint64_t frame_elems,
                       uint32_t n_conns, uint64_t* __restrict__ udp, uint32_t span)
{
    __shared__ uint64_t red[kBlock / 64][kCounterCount];
    __shared__ uint64_t tail_sum[kBlock / 64][5];
    __shared__ uint32_t tail_key[kBlock / 64][2];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lo = ((uint64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64) * span;
    const uint64_t hi = lo + span < (uint64_t)n ? lo + span : (uint64_t)n;  // lo >= n: an empty span
    uint64_t node_bits = 0;
    uint32_t node_err = 0, node_dg = 0;  // per lane: fewer than 2^32 datagrams per launch
    // the open run: the one that reached lane 63 of the previous tile (wave-uniform)
    uint32_t ckey = kNone, cdg = 0, cafter = 0, cerr = 0, cin = 0;
    uint64_t cbits = 0;
    bool whole = true;  // the span so far is one run (wave-uniform)
    // per-lane sums of the tiles that were nothing but the open run, not yet in cbits .. cin
    uint64_t pbits = 0;
    uint32_t pdg = 0, pafter = 0, perr = 0, pin = 0;
    bool parked = false;
    MsMeta mn = MsMeta{kNone, 0, 0u, 0u};
    if (lo < hi) mn = ms_meta<NT>(descs, status, lo + lane < hi ? lo + lane : hi - 1);
    for (uint64_t t = lo; t < hi; t += 64) {
        const uint64_t i = t + lane;
        const MsMeta m = mn;
        if (t + 64 < hi) mn = ms_meta<NT>(descs, status, i + 64 < hi ? i + 64 : hi - 1);  // the next tile, early
        const bool ok = i < hi;
        const uint32_t key = ok ? m.conn : kNone;
        const bool has = ok && m.conn < n_conns;  // a connection without a slot never fails and has no window
        uint32_t first = kNone, fin = 0u, frames = 0u;
        int64_t head = 0, final_frame = 0;
        uint64_t fbase = 0;
        if (has) {
            const cts_ms_conn_state* e = state + m.conn;
            first = conn_first_fail[m.conn];
            fin = e->finished;
            head = e->head_sequence_number;
            final_frame = e->final_frame;
            fbase = e->frame_base;
            frames = e->frames;
        }
        const uint32_t kind = (m.fkp >> 16) & 0xFFu;
        const bool clean = kind == CTS_DGRAM_DATA && (m.fkp >> 24) != 0u;
        const uint32_t g = base_index + (uint32_t)i;  // base_index + n <= 0xFFFFFFFF (checked by the entry point)
        uint64_t bits = 0;
        uint32_t dg = 0, after = 0, err = 0, in = 0;
        if (ok) {
            if (has && (fin != 0u || g > first)) {
                after = 1u;  // the renderer or a close ended the stream, or it failed on an earlier datagram
            } else {
                dg = 1u;
                if (has && g == first) {
                    // the datagram that fails the stream: UpdateLastError, once per connection
                    cts_ms_conn_state* e = state + m.conn;
                    e->last_error = kind == CTS_DGRAM_DATA ? CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN
                                                           : CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED;
                    e->has_failure = 1u;
                } else if (clean) {
                    bits = (uint64_t)m.completed * 8u;
                    if (has) {
                        // FindSequenceNumber: sequence number s sits at (s - 1) mod frames of the connection's ring
                        const bool inside = m.seq <= final_frame && m.seq >= head &&
                                            (uint64_t)(m.seq - head) < (uint64_t)frames;
                        const uint64_t at = inside ? fbase + (uint64_t)(m.seq - 1) % frames : frame_elems;
                        if (at < frame_elems) {
                            atomicAdd((unsigned long long*)&frame_bytes[at], (unsigned long long)m.completed);
                            in = 1u;
                        } else {
                            err = 1u;
                        }
                    }
                }
            }
        }
        node_bits += bits;
        node_err += err;
        node_dg += dg;
        // run heads, and for every lane the head of its run
        const uint32_t below = (uint32_t)__shfl_up((int)key, 1, 64);
        const bool rhead = lane == 0u || key != below;
        const uint64_t heads = __ballot(rhead);
        const uint32_t h = 63u - (uint32_t)__builtin_clzll(heads & (~0ull >> (63u - lane)));
        const bool merge = (uint32_t)__shfl((int)key, 0, 64) == ckey;
        if (heads == 1ull && merge) {
            // the whole tile goes on the open run: per-lane sums, no shuffle (they join the run when it is next needed)
            pbits += bits;
            pdg += dg;
            pafter += after;
            perr += err;
            pin += in;
            parked = true;
            continue;
        }
        if (parked) {
            cbits += wave_sum64(pbits);
            cdg += wave_sum(pdg);
            cafter += wave_sum(pafter);
            cerr += wave_sum(perr);
            cin += wave_sum(pin);
            pbits = 0;
            pdg = pafter = perr = pin = 0;
            parked = false;
        }
        // segmented inclusive scan: the bits, and the four counts a byte each (each <= 64)
        uint64_t a = bits;
        uint32_t c = dg | (after << 8) | (err << 16) | (in << 24);
#pragma unroll
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint64_t ua = (uint64_t)__shfl_up((unsigned long long)a, off, 64);
            const uint32_t uc = (uint32_t)__shfl_up((int)c, off, 64);
            if (lane >= h + off) {
                a += ua;
                c += uc;
            }
        }
        uint32_t rdg = c & 0xFFu, rafter = (c >> 8) & 0xFFu, rerr = (c >> 16) & 0xFFu, rin = c >> 24;
        // the open run goes on in lane 0's run, or ends here
        whole = whole && heads == 1ull && (merge || t == lo);
        if (merge && h == 0u) {
            a += cbits;
            rdg += cdg;
            rafter += cafter;
            rerr += cerr;
            rin += cin;
        }
        if (!merge && lane == 0u) ms_run_add(state, ckey, n_conns, cbits, cdg, cafter, cerr, cin);
        const bool tail = lane == 63u || ((heads >> (lane + 1u)) & 1ull) != 0ull;
        if (tail && lane != 63u) ms_run_add(state, key, n_conns, a, rdg, rafter, rerr, rin);
        ckey = (uint32_t)__shfl((int)key, 63, 64);
        cbits = (uint64_t)__shfl((unsigned long long)a, 63, 64);
        cdg = (uint32_t)__shfl((int)rdg, 63, 64);
        cafter = (uint32_t)__shfl((int)rafter, 63, 64);
        cerr = (uint32_t)__shfl((int)rerr, 63, 64);
        cin = (uint32_t)__shfl((int)rin, 63, 64);
    }
    if (parked) {
        cbits += wave_sum64(pbits);
        cdg += wave_sum(pdg);
        cafter += wave_sum(pafter);
        cerr += wave_sum(perr);
        cin += wave_sum(pin);
    }
    // the waves' last open runs meet in LDS, as in conn_accumulate
    if (lane == 0u) {
        tail_sum[threadIdx.x / 64][0] = cbits;
        tail_sum[threadIdx.x / 64][1] = cdg;
        tail_sum[threadIdx.x / 64][2] = cafter;
        tail_sum[threadIdx.x / 64][3] = cerr;
        tail_sum[threadIdx.x / 64][4] = cin;
        tail_key[threadIdx.x / 64][0] = ckey;
        tail_key[threadIdx.x / 64][1] = whole ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t key = tail_key[0][0];
        uint64_t acc[5] = {tail_sum[0][0], tail_sum[0][1], tail_sum[0][2], tail_sum[0][3], tail_sum[0][4]};
        for (int w = 1; w < kBlock / 64; ++w) {
            if (tail_key[w][1] == 0u || tail_key[w][0] != key) {
                ms_run_add(state, key, n_conns, acc[0], (uint32_t)acc[1], (uint32_t)acc[2], (uint32_t)acc[3],
                           (uint32_t)acc[4]);
                key = tail_key[w][0];
                acc[0] = acc[1] = acc[2] = acc[3] = acc[4] = 0;
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) acc[k] += tail_sum[w][k];
        }
        ms_run_add(state, key, n_conns, acc[0], (uint32_t)acc[1], (uint32_t)acc[2], (uint32_t)acc[3], (uint32_t)acc[4]);
    }
    uint64_t v[kCounterCount] = {0, 0, 0, 0, 0, 0};
    v[kUdpBits] = wave_sum64(node_bits);
    v[kUdpErrorFrames] = wave_sum(node_err);  // a wave's 64 lanes of one launch: still below 2^32
    v[kUdpDatagrams] = wave_sum(node_dg);
    block_add_six(v, red, udp);
}

// cts_media_stream_conns_render: one lane per listed connection, TimerCallback and RenderFrame
// (ctsIOPatternMediaStream.cpp:360-530) on its entry; the frame outcomes go to the UDP block's shard.
__global__ void __launch_bounds__(kBlock)
    ms_conn_render(const uint32_t* __restrict__ ids, uint32_t n, cts_ms_conn_state* state,
                   uint64_t* __restrict__ frame_bytes, uint32_t n_conns, uint64_t* __restrict__ udp,
                   uint32_t* __restrict__ codes)
{
    __shared__ uint64_t red[kBlock / 64][kCounterCount];
    uint32_t successful = 0, duplicate = 0;
    uint64_t dropped = 0;  // a FatalAbort drops final_frame frames at once
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
        const uint32_t c = ids[i];
        uint32_t code = 0u;
        if (c < n_conns) {
            cts_ms_conn_state* e = state + c;
            if (e->last_error != CTS_STATUS_IO_RUNNING || e->frames == 0u) {
                code = e->finished;  // failed, ended or closed earlier: not rendered again
            } else {
                const uint32_t wheel = e->timer_wheel_offset + 1u;
                e->timer_wheel_offset = wheel;
                int64_t head = e->head_sequence_number;
                const int64_t final_frame = e->final_frame;
                if (wheel >= e->initial_buffer_frames && head <= final_frame) {
                    if (e->received_any == 0u && head == 1) {
                        // "have received nothing from the server": every frame counts as dropped, FatalAbort
                        e->dropped_frames += (uint64_t)final_frame;
                        dropped += (uint64_t)final_frame;
                        e->finished = CTS_MS_CONN_FATAL;
                        e->last_error = CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED;
                        code = 2u;
                    } else {
                        uint64_t* slot = frame_bytes + e->frame_base + (uint64_t)(head - 1) % e->frames;
                        const uint64_t got = *slot;
                        if (got == (uint64_t)e->frame_size_bytes) {
                            e->successful_frames += 1u;
                            successful += 1u;
                        } else if (got < (uint64_t)e->frame_size_bytes) {
                            e->dropped_frames += 1u;
                            dropped += 1u;
                        } else {
                            e->duplicate_frames += 1u;
                            duplicate += 1u;
                        }
                        *slot = 0;
                        head += 1;
                        e->head_sequence_number = head;
                    }
                }
                if (code == 0u && head > final_frame) {
                    e->finished = CTS_MS_CONN_FINISHED;
                    e->last_error = 0u;
                    code = 1u;
                }
            }
        }
        if (codes != nullptr) codes[i] = code;
    }
    uint64_t v[kCounterCount] = {0, 0, 0, 0, 0, 0};
    v[kUdpSuccessful] = wave_sum(successful);  // fewer than 2^32 ids per launch
    v[kUdpDropped] = wave_sum64(dropped);
    v[kUdpDuplicate] = wave_sum(duplicate);
    block_add_six(v, red, udp);
}

// cts_media_stream_conns_close: one wave per closed connection. Every lane reads the entry (one broadcast line), the
// wave zeroes the connection's ring, lane 0 writes the result, empties the slot and leaves the entry ended; the class
// counts and the byte sum go to the close block's shard by the route of conn_close.
__global__ void __launch_bounds__(kBlock)
    ms_conn_close(const uint32_t* __restrict__ ids, uint32_t n, uint32_t* __restrict__ conn_first_fail,
                  cts_ms_conn_state* state, uint64_t* __restrict__ frame_bytes, uint32_t n_conns,
                  cts_ms_conn_result* __restrict__ results, uint64_t* __restrict__ block)
{
    __shared__ uint64_t red[kBlock / 64][kCounterCount];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t step = (uint64_t)gridDim.x * (kBlock / 64);
    uint32_t closed = 0, successful = 0, data_errors = 0, not_all = 0;  // wave-uniform
    uint64_t bytes = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * (kBlock / 64) + threadIdx.x / 64; i < n; i += step) {
        const uint32_t c = ids[i];
        cts_ms_conn_result r = cts_ms_conn_result{0, 0, 0, 0, 0, 0, 0, 0, kNone, 0u, 0u, c, 0u, 0u};
        if (c >= n_conns) {
            r.flags = CTS_MS_CONN_RESULT_FLAG_BAD_CONN;
        } else {
            cts_ms_conn_state* e = state + c;
            const cts_ms_conn_state s = *e;
            uint32_t status = s.last_error;
            if (status == CTS_STATUS_IO_RUNNING) {
                // the device's own rule: a client closed while its renderer still runs did not get all its data
                status = CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED;
                r.flags |= CTS_MS_CONN_RESULT_FLAG_RUNNING;
            }
            if (status == 0u) successful += 1u;
            else if (status == CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN) data_errors += 1u;
            else not_all += 1u;
            closed += 1u;
            bytes += s.bits_received / 8u;
            r.bits_received = s.bits_received;
            r.successful_frames = s.successful_frames;
            r.dropped_frames = s.dropped_frames;
            r.duplicate_frames = s.duplicate_frames;
            r.error_frames = s.error_frames;
            r.datagrams = s.datagrams;
            r.datagrams_after_end = s.datagrams_after_end;
            r.head_sequence_number = s.head_sequence_number;
            if (s.has_failure != 0u) {
                r.flags |= CTS_MS_CONN_RESULT_FLAG_HAS_FAILURE;
                r.fail_datagram = (uint32_t)(s.datagrams - 1u);
            }
            r.first_fail = conn_first_fail[c];
            r.status = status;
            r.finished = s.finished;
            for (uint64_t k = lane; k < (uint64_t)s.frames; k += 64) frame_bytes[s.frame_base + k] = 0;
            if (lane == 0u) {
                // late datagrams count as after the end until a fresh entry is written over this one
                conn_first_fail[c] = kNone;
                e->last_error = status;
                e->finished = s.finished != 0u ? s.finished : CTS_MS_CONN_CLOSED;
            }
        }
        if (results != nullptr && lane == 0u) results[i] = r;
    }
    uint64_t v[kCounterCount] = {0, 0, 0, 0, 0, 0};
    v[kCloseClosed] = closed;
    v[kCloseSuccessful] = successful;
    v[kCloseDataErrors] = data_errors;
    v[kCloseNotAllData] = not_all;
    v[kCloseBytesRecv] = bytes;
    block_add_six(v, red, block);
}

// ---------------------------------------------------------------------------------------------
// The launchers. Every grid is item_grid's (cts_spans.hpp): one item per lane (per wave for ms_conn_close), capped per
// CU; the kernels go grid-stride beyond the cap.
static_assert(kSpanBlock == (uint32_t)kBlock, "cts_spans.hpp describes these kernels' workgroups");

// cts_refview_accumulate(_strided): one descriptor per lane
template <bool STRIDED>
static hipError_t launch_refview_src(uint64_t arena_bytes, const VSource& src, uint32_t n, uint32_t base_index,
                                     const uint32_t* conn_first_fail, uint32_t n_conns, uint64_t* ref_counters,
                                     hipStream_t stream, const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    const uint32_t grid = item_grid(n, kBlock, geo.num_cus);
    if (geo.nontemporal)
        refview_accumulate<true, STRIDED><<<grid, kBlock, 0, stream>>>(arena_bytes, src, n, base_index, conn_first_fail,
                                                                       n_conns, ref_counters);
    else
        refview_accumulate<false, STRIDED><<<grid, kBlock, 0, stream>>>(arena_bytes, src, n, base_index, conn_first_fail,
                                                                        n_conns, ref_counters);
    return hipGetLastError();
}

hipError_t launch_refview(uint64_t arena_bytes, const cts_buf_desc* descs, uint32_t n, uint32_t base_index,
                          const uint32_t* conn_first_fail, uint32_t n_conns, uint64_t* ref_counters, hipStream_t stream,
                          const LaunchGeometry& geo)
{
    return launch_refview_src<false>(arena_bytes, VSource{descs, nullptr, 0u, 0u, 0u, 0u}, n, base_index,
                                     conn_first_fail, n_conns, ref_counters, stream, geo);
}

hipError_t launch_refview_strided(uint64_t arena_bytes, uint32_t stride, const uint32_t* lens, uint32_t n,
                                  uint32_t skip_head, uint32_t conn_index, uint32_t base_index,
                                  const uint32_t* conn_first_fail, uint32_t n_conns, uint64_t* ref_counters,
                                  hipStream_t stream, const LaunchGeometry& geo)
{
    // expected offset 0: the pass reads no pattern, the field only carries vs_desc's length > stride rule
    return launch_refview_src<true>(arena_bytes, VSource{nullptr, lens, stride, skip_head, 0u, conn_index}, n,
                                    base_index, conn_first_fail, n_conns, ref_counters, stream, geo);
}

// cts_refview_accumulate_conns(_strided): refview's grid; every wave of it takes one contiguous span of the batch, a
// multiple of 64 descriptors (span_geometry, cts_spans.hpp)
template <bool STRIDED>
static hipError_t launch_conn_accumulate_src(uint64_t arena_bytes, const VSource& src, uint32_t n, uint32_t base_index,
                                             const uint32_t* conn_first_fail, uint32_t n_conns, uint64_t* ref_counters,
                                             cts_conn_state* conn_state, hipStream_t stream, const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    const SpanGeometry sg = span_geometry(n, geo.num_cus);
    const uint32_t grid = sg.grid, span = sg.span;
    if (geo.nontemporal)
        conn_accumulate<true, STRIDED><<<grid, kBlock, 0, stream>>>(arena_bytes, src, n, base_index, conn_first_fail,
                                                                    n_conns, ref_counters, conn_state, span);
    else
        conn_accumulate<false, STRIDED><<<grid, kBlock, 0, stream>>>(arena_bytes, src, n, base_index, conn_first_fail,
                                                                     n_conns, ref_counters, conn_state, span);
    return hipGetLastError();
}

hipError_t launch_conn_accumulate(uint64_t arena_bytes, const cts_buf_desc* descs, uint32_t n, uint32_t base_index,
                                  const uint32_t* conn_first_fail, uint32_t n_conns, uint64_t* ref_counters,
                                  cts_conn_state* conn_state, hipStream_t stream, const LaunchGeometry& geo)
{
    return launch_conn_accumulate_src<false>(arena_bytes, VSource{descs, nullptr, 0u, 0u, 0u, 0u}, n, base_index,
                                             conn_first_fail, n_conns, ref_counters, conn_state, stream, geo);
}

hipError_t launch_conn_accumulate_strided(uint64_t arena_bytes, uint32_t stride, const uint32_t* lens, uint32_t n,
                                          uint32_t skip_head, uint32_t conn_index, uint32_t base_index,
                                          const uint32_t* conn_first_fail, uint32_t n_conns, uint64_t* ref_counters,
                                          cts_conn_state* conn_state, hipStream_t stream, const LaunchGeometry& geo)
{
    return launch_conn_accumulate_src<true>(arena_bytes, VSource{nullptr, lens, stride, skip_head, 0u, conn_index}, n,
                                            base_index, conn_first_fail, n_conns, ref_counters, conn_state, stream,
                                            geo);
}

// one lane per id (cts_conns_close) or per slot (cts_conn_slots_rebase)
hipError_t launch_conn_close(const uint32_t* conn_ids, const uint64_t* expected_bytes, uint32_t n,
                             uint32_t* conn_first_fail, cts_conn_state* conn_state, uint32_t n_conns,
                             cts_conn_result* results, uint64_t* close_counters, hipStream_t stream,
                             const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    const uint32_t grid = item_grid(n, kBlock, geo.num_cus);
    if (geo.nontemporal)
        conn_close<true><<<grid, kBlock, 0, stream>>>(conn_ids, expected_bytes, n, conn_first_fail, conn_state, n_conns,
                                                      results, close_counters);
    else
        conn_close<false><<<grid, kBlock, 0, stream>>>(conn_ids, expected_bytes, n, conn_first_fail, conn_state,
                                                       n_conns, results, close_counters);
    return hipGetLastError();
}

hipError_t launch_conn_slots_rebase(uint32_t* conn_first_fail, uint32_t n_conns, uint32_t delta, hipStream_t stream,
                                    const LaunchGeometry& geo)
{
    if (n_conns == 0 || delta == 0) return hipSuccess;
    conn_slots_rebase<<<item_grid(n_conns, kBlock, geo.num_cus), kBlock, 0, stream>>>(conn_first_fail, n_conns, delta);
    return hipGetLastError();
}

// cts_media_stream_conns_accumulate: conn_accumulate's grid and spans
hipError_t launch_ms_conn_accumulate(const cts_buf_desc* descs, const cts_datagram_status* status, uint32_t n,
                                     uint32_t base_index, const uint32_t* conn_first_fail, cts_ms_conn_state* conns,
                                     uint64_t* frame_bytes, uint64_t frame_elems, uint32_t n_conns,
                                     uint64_t* udp_counters, hipStream_t stream, const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    const SpanGeometry sg = span_geometry(n, geo.num_cus);
    const uint32_t grid = sg.grid, span = sg.span;
    if (geo.nontemporal)
        ms_conn_accumulate<true><<<grid, kBlock, 0, stream>>>(descs, status, n, base_index, conn_first_fail, conns,
                                                              frame_bytes, frame_elems, n_conns, udp_counters, span);
    else
        ms_conn_accumulate<false><<<grid, kBlock, 0, stream>>>(descs, status, n, base_index, conn_first_fail, conns,
                                                               frame_bytes, frame_elems, n_conns, udp_counters, span);
    return hipGetLastError();
}

hipError_t launch_ms_conn_render(const uint32_t* conn_ids, uint32_t n, cts_ms_conn_state* conns, uint64_t* frame_bytes,
                                 uint32_t n_conns, uint64_t* udp_counters, uint32_t* codes, hipStream_t stream,
                                 const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    ms_conn_render<<<item_grid(n, kBlock, geo.num_cus), kBlock, 0, stream>>>(conn_ids, n, conns, frame_bytes, n_conns,
                                                                             udp_counters, codes);
    return hipGetLastError();
}

// one wave per id
hipError_t launch_ms_conn_close(const uint32_t* conn_ids, uint32_t n, uint32_t* conn_first_fail,
                                cts_ms_conn_state* conns, uint64_t* frame_bytes, uint32_t n_conns,
                                cts_ms_conn_result* results, uint64_t* close_counters, hipStream_t stream,
                                const LaunchGeometry& geo)
{
    if (n == 0) return hipSuccess;
    ms_conn_close<<<item_grid(n, kBlock / 64, geo.num_cus), kBlock, 0, stream>>>(conn_ids, n, conn_first_fail, conns,
                                                                                frame_bytes, n_conns, results,
                                                                                close_counters);
    return hipGetLastError();
}

}  // namespace cts
