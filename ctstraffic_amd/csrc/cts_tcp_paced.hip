// cts_tcp_paced.hip — the planning of the paced TCP senders' tick (cts_tcp_senders_send_paced, cts_tcp_senders.h):
// cts_tcp_senders_send's three-launch scheme (cts_fill.hip) with every listed connection's wanted slots cut to what
// CreateNewTask's send branch (ctsIOPattern.cpp:593-674) lets out at now_ms, from a 64-byte pace entry per connection.
//
//   tcp_paced_sums    each tile's sum of wants; the pace machine runs on a register copy, nothing is stored
//   tcp_paced_scan    one workgroup: exclusive scan of the tile sums in place, prefix[n] = the grand total, the 48-byte
//                     tick block zeroed and its next_due_ms set to INT64_MAX
//   tcp_paced_apply   the machine again, p_i, the taken count t_i, the codes, both entries' updates, the tick with its
//                     tail and the sent block
//
// The descriptor pass and the fill are the plain tick's launches, unchanged: they read prefix, before and the tick
// block's first 32 bytes.
//
// A translation unit of its own: the kernels of cts_fill.hip keep their instruction text whatever is compiled here
// (DESIGN §3). For the same reason the tile scan and the limb-wise wave sum are restated here instead of being moved
// out of cts_fill.hip into a header.
#include <hip/hip_runtime.h>

#include "cts_chunks.hpp"
#include "cts_internal.hpp"

namespace cts {

static_assert(sizeof(cts_tcp_sender_pace) == 64 && alignof(cts_tcp_sender_pace) == 8, "cts_tcp_sender_pace: 64 bytes");
static_assert(sizeof(cts_tcp_sender_paced_tick) == 48 && offsetof(cts_tcp_sender_paced_tick, next_due_ms) == 32,
              "cts_tcp_sender_paced_tick: a plain tick and 16 bytes");
static_assert(kMsServerTile == (uint32_t)kBlock, "one listed connection per thread of a tile");

namespace {

constexpr int64_t kNoDue = INT64_MAX;

// The members of a pace entry that a tick reads, in registers; save() stores the five that a tick moves.
struct PaceRegs {
    int64_t per, cur, start, due;
    uint32_t period, burst_count, burst_left, burst_delay, pending;

    __device__ __forceinline__ void load(const cts_tcp_sender_pace* __restrict__ q)
    {
        per = q->bytes_per_quantum;
        cur = q->bytes_this_quantum;
        start = q->quantum_start_ms;
        due = q->due_ms;
        period = q->quantum_period_ms;
        burst_count = q->burst_count;
        burst_left = q->burst_left;
        burst_delay = q->burst_delay_ms;
        pending = q->pending;
    }
    __device__ __forceinline__ void save(cts_tcp_sender_pace* __restrict__ q) const
    {
        q->bytes_this_quantum = cur;
        q->quantum_start_ms = start;
        q->due_ms = due;
        q->burst_left = burst_left;
        q->pending = pending;
    }
    // no rate limit, no burst setting, nothing waiting: the plain tick's connection
    __device__ __forceinline__ bool unpaced() const { return per <= 0 && burst_count == 0u && pending == 0u; }

    // CreateNewTask's send branch for a send of `size` bytes at `now` (ctsIOPattern.cpp:593-674, as cts_pattern.cpp's
    // SendTimeOffset states it): the task's time offset. One 64-bit division at the most: either the quanta that now
    // has skipped or the quanta that the carried bytes fill, never both.
    __device__ __forceinline__ int64_t step(int64_t now, int64_t size)
    {
        int64_t offset = 0;
        if (per > 0) {
            const int64_t T = (int64_t)period;
            const bool room = cur < per;
            const bool past = room && now > start + T;
            int64_t q = 0;
            if (past || !room) q = (room ? now - start : cur) / (room ? T : per);
            if (room) {
                cur += size;
                if (past) {
                    // now past this quantum: move to the one we are in, and take back the bytes the skipped quanta
                    // would have carried (never below zero)
                    start += q * T;
                    const int64_t adjust = per * q;
                    cur = adjust > cur ? 0 : cur - adjust;
                }
            } else {
                // this quantum (and maybe more) is already full: carry the excess, defer this send to the end of the
                // quanta it fills
                const int64_t skip_ms = (q - 1) * T;
                cur -= per * q;
                cur += size;
                if (now < start + T) offset = start + T - now;
                offset += skip_ms;
                start += skip_ms + T;
            }
        } else if (burst_count != 0u) {
            if (burst_left == 0u) burst_left = burst_count;
            burst_left -= 1u;
            if (burst_left == 0u) offset = (int64_t)burst_delay;
        }
        return offset;
    }

    // run(cap) of cts_tcp_senders.h; cap <= ceil(R / B), so bytes are left at every step. The loop's length differs
    // from lane to lane: a wave takes as long as its longest lane.
    __device__ __forceinline__ uint32_t run(int64_t now, uint32_t cap, uint64_t R, uint32_t B)
    {
        uint32_t count = 0;
        uint64_t left = R;
        while (count < cap) {
            const uint64_t size = left < (uint64_t)B ? left : (uint64_t)B;
            if (pending != 0u) {
                if (now < due) break;
                pending = 0u;
            } else {
                const int64_t off = step(now, (int64_t)size);
                if (off > 0) {
                    pending = 1u;
                    due = now + off;
                    break;
                }
            }
            ++count;
            left -= size;
        }
        return count;
    }
};

// The plain tick's wanted slots of connection c, its code when it sends nothing whatever the room or the time, and R
// and B of a running connection (tcp_sender_want of cts_fill.hip).
__device__ __forceinline__ uint32_t tcp_paced_limit(const cts_tcp_sender_state* __restrict__ senders, uint32_t c,
                                                    uint32_t n_conns, uint32_t stride, uint32_t max_buffers,
                                                    uint32_t& code, uint64_t& R, uint32_t& B)
{
    code = CTS_TCP_SENDER_SKIPPED;
    R = 0u;
    B = 0u;
    if (c >= n_conns) return 0u;
    B = senders[c].buffer_size;
    if (B == 0u || B > stride) return 0u;
    code = CTS_TCP_SENDER_ENDED;
    const uint64_t sent = senders[c].bytes_sent, transfer = senders[c].transfer_bytes;
    if (senders[c].finished != 0u || sent >= transfer) return 0u;
    code = CTS_TCP_SENDER_SENT;
    R = transfer - sent;
    const uint64_t k = R / B + (R % B != 0u ? 1u : 0u);
    return k < (uint64_t)max_buffers ? (uint32_t)k : max_buffers;
}

// Listed connection c's wanted slots at now_ms: the limit, or run(limit) on Q, a register copy of its pace entry.
// paced = Q holds the entry and has been moved.
__device__ __forceinline__ uint32_t tcp_paced_want(const cts_tcp_sender_state* __restrict__ senders,
                                                   const cts_tcp_sender_pace* __restrict__ pace, uint32_t c,
                                                   uint32_t n_conns, uint32_t stride, uint32_t max_buffers,
                                                   int64_t now, uint32_t& code, uint64_t& R, uint32_t& B, PaceRegs& Q,
                                                   bool& paced)
{
    paced = false;
    const uint32_t limit = tcp_paced_limit(senders, c, n_conns, stride, max_buffers, code, R, B);
    if (code != CTS_TCP_SENDER_SENT) return 0u;
    Q.load(pace + c);
    if (Q.unpaced()) return limit;
    paced = true;
    return Q.run(now, limit, R, B);
}

// tile_scan_exclusive of cts_fill.hip: exclusive scan of v over the workgroup's kBlock threads; total = the
// workgroup's sum. Ends with a barrier: wsum is free again.
__device__ __forceinline__ uint64_t tcp_paced_tile_scan(uint64_t v, uint64_t* wsum, uint64_t& total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint64_t u = (uint64_t)__shfl_up((unsigned long long)inc, off, 64);
        if (lane >= off) inc += u;
    }
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    uint64_t base = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kBlock / 64u; ++w) {
        if (w < wave) base += wsum[w];
        total += wsum[w];
    }
    __syncthreads();
    return base + inc - v;
}

// tcp_wave_sum64 of cts_fill.hip: a wave's 64-bit sum from four 16-bit limbs summed in 32 bits.
__device__ __forceinline__ uint64_t tcp_paced_wave_sum64(uint64_t v)
{
    uint64_t s = 0;
#pragma unroll
    for (int l = 0; l < 4; ++l) s += (uint64_t)wave_sum((uint32_t)(v >> (16 * l)) & 0xFFFFu) << (16 * l);
    return s;
}

__device__ __forceinline__ int64_t tcp_paced_wave_min(int64_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t u = (int64_t)__shfl_xor((long long)v, off, 64);
        v = u < v ? u : v;
    }
    return v;
}

}  // namespace

__global__ void __launch_bounds__(kBlock)
    tcp_paced_sums(const uint32_t* __restrict__ ids, uint32_t n, const cts_tcp_sender_state* __restrict__ senders,
                   const cts_tcp_sender_pace* __restrict__ pace, uint32_t n_conns, uint32_t stride,
                   uint32_t max_buffers, int64_t now, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t wsum[kBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kMsServerTile + threadIdx.x;
    uint64_t want = 0;
    if (i < n) {
        uint32_t code, B;
        uint64_t R;
        PaceRegs Q{};
        bool paced;
        want = tcp_paced_want(senders, pace, ids[i], n_conns, stride, max_buffers, now, code, R, B, Q, paced);
    }
    const uint64_t s = tcp_paced_wave_sum64(want);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) t += wsum[w];
        sums[blockIdx.x] = t;
    }
}

// One workgroup. tick is 12 dwords (cts_tcp_sender_paced_tick); its next_due_ms starts at INT64_MAX.
__global__ void __launch_bounds__(kBlock)
    tcp_paced_scan(uint64_t* __restrict__ sums, uint64_t tiles, uint64_t* __restrict__ prefix_total,
                   uint32_t* __restrict__ tick)
{
    __shared__ uint64_t wsum[kBlock / 64];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < tiles; base += kBlock) {
        const uint64_t t = base + threadIdx.x;
        const uint64_t v = t < tiles ? sums[t] : 0u;
        uint64_t total;
        const uint64_t ex = tcp_paced_tile_scan(v, wsum, total);
        if (t < tiles) sums[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0u) *prefix_total = carry;
    constexpr uint32_t kDue = offsetof(cts_tcp_sender_paced_tick, next_due_ms) / 4u;
    if (threadIdx.x < sizeof(cts_tcp_sender_paced_tick) / 4u)
        tick[threadIdx.x] = threadIdx.x == kDue ? 0xFFFFFFFFu : threadIdx.x == kDue + 1u ? 0x7FFFFFFFu : 0u;
}

__global__ void __launch_bounds__(kBlock)
    tcp_paced_apply(const uint32_t* __restrict__ ids, uint32_t n, cts_tcp_sender_state* __restrict__ senders,
                    cts_tcp_sender_pace* __restrict__ pace, uint32_t n_conns, uint32_t stride, uint32_t capacity,
                    uint32_t max_buffers, int64_t now, const uint64_t* __restrict__ sums,
                    uint64_t* __restrict__ prefix, uint64_t* __restrict__ before, uint32_t* __restrict__ codes,
                    cts_tcp_sender_paced_tick* __restrict__ tick, uint64_t* __restrict__ sent_block)
{
    __shared__ uint64_t wsum[kBlock / 64];
    __shared__ uint64_t ctr[kBlock / 64][kCounterCount];
    __shared__ uint32_t red[kBlock / 64][7];
    __shared__ int64_t due[kBlock / 64];
    zero_counters<kBlock / 64>(ctr);
    const uint64_t i = (uint64_t)blockIdx.x * kMsServerTile + threadIdx.x;
    uint32_t code = CTS_TCP_SENDER_SENT, c = 0u, B = 0u;
    uint64_t want = 0, R = 0;
    PaceRegs Q{};
    bool paced = false;
    if (i < n) {
        c = ids[i];
        want = tcp_paced_want(senders, pace, c, n_conns, stride, max_buffers, now, code, R, B, Q, paced);
    }
    uint64_t total;
    const uint64_t p = sums[blockIdx.x] + tcp_paced_tile_scan(want, wsum, total);
    uint64_t bytes = 0;
    int64_t my_due = kNoDue;
    uint32_t buffers = 0, sent = 0, finished = 0, no_room = 0, skipped = 0, waiting = 0, pending = 0;
    if (i < n) {
        prefix[i] = p;
        const uint64_t pc = p < (uint64_t)capacity ? p : (uint64_t)capacity;
        const uint64_t t = want < (uint64_t)capacity - pc ? want : (uint64_t)capacity - pc;
        uint64_t was = 0;
        if (code != CTS_TCP_SENDER_SENT) {
            skipped = 1u;
        } else if (want == 0u) {
            // pacing lets nothing out: the sender entry stays, the pace entry may hold a new pending task
            waiting = 1u;
            code = CTS_TCP_SENDER_WAITING;
            Q.save(pace + c);
        } else if (t == 0u) {
            no_room = 1u;
            code = CTS_TCP_SENDER_NO_ROOM;
            if (paced) Q.load(pace + c);  // both entries stay: what counts below is the stored entry
        } else {
            if (paced) {
                if (t < want) {  // cut by the capacity: the machine moves t steps from the stored entry
                    Q.load(pace + c);
                    (void)Q.run(now, (uint32_t)t, R, B);
                }
                Q.save(pace + c);
            }
            // the only step that knows how many slots the connection takes is the one that moves its entry
            cts_tcp_sender_state* e = senders + c;
            was = e->bytes_sent;
            const uint64_t full = t * B;  // t <= capacity < 2^32
            bytes = full < R ? full : R;
            buffers = (uint32_t)t;
            sent = 1u;
            e->bytes_sent = was + bytes;
            e->buffers_sent += t;
            if (bytes == R) {
                e->finished = 1u;
                finished = 1u;
                code = CTS_TCP_SENDER_FINISHED;
            }
        }
        if (skipped == 0u && Q.pending != 0u) {
            pending = 1u;
            my_due = Q.due;
        }
        before[i] = was;
        if (codes != nullptr) codes[i] = code;
    }
    const uint64_t own_bytes = tcp_paced_wave_sum64(bytes);
    buffers = wave_sum(buffers);
    sent = wave_sum(sent);
    finished = wave_sum(finished);
    no_room = wave_sum(no_room);
    skipped = wave_sum(skipped);
    waiting = wave_sum(waiting);
    pending = wave_sum(pending);
    my_due = tcp_paced_wave_min(my_due);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        ctr[wave][0] = own_bytes;  // cts_counters_sent.bytes_sent (TcpStatusDetails.m_bytesSent, ctsIOPattern.cpp:510)
        ctr[wave][1] = buffers;    // .buffers_sent
        ctr[wave][2] = finished;   // .connections_finished
        red[wave][0] = buffers;
        red[wave][1] = sent;
        red[wave][2] = finished;
        red[wave][3] = no_room;
        red[wave][4] = skipped;
        red[wave][5] = waiting;
        red[wave][6] = pending;
        due[wave] = my_due;
    }
    flush_counters<kBlock / 64>(sent_block, ctr);  // barrier first
    if (threadIdx.x < 7u) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) s += red[w][threadIdx.x];
        // buffers, connections_sent, _finished, _no_room, _skipped; then the tail's connections_waiting, _pending
        uint32_t* const word = threadIdx.x < 5u ? &tick->tick.buffers + threadIdx.x
                                                : &tick->connections_waiting + (threadIdx.x - 5u);
        if (s) atomicAdd(word, s);
    } else if (threadIdx.x == 7u) {
        uint64_t s = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) s += ctr[w][0];
        if (s) atomicAdd((unsigned long long*)&tick->tick.bytes, (unsigned long long)s);
    } else if (threadIdx.x == 8u) {
        // one 64-bit minimum per workgroup, and none where nothing is pending
        int64_t m = kNoDue;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) m = due[w] < m ? due[w] : m;
        if (m != kNoDue) atomicMin((long long*)&tick->next_due_ms, (long long)m);
    }
}

// cts_tcp_senders_send_paced's planning: three launches, the middle one a single workgroup
hipError_t launch_tcp_paced_plan(const uint32_t* conn_ids, uint32_t n, uint32_t max_buffers,
                                 cts_tcp_sender_state* senders, cts_tcp_sender_pace* pace, uint32_t n_conns,
                                 int64_t now_ms, uint32_t stride, uint32_t capacity, uint32_t* codes,
                                 cts_tcp_sender_paced_tick* tick, uint64_t* sent_counters,
                                 const TcpPacedScratch& scratch, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const uint64_t tiles = ms_server_tiles(n);
    tcp_paced_sums<<<(uint32_t)tiles, kBlock, 0, stream>>>(conn_ids, n, senders, pace, n_conns, stride, max_buffers,
                                                           now_ms, scratch.plain.sums);
    tcp_paced_scan<<<1, kBlock, 0, stream>>>(scratch.plain.sums, tiles, scratch.plain.prefix + n,
                                             reinterpret_cast<uint32_t*>(tick));
    tcp_paced_apply<<<(uint32_t)tiles, kBlock, 0, stream>>>(conn_ids, n, senders, pace, n_conns, stride, capacity,
                                                            max_buffers, now_ms, scratch.plain.sums,
                                                            scratch.plain.prefix, scratch.plain.before, codes, tick,
                                                            sent_counters);
    return hipGetLastError();
}

}  // namespace cts
