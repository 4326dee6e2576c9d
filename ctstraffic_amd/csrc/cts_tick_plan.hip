// cts_tick_plan.hip — the planning of a device-resident sender's tick for gfx950: which ring slots every listed
// connection takes, with no pattern byte written. Five ticks plan the same way (cts_media_stream_servers_send,
// cts_tcp_senders_send, cts_tcp_senders_send_paced, cts_tcp_exchange_send, cts_tcp_exchange_send_paced): listed
// connection i wants w_i slots (0 when it sends nothing whatever the room); p_i, the exclusive 64-bit prefix of the
// wants in listed order, is its first slot, and the room left at p_i decides what it takes. Three plain launches in
// tiles of kPlanTile listed connections (no workgroup ever waits for another):
//   *_sums    each tile's sum of wants                              -> sums[tile]
//   *_scan    one workgroup: exclusive scan of the tile sums in place in passes of kBlock tiles, prefix[n] = the grand
//             total, the tick block initialised
//   *_apply   p_i = sums[tile] + the tile's own scan -> prefix[i]; the code, the entries' updates, the tick block and
//             the counter block
//   ms_server_sums / _scan / _apply     the MediaStream servers: a connection sends its whole frame or nothing
//   tcp_sender_sums / _apply            the TCP senders (with ms_server_scan: both tick blocks are eight dwords)
//   tcp_paced_sums / _scan / _apply     the paced TCP senders: the wants cut to what CreateNewTask's send branch
//                                       (ctsIOPattern.cpp:593-674) lets out at now_ms, from a pace entry per connection
//   tcp_exchange_sums / _scan / _apply  the exchange tick (cts_tcp_exchange_send): Push, Pull, PushPull and Duplex
//                                       connections, the wants counted in buffers of a fixed sequence
//   tcp_exchange_paced_sums / _scan / _apply  the paced exchange tick (cts_tcp_exchange_send_paced): those wants cut
//                                       by the pace entries of the two sides, one walk over directions and quanta
// Each step of the scheme is written once here (the tile scan, the tile-sum tail, the scan's passes, the TCP limit, the
// TCP entry move, the apply tail). What writes the ring from prefix[] is in cts_fill.hip, beside the loops it shares
// with the other fills.
// Scratch (MsServerScratch, TcpSenderScratch, TcpPacedScratch of cts_internal.hpp): u64 prefix[n + 1], u64 sums[tiles],
// for the TCP senders u64 before[n], and a tick.
#include <hip/hip_runtime.h>

#include "cts_chunks.hpp"
#include "cts_internal.hpp"
#include "cts_tcp_exchange_math.hpp"

namespace cts {

static_assert(sizeof(cts_tcp_exchange_tick) == 48 && offsetof(cts_tcp_exchange_tick, bytes_dir) == 32,
              "cts_tcp_exchange_tick: a plain tick and 16 bytes");
static_assert(kPlanTile == (uint32_t)kBlock, "one listed connection per thread of a tile");
static_assert(sizeof(cts_tcp_sender_tick) == sizeof(cts_ms_server_tick), "ms_server_scan zeroes either tick block");
static_assert(sizeof(cts_tcp_sender_pace) == 64 && alignof(cts_tcp_sender_pace) == 8, "cts_tcp_sender_pace: 64 bytes");
static_assert(sizeof(cts_tcp_sender_paced_tick) == 48 && offsetof(cts_tcp_sender_paced_tick, next_due_ms) == 32,
              "cts_tcp_sender_paced_tick: a plain tick and 16 bytes");

namespace {

// ---------------------------------------------------------------------------------------------
// The steps every planner shares.

// Exclusive scan of v over the workgroup's kBlock threads (wave scans, then the waves' sums through wsum); total = the
// workgroup's sum. Ends with a barrier: wsum is free again.
__device__ __forceinline__ uint64_t tile_scan_exclusive(uint64_t v, uint64_t* wsum, uint64_t& total)
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

// The tail of a *_sums kernel: the tile's sum of wants -> sums[blockIdx.x].
__device__ __forceinline__ void tile_sum_store(uint64_t want, uint64_t* wsum, uint64_t* __restrict__ sums)
{
    const uint64_t s = wave_sum64(want);
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) t += wsum[w];
        sums[blockIdx.x] = t;
    }
}

// The body of a *_scan kernel (one workgroup): sums[] becomes its own exclusive scan, kBlock tiles a pass with the
// passes' carry; the grand total is returned to every thread.
__device__ __forceinline__ uint64_t tile_sums_scan(uint64_t* __restrict__ sums, uint64_t tiles, uint64_t* wsum)
{
    uint64_t carry = 0;
    for (uint64_t base = 0; base < tiles; base += kBlock) {
        const uint64_t t = base + threadIdx.x;
        const uint64_t v = t < tiles ? sums[t] : 0u;
        uint64_t total;
        const uint64_t ex = tile_scan_exclusive(v, wsum, total);
        if (t < tiles) sums[t] = carry + ex;
        carry += total;
    }
    return carry;
}

// The tail of an *_apply kernel: words[] and bytes are a wave's sums of the tick's WORDS 32-bit words and of its byte
// count, and the kernel has filled its wave's row of ctr. The counter block takes ctr, tick word k the workgroup's sum
// through word(k), *tick_bytes the workgroup's bytes. wsum is the tile scan's, free since that scan's last barrier.
template <int WORDS, typename Word>
__device__ __forceinline__ void apply_flush(const uint32_t (&words)[WORDS], uint64_t bytes, uint32_t (*red)[WORDS],
                                            uint64_t* wsum, uint64_t (*ctr)[kCounterCount], uint64_t* counters,
                                            Word word, uint64_t* tick_bytes)
{
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < WORDS; ++k) red[threadIdx.x >> 6][k] = words[k];
        wsum[threadIdx.x >> 6] = bytes;
    }
    flush_counters<kBlock / 64>(counters, ctr);  // barrier first
    if (threadIdx.x < (uint32_t)WORDS) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) s += red[w][threadIdx.x];
        if (s) atomicAdd(word(threadIdx.x), s);
    } else if (threadIdx.x == (uint32_t)WORDS) {
        uint64_t s = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) s += wsum[w];
        if (s) atomicAdd((unsigned long long*)tick_bytes, (unsigned long long)s);
    }
}

// Beside apply_flush, for the ticks whose block has more than words and bytes: thread `at` of the workgroup takes the
// minimum of the waves' due[] to *tick_due (one 64-bit atomicMin per workgroup, none where nothing is pending), and
// threads at, at + 1 add the waves' dir[][0 .. 1] to tick_dir. Both arrays are written before apply_flush's barrier.
constexpr int64_t kNoDue = INT64_MAX;

__device__ __forceinline__ void apply_flush_due(const int64_t* due, int64_t* tick_due, uint32_t at)
{
    if (threadIdx.x == at) {
        int64_t m = kNoDue;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) m = due[w] < m ? due[w] : m;
        if (m != kNoDue) atomicMin((long long*)tick_due, (long long)m);
    }
}

__device__ __forceinline__ void apply_flush_dir(const uint64_t (*dir)[2], uint64_t* tick_dir, uint32_t at)
{
    if (threadIdx.x >= at && threadIdx.x < at + 2u) {
        const uint32_t d = threadIdx.x - at;
        uint64_t s = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) s += dir[w][d];
        if (s) atomicAdd((unsigned long long*)&tick_dir[d], (unsigned long long)s);
    }
}

// ---------------------------------------------------------------------------------------------
// MediaStream servers (cts_media_stream_servers_send): listed connection i wants k_i = datagrams_per_frame slots and
// sends when p_i + k_i <= capacity. p is monotonic, so the connections that send are a prefix of those that want and
// the tick's datagrams are the slots [0, total) with no gap. ms_server_fill (cts_fill.hip) writes the ring from
// prefix[] and the entries.

// The slots listed connection c wants, and its code when it sends nothing whatever the room.
__device__ __forceinline__ uint32_t ms_server_want(const cts_ms_server_state* __restrict__ servers, uint32_t c,
                                                   uint32_t n_conns, uint32_t stride, uint32_t& code)
{
    code = CTS_MS_SERVER_SKIPPED;
    if (c >= n_conns) return 0u;
    if (servers[c].finished != 0u) {
        code = CTS_MS_SERVER_ENDED;
        return 0u;
    }
    if (servers[c].datagram_max_size > stride) return 0u;
    code = CTS_MS_SERVER_SENT;
    return servers[c].datagrams_per_frame;
}

}  // namespace

__global__ void __launch_bounds__(kBlock)
    ms_server_sums(const uint32_t* __restrict__ ids, uint32_t n, const cts_ms_server_state* __restrict__ servers,
                   uint32_t n_conns, uint32_t stride, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t wsum[kBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint32_t code;
    const uint64_t want = i < n ? ms_server_want(servers, ids[i], n_conns, stride, code) : 0u;
    tile_sum_store(want, wsum, sums);
}

// One workgroup. tick is 8 dwords (cts_ms_server_tick, cts_tcp_sender_tick).
__global__ void __launch_bounds__(kBlock)
    ms_server_scan(uint64_t* __restrict__ sums, uint64_t tiles, uint64_t* __restrict__ prefix_total,
                   uint32_t* __restrict__ tick)
{
    __shared__ uint64_t wsum[kBlock / 64];
    const uint64_t total = tile_sums_scan(sums, tiles, wsum);
    if (threadIdx.x == 0u) *prefix_total = total;
    if (threadIdx.x < sizeof(cts_ms_server_tick) / 4u) tick[threadIdx.x] = 0u;
}

__global__ void __launch_bounds__(kBlock)
    ms_server_apply(const uint32_t* __restrict__ ids, uint32_t n, cts_ms_server_state* __restrict__ servers,
                    uint32_t n_conns, uint32_t stride, uint32_t capacity, const uint64_t* __restrict__ sums,
                    uint64_t* __restrict__ prefix, uint32_t* __restrict__ codes, cts_ms_server_tick* __restrict__ tick,
                    uint64_t* __restrict__ udp)
{
    __shared__ uint64_t wsum[kBlock / 64];
    __shared__ uint64_t ctr[kBlock / 64][kCounterCount];
    __shared__ uint32_t red[kBlock / 64][5];
    zero_counters<kBlock / 64>(ctr);
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint32_t code = CTS_MS_SERVER_SENT, c = 0u;
    uint64_t want = 0;
    if (i < n) {
        c = ids[i];
        want = ms_server_want(servers, c, n_conns, stride, code);
    }
    uint64_t total;
    const uint64_t p = sums[blockIdx.x] + tile_scan_exclusive(want, wsum, total);
    uint64_t bytes = 0;
    uint32_t datagrams = 0, sent = 0, finished = 0, no_room = 0, skipped = 0;
    if (i < n) {
        prefix[i] = p;
        if (code != CTS_MS_SERVER_SENT) {
            skipped = 1u;
        } else if (p + want > (uint64_t)capacity) {
            no_room = 1u;
            code = CTS_MS_SERVER_NO_ROOM;
        } else {
            // the only step that knows whether the connection fits is the one that moves its entry
            cts_ms_server_state* e = servers + c;
            bytes = e->frame_size_bytes;
            datagrams = (uint32_t)want;
            sent = 1u;
            e->bits_sent += 8u * bytes;
            e->datagrams_sent += want;
            const int64_t next = e->current_frame + 1;
            e->current_frame = next;
            if (next > e->final_frame) {
                e->finished = 1u;
                finished = 1u;
                code = CTS_MS_SERVER_FINISHED;
            }
        }
        if (codes != nullptr) codes[i] = code;
    }
    bytes = wave_sum64(bytes);
    // datagrams, connections_sent, _finished, _no_room, _skipped
    const uint32_t words[5] = {wave_sum(datagrams), wave_sum(sent), wave_sum(finished), wave_sum(no_room),
                               wave_sum(skipped)};
    if ((threadIdx.x & 63u) == 0u) {
        // the reference's server adds its sent bits to UdpStatusDetails.m_bitsReceived (ctsIOPattern.cpp:1162)
        ctr[threadIdx.x >> 6][0] = 8u * bytes;                 // cts_counters_udp.bits_received
        ctr[threadIdx.x >> 6][kCounterCount - 1] = words[0];  // cts_counters_udp.datagrams
    }
    apply_flush(words, bytes, red, wsum, ctr, udp, [&](uint32_t k) { return &tick->datagrams + k; }, &tick->bytes);
}

// cts_media_stream_servers_send's planning: three launches, the middle one a single workgroup
hipError_t launch_ms_server_plan(const uint32_t* conn_ids, uint32_t n, cts_ms_server_state* servers, uint32_t n_conns,
                                 uint32_t stride, uint32_t capacity, uint32_t* codes, cts_ms_server_tick* tick,
                                 uint64_t* udp_counters, const MsServerScratch& scratch, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const uint64_t tiles = plan_tiles(n);
    ms_server_sums<<<(uint32_t)tiles, kBlock, 0, stream>>>(conn_ids, n, servers, n_conns, stride, scratch.sums);
    ms_server_scan<<<1, kBlock, 0, stream>>>(scratch.sums, tiles, scratch.prefix + n,
                                             reinterpret_cast<uint32_t*>(tick));
    ms_server_apply<<<(uint32_t)tiles, kBlock, 0, stream>>>(conn_ids, n, servers, n_conns, stride, capacity,
                                                            scratch.sums, scratch.prefix, codes, tick, udp_counters);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// TCP senders (cts_tcp_senders_send): listed connection i wants w_i = min(max_buffers, ceil(R / B)) slots and takes
// t_i = min(w_i, capacity - min(p_i, capacity)) of them. apply also leaves every listed connection's bytes_sent from
// before the move in the scratch; tcp_sender_descs and the fill (cts_fill.hip) read prefix, before and the tick.

namespace {

// The slots listed connection c wants whatever the time, its code when it sends nothing whatever the room or the time,
// and R (bytes left) and B (buffer size) of a running connection.
__device__ __forceinline__ uint32_t tcp_sender_limit(const cts_tcp_sender_state* __restrict__ senders, uint32_t c,
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

// Entry e takes t > 0 slots of B bytes with R bytes left: the bytes it sends; was = its bytes_sent before, ended =
// the transfer is complete. The only step that knows how many slots a connection takes is the one that moves its entry.
__device__ __forceinline__ uint64_t tcp_sender_move(cts_tcp_sender_state* e, uint64_t t, uint64_t R, uint32_t B,
                                                    uint64_t& was, bool& ended)
{
    was = e->bytes_sent;
    const uint64_t full = t * B;  // t <= capacity < 2^32
    const uint64_t bytes = full < R ? full : R;
    e->bytes_sent = was + bytes;
    e->buffers_sent += t;
    ended = bytes == R;
    if (ended) e->finished = 1u;
    return bytes;
}

}  // namespace

__global__ void __launch_bounds__(kBlock)
    tcp_sender_sums(const uint32_t* __restrict__ ids, uint32_t n, const cts_tcp_sender_state* __restrict__ senders,
                    uint32_t n_conns, uint32_t stride, uint32_t max_buffers, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t wsum[kBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint64_t want = 0;
    if (i < n) {
        uint32_t code, B;
        uint64_t R;
        want = tcp_sender_limit(senders, ids[i], n_conns, stride, max_buffers, code, R, B);
    }
    tile_sum_store(want, wsum, sums);
}

__global__ void __launch_bounds__(kBlock)
    tcp_sender_apply(const uint32_t* __restrict__ ids, uint32_t n, cts_tcp_sender_state* __restrict__ senders,
                     uint32_t n_conns, uint32_t stride, uint32_t capacity, uint32_t max_buffers,
                     const uint64_t* __restrict__ sums, uint64_t* __restrict__ prefix, uint64_t* __restrict__ before,
                     uint32_t* __restrict__ codes, cts_tcp_sender_tick* __restrict__ tick, uint64_t* __restrict__ sent_block)
{
    __shared__ uint64_t wsum[kBlock / 64];
    __shared__ uint64_t ctr[kBlock / 64][kCounterCount];
    __shared__ uint32_t red[kBlock / 64][5];
    zero_counters<kBlock / 64>(ctr);
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint32_t code = CTS_TCP_SENDER_SENT, c = 0u, B = 0u;
    uint64_t want = 0, R = 0;
    if (i < n) {
        c = ids[i];
        want = tcp_sender_limit(senders, c, n_conns, stride, max_buffers, code, R, B);
    }
    uint64_t total;
    const uint64_t p = sums[blockIdx.x] + tile_scan_exclusive(want, wsum, total);
    uint64_t bytes = 0;
    uint32_t buffers = 0, sent = 0, finished = 0, no_room = 0, skipped = 0;
    if (i < n) {
        prefix[i] = p;
        const uint64_t pc = p < (uint64_t)capacity ? p : (uint64_t)capacity;
        const uint64_t t = want < (uint64_t)capacity - pc ? want : (uint64_t)capacity - pc;
        uint64_t was = 0;
        if (code != CTS_TCP_SENDER_SENT) {
            skipped = 1u;
        } else if (t == 0u) {
            no_room = 1u;
            code = CTS_TCP_SENDER_NO_ROOM;
        } else {
            bool ended;
            bytes = tcp_sender_move(senders + c, t, R, B, was, ended);
            buffers = (uint32_t)t;
            sent = 1u;
            if (ended) {
                finished = 1u;
                code = CTS_TCP_SENDER_FINISHED;
            }
        }
        before[i] = was;
        if (codes != nullptr) codes[i] = code;
    }
    bytes = wave_sum64(bytes);
    // buffers, connections_sent, _finished, _no_room, _skipped
    const uint32_t words[5] = {wave_sum(buffers), wave_sum(sent), wave_sum(finished), wave_sum(no_room),
                               wave_sum(skipped)};
    if ((threadIdx.x & 63u) == 0u) {
        uint64_t* const own = ctr[threadIdx.x >> 6];
        own[0] = bytes;     // cts_counters_sent.bytes_sent (TcpStatusDetails.m_bytesSent, ctsIOPattern.cpp:510)
        own[1] = words[0];  // .buffers_sent
        own[2] = words[2];  // .connections_finished
    }
    apply_flush(words, bytes, red, wsum, ctr, sent_block, [&](uint32_t k) { return &tick->buffers + k; },
                &tick->bytes);
}

// cts_tcp_senders_send's planning: three launches, the middle one the servers' single-workgroup scan
hipError_t launch_tcp_sender_plan(const uint32_t* conn_ids, uint32_t n, uint32_t max_buffers,
                                  cts_tcp_sender_state* senders, uint32_t n_conns, uint32_t stride, uint32_t capacity,
                                  uint32_t* codes, cts_tcp_sender_tick* tick, uint64_t* sent_counters,
                                  const TcpSenderScratch& scratch, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const uint64_t tiles = plan_tiles(n);
    tcp_sender_sums<<<(uint32_t)tiles, kBlock, 0, stream>>>(conn_ids, n, senders, n_conns, stride, max_buffers,
                                                            scratch.sums);
    ms_server_scan<<<1, kBlock, 0, stream>>>(scratch.sums, tiles, scratch.prefix + n,
                                             reinterpret_cast<uint32_t*>(tick));
    tcp_sender_apply<<<(uint32_t)tiles, kBlock, 0, stream>>>(conn_ids, n, senders, n_conns, stride, capacity,
                                                             max_buffers, scratch.sums, scratch.prefix, scratch.before,
                                                             codes, tick, sent_counters);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Paced TCP senders (cts_tcp_senders_send_paced): the plain tick with every listed connection's wanted slots cut to what
// its 64-byte pace entry lets out at now_ms.
//   tcp_paced_sums    the pace machine runs on a register copy, nothing is stored
//   tcp_paced_scan    the 48-byte tick block zeroed and its next_due_ms set to INT64_MAX
//   tcp_paced_apply   the machine again, p_i, the taken count t_i, the codes, both entries' updates, the tick with its
//                     tail and the sent block
// The descriptor pass and the fill are the plain tick's launches, unchanged: they read prefix, before and the tick
// block's first 32 bytes.

namespace {

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

// Listed connection c's wanted slots at now_ms: the limit, or run(limit) on Q, a register copy of its pace entry.
// paced = Q holds the entry and has been moved.
__device__ __forceinline__ uint32_t tcp_paced_want(const cts_tcp_sender_state* __restrict__ senders,
                                                   const cts_tcp_sender_pace* __restrict__ pace, uint32_t c,
                                                   uint32_t n_conns, uint32_t stride, uint32_t max_buffers,
                                                   int64_t now, uint32_t& code, uint64_t& R, uint32_t& B, PaceRegs& Q,
                                                   bool& paced)
{
    paced = false;
    const uint32_t limit = tcp_sender_limit(senders, c, n_conns, stride, max_buffers, code, R, B);
    if (code != CTS_TCP_SENDER_SENT) return 0u;
    Q.load(pace + c);
    if (Q.unpaced()) return limit;
    paced = true;
    return Q.run(now, limit, R, B);
}

__device__ __forceinline__ int64_t wave_min64(int64_t v)
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
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint64_t want = 0;
    if (i < n) {
        uint32_t code, B;
        uint64_t R;
        PaceRegs Q{};
        bool paced;
        want = tcp_paced_want(senders, pace, ids[i], n_conns, stride, max_buffers, now, code, R, B, Q, paced);
    }
    tile_sum_store(want, wsum, sums);
}

// One workgroup. tick is 12 dwords (cts_tcp_sender_paced_tick); its next_due_ms starts at INT64_MAX.
__global__ void __launch_bounds__(kBlock)
    tcp_paced_scan(uint64_t* __restrict__ sums, uint64_t tiles, uint64_t* __restrict__ prefix_total,
                   uint32_t* __restrict__ tick)
{
    __shared__ uint64_t wsum[kBlock / 64];
    const uint64_t total = tile_sums_scan(sums, tiles, wsum);
    if (threadIdx.x == 0u) *prefix_total = total;
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
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint32_t code = CTS_TCP_SENDER_SENT, c = 0u, B = 0u;
    uint64_t want = 0, R = 0;
    PaceRegs Q{};
    bool paced = false;
    if (i < n) {
        c = ids[i];
        want = tcp_paced_want(senders, pace, c, n_conns, stride, max_buffers, now, code, R, B, Q, paced);
    }
    uint64_t total;
    const uint64_t p = sums[blockIdx.x] + tile_scan_exclusive(want, wsum, total);
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
            bool ended;
            bytes = tcp_sender_move(senders + c, t, R, B, was, ended);
            buffers = (uint32_t)t;
            sent = 1u;
            if (ended) {
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
    bytes = wave_sum64(bytes);
    // buffers, connections_sent, _finished, _no_room, _skipped; then the tail's connections_waiting, _pending
    const uint32_t words[7] = {wave_sum(buffers), wave_sum(sent),    wave_sum(finished), wave_sum(no_room),
                               wave_sum(skipped), wave_sum(waiting), wave_sum(pending)};
    my_due = wave_min64(my_due);
    if ((threadIdx.x & 63u) == 0u) {
        uint64_t* const own = ctr[threadIdx.x >> 6];
        own[0] = bytes;     // cts_counters_sent.bytes_sent (TcpStatusDetails.m_bytesSent, ctsIOPattern.cpp:510)
        own[1] = words[0];  // .buffers_sent
        own[2] = words[2];  // .connections_finished
        due[threadIdx.x >> 6] = my_due;
    }
    apply_flush(
        words, bytes, red, wsum, ctr, sent_block,
        [&](uint32_t k) { return k < 5u ? &tick->tick.buffers + k : &tick->connections_waiting + (k - 5u); },
        &tick->tick.bytes);
    apply_flush_due(due, &tick->next_due_ms, 8u);
}

// cts_tcp_senders_send_paced's planning: three launches, the middle one a single workgroup
hipError_t launch_tcp_paced_plan(const uint32_t* conn_ids, uint32_t n, uint32_t max_buffers,
                                 cts_tcp_sender_state* senders, cts_tcp_sender_pace* pace, uint32_t n_conns,
                                 int64_t now_ms, uint32_t stride, uint32_t capacity, uint32_t* codes,
                                 cts_tcp_sender_paced_tick* tick, uint64_t* sent_counters,
                                 const TcpPacedScratch& scratch, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const uint64_t tiles = plan_tiles(n);
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

// ---------------------------------------------------------------------------------------------
// The exchange tick (cts_tcp_exchange_send): Push, Pull, PushPull and Duplex connections from 64-byte entries. Listed
// connection i wants w_i = min(max_buffers, N - buffers_sent) slots of its buffer sequence and takes t_i as the TCP
// senders do; whose turn each buffer is follows from its index (cts_tcp_exchange_math.hpp), so the planning never
// looks at a direction: the move asks the closed form where the entry stands t buffers on.
//   tcp_exchange_sums    the wants
//   tcp_exchange_scan    ms_server_scan with the 48-byte tick block zeroed
//   tcp_exchange_apply   p_i, t_i, the codes, the entries' moves, the tick with its bytes by direction, the sent block
// apply leaves every listed connection's buffers_sent from before the move in the scratch; tcp_exchange_descs
// (cts_fill.hip) reads prefix, before and the tick.

namespace {

// The slots listed connection c wants, its code when it sends nothing whatever the room, and of a running connection
// the entry's constants S and its position m.
__device__ __forceinline__ uint32_t tcp_exchange_limit(const cts_tcp_exchange_state* __restrict__ entries, uint32_t c,
                                                       uint32_t n_conns, uint32_t stride, uint32_t max_buffers,
                                                       uint32_t& code, ExchangeShape& S, uint64_t& m)
{
    code = CTS_TCP_SENDER_SKIPPED;
    m = 0u;
    if (c >= n_conns) return 0u;
    S = exchange_shape(entries + c);
    if (!exchange_shape_ok(S) || S.B > stride) return 0u;
    code = CTS_TCP_SENDER_ENDED;
    m = entries[c].buffers_sent;
    if (entries[c].finished != 0u || m >= S.N) return 0u;
    code = CTS_TCP_SENDER_SENT;
    const uint64_t k = S.N - m;
    return k < (uint64_t)max_buffers ? (uint32_t)k : max_buffers;
}

// Entry e at position m takes t > 0 slots: the bytes it sends by direction; true = the sequence is complete. The only
// step that knows how many slots a connection takes is the one that moves its entry: the bytes of buffers m .. m + t by
// direction are the difference of two positions, whatever segment ends lie between, and the entry holds the position
// at m (cts_tcp_exchange_init, _seek and this move keep it so).
__device__ __forceinline__ bool tcp_exchange_move(cts_tcp_exchange_state* e, const ExchangeShape& S, uint64_t m,
                                                  uint64_t t, uint64_t& bytes0, uint64_t& bytes1)
{
    uint64_t to[2];
    exchange_position(S, m + t, to);
    bytes0 = exchange_sub(to[0], e->bytes_sent[0]);
    bytes1 = exchange_sub(to[1], e->bytes_sent[1]);
    e->bytes_sent[0] += bytes0;
    e->bytes_sent[1] += bytes1;
    e->buffers_sent = m + t;
    const bool ended = m + t == S.N;
    if (ended) e->finished = 1u;
    return ended;
}

}  // namespace

__global__ void __launch_bounds__(kBlock)
    tcp_exchange_sums(const uint32_t* __restrict__ ids, uint32_t n, const cts_tcp_exchange_state* __restrict__ entries,
                      uint32_t n_conns, uint32_t stride, uint32_t max_buffers, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t wsum[kBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint64_t want = 0;
    if (i < n) {
        uint32_t code;
        ExchangeShape S{};
        uint64_t m;
        want = tcp_exchange_limit(entries, ids[i], n_conns, stride, max_buffers, code, S, m);
    }
    tile_sum_store(want, wsum, sums);
}

// One workgroup. tick is 12 dwords (cts_tcp_exchange_tick).
__global__ void __launch_bounds__(kBlock)
    tcp_exchange_scan(uint64_t* __restrict__ sums, uint64_t tiles, uint64_t* __restrict__ prefix_total,
                      uint32_t* __restrict__ tick)
{
    __shared__ uint64_t wsum[kBlock / 64];
    const uint64_t total = tile_sums_scan(sums, tiles, wsum);
    if (threadIdx.x == 0u) *prefix_total = total;
    if (threadIdx.x < sizeof(cts_tcp_exchange_tick) / 4u) tick[threadIdx.x] = 0u;
}

__global__ void __launch_bounds__(kBlock)
    tcp_exchange_apply(const uint32_t* __restrict__ ids, uint32_t n, cts_tcp_exchange_state* __restrict__ entries,
                       uint32_t n_conns, uint32_t stride, uint32_t capacity, uint32_t max_buffers,
                       const uint64_t* __restrict__ sums, uint64_t* __restrict__ prefix, uint64_t* __restrict__ before,
                       uint32_t* __restrict__ codes, cts_tcp_exchange_tick* __restrict__ tick,
                       uint64_t* __restrict__ sent_block)
{
    __shared__ uint64_t wsum[kBlock / 64];
    __shared__ uint64_t ctr[kBlock / 64][kCounterCount];
    __shared__ uint32_t red[kBlock / 64][5];
    __shared__ uint64_t dir[kBlock / 64][2];
    zero_counters<kBlock / 64>(ctr);
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint32_t code = CTS_TCP_SENDER_SENT, c = 0u;
    uint64_t want = 0, m = 0;
    ExchangeShape S{};
    if (i < n) {
        c = ids[i];
        want = tcp_exchange_limit(entries, c, n_conns, stride, max_buffers, code, S, m);
    }
    uint64_t total;
    const uint64_t p = sums[blockIdx.x] + tile_scan_exclusive(want, wsum, total);
    uint64_t bytes0 = 0, bytes1 = 0;
    uint32_t buffers = 0, sent = 0, finished = 0, no_room = 0, skipped = 0;
    if (i < n) {
        prefix[i] = p;
        const uint64_t pc = p < (uint64_t)capacity ? p : (uint64_t)capacity;
        const uint64_t t = want < (uint64_t)capacity - pc ? want : (uint64_t)capacity - pc;
        if (code != CTS_TCP_SENDER_SENT) {
            skipped = 1u;
        } else if (t == 0u) {
            no_room = 1u;
            code = CTS_TCP_SENDER_NO_ROOM;
        } else {
            buffers = (uint32_t)t;
            sent = 1u;
            if (tcp_exchange_move(entries + c, S, m, t, bytes0, bytes1)) {
                finished = 1u;
                code = CTS_TCP_SENDER_FINISHED;
            }
        }
        before[i] = m;
        if (codes != nullptr) codes[i] = code;
    }
    bytes0 = wave_sum64(bytes0);
    bytes1 = wave_sum64(bytes1);
    const uint64_t bytes = bytes0 + bytes1;
    // buffers, connections_sent, _finished, _no_room, _skipped
    const uint32_t words[5] = {wave_sum(buffers), wave_sum(sent), wave_sum(finished), wave_sum(no_room),
                               wave_sum(skipped)};
    if ((threadIdx.x & 63u) == 0u) {
        uint64_t* const own = ctr[threadIdx.x >> 6];
        own[0] = bytes;     // cts_counters_sent.bytes_sent (TcpStatusDetails.m_bytesSent of whichever side sent)
        own[1] = words[0];  // .buffers_sent
        own[2] = words[2];  // .connections_finished
        dir[threadIdx.x >> 6][0] = bytes0;
        dir[threadIdx.x >> 6][1] = bytes1;
    }
    apply_flush(words, bytes, red, wsum, ctr, sent_block, [&](uint32_t k) { return &tick->tick.buffers + k; },
                &tick->tick.bytes);
    apply_flush_dir(dir, tick->bytes_dir, 8u);
}

// cts_tcp_exchange_send's planning: three launches, the middle one a single workgroup
hipError_t launch_tcp_exchange_plan(const uint32_t* conn_ids, uint32_t n, uint32_t max_buffers,
                                    cts_tcp_exchange_state* entries, uint32_t n_conns, uint32_t stride,
                                    uint32_t capacity, uint32_t* codes, cts_tcp_exchange_tick* tick,
                                    uint64_t* sent_counters, const TcpExchangeScratch& scratch, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const uint64_t tiles = plan_tiles(n);
    tcp_exchange_sums<<<(uint32_t)tiles, kBlock, 0, stream>>>(conn_ids, n, entries, n_conns, stride, max_buffers,
                                                              scratch.plain.sums);
    tcp_exchange_scan<<<1, kBlock, 0, stream>>>(scratch.plain.sums, tiles, scratch.plain.prefix + n,
                                                reinterpret_cast<uint32_t*>(tick));
    tcp_exchange_apply<<<(uint32_t)tiles, kBlock, 0, stream>>>(conn_ids, n, entries, n_conns, stride, capacity,
                                                               max_buffers, scratch.plain.sums, scratch.plain.prefix,
                                                               scratch.plain.before, codes, tick, sent_counters);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The paced exchange tick (cts_tcp_exchange_send_paced): the exchange tick with every listed connection's wanted slots
// cut by run_x of cts_tcp_exchange.h, the pace machine's walk with each step taken on the pace entry of the next
// buffer's direction (entry c + d x n_conns: the side that sends direction d).
//   tcp_exchange_paced_sums    the walk on register copies, nothing is stored
//   tcp_exchange_paced_scan    the 64-byte tick block zeroed and its next_due_ms set to INT64_MAX
//   tcp_exchange_paced_apply   the walk again, p_i, t_i, the codes, the entry's move (tcp_exchange_move), the pace
//                              entries' updates, the tick with bytes_dir and the tail, the sent block
// The walk pays exchange_element's division once: an ExchangeCursor is seeded at m and moved by additions. A lane keeps
// both directions' pace registers, `cur` for the next buffer's direction and `oth`, and swaps them when the direction
// flips, so no register is ever indexed by a direction. tcp_exchange_descs and the fill follow unchanged: they read
// prefix, before and the block's first 32 bytes.

static_assert(sizeof(cts_tcp_exchange_paced_tick) == 64 && offsetof(cts_tcp_exchange_paced_tick, next_due_ms) == 48 &&
                  offsetof(cts_tcp_exchange_paced_tick, connections_waiting) == 56,
              "cts_tcp_exchange_paced_tick: an exchange tick and the paced tick's 16-byte tail");

namespace {

// A listed connection's two pace entries in registers. two = the pattern sends both ways (PushPull, Duplex); a one-way
// pattern never loads, moves or saves `oth`, whose registers stay zero.
struct ExchangePace {
    PaceRegs cur, oth;
    ExchangeCursor at;
    bool two;

    __device__ __forceinline__ void load(const cts_tcp_sender_pace* __restrict__ pace, uint32_t c, uint32_t n_conns,
                                         const ExchangeShape& S, uint64_t m)
    {
        at.seed(S, m);
        two = S.pattern >= CTS_TCP_EXCHANGE_PUSHPULL;
        cur.load(pace + ((uint64_t)c + (uint64_t)at.d * n_conns));
        if (two) oth.load(pace + ((uint64_t)c + (uint64_t)(at.d ^ 1u) * n_conns));
    }
    __device__ __forceinline__ void save(cts_tcp_sender_pace* __restrict__ pace, uint32_t c, uint32_t n_conns) const
    {
        cur.save(pace + ((uint64_t)c + (uint64_t)at.d * n_conns));
        if (two) oth.save(pace + ((uint64_t)c + (uint64_t)(at.d ^ 1u) * n_conns));
    }
    __device__ __forceinline__ bool unpaced() const { return cur.unpaced() && (!two || oth.unpaced()); }

    // run_x(cap) of cts_tcp_exchange.h; cap <= N - m. PaceRegs::run's loop with the size and the entry taken from the
    // cursor. A wave takes as long as its longest lane.
    __device__ __forceinline__ uint32_t run(int64_t now, uint32_t cap, const ExchangeShape& S)
    {
        uint32_t count = 0;
        while (count < cap) {
            const uint32_t size = at.len(S);
            if (cur.pending != 0u) {
                if (now < cur.due) break;
                cur.pending = 0u;
            } else {
                const int64_t off = cur.step(now, (int64_t)size);
                if (off > 0) {
                    cur.pending = 1u;
                    cur.due = now + off;
                    break;
                }
            }
            ++count;
            if (at.advance(S, size)) {
                const PaceRegs was = cur;
                cur = oth;
                oth = was;
            }
        }
        return count;
    }
};

// Listed connection c's wanted slots at now_ms: the limit, or run_x(limit) on X, register copies of its pace entries.
// paced = X holds the entries and has been moved.
__device__ __forceinline__ uint32_t tcp_exchange_paced_want(const cts_tcp_exchange_state* __restrict__ entries,
                                                            const cts_tcp_sender_pace* __restrict__ pace, uint32_t c,
                                                            uint32_t n_conns, uint32_t stride, uint32_t max_buffers,
                                                            int64_t now, uint32_t& code, ExchangeShape& S, uint64_t& m,
                                                            ExchangePace& X, bool& paced)
{
    paced = false;
    const uint32_t limit = tcp_exchange_limit(entries, c, n_conns, stride, max_buffers, code, S, m);
    if (code != CTS_TCP_SENDER_SENT) return 0u;
    X.load(pace, c, n_conns, S, m);
    if (X.unpaced()) return limit;
    paced = true;
    return X.run(now, limit, S);
}

}  // namespace

__global__ void __launch_bounds__(kBlock)
    tcp_exchange_paced_sums(const uint32_t* __restrict__ ids, uint32_t n,
                            const cts_tcp_exchange_state* __restrict__ entries,
                            const cts_tcp_sender_pace* __restrict__ pace, uint32_t n_conns, uint32_t stride,
                            uint32_t max_buffers, int64_t now, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t wsum[kBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint64_t want = 0;
    if (i < n) {
        uint32_t code;
        ExchangeShape S{};
        uint64_t m;
        ExchangePace X{};
        bool paced;
        want = tcp_exchange_paced_want(entries, pace, ids[i], n_conns, stride, max_buffers, now, code, S, m, X, paced);
    }
    tile_sum_store(want, wsum, sums);
}

// One workgroup. tick is 16 dwords (cts_tcp_exchange_paced_tick); its next_due_ms starts at INT64_MAX.
__global__ void __launch_bounds__(kBlock)
    tcp_exchange_paced_scan(uint64_t* __restrict__ sums, uint64_t tiles, uint64_t* __restrict__ prefix_total,
                            uint32_t* __restrict__ tick)
{
    __shared__ uint64_t wsum[kBlock / 64];
    const uint64_t total = tile_sums_scan(sums, tiles, wsum);
    if (threadIdx.x == 0u) *prefix_total = total;
    constexpr uint32_t kDue = offsetof(cts_tcp_exchange_paced_tick, next_due_ms) / 4u;
    if (threadIdx.x < sizeof(cts_tcp_exchange_paced_tick) / 4u)
        tick[threadIdx.x] = threadIdx.x == kDue ? 0xFFFFFFFFu : threadIdx.x == kDue + 1u ? 0x7FFFFFFFu : 0u;
}

__global__ void __launch_bounds__(kBlock)
    tcp_exchange_paced_apply(const uint32_t* __restrict__ ids, uint32_t n,
                             cts_tcp_exchange_state* __restrict__ entries, cts_tcp_sender_pace* __restrict__ pace,
                             uint32_t n_conns, uint32_t stride, uint32_t capacity, uint32_t max_buffers, int64_t now,
                             const uint64_t* __restrict__ sums, uint64_t* __restrict__ prefix,
                             uint64_t* __restrict__ before, uint32_t* __restrict__ codes,
                             cts_tcp_exchange_paced_tick* __restrict__ tick, uint64_t* __restrict__ sent_block)
{
    __shared__ uint64_t wsum[kBlock / 64];
    __shared__ uint64_t ctr[kBlock / 64][kCounterCount];
    __shared__ uint32_t red[kBlock / 64][7];
    __shared__ uint64_t dir[kBlock / 64][2];
    __shared__ int64_t due[kBlock / 64];
    zero_counters<kBlock / 64>(ctr);
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint32_t code = CTS_TCP_SENDER_SENT, c = 0u;
    uint64_t want = 0, m = 0;
    ExchangeShape S{};
    ExchangePace X{};
    bool paced = false;
    if (i < n) {
        c = ids[i];
        want = tcp_exchange_paced_want(entries, pace, c, n_conns, stride, max_buffers, now, code, S, m, X, paced);
    }
    uint64_t total;
    const uint64_t p = sums[blockIdx.x] + tile_scan_exclusive(want, wsum, total);
    uint64_t bytes0 = 0, bytes1 = 0;
    int64_t my_due = kNoDue;
    uint32_t buffers = 0, sent = 0, finished = 0, no_room = 0, skipped = 0, waiting = 0, pending = 0;
    if (i < n) {
        prefix[i] = p;
        const uint64_t pc = p < (uint64_t)capacity ? p : (uint64_t)capacity;
        const uint64_t t = want < (uint64_t)capacity - pc ? want : (uint64_t)capacity - pc;
        if (code != CTS_TCP_SENDER_SENT) {
            skipped = 1u;
        } else if (want == 0u) {
            // pacing lets nothing out: the entry stays, the next direction's pace entry may hold a new pending task
            waiting = 1u;
            code = CTS_TCP_SENDER_WAITING;
            X.save(pace, c, n_conns);
        } else if (t == 0u) {
            no_room = 1u;
            code = CTS_TCP_SENDER_NO_ROOM;
            if (paced) X.load(pace, c, n_conns, S, m);  // all three entries stay: what counts below is what is stored
        } else {
            if (paced) {
                if (t < want) {  // cut by the capacity: the machine moves t steps from the stored entries
                    X.load(pace, c, n_conns, S, m);
                    (void)X.run(now, (uint32_t)t, S);
                }
                X.save(pace, c, n_conns);
            }
            buffers = (uint32_t)t;
            sent = 1u;
            if (tcp_exchange_move(entries + c, S, m, t, bytes0, bytes1)) {
                finished = 1u;
                code = CTS_TCP_SENDER_FINISHED;
            }
        }
        if (skipped == 0u) {
            // a connection counts once; of a table kept by this tick only the next buffer's entry can be pending
            if (X.cur.pending != 0u) my_due = X.cur.due;
            if (X.oth.pending != 0u && X.oth.due < my_due) my_due = X.oth.due;
            pending = (X.cur.pending | X.oth.pending) != 0u ? 1u : 0u;
        }
        before[i] = m;
        if (codes != nullptr) codes[i] = code;
    }
    bytes0 = wave_sum64(bytes0);
    bytes1 = wave_sum64(bytes1);
    const uint64_t bytes = bytes0 + bytes1;
    // buffers, connections_sent, _finished, _no_room, _skipped; then the tail's connections_waiting, _pending
    const uint32_t words[7] = {wave_sum(buffers), wave_sum(sent),    wave_sum(finished), wave_sum(no_room),
                               wave_sum(skipped), wave_sum(waiting), wave_sum(pending)};
    my_due = wave_min64(my_due);
    if ((threadIdx.x & 63u) == 0u) {
        uint64_t* const own = ctr[threadIdx.x >> 6];
        own[0] = bytes;     // cts_counters_sent.bytes_sent (TcpStatusDetails.m_bytesSent of whichever side sent)
        own[1] = words[0];  // .buffers_sent
        own[2] = words[2];  // .connections_finished
        dir[threadIdx.x >> 6][0] = bytes0;
        dir[threadIdx.x >> 6][1] = bytes1;
        due[threadIdx.x >> 6] = my_due;
    }
    apply_flush(
        words, bytes, red, wsum, ctr, sent_block,
        [&](uint32_t k) { return k < 5u ? &tick->tick.tick.buffers + k : &tick->connections_waiting + (k - 5u); },
        &tick->tick.tick.bytes);
    apply_flush_dir(dir, tick->tick.bytes_dir, 8u);
    apply_flush_due(due, &tick->next_due_ms, 10u);
}

// cts_tcp_exchange_send_paced's planning: three launches, the middle one a single workgroup
hipError_t launch_tcp_exchange_paced_plan(const uint32_t* conn_ids, uint32_t n, uint32_t max_buffers,
                                          cts_tcp_exchange_state* entries, cts_tcp_sender_pace* pace,
                                          uint32_t n_conns, int64_t now_ms, uint32_t stride, uint32_t capacity,
                                          uint32_t* codes, cts_tcp_exchange_paced_tick* tick, uint64_t* sent_counters,
                                          const TcpExchangePacedScratch& scratch, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const uint64_t tiles = plan_tiles(n);
    const TcpSenderScratch& plain = scratch.exchange.plain;
    tcp_exchange_paced_sums<<<(uint32_t)tiles, kBlock, 0, stream>>>(conn_ids, n, entries, pace, n_conns, stride,
                                                                    max_buffers, now_ms, plain.sums);
    tcp_exchange_paced_scan<<<1, kBlock, 0, stream>>>(plain.sums, tiles, plain.prefix + n,
                                                      reinterpret_cast<uint32_t*>(tick));
    tcp_exchange_paced_apply<<<(uint32_t)tiles, kBlock, 0, stream>>>(conn_ids, n, entries, pace, n_conns, stride,
                                                                     capacity, max_buffers, now_ms, plain.sums,
                                                                     plain.prefix, plain.before, codes, tick,
                                                                     sent_counters);
    return hipGetLastError();
}

}  // namespace cts
