// cts_tick_plan.hip — the planning of a device-resident sender's tick for gfx950: which ring slots every listed
// connection takes, with no pattern byte written. Six ticks plan the same way (cts_media_stream_servers_send, _send_at,
// cts_tcp_senders_send, cts_tcp_senders_send_paced, cts_tcp_exchange_send, cts_tcp_exchange_send_paced): listed
// connection i wants w_i slots (0 when it sends nothing whatever the room); p_i, the exclusive 64-bit prefix of the
// wants in listed order, is its first slot, and the room left at p_i decides what it takes. Three plain launches in
// tiles of kPlanTile listed connections (no workgroup ever waits for another), issued by launch_plan:
//   *_sums          each tile's sum of wants                              -> sums[tile]
//   tick_plan_scan  one workgroup, one kernel for all six ticks: exclusive scan of the tile sums in place in passes
//                   of kBlock tiles, prefix[n] = the grand total, the tick block initialised
//   *_apply         p_i = sums[tile] + the tile's own scan -> prefix[i]; the code, the entries' updates, the tick block
//                   and the counter block
// The steps every planner shares come first (the tile scan, the tile-sum tail, the scan's passes, the apply tails, the
// scan kernel, the three launches). Then
//   ms_server_sums / _apply   the MediaStream servers, with a body of their own: a connection sends its whole frame or
//                             nothing, and the tick moves another kind of entry
//   ms_server_timed_sums / _apply
//                             the same servers by the clock: whole frames, as many as the schedule has released
//   tcp_tick_sums / _apply    the frame of the four TCP ticks, written once over a lane type: the index, the scan, the
//                             clamp to the capacity, the ladder of codes, the stores, the wave sums, the sent block and
//                             the tick block with its tails
//   SenderLane, PacedSenderLane, ExchangeLane, PacedExchangeLane
//                             what differs between the four: the entry and tick types, a lane's registers, want() (the
//                             slots a connection asks for), move() (the entry's update and the bytes by direction),
//                             what goes to before[], and for the paced two the pace registers' keep / reload / rerun
//                             and their pending task. The pace machine (PaceRegs: CreateNewTask's send branch and the
//                             walk that repeats it) is written once for both.
//   tcp_sender_ / tcp_paced_ / tcp_exchange_ / tcp_exchange_paced_ sums and apply: the frame over one lane type each
// What writes the ring from prefix[] is in cts_fill.hip, beside the loops it shares with the other fills.
// Scratch (MsServerScratch, TcpTickScratch<Tick> of cts_internal.hpp): u64 prefix[n + 1], u64 sums[tiles], for the TCP
// ticks and the servers' timed tick u64 before[n], and a tick.
#include <hip/hip_runtime.h>

#include "cts_chunks.hpp"
#include "cts_internal.hpp"
#include "cts_ms_server_schedule_math.hpp"
#include "cts_tcp_exchange_math.hpp"

namespace cts {

static_assert(sizeof(cts_tcp_exchange_tick) == 48 && offsetof(cts_tcp_exchange_tick, bytes_dir) == 32,
              "cts_tcp_exchange_tick: a plain tick and 16 bytes");
static_assert(kPlanTile == (uint32_t)kBlock, "one listed connection per thread of a tile");
static_assert(sizeof(cts_tcp_sender_pace) == 64 && alignof(cts_tcp_sender_pace) == 8, "cts_tcp_sender_pace: 64 bytes");
static_assert(sizeof(cts_tcp_sender_paced_tick) == 48 && offsetof(cts_tcp_sender_paced_tick, next_due_ms) == 32,
              "cts_tcp_sender_paced_tick: a plain tick and 16 bytes");
static_assert(sizeof(cts_tcp_exchange_paced_tick) == 64 && offsetof(cts_tcp_exchange_paced_tick, next_due_ms) == 48 &&
                  offsetof(cts_tcp_exchange_paced_tick, connections_waiting) == 56,
              "cts_tcp_exchange_paced_tick: an exchange tick and the paced tick's 16-byte tail");

static_assert(sizeof(cts_ms_server_schedule) == 16 && alignof(cts_ms_server_schedule) == 8, "cts_ms_server_schedule: 16 bytes");
static_assert(sizeof(cts_ms_server_timed_tick) == 48 && offsetof(cts_ms_server_timed_tick, next_due_ms) == 32 &&
                  offsetof(cts_ms_server_timed_tick, connections_waiting) == 40 &&
                  offsetof(cts_ms_server_timed_tick, frames) == 44,
              "cts_ms_server_timed_tick: a plain tick and 16 bytes");

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

// The body of the scan kernel (one workgroup): sums[] becomes its own exclusive scan, kBlock tiles a pass with the
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

__device__ __forceinline__ int64_t wave_min64(int64_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t u = (int64_t)__shfl_xor((long long)v, off, 64);
        v = u < v ? u : v;
    }
    return v;
}

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

// tick_plan_scan's max_at for a tick block without a word that starts at INT64_MAX (no thread index reaches it)
constexpr uint32_t kNoMaxWord = 0x7FFFFFFFu;

}  // namespace

// One workgroup. tick is `dwords` 32-bit words, zeroed, but for the 64-bit word at dword max_at, which starts at
// INT64_MAX (a paced tick's next_due_ms; kNoMaxWord = the block has none).
__global__ void __launch_bounds__(kBlock)
    tick_plan_scan(uint64_t* __restrict__ sums, uint64_t tiles, uint64_t* __restrict__ prefix_total,
                   uint32_t* __restrict__ tick, uint32_t dwords, uint32_t max_at)
{
    __shared__ uint64_t wsum[kBlock / 64];
    const uint64_t total = tile_sums_scan(sums, tiles, wsum);
    if (threadIdx.x == 0u) *prefix_total = total;
    if (threadIdx.x < dwords)
        tick[threadIdx.x] = threadIdx.x == max_at ? 0xFFFFFFFFu : threadIdx.x == max_at + 1u ? 0x7FFFFFFFu : 0u;
}

namespace {

// A tick's planning: three launches, the middle one a single workgroup. sums(tiles) and apply(tiles) launch the tick's
// own two kernels on that many workgroups.
template <typename Tick, typename Sums, typename Apply>
hipError_t launch_plan(uint32_t n, uint64_t* tile_sums, uint64_t* prefix, Tick* tick, uint32_t max_at,
                       hipStream_t stream, Sums sums, Apply apply)
{
    static_assert(sizeof(Tick) % 4u == 0u && sizeof(Tick) / 4u <= (size_t)kBlock, "a thread per dword of the block");
    if (n == 0) return hipSuccess;
    const uint64_t tiles = plan_tiles(n);
    sums((uint32_t)tiles);
    tick_plan_scan<<<1, kBlock, 0, stream>>>(tile_sums, tiles, prefix + n, reinterpret_cast<uint32_t*>(tick),
                                             (uint32_t)(sizeof(Tick) / 4u), max_at);
    apply((uint32_t)tiles);
    return hipGetLastError();
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

// cts_media_stream_servers_send's planning
hipError_t launch_ms_server_plan(const uint32_t* conn_ids, uint32_t n, cts_ms_server_state* servers, uint32_t n_conns,
                                 uint32_t stride, uint32_t capacity, uint32_t* codes, cts_ms_server_tick* tick,
                                 uint64_t* udp_counters, const MsServerScratch& scratch, hipStream_t stream)
{
    return launch_plan(
        n, scratch.sums, scratch.prefix, tick, kNoMaxWord, stream,
        [&](uint32_t tiles) {
            ms_server_sums<<<tiles, kBlock, 0, stream>>>(conn_ids, n, servers, n_conns, stride, scratch.sums);
        },
        [&](uint32_t tiles) {
            ms_server_apply<<<tiles, kBlock, 0, stream>>>(conn_ids, n, servers, n_conns, stride, capacity,
                                                          scratch.sums, scratch.prefix, codes, tick, udp_counters);
        });
}

// ---------------------------------------------------------------------------------------------
// The servers' timed tick (cts_media_stream_servers_send_at): the plain tick with every listed connection's frames
// those that its schedule entry releases at now (cts_ms_server_schedule_math.hpp: two divisions, no loop over
// frames), at most max_frames of them. Listed connection i wants w_i = min(wf_i x k_i, UINT32_MAX) slots and takes t_i
// = min(wf_i, room / k_i) whole frames, so a connection cut by the capacity has pushed every later prefix past the
// capacity and the tick's datagrams are still the slots [0, total) with no gap. before[i] is the connection's
// current_frame from before the move; ms_server_timed_fill (cts_fill.hip) reads prefix, before and the entries.

namespace {

// The frames listed connection c wants (0 with its code when it sends nothing whatever the room; code 5 when no frame
// is out) and its k. The schedule entry is read for a running connection only.
__device__ __forceinline__ uint32_t ms_server_timed_want(const cts_ms_server_state* __restrict__ servers,
                                                         const cts_ms_server_schedule* __restrict__ schedule,
                                                         uint32_t c, uint32_t n_conns, uint32_t stride,
                                                         uint32_t max_frames, int64_t now, uint32_t& code, uint32_t& k)
{
    // the plain tick's codes 4, 2 and 4 first, as ms_server_want decides them
    code = CTS_MS_SERVER_SKIPPED;
    k = 0u;
    if (c >= n_conns) return 0u;
    if (servers[c].finished != 0u) {
        code = CTS_MS_SERVER_ENDED;
        return 0u;
    }
    if (servers[c].datagram_max_size > stride) return 0u;
    code = CTS_MS_SERVER_SENT;
    k = servers[c].datagrams_per_frame;
    const uint32_t fps = schedule[c].frames_per_second;
    const uint32_t wf = ms_schedule_frames(schedule[c].base_time_ms, fps != 0u ? fps : 1u, servers[c].current_frame,
                                           servers[c].final_frame, now, max_frames);
    if (wf == 0u) code = CTS_MS_SERVER_WAITING;
    return wf;
}

// w = min(wf x k, UINT32_MAX): the cap keeps the 64-bit prefix from wrapping over 2^32 listed connections
// (returned as 32 bits from the product's halves: with a 64-bit minimum here the compiler swapped the operands of one
// add in ms_server_sums, and tools/kernel_text.py no longer showed that kernel as the one before this tick existed)
__device__ __forceinline__ uint32_t ms_server_timed_slots(uint32_t wf, uint32_t k)
{
    const uint64_t w = (uint64_t)wf * k;
    return (uint32_t)(w >> 32) != 0u ? 0xFFFFFFFFu : (uint32_t)w;
}

}  // namespace

__global__ void __launch_bounds__(kBlock)
    ms_server_timed_sums(const uint32_t* __restrict__ ids, uint32_t n, const cts_ms_server_state* __restrict__ servers,
                         const cts_ms_server_schedule* __restrict__ schedule, uint32_t n_conns, uint32_t stride,
                         uint32_t max_frames, int64_t now, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t wsum[kBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint64_t want = 0;
    if (i < n) {
        uint32_t code, k;
        const uint32_t wf = ms_server_timed_want(servers, schedule, ids[i], n_conns, stride, max_frames, now, code, k);
        want = ms_server_timed_slots(wf, k);
    }
    tile_sum_store(want, wsum, sums);
}

__global__ void __launch_bounds__(kBlock)
    ms_server_timed_apply(const uint32_t* __restrict__ ids, uint32_t n, cts_ms_server_state* __restrict__ servers,
                          const cts_ms_server_schedule* __restrict__ schedule, uint32_t n_conns, uint32_t stride,
                          uint32_t capacity, uint32_t max_frames, int64_t now, const uint64_t* __restrict__ sums,
                          uint64_t* __restrict__ prefix, uint64_t* __restrict__ before, uint32_t* __restrict__ codes,
                          cts_ms_server_timed_tick* __restrict__ tick, uint64_t* __restrict__ udp)
{
    // datagrams, connections_sent, _finished, _no_room, _skipped; then the tail's connections_waiting, frames
    constexpr int WORDS = 7;
    constexpr uint32_t kDueAt = 8u;  // apply_flush keeps threads 0 .. WORDS busy
    static_assert(WORDS < (int)kDueAt, "next_due_ms's thread lies past apply_flush's");
    __shared__ uint64_t wsum[kBlock / 64];
    __shared__ uint64_t ctr[kBlock / 64][kCounterCount];
    __shared__ uint32_t red[kBlock / 64][WORDS];
    __shared__ int64_t due[kBlock / 64];
    zero_counters<kBlock / 64>(ctr);
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint32_t code = CTS_MS_SERVER_SENT, c = 0u, k = 0u, wf = 0u;
    if (i < n) {
        c = ids[i];
        wf = ms_server_timed_want(servers, schedule, c, n_conns, stride, max_frames, now, code, k);
    }
    uint64_t total;
    const uint64_t p = sums[blockIdx.x] + tile_scan_exclusive(ms_server_timed_slots(wf, k), wsum, total);
    uint64_t bytes = 0;
    int64_t my_due = kNoDue;
    uint32_t datagrams = 0, sent = 0, finished = 0, no_room = 0, skipped = 0, waiting = 0, frames = 0;
    if (i < n) {
        prefix[i] = p;
        uint64_t was = 0;
        if (code == CTS_MS_SERVER_WAITING) {
            waiting = 1u;
        } else if (code != CTS_MS_SERVER_SENT) {
            skipped = 1u;
        } else {
            const uint32_t pc = p < (uint64_t)capacity ? (uint32_t)p : capacity;
            const uint32_t fit = (capacity - pc) / (k != 0u ? k : 1u);
            const uint32_t t = wf < fit ? wf : fit;
            if (t == 0u) {
                no_room = 1u;
                code = CTS_MS_SERVER_NO_ROOM;
            } else {
                // the only step that knows how many frames the connection takes is the one that moves its entry
                cts_ms_server_state* e = servers + c;
                bytes = (uint64_t)t * e->frame_size_bytes;  // t x F <= capacity x stride < 2^52
                datagrams = t * k;                         // <= capacity
                frames = t;
                sent = 1u;
                e->bits_sent += 8u * bytes;
                e->datagrams_sent += datagrams;
                was = (uint64_t)e->current_frame;
                const int64_t next = e->current_frame + (int64_t)t;
                e->current_frame = next;
                if (next > e->final_frame) {
                    e->finished = 1u;
                    finished = 1u;
                    code = CTS_MS_SERVER_FINISHED;
                }
            }
        }
        // what the tick leaves running: the time of its next frame
        if (skipped == 0u && finished == 0u) {
            const uint32_t fps = schedule[c].frames_per_second;
            my_due = ms_schedule_due(schedule[c].base_time_ms, fps != 0u ? fps : 1u, servers[c].current_frame);
        }
        before[i] = was;
        if (codes != nullptr) codes[i] = code;
    }
    bytes = wave_sum64(bytes);
    const uint32_t words[WORDS] = {wave_sum(datagrams), wave_sum(sent),    wave_sum(finished), wave_sum(no_room),
                                   wave_sum(skipped),   wave_sum(waiting), wave_sum(frames)};
    my_due = wave_min64(my_due);
    if ((threadIdx.x & 63u) == 0u) {
        // the reference's server adds its sent bits to UdpStatusDetails.m_bitsReceived (ctsIOPattern.cpp:1162)
        ctr[threadIdx.x >> 6][0] = 8u * bytes;                 // cts_counters_udp.bits_received
        ctr[threadIdx.x >> 6][kCounterCount - 1] = words[0];  // cts_counters_udp.datagrams
        due[threadIdx.x >> 6] = my_due;
    }
    apply_flush(
        words, bytes, red, wsum, ctr, udp,
        [&](uint32_t w) { return w < 5u ? &tick->tick.datagrams + w : &tick->connections_waiting + (w - 5u); },
        &tick->tick.bytes);
    apply_flush_due(due, &tick->next_due_ms, kDueAt);
}

// cts_media_stream_servers_send_at's planning
hipError_t launch_ms_server_timed_plan(const uint32_t* conn_ids, uint32_t n, cts_ms_server_state* servers,
                                       const cts_ms_server_schedule* schedule, uint32_t n_conns, uint32_t stride,
                                       uint32_t capacity, uint32_t max_frames, int64_t now_ms, uint32_t* codes,
                                       cts_ms_server_timed_tick* tick, uint64_t* udp_counters,
                                       const MsServerTimedScratch& scratch, hipStream_t stream)
{
    return launch_plan(
        n, scratch.sums, scratch.prefix, tick, (uint32_t)(offsetof(cts_ms_server_timed_tick, next_due_ms) / 4u), stream,
        [&](uint32_t tiles) {
            ms_server_timed_sums<<<tiles, kBlock, 0, stream>>>(conn_ids, n, servers, schedule, n_conns, stride,
                                                               max_frames, now_ms, scratch.sums);
        },
        [&](uint32_t tiles) {
            ms_server_timed_apply<<<tiles, kBlock, 0, stream>>>(conn_ids, n, servers, schedule, n_conns, stride,
                                                                capacity, max_frames, now_ms, scratch.sums,
                                                                scratch.prefix, scratch.before, codes, tick,
                                                                udp_counters);
        });
}

// ---------------------------------------------------------------------------------------------
// The frame of the four TCP ticks. Listed connection i wants w_i slots and takes t_i = min(w_i, capacity - min(p_i,
// capacity)) of them. apply also leaves a word per listed connection from before the move in the scratch's before[];
// the descriptor passes and the fill (cts_fill.hip) read prefix, before and the tick.
//
// A lane type holds the tick's uniform arguments and one listed connection's registers, and has
//   Entry, Tick, kPaced, kTwoWay
//   want(c, code)      the slots connection c wants and its code (CTS_TCP_SENDER_SENT, or what it is when it sends
//                      nothing whatever the room); loads the lane's registers
//   move(c, t, bytes)  connection c takes t > 0 slots: its entry's update, the bytes sent by direction (a one-way
//                      tick leaves bytes[1] alone); true = the connection has ended. The only step that knows how many
//                      slots a connection takes is the one that moves its entry.
//   before()           the word for before[i]
//   kPaced lanes: `paced` (the pace registers hold this connection's entries and want() has moved them), keep(c)
//   (store them), reload(c) (load the stored entries again), rerun(t) (the walk of t steps), due_of(pending, due)
//   (whether a task is pending, and when it is due)
//   kTwoWay lanes: dir_of(tick), the tick block's bytes_dir
// plain_tick(tick) of cts_internal.hpp is the 32-byte block every tick begins with.

namespace {

template <typename Lane>
__device__ __forceinline__ void tcp_tick_sums(Lane lane, const uint32_t* __restrict__ ids, uint32_t n,
                                              uint64_t* __restrict__ sums)
{
    __shared__ uint64_t wsum[kBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint64_t want = 0;
    if (i < n) {
        uint32_t code;
        want = lane.want(ids[i], code);
    }
    tile_sum_store(want, wsum, sums);
}

template <typename Lane>
__device__ __forceinline__ void tcp_tick_apply(Lane lane, const uint32_t* __restrict__ ids, uint32_t n,
                                               uint32_t capacity, const uint64_t* __restrict__ sums,
                                               uint64_t* __restrict__ prefix, uint64_t* __restrict__ before,
                                               uint32_t* __restrict__ codes, typename Lane::Tick* __restrict__ tick,
                                               uint64_t* __restrict__ sent_block)
{
    // buffers, connections_sent, _finished, _no_room, _skipped; then a paced tail's connections_waiting, _pending
    constexpr int WORDS = Lane::kPaced ? 7 : 5;
    // apply_flush keeps threads 0 .. WORDS busy; the tails' threads follow: bytes_dir's two, then next_due_ms's one
    constexpr uint32_t kDirAt = 8u, kDueAt = Lane::kTwoWay ? kDirAt + 2u : kDirAt;
    static_assert(WORDS < (int)kDirAt, "the tails' threads lie past apply_flush's");
    __shared__ uint64_t wsum[kBlock / 64];
    __shared__ uint64_t ctr[kBlock / 64][kCounterCount];
    __shared__ uint32_t red[kBlock / 64][WORDS];
    __shared__ uint64_t dir[kBlock / 64][2];  // kTwoWay
    __shared__ int64_t due[kBlock / 64];      // kPaced
    zero_counters<kBlock / 64>(ctr);
    const uint64_t i = (uint64_t)blockIdx.x * kPlanTile + threadIdx.x;
    uint32_t code = CTS_TCP_SENDER_SENT, c = 0u;
    uint64_t want = 0;
    if (i < n) {
        c = ids[i];
        want = lane.want(c, code);
    }
    uint64_t total;
    const uint64_t p = sums[blockIdx.x] + tile_scan_exclusive(want, wsum, total);
    uint64_t bytes_by[2] = {0u, 0u};
    int64_t my_due = kNoDue;
    uint32_t buffers = 0, sent = 0, finished = 0, no_room = 0, skipped = 0, waiting = 0, pending = 0;
    if (i < n) {
        prefix[i] = p;
        const uint64_t pc = p < (uint64_t)capacity ? p : (uint64_t)capacity;
        const uint64_t t = want < (uint64_t)capacity - pc ? want : (uint64_t)capacity - pc;
        if (code != CTS_TCP_SENDER_SENT) {
            skipped = 1u;
        } else if (Lane::kPaced && want == 0u) {
            // pacing lets nothing out: the connection's entry stays, a pace entry may hold a new pending task
            waiting = 1u;
            code = CTS_TCP_SENDER_WAITING;
            if constexpr (Lane::kPaced) lane.keep(c);
        } else if (t == 0u) {
            no_room = 1u;
            code = CTS_TCP_SENDER_NO_ROOM;
            if constexpr (Lane::kPaced) {
                if (lane.paced) lane.reload(c);  // every entry stays: what counts below is what is stored
            }
        } else {
            if constexpr (Lane::kPaced) {
                if (lane.paced) {
                    if (t < want) {  // cut by the capacity: the machine moves t steps from the stored entries
                        lane.reload(c);
                        lane.rerun((uint32_t)t);
                    }
                    lane.keep(c);
                }
            }
            buffers = (uint32_t)t;
            sent = 1u;
            if (lane.move(c, t, bytes_by)) {
                finished = 1u;
                code = CTS_TCP_SENDER_FINISHED;
            }
        }
        if constexpr (Lane::kPaced) {
            if (skipped == 0u) lane.due_of(pending, my_due);
        }
        before[i] = lane.before();
        if (codes != nullptr) codes[i] = code;
    }
    bytes_by[0] = wave_sum64(bytes_by[0]);
    uint64_t bytes = bytes_by[0];
    if constexpr (Lane::kTwoWay) {
        bytes_by[1] = wave_sum64(bytes_by[1]);
        bytes += bytes_by[1];
    }
    uint32_t words[WORDS] = {wave_sum(buffers), wave_sum(sent), wave_sum(finished), wave_sum(no_room),
                             wave_sum(skipped)};
    if constexpr (Lane::kPaced) {
        words[5] = wave_sum(waiting);
        words[6] = wave_sum(pending);
        my_due = wave_min64(my_due);
    }
    if ((threadIdx.x & 63u) == 0u) {
        uint64_t* const own = ctr[threadIdx.x >> 6];
        own[0] = bytes;     // cts_counters_sent.bytes_sent (TcpStatusDetails.m_bytesSent of whichever side sent,
                            // ctsIOPattern.cpp:510)
        own[1] = words[0];  // .buffers_sent
        own[2] = words[2];  // .connections_finished
        if constexpr (Lane::kTwoWay) {
            dir[threadIdx.x >> 6][0] = bytes_by[0];
            dir[threadIdx.x >> 6][1] = bytes_by[1];
        }
        if constexpr (Lane::kPaced) due[threadIdx.x >> 6] = my_due;
    }
    cts_tcp_sender_tick* const plain = plain_tick(tick);
    apply_flush(
        words, bytes, red, wsum, ctr, sent_block,
        [&](uint32_t k) {
            if constexpr (Lane::kPaced) return k < 5u ? &plain->buffers + k : &tick->connections_waiting + (k - 5u);
            else return &plain->buffers + k;
        },
        &plain->bytes);
    if constexpr (Lane::kTwoWay) apply_flush_dir(dir, Lane::dir_of(tick), kDirAt);
    if constexpr (Lane::kPaced) apply_flush_due(due, &tick->next_due_ms, kDueAt);
}

// A _sums kernel calls want() alone, which stores nothing: it hands its const table to a lane as the pointer move()
// needs.
template <typename T>
__device__ __forceinline__ T* lane_table(const T* table)
{
    return const_cast<T*>(table);
}

// ---------------------------------------------------------------------------------------------
// TCP senders (cts_tcp_senders_send): listed connection i wants w_i = min(max_buffers, ceil(R / B)) slots; before[i] is
// its bytes_sent from before the move (0 when it did not move).

struct SenderLane {
    using Entry = cts_tcp_sender_state;
    using Tick = cts_tcp_sender_tick;
    static constexpr bool kPaced = false, kTwoWay = false;
    Entry* senders;
    uint32_t n_conns, stride, max_buffers;
    uint64_t R = 0, was = 0;  // bytes left; bytes_sent before the move
    uint32_t B = 0;           // buffer size

    // The slots whatever the time; R and B of a running connection.
    __device__ __forceinline__ uint32_t want(uint32_t c, uint32_t& code)
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
    __device__ __forceinline__ bool move(uint32_t c, uint64_t t, uint64_t (&bytes)[2])
    {
        Entry* const e = senders + c;
        was = e->bytes_sent;
        const uint64_t full = t * B;  // t <= capacity < 2^32
        bytes[0] = full < R ? full : R;
        e->bytes_sent = was + bytes[0];
        e->buffers_sent += t;
        const bool ended = bytes[0] == R;
        if (ended) e->finished = 1u;
        return ended;
    }
    __device__ __forceinline__ uint64_t before() const { return was; }
};

}  // namespace

__global__ void __launch_bounds__(kBlock)
    tcp_sender_sums(const uint32_t* __restrict__ ids, uint32_t n, const cts_tcp_sender_state* __restrict__ senders,
                    uint32_t n_conns, uint32_t stride, uint32_t max_buffers, uint64_t* __restrict__ sums)
{
    tcp_tick_sums(SenderLane{lane_table(senders), n_conns, stride, max_buffers}, ids, n, sums);
}

__global__ void __launch_bounds__(kBlock)
    tcp_sender_apply(const uint32_t* __restrict__ ids, uint32_t n, cts_tcp_sender_state* __restrict__ senders,
                     uint32_t n_conns, uint32_t stride, uint32_t capacity, uint32_t max_buffers,
                     const uint64_t* __restrict__ sums, uint64_t* __restrict__ prefix, uint64_t* __restrict__ before,
                     uint32_t* __restrict__ codes, cts_tcp_sender_tick* __restrict__ tick, uint64_t* __restrict__ sent_block)
{
    tcp_tick_apply(SenderLane{senders, n_conns, stride, max_buffers}, ids, n, capacity, sums, prefix, before, codes,
                   tick, sent_block);
}

// ---------------------------------------------------------------------------------------------
// Paced TCP senders (cts_tcp_senders_send_paced): the plain tick with every listed connection's wanted slots cut to what
// its 64-byte pace entry lets out at now_ms. _sums runs the pace machine on a register copy and stores nothing; _apply
// runs it again and moves both entries. The descriptor pass and the fill are the plain tick's launches, unchanged: they
// read prefix, before and the tick block's first 32 bytes.

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

    // The pacing walk, run(cap) of cts_tcp_senders.h and run_x(cap) of cts_tcp_exchange.h: up to cap sends at `now`,
    // stopped by a task that is not due yet; the count of sends let out. next() is the next send's bytes, taken(bytes)
    // follows every send that is let out (the exchange tick's may swap *this for the other direction's registers).
    // The loop's length differs from lane to lane: a wave takes as long as its longest lane.
    template <typename Next, typename Taken>
    __device__ __forceinline__ uint32_t walk(int64_t now, uint32_t cap, Next next, Taken taken)
    {
        uint32_t count = 0;
        while (count < cap) {
            const auto size = next();
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
            taken(size);
        }
        return count;
    }
};

struct PacedSenderLane : SenderLane {
    using Tick = cts_tcp_sender_paced_tick;
    static constexpr bool kPaced = true;
    cts_tcp_sender_pace* pace;
    int64_t now;
    PaceRegs Q{};  // a register copy of the connection's pace entry
    bool paced = false;

    // the walk of cap <= ceil(R / B) steps, so bytes are left at every step
    __device__ __forceinline__ uint32_t run(uint32_t cap)
    {
        uint64_t left = R;
        return Q.walk(
            now, cap, [&] { return left < (uint64_t)B ? left : (uint64_t)B; }, [&](uint64_t size) { left -= size; });
    }
    // The plain want, or what the walk lets out of it at now.
    __device__ __forceinline__ uint32_t want(uint32_t c, uint32_t& code)
    {
        paced = false;
        const uint32_t limit = SenderLane::want(c, code);
        if (code != CTS_TCP_SENDER_SENT) return 0u;
        Q.load(pace + c);
        if (Q.unpaced()) return limit;
        paced = true;
        return run(limit);
    }
    __device__ __forceinline__ void keep(uint32_t c) const { Q.save(pace + c); }
    __device__ __forceinline__ void reload(uint32_t c) { Q.load(pace + c); }
    __device__ __forceinline__ void rerun(uint32_t t) { (void)run(t); }
    __device__ __forceinline__ void due_of(uint32_t& pending, int64_t& due) const
    {
        if (Q.pending != 0u) {
            pending = 1u;
            due = Q.due;
        }
    }
};

}  // namespace

__global__ void __launch_bounds__(kBlock)
    tcp_paced_sums(const uint32_t* __restrict__ ids, uint32_t n, const cts_tcp_sender_state* __restrict__ senders,
                   const cts_tcp_sender_pace* __restrict__ pace, uint32_t n_conns, uint32_t stride,
                   uint32_t max_buffers, int64_t now, uint64_t* __restrict__ sums)
{
    tcp_tick_sums(PacedSenderLane{{lane_table(senders), n_conns, stride, max_buffers}, lane_table(pace), now}, ids, n,
                  sums);
}

__global__ void __launch_bounds__(kBlock)
    tcp_paced_apply(const uint32_t* __restrict__ ids, uint32_t n, cts_tcp_sender_state* __restrict__ senders,
                    cts_tcp_sender_pace* __restrict__ pace, uint32_t n_conns, uint32_t stride, uint32_t capacity,
                    uint32_t max_buffers, int64_t now, const uint64_t* __restrict__ sums,
                    uint64_t* __restrict__ prefix, uint64_t* __restrict__ before, uint32_t* __restrict__ codes,
                    cts_tcp_sender_paced_tick* __restrict__ tick, uint64_t* __restrict__ sent_block)
{
    tcp_tick_apply(PacedSenderLane{{senders, n_conns, stride, max_buffers}, pace, now}, ids, n, capacity, sums, prefix,
                   before, codes, tick, sent_block);
}

// ---------------------------------------------------------------------------------------------
// The exchange tick (cts_tcp_exchange_send): Push, Pull, PushPull and Duplex connections from 64-byte entries. Listed
// connection i wants w_i = min(max_buffers, N - buffers_sent) slots of its buffer sequence; whose turn each buffer is
// follows from its index (cts_tcp_exchange_math.hpp), so the planning never looks at a direction: the move asks the
// closed form where the entry stands t buffers on. before[i] is the connection's buffers_sent from before the move;
// tcp_exchange_descs (cts_fill.hip) reads prefix, before and the tick.

namespace {

struct ExchangeLane {
    using Entry = cts_tcp_exchange_state;
    using Tick = cts_tcp_exchange_tick;
    static constexpr bool kPaced = false, kTwoWay = true;
    Entry* entries;
    uint32_t n_conns, stride, max_buffers;
    ExchangeShape S{};  // the entry's constants
    uint64_t m = 0;     // its position

    __device__ __forceinline__ uint32_t want(uint32_t c, uint32_t& code)
    {
        return limit(entries, c, n_conns, stride, max_buffers, code, S, m);
    }
    // want()'s body, static and over references: the compiler simplifies it before it is inlined, and over this->S the
    // same text ends as branches that cost tcp_exchange_sums two more VGPRs (12 for 10)
    static __device__ __forceinline__ uint32_t limit(const Entry* __restrict__ entries, uint32_t c, uint32_t n_conns,
                                                     uint32_t stride, uint32_t max_buffers, uint32_t& code,
                                                     ExchangeShape& S, uint64_t& m)
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
    // The bytes of buffers m .. m + t by direction are the difference of two positions, whatever segment ends lie
    // between, and the entry holds the position at m (cts_tcp_exchange_init, _seek and this move keep it so).
    __device__ __forceinline__ bool move(uint32_t c, uint64_t t, uint64_t (&bytes)[2])
    {
        Entry* const e = entries + c;
        uint64_t to[2];
        exchange_position(S, m + t, to);
        bytes[0] = exchange_sub(to[0], e->bytes_sent[0]);
        bytes[1] = exchange_sub(to[1], e->bytes_sent[1]);
        e->bytes_sent[0] += bytes[0];
        e->bytes_sent[1] += bytes[1];
        e->buffers_sent = m + t;
        const bool ended = m + t == S.N;
        if (ended) e->finished = 1u;
        return ended;
    }
    __device__ __forceinline__ uint64_t before() const { return m; }
    static __device__ __forceinline__ uint64_t* dir_of(Tick* tick) { return tick->bytes_dir; }
};

}  // namespace

__global__ void __launch_bounds__(kBlock)
    tcp_exchange_sums(const uint32_t* __restrict__ ids, uint32_t n, const cts_tcp_exchange_state* __restrict__ entries,
                      uint32_t n_conns, uint32_t stride, uint32_t max_buffers, uint64_t* __restrict__ sums)
{
    tcp_tick_sums(ExchangeLane{lane_table(entries), n_conns, stride, max_buffers}, ids, n, sums);
}

__global__ void __launch_bounds__(kBlock)
    tcp_exchange_apply(const uint32_t* __restrict__ ids, uint32_t n, cts_tcp_exchange_state* __restrict__ entries,
                       uint32_t n_conns, uint32_t stride, uint32_t capacity, uint32_t max_buffers,
                       const uint64_t* __restrict__ sums, uint64_t* __restrict__ prefix, uint64_t* __restrict__ before,
                       uint32_t* __restrict__ codes, cts_tcp_exchange_tick* __restrict__ tick,
                       uint64_t* __restrict__ sent_block)
{
    tcp_tick_apply(ExchangeLane{entries, n_conns, stride, max_buffers}, ids, n, capacity, sums, prefix, before, codes,
                   tick, sent_block);
}

// ---------------------------------------------------------------------------------------------
// The paced exchange tick (cts_tcp_exchange_send_paced): the exchange tick with every listed connection's wanted slots
// cut by run_x of cts_tcp_exchange.h, the pace machine's walk with each step taken on the pace entry of the next
// buffer's direction (entry c + d x n_conns: the side that sends direction d). _sums walks on register copies and
// stores nothing; _apply walks again and moves the entry and the pace entries.
// The walk pays exchange_element's division once: an ExchangeCursor is seeded at m and moved by additions. A lane keeps
// both directions' pace registers, `cur` for the next buffer's direction and `oth`, and swaps them when the direction
// flips, so no register is ever indexed by a direction. tcp_exchange_descs and the fill follow unchanged: they read
// prefix, before and the block's first 48 and 32 bytes.

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

    // the walk of cap <= N - m steps, the size and the entry of each taken from the cursor
    __device__ __forceinline__ uint32_t run(int64_t now, uint32_t cap, const ExchangeShape& S)
    {
        return cur.walk(
            now, cap, [&] { return at.len(S); },
            [&](uint32_t size) {
                if (at.advance(S, size)) {
                    const PaceRegs was = cur;
                    cur = oth;
                    oth = was;
                }
            });
    }
};

struct PacedExchangeLane : ExchangeLane {
    using Tick = cts_tcp_exchange_paced_tick;
    static constexpr bool kPaced = true;
    cts_tcp_sender_pace* pace;
    int64_t now;
    ExchangePace X{};  // register copies of the connection's pace entries
    bool paced = false;

    // The plain want, or what the walk lets out of it at now.
    __device__ __forceinline__ uint32_t want(uint32_t c, uint32_t& code)
    {
        paced = false;
        const uint32_t limit = ExchangeLane::want(c, code);
        if (code != CTS_TCP_SENDER_SENT) return 0u;
        X.load(pace, c, n_conns, S, m);
        if (X.unpaced()) return limit;
        paced = true;
        return X.run(now, limit, S);
    }
    __device__ __forceinline__ void keep(uint32_t c) const { X.save(pace, c, n_conns); }
    __device__ __forceinline__ void reload(uint32_t c) { X.load(pace, c, n_conns, S, m); }
    __device__ __forceinline__ void rerun(uint32_t t) { (void)X.run(now, t, S); }
    // a connection counts once; of a table kept by this tick only the next buffer's entry can be pending
    __device__ __forceinline__ void due_of(uint32_t& pending, int64_t& due) const
    {
        if (X.cur.pending != 0u) due = X.cur.due;
        if (X.oth.pending != 0u && X.oth.due < due) due = X.oth.due;
        pending = (X.cur.pending | X.oth.pending) != 0u ? 1u : 0u;
    }
    static __device__ __forceinline__ uint64_t* dir_of(Tick* tick) { return tick->tick.bytes_dir; }
};

}  // namespace

__global__ void __launch_bounds__(kBlock)
    tcp_exchange_paced_sums(const uint32_t* __restrict__ ids, uint32_t n,
                            const cts_tcp_exchange_state* __restrict__ entries,
                            const cts_tcp_sender_pace* __restrict__ pace, uint32_t n_conns, uint32_t stride,
                            uint32_t max_buffers, int64_t now, uint64_t* __restrict__ sums)
{
    tcp_tick_sums(PacedExchangeLane{{lane_table(entries), n_conns, stride, max_buffers}, lane_table(pace), now}, ids,
                  n, sums);
}

__global__ void __launch_bounds__(kBlock)
    tcp_exchange_paced_apply(const uint32_t* __restrict__ ids, uint32_t n,
                             cts_tcp_exchange_state* __restrict__ entries, cts_tcp_sender_pace* __restrict__ pace,
                             uint32_t n_conns, uint32_t stride, uint32_t capacity, uint32_t max_buffers, int64_t now,
                             const uint64_t* __restrict__ sums, uint64_t* __restrict__ prefix,
                             uint64_t* __restrict__ before, uint32_t* __restrict__ codes,
                             cts_tcp_exchange_paced_tick* __restrict__ tick, uint64_t* __restrict__ sent_block)
{
    tcp_tick_apply(PacedExchangeLane{{entries, n_conns, stride, max_buffers}, pace, now}, ids, n, capacity, sums,
                   prefix, before, codes, tick, sent_block);
}

// ---------------------------------------------------------------------------------------------
// The four TCP ticks' planning (launch_tcp_plan of cts_internal.hpp): launch_plan over the tick's two kernels.

namespace {

template <typename Tick>
struct TickKernels;
template <>
struct TickKernels<cts_tcp_sender_tick> {
    static constexpr bool kPaced = false;
    static constexpr auto sums = tcp_sender_sums;
    static constexpr auto apply = tcp_sender_apply;
};
template <>
struct TickKernels<cts_tcp_sender_paced_tick> {
    static constexpr bool kPaced = true;
    static constexpr auto sums = tcp_paced_sums;
    static constexpr auto apply = tcp_paced_apply;
};
template <>
struct TickKernels<cts_tcp_exchange_tick> {
    static constexpr bool kPaced = false;
    static constexpr auto sums = tcp_exchange_sums;
    static constexpr auto apply = tcp_exchange_apply;
};
template <>
struct TickKernels<cts_tcp_exchange_paced_tick> {
    static constexpr bool kPaced = true;
    static constexpr auto sums = tcp_exchange_paced_sums;
    static constexpr auto apply = tcp_exchange_paced_apply;
};

}  // namespace

template <typename Tick, typename Entry>
hipError_t launch_tcp_plan(const TcpTickArgs& a, Entry* entries, Tick* tick, const TcpTickScratch<Tick>& scratch,
                           hipStream_t stream)
{
    using K = TickKernels<Tick>;
    uint32_t max_at = kNoMaxWord;
    if constexpr (K::kPaced) max_at = offsetof(Tick, next_due_ms) / 4u;
    uint64_t* const sent = static_cast<uint64_t*>(a.sent_counters);
    return launch_plan(
        a.n, scratch.sums, scratch.prefix, tick, max_at, stream,
        [&](uint32_t tiles) {
            if constexpr (K::kPaced)
                K::sums<<<tiles, kBlock, 0, stream>>>(a.conn_ids, a.n, entries, a.pace, a.n_conns, a.stride,
                                                      a.max_buffers, a.now_ms, scratch.sums);
            else
                K::sums<<<tiles, kBlock, 0, stream>>>(a.conn_ids, a.n, entries, a.n_conns, a.stride, a.max_buffers,
                                                      scratch.sums);
        },
        [&](uint32_t tiles) {
            if constexpr (K::kPaced)
                K::apply<<<tiles, kBlock, 0, stream>>>(a.conn_ids, a.n, entries, a.pace, a.n_conns, a.stride,
                                                       a.capacity, a.max_buffers, a.now_ms, scratch.sums,
                                                       scratch.prefix, scratch.before, a.codes, tick, sent);
            else
                K::apply<<<tiles, kBlock, 0, stream>>>(a.conn_ids, a.n, entries, a.n_conns, a.stride, a.capacity,
                                                       a.max_buffers, scratch.sums, scratch.prefix, scratch.before,
                                                       a.codes, tick, sent);
        });
}

template hipError_t launch_tcp_plan(const TcpTickArgs&, cts_tcp_sender_state*, cts_tcp_sender_tick*,
                                    const TcpTickScratch<cts_tcp_sender_tick>&, hipStream_t);
template hipError_t launch_tcp_plan(const TcpTickArgs&, cts_tcp_sender_state*, cts_tcp_sender_paced_tick*,
                                    const TcpTickScratch<cts_tcp_sender_paced_tick>&, hipStream_t);
template hipError_t launch_tcp_plan(const TcpTickArgs&, cts_tcp_exchange_state*, cts_tcp_exchange_tick*,
                                    const TcpTickScratch<cts_tcp_exchange_tick>&, hipStream_t);
template hipError_t launch_tcp_plan(const TcpTickArgs&, cts_tcp_exchange_state*, cts_tcp_exchange_paced_tick*,
                                    const TcpTickScratch<cts_tcp_exchange_paced_tick>&, hipStream_t);

}  // namespace cts
