// cts_pattern_pipeline.hpp — the DEFERRED batch pipeline of the ctsIoPattern mirror: the one owner of "completions
// queued, batches launched, verdicts not yet applied". The pattern enqueues each completed recv with its accounting
// snapshot and gets every batch's verdicts back through cts_io_pattern::ApplyVerdicts; it never sees an event, a
// descriptor set or a staging buffer, and the pipeline never touches the pattern's counters.
#pragma once

#include <algorithm>
#include <cstdint>
#include <deque>
#include <vector>

#include "cts_pattern_device.hpp"

struct cts_io_pattern;

namespace cts {

struct Pinned {  // pinned host memory with its device view
    uint8_t* host = nullptr;
    uint8_t* dev = nullptr;  // hipHostGetDevicePointer
    uint64_t bytes = 0;
    cts_engine* engine = nullptr;
    int alloc(cts_engine* e, uint64_t n)
    {
        void *h = nullptr, *d = nullptr;
        const int rc = cts_host_alloc(e, n, &h, &d);
        if (rc != CTS_OK) return rc;
        host = static_cast<uint8_t*>(h);
        dev = static_cast<uint8_t*>(d);
        bytes = n;
        engine = e;
        return CTS_OK;
    }
    void release()
    {
        if (host) (void)cts_host_free(engine, host);
        host = dev = nullptr;
        bytes = 0;
    }
    ~Pinned() { release(); }
};

// One queued recv completion: what the pattern's accounting was right after it (the pattern rolls back to it when the
// buffer fails). The pipeline carries it and reads only `transferred` and `expected`.
struct Queued {
    uint32_t completion;        // recv completion index
    uint32_t transferred;
    uint64_t bytes_recv_after;  // m_bytesRecv after this completion (as the reference would count it)
    uint64_t bytes_sent_after;  // m_bytesSent at that point (sends completed later are rolled back on failure)
    uint32_t expected;          // the task's m_expectedPatternOffset
    uint64_t status_recv_after; // this pattern's TcpStatusDetails.m_bytesRecv contribution after this completion
    uint64_t status_sent_after; // ... and its m_bytesSent contribution at that point
};

class DeferredPipeline {
public:
    DeferredPipeline(cts_io_pattern& owner, PatternDevice& dev, uint32_t batch_buffers, uint64_t batch_bytes)
        : owner(owner), dev(dev), batch_buffers(batch_buffers), batch_bytes(batch_bytes)
    {
    }
    ~DeferredPipeline();
    DeferredPipeline(const DeferredPipeline&) = delete;

    // RetireDone / Rotate / Flush return CTS_OK, a negative CTS_E_*, or kBatchFailed: a batch held a failing buffer (the
    // pattern latched it in ApplyVerdicts) and everything queued or launched behind that batch was dropped.
    static constexpr int kBatchFailed = 1;

    // The zero-copy recv ring (a completion inside it is verified in place, anything else is staged): its host view,
    // its device view when it is pinned, its size.
    void SetRing(const char* host, const uint8_t* device, uint64_t bytes)
    {
        ring_host = host;
        ring_dev = device;
        ring_bytes = bytes;
    }
    uint32_t BatchCapacity() const { return batch_buffers ? batch_buffers : 1024u; }
    // Batches in flight at once (pipelined: at least 1, and at most BatchCapacity() - 1 so that a launch holds a
    // buffer or more)
    uint32_t Depth() const
    {
        const uint32_t b = BatchCapacity();
        return b < 3u ? 1u : std::min(depth_env, b - 1u);
    }
    bool Pending() const { return !queue.empty() || !flights.empty(); }
    uint32_t PendingCount() const  // completions queued or in flight
    {
        uint32_t n = (uint32_t)queue.size();
        for (const Flight& f : flights) n += (uint32_t)f.q.size();
        return n;
    }
    // The filling batch has to be flushed before [src, src + n) can join it: a batch verified in place takes no
    // staged entry, and the staging arena is full.
    bool MustFlushBefore(const char* src, uint32_t n) const
    {
        if (queue.empty() || ZeroCopy(src, n)) return false;
        return queue_in_ring || stage_used + StageSlot(n) > StageCapacity();
    }
    int Enqueue(const char* src, const Queued& e);  // one completed recv joins the filling batch
    bool Full() const { return queue.size() >= LaunchAt(); }
    // It is time to ask, and the oldest batch in flight has finished: every query_period-th completion (a query costs
    // about a microsecond, a completion of 64 KiB arrives every ~1.3 us at 50 GB/s).
    bool VerdictsDue() const
    {
        return query_period != 0 && (queue.size() & (query_period - 1u)) == 0 && InflightDone();
    }
    int RetireDone();  // applies the batches in flight whose kernels have finished, oldest first
    int Rotate();      // the filling batch is full: launch it and keep receiving
    int Flush();       // applies everything: the batches in flight, then the filling one

private:
    // pipelined batches (ring mode, device verify): a full batch is launched and left running while the next one
    // fills in another set of stage_desc/stage_res; up to Depth() batches run at once. The oldest one's verdicts are
    // applied when a launch would exceed Depth(), as soon as CompleteIo sees its kernel done, at any non-benign
    // completion and at Flush. A failing batch discards the ones launched after it.
    struct Flight {
        std::vector<Queued> q;
        hipEvent_t done = nullptr;  // recorded after the batch's launch, queried by CompleteIo
        uint32_t set = 0;           // its descriptor / result set
    };

    cts_io_pattern& owner;
    PatternDevice& dev;
    const uint32_t batch_buffers;  // cts_pattern_config: 0 = 1024 buffers, 64 MiB
    const uint64_t batch_bytes;
    const char* ring_host = nullptr;
    const uint8_t* ring_dev = nullptr;
    uint64_t ring_bytes = 0;

    std::vector<Queued> queue;  // the filling batch
    bool queue_in_ring = false;
    uint64_t stage_used = 0;
    uint32_t desc_set = 0;                   // the set the filling batch uses
    std::deque<Flight> flights;              // oldest first
    std::vector<hipEvent_t> spare_events;    // events of retired flights, for reuse
    std::vector<std::vector<Queued>> spare_queues;  // their entry vectors (capacity kept across batches)
    Pinned stage, stage_desc, stage_res;     // the staging arena; every set's descriptors and results
    std::vector<uint8_t> hstage;             // the same three when a hook verifies
    std::vector<cts_buf_desc> hdesc;
    std::vector<cts_verify_result> hres;
    // Batches in flight per connection (CTS_DEFERRED_DEPTH, 1-4; default 2). Each launch holds
    // BatchCapacity() / (Depth() + 1) buffers, so a verdict is still known within BatchCapacity() completions.
    // Config 1 over loopback, four boxes, 40 alternated rounds: 2 beat 1 in 29.
    const uint32_t depth_env = (uint32_t)std::min(std::max(env_long("CTS_DEFERRED_DEPTH", 2), 1L), 4L);
    // VerdictsDue's period (a power of two; CTS_DEFERRED_QUERY_PERIOD, default 16; 0 = never: verdicts land at the
    // next Rotate / Flush only)
    const uint32_t query_period = [] {
        const long n = env_long("CTS_DEFERRED_QUERY_PERIOD", 16);
        uint32_t p = n > 0 ? 1u : 0u;
        while (p != 0 && p < (uint32_t)std::min<long>(n, 1L << 20)) p <<= 1;
        return p;
    }();

    uint64_t StageCapacity() const { return batch_bytes ? batch_bytes : (64ull << 20); }
    static uint64_t StageSlot(uint32_t n) { return ((uint64_t)n + 15u) & ~15ull; }
    uint32_t Sets() const { return Depth() + 1u; }  // descriptor / result sets: the filling batch + those in flight
    // Completions queued before a batch goes to the device. Pipelined, each launch holds BatchCapacity() / Sets():
    // the oldest launch is retired at the latest when the filling one is full and Depth() are in flight, so every
    // verdict is known within BatchCapacity() completions of its own (fewer when a kernel is seen done earlier).
    uint32_t LaunchAt() const
    {
        const uint32_t b = BatchCapacity();
        return dev.OnDevice() && queue_in_ring ? std::max(1u, b / Sets()) : b;
    }
    // [p, p + n) is verified where it lies: it is in the ring and the filling batch is not a staged one
    bool ZeroCopy(const char* p, uint32_t n) const
    {
        return ring_host != nullptr && p >= ring_host && p + n <= ring_host + ring_bytes &&
               (queue.empty() || queue_in_ring);
    }
    bool InflightDone() const  // a non-blocking event query
    {
        return !flights.empty() && flights.front().done && hipEventQuery(flights.front().done) == hipSuccess;
    }
    cts_buf_desc* Descs();  // of the filling batch
    const cts_verify_result* Results(uint32_t set) const
    {
        return reinterpret_cast<const cts_verify_result*>(stage_res.host) + (size_t)set * BatchCapacity();
    }
    int EnsureBatchDescs();
    int Launch(bool in_flight);
    int RetireOldest();
    int Retire();
};

}  // namespace cts
