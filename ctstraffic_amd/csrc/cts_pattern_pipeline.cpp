// cts_pattern_pipeline.cpp — the DEFERRED batch pipeline (cts_pattern_pipeline.hpp): queue, launch, retire.
#include "cts_pattern_pipeline.hpp"

#include <algorithm>
#include <cstring>

#include "cts_pattern_impl.hpp"  // cts_io_pattern::ApplyVerdicts, the one call back into the pattern

namespace cts {

DeferredPipeline::~DeferredPipeline()
{
    EngineDevice on(dev.engine);
    for (Flight& f : flights) spare_events.push_back(f.done);
    for (hipEvent_t e : spare_events)
        if (e) (void)hipEventDestroy(e);
}

cts_buf_desc* DeferredPipeline::Descs()
{
    if (dev.hook != nullptr) return hdesc.data();
    return reinterpret_cast<cts_buf_desc*>(stage_desc.host) + (size_t)desc_set * BatchCapacity();
}

int DeferredPipeline::EnsureBatchDescs()  // every set
{
    if (dev.hook != nullptr) {
        if (hdesc.size() < BatchCapacity()) {
            hdesc.resize(BatchCapacity());
            hres.resize(BatchCapacity());
        }
        return CTS_OK;
    }
    if (dev.engine == nullptr) return CTS_E_INVALID;
    if (stage_desc.host != nullptr) return CTS_OK;
    const uint64_t n = (uint64_t)Sets() * BatchCapacity();
    const int rc = stage_desc.alloc(dev.engine, sizeof(cts_buf_desc) * n);
    return rc != CTS_OK ? rc : stage_res.alloc(dev.engine, sizeof(cts_verify_result) * n);
}

int DeferredPipeline::Enqueue(const char* src, const Queued& e)
{
    int rc = EnsureBatchDescs();
    if (rc != CTS_OK) return rc;
    uint64_t at = 0;
    queue_in_ring = ZeroCopy(src, e.transferred);
    if (queue_in_ring) {
        at = (uint64_t)(src - ring_host);  // the batch descriptor points at the recv buffer itself
    } else {
        const uint64_t slot = StageSlot(e.transferred);
        const uint64_t cap = std::max<uint64_t>(StageCapacity(), slot);
        uint8_t* base = nullptr;
        if (dev.hook != nullptr) {
            if (hstage.size() < cap) hstage.resize(cap);
            base = hstage.data();
        } else {
            if (stage.bytes < cap) {
                stage.release();
                if ((rc = stage.alloc(dev.engine, cap)) != CTS_OK) return rc;
            }
            base = stage.host;
        }
        if (e.transferred) std::memcpy(base + stage_used, src, e.transferred);
        at = stage_used;
        stage_used += slot;
    }
    Descs()[queue.size()] = cts_buf_desc{at, e.transferred, e.expected, 0, 0};
    queue.push_back(e);
    return CTS_OK;
}

// The one place a batch goes to the device: `queue` (descriptor set desc_set) on the pattern's stream, async. In
// flight, it leaves `queue` for a Flight with an event behind it and the next set starts filling; otherwise (Flush)
// it stays in `queue` and the caller waits for the stream.
// a Flush whose wait runs out leaves `queue` filled, so the next Flush launches the same batch
// again. Launching it in flight here too (and retiring it) is the fix; nothing else knows a batch was launched.
int DeferredPipeline::Launch(bool in_flight)
{
    int rc = dev.EnsureStream();
    if (rc != CTS_OK) return rc;
    uint32_t maxlen = 0;
    for (const auto& q : queue) maxlen = std::max(maxlen, q.transferred);
    const size_t set = (size_t)desc_set * BatchCapacity();
    rc = cts_verify(dev.engine, queue_in_ring ? ring_dev : stage.dev, queue_in_ring ? ring_bytes : stage.bytes,
                    reinterpret_cast<cts_buf_desc*>(stage_desc.dev) + set, (uint32_t)queue.size(), maxlen,
                    reinterpret_cast<cts_verify_result*>(stage_res.dev) + set, nullptr, nullptr, 0, dev.stream);
    if (rc != CTS_OK || !in_flight) return rc;
    EngineDevice on(dev.engine);
    hipEvent_t e = nullptr;
    if (!spare_events.empty()) {
        e = spare_events.back();
        spare_events.pop_back();
    } else if ((e = dev.NewEvent()) == nullptr) {
        return CTS_E_HIP;
    }
    if (hipEventRecord(e, dev.stream) != hipSuccess) {
        spare_events.push_back(e);
        return CTS_E_HIP;
    }
    flights.push_back(Flight{{}, e, desc_set});
    flights.back().q.swap(queue);
    if (!spare_queues.empty()) {
        queue.swap(spare_queues.back());
        spare_queues.pop_back();
    }
    queue.clear();
    desc_set = (desc_set + 1u) % Sets();
    return CTS_OK;
}

// Waits for the oldest in-flight batch and applies its verdicts. A failure in it takes back everything completed
// after the failing buffer: the batches launched after it and the filling batch are dropped.
int DeferredPipeline::RetireOldest()
{
    if (flights.empty()) return CTS_OK;
    Flight& f = flights.front();
    const auto w0 = std::chrono::steady_clock::now();
    const hipError_t wr = dev.WaitInflight(f.done);
    dev.AddVerifyWait(w0);
    if (wr != hipSuccess) return CTS_E_HIP;
    const bool failed = owner.ApplyVerdicts(f.q, Results(f.set));
    spare_events.push_back(f.done);
    f.q.clear();
    spare_queues.push_back(std::move(f.q));
    flights.pop_front();
    if (!failed) return CTS_OK;
    // the later kernels' verdicts are never applied; they finish before their sets are written again
    if (!flights.empty() && dev.WaitIdle() != hipSuccess) return CTS_E_HIP;
    for (Flight& g : flights) spare_events.push_back(g.done);
    flights.clear();
    queue.clear();
    stage_used = 0;
    return kBatchFailed;
}

int DeferredPipeline::Retire()  // every in-flight batch, oldest first, up to a failing one
{
    int rc = CTS_OK;
    while (rc == CTS_OK && !flights.empty()) rc = RetireOldest();
    return rc;
}

int DeferredPipeline::RetireDone()
{
    int rc = CTS_OK;
    while (rc == CTS_OK && InflightDone()) rc = RetireOldest();
    return rc;
}

// Pipelined, the oldest in-flight batch is retired first if Depth() are running.
int DeferredPipeline::Rotate()
{
    if (!dev.OnDevice() || !queue_in_ring) return Flush();
    int rc = CTS_OK;
    while (rc == CTS_OK && flights.size() >= Depth()) rc = RetireOldest();
    if (rc != CTS_OK || queue.empty()) return rc;  // (an in-flight batch failed: the filling one went with it)
    return Launch(true);
}

int DeferredPipeline::Flush()
{
    const int rr = Retire();
    if (rr != CTS_OK || queue.empty()) return rr;
    const cts_verify_result* res = nullptr;
    if (dev.hook != nullptr) {
        const uint8_t* arena = queue_in_ring ? reinterpret_cast<const uint8_t*>(ring_host) : hstage.data();
        if (dev.hook(dev.hook_ctx, arena, queue_in_ring ? ring_bytes : stage_used, hdesc.data(), (uint32_t)queue.size(),
                     hres.data()) != 0)
            return CTS_E_INVALID;
        res = hres.data();
    } else {
        const int rc = Launch(false);
        if (rc != CTS_OK) return rc;
        const auto w0 = std::chrono::steady_clock::now();
        const hipError_t wr = dev.StreamWait(50);  // (destroy's flush of the filling batch: up to the deadline)
        dev.AddVerifyWait(w0);
        if (wr != hipSuccess) return CTS_E_HIP;
        res = Results(desc_set);
    }
    const bool failed = owner.ApplyVerdicts(queue, res);
    queue.clear();
    stage_used = 0;
    return failed ? kBatchFailed : CTS_OK;
}

}  // namespace cts
