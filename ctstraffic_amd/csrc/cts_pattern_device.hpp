// cts_pattern_device.hpp — what verifies for one ctsIoPattern mirror: the engine with the pattern's own stream and
// its waits, or the device-less harness hook. Its users are the SYNC one-buffer verify (cts_io_pattern::VerifyNow),
// the DEFERRED pipeline (cts_pattern_pipeline.cpp) and the MediaStream client's batch (MediaStreamClient::FlushMs).
#pragma once

#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <thread>

#include "cts_engine.h"
#include "cts_pattern.h"

namespace cts {

// An integer setting from the environment; unset or empty is `dflt`.
inline long env_long(const char* name, long dflt)
{
    const char* v = std::getenv(name);
    return v == nullptr || *v == 0 ? dflt : std::atol(v);
}

// Makes an engine's device current for the HIP calls a pattern makes itself (events, waits, copies, stream-ordered
// allocations) and gives the thread its own device back. IO threads and the MediaStream timer thread may have any
// device current, and an event must be created on the device of the stream it is recorded on.
struct EngineDevice {
    int prev = -1;
    bool switched = false;
    explicit EngineDevice(const cts_engine* e)
    {
        const int d = e != nullptr ? cts_engine_device(e) : -1;
        if (d < 0 || hipGetDevice(&prev) != hipSuccess) return;
        switched = prev != d && hipSetDevice(d) == hipSuccess;
    }
    ~EngineDevice()
    {
        if (switched) (void)hipSetDevice(prev);
    }
    EngineDevice(const EngineDevice&) = delete;
    EngineDevice& operator=(const EngineDevice&) = delete;
};

struct DeviceError {  // a verify call failed (HIP / engine status): CompleteIo returns it
    int rc;
};

class PatternDevice {
public:
    cts_engine* engine = nullptr;
    cts_batch_verifier hook = nullptr;  // cts_io_pattern_set_verifier: verifies instead of the engine
    void* hook_ctx = nullptr;
    hipStream_t stream = nullptr;
    // time the calls spent waiting for a DEFERRED batch's device verdicts (cts_pattern_stats.verify_wait_ns)
    uint64_t verify_wait_ns = 0;

    PatternDevice() = default;
    PatternDevice(const PatternDevice&) = delete;
    ~PatternDevice()
    {
        EngineDevice on(engine);
        if (sync_done) (void)hipEventDestroy(sync_done);
    }
    bool HasVerifier() const { return hook != nullptr || engine != nullptr; }
    bool OnDevice() const { return engine != nullptr && hook == nullptr; }  // kernels verify (DEFERRED: pipelined)

    int EnsureStream()  // on the engine's device, not the calling thread's current one
    {
        if (stream != nullptr) return CTS_OK;
        void* s = nullptr;
        const int rc = cts_engine_stream_create(engine, &s);
        stream = static_cast<hipStream_t>(s);
        return rc;
    }
    void CloseStream()  // the pattern is going: its kernels may still read its buffers (cheap when idle)
    {
        if (stream == nullptr) return;
        EngineDevice on(engine);
        (void)hipStreamSynchronize(stream);
        (void)cts_engine_stream_destroy(engine, stream);
        stream = nullptr;
    }

    // cts_io_pattern_destroy bounds its waits (a hung kernel must not hang teardown): while set, every wait below
    // polls its event and gives up with hipErrorNotReady once CTS_PATTERN_DESTROY_WAIT_MS (default 2000) have passed.
    void BoundWaits()
    {
        const long ms = env_long("CTS_PATTERN_DESTROY_WAIT_MS", 2000);
        bounded_wait = true;
        wait_deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(ms > 0 ? ms : 2000);
    }
    void UnboundWaits() { bounded_wait = false; }
    // Everything enqueued on the stream has finished (hipErrorNotReady: not within the bound).
    hipError_t WaitIdle(uint32_t step_us = 50) { return stream != nullptr ? SleepSyncImpl(step_us) : hipSuccess; }

    void AddVerifyWait(std::chrono::steady_clock::time_point t0)
    {
        verify_wait_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
                              std::chrono::steady_clock::now() - t0).count();
    }
    // Waits for everything enqueued on the pattern's stream. With retire_wait 2 (or a bounded wait) it sleeps in
    // `step_us` steps between non-blocking queries of an event recorded behind the work (the runtime's own waits
    // spin first). Counted as verify wait.
    hipError_t SleepSync(uint32_t step_us)
    {
        const auto w0 = std::chrono::steady_clock::now();
        const hipError_t rc = SleepSyncImpl(step_us);
        AddVerifyWait(w0);
        return rc;
    }
    // A plain wait for the pattern's stream, bounded like the others while cts_io_pattern_destroy runs.
    hipError_t StreamWait(uint32_t step_us)
    {
        if (bounded_wait) return SleepSyncImpl(step_us);
        EngineDevice on(engine);
        return hipStreamSynchronize(stream);
    }
    // An event for WaitInflight, to be recorded behind a launch (nullptr: none could be created).
    hipEvent_t NewEvent() const
    {
        hipEvent_t e = nullptr;
        const unsigned flags = hipEventDisableTiming | (retire_wait == 1 ? hipEventBlockingSync : 0u);
        return hipEventCreateWithFlags(&e, flags) == hipSuccess ? e : nullptr;
    }
    hipError_t WaitInflight(hipEvent_t done)  // the kernel behind `done`
    {
        EngineDevice on(engine);
        if (bounded_wait) return done != nullptr ? PollEvent(done, 50) : SleepSyncImpl(50);
        if (done == nullptr || retire_wait == 0) return hipStreamSynchronize(stream);
        if (retire_wait == 1) return hipEventSynchronize(done);
        return PollEvent(done, 50);
    }

private:
    // How a DEFERRED batch in flight is waited for (CTS_DEFERRED_BLOCKING_SYNC): 0 = spin in hipStreamSynchronize,
    // 1 = hipEventSynchronize on a blocking-sync event, 2 (default) = sleep in 50 us steps between non-blocking
    // queries of the event. With 8 connections sharing the PCIe link, the first two burned ~2 ms of receive-thread
    // CPU per wait, 1 as much as 0 (tools/pattern_cpu_probe, profiles/r03/pattern_cpu/): the runtime's blocking wait
    // spins before it sleeps
    const int retire_wait = [] {
        const long n = env_long("CTS_DEFERRED_BLOCKING_SYNC", 2);
        return n < 0 || n > 2 ? 2 : (int)n;
    }();
    bool bounded_wait = false;
    std::chrono::steady_clock::time_point wait_deadline{};
    hipEvent_t sync_done = nullptr;  // SleepSyncImpl's event

    hipError_t PollEvent(hipEvent_t e, uint32_t step_us)
    {
        for (;;) {
            const hipError_t q = hipEventQuery(e);
            if (q != hipErrorNotReady) return q;
            if (bounded_wait && std::chrono::steady_clock::now() > wait_deadline) return hipErrorNotReady;
            std::this_thread::sleep_for(std::chrono::microseconds(step_us));
        }
    }
    hipError_t SleepSyncImpl(uint32_t step_us)
    {
        EngineDevice on(engine);
        if (retire_wait != 2 && !bounded_wait) return hipStreamSynchronize(stream);
        if (sync_done == nullptr && hipEventCreateWithFlags(&sync_done, hipEventDisableTiming) != hipSuccess) {
            sync_done = nullptr;
            return bounded_wait ? hipErrorNotReady : hipStreamSynchronize(stream);
        }
        const hipError_t rc = hipEventRecord(sync_done, stream);
        if (rc != hipSuccess) return rc;
        return PollEvent(sync_done, step_us);
    }
};

}  // namespace cts
