// cts_pattern_impl.hpp — private to the ctsIoPattern mirror: the process-wide state and the base pattern
// (ctsTraffic/ctsIOPattern.cpp:133-743) that cts_pattern.cpp defines, the MediaStream patterns
// (cts_pattern_media_stream.cpp) derive from and the DEFERRED pipeline (cts_pattern_pipeline.cpp) reports to.
#pragma once

#include <array>
#include <atomic>
#include <mutex>
#include <random>
#include <string>
#include <vector>

#include "cts_pattern_pipeline.hpp"
#include "cts_pattern_state.hpp"

namespace cts {

constexpr uint32_t kPatternSize = CTS_PATTERN_PERIOD;  // c_bufferPatternSize, ctsIOPattern.cpp:35
constexpr uint32_t kStatusIoRunning = CTS_STATUS_IO_RUNNING;
constexpr uint32_t kNoError = 0;
constexpr uint64_t kRioInvalid = CTS_RIO_INVALID_BUFFERID;

// ---- process-wide state (defined in cts_pattern.cpp) ----------------------------------------
// g_senderSharedBuffer / g_maximumBufferSize (ctsIOPattern.cpp:40-47): one per process.
struct SharedBuffer {
    std::mutex mu;
    char* host = nullptr;
    uint64_t bytes = 0;
    bool owned = false;       // pinned by cts_shared_buffer_init (hipHostFree on release)
    cts_engine* engine = nullptr;
    std::vector<char> receiver;  // g_receiverSharedBuffer (UseSharedBuffer, ctsIOPattern.cpp:138-152)
};
extern SharedBuffer g_shared;

// g_configSettings->rioFunctions: RIORegisterBuffer / RIODeregisterBuffer (cts_rio_functions_set)
struct RioFunctions {
    std::mutex mu;
    cts_rio_register_buffer_fn reg = nullptr;
    cts_rio_deregister_buffer_fn dereg = nullptr;
    void* ctx = nullptr;
};
extern RioFunctions g_rio;
struct RioRegisterFailed {};

int64_t NowMs();  // ctTimer::snap_qpc_as_msec, replaceable by cts_pattern_clock_set (the unit-test hook)

// TcpStatusDetails (ctsConfig.h:415) + a DataError tally
extern std::atomic<uint64_t> g_bytesSent, g_bytesRecv, g_dataErrors;

inline cts_task EmptyTask()
{
    cts_task t{};
    t.rio_buffer_id = kRioInvalid;
    return t;
}

}  // namespace cts

// ---- ctsIoPattern -----------------------------------------------------------------------------
struct cts_io_pattern {
    cts_io_pattern(const cts_pattern_config& c, uint32_t maxbuf, uint32_t recv_count);
    virtual ~cts_io_pattern();

    cts_pattern_config cfg;
    uint32_t max_buffer_size;
    // the pattern's critical section (ctsIoPattern::AcquireIoPatternLock, ctsIOPattern.h:405): every C-ABI call and
    // the MediaStream client's timer callbacks hold it; recursive, as a Windows critical section is, because a
    // callback may complete the task it hands out (ctsMediaStreamClient.cpp:317-331)
    mutable std::recursive_mutex mu;
    cts_task_callback m_callback = nullptr;  // RegisterCallback (ctsIOPattern.h:94-97)
    void* m_callback_ctx = nullptr;
    void SendTaskToCallback(const cts_task& t) const  // ctsIOPattern.h:333-339
    {
        if (m_callback != nullptr) m_callback(m_callback_ctx, &t);
    }
    cts::PatternState state;
    std::mt19937_64 rng;
    uint32_t recvCount;
    cts::PatternDevice dev;  // the engine (or the hook) with the pattern's stream and waits

    uint32_t m_sendPatternOffset = 0;
    uint32_t m_recvPatternOffset = 0;
    // send pacing (ctsIOPattern.h:204-205, 273-275); m_burstCount 0 with cfg.burst_count 0 = no burst
    int64_t m_quantumPeriodMs;
    int64_t m_bytesSendingPerQuantum;
    uint32_t m_burstCount;
    int64_t m_bytesSendingThisQuantum = 0;
    int64_t m_quantumStartTimeMs;
    uint32_t m_lastError = cts::kStatusIoRunning;
    std::vector<char*> m_recvBufferFreeList;
    cts::Pinned recv_pinned;            // m_recvBufferContainer when a device verifies in place
    std::vector<char> recv_plain;       // m_recvBufferContainer otherwise
    std::array<char, CTS_COMPLETION_MESSAGE_SIZE> m_completionMessageBuffer{};
    char connection_id[CTS_CONNECTION_ID_LENGTH] = {};
    std::string fail_fast;

    // ---- byte accounting and publication ---------------------------------------------------
    uint64_t bytes_sent = 0, bytes_recv = 0;
    // The reference's byte counters only ever Add (ctsStatistics.hpp:153-186; ctsIOPattern.cpp:505-521), and its
    // status timer prints their SnapValueDifference (ctsStatistics.hpp:363). A DEFERRED pattern therefore holds back
    // the bytes of every completion behind a recv whose verdict is not in yet: status_* is this pattern's running
    // contribution to TcpStatusDetails, published_* what it has added to g_bytesSent/g_bytesRecv so far. A batch that
    // verifies publishes up to its last buffer; a failing buffer publishes up to and including itself, and everything
    // after it is dropped unpublished (the reference never saw it). Nothing published is ever taken back.
    uint64_t status_sent = 0, status_recv = 0;
    uint64_t published_sent = 0, published_recv = 0;
    void Publish(uint64_t recv_to, uint64_t sent_to);
    // held back: completed, counted by the pattern, not yet published (only while a DEFERRED verdict is pending; every
    // completion accepted meanwhile is a pattern-requested send/recv, so the per-connection counters hold back the same)
    uint64_t HeldRecv() const { return status_recv - published_recv; }
    uint64_t HeldSent() const { return status_sent - published_sent; }
    bool VerdictsPending() const { return pipe.Pending(); }
    void PublishIfSettled()
    {
        if (!VerdictsPending()) Publish(status_recv, status_sent);
    }
    uint64_t buffers_verified = 0, bytes_verified = 0, buffers_failed = 0;
    uint64_t bytes_recv_at_failure = 0;
    uint32_t recv_completions = 0;
    bool has_failure = false;
    uint32_t fail_length = 0, fail_offset = 0, fail_completion = 0;
    uint8_t fail_expected = 0, fail_actual = 0;
    void RecordFailure(uint32_t completion, uint32_t transferred, const cts_verify_result& r, uint64_t recv_after);
    // Counts the verdicts of one DEFERRED batch (the pipeline's one call back); true if one of its buffers failed.
    bool ApplyVerdicts(const std::vector<cts::Queued>& q, const cts_verify_result* res);
    void RollbackAfter(const cts::Queued& f);

    // ---- verify ----------------------------------------------------------------------------
    cts::Pinned one;  // SYNC device verify: one descriptor + one result, pinned and device-mapped
    int VerifyNow(const cts_task& t, uint32_t transferred, cts_verify_result& r);
    // DEFERRED: completions queued, batches launched, verdicts not yet applied
    cts::DeferredPipeline pipe{*this, dev, cfg.batch_buffers, cfg.batch_bytes};
    uint32_t BatchCapacity() const { return pipe.BatchCapacity(); }
    bool Deferred() const { return cfg.verify_mode == CTS_VERIFY_DEFERRED; }
    // A pipeline call's result: a negative CTS_E_* as it is; otherwise whatever settled is published
    int Settle(int rc)
    {
        if (rc >= 0) PublishIfSettled();
        return rc;
    }
    int Flush()  // cts_io_pattern_flush
    {
        const int rc = Settle(pipe.Flush());
        return rc < 0 ? rc : GetCurrentStatus();
    }

    // DEFERRED zero-copy ring: the recv container holds (1 or 2) x BatchCapacity() + recvCount + 1
    // buffer slots and a completed buffer's slot is not handed out again before its batch was
    // verified, so a batch is verified in place (no staging copy)
    bool ring = false;
    uint32_t ring_slots = 0, ring_next = 0;
    uint32_t slot_bytes = 0;  // one recv buffer (RecvSlotBytes)
    char* ring_base = nullptr;
    uint64_t ring_bytes = 0;
    bool InRing(const char* p, uint32_t n) const { return ring && p >= ring_base && p + n <= ring_base + ring_bytes; }
    uint32_t RingSlot(const char* b) const { return (uint32_t)((size_t)(b - ring_base) / slot_bytes); }

    // RIO buffer ids (ctsIOPattern.h:219-269). m_receivingRioBufferIds pairs with
    // m_recvBufferFreeList entry for entry; in ring mode every ring slot has its own id
    // (ring_rio_ids) and a recycled slot goes back with its id.
    std::vector<uint64_t> m_receivingRioBufferIds;
    std::vector<uint64_t> m_sendingRioBufferIds;
    std::vector<uint64_t> ring_rio_ids;
    std::vector<uint64_t> rio_owned;  // every id registered by this pattern (deregistered at destroy)
    uint64_t m_rioConnectionId = cts::kRioInvalid;
    uint64_t m_rioCompletionMessage = cts::kRioInvalid;
    bool Rio() const { return cfg.registered_io != 0; }
    uint64_t RioRegister(char* buffer, uint32_t length);  // RIORegisterBuffer, THROW_WIN32 on failure
    uint64_t RioBufferIdCount() const  // ctsIOPattern.h:114-123
    {
        if (!Rio()) return 0;
        return m_receivingRioBufferIds.size() + m_sendingRioBufferIds.size() + 2;
    }

    // derived-pattern interface (ctsIOPattern.h:187-188)
    virtual cts_task GetNextTaskFromPattern() = 0;
    virtual cts::PatternError CompleteTaskBackToPattern(const cts_task&, uint32_t) = 0;
    // a completion of t must be verified (and so needs an engine or a hook)
    virtual bool NeedsVerifier(const cts_task& t) const
    {
        return cfg.verify_buffers && t.io_action == CTS_TASK_RECV && t.track_io;
    }
    // The bytes of one recv buffer (m_recvBufferContainer holds GetMaxBufferSize() per recv, ctsIOPattern.cpp:156-175).
    // The MediaStream patterns never post a recv that large: their slots are sized to what they post.
    virtual uint32_t RecvSlotBytes() const { return max_buffer_size; }
    // Whether its recvs carry data to verify (a DEFERRED pattern that does gets the zero-copy recv ring)
    virtual bool VerifiesRecvs() const { return cfg.verify_buffers != 0; }
    // MediaStream surface (cts_io_pattern_media_stream_*): CTS_E_INVALID for the TCP patterns
    virtual int FireTimer(int) { return CTS_E_INVALID; }
    virtual int Timers(int64_t*, int64_t*) { return CTS_E_INVALID; }
    virtual int UdpStats(cts_media_stream_stats*) { return CTS_E_INVALID; }
    // cts_io_pattern_flush: the DEFERRED queue of this pattern
    virtual int FlushPending() { return Flush(); }
    // Stops and joins any thread of the pattern's own that calls into it (the MediaStream client's timers).
    virtual void StopTimers() {}

    uint64_t GetTotalTransfer() const { return state.GetMaxTransfer(); }
    void SetTotalTransfer(uint64_t v) { state.SetMaxTransfer(v); }
    uint32_t GetIdealSendBacklog() const { return state.GetIdealSendBacklog(); }
    uint32_t UpdateLastError(uint32_t error);            // ctsIOPattern.h:344-365
    void UpdateLastPatternError(cts::PatternError e);    // ctsIOPattern.h:367-392
    int GetCurrentStatus() const  // ctsIOPattern.h:160-174
    {
        if (m_lastError == cts::kStatusIoRunning) return CTS_IO_CONTINUE;
        if (m_lastError == cts::kNoError) return CTS_IO_COMPLETED;
        return CTS_IO_FAILED;
    }

    int CreateRecvBuffers();   // ctsIOPattern.cpp:133-193
    int CreateRecvSlots();
    void RecycleRecvBuffer(const cts_task& t);
    void CreateSendBuffers();  // ctsIOPattern.cpp:195-217
    uint32_t GetBufferSize();  // ctsConfig.cpp:4679-4684
    int64_t SendTimeOffset(uint64_t size);
    cts_task CreateNewTask(uint8_t action, uint32_t maxTransfer);  // ctsIOPattern.cpp:550-743
    cts_task CreateTrackedTask(uint8_t a, uint32_t maxTransfer = 0)
    {
        cts_task t = CreateNewTask(a, maxTransfer);
        t.track_io = 1;
        return t;
    }
    cts_task InitiateIo();  // ctsIOPattern.cpp:251-356
    bool VerifyGate(const cts_task& t) const  // ctsIOPattern.cpp:475-479
    {
        return cfg.protocol == CTS_PROTOCOL_TCP && cfg.verify_buffers && t.io_action == CTS_TASK_RECV && t.track_io;
    }
    int CompleteIo(const cts_task& t, uint32_t transfer, uint32_t status);  // ctsIOPattern.cpp:364-534
};

namespace cts {
// cts_io_pattern_create's two MediaStream patterns (cts_pattern_media_stream.cpp); the client comes with its jitter
// queue (a CTS_E_* when that could not be made: *out stays null)
cts_io_pattern* NewMediaStreamServer(const cts_pattern_config& c, uint32_t maxbuf);
int NewMediaStreamClient(const cts_pattern_config& c, uint32_t maxbuf, cts_io_pattern** out);
}  // namespace cts
