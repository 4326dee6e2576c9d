// cts_pattern_media_stream.cpp — the MediaStream (UDP) patterns of the ctsIoPattern mirror behind the same
// cts_io_pattern_* ABI: the server (ctsTraffic/ctsIOPattern.cpp:1100-1175) and the client with its two timers
// (ctsTraffic/ctsIOPatternMediaStream.cpp:46-530; the frame accounting is cts_media_stream.cpp's).
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <exception>
#include <system_error>
#include <thread>

#include "cts_media_stream_client.hpp"
#include "cts_pattern_impl.hpp"

namespace cts {
namespace {

uint16_t load_u16(const char* p)
{
    uint16_t v;
    std::memcpy(&v, p, sizeof v);
    return v;
}
int64_t load_i64(const char* p)
{
    int64_t v;
    std::memcpy(&v, p, sizeof v);
    return v;
}

// ctsIoPatternMediaStreamServer (ctsIOPattern.cpp:1100-1175): the connection-id datagram, then one tracked send
// of one frame per frame, timed to the frame rate.
struct MediaStreamServer : cts_io_pattern {
    MediaStreamServer(const cts_pattern_config& c, uint32_t maxbuf)
        : cts_io_pattern(c, maxbuf, 1),  // one recv buffer: the connection-id datagram is built in it
          m_frameSizeBytes(c.buffer_size_low), m_frameRateFps(c.ms_frames_per_second)
    {
    }
    enum class ServerState { NotStarted, IdSent, IoStarted } m_state = ServerState::NotStarted;
    // its one recv buffer only ever holds the connection-id datagram, and it receives nothing to verify (no ring)
    uint32_t RecvSlotBytes() const override { return (CTS_UDP_CONNECTION_ID_HEADER_LENGTH + 15u) & ~15u; }
    bool VerifiesRecvs() const override { return false; }
    int64_t m_baseTimeMilliseconds = 0;
    uint32_t m_frameSizeBytes;
    uint32_t m_currentFrameRequested = 0;
    uint32_t m_currentFrameCompleted = 0;
    uint32_t m_frameRateFps;
    uint32_t m_currentFrame = 1;
    int64_t m_bitsReceived = 0;  // m_statistics.m_bitsReceived (counts the bits sent)

    cts_task GetNextTaskFromPattern() override  // :1119-1154
    {
        cts_task t = EmptyTask();
        switch (m_state) {
        case ServerState::NotStarted: {
            // ctsMediaStreamMessage::MakeConnectionIdTask (ctsMediaStreamProtocol.hpp:389-405) over a writable
            // (recv) buffer of c_udpDatagramConnectionIdHeaderLength bytes
            t = CreateNewTask(CTS_TASK_RECV, CTS_UDP_CONNECTION_ID_HEADER_LENGTH);
            if (t.buffer_length != CTS_CONNECTION_ID_LENGTH + CTS_UDP_FLAG_LENGTH)
                throw FailFast{"MakeConnectionIdTask: the task's buffer length is not the connection-id datagram length"};
            const uint16_t flag = CTS_UDP_FLAG_ID;
            std::memcpy(t.buffer, &flag, CTS_UDP_FLAG_LENGTH);
            std::memcpy(t.buffer + CTS_UDP_FLAG_LENGTH, connection_id, CTS_CONNECTION_ID_LENGTH);
            t.io_action = CTS_TASK_SEND;
            t.buffer_type = CTS_BUFFER_UDP_CONNECTION_ID;
            t.track_io = 0;
            m_state = ServerState::IdSent;
            break;
        }
        case ServerState::IdSent:
            m_baseTimeMilliseconds = NowMs();
            m_state = ServerState::IoStarted;
            [[fallthrough]];
        case ServerState::IoStarted:
            if (m_currentFrameRequested < m_frameSizeBytes) {
                t = CreateTrackedTask(CTS_TASK_SEND, m_frameSizeBytes);
                // the time of this frame relative to now
                t.time_offset_ms = m_baseTimeMilliseconds + ((int64_t)m_currentFrame * 1000LL / m_frameRateFps) - NowMs();
                m_currentFrameRequested += t.buffer_length;
            }
            break;
        }
        return t;
    }

    PatternError CompleteTaskBackToPattern(const cts_task& t, uint32_t currentTransfer) override  // :1156-1173
    {
        if (t.buffer_type != CTS_BUFFER_UDP_CONNECTION_ID) {
            const int64_t bits = (int64_t)currentTransfer * 8;
            cts::udp_status_add_bits(bits);
            m_bitsReceived += bits;
            m_currentFrameCompleted += currentTransfer;
            if (m_currentFrameCompleted == m_frameSizeBytes) {
                ++m_currentFrame;
                m_currentFrameRequested = 0;
                m_currentFrameCompleted = 0;
            }
        }
        return PatternError::NoError;
    }

    int UdpStats(cts_media_stream_stats* o) override
    {
        *o = cts_media_stream_stats{};
        o->bits_received = m_bitsReceived;
        o->last_error = m_lastError;
        return CTS_OK;
    }
};

// ctsIoPatternMediaStreamClient (ctsIOPatternMediaStream.cpp:46-530): untracked recvs of one datagram each;
// every data datagram's payload is verified (on the GPU) and booked to its frame in the jitter queue, which
// the renderer timer drains at the frame rate. The frame accounting is the one cts_media_stream_client_*
// exports (cts_media_stream.cpp); the pattern adds the recv tasks, the header checks, the verify and the timers.
struct MediaStreamClient : cts_io_pattern {
    MediaStreamClient(const cts_pattern_config& c, uint32_t maxbuf)
        : cts_io_pattern(c, maxbuf, c.pre_post_recvs),
          m_frameRateMsPerFrame(1000.0 / (double)c.ms_frames_per_second), m_frameSizeBytes(c.buffer_size_low),
          m_recvNeeded(c.pre_post_recvs), m_maxDatagramSize(c.ms_datagram_max_size), manual(c.ms_manual_timers != 0)
    {
    }
    void StopTimers() override
    {
        {
            std::lock_guard<std::recursive_mutex> lk(mu);
            stop = true;
            start_due = render_due = -1;
        }
        cv.notify_all();
        if (timer_thread.joinable()) timer_thread.join();
    }
    ~MediaStreamClient() override
    {
        StopTimers();
        if (ms != nullptr) (void)cts_media_stream_client_destroy(ms);
        EngineDevice on(dev.engine);
        if (d_sums != nullptr) (void)hipFreeAsync(d_sums, dev.stream);
        if (dev.stream != nullptr) (void)hipStreamSynchronize(dev.stream);
    }

    cts_media_stream_client* ms = nullptr;  // the jitter queue and frame accounting
    int64_t m_baseTimeMilliseconds = 0;
    const double m_frameRateMsPerFrame;
    const uint32_t m_frameSizeBytes;
    uint32_t m_recvNeeded;
    const uint32_t m_maxDatagramSize;
    uint64_t datagrams = 0;  // recv completions handed to CompleteTaskBackToPattern
    // the two timers (ctsIOPatternMediaStream.cpp:321-364): when each is due on the pattern clock, -1 = not armed
    const bool manual;
    int64_t start_due = -1, render_due = -1;
    bool stop = false;
    std::condition_variable_any cv;
    std::thread timer_thread;

    bool NeedsVerifier(const cts_task& t) const override  // every recv is a datagram to verify
    {
        return cfg.verify_buffers && t.io_action == CTS_TASK_RECV;
    }
    // every recv is one datagram of min(frame, DatagramMaxSize) bytes (GetNextTaskFromPattern): a slot of a frame's
    // size would leave 97 % of a README-sized (52083-B) slot unused, per slot of the DEFERRED ring
    uint32_t RecvSlotBytes() const override
    {
        return (std::max(std::min(m_frameSizeBytes, m_maxDatagramSize), 16u) + 15u) & ~15u;
    }

    // ---- DEFERRED: batched datagram verify (round 3) ---------------------------------------------------------
    // A data datagram whose header the CPU has checked (it is in host memory) stays in its recv-ring slot and is
    // queued; a batch goes to the GPU's frame-sum receive pass (cts_media_stream_verify_frames), whose sums are
    // applied as CompleteTaskBackToPattern would have applied each datagram (the jitter window moves only at a
    // render tick, and every tick flushes first). A batch holding a corrupt payload is replayed datagram by
    // datagram from the compact statuses (cts_media_stream_verify_status) up to that datagram, which fails the
    // stream with the first mismatch cts_verify finds in its payload. Anything else that completes (zero-byte,
    // short, unknown or ID datagram, Abort) flushes first, so the stream's status and counters are the reference's;
    // only the completion that reports a corrupt datagram comes later (at most one batch).
    struct MsQueued {
        uint64_t offset;     // of the datagram in the recv ring
        uint32_t completed;  // its bytes
        uint32_t index;      // its completion index
    };
    std::vector<MsQueued> msq, msq_spare;
    Pinned ms_desc, ms_sums, ms_status, ms_res;
    // the frame-sum pass adds into its totals and frame bytes with device-scope atomics: they live in device memory
    // (as cts_media_stream_verify_frames documents them), back to back in one allocation (the totals' shards, then one
    // u64 per window slot), so one memset clears them and one copy brings them to the pinned ms_sums: per render tick
    // a connection pays one launch, one memset and one copy (round 4; two of each before)
    static constexpr size_t kTotalsWords = CTS_FRAME_TOTAL_SHARDS * 4u;
    uint64_t* d_sums = nullptr;
    uint32_t d_sums_cap = 0;  // window slots
    // stream-ordered (hipMallocAsync / hipFreeAsync on the pattern's stream): a plain hipFree waits for the whole
    // device, and with other connections posting to the engine's resident SYNC mailbox grid that can be a long time
    int DeviceAlloc(void** p, size_t bytes)
    {
        return hipMallocAsync(p, bytes, dev.stream) == hipSuccess ? CTS_OK : CTS_E_NOMEM;
    }
    // A launch's status and then the wait for the pattern's stream (`sleeping`: a short kernel behind a launch, sleep
    // rather than spin while it runs): a DeviceError unless both are good.
    void WaitOrThrow(int rc, bool sleeping = false)
    {
        if (rc == CTS_OK && (sleeping ? dev.SleepSync(20) : dev.StreamWait(20)) != hipSuccess) rc = CTS_E_HIP;
        if (rc != CTS_OK) throw DeviceError{rc};
    }

    void CountVerified(const MsQueued& q)
    {
        ++buffers_verified;
        bytes_verified += q.completed - CTS_UDP_DATA_HEADER_LENGTH;
    }
    void ApplyClean(const MsQueued& q)
    {
        const char* b = ring_base + q.offset;
        const cts::MsDatagram d{load_i64(b + CTS_UDP_FLAG_LENGTH), load_i64(b + 8), load_i64(b + 16), q.completed};
        cts::ms_client_apply_data(ms, d, ReceiverQpc(), 1000000000LL);
        CountVerified(q);
    }
    static int64_t ReceiverQpc()
    {
        return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
            .count();
    }
    void FailQueued(const MsQueued& q, const cts_verify_result& r)
    {
        RecordFailure(q.index, q.completed - CTS_UDP_DATA_HEADER_LENGTH, r, 0);
        CountVerified(q);
        UpdateLastPatternError(Fail(q.index, PatternError::CorruptedBytes));
    }

    // Verifies and applies every queued datagram; true when one of them failed the stream.
    bool FlushMs()
    {
        if (msq.empty()) return false;
        const uint32_t n = (uint32_t)msq.size();
        // the batch moves to msq_spare and msq takes msq_spare's storage: both keep their capacity across ticks
        std::vector<MsQueued>& q = msq_spare;
        q.clear();
        q.swap(msq);
        if (dev.hook != nullptr) {  // device-less harness: the batch verifier on the payload spans, then one by one
            std::vector<cts_buf_desc> d(n);
            std::vector<cts_verify_result> r(n);
            for (uint32_t i = 0; i < n; ++i)
                d[i] = cts_buf_desc{q[i].offset, q[i].completed, 0u, 0u, CTS_UDP_DATA_HEADER_LENGTH};
            if (dev.hook(dev.hook_ctx, reinterpret_cast<const uint8_t*>(ring_base), ring_bytes, d.data(), n, r.data()) != 0)
                throw DeviceError{CTS_E_INVALID};
            for (uint32_t i = 0; i < n; ++i) {
                if (!r[i].pass) {
                    FailQueued(q[i], r[i]);
                    return true;
                }
                ApplyClean(q[i]);
            }
            return false;
        }
        cts_engine* const engine = dev.engine;
        EngineDevice on(engine);
        int rc = dev.EnsureStream();
        const hipStream_t stream = dev.stream;
        if (rc == CTS_OK && ms_desc.host == nullptr) {
            const uint32_t b = BatchCapacity();
            if ((rc = ms_desc.alloc(engine, sizeof(cts_buf_desc) * (uint64_t)b)) == CTS_OK &&
                (rc = ms_status.alloc(engine, sizeof(cts_datagram_status) * (uint64_t)b)) == CTS_OK)
                rc = ms_res.alloc(engine, sizeof(cts_verify_result) + sizeof(cts_buf_desc));
        }
        static_assert(kTotalsWords * sizeof(uint64_t) == (size_t)CTS_FRAME_TOTAL_SHARDS * 32u, "the totals block");
        cts_frame_window w{};
        if (rc == CTS_OK) rc = cts_media_stream_client_window(ms, &w);
        if (rc == CTS_OK && (d_sums == nullptr || d_sums_cap < std::max(w.frames, 1u))) {
            ms_sums.release();
            if (d_sums != nullptr) (void)hipFreeAsync(d_sums, stream);
            d_sums = nullptr;
            d_sums_cap = 0;
            const uint32_t cap = std::max(w.frames, 1u);
            const uint64_t bytes = sizeof(uint64_t) * (kTotalsWords + (uint64_t)cap);
            void* p = nullptr;
            if ((rc = DeviceAlloc(&p, bytes)) == CTS_OK && (rc = ms_sums.alloc(engine, bytes)) == CTS_OK) {
                d_sums = static_cast<uint64_t*>(p);
                d_sums_cap = cap;
            } else if (p != nullptr) {
                (void)hipFreeAsync(p, stream);
            }
        }
        if (rc != CTS_OK) throw DeviceError{rc};
        auto* descs = reinterpret_cast<cts_buf_desc*>(ms_desc.host);
        for (uint32_t i = 0; i < n; ++i) descs[i] = cts_buf_desc{q[i].offset, q[i].completed, 0u, 0u, 0u};
        rc = cts_media_stream_verify_frames(engine, recv_pinned.dev, recv_pinned.bytes,
                                            reinterpret_cast<const cts_buf_desc*>(ms_desc.dev), n, &w, d_sums,
                                            d_sums + kTotalsWords, nullptr, stream);
        if (rc == CTS_OK && hipMemcpyAsync(ms_sums.host, d_sums, sizeof(uint64_t) * (kTotalsWords + (uint64_t)w.frames),
                                           hipMemcpyDeviceToHost, stream) != hipSuccess)
            rc = CTS_E_HIP;
        WaitOrThrow(rc, true);
        cts_frame_totals t{};
        (void)cts_frame_totals_fold(ms_sums.host, &t);
        if (t.exceptions == 0 && t.datagrams == n) {
            // every datagram clean: the sums are CompleteTaskBackToPattern over the batch (no sender timestamps)
            const int st = cts_media_stream_client_complete_frames(ms, &w, &t,
                                                                   reinterpret_cast<const uint64_t*>(ms_sums.host) +
                                                                       kTotalsWords,
                                                                   n, ReceiverQpc(), 1000000000LL);
            if (st < 0) throw DeviceError{st};
            for (const MsQueued& e : q) CountVerified(e);
            return false;
        }
        // a corrupt payload in the batch: replay from the statuses up to it
        WaitOrThrow(cts_media_stream_verify_status(engine, recv_pinned.dev, recv_pinned.bytes,
                                                   reinterpret_cast<const cts_buf_desc*>(ms_desc.dev), n,
                                                   reinterpret_cast<cts_datagram_status*>(ms_status.dev), nullptr, stream));
        const auto* st = reinterpret_cast<const cts_datagram_status*>(ms_status.host);
        for (uint32_t i = 0; i < n; ++i) {
            if (st[i].pass) {
                ApplyClean(q[i]);
                continue;
            }
            // the first mismatch of its payload (the reference prints it, ctsIOPattern.cpp:761-772)
            // (the descriptor first: the C ABI wants it 8-byte aligned, the result 4-byte aligned)
            *reinterpret_cast<cts_buf_desc*>(ms_res.host) =
                cts_buf_desc{q[i].offset, q[i].completed, 0u, 0u, CTS_UDP_DATA_HEADER_LENGTH};
            WaitOrThrow(cts_verify(engine, recv_pinned.dev, recv_pinned.bytes,
                                   reinterpret_cast<const cts_buf_desc*>(ms_res.dev), 1, q[i].completed,
                                   reinterpret_cast<cts_verify_result*>(ms_res.dev + sizeof(cts_buf_desc)), nullptr,
                                   nullptr, 0, stream));
            FailQueued(q[i], *reinterpret_cast<const cts_verify_result*>(ms_res.host + sizeof(cts_buf_desc)));
            return true;
        }
        return false;
    }
    int FlushPending() override
    {
        (void)FlushMs();
        return GetCurrentStatus();
    }
    // FlushMs from a timer callback, which has no caller to return a device error to: the error fails the
    // pattern (a latched FAIL_FAST, as an inconsistency would). False when it has: the callback ends (SendDeviceAbort).
    bool TimerFlush()
    {
        try {
            (void)FlushMs();
        } catch (const DeviceError& d) {
            Latch("the batched datagram verify failed in a timer callback (status " + std::to_string(d.rc) + ")");
        }
        if (m_lastError != CTS_PATTERN_E_FAIL_FAST) return true;
        SendDeviceAbort();
        return false;
    }
    void Latch(const std::string& reason)  // a FAIL_FAST from the timer thread
    {
        if (fail_fast.empty()) fail_fast = reason;
        m_lastError = CTS_PATTERN_E_FAIL_FAST;
    }

    // The batched verify failed on the device: the stream cannot be rendered further, so it ends here as a stream
    // that cannot continue does (ctsIOPatternMediaStream.cpp:490-508: a FatalAbort task). Sent once, by whichever
    // timer saw the failure first (the START timer can run before the renderer has been armed).
    bool device_abort_sent = false;
    void SendDeviceAbort()
    {
        if (device_abort_sent) return;
        device_abort_sent = true;
        cts_task t = EmptyTask();
        t.io_action = CTS_TASK_FATAL_ABORT;
        SendTaskToCallback(t);
    }

    // SetNextTimer (:321-349): the renderer's next tick at base + offset frames; armed when more than 2 ms ahead
    // (always on the initial call)
    bool SetNextTimer(bool initial)
    {
        const int64_t due = m_baseTimeMilliseconds +
                            (int64_t)((double)cts::ms_client_timer_wheel_offset(ms) * m_frameRateMsPerFrame);
        if (!initial && due - NowMs() <= 2) return false;
        render_due = due;
        cv.notify_all();
        return true;
    }
    void SetNextStartTimer()  // :351-364
    {
        start_due = NowMs() + (int64_t)m_frameRateMsPerFrame + 500;
        cv.notify_all();
    }

    // StartCallback (:440-468): re-send START until the first datagram arrived
    void StartTimer()
    {
        static char kStart[] = "START";
        if (cts::ms_client_finished(ms)) return;
        if (!TimerFlush()) return;  // DEFERRED: the datagrams that arrived count
        if (!cts::ms_client_received_buffered_frames(ms)) {
            cts_task t = EmptyTask();
            t.io_action = CTS_TASK_SEND;
            t.track_io = 0;
            t.buffer = kStart;
            t.buffer_offset = 0;
            t.buffer_length = sizeof(kStart) - 1;
            t.buffer_type = CTS_BUFFER_STATIC;
            SetNextStartTimer();
            SendTaskToCallback(t);
        }
    }
    // TimerCallback (:470-530): render frames until the next tick lies in the future
    void RenderTimer()
    {
        bool scheduled = false;
        while (!scheduled) {
            if (cts::ms_client_finished(ms)) return;
            if (!TimerFlush()) return;  // DEFERRED: a tick renders what arrived before it
            const int code = cts::ms_client_tick(ms);
            if (code != 0) {
                cts_task t = EmptyTask();
                t.io_action = code == 2 ? CTS_TASK_FATAL_ABORT : CTS_TASK_ABORT;
                SendTaskToCallback(t);
                return;
            }
            scheduled = SetNextTimer(false);
        }
    }

    void TimerLoop()  // the threadpool timers: run each callback when it is due
    {
        std::unique_lock<std::recursive_mutex> lk(mu);
        while (!stop) {
            int64_t due = start_due;
            if (render_due >= 0 && (due < 0 || render_due < due)) due = render_due;
            if (due < 0) {
                cv.wait(lk);
                continue;
            }
            const int64_t now = NowMs();
            if (due > now) {
                // a bounded wait on the system clock: libstdc++ turns wait_for into pthread_cond_clockwait, which
                // ThreadSanitizer does not intercept (it then reports the pattern lock as double-locked); the
                // bound keeps a wall-clock step from stretching a wait
                cv.wait_until(lk, std::chrono::system_clock::now() + std::chrono::milliseconds(std::min<int64_t>(due - now, 50)));
                continue;
            }
            try {
                if (start_due >= 0 && start_due <= now) {
                    start_due = -1;
                    StartTimer();
                }
                if (!stop && render_due >= 0 && render_due <= now) {
                    render_due = -1;
                    RenderTimer();
                }
            } catch (const FailFast& f) {  // nothing may leave the timer thread
                Latch(f.reason);
            } catch (const DeviceError& d) {
                Latch("a timer callback failed (status " + std::to_string(d.rc) + ")");
            } catch (const std::exception& e) {  // e.g. bad_alloc growing a queue: latched, never std::terminate
                Latch(std::string("a timer callback threw: ") + e.what());
            }
        }
    }

    int FireTimer(int timer) override
    {
        if (timer == CTS_MS_TIMER_START) {
            start_due = -1;
            StartTimer();
        } else if (timer == CTS_MS_TIMER_RENDER) {
            render_due = -1;
            RenderTimer();
        } else {
            return CTS_E_INVALID;
        }
        return CTS_OK;
    }
    int Timers(int64_t* s, int64_t* r) override
    {
        if (s != nullptr) *s = start_due;
        if (r != nullptr) *r = render_due;
        return CTS_OK;
    }

    cts_task GetNextTaskFromPattern() override  // :115-138
    {
        if (m_baseTimeMilliseconds == 0) {
            // start the timers the first time the pattern is used: the thread first, so a thread that cannot start
            // leaves no armed timer behind and fails the pattern (a latched FAIL_FAST; nothing crosses the C ABI)
            if (!manual && !timer_thread.joinable()) {
                try {
                    timer_thread = std::thread([this] { TimerLoop(); });
                } catch (const std::system_error& e) {
                    throw FailFast{std::string("the MediaStream client's timer thread could not start: ") + e.what()};
                }
            }
            m_baseTimeMilliseconds = NowMs();
            SetNextStartTimer();
            (void)SetNextTimer(true);
        }
        cts_task t = EmptyTask();
        if (m_recvNeeded > 0) {
            // one datagram per recv; a zero where the header's sequence number goes
            t = CreateNewTask(CTS_TASK_RECV, std::min(m_frameSizeBytes, m_maxDatagramSize));
            std::memset(t.buffer, 0, sizeof(int64_t));
            --m_recvNeeded;
        }
        return t;
    }

    PatternError CompleteTaskBackToPattern(const cts_task& t, uint32_t completedBytes) override  // :140-272
    {
        if (t.io_action == CTS_TASK_ABORT) {
            if (!cts::ms_client_finished(ms)) throw FailFast{"processed an Abort before the stream was finished"};
            if (FlushMs()) return PatternError::NoError;  // DEFERRED: a queued datagram failed the stream first
            return PatternError::SuccessfullyCompleted;
        }
        if (t.io_action != CTS_TASK_RECV) return PatternError::NoError;  // a START send
        const uint64_t index = datagrams++;
        const bool queue_data = Deferred() && cfg.verify_buffers && completedBytes >= CTS_UDP_DATA_HEADER_LENGTH &&
                                load_u16(t.buffer) == CTS_UDP_FLAG_DATA && InRing(t.buffer, completedBytes);
        if (queue_data) {
            // DEFERRED: verified and applied with its batch (FlushMs)
            msq.push_back(MsQueued{(uint64_t)(t.buffer - ring_base), completedBytes, (uint32_t)index});
            ++m_recvNeeded;
            if (msq.size() >= BatchCapacity()) (void)FlushMs();
            return PatternError::NoError;
        }
        if (FlushMs()) return PatternError::NoError;  // the datagrams before this one first
        if (completedBytes == 0) {
            // the final recv may complete with zero bytes once the sender closed
            return cts::ms_client_finished(ms) ? PatternError::NoError : Fail(index, PatternError::TooFewBytes);
        }
        // ValidateBufferLengthFromTask (ctsMediaStreamProtocol.hpp:284-329); GetProtocolHeaderFromTask reads the
        // flag at m_buffer itself (:331-334)
        if (completedBytes < CTS_UDP_FLAG_LENGTH) return Fail(index, PatternError::TooFewBytes);
        const uint16_t flag = load_u16(t.buffer);
        if (flag == CTS_UDP_FLAG_DATA) {
            if (completedBytes < CTS_UDP_DATA_HEADER_LENGTH) return Fail(index, PatternError::TooFewBytes);
        } else if (flag == CTS_UDP_FLAG_ID) {
            if (completedBytes < CTS_UDP_CONNECTION_ID_HEADER_LENGTH) return Fail(index, PatternError::TooFewBytes);
            // SetConnectionIdFromTask (:336-347)
            std::memcpy(connection_id, t.buffer + t.buffer_offset + CTS_UDP_FLAG_LENGTH, CTS_CONNECTION_ID_LENGTH);
            ++m_recvNeeded;
            return PatternError::NoError;
        } else {
            return Fail(index, PatternError::TooFewBytes);
        }
        // VerifyBuffer of the payload: skip the data header, pattern offset 0 (:185-192)
        if (cfg.verify_buffers) {
            const uint32_t payload = completedBytes - CTS_UDP_DATA_HEADER_LENGTH;
            cts_verify_result r{};
            r.first_mismatch = payload;
            r.pass = 1;
            if (payload > 0) {
                cts_task vt = t;
                vt.buffer_offset = CTS_UDP_DATA_HEADER_LENGTH;
                vt.buffer_length -= CTS_UDP_DATA_HEADER_LENGTH;
                const int rc = VerifyNow(vt, payload, r);
                if (rc != CTS_OK) throw DeviceError{rc};
            }
            ++buffers_verified;
            bytes_verified += payload;
            if (!r.pass) {
                RecordFailure((uint32_t)index, payload, r, 0);
                return Fail(index, PatternError::CorruptedBytes);
            }
        }
        // GetSequenceNumberFromTask (buffer + offset + 2) and the sender's QPC / QPF as the client reads them
        // (m_buffer + 8, + 16: ctsIOPatternMediaStream.cpp:218-219)
        const cts::MsDatagram d{load_i64(t.buffer + t.buffer_offset + CTS_UDP_FLAG_LENGTH), load_i64(t.buffer + 8),
                                load_i64(t.buffer + 16), completedBytes};
        cts::ms_client_apply_data(ms, d, ReceiverQpc(), 1000000000LL);
        ++m_recvNeeded;
        return PatternError::NoError;
    }

    PatternError Fail(uint64_t index, PatternError e)
    {
        if (!udp_failed) {
            udp_failed = true;
            fail_datagram = (uint32_t)index;
        }
        return e;
    }
    bool udp_failed = false;
    uint32_t fail_datagram = 0;

    int UdpStats(cts_media_stream_stats* o) override
    {
        const int rc = cts_media_stream_client_stats(ms, o);
        if (rc != CTS_OK) return rc;
        o->datagrams = datagrams;
        o->last_error = m_lastError;
        o->fail_datagram = fail_datagram;
        o->has_failure = udp_failed ? 1u : 0u;
        return CTS_OK;
    }
};

}  // namespace

cts_io_pattern* NewMediaStreamServer(const cts_pattern_config& c, uint32_t maxbuf)
{
    return new MediaStreamServer(c, maxbuf);
}

int NewMediaStreamClient(const cts_pattern_config& c, uint32_t maxbuf, cts_io_pattern** out)
{
    auto* mc = new MediaStreamClient(c, maxbuf);
    const cts_media_stream_settings st{c.buffer_size_low, c.ms_datagram_max_size, c.ms_frames_per_second,
                                       c.ms_buffered_frames, c.ms_stream_length_frames};
    const int rc = cts_media_stream_client_create(&st, &mc->ms);
    if (rc == CTS_OK) *out = mc;
    else delete mc;
    return rc;
}

}  // namespace cts
