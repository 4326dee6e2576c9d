// cts_pattern.cpp — host-side ctsIoPattern mirror (include/cts_pattern.h): the
// caller of the gfx950 fill/verify engine, restated from the reference
// (microsoft/ctsTraffic) so the IO functors can hand completed buffers over
// unchanged. This file: the base pattern, the TCP patterns and the C ABI.
//
//   PatternState     ctsTraffic/ctsIOPatternState.hpp:57-504 (ctsIoPatternState)    cts_pattern_state.hpp / .cpp
//   IoPattern        ctsTraffic/ctsIOPattern.cpp:133-743     (ctsIoPattern base)    cts_pattern_impl.hpp, here
//   Push/Pull/...    ctsTraffic/ctsIOPattern.cpp:796-1031    (concrete TCP patterns) here
//   MediaStream      ctsTraffic/ctsIOPattern.cpp:1100-1175   (UDP server)           cts_pattern_media_stream.cpp
//                    ctsTraffic/ctsIOPatternMediaStream.cpp  (UDP client; frame accounting in cts_media_stream.cpp)
//
// The two hot-path pieces go to the GPU: the sender buffer is written by the
// fill kernel (cts_shared_buffer_init) and VerifyBuffer runs the verify kernel
// on the pattern's pinned, device-mapped recv buffers (zero copy) — per
// completion (CTS_VERIFY_SYNC, VerifyNow) or batched (CTS_VERIFY_DEFERRED, cts_pattern_pipeline.cpp), on the
// pattern's own stream (cts_pattern_device.hpp).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <exception>
#include <new>

#include "cts_pattern_impl.hpp"
#include "cts_slices.hpp"

using namespace cts;

// ---- ctsIoPattern -----------------------------------------------------------------------------
cts_io_pattern::cts_io_pattern(const cts_pattern_config& c, uint32_t maxbuf, uint32_t recv_count)
    : cfg(c), max_buffer_size(maxbuf), state(c, maxbuf), rng(c.random_seed), recvCount(recv_count),
      m_quantumPeriodMs(c.tcp_bytes_per_second_period > 0 ? c.tcp_bytes_per_second_period : 100),
      // (bytes/sec) * (1 sec/1000 ms) * (x ms/Quantum) == (bytes/quantum) (ctsIOPattern.cpp:219-224)
      m_bytesSendingPerQuantum(c.tcp_bytes_per_second * m_quantumPeriodMs / 1000),
      m_burstCount(c.burst_count), m_quantumStartTimeMs(NowMs())
{
}

cts_io_pattern::~cts_io_pattern()
{
    dev.CloseStream();  // kernels may still read the ring; the members free their events and buffers after it
    // ~RioBufferId (ctsIOPattern.h:230-238) for every id this pattern registered
    if (!rio_owned.empty()) {
        std::lock_guard<std::mutex> lk(g_rio.mu);
        if (g_rio.dereg != nullptr)
            for (const uint64_t id : rio_owned) g_rio.dereg(g_rio.ctx, id);
    }
}

void cts_io_pattern::Publish(uint64_t recv_to, uint64_t sent_to)
{
    if (recv_to > published_recv) {
        g_bytesRecv.fetch_add(recv_to - published_recv);
        published_recv = recv_to;
    }
    if (sent_to > published_sent) {
        g_bytesSent.fetch_add(sent_to - published_sent);
        published_sent = sent_to;
    }
}

uint64_t cts_io_pattern::RioRegister(char* buffer, uint32_t length)
{
    uint64_t id = kRioInvalid;
    {
        std::lock_guard<std::mutex> lk(g_rio.mu);
        if (g_rio.reg != nullptr) id = g_rio.reg(g_rio.ctx, buffer, length);
    }
    if (id == kRioInvalid) throw RioRegisterFailed{};
    rio_owned.push_back(id);
    return id;
}

uint32_t cts_io_pattern::GetBufferSize()
{
    if (cfg.buffer_size_high == 0) return cfg.buffer_size_low;
    std::uniform_int_distribution<uint32_t> d(cfg.buffer_size_low, cfg.buffer_size_high);
    return d(rng);
}

uint32_t cts_io_pattern::UpdateLastError(uint32_t error)
{
    if (m_lastError == kStatusIoRunning) {
        const PatternError st = state.UpdateError(error);
        if (error == kNoError) {
            if (st != PatternError::ErrorIoFailed) m_lastError = kNoError;
        } else if (st == PatternError::ErrorIoFailed) {
            m_lastError = error;
            if (error == CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN) g_dataErrors.fetch_add(1);
        }
    }
    return m_lastError;
}

void cts_io_pattern::UpdateLastPatternError(PatternError e)
{
    switch (e) {
    case PatternError::CorruptedBytes: UpdateLastError(CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN); break;
    case PatternError::TooFewBytes: UpdateLastError(CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED); break;
    case PatternError::TooManyBytes: UpdateLastError(CTS_STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED); break;
    case PatternError::SuccessfullyCompleted: UpdateLastError(kNoError); break;
    case PatternError::NoError:
    case PatternError::ErrorIoFailed: break;
    }
}

int cts_io_pattern::CreateRecvBuffers()
{
    const int rc = CreateRecvSlots();
    if (rc != CTS_OK || !Rio()) return rc;
    // register the recv slots, then the connection id and the completion message (:141-192)
    if (ring) {
        ring_rio_ids.resize(ring_slots);
        for (uint32_t i = 0; i < ring_slots; ++i)
            ring_rio_ids[i] = RioRegister(ring_base + (size_t)i * slot_bytes, slot_bytes);
        for (const char* b : m_recvBufferFreeList) m_receivingRioBufferIds.push_back(ring_rio_ids[RingSlot(b)]);
    } else {
        const uint32_t len = cfg.use_shared_buffer ? (uint32_t)g_shared.bytes : slot_bytes;
        for (char* b : m_recvBufferFreeList) m_receivingRioBufferIds.push_back(RioRegister(b, len));
    }
    m_rioConnectionId = RioRegister(connection_id, CTS_CONNECTION_ID_LENGTH);
    m_rioCompletionMessage = RioRegister(m_completionMessageBuffer.data(), CTS_COMPLETION_MESSAGE_SIZE);
    return CTS_OK;
}

int cts_io_pattern::CreateRecvSlots()
{
    m_recvBufferFreeList.assign(recvCount, nullptr);
    if (recvCount == 0) return CTS_OK;
    if (cfg.use_shared_buffer) {
        std::lock_guard<std::mutex> lk(g_shared.mu);
        if (g_shared.receiver.size() < g_shared.bytes) g_shared.receiver.resize(g_shared.bytes);
        for (auto& b : m_recvBufferFreeList) b = g_shared.receiver.data();
        return CTS_OK;
    }
    ring = Deferred() && VerifiesRecvs();
    slot_bytes = RecvSlotBytes();
    // a slot is handed out again only after every batch that may hold it was verified: the filling batch and the
    // up to Depth() launches in flight hold (Depth() + 1) x BatchCapacity() / (Depth() + 1) = BatchCapacity()
    // unverified slots, and recvCount more are posted. The pipelined ring keeps a second BatchCapacity() of slots
    // beyond that bound (the depth-1 layout of round 3; config-1 throughput did not move with the ring's size
    // within the run-to-run spread)
    ring_slots = ring ? BatchCapacity() * (dev.OnDevice() ? 2u : 1u) + recvCount + 1 : recvCount;
    const uint64_t bytes = (uint64_t)slot_bytes * ring_slots;
    char* base = nullptr;
    if (dev.OnDevice()) {
        const int rc = recv_pinned.alloc(dev.engine, bytes ? bytes : 16);
        if (rc != CTS_OK) return rc;
        base = reinterpret_cast<char*>(recv_pinned.host);
    } else {
        recv_plain.assign(bytes, 0);
        base = recv_plain.data();
    }
    for (uint32_t i = 0; i < recvCount; ++i) m_recvBufferFreeList[i] = base + (size_t)i * slot_bytes;
    ring_base = base;
    ring_bytes = bytes;
    ring_next = recvCount;
    if (ring) pipe.SetRing(ring_base, recv_pinned.dev, ring_bytes);
    return CTS_OK;
}

// the buffer (and its RIO id) to put back on the free lists after a completion
// (ctsIOPattern.cpp:369-386): the completed one, or in ring mode the next ring slot (the
// completed one waits for its batch)
void cts_io_pattern::RecycleRecvBuffer(const cts_task& t)
{
    char* b = t.buffer;
    if (ring) {
        b = ring_base + (size_t)(ring_next % ring_slots) * slot_bytes;
        ++ring_next;
    }
    m_recvBufferFreeList.push_back(b);
    if (Rio()) m_receivingRioBufferIds.push_back(ring ? ring_rio_ids[RingSlot(b)] : t.rio_buffer_id);
}

void cts_io_pattern::CreateSendBuffers()
{
    std::memcpy(m_completionMessageBuffer.data(), kCompletionMessage, CTS_COMPLETION_MESSAGE_SIZE);
    if (Rio()) {
        // g_maxNumberOfRioSendBuffers = c_maxSupportedBytesInFlight / GetMinBufferSize() + 1 (:49, :61)
        const uint64_t n = 0x1000000 / cfg.buffer_size_low + 1;
        m_sendingRioBufferIds.reserve(n);
        for (uint64_t i = 0; i < n; ++i)
            m_sendingRioBufferIds.push_back(RioRegister(g_shared.host, (uint32_t)g_shared.bytes));
    }
}

// When the next send of `size` bytes may go out (ctsIOPattern.cpp:593-674): with a rate limit, the
// bytes of each TcpBytesPerSecondPeriod quantum are capped and a send past the cap is deferred to
// the quantum it fills; otherwise every BurstCount-th send waits BurstDelay ms.
int64_t cts_io_pattern::SendTimeOffset(uint64_t size)
{
    int64_t offset = 0;
    if (m_bytesSendingPerQuantum > 0) {
        const int64_t now = NowMs();
        if (m_bytesSendingThisQuantum < m_bytesSendingPerQuantum) {
            m_bytesSendingThisQuantum += (int64_t)size;
            if (now > m_quantumStartTimeMs + m_quantumPeriodMs) {
                // now past this quantum: move to the one we are in, and take back the bytes the
                // skipped quantums would have carried (never below zero)
                const int64_t skipped = (now - m_quantumStartTimeMs) / m_quantumPeriodMs;
                m_quantumStartTimeMs += skipped * m_quantumPeriodMs;
                const int64_t adjust = m_bytesSendingPerQuantum * skipped;
                m_bytesSendingThisQuantum = adjust > m_bytesSendingThisQuantum ? 0 : m_bytesSendingThisQuantum - adjust;
            }
        } else {
            // this quantum (and maybe more) is already full: carry the excess, defer this send to
            // the end of the quantums it fills
            const int64_t ahead = m_bytesSendingThisQuantum / m_bytesSendingPerQuantum;
            const int64_t skip_ms = (ahead - 1) * m_quantumPeriodMs;
            m_bytesSendingThisQuantum -= m_bytesSendingPerQuantum * ahead;
            m_bytesSendingThisQuantum += (int64_t)size;
            if (now < m_quantumStartTimeMs + m_quantumPeriodMs) offset = m_quantumStartTimeMs + m_quantumPeriodMs - now;
            offset += skip_ms;
            m_quantumStartTimeMs += skip_ms + m_quantumPeriodMs;
        }
    } else if (cfg.burst_count != 0) {
        if (m_burstCount == 0) m_burstCount = cfg.burst_count;
        m_burstCount -= 1;
        if (m_burstCount == 0) offset = (int64_t)cfg.burst_delay;
    }
    return offset;
}

cts_task cts_io_pattern::CreateNewTask(uint8_t action, uint32_t maxTransfer)
{
    const uint64_t remaining = state.GetRemainingTransfer();
    const uint64_t next = GetBufferSize();
    const uint64_t minBuf = std::min<uint64_t>(remaining, next);
    uint64_t newSize = minBuf;
    if (maxTransfer > 0 && maxTransfer < minBuf) newSize = maxTransfer;
    if (newSize > 0xFFFFFFFFull) throw FailFast{"next buffer size is greater than MAXDWORD"};
    const uint32_t size = (uint32_t)newSize;
    cts_task t = EmptyTask();
    // with RIO only so many registered send buffers exist: once every one is in flight, no IO yet
    // (ctsIOPattern.cpp:580-587)
    if (action == CTS_TASK_SEND && Rio() && m_sendingRioBufferIds.empty()) return t;
    if (action == CTS_TASK_SEND) {
        t.time_offset_ms = SendTimeOffset(size);
        t.io_action = CTS_TASK_SEND;
        t.buffer_type = CTS_BUFFER_STATIC;
        t.buffer_length = size;
        t.buffer_offset = m_sendPatternOffset;
        t.expected_pattern_offset = 0;
        t.buffer = g_shared.host;
        // every RIOSend needs its own RIO_BUFFERID (ctsIOPattern.cpp:683-692)
        if (Rio()) {
            if (m_sendingRioBufferIds.empty()) throw FailFast{"m_sendingRioBufferIds is empty for a new Send task"};
            t.buffer_type = CTS_BUFFER_DYNAMIC;
            t.rio_buffer_id = m_sendingRioBufferIds.back();
            m_sendingRioBufferIds.pop_back();
        }
        m_sendPatternOffset += size;
        m_sendPatternOffset %= kPatternSize;
        if ((uint64_t)t.buffer_length + t.buffer_offset > g_shared.bytes)
            throw FailFast{"send task is larger than the shared sender buffer"};
    } else {
        t.io_action = CTS_TASK_RECV;
        t.buffer_type = CTS_BUFFER_DYNAMIC;
        t.buffer_length = size;
        t.buffer_offset = 0;
        t.expected_pattern_offset = m_recvPatternOffset;
        if (m_recvBufferFreeList.empty()) throw FailFast{"m_recvBufferFreeList is empty for a new Recv task"};
        t.buffer = m_recvBufferFreeList.back();
        m_recvBufferFreeList.pop_back();
        if (Rio()) {  // ctsIOPattern.cpp:716-725
            if (m_receivingRioBufferIds.empty()) throw FailFast{"m_receivingRioBufferIds is empty for a new Recv task"};
            t.rio_buffer_id = m_receivingRioBufferIds.back();
            m_receivingRioBufferIds.pop_back();
        }
        if (m_recvPatternOffset >= kPatternSize) throw FailFast{"recv pattern offset too large"};
    }
    return t;
}

cts_task cts_io_pattern::InitiateIo()
{
    cts_task t = EmptyTask();
    switch (state.GetNextPatternType()) {
    case PatternType::MoreIo:
        t = GetNextTaskFromPattern();
        if (t.io_action == CTS_TASK_NONE) t.rio_buffer_id = kRioInvalid;
        break;
    case PatternType::NoIo: break;
    case PatternType::SendConnectionId:
    case PatternType::RecvConnectionId:
        t.io_action = cfg.listening ? CTS_TASK_SEND : CTS_TASK_RECV;
        t.buffer = connection_id;
        t.rio_buffer_id = m_rioConnectionId;
        t.buffer_length = CTS_CONNECTION_ID_LENGTH;
        t.buffer_type = CTS_BUFFER_TCP_CONNECTION_ID;
        break;
    case PatternType::SendCompletion:
    case PatternType::RecvCompletion:
        t.io_action = cfg.listening ? CTS_TASK_SEND : CTS_TASK_RECV;
        t.buffer = m_completionMessageBuffer.data();
        t.rio_buffer_id = m_rioCompletionMessage;
        t.buffer_length = CTS_COMPLETION_MESSAGE_SIZE;
        t.buffer_type = CTS_BUFFER_COMPLETION_MESSAGE;
        break;
    case PatternType::HardShutdown: t.io_action = CTS_TASK_HARD_SHUTDOWN; break;
    case PatternType::GracefulShutdown: t.io_action = CTS_TASK_GRACEFUL_SHUTDOWN; break;
    case PatternType::RequestFin:
        t.io_action = CTS_TASK_RECV;
        t.buffer = m_completionMessageBuffer.data();
        t.rio_buffer_id = m_rioCompletionMessage;
        t.buffer_length = CTS_COMPLETION_MESSAGE_SIZE;
        t.buffer_type = CTS_BUFFER_STATIC;
        break;
    }
    state.NotifyNextTask(t);
    return t;
}

// ---- VerifyBuffer ------------------------------------------------------------------------
void cts_io_pattern::RecordFailure(uint32_t completion, uint32_t transferred, const cts_verify_result& r,
                                   uint64_t recv_after)
{
    ++buffers_failed;
    if (has_failure) return;
    has_failure = true;
    fail_completion = completion;
    fail_length = transferred;
    fail_offset = r.first_mismatch;
    fail_expected = r.expected;
    fail_actual = r.actual;
    bytes_recv_at_failure = recv_after;
}

// One buffer, now (ctsIOPattern.cpp:745-775). Returns CTS_OK and sets *pass.
int cts_io_pattern::VerifyNow(const cts_task& t, uint32_t transferred, cts_verify_result& r)
{
    const char* src = t.buffer + t.buffer_offset;
    if (dev.hook != nullptr) {
        cts_buf_desc d{0, transferred, t.expected_pattern_offset, 0, 0};
        return dev.hook(dev.hook_ctx, reinterpret_cast<const uint8_t*>(src), transferred, &d, 1, &r) == 0 ? CTS_OK
                                                                                                          : CTS_E_INVALID;
    }
    cts_engine* const engine = dev.engine;
    if (engine == nullptr) return CTS_E_INVALID;
    const uint8_t* rp = reinterpret_cast<const uint8_t*>(src);
    if (recv_pinned.host != nullptr && rp >= recv_pinned.host && rp + transferred <= recv_pinned.host + recv_pinned.bytes) {
        // zero copy: the kernel reads the pinned recv buffer in place over PCIe, as up to
        // cts::kSliceMax slices so the reads go out together (latency-bound; cts_slices.hpp)
        int mailbox = 0;
        if (cts_engine_get_attr(engine, CTS_ATTR_SYNC_MAILBOX, &mailbox) == CTS_OK && mailbox)
            return cts_verify_mapped(engine, recv_pinned.dev + (rp - recv_pinned.host), transferred,
                                     t.expected_pattern_offset, &r);
        int rc = dev.EnsureStream();
        if (rc != CTS_OK) return rc;
        constexpr uint32_t kResAt = cts::kSliceMax * sizeof(cts_buf_desc);
        if (one.host == nullptr &&
            (rc = one.alloc(engine, kResAt + cts::kSliceMax * sizeof(cts_verify_result))) != CTS_OK)
            return rc;
        uint32_t slice_len = 0;
        const uint32_t ns = cts::slice_plan((uint64_t)(rp - recv_pinned.host), transferred,
                                            t.expected_pattern_offset, 0, reinterpret_cast<cts_buf_desc*>(one.host),
                                            &slice_len);
        rc = cts_verify(engine, recv_pinned.dev, recv_pinned.bytes, reinterpret_cast<cts_buf_desc*>(one.dev), ns,
                        slice_len, reinterpret_cast<cts_verify_result*>(one.dev + kResAt), nullptr, nullptr, 0,
                        dev.stream);
        if (rc != CTS_OK) return rc;
        EngineDevice on(engine);
        if (hipStreamSynchronize(dev.stream) != hipSuccess) return CTS_E_HIP;
        r = cts::slice_merge(reinterpret_cast<const cts_verify_result*>(one.host + kResAt), ns, slice_len,
                             transferred);
        return CTS_OK;
    }
    return cts_verify_host(engine, src, transferred, t.expected_pattern_offset, &r);
}

// The reference stops at the first failing buffer (its CompleteIo fails the connection on that
// completion, ctsIOPattern.cpp:486-489, and TCP verify allows one posted recv,
// ctsConfig.cpp:3440-3446). Buffers queued after it were never received there: they are neither
// counted as verified nor as received, and the sends that completed after it are dropped too,
// so every counter equals what the reference reports when it stops at that completion.
bool cts_io_pattern::ApplyVerdicts(const std::vector<Queued>& q, const cts_verify_result* res)
{
    const uint32_t n = (uint32_t)q.size();
    uint32_t bad = n;
    for (uint32_t i = 0; i < n; ++i)
        if (!res[i].pass) {
            bad = i;
            break;
        }
    const uint32_t counted = bad < n ? bad + 1 : n;
    for (uint32_t i = 0; i < counted; ++i) {
        ++buffers_verified;
        bytes_verified += q[i].transferred;
    }
    if (n == 0) return false;
    if (bad == n) {
        // every buffer of the batch verified: the bytes up to its last completion are the reference's
        Publish(q[n - 1].status_recv_after, q[n - 1].status_sent_after);
        return false;
    }
    const Queued& f = q[bad];
    RecordFailure(f.completion, f.transferred, res[bad], f.bytes_recv_after);
    // the failing completion's own bytes are counted (the reference adds them after VerifyBuffer failed,
    // ctsIOPattern.cpp:505-516); nothing after it is
    Publish(f.status_recv_after, f.status_sent_after);
    RollbackAfter(f);
    UpdateLastError(CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN);
    return true;
}

// Drop the byte accounting (ctsStatistics, the pattern state and the recv pattern offset) of every
// completion after the failing buffer f (DEFERRED; see ApplyVerdicts). Those bytes were held back, never
// published to TcpStatusDetails, so the process-wide counters are not touched.
void cts_io_pattern::RollbackAfter(const Queued& f)
{
    const uint64_t recv_undo = bytes_recv - f.bytes_recv_after;
    const uint64_t send_undo = bytes_sent - f.bytes_sent_after;
    bytes_recv = f.bytes_recv_after;
    bytes_sent = f.bytes_sent_after;
    status_recv = f.status_recv_after;
    status_sent = f.status_sent_after;
    state.RollbackConfirmed(recv_undo + send_undo);
    m_recvPatternOffset = (uint32_t)(((uint64_t)f.expected + f.transferred) % kPatternSize);
    recv_completions = f.completion + 1;
}

int cts_io_pattern::CompleteIo(const cts_task& t, uint32_t transfer, uint32_t status)
{
    // DEFERRED: anything but a plain in-transfer tracked send/recv sees the
    // queued verdicts first, so a pending data error latches before it.
    bool benign = status == kNoError && (t.io_action == CTS_TASK_SEND || t.io_action == CTS_TASK_RECV) &&
                  state.WouldStayMoreIo(t, transfer) && m_lastError == kStatusIoRunning;
    // A benign one applies the verdicts of an in-flight batch that is seen done, so a data error fails the connection
    // at this completion rather than at the next launch (ctsIOPattern.cpp:486-489 fails it at the failing one; the
    // completions in between are taken back by RollbackAfter).
    if (Deferred() && (benign ? pipe.VerdictsDue() : VerdictsPending())) {
        const int rc = Settle(benign ? pipe.RetireDone() : pipe.Flush());
        // a queued buffer failed: the reference failed the connection at that completion and never
        // saw this one, so it is not accounted (ctsIOPattern.cpp:486-489)
        if (rc != CTS_OK) return rc < 0 ? rc : GetCurrentStatus();
    }
    const bool wasIoRequestedFromPattern = state.IsCurrentStateMoreIo();
    if (t.buffer_type == CTS_BUFFER_DYNAMIC) {  // ctsIOPattern.cpp:369-386
        if (t.io_action == CTS_TASK_RECV) RecycleRecvBuffer(t);
        else if (Rio() && t.io_action == CTS_TASK_SEND) m_sendingRioBufferIds.push_back(t.rio_buffer_id);
    }

    bool verified_now = false, defer_this = false;
    cts_verify_result vr{};
    switch (t.io_action) {
    case CTS_TASK_NONE: break;
    case CTS_TASK_FATAL_ABORT: UpdateLastError(CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED); break;
    case CTS_TASK_ABORT: break;
    case CTS_TASK_GRACEFUL_SHUTDOWN:
    case CTS_TASK_HARD_SHUTDOWN:
    case CTS_TASK_RECV:
    case CTS_TASK_SEND: {
        bool verifyIo = true;
        if (t.buffer_type == CTS_BUFFER_TCP_CONNECTION_ID || t.buffer_type == CTS_BUFFER_COMPLETION_MESSAGE) {
            verifyIo = false;
            if (status != kNoError) {
                UpdateLastError(status);
            } else {
                UpdateLastPatternError(state.CompletedTask(t, transfer));
            }
        } else if (status != kNoError) {
            if (!(t.io_action == CTS_TASK_RECV && state.IsCompleted())) {
                if (UpdateLastError(status) != kStatusIoRunning) verifyIo = false;
            }
        }
        if (verifyIo) {
            const PatternError ps = state.CompletedTask(t, transfer);
            UpdateLastPatternError(ps);
            if (VerifyGate(t) && (ps == PatternError::SuccessfullyCompleted || ps == PatternError::NoError)) {
                if (t.expected_pattern_offset != m_recvPatternOffset)
                    throw FailFast{"task expected_pattern_offset does not match the current pattern offset"};
                if (Deferred()) {
                    defer_this = true;
                } else {
                    const int rc = VerifyNow(t, transfer, vr);
                    if (rc != CTS_OK) return rc;
                    verified_now = true;
                }
                m_recvPatternOffset += transfer;
                m_recvPatternOffset %= kPatternSize;
            }
        }
        break;
    }
    default: throw FailFast{"CompleteIo: unknown task action"};
    }

    if (t.io_action != CTS_TASK_NONE && status == kNoError) {
        // TcpStatusDetails (ctsIOPattern.cpp:505-516): published below, or held back while a verdict is pending
        if (t.io_action == CTS_TASK_SEND) status_sent += transfer;
        else if (t.io_action == CTS_TASK_RECV) status_recv += transfer;
        if (wasIoRequestedFromPattern) UpdateLastPatternError(CompleteTaskBackToPattern(t, transfer));
    }
    if (verified_now) {
        ++buffers_verified;
        bytes_verified += transfer;
        if (!vr.pass) {
            RecordFailure(recv_completions, transfer, vr, bytes_recv);
            UpdateLastError(CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN);
        }
    }
    if (defer_this) {
        const char* src = t.buffer + t.buffer_offset;
        const uint64_t recv_after = bytes_recv;
        int rc = pipe.MustFlushBefore(src, transfer) ? Flush() : CTS_OK;
        if (rc >= 0)
            rc = pipe.Enqueue(src, Queued{recv_completions, transfer, recv_after, bytes_sent, t.expected_pattern_offset,
                                          status_recv, status_sent});
        if (rc >= 0 && (!benign || pipe.Full())) rc = benign ? pipe.Rotate() : pipe.Flush();
        if (Settle(rc) < 0) return rc;
    }
    if (t.io_action == CTS_TASK_RECV && t.track_io) ++recv_completions;
    PublishIfSettled();
    if (state.IsCompleted()) UpdateLastError(kNoError);
    return GetCurrentStatus();
}

// The reference verifies inside CompleteIo *before* CompleteTaskBackToPattern
// adds the bytes to m_statistics; the data-error latch order is identical here
// (UpdateLastError keeps the first error), the verify call merely runs after the
// byte accounting so bytes_recv_at_failure includes the failing completion, as
// ctsIOPattern.cpp:505-521 counts it.

namespace {

// ---- concrete patterns (ctsIOPattern.cpp:796-1031) -------------------------------------------
struct PushOrPull : cts_io_pattern {
    // Push: the client sends, the server receives. Pull: the reverse.
    PushOrPull(const cts_pattern_config& c, uint32_t maxbuf, bool receiving)
        : cts_io_pattern(c, maxbuf, receiving ? c.pre_post_recvs : 0),
          m_ioAction(receiving ? CTS_TASK_RECV : CTS_TASK_SEND),
          m_recvNeeded(receiving ? c.pre_post_recvs : 0)
    {
    }
    uint8_t m_ioAction;
    uint32_t m_recvNeeded;
    uint32_t m_sendBytesInFlight = 0;
    cts_task GetNextTaskFromPattern() override  // :803-822 / :856-875
    {
        if (m_ioAction == CTS_TASK_RECV && m_recvNeeded > 0) {
            --m_recvNeeded;
            return CreateTrackedTask(m_ioAction);
        }
        if (m_ioAction == CTS_TASK_SEND && GetIdealSendBacklog() > m_sendBytesInFlight) {
            const cts_task t = CreateTrackedTask(m_ioAction);
            m_sendBytesInFlight += t.buffer_length;
            return t;
        }
        return cts_task{};
    }
    PatternError CompleteTaskBackToPattern(const cts_task& t, uint32_t bytes) override  // :824-838
    {
        if (t.io_action == CTS_TASK_SEND) {
            bytes_sent += bytes;
            m_sendBytesInFlight -= bytes;
        } else if (t.io_action == CTS_TASK_RECV) {
            bytes_recv += bytes;
            ++m_recvNeeded;
        }
        return PatternError::NoError;
    }
};

struct PushPull : cts_io_pattern {  // :888-966
    PushPull(const cts_pattern_config& c, uint32_t maxbuf)
        : cts_io_pattern(c, maxbuf, 1), m_push(c.push_bytes), m_pull(c.pull_bytes), m_listening(c.listening != 0),
          m_sending(c.listening == 0)
    {
    }
    uint32_t m_push, m_pull, m_intra = 0;
    bool m_listening, m_ioNeeded = true, m_sending;
    uint32_t Segment() const
    {
        return m_listening ? (m_sending ? m_pull : m_push) : (m_sending ? m_push : m_pull);
    }
    cts_task GetNextTaskFromPattern() override
    {
        const uint32_t seg = Segment();
        if (m_intra >= seg) throw FailFast{"invalid PushPull state: intra-segment transfer >= segment size"};
        if (m_ioNeeded) {
            m_ioNeeded = false;
            return CreateTrackedTask(m_sending ? CTS_TASK_SEND : CTS_TASK_RECV, seg - m_intra);
        }
        return cts_task{};
    }
    PatternError CompleteTaskBackToPattern(const cts_task& t, uint32_t bytes) override
    {
        if (t.io_action == CTS_TASK_SEND) bytes_sent += bytes;
        else if (t.io_action == CTS_TASK_RECV) bytes_recv += bytes;
        m_ioNeeded = true;
        m_intra += bytes;
        const uint32_t seg = Segment();
        if (m_intra > seg) throw FailFast{"invalid PushPull state: intra-segment transfer > segment size"};
        if (seg == m_intra) {
            m_sending = !m_sending;
            m_intra = 0;
        }
        return PatternError::NoError;
    }
};

struct Duplex : cts_io_pattern {  // :968-1031
    Duplex(const cts_pattern_config& c, uint32_t maxbuf)
        : cts_io_pattern(c, maxbuf, c.pre_post_recvs), m_recvNeeded(c.pre_post_recvs)
    {
        uint64_t total = GetTotalTransfer();
        if (total % 2 != 0) SetTotalTransfer(++total);
        m_remainingSend = total / 2;
        m_remainingRecv = m_remainingSend;
    }
    uint64_t m_remainingSend = 0, m_remainingRecv = 0;
    uint32_t m_recvNeeded;
    uint32_t m_sendBytesInFlight = 0;
    cts_task GetNextTaskFromPattern() override
    {
        constexpr uint64_t kMaxLong = 0x7FFFFFFF;
        cts_task t{};
        if (m_remainingRecv > 0 && m_recvNeeded > 0) {
            t = CreateTrackedTask(CTS_TASK_RECV, (uint32_t)std::min(m_remainingRecv, kMaxLong));
            m_remainingRecv -= t.buffer_length;
            --m_recvNeeded;
        } else if (m_remainingSend > 0 && GetIdealSendBacklog() > m_sendBytesInFlight) {
            t = CreateTrackedTask(CTS_TASK_SEND, (uint32_t)std::min(m_remainingSend, kMaxLong));
            m_remainingSend -= t.buffer_length;
            m_sendBytesInFlight += t.buffer_length;
        }
        return t;
    }
    PatternError CompleteTaskBackToPattern(const cts_task& t, uint32_t bytes) override
    {
        if (t.io_action == CTS_TASK_SEND) {
            bytes_sent += bytes;
            m_sendBytesInFlight -= bytes;
            m_remainingSend += t.buffer_length;
            m_remainingSend -= bytes;
        } else if (t.io_action == CTS_TASK_RECV) {
            bytes_recv += bytes;
            ++m_recvNeeded;
            m_remainingRecv += t.buffer_length;
            m_remainingRecv -= bytes;
        }
        return PatternError::NoError;
    }
};

void make_connection_id(char* out)  // ctsStatistics::GenerateConnectionId: a UUID string
{
    std::random_device rd;
    std::mt19937_64 g(((uint64_t)rd() << 32) ^ rd());
    uint8_t b[16];
    for (auto& x : b) x = (uint8_t)g();
    b[6] = (uint8_t)((b[6] & 0x0F) | 0x40);
    b[8] = (uint8_t)((b[8] & 0x3F) | 0x80);
    std::snprintf(out, CTS_CONNECTION_ID_LENGTH,
                  "%02x%02x%02x%02x-%02x%02x-%02x%02x-%02x%02x-%02x%02x%02x%02x%02x%02x", b[0], b[1], b[2], b[3],
                  b[4], b[5], b[6], b[7], b[8], b[9], b[10], b[11], b[12], b[13], b[14], b[15]);
}

void latch_fail_fast(cts_io_pattern* p, const std::string& reason)
{
    if (p->fail_fast.empty()) p->fail_fast = reason;
    p->m_lastError = CTS_PATTERN_E_FAIL_FAST;
}

// Runs f for a C-ABI call that holds the pattern lock: nothing may cross the C ABI. A FAIL_FAST, and any other
// exception as "<what> threw: ...", is latched and answered with on_fail_fast; a failed verify call is its status.
template <typename F>
int guarded_call(cts_io_pattern* p, const char* what, int on_fail_fast, F f)
{
    try {
        return f();
    } catch (const FailFast& e) {
        latch_fail_fast(p, e.reason);
    } catch (const DeviceError& d) {
        return d.rc;
    } catch (const std::bad_alloc&) {
        return CTS_E_NOMEM;
    } catch (const std::exception& e) {
        latch_fail_fast(p, std::string(what) + " threw: " + e.what());
    }
    return on_fail_fast;
}

}  // namespace

extern "C" {

int cts_io_pattern_create(const cts_pattern_config* c, cts_engine* engine, cts_io_pattern** out)
{
    if (c == nullptr || out == nullptr) return CTS_E_INVALID;
    *out = nullptr;
    const bool media = c->io_pattern == CTS_PATTERN_MEDIA_STREAM;
    if (c->protocol != (media ? CTS_PROTOCOL_UDP : CTS_PROTOCOL_TCP)) return CTS_E_INVALID;  // UDP is MediaStream only
    if (c->buffer_size_low == 0 || (c->buffer_size_high != 0 && c->buffer_size_high < c->buffer_size_low))
        return CTS_E_INVALID;
    if (c->pre_post_recvs == 0) return CTS_E_INVALID;                         // ctsConfig.cpp:2169-2171
    if (!media && c->verify_buffers && c->pre_post_recvs > 1) return CTS_E_INVALID;  // TCP: ctsConfig.cpp:3440-3446
    if (media) {
        // MediaStreamSettings::CalculateTransferSize and the buffer override (ctsConfig.h:297-364,
        // ctsConfig.cpp:3341-3350): the frame is the buffer, the stream is whole frames
        if (c->buffer_size_high != 0 || c->buffer_size_low < 40 || c->ms_frames_per_second == 0 ||
            c->ms_stream_length_frames <= 0 || c->ms_stream_length_frames > (int64_t)UINT32_MAX ||
            c->transfer_size != (uint64_t)c->buffer_size_low * (uint64_t)c->ms_stream_length_frames)
            return CTS_E_INVALID;
        if (!c->listening && (c->ms_buffered_frames == 0 || c->ms_datagram_max_size == 0)) return CTS_E_INVALID;
        // no RIO and no TCP pacing on the MediaStream path
        if (c->verify_mode > CTS_VERIFY_DEFERRED || c->registered_io || c->tcp_bytes_per_second != 0 || c->burst_count != 0)
            return CTS_E_INVALID;
    }
    if (c->use_shared_buffer && c->verify_buffers) return CTS_E_INVALID;      // ctsIOPattern.cpp:225-227
    if (c->verify_mode != CTS_VERIFY_SYNC && c->verify_mode != CTS_VERIFY_DEFERRED) return CTS_E_INVALID;
    const uint32_t maxbuf = c->buffer_size_high == 0 ? c->buffer_size_low : c->buffer_size_high;  // GetMaxBufferSize
    if (engine != nullptr) {
        const int rc = cts_shared_buffer_init(engine, maxbuf);  // InitOnceExecuteOnce(InitOnceIoPatternCallback)
        if (rc != CTS_OK) return rc;
    }
    if (g_shared.host == nullptr || g_shared.bytes < cts_sender_buffer_size(maxbuf)) return CTS_E_INVALID;
    cts_io_pattern* p = nullptr;
    try {
        switch (c->io_pattern) {
        case CTS_PATTERN_PUSH: p = new PushOrPull(*c, maxbuf, c->listening != 0); break;
        case CTS_PATTERN_PULL: p = new PushOrPull(*c, maxbuf, c->listening == 0); break;
        case CTS_PATTERN_PUSHPULL:
            if (c->push_bytes == 0 || c->pull_bytes == 0) return CTS_E_INVALID;
            p = new PushPull(*c, maxbuf);
            break;
        case CTS_PATTERN_DUPLEX: p = new Duplex(*c, maxbuf); break;
        case CTS_PATTERN_MEDIA_STREAM:
            if (c->listening) {
                p = NewMediaStreamServer(*c, maxbuf);
            } else {
                const int mrc = NewMediaStreamClient(*c, maxbuf, &p);
                if (mrc != CTS_OK) return mrc;
            }
            break;
        default: return CTS_E_INVALID;
        }
    } catch (const std::bad_alloc&) {
        return CTS_E_NOMEM;
    }
    p->dev.engine = engine;
    if (c->listening) make_connection_id(p->connection_id);
    // ctsIoPatternStatistics ctor: CreateRecvBuffers + CreateSendBuffers (ctsIOPattern.h:420-432)
    int rc = CTS_OK;
    try {
        rc = p->CreateRecvBuffers();
        if (rc == CTS_OK) p->CreateSendBuffers();
    } catch (const std::bad_alloc&) {
        rc = CTS_E_NOMEM;
    } catch (const RioRegisterFailed&) {
        rc = CTS_E_INVALID;  // THROW_WIN32_MSG(WSAGetLastError(), "RIORegisterBuffer")
    }
    if (rc != CTS_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return CTS_OK;
}

int cts_io_pattern_destroy(cts_io_pattern* p)
{
    if (p == nullptr) return CTS_E_INVALID;
    // a MediaStream client's timer thread is stopped and joined first (not under the pattern lock, which its
    // callbacks take): nothing calls into the engine from it once destroy has begun, whatever destroy returns
    p->StopTimers();
    int rc = CTS_OK;
    {
        // DEFERRED: completions still waiting for a verdict are verified now, so their bytes reach TcpStatusDetails
        // as the reference's (verified at completion) did. Every wait is bounded (PatternDevice::BoundWaits);
        // nothing may leave the ABI.
        std::lock_guard<std::recursive_mutex> lk(p->mu);
        p->dev.BoundWaits();
        if (p->fail_fast.empty() && p->VerdictsPending()) {
            try {
                const int fr = p->FlushPending();  // an io status (>= 0), or a negative CTS_E_* of the final verify
                if (fr < 0) rc = fr;
            } catch (const DeviceError& d) {
                rc = d.rc < 0 ? d.rc : CTS_E_HIP;
            } catch (...) {
                rc = CTS_E_HIP;
            }
        }
        // the pattern's buffers go with it: a kernel still reading them (it did not finish within the bound) keeps
        // them, and the pattern is left allocated rather than freed under the GPU's reads (CTS_E_TIMEOUT: call
        // destroy again later). Any other failure of that wait is the device's own (a sticky error): no kernel of
        // the pattern runs any more and a later call could not do better, so the pattern is freed (CTS_E_HIP).
        const hipError_t w = p->dev.WaitIdle();
        if (w == hipErrorNotReady) {
            p->dev.UnboundWaits();
            return CTS_E_TIMEOUT;
        }
        if (w != hipSuccess) rc = CTS_E_HIP;
    }
    delete p;
    return rc;
}

int cts_io_pattern_set_verifier(cts_io_pattern* p, cts_batch_verifier fn, void* ctx)
{
    if (p == nullptr) return CTS_E_INVALID;
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    if (p->VerdictsPending()) return CTS_E_INVALID;
    p->dev.hook = fn;
    p->dev.hook_ctx = ctx;
    return CTS_OK;
}

int cts_io_pattern_initiate_io(cts_io_pattern* p, cts_task* out)
{
    if (p == nullptr || out == nullptr) return CTS_E_INVALID;
    *out = EmptyTask();
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    if (!p->fail_fast.empty()) return CTS_OK;
    return guarded_call(p, "InitiateIo", CTS_OK, [&] {
        const cts_task t = p->InitiateIo();  // (a throw leaves *out the empty task)
        *out = t;
        return CTS_OK;
    });
}

int cts_io_pattern_complete_io(cts_io_pattern* p, const cts_task* t, uint32_t current_transfer, uint32_t status)
{
    if (p == nullptr || t == nullptr) return CTS_E_INVALID;
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    if (!p->fail_fast.empty()) return CTS_IO_FAILED;
    if (!p->dev.HasVerifier() && p->NeedsVerifier(*t)) return CTS_E_INVALID;  // the product has no CPU verify path
    return guarded_call(p, "CompleteIo", CTS_IO_FAILED, [&] { return p->CompleteIo(*t, current_transfer, status); });
}

uint32_t cts_io_pattern_last_error(const cts_io_pattern* p)
{
    if (p == nullptr) return CTS_STATUS_IO_RUNNING;
    std::lock_guard<std::recursive_mutex> lk(p->mu);  // a MediaStream client's timer thread may be completing a task
    return p->m_lastError;
}

uint64_t cts_io_pattern_rio_buffer_id_count(const cts_io_pattern* p)
{
    if (p == nullptr) return 0;
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    return p->RioBufferIdCount();
}

int cts_io_pattern_set_ideal_send_backlog(cts_io_pattern* p, uint32_t bytes)
{
    if (p == nullptr) return CTS_E_INVALID;
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    p->state.SetIdealSendBacklog(bytes);
    return CTS_OK;
}

int cts_io_pattern_flush(cts_io_pattern* p)
{
    if (p == nullptr) return CTS_E_INVALID;
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    return guarded_call(p, "Flush", CTS_IO_FAILED, [&] { return p->FlushPending(); });
}

int cts_io_pattern_get_stats(const cts_io_pattern* p, cts_pattern_stats* o)
{
    if (p == nullptr || o == nullptr) return CTS_E_INVALID;
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    *o = cts_pattern_stats{};
    // m_statistics as published: a DEFERRED pattern's bytes behind a pending verdict are reported apart
    o->bytes_sent_held = std::min(p->HeldSent(), p->bytes_sent);
    o->bytes_recv_held = std::min(p->HeldRecv(), p->bytes_recv);
    o->bytes_sent = p->bytes_sent - o->bytes_sent_held;
    o->bytes_recv = p->bytes_recv - o->bytes_recv_held;
    o->buffers_verified = p->buffers_verified;
    o->bytes_verified = p->bytes_verified;
    o->buffers_failed = p->buffers_failed;
    o->bytes_recv_at_failure = p->has_failure ? p->bytes_recv_at_failure : o->bytes_recv;
    o->recv_pattern_offset = p->m_recvPatternOffset;
    o->send_pattern_offset = p->m_sendPatternOffset;
    o->last_error = p->m_lastError;
    o->queued = p->pipe.PendingCount();
    o->fail_length = p->fail_length;
    o->fail_offset = p->fail_offset;
    o->fail_expected = p->fail_expected;
    o->fail_actual = p->fail_actual;
    o->has_failure = p->has_failure ? 1 : 0;
    o->fail_completion = p->fail_completion;
    o->verify_wait_ns = p->dev.verify_wait_ns;
    o->deferred_depth = p->Deferred() && p->dev.OnDevice() ? p->pipe.Depth() : 0u;
    return CTS_OK;
}

int cts_io_pattern_failure_message(const cts_io_pattern* p, char* buf, uint32_t buf_len)
{
    if (p == nullptr) return 0;
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    if (!p->has_failure) return 0;
    // ctsIOPattern.cpp:761-772: the bytes are `char`, so values >= 0x80 print sign-extended
    // through %x (MSVC: 32-bit unsigned). Pointers are not part of the parity contract.
    char tmp[512];
    const int n = std::snprintf(tmp, sizeof(tmp),
                                "ctsIOPattern found data corruption: detected an invalid byte pattern in the returned "
                                "buffer (length %u): mismatch from expected pattern at offset (%u) [expected 32-bit "
                                "value '0x%x' didn't match '0x%x']",
                                p->fail_length, p->fail_offset, (unsigned)(int)(int8_t)p->fail_expected,
                                (unsigned)(int)(int8_t)p->fail_actual);
    if (buf != nullptr && buf_len > 0) {
        const size_t k = std::min<size_t>((size_t)n, buf_len - 1);
        std::memcpy(buf, tmp, k);
        buf[k] = 0;
    }
    return n;
}

const char* cts_io_pattern_fail_fast_reason(const cts_io_pattern* p)
{
    if (p == nullptr) return nullptr;
    std::lock_guard<std::recursive_mutex> lk(p->mu);  // the reason is written once and never changes after
    return p->fail_fast.empty() ? nullptr : p->fail_fast.c_str();
}

const char* cts_io_pattern_connection_id(cts_io_pattern* p) { return p ? p->connection_id : nullptr; }

int cts_io_pattern_register_callback(cts_io_pattern* p, cts_task_callback fn, void* ctx)
{
    if (p == nullptr) return CTS_E_INVALID;
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    p->m_callback = fn;
    p->m_callback_ctx = fn != nullptr ? ctx : nullptr;
    return CTS_OK;
}

int cts_io_pattern_media_stream_fire(cts_io_pattern* p, int timer)
{
    if (p == nullptr) return CTS_E_INVALID;
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    return guarded_call(p, "a timer callback", CTS_OK, [&] { return p->FireTimer(timer); });
}

int cts_io_pattern_media_stream_timers(cts_io_pattern* p, int64_t* start_due_ms, int64_t* render_due_ms)
{
    if (p == nullptr) return CTS_E_INVALID;
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    return p->Timers(start_due_ms, render_due_ms);
}

int cts_io_pattern_media_stream_stats(cts_io_pattern* p, cts_media_stream_stats* out)
{
    if (p == nullptr || out == nullptr) return CTS_E_INVALID;
    std::lock_guard<std::recursive_mutex> lk(p->mu);
    return p->UdpStats(out);
}

}  // extern "C"
