// cts_pattern_state.hpp — ctsIoPatternState restated (ctsTraffic/ctsIOPatternState.hpp:57-504): which IO a
// connection may ask for next and what a completion does to it. Pure logic, no device call; the ctsIoPattern
// mirror holds one (cts_pattern_impl.hpp) and cts_pattern_state.cpp exports it on its own.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "cts_pattern.h"

namespace cts {

constexpr char kCompletionMessage[CTS_COMPLETION_MESSAGE_SIZE + 1] = "DONE";  // ctsIOPatternState.hpp:24

enum class PatternType { NoIo, SendConnectionId, RecvConnectionId, MoreIo, SendCompletion, RecvCompletion,
                         GracefulShutdown, HardShutdown, RequestFin };
enum class PatternError { NoError, TooManyBytes, TooFewBytes, CorruptedBytes, ErrorIoFailed, SuccessfullyCompleted };

struct FailFast {  // an internal-consistency FAIL_FAST of the reference: latched by the C ABI, never thrown across it
    std::string reason;
};

class PatternState {
public:
    enum class Internal { Initialized, MoreIo, ServerSendConnectionId, ClientRecvConnectionId, ServerSendCompletion,
                          ClientRecvCompletion, CompletedTransfer, ErrorIoFailed, GracefulShutdown, HardShutdown,
                          RequestFin };

    PatternState(const cts_pattern_config& c, uint32_t max_buffer_size)  // ctsIOPatternState.hpp:108-114
        : m_maxTransfer(c.transfer_size),
          m_idealSendBacklog(c.pre_post_sends == 0 ? max_buffer_size : max_buffer_size * c.pre_post_sends),
          m_listening(c.listening != 0),
          m_graceful(c.tcp_shutdown != CTS_SHUTDOWN_HARD),
          m_udp(c.protocol == CTS_PROTOCOL_UDP)
    {
        if (m_udp) m_internal = Internal::MoreIo;
    }

    uint64_t GetRemainingTransfer() const  // ctsIOPatternState.hpp:123-141
    {
        const uint64_t already = m_confirmedBytes + m_inFlightBytes;
        if (already > m_maxTransfer) throw FailFast{"bytes already transferred exceed the total to transfer"};
        return m_maxTransfer - already;
    }
    uint64_t GetMaxTransfer() const { return m_maxTransfer; }
    // DEFERRED: completions accepted after a buffer that later failed verification are taken back
    // (the reference never saw them: it failed the connection at that buffer, ctsIOPattern.cpp:486-489)
    void RollbackConfirmed(uint64_t bytes) { m_confirmedBytes -= std::min(bytes, m_confirmedBytes); }
    void SetMaxTransfer(uint64_t v) { m_maxTransfer = v; }
    uint32_t GetIdealSendBacklog() const { return m_idealSendBacklog; }
    void SetIdealSendBacklog(uint32_t isb) { m_idealSendBacklog = isb; }  // ctsIOPatternState.hpp:155-158
    bool IsCompleted() const { return m_internal == Internal::CompletedTransfer || m_internal == Internal::ErrorIoFailed; }
    bool IsCurrentStateMoreIo() const { return m_internal == Internal::MoreIo; }

    PatternType GetNextPatternType()  // ctsIOPatternState.hpp:177-244
    {
        if (m_pended) return PatternType::NoIo;
        switch (m_internal) {
        case Internal::Initialized:
            m_pended = true;
            if (m_listening) {
                m_internal = Internal::ServerSendConnectionId;
                return PatternType::SendConnectionId;
            }
            m_internal = Internal::ClientRecvConnectionId;
            return PatternType::RecvConnectionId;
        case Internal::ServerSendConnectionId:
        case Internal::ClientRecvConnectionId:
            m_internal = Internal::MoreIo;
            return PatternType::MoreIo;
        case Internal::MoreIo:
            return (m_confirmedBytes + m_inFlightBytes) < m_maxTransfer ? PatternType::MoreIo : PatternType::NoIo;
        case Internal::ServerSendCompletion: m_pended = true; return PatternType::SendCompletion;
        case Internal::ClientRecvCompletion: m_pended = true; return PatternType::RecvCompletion;
        case Internal::GracefulShutdown: m_pended = true; return PatternType::GracefulShutdown;
        case Internal::HardShutdown: m_pended = true; return PatternType::HardShutdown;
        case Internal::RequestFin: m_pended = true; return PatternType::RequestFin;
        case Internal::CompletedTransfer:
        case Internal::ErrorIoFailed: return PatternType::NoIo;
        }
        throw FailFast{"GetNextPatternType called in an invalid state"};
    }

    void NotifyNextTask(const cts_task& t)  // ctsIOPatternState.hpp:246-252
    {
        if (t.track_io) m_inFlightBytes += t.buffer_length;
    }

    PatternError UpdateError(uint32_t error)  // ctsIOPatternState.hpp:254-293
    {
        if (m_internal == Internal::ErrorIoFailed) return PatternError::ErrorIoFailed;
        if (m_udp) {
            if (error != 0) {
                m_internal = Internal::ErrorIoFailed;
                return PatternError::ErrorIoFailed;
            }
            return PatternError::NoError;
        }
        if (error != 0 && !IsCompleted()) {
            // WSAETIMEDOUT / WSAECONNRESET / WSAECONNABORTED while a server waits for the FIN
            if (m_listening && m_internal == Internal::RequestFin && (error == 10060 || error == 10054 || error == 10053))
                return PatternError::NoError;
            m_internal = Internal::ErrorIoFailed;
            return PatternError::ErrorIoFailed;
        }
        return PatternError::NoError;
    }

    // True when CompletedTask(task, bytes) would return NoError and leave the
    // state in MoreIo without side effects beyond the byte accounting — the
    // completions a DEFERRED pattern may verify later (cts_io_pattern_flush).
    bool WouldStayMoreIo(const cts_task& t, uint32_t bytes) const
    {
        if (m_internal != Internal::MoreIo || !t.track_io) return false;
        if (bytes > t.buffer_length || t.buffer_length > m_inFlightBytes) return false;
        const uint64_t inflight = m_inFlightBytes - t.buffer_length;
        const uint64_t already = m_confirmedBytes + bytes + inflight;
        if (already < m_maxTransfer) return bytes != 0;
        if (already == m_maxTransfer) return inflight != 0;
        return false;
    }

    PatternError CompletedTask(const cts_task& t, uint32_t bytes)  // ctsIOPatternState.hpp:295-504
    {
        if (m_internal == Internal::ErrorIoFailed) return PatternError::ErrorIoFailed;
        if (m_internal == Internal::ServerSendConnectionId || m_internal == Internal::ClientRecvConnectionId) {
            if (bytes != CTS_CONNECTION_ID_LENGTH) {
                m_internal = Internal::ErrorIoFailed;
                return PatternError::TooFewBytes;
            }
            m_pended = false;
        }
        if (t.track_io) {
            if (bytes > m_inFlightBytes) throw FailFast{"task returned more bytes than were in flight"};
            if (t.buffer_length > m_inFlightBytes) throw FailFast{"task requested more bytes than were in flight"};
            if (bytes > t.buffer_length) throw FailFast{"task returned more bytes than were posted"};
            m_inFlightBytes -= t.buffer_length;
            m_confirmedBytes += bytes;
        }
        const uint64_t already = m_confirmedBytes + m_inFlightBytes;
        if (m_udp) return already == m_maxTransfer ? PatternError::SuccessfullyCompleted : PatternError::NoError;
        if (already < m_maxTransfer) {
            if (bytes == 0) {
                m_internal = Internal::ErrorIoFailed;
                return PatternError::TooFewBytes;
            }
        } else if (already == m_maxTransfer) {
            if (m_inFlightBytes == 0) {
                if (m_listening) {
                    switch (m_internal) {
                    case Internal::MoreIo:
                        m_internal = Internal::ServerSendCompletion;
                        m_pended = false;
                        break;
                    case Internal::ServerSendCompletion:
                        m_internal = Internal::RequestFin;
                        m_pended = false;
                        break;
                    case Internal::RequestFin:
                        if (bytes != 0) {
                            m_internal = Internal::ErrorIoFailed;
                            return PatternError::TooManyBytes;
                        }
                        m_internal = Internal::CompletedTransfer;
                        return PatternError::SuccessfullyCompleted;
                    default: throw FailFast{"CompletedTask: invalid server state"};
                    }
                } else {
                    switch (m_internal) {
                    case Internal::MoreIo:
                        m_internal = Internal::ClientRecvCompletion;
                        m_pended = false;
                        break;
                    case Internal::ClientRecvCompletion:
                        if (bytes != CTS_COMPLETION_MESSAGE_SIZE ||
                            std::memcmp(t.buffer, kCompletionMessage, CTS_COMPLETION_MESSAGE_SIZE) != 0) {
                            m_internal = Internal::ErrorIoFailed;
                            return PatternError::TooFewBytes;
                        }
                        m_internal = m_graceful ? Internal::GracefulShutdown : Internal::HardShutdown;
                        m_pended = false;
                        break;
                    case Internal::GracefulShutdown:
                        m_internal = Internal::RequestFin;
                        m_pended = false;
                        break;
                    case Internal::RequestFin:
                        if (bytes != 0) {
                            m_internal = Internal::ErrorIoFailed;
                            return PatternError::TooManyBytes;
                        }
                        m_internal = Internal::CompletedTransfer;
                        return PatternError::SuccessfullyCompleted;
                    case Internal::HardShutdown:
                        m_internal = Internal::CompletedTransfer;
                        return PatternError::SuccessfullyCompleted;
                    default: throw FailFast{"CompletedTask: invalid client state"};
                    }
                }
            }
        } else {
            m_internal = Internal::ErrorIoFailed;
            return PatternError::TooManyBytes;
        }
        return PatternError::NoError;
    }

private:
    uint64_t m_confirmedBytes = 0;
    uint64_t m_maxTransfer;
    uint64_t m_inFlightBytes = 0;
    uint32_t m_idealSendBacklog;
    Internal m_internal = Internal::Initialized;
    bool m_pended = false;
    bool m_listening;
    bool m_graceful;
    bool m_udp;
};

}  // namespace cts
