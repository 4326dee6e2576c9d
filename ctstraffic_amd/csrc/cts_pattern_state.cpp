// cts_pattern_state.cpp — ctsIoPatternState on its own behind the C ABI (cts_io_pattern_state_*,
// include/cts_pattern.h; ctsIOPatternState.hpp:51-504): the MSTest replays drive the state machine through it.
#include <new>

#include "cts_pattern_state.hpp"

using namespace cts;

struct cts_io_pattern_state {
    PatternState st;
    std::string fail_fast;
    explicit cts_io_pattern_state(const cts_pattern_config& c)
        : st(c, c.buffer_size_high ? c.buffer_size_high : c.buffer_size_low)
    {
    }
};

namespace {
// an internal-consistency FAIL_FAST of the reference: latched, reported as CTS_E_INVALID
template <typename F>
int state_call(cts_io_pattern_state* s, F f)
{
    if (s == nullptr) return CTS_E_INVALID;
    if (!s->fail_fast.empty()) return CTS_E_INVALID;
    try {
        return f();
    } catch (const FailFast& e) {
        s->fail_fast = e.reason;
        return CTS_E_INVALID;
    }
}
}  // namespace

extern "C" {

int cts_io_pattern_state_create(const cts_pattern_config* c, cts_io_pattern_state** out)
{
    if (c == nullptr || out == nullptr) return CTS_E_INVALID;
    *out = nullptr;
    if (c->protocol != CTS_PROTOCOL_TCP && c->protocol != CTS_PROTOCOL_UDP) return CTS_E_INVALID;
    cts_io_pattern_state* s = new (std::nothrow) cts_io_pattern_state(*c);
    if (s == nullptr) return CTS_E_NOMEM;
    *out = s;
    return CTS_OK;
}

int cts_io_pattern_state_destroy(cts_io_pattern_state* s)
{
    if (s == nullptr) return CTS_E_INVALID;
    delete s;
    return CTS_OK;
}

uint64_t cts_io_pattern_state_get_remaining_transfer(cts_io_pattern_state* s)
{
    uint64_t v = 0;
    (void)state_call(s, [&] {
        v = s->st.GetRemainingTransfer();
        return CTS_OK;
    });
    return v;
}

uint64_t cts_io_pattern_state_get_max_transfer(const cts_io_pattern_state* s) { return s ? s->st.GetMaxTransfer() : 0; }

int cts_io_pattern_state_set_max_transfer(cts_io_pattern_state* s, uint64_t max_transfer)
{
    return state_call(s, [&] {
        s->st.SetMaxTransfer(max_transfer);
        return CTS_OK;
    });
}

uint32_t cts_io_pattern_state_get_ideal_send_backlog(const cts_io_pattern_state* s)
{
    return s ? s->st.GetIdealSendBacklog() : 0;
}

int cts_io_pattern_state_set_ideal_send_backlog(cts_io_pattern_state* s, uint32_t bytes)
{
    return state_call(s, [&] {
        s->st.SetIdealSendBacklog(bytes);
        return CTS_OK;
    });
}

int cts_io_pattern_state_is_completed(const cts_io_pattern_state* s) { return s ? (s->st.IsCompleted() ? 1 : 0) : CTS_E_INVALID; }

int cts_io_pattern_state_is_current_state_more_io(const cts_io_pattern_state* s)
{
    return s ? (s->st.IsCurrentStateMoreIo() ? 1 : 0) : CTS_E_INVALID;
}

int cts_io_pattern_state_get_next_pattern_type(cts_io_pattern_state* s)
{
    return state_call(s, [&] { return (int)s->st.GetNextPatternType(); });
}

int cts_io_pattern_state_notify_next_task(cts_io_pattern_state* s, const cts_task* t)
{
    if (t == nullptr) return CTS_E_INVALID;
    return state_call(s, [&] {
        s->st.NotifyNextTask(*t);
        return CTS_OK;
    });
}

int cts_io_pattern_state_completed_task(cts_io_pattern_state* s, const cts_task* t, uint32_t completed_bytes)
{
    if (t == nullptr) return CTS_E_INVALID;
    return state_call(s, [&] { return (int)s->st.CompletedTask(*t, completed_bytes); });
}

int cts_io_pattern_state_update_error(cts_io_pattern_state* s, uint32_t error)
{
    return state_call(s, [&] { return (int)s->st.UpdateError(error); });
}

const char* cts_io_pattern_state_fail_fast_reason(const cts_io_pattern_state* s)
{
    return (s == nullptr || s->fail_fast.empty()) ? nullptr : s->fail_fast.c_str();
}

}  // extern "C"
