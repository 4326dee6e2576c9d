// cts_pattern_process.cpp — what every ctsIoPattern mirror of the process shares (cts_pattern_impl.hpp), with its C
// ABI: the sender's shared buffer (cts_shared_buffer_*), the RIO functions, the pattern clock and TcpStatusDetails.
#include <chrono>

#include "cts_pattern_impl.hpp"

namespace cts {

SharedBuffer g_shared;
RioFunctions g_rio;
std::atomic<uint64_t> g_bytesSent{0}, g_bytesRecv{0}, g_dataErrors{0};

namespace {
struct Clock {
    std::mutex mu;
    cts_clock_ms_fn fn = nullptr;
    void* ctx = nullptr;
};
Clock g_clock;

// The shared sender buffer becomes [host, host + bytes), pinned by `engine` or (nullptr) the caller's own; an owned one
// it replaces is freed. Under g_shared.mu.
void set_shared(void* host, uint64_t bytes, cts_engine* engine)
{
    if (g_shared.owned && g_shared.host) (void)cts_host_free(g_shared.engine, g_shared.host);
    g_shared.host = static_cast<char*>(host);
    g_shared.bytes = bytes;
    g_shared.owned = engine != nullptr;
    g_shared.engine = engine;
}
}  // namespace

int64_t NowMs()
{
    {
        std::lock_guard<std::mutex> lk(g_clock.mu);
        if (g_clock.fn != nullptr) return g_clock.fn(g_clock.ctx);
    }
    return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

}  // namespace cts

using namespace cts;

extern "C" {

int cts_shared_buffer_init(cts_engine* engine, uint32_t max_buffer_size)
{
    if (engine == nullptr) return CTS_E_INVALID;
    std::lock_guard<std::mutex> lk(g_shared.mu);
    const uint64_t need = cts_sender_buffer_size(max_buffer_size);
    if (g_shared.host != nullptr && g_shared.owned && g_shared.bytes >= need) return CTS_OK;
    void *h = nullptr, *d = nullptr;
    int rc = cts_host_alloc(engine, need, &h, &d);
    if (rc != CTS_OK) return rc;
    // the fill kernel writes the pinned sender buffer through its device view
    void* s = nullptr;
    if ((rc = cts_engine_stream_create(engine, &s)) != CTS_OK) {
        (void)cts_host_free(engine, h);
        return rc;
    }
    rc = cts_sender_buffer_fill(engine, d, max_buffer_size, s);
    if (rc == CTS_OK) {
        EngineDevice on(engine);
        if (hipStreamSynchronize(static_cast<hipStream_t>(s)) != hipSuccess) rc = CTS_E_HIP;
    }
    (void)cts_engine_stream_destroy(engine, s);
    if (rc != CTS_OK) {
        (void)cts_host_free(engine, h);
        return rc;
    }
    set_shared(h, need, engine);
    return CTS_OK;
}

int cts_shared_buffer_attach(const void* host, uint64_t bytes)
{
    if (host == nullptr || bytes < CTS_PATTERN_PERIOD) return CTS_E_INVALID;
    std::lock_guard<std::mutex> lk(g_shared.mu);
    set_shared(const_cast<void*>(host), bytes, nullptr);
    return CTS_OK;
}

char* cts_shared_buffer(void) { return g_shared.host; }
uint64_t cts_shared_buffer_bytes(void) { return g_shared.bytes; }

void cts_shared_buffer_release(void)
{
    std::lock_guard<std::mutex> lk(g_shared.mu);
    set_shared(nullptr, 0, nullptr);
}

int cts_pattern_clock_set(cts_clock_ms_fn fn, void* ctx)
{
    std::lock_guard<std::mutex> lk(g_clock.mu);
    g_clock.fn = fn;
    g_clock.ctx = fn != nullptr ? ctx : nullptr;
    return CTS_OK;
}

int cts_rio_functions_set(cts_rio_register_buffer_fn register_fn, cts_rio_deregister_buffer_fn deregister_fn,
                          void* ctx)
{
    if ((register_fn == nullptr) != (deregister_fn == nullptr)) return CTS_E_INVALID;
    std::lock_guard<std::mutex> lk(g_rio.mu);
    g_rio.reg = register_fn;
    g_rio.dereg = deregister_fn;
    g_rio.ctx = ctx;
    return CTS_OK;
}

int cts_status_details_read(cts_status_details* o)
{
    if (o == nullptr) return CTS_E_INVALID;
    o->bytes_sent = g_bytesSent.load();
    o->bytes_recv = g_bytesRecv.load();
    o->data_errors = g_dataErrors.load();
    return CTS_OK;
}

void cts_status_details_reset(void)
{
    g_bytesSent = 0;
    g_bytesRecv = 0;
    g_dataErrors = 0;
}

}  // extern "C"
