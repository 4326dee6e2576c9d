// cts_ms_server_schedule_math.hpp — the frame schedule of cts_media_stream_servers.h in closed form, written once for
// the host helper (cts_ms_server_frames_due, cts_media_stream_servers.cpp) and the timed tick's planning
// (cts_tick_plan.hip). The reference gives frame f the time offset base + f x 1000 / fps - now
// (ctsIOPattern.cpp:1136-1150) and sends it at once when that is below 2 (ctsMediaStreamServerConnectedSocket.cpp:
// 62-74): here the last frame that rule lets out at `now` comes from two divisions, whatever the distance between the
// connection and the clock. Nothing but <stdint.h>: a stand-alone program can include this file.
#pragma once

#include <stdint.h>

#if defined(__HIP__)
#define CTS_MSS_FN __host__ __device__ __forceinline__
#else
#define CTS_MSS_FN inline
#endif

namespace cts {

// due(f) = base + f x 1000 / fps, the reference's expression. f <= 2^32 (a running entry's current_frame is at most
// final_frame + 1 <= 2^32), so the product stays below 2^42; base < 2^62. fps != 0.
CTS_MSS_FN int64_t ms_schedule_due(int64_t base, uint32_t fps, int64_t frame)
{
    return (int64_t)((uint64_t)base + (uint64_t)frame * 1000u / fps);
}

// The frames current .. last that "due(f) - now < 2" releases, at most max_frames of them; 0 when none is out.
// due(f) - now < 2 is f x 1000 / fps <= d with d = now + 1 - base, which is f x 1000 < (d + 1) x fps, which is
// f <= ((d + 1) x fps - 1) / 1000. The product (d + 1) x fps is only formed when frame `final` is not out yet, d <
// final x 1000 / fps: then (d + 1) x fps <= final x 1000 + fps < 2^43 with final <= 2^32 - 1, and nothing overflows
// whatever now and base are (d itself is taken modulo 2^64, exact for now and base in [0, 2^62)). fps != 0.
CTS_MSS_FN uint32_t ms_schedule_frames(int64_t base, uint32_t fps, int64_t current, int64_t final, int64_t now,
                                       uint32_t max_frames)
{
    const int64_t d = (int64_t)((uint64_t)now + 1u - (uint64_t)base);
    if (d < 0) return 0u;
    int64_t last = final;
    if ((uint64_t)d < (uint64_t)final * 1000u / fps) last = (int64_t)((((uint64_t)d + 1u) * fps - 1u) / 1000u);
    if (last < current) return 0u;
    const uint64_t m = (uint64_t)last - (uint64_t)current + 1u;
    return m < (uint64_t)max_frames ? (uint32_t)m : max_frames;
}

}  // namespace cts

#undef CTS_MSS_FN
