// ms_server_schedule_edges.cpp — the frame schedule's closed form (ctstraffic_amd/csrc/cts_ms_server_schedule_math.hpp,
// the header the host helper and the planning kernels share) on its edge grid, as a stand-alone program for a
// sanitizer build: tests/test_media_stream_servers_timed_ubsan.py compiles it with -fsanitize=undefined,address and
// -fno-sanitize-recover, so any signed overflow, out-of-range shift or division by zero in the header ends the run.
// Every result is also held against the reference's rule taken one frame at a time in 128-bit integers: frame f is
// out at `now` while base + f * 1000 / fps - now < 2 (ctsIOPattern.cpp:1136-1150,
// ctsMediaStreamServerConnectedSocket.cpp:62-74).
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "cts_ms_server_schedule_math.hpp"

namespace {

typedef __int128 wide;

wide due_wide(int64_t base, uint32_t fps, int64_t f) { return (wide)base + (wide)f * 1000 / fps; }

// the iteration, stopped after `limit` frames (the caller keeps the frames that are out few, or max_frames small)
uint32_t frames_by_iteration(int64_t base, uint32_t fps, int64_t current, int64_t final, int64_t now,
                             uint32_t max_frames)
{
    int64_t f = current;
    while (f <= final && (uint64_t)(f - current) < max_frames && due_wide(base, fps, f) - now < 2) ++f;
    return (uint32_t)(f - current);
}

}  // namespace

int main()
{
    const uint32_t kU32 = 0xFFFFFFFFu;
    const uint32_t rates[] = {1, 3, 7, 30, 60, 999, 1000, 1001, kU32};
    const int64_t kTop = ((int64_t)1 << 62) - 1;
    const int64_t bases[] = {0, 5000, kTop - 7000, kTop};
    struct Stream {
        int64_t final;
        std::vector<int64_t> currents;
    };
    const Stream streams[] = {{1, {1}},
                              {100, {1, 2, 50, 99, 100}},
                              {4000, {1, 1000, 3999}},
                              {(int64_t)kU32, {1, 77, (int64_t)kU32 - 3, (int64_t)kU32 - 2, (int64_t)kU32 - 1, kU32}}};
    uint64_t cases = 0, bad = 0;
    bool before = false, all = false, exact = false, inexact = false;
    for (uint32_t fps : rates)
        for (int64_t base : bases)
            for (const Stream& s : streams) {
                std::set<int64_t> nows = {0, base - 1, base, base + 1, kTop};
                std::set<int64_t> frames = {1, 2, 3, 29, 30, 31, 999, 1000, 1001, s.final - 1, s.final};
                frames.insert(s.currents.begin(), s.currents.end());
                for (int64_t f : frames) {
                    if (f < 1 || f > s.final) continue;
                    const wide due = due_wide(base, fps, f);
                    for (int x = -3; x <= 1; ++x)
                        if (due + x <= kTop) nows.insert((int64_t)(due + x));
                }
                const wide edge = (wide)base - 1 + (wide)s.final * 1000 / fps;  // d == final x 1000 / fps here
                for (int x : {-2, -1, 0, 1, 1000})
                    if (edge + x <= kTop) nows.insert((int64_t)(edge + x));
                for (int64_t current : s.currents)
                    for (int64_t now : nows) {
                        if (now < 0 || now > kTop) continue;
                        const wide d = (wide)now + 1 - base;
                        if (d < 0) before = true;
                        else if (d >= (wide)s.final * 1000 / fps) all = true;
                        else if (((d + 1) * fps - 1) % 1000 == 0) exact = true;
                        else inexact = true;
                        const bool far = s.final == (int64_t)kU32 && current < (int64_t)kU32 - 3 && d >= 0;
                        for (uint32_t max_frames : {1u, 2u, kU32}) {
                            if (far && max_frames == kU32) continue;  // the iteration would walk 2^32 frames
                            const uint32_t got = cts::ms_schedule_frames(base, fps, current, s.final, now, max_frames);
                            const uint32_t want = frames_by_iteration(base, fps, current, s.final, now, max_frames);
                            ++cases;
                            if (got != want) {
                                if (bad++ < 10)
                                    std::fprintf(stderr, "base %lld fps %u current %lld final %lld now %lld max %u: %u, "
                                                 "the iteration %u\n", (long long)base, fps, (long long)current,
                                                 (long long)s.final, (long long)now, max_frames, got, want);
                            }
                            const int64_t next = current + got;
                            if ((wide)cts::ms_schedule_due(base, fps, next) != due_wide(base, fps, next)) ++bad;
                        }
                    }
            }
    if (!(before && all && exact && inexact)) {
        std::fprintf(stderr, "the grid missed a branch: before %d all %d exact %d inexact %d\n", before, all, exact,
                     inexact);
        return 2;
    }
    if (bad != 0) return 1;
    std::printf("ms_server_schedule_edges: ok (%llu cases)\n", (unsigned long long)cases);
    return 0;
}
