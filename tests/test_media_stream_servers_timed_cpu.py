"""The MediaStream servers' frame schedule on the device-resident path, host side (cts_media_stream_servers_send_at of
include/cts_media_stream_servers.h): the schedule entry's initialiser, the closed form cts_ms_server_frames_due against
the reference's rule taken one frame at a time in Python integers (workload.media_stream_frames_out), the timed tick's
argument checks, and the model that the GPU tests compare against held against the plain tick's model."""
import ctypes

import numpy as np
import pytest

from ctstraffic_amd import media_stream as ms
from ctstraffic_amd import workload as wl
from ctstraffic_amd._lib import CtsError, lib
from ctstraffic_amd.types import (MS_SERVER_SCHEDULE_DTYPE, MS_SERVER_STATE_DTYPE, MS_SERVER_TICK_DTYPE,
                                  MS_SERVER_TIMED_TICK_DTYPE, MS_SERVER_WAITING)

I64_MAX = (1 << 63) - 1
U32_MAX = 0xFFFFFFFF
FPS = [1, 3, 7, 30, 60, 999, 1000, 1001, U32_MAX]


def test_layouts():
    assert MS_SERVER_SCHEDULE_DTYPE.itemsize == 16 and MS_SERVER_TIMED_TICK_DTYPE.itemsize == 48
    assert MS_SERVER_SCHEDULE_DTYPE.fields["frames_per_second"][1] == 8
    for f in MS_SERVER_TICK_DTYPE.names:  # the first 32 bytes are the plain tick's
        assert MS_SERVER_TIMED_TICK_DTYPE.fields[f] == MS_SERVER_TICK_DTYPE.fields[f]
    assert [MS_SERVER_TIMED_TICK_DTYPE.fields[f][1] for f in ("next_due_ms", "connections_waiting", "frames")] == \
        [32, 40, 44]
    assert MS_SERVER_WAITING == 5


def test_schedule_init():
    for fps, base in [(1, 0), (60, 12345), (U32_MAX, (1 << 62) - 1)]:
        q = ms.server_schedule_init(fps, base)
        assert (int(q["base_time_ms"]), int(q["frames_per_second"]), int(q["reserved"])) == (base, fps, 0)
        assert q == wl.media_stream_server_schedule([(fps, base)])[0]
    for fps, base in [(0, 0), (60, -1), (60, 1 << 62), (60, -(1 << 63)), (60, I64_MAX)]:
        with pytest.raises(CtsError):
            ms.server_schedule_init(fps, base)
        with pytest.raises(ValueError):
            wl.media_stream_server_schedule([(fps, base)])
    s = ms.Settings(3000, 1400, 60, 0, 5)
    out = np.zeros(1, dtype=MS_SERVER_SCHEDULE_DTYPE)
    assert lib().cts_ms_server_schedule_init(None, 0, out.ctypes.data) == -1
    assert lib().cts_ms_server_schedule_init(ctypes.addressof(s), 0, None) == -1
    assert not out.view(np.uint8).any()
    assert lib().cts_ms_server_schedule_init(ctypes.addressof(s), 7, out.ctypes.data) == 0
    assert int(out[0]["base_time_ms"]) == 7 and int(out[0]["frames_per_second"]) == 60


def test_scratch_bytes():
    """The plain scratch, a word per listed connection and the 16 bytes by which the tick block is larger."""
    for n in (0, 1, 256, 257, 65536, U32_MAX):
        assert ms.servers_timed_scratch_bytes(n) == ms.servers_scratch_bytes(n) + 8 * n + 16


def _entry(current, final):
    e = wl.media_stream_server_entries([(3000, 1400, final)])[0]
    e["current_frame"] = current
    return e


def _branch(base, fps, final, now):
    """Which branch of the closed form (now, base, fps, final) takes, worked out here from the definitions."""
    d = now + 1 - base
    if d < 0:
        return "before"
    if d >= final * 1000 // fps:
        return "all"
    return "middle, exact" if ((d + 1) * fps - 1) % 1000 == 0 else "middle, inexact"


def _grid():
    """(base, fps, current, final, now) of the sweep."""
    for fps in FPS:
        for base in (0, 5000, (1 << 62) - 1 - 7000):
            for final, currents in [(1, [1]), (100, [1, 2, 50, 99, 100]), (4000, [1, 1000, 3999]),
                                    (U32_MAX, [1, 77, U32_MAX - 3, U32_MAX - 2, U32_MAX - 1, U32_MAX])]:
                nows = {0, base - 1, base, base + 1}
                for f in {1, 2, 3, 29, 30, 31, 999, 1000, 1001, final - 1, final} | set(currents):
                    if 1 <= f <= final:
                        due = wl.media_stream_frame_due(base, fps, f)
                        nows |= {due + x for x in (-3, -2, -1, 0, 1)}
                # d just below and just above final x 1000 / fps
                edge = base - 1 + final * 1000 // fps
                nows |= {edge - 2, edge - 1, edge, edge + 1, edge + 1000}
                for current in currents:
                    for now in nows:
                        if 0 <= now < (1 << 62):
                            yield base, fps, current, final, now


def test_frames_due_against_the_iteration():
    """cts_ms_server_frames_due over the issue's grid against the reference's rule one frame at a time, with
    max_frames 1, 2 and 2^32 - 1; both sides of "< 2" around several frames, now before the base, a base at the top of
    its range, the last frames of the longest stream, and d on both sides of final x 1000 / fps."""
    seen, sides, cases = set(), set(), 0
    L = lib()
    q = np.zeros(1, dtype=MS_SERVER_SCHEDULE_DTYPE)
    e = np.zeros(1, dtype=MS_SERVER_STATE_DTYPE)
    frames, due = ctypes.c_uint32(0), ctypes.c_int64(0)
    for base, fps, current, final, now in _grid():
        e[0] = _entry(current, final)
        q[0]["base_time_ms"], q[0]["frames_per_second"] = base, fps
        branch = _branch(base, fps, final, now)
        seen.add((fps, branch))
        # the iteration walks the frames that are out: near the end of the longest stream, or few of them
        if final == U32_MAX and current < U32_MAX - 3 and branch != "before":
            maxes = [1, 2]
        else:
            maxes = [1, 2, U32_MAX]
        for max_frames in maxes:
            want = wl.media_stream_frames_out(base, fps, current, final, now, max_frames)
            assert L.cts_ms_server_frames_due(e.ctypes.data, q.ctypes.data, now, max_frames, ctypes.byref(frames),
                                              ctypes.byref(due)) == 0
            where = (base, fps, current, final, now, max_frames)
            assert frames.value == want, where
            nxt = current + want
            assert due.value == (wl.media_stream_frame_due(base, fps, nxt) if nxt <= final else I64_MAX), where
            cases += 1
        d0 = wl.media_stream_frame_due(base, fps, current) - now
        if d0 in (1, 2):
            sides.add(d0)
    # every branch of the closed form, on both sides of each test: before the base and not, the whole stream out and
    # not, and in the middle branch (d + 1) x fps - 1 an exact multiple of 1000 and not
    assert {b for _, b in seen} == {"before", "all", "middle, exact", "middle, inexact"}
    for fps in FPS:
        assert {"before", "all"} <= {b for r, b in seen if r == fps}, fps
        assert any(b.startswith("middle") for r, b in seen if r == fps), fps
    assert sides == {1, 2}  # a frame one millisecond inside the "< 2" rule, and one just outside it
    assert cases > 20000


def test_frames_due_refuses():
    e = np.array([_entry(1, 5)], dtype=MS_SERVER_STATE_DTYPE)
    q = np.array([ms.server_schedule_init(30, 1000)], dtype=MS_SERVER_SCHEDULE_DTYPE)
    L = lib()
    f, d = ctypes.c_uint32(9), ctypes.c_int64(9)

    def call(state=e.ctypes.data, sched=q.ctypes.data, now=1100, max_frames=4, fp=ctypes.byref(f), dp=ctypes.byref(d)):
        return L.cts_ms_server_frames_due(state, sched, now, max_frames, fp, dp)

    assert call(state=None) == -1 and call(sched=None) == -1 and call(max_frames=0) == -1
    assert call(now=-1) == -1 and call(now=1 << 62) == -1
    bad = q.copy()
    bad[0]["frames_per_second"] = 0
    assert call(sched=bad.ctypes.data) == -1
    bad = q.copy()
    bad[0]["base_time_ms"] = -1
    assert call(sched=bad.ctypes.data) == -1
    assert (f.value, d.value) == (9, 9)
    assert call() == 0 and (f.value, d.value) == (3, 1000 + 4000 // 30)  # frames 1..3 are due by 1100 + 1
    assert call(fp=None) == 0 and call(dp=None) == 0
    e[0]["finished"] = 1
    assert call() == 0 and (f.value, d.value) == (0, I64_MAX)
    assert ms.server_frames_due(_entry(5, 5), q[0], 10**6, 1) == (1, I64_MAX)


def test_refused_arguments():
    """Every argument check comes before the engine is used: with a null engine, and with a non-null one that is
    never dereferenced because an argument is refused first."""
    L = lib()
    mem = np.zeros(1 << 16, dtype=np.uint8)
    base = (mem.ctypes.data + 63) & ~63  # a 64-byte aligned address inside host memory: only ever compared
    good = dict(engine=base, arena=base + 4096, arena_bytes=8 * 1488, stride=1488, first_slot=0, capacity=8,
                ids=base + 64, n=2, servers=base + 128, schedule=base + 2048, n_conns=2, max_frames=3, now=7,
                descs=base + 256, lengths=base + 448, codes=base + 512, tick=base + 576, udp=base + 640,
                scratch=base + 1024, scratch_bytes=ms.servers_timed_scratch_bytes(2))

    def send(**over):
        a = dict(good, **over)
        return L.cts_media_stream_servers_send_at(a["engine"], a["arena"], a["arena_bytes"], a["stride"],
                                                  a["first_slot"], a["capacity"], a["ids"], a["n"], a["servers"],
                                                  a["schedule"], a["n_conns"], a["max_frames"], a["now"], 1, 2,
                                                  a["descs"], a["lengths"], a["codes"], a["tick"], a["udp"],
                                                  a["scratch"], a["scratch_bytes"], None)

    assert send(engine=None) == -1
    assert send(engine=None, n=0) == -1            # a null engine is refused before n == 0 is looked at
    assert send(n=0, stride=7, arena=None, schedule=None, now=-5, max_frames=0) == 0  # n == 0 is CTS_OK
    bad = [dict(schedule=None), dict(schedule=good["schedule"] + 4), dict(schedule=good["schedule"] + 1),
           dict(now=-1), dict(now=-(1 << 63)), dict(max_frames=0),
           dict(stride=1480), dict(stride=0), dict(stride=16), dict(stride=(1 << 20) + 16),
           dict(arena=None), dict(arena=good["arena"] + 8),
           dict(first_slot=1), dict(capacity=9), dict(first_slot=9, capacity=0), dict(first_slot=(1 << 64) - 1),
           dict(first_slot=(1 << 64) - 4, capacity=8), dict(arena_bytes=8 * 1488 - 1),
           dict(ids=None), dict(ids=good["ids"] + 2), dict(servers=None), dict(servers=good["servers"] + 4),
           dict(descs=good["descs"] + 4), dict(lengths=good["lengths"] + 2), dict(codes=good["codes"] + 2),
           dict(tick=good["tick"] + 4), dict(udp=good["udp"] + 4), dict(scratch=None),
           dict(scratch=good["scratch"] + 4), dict(scratch_bytes=good["scratch_bytes"] - 1),
           dict(scratch_bytes=ms.servers_scratch_bytes(2)), dict(scratch_bytes=0)]
    for kw in bad:
        assert send(**kw) == -1, kw
    assert not mem.any()


# ---- the model ---------------------------------------------------------------------------------------------------
def _settings(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        M = int(rng.integers(53, 300))
        k = 1 + (c % 9)
        F = int(rng.integers((k - 1) * M + 1, k * M + 1))
        out.append((max(F, 27), M, 1 + int(rng.integers(0, 4))))
    return out


def _same_views(a, b):
    for f in MS_SERVER_STATE_DTYPE.names:
        assert np.array_equal(a.entries[f], b.entries[f]), f
    assert np.array_equal(a.codes, b.codes) and np.array_equal(a.ring, b.ring)
    assert np.array_equal(a.descs, b.descs) and np.array_equal(a.lengths, b.lengths) and a.udp == b.udp
    for f in wl.MS_SERVER_TICK_FIELDS:
        assert a.tick[f] == b.tick[f], f


def test_model_equals_the_plain_model_at_one_frame():
    """max_frames = 1 and a frame of every running connection out: send_at leaves what send leaves, tick after tick,
    with finished connections, ids beyond the table and a capacity that cuts the list."""
    settings = _settings(40, 1)
    stride, capacity, first_slot = 304, 120, 2
    entries = wl.media_stream_server_entries(settings)
    schedule = wl.media_stream_server_schedule([(1 + 7 * c, 100 + c) for c in range(40)])
    ring0 = np.full((first_slot + capacity) * stride, 0xA5, dtype=np.uint8)
    timed = wl.media_stream_server_view(entries, stride, ring0, capacity)
    plain = wl.media_stream_server_view(entries, stride, ring0, capacity)
    rng = np.random.default_rng(2)
    seen = set()
    for tick in range(6):
        ids = [int(x) for x in rng.permutation(40)[:33]] + [40, 1000]
        rng.shuffle(ids)
        qpc, qpf = 0x0102030405060708 + tick, -0x1112131415161718
        timed.send_at(ids, schedule, 10**7, 1, qpc, qpf, first_slot=first_slot)  # every frame long due
        plain.send(ids, qpc, qpf, first_slot=first_slot)
        _same_views(timed, plain)
        assert timed.tick["frames"] == timed.tick["connections_sent"] and timed.tick["connections_waiting"] == 0
        running = [c for c in ids if c < 40 and not timed.entries["finished"][c]]
        assert timed.tick["next_due_ms"] == min(
            [wl.media_stream_frame_due(int(schedule["base_time_ms"][c]), int(schedule["frames_per_second"][c]),
                                       int(timed.entries["current_frame"][c])) for c in running], default=I64_MAX)
        seen |= set(timed.codes.tolist())
    assert seen == {0, 1, 2, 3, 4}


def test_model_by_hand():
    """One connection at 4 frames a second from 1 000 ms, 3 datagrams a frame, 10 frames: due(f) = 1000 + 250 f."""
    entries = wl.media_stream_server_entries([(3000, 1400, 10)])
    schedule = wl.media_stream_server_schedule([(4, 1000)])
    view = wl.media_stream_server_view(entries, 1408, np.zeros(64 * 1408, dtype=np.uint8), 64)

    def tick(now, max_frames, capacity=None):
        codes, t = view.send_at([0], schedule, now, max_frames, 1, 2, capacity=capacity)
        return int(codes[0]), t["frames"], t["datagrams"], t["next_due_ms"], t["connections_waiting"]

    assert tick(0, 8) == (5, 0, 0, 1250, 1)
    assert tick(1248, 8) == (5, 0, 0, 1250, 1)           # 1250 - 1248 = 2: not yet
    assert tick(1249, 8) == (0, 1, 3, 1500, 0)           # 1250 - 1249 = 1 < 2
    assert tick(1249, 8) == (5, 0, 0, 1500, 1)
    assert tick(2249, 2) == (0, 2, 6, 2000, 0)           # frames 2..5 are out, max_frames lets two go
    assert tick(2249, 8, capacity=5) == (0, 1, 3, 2250, 0)  # frames 4, 5 are out, the capacity holds one
    assert tick(2249, 8, capacity=2) == (3, 0, 0, 2250, 0)
    assert view.tick["connections_no_room"] == 1
    assert tick(10**6, 8) == (1, 6, 18, I64_MAX, 0)      # frames 5..10: the stream ends
    assert tick(10**6, 8) == (2, 0, 0, I64_MAX, 0)
    e = view.entries[0]
    assert (int(e["current_frame"]), int(e["bits_sent"]), int(e["datagrams_sent"]), int(e["finished"])) == \
        (11, 8 * 3000 * 10, 30, 1)
    assert view.udp["bits_received"] == 8 * 3000 * 10 and view.udp["datagrams"] == 30
