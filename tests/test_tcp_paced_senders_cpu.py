"""Send pacing on the device-resident path, host side (include/cts_tcp_senders.h): the pace entry's initialiser, the
struct layouts, every refused argument of the paced tick (nothing launches, so no device is needed), and the model
that the GPU tests compare against (ctstraffic_amd.workload.tcp_paced_sender_view) held against the ctsIoPattern
mirror's CreateNewTask under a fake clock and against sequences worked out by hand."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from ctstraffic_amd import _pattern_abi as A
from ctstraffic_amd import tcp_senders as T
from ctstraffic_amd import workload as wl
from ctstraffic_amd._lib import CtsError, lib
from ctstraffic_amd.pattern import IoPattern, PatternConfig, clock_set, shared_buffer_attach
from ctstraffic_amd.types import (TCP_SENDER_NO_DUE, TCP_SENDER_PACE_DTYPE, TCP_SENDER_PACED_TICK_DTYPE,
                                  TCP_SENDER_TICK_DTYPE, TCP_SENDER_WAITING)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
_SENDER = oracle.sender_buffer(4 * 65536)
I64_MAX = (1 << 63) - 1


def test_layouts_against_offsetof():
    probe = r"""
#include <stdio.h>
#include <stddef.h>
#include "cts_tcp_senders.h"
#define O(T,f) printf("%s.%s %zu\n", #T, #f, offsetof(T,f))
int main(void){
 printf("sizeof %zu %zu %u\n", sizeof(cts_tcp_sender_pace), sizeof(cts_tcp_sender_paced_tick), CTS_TCP_SENDER_WAITING);
 O(cts_tcp_sender_pace,bytes_per_quantum); O(cts_tcp_sender_pace,bytes_this_quantum);
 O(cts_tcp_sender_pace,quantum_start_ms); O(cts_tcp_sender_pace,due_ms); O(cts_tcp_sender_pace,quantum_period_ms);
 O(cts_tcp_sender_pace,burst_count); O(cts_tcp_sender_pace,burst_left); O(cts_tcp_sender_pace,burst_delay_ms);
 O(cts_tcp_sender_pace,pending); O(cts_tcp_sender_pace,reserved);
 O(cts_tcp_sender_paced_tick,tick); O(cts_tcp_sender_paced_tick,tick.bytes); O(cts_tcp_sender_paced_tick,tick.buffers);
 O(cts_tcp_sender_paced_tick,tick.connections_sent); O(cts_tcp_sender_paced_tick,tick.connections_finished);
 O(cts_tcp_sender_paced_tick,tick.connections_no_room); O(cts_tcp_sender_paced_tick,tick.connections_skipped);
 O(cts_tcp_sender_paced_tick,tick.reserved); O(cts_tcp_sender_paced_tick,next_due_ms);
 O(cts_tcp_sender_paced_tick,connections_waiting); O(cts_tcp_sender_paced_tick,connections_pending);
 return 0; }
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(probe)
        exe = os.path.join(d, "p")
        subprocess.run(["gcc", "-std=c11", "-I", INCLUDE, c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert list(map(int, lines[0].split()[1:])) == [TCP_SENDER_PACE_DTYPE.itemsize,
                                                    TCP_SENDER_PACED_TICK_DTYPE.itemsize,
                                                    TCP_SENDER_WAITING] == [64, 48, 5]
    seen = set()
    for line in lines[1:]:
        name, off = line.split()
        struct, field = name.split(".", 1)
        dtype = TCP_SENDER_PACE_DTYPE if struct == "cts_tcp_sender_pace" else TCP_SENDER_PACED_TICK_DTYPE
        if field == "tick":
            assert int(off) == 0
            continue
        field = field.split(".")[-1]
        assert dtype.fields[field][1] == int(off), name
        seen.add((struct, field))
    assert len(seen) == len(TCP_SENDER_PACE_DTYPE.names) + len(TCP_SENDER_PACED_TICK_DTYPE.names)
    # the block's first 32 bytes are the plain tick's, field for field
    for f in TCP_SENDER_TICK_DTYPE.names:
        assert TCP_SENDER_PACED_TICK_DTYPE.fields[f] == TCP_SENDER_TICK_DTYPE.fields[f]
    assert TCP_SENDER_PACED_TICK_DTYPE.names[-3:] == wl.TCP_SENDER_PACED_TAIL_FIELDS
    assert TCP_SENDER_NO_DUE == wl.TCP_SENDER_NO_DUE == I64_MAX


def test_pace_init():
    cases = [dict(), dict(bytes_per_second=655360, period_ms=100), dict(bytes_per_second=655360),
             dict(bytes_per_second=1, period_ms=1), dict(bytes_per_second=999, period_ms=1, burst_count=4,
                                                         burst_delay_ms=9),
             dict(bytes_per_second=50_000_000, period_ms=250, burst_count=2, burst_delay_ms=3),
             dict(burst_count=0xFFFFFFFF, burst_delay_ms=0xFFFFFFFF), dict(bytes_per_second=1 << 40, period_ms=1000),
             dict(bytes_per_second=I64_MAX // 0xFFFFFFFF, period_ms=0xFFFFFFFF),
             dict(bytes_per_second=I64_MAX // 100)]
    for kw in cases:
        for start in (0, 5000, I64_MAX):
            q = T.pace_init(start_ms=start, **kw)
            m = wl.tcp_sender_pace_entries([kw], start)[0]
            assert q == m, kw
            period = kw.get("period_ms", 0) or 100
            assert int(q["quantum_period_ms"]) == period
            assert int(q["bytes_per_quantum"]) == kw.get("bytes_per_second", 0) * period // 1000
            assert int(q["burst_left"]) == int(q["burst_count"]) == kw.get("burst_count", 0)
            assert (int(q["bytes_this_quantum"]), int(q["due_ms"]), int(q["pending"])) == (0, 0, 0)
            assert int(q["quantum_start_ms"]) == start and not q["reserved"].any()
    # a rate that rounds to 0 bytes per quantum leaves the burst settings in charge
    assert int(T.pace_init(bytes_per_second=999, period_ms=1, burst_count=4)["bytes_per_quantum"]) == 0
    out = np.zeros(1, dtype=TCP_SENDER_PACE_DTYPE)
    L = lib()
    assert L.cts_tcp_sender_pace_init(1, 1, 0, 0, 0, None) == -1
    assert L.cts_tcp_sender_pace_init(1, 1, 0, 0, -1, out.ctypes.data) == -1
    assert L.cts_tcp_sender_pace_init(I64_MAX // 100 + 1, 0, 0, 0, 0, out.ctypes.data) == -1
    assert L.cts_tcp_sender_pace_init(1 << 63, 1, 0, 0, 0, out.ctypes.data) == -1
    assert L.cts_tcp_sender_pace_init(I64_MAX // 0xFFFFFFFF + 1, 0xFFFFFFFF, 0, 0, 0, out.ctypes.data) == -1
    assert not out.view(np.uint8).any()
    assert L.cts_tcp_sender_pace_init(I64_MAX, 1, 0, 0, 0, out.ctypes.data) == 0
    for bad in [dict(start_ms=-1), dict(bytes_per_second=I64_MAX // 100 + 1), dict(bytes_per_second=I64_MAX,
                                                                                   period_ms=2)]:
        with pytest.raises(CtsError):
            T.pace_init(**bad)
        with pytest.raises(ValueError):
            wl.tcp_sender_pace_entries([{k: v for k, v in bad.items() if k != "start_ms"}], bad.get("start_ms", 0))


def test_scratch_bytes():
    for n in (0, 1, 256, 257, 65536, 0xFFFFFFFF):
        assert T.senders_paced_scratch_bytes(n) == T.senders_scratch_bytes(n) + 16


def test_refused_arguments():
    """Every argument check comes before the engine is used: with a null engine, and with a non-null one that is
    never dereferenced because an argument is refused first."""
    L = lib()
    mem = np.zeros(1 << 16, dtype=np.uint8)
    base = (mem.ctypes.data + 63) & ~63  # a 64-byte aligned address inside host memory: only ever compared
    good = dict(engine=base, arena=base + 4096, arena_bytes=8 * 1488, stride=1488, first_slot=0, capacity=8,
                ids=base + 64, n=2, max_buffers=3, senders=base + 128, pace=base + 2048, n_conns=2, now=7,
                descs=base + 256, codes=base + 512, tick=base + 576, sent=base + 640, scratch=base + 1024,
                scratch_bytes=T.senders_paced_scratch_bytes(2))

    def send(**over):
        a = dict(good, **over)
        return L.cts_tcp_senders_send_paced(a["engine"], a["arena"], a["arena_bytes"], a["stride"], a["first_slot"],
                                            a["capacity"], a["ids"], a["n"], a["max_buffers"], a["senders"],
                                            a["pace"], a["n_conns"], a["now"], a["descs"], a["codes"], a["tick"],
                                            a["sent"], a["scratch"], a["scratch_bytes"], None)

    assert send(engine=None) == -1
    assert send(engine=None, n=0) == -1            # a null engine is refused before n == 0 is looked at
    assert send(n=0, stride=7, arena=None, pace=None, now=-5) == 0  # n == 0 is CTS_OK whatever else is passed
    bad = [dict(pace=None), dict(pace=good["pace"] + 4), dict(pace=good["pace"] + 1), dict(now=-1),
           dict(now=-(1 << 63)),
           dict(stride=1480), dict(stride=0), dict(stride=8), dict(stride=(16 << 20) + 16), dict(max_buffers=0),
           dict(arena=None), dict(arena=good["arena"] + 8),
           dict(first_slot=1), dict(capacity=9), dict(first_slot=9, capacity=0), dict(first_slot=(1 << 64) - 1),
           dict(first_slot=(1 << 64) - 4, capacity=8), dict(arena_bytes=8 * 1488 - 1),
           dict(ids=None), dict(ids=good["ids"] + 2), dict(senders=None), dict(senders=good["senders"] + 4),
           dict(descs=None), dict(descs=good["descs"] + 4), dict(codes=good["codes"] + 2),
           dict(tick=good["tick"] + 4), dict(sent=good["sent"] + 4), dict(scratch=None),
           dict(scratch=good["scratch"] + 4), dict(scratch_bytes=good["scratch_bytes"] - 1),
           dict(scratch_bytes=T.senders_scratch_bytes(2)), dict(scratch_bytes=0)]
    for kw in bad:
        assert send(**kw) == -1, kw
    assert not mem.any()


# ---- the model by hand ---------------------------------------------------------------------------------------------
class _One:
    """One connection's paced ticks through the model."""

    def __init__(self, pace, start, B, transfer=1 << 40, capacity=8):
        self.e = wl.tcp_sender_entries([(transfer, B)])
        self.q = wl.tcp_sender_pace_entries([pace], start)
        self.stride = B + (-B) % 16
        self.capacity = capacity
        self.arena = np.zeros(capacity * self.stride, dtype=np.uint8)

    def tick(self, now, max_buffers, capacity=None):
        v = wl.tcp_paced_sender_view(self.e, self.q, now, self.stride, self.arena, 0,
                                     self.capacity if capacity is None else capacity, [0], max_buffers)
        self.e, self.q = v.entries, v.pace
        return v

    def run(self, times, max_buffers):
        counts, dues = [], []
        for now in times:
            v = self.tick(now, max_buffers)
            counts.append(int(v.taken[0]))
            dues.append(int(self.q["due_ms"][0]))
            assert v.codes[0] == (0 if v.taken[0] else 5) and v.tick["buffers"] == int(v.taken[0])
            assert v.tail["connections_waiting"] == (0 if v.taken[0] else 1)
            pending = int(self.q["pending"][0])
            assert v.tail["connections_pending"] == pending
            assert v.tail["next_due_ms"] == (dues[-1] if pending else I64_MAX)
        return counts, dues


def test_one_buffer_per_quantum_by_hand():
    """655 360 B/s in 100 ms quanta = one 64 KiB buffer per quantum, first quantum at 5 000."""
    one = _One(dict(bytes_per_second=655360, period_ms=100), 5000, 65536)
    counts, dues = one.run([5000, 5000, 5050, 5100, 5100, 5350, 5350, 5400], 8)
    assert counts == [1, 0, 0, 1, 0, 2, 0, 1]
    assert dues == [5100, 5100, 5100, 5200, 5200, 5400, 5400, 5500]
    assert int(one.e["bytes_sent"][0]) == 5 * 65536 and int(one.e["buffers_sent"][0]) == 5


def test_burst_by_hand():
    """-BurstCount 3 -BurstDelay 50: every third task waits 50 ms, and nothing is asked for while it waits."""
    one = _One(dict(burst_count=3, burst_delay_ms=50), 0, 1000)
    counts, dues = one.run([0, 10, 50, 50, 100, 1000], 8)
    assert counts == [2, 0, 3, 0, 3, 3]
    assert dues == [50, 50, 100, 100, 150, 1050]


def test_fractional_quantum_by_hand():
    """2 500 B per 10 ms quantum in buffers of 1 000: the carried bytes make the quanta take 3 and 2 in turn."""
    one = _One(dict(bytes_per_second=250_000, period_ms=10), 0, 1000)
    counts, _ = one.run(range(0, 101, 5), 3)
    assert counts == [3, 0, 2, 0] * 5 + [3] and sum(counts) == 28


def test_rate_rounding_to_zero_falls_through_to_the_burst():
    one = _One(dict(bytes_per_second=999, period_ms=1, burst_count=2, burst_delay_ms=7), 0, 1000)
    assert int(one.q["bytes_per_quantum"][0]) == 0
    counts, dues = one.run([0, 6, 7, 7, 14], 8)
    assert counts == [1, 0, 2, 0, 2] and dues == [7, 7, 14, 14, 21]


def test_rate_limit_takes_precedence_over_the_burst():
    one = _One(dict(bytes_per_second=10 ** 9, burst_count=1, burst_delay_ms=7), 0, 1000)
    counts, _ = one.run([0, 0, 0], 8)
    assert counts == [8, 8, 8] and int(one.q["burst_left"][0]) == 1 and int(one.q["pending"][0]) == 0
    only_burst = _One(dict(burst_count=1, burst_delay_ms=7), 0, 1000)
    assert only_burst.run([0, 0, 7], 8)[0] == [0, 0, 1]


def test_unpaced_entries_give_the_plain_tick():
    settings = [(10 * 1000 + c, 1000) for c in range(9)] + [(5, 2000)]
    e = wl.tcp_sender_entries(settings)
    q = wl.tcp_sender_pace_entries([{}] * len(settings), 3)
    arena = np.full(12 * 1008, 0xA5, dtype=np.uint8)
    ids = [3, 9, 1, 77, 0, 8]
    for now in (3, 3, 1000):
        plain = wl.tcp_sender_view(e, 1008, arena, 1, 10, ids, 4)
        paced = wl.tcp_paced_sender_view(e, q, now, 1008, arena, 1, 10, ids, 4)
        for f in ("arena", "descs", "codes", "entries", "prefix", "taken"):
            assert np.array_equal(getattr(plain, f), getattr(paced, f)), f
        assert plain.tick == paced.tick and plain.counters == paced.counters
        assert np.array_equal(paced.pace, q) and (paced.wanted >= paced.taken).all()
        assert paced.tick["buffers"] == min(10, int(paced.wanted.sum()))
        assert paced.tail == {"next_due_ms": I64_MAX, "connections_waiting": 0, "connections_pending": 0}
        e = paced.entries


def test_capacity_cut_moves_the_pace_entry_by_the_taken_steps():
    """Burst of 4: a connection cut to 2 of its 3 by the capacity moves two steps, and creates no pending task; one
    with no room keeps both entries; at capacity 0 a waiting connection is still code 5."""
    pace = [dict(burst_count=4, burst_delay_ms=9)] * 3 + [dict(burst_count=1, burst_delay_ms=9)]
    e = wl.tcp_sender_entries([(100_000, 1000)] * 4)
    q = wl.tcp_sender_pace_entries(pace, 0)
    arena = np.zeros(8 * 1008, dtype=np.uint8)
    v = wl.tcp_paced_sender_view(e, q, 0, 1008, arena, 0, 5, [0, 1, 2, 3], 8)
    assert v.wanted.tolist() == [3, 3, 3, 0] and v.taken.tolist() == [3, 2, 0, 0] and v.codes.tolist() == [0, 0, 3, 5]
    assert v.pace["burst_left"].tolist() == [0, 2, 4, 0] and v.pace["pending"].tolist() == [1, 0, 0, 1]
    assert v.pace["due_ms"].tolist() == [9, 0, 0, 9] and np.array_equal(v.pace[2], q[2])
    assert np.array_equal(v.entries[2], e[2]) and np.array_equal(v.entries[3], e[3])
    assert v.tail == {"next_due_ms": 9, "connections_waiting": 1, "connections_pending": 2}
    assert v.tick["connections_no_room"] == 1 and v.tick["buffers"] == 5
    v0 = wl.tcp_paced_sender_view(v.entries, v.pace, 5, 1008, arena, 0, 0, [0, 1, 2, 3], 8)
    assert v0.codes.tolist() == [5, 3, 3, 5] and v0.tick["buffers"] == 0
    assert np.array_equal(v0.pace, v.pace) and np.array_equal(v0.entries, v.entries)


def test_last_buffer_and_no_task_past_the_transfer():
    """The transfer's end stops run(): no task, so no pending send, is created past the last byte."""
    one = _One(dict(burst_count=2, burst_delay_ms=5), 0, 1000, transfer=3500)
    v = one.tick(0, 8)
    assert v.taken.tolist() == [1] and int(one.q["pending"][0]) == 1
    v = one.tick(5, 8)
    assert v.taken.tolist() == [2]
    v = one.tick(10, 8)
    assert v.taken.tolist() == [1] and v.codes.tolist() == [1] and v.descs["length"][0] == 500
    assert int(one.q["pending"][0]) == 0 and int(one.q["burst_left"][0]) == 0
    assert one.tick(15, 8).codes.tolist() == [2]


# ---- the model against the ctsIoPattern mirror -------------------------------------------------------------------
class _Clock:
    def __init__(self, t):
        self.t = t

    def __call__(self):
        return self.t


def _mirror(clock, **kw):
    """A Push client of the mirror (it sends), past its connection id."""
    shared_buffer_attach(_SENDER)
    cfg = dict(io_pattern=A.PATTERN_PUSH, listening=False, verify_buffers=True, pre_post_recvs=1,
               pre_post_sends=64)
    cfg.update(kw)
    p = IoPattern.MakeIoPattern(PatternConfig(**cfg), None)
    t = p.InitiateIo()
    assert t.io_action == A.TASK_RECV and t.time_offset_ms == 0
    assert p.CompleteIo(t, A.CONNECTION_ID_LENGTH, 0) == A.IO_CONTINUE
    return p


def _against_the_mirror(pace, B, transfer, start, steps, max_buffers):
    """Tick by tick: the mirror is asked for tasks until one comes back with a time offset or `limit` have gone out;
    the task with the offset is held until the clock reaches it and goes out first. Per tick the count, every
    length and pattern offset, and the due time are the model's."""
    clock = _Clock(start)
    clock_set(clock)
    try:
        p = _mirror(clock, buffer_size=B, transfer_size=transfer,
                    tcp_bytes_per_second=pace.get("bytes_per_second", 0),
                    tcp_bytes_per_second_period=pace.get("period_ms", 0),
                    burst_count=pace.get("burst_count", 0), burst_delay=pace.get("burst_delay_ms", 0))
        one = _One(pace, start, B, transfer=transfer, capacity=max_buffers)
        held, held_due, sent, counts = None, None, 0, []
        for step in steps:
            clock.t += step
            limit = min(max_buffers, -(-(transfer - sent) // B))
            got = []
            while len(got) < limit:
                if held is not None:
                    if clock.t < held_due:
                        break
                    task, held = held, None
                else:
                    task = p.InitiateIo()
                    assert task.io_action == A.TASK_SEND
                    if task.time_offset_ms > 0:
                        held, held_due = task, clock.t + task.time_offset_ms
                        break
                got.append((task.buffer_length, task.buffer_offset))
                sent += task.buffer_length
                status = p.CompleteIo(task, task.buffer_length, 0)
                assert status == A.IO_CONTINUE or sent == transfer
            v = one.tick(clock.t, max_buffers)
            n = v.tick["buffers"]
            where = (pace, B, clock.t, len(counts))
            assert n == len(got) == int(v.taken[0]), where
            assert [(int(d["length"]), int(d["expected_pattern_offset"])) for d in v.descs[:n]] == got, where
            assert int(one.q["pending"][0]) == (held is not None), where
            if held is not None:
                assert int(one.q["due_ms"][0]) == held_due == v.tail["next_due_ms"], where
            else:
                assert v.tail["next_due_ms"] == I64_MAX
            assert int(one.e["bytes_sent"][0]) == sent
            counts.append(n)
        p.close()
        return counts
    finally:
        clock_set(None)


@pytest.mark.parametrize("max_buffers", [1, 3, 8])
@pytest.mark.parametrize("seed", range(6))
def test_model_against_the_pattern_mirror_random(seed, max_buffers):
    rng = np.random.default_rng(seed)
    bps = int(rng.choice([1, 100_000, 655_360, 3_000_000, 50_000_000]))
    period = int(rng.choice([1, 10, 100, 250]))
    B = int(rng.integers(1000, 30000))
    start = int(rng.integers(0, 10 ** 6))
    # the clock stands, moves inside a quantum, by one quantum, by several and one
    steps = [int(rng.choice([0, 0, 1, period // 2, period, 3 * period + 1, 17])) for _ in range(320)]
    counts = _against_the_mirror(dict(bytes_per_second=bps, period_ms=period), B, 1 << 40, start, steps, max_buffers)
    assert len(counts) == 320


@pytest.mark.parametrize("pace,B,transfer,max_buffers", [
    (dict(burst_count=3, burst_delay_ms=50), 1000, 40_500, 8),
    (dict(burst_count=1, burst_delay_ms=4), 33, 33 * 40 + 1, 3),
    (dict(burst_count=5, burst_delay_ms=20), 9000, 9000 * 90, 3),
    (dict(bytes_per_second=999, period_ms=1, burst_count=2, burst_delay_ms=7), 1000, 50_000, 8),
    (dict(bytes_per_second=10 ** 9, burst_count=1, burst_delay_ms=7), 1000, 300_000, 8),
    (dict(bytes_per_second=655_360, period_ms=100), 65536, 65536 * 40 + 5, 3),
    (dict(bytes_per_second=250_000, period_ms=10), 1000, 1 << 30, 3),
    ({}, 1472, 1472 * 100, 8),
])
def test_model_against_the_pattern_mirror_settings(pace, B, transfer, max_buffers):
    """Burst settings, a rate that rounds to nothing, a rate over a burst, no pacing, and transfers that end inside
    the run (the last, short buffer; no task past the end)."""
    rng = np.random.default_rng(B)
    steps = [int(x) for x in rng.choice([0, 1, 3, 10, 25, 50, 120], 300)]
    counts = _against_the_mirror(pace, B, transfer, 1234, steps, max_buffers)
    assert sum(counts) > 0
