"""Send pacing for Pull, PushPull and Duplex on the device-resident path, host side (cts_tcp_exchange_send_paced of
include/cts_tcp_exchange.h): the struct layout, the scratch size, every refused argument (nothing launches, so no
device is needed), and the model that the GPU tests compare against (ctstraffic_amd.workload.tcp_paced_exchange_view)
held against sequences worked out by hand, against the two models it joins (tcp_exchange_view and
tcp_paced_sender_view), and against a client and a server ctsIoPattern mirror on one injected clock."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from ctstraffic_amd import _pattern_abi as A
from ctstraffic_amd import tcp_exchange as X
from ctstraffic_amd import workload as wl
from ctstraffic_amd._lib import lib
from ctstraffic_amd.pattern import IoPattern, PatternConfig, clock_set, shared_buffer_attach
from ctstraffic_amd.types import (DESC_DTYPE, TCP_EXCHANGE_DUPLEX, TCP_EXCHANGE_PACED_TICK_DTYPE, TCP_EXCHANGE_PULL,
                                  TCP_EXCHANGE_PUSH, TCP_EXCHANGE_PUSHPULL, TCP_EXCHANGE_TICK_DTYPE,
                                  TCP_SENDER_PACE_DTYPE, TCP_SENDER_PACED_TICK_DTYPE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
_SENDER = oracle.sender_buffer(4 * 65536)
PUSH, PULL, PUSHPULL, DUPLEX = TCP_EXCHANGE_PUSH, TCP_EXCHANGE_PULL, TCP_EXCHANGE_PUSHPULL, TCP_EXCHANGE_DUPLEX
I64_MAX = (1 << 63) - 1
NO_TAIL = {"next_due_ms": I64_MAX, "connections_waiting": 0, "connections_pending": 0}


def test_layout_against_offsetof():
    probe = r"""
#include <stdio.h>
#include <stddef.h>
#include "cts_tcp_exchange.h"
#define O(T,f) printf("%s %zu\n", #f, offsetof(T,f))
int main(void){
 printf("sizeof %zu %zu\n", sizeof(cts_tcp_exchange_paced_tick), _Alignof(cts_tcp_exchange_paced_tick));
 O(cts_tcp_exchange_paced_tick,tick); O(cts_tcp_exchange_paced_tick,tick.tick.bytes);
 O(cts_tcp_exchange_paced_tick,tick.tick.buffers); O(cts_tcp_exchange_paced_tick,tick.tick.connections_sent);
 O(cts_tcp_exchange_paced_tick,tick.tick.connections_finished);
 O(cts_tcp_exchange_paced_tick,tick.tick.connections_no_room);
 O(cts_tcp_exchange_paced_tick,tick.tick.connections_skipped); O(cts_tcp_exchange_paced_tick,tick.tick.reserved);
 O(cts_tcp_exchange_paced_tick,tick.bytes_dir); O(cts_tcp_exchange_paced_tick,next_due_ms);
 O(cts_tcp_exchange_paced_tick,connections_waiting); O(cts_tcp_exchange_paced_tick,connections_pending);
 return 0; }
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(probe)
        exe = os.path.join(d, "p")
        subprocess.run(["gcc", "-std=c11", "-I", INCLUDE, c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert list(map(int, lines[0].split()[1:])) == [TCP_EXCHANGE_PACED_TICK_DTYPE.itemsize, 8] == [64, 8]
    seen = set()
    for line in lines[1:]:
        name, off = line.split()
        if name == "tick":
            assert int(off) == 0
            continue
        field = name.split(".")[-1]
        assert TCP_EXCHANGE_PACED_TICK_DTYPE.fields[field][1] == int(off), name
        seen.add(field)
    assert seen == set(TCP_EXCHANGE_PACED_TICK_DTYPE.names)
    # the block's first 48 bytes are the exchange tick's, its tail is the paced senders' tick's tail
    for f in TCP_EXCHANGE_TICK_DTYPE.names:
        assert TCP_EXCHANGE_PACED_TICK_DTYPE.fields[f] == TCP_EXCHANGE_TICK_DTYPE.fields[f]
    for f in wl.TCP_SENDER_PACED_TAIL_FIELDS:
        assert TCP_EXCHANGE_PACED_TICK_DTYPE.fields[f][0] == TCP_SENDER_PACED_TICK_DTYPE.fields[f][0]
        assert TCP_EXCHANGE_PACED_TICK_DTYPE.fields[f][1] == TCP_SENDER_PACED_TICK_DTYPE.fields[f][1] + 16
    assert TCP_EXCHANGE_PACED_TICK_DTYPE.names[-3:] == wl.TCP_SENDER_PACED_TAIL_FIELDS


def test_scratch_bytes_grow_with_n():
    ns = (0, 1, 256, 257, 65536, 0xFFFFFFFF)
    b = [X.exchange_paced_scratch_bytes(n) for n in ns]
    assert all(x % 8 == 0 for x in b) and b == sorted(b) and len(set(b)) == len(b)
    for n, x in zip(ns, b):
        assert x == X.exchange_scratch_bytes(n) + 16  # the plain tick's, with the larger tick block


def test_refused_arguments():
    """Every argument check comes before the engine is used: with a null engine, and with a non-null one that is
    never dereferenced because an argument is refused first. The canary memory all the pointers lie in stays zero."""
    L = lib()
    mem = np.zeros(1 << 16, dtype=np.uint8)
    base = (mem.ctypes.data + 63) & ~63  # a 64-byte aligned address inside host memory: only ever compared
    good = dict(engine=base, arena=base + 4096, arena_bytes=8 * 1488, stride=1488, first_slot=0, capacity=8,
                ids=base + 64, n=2, max_buffers=3, entries=base + 128, pace=base + 2048, n_conns=2, now=7,
                descs=base + 256, codes=base + 512, tick=base + 576, sent=base + 640, scratch=base + 1024,
                scratch_bytes=X.exchange_paced_scratch_bytes(2))

    def send(**over):
        a = dict(good, **over)
        return L.cts_tcp_exchange_send_paced(a["engine"], a["arena"], a["arena_bytes"], a["stride"], a["first_slot"],
                                             a["capacity"], a["ids"], a["n"], a["max_buffers"], a["entries"],
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
           dict(ids=None), dict(ids=good["ids"] + 2), dict(entries=None), dict(entries=good["entries"] + 4),
           dict(descs=None), dict(descs=good["descs"] + 4), dict(codes=good["codes"] + 2),
           dict(tick=good["tick"] + 4), dict(sent=good["sent"] + 4), dict(scratch=None),
           dict(scratch=good["scratch"] + 4), dict(scratch_bytes=good["scratch_bytes"] - 1), dict(scratch_bytes=0),
           dict(scratch_bytes=X.exchange_scratch_bytes(2)),  # the plain tick's scratch is 16 bytes too small
           dict(n_conns=(1 << 31) + 1), dict(n_conns=0xFFFFFFFF)]
    for kw in bad:
        assert send(**kw) == -1, kw
    assert not mem.any()


def test_cursor_against_the_closed_form():
    """ExchangeCursor (cts_tcp_exchange_math.hpp), which the kernels' walk advances by additions, against
    exchange_element, the closed form with its division, from random positions of random shapes of the four patterns:
    every direction, every length, and every flip it reports. A stand-alone host program."""
    probe = r"""
#include <cstdio>
#include <cstdlib>
#include "cts_tcp_exchange_math.hpp"
using namespace cts;
int main() {
    unsigned bad = 0;
    long checked = 0;
    srand(7);
    for (int it = 0; it < 60000; ++it) {
        ExchangeShape s{};
        s.pattern = rand() % 4; s.B = 1 + rand() % 50; s.T = 1 + rand() % 2000; s.P = 1 + rand() % 120;
        s.Q = 1 + rand() % 120;
        if (s.pattern == CTS_TCP_EXCHANGE_DUPLEX && (s.T & 1)) s.T++;
        s.N = exchange_total_buffers(s);
        const uint64_t m = rand() % s.N;
        ExchangeCursor c;
        c.seed(s, m);
        for (uint64_t k = m; k < s.N && k < m + 40; ++k, ++checked) {
            uint32_t d, len, d2, len2;
            uint64_t pos;
            exchange_element(s, k, d, pos, len);
            const uint32_t n = c.len(s);
            bad += n != len || c.d != d;
            const bool flipped = c.advance(s, n);
            if (k + 1 < s.N) {
                exchange_element(s, k + 1, d2, pos, len2);
                bad += flipped != (d2 != d);
            }
        }
    }
    std::printf("%ld %u\n", checked, bad);
    return bad != 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "cursor.cpp")
        open(src, "w").write(probe)
        exe = os.path.join(d, "cursor")
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", INCLUDE, "-I", os.path.join(ROOT, "ctstraffic_amd", "csrc"),
                        src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    checked, bad = map(int, out.stdout.split())
    assert out.returncode == 0 and bad == 0 and checked > 1_000_000


# ---- the model by hand ---------------------------------------------------------------------------------------------
class _Table:
    """Connections' paced ticks through the model. pace: per connection a pair (client, server) of settings."""

    def __init__(self, settings, pace, start=0, capacity=8, stride=1008):
        self.e = wl.tcp_exchange_entries(settings)
        self.q = wl.tcp_exchange_pace_entries(pace, start)
        self.n = len(settings)
        self.stride, self.capacity = stride, capacity
        self.arena = np.zeros(max(1, capacity) * stride, dtype=np.uint8)

    def tick(self, now, max_buffers, ids=None, capacity=None):
        v = wl.tcp_paced_exchange_view(self.e, self.q, now, self.stride, self.arena, 0,
                                       self.capacity if capacity is None else capacity,
                                       list(range(self.n)) if ids is None else ids, max_buffers)
        self.e, self.q = v.entries, v.pace
        return v

    def sent(self, v):
        """The tick's buffers as (direction, length) in slot order."""
        n = v.tick["buffers"]
        return [(int(c) // self.n, int(ln)) for c, ln in zip(v.descs["conn_index"][:n], v.descs["length"][:n])]

    def pending(self):
        """Per connection (client entry pending, server entry pending)."""
        return [(int(self.q["pending"][c]), int(self.q["pending"][c + self.n])) for c in range(self.n)]


# PushPull with P = 2500, Q = 1500, B = 1000: kp = 3, kq = 2, a cycle is push 1000 1000 500, pull 1000 500
PP = (PUSHPULL, 1 << 30, 1000, 2500, 1500)
CYCLE = [(0, 1000), (0, 1000), (0, 500), (1, 1000), (1, 500)]


def test_pushpull_client_rate_by_hand():
    """The client sends 3 000 B per 100 ms quantum, the server is not paced, max_buffers = 8.
    t = 0: pushes 1000 1000 500 (2500 of the quantum), the server's 1000 500, push 1000 (2500 < 3000 lets it out:
    3500); the next push finds the quantum full, carries 500 + its own 1000 and waits for the quantum's end at 100.
    Six buffers across two segment ends. t = 50: nothing. t = 100: the held 1000, push 500 (2000), pulls 1000 500,
    push 1000 (3000); the next push finds 3000 >= 3000 and waits for 200."""
    one = _Table([PP], [(dict(bytes_per_second=30000, period_ms=100), {})])
    v = one.tick(0, 8)
    assert one.sent(v) == CYCLE + [(0, 1000)] and v.codes.tolist() == [0]
    assert one.pending() == [(1, 0)] and int(one.q["due_ms"][0]) == 100
    assert int(one.q["bytes_this_quantum"][0]) == 1500 and int(one.q["quantum_start_ms"][0]) == 100
    assert v.tail == {"next_due_ms": 100, "connections_waiting": 0, "connections_pending": 1}
    assert v.tick["bytes_dir"] == [3500, 1500] and v.entries["bytes_sent"].tolist() == [[3500, 1500]]
    assert np.array_equal(one.q[1], wl.tcp_sender_pace_entries([{}])[0])  # the server's entry has not moved
    v = one.tick(50, 8)
    assert one.sent(v) == [] and v.codes.tolist() == [5] and v.wanted.tolist() == [0]
    assert v.tail == {"next_due_ms": 100, "connections_waiting": 1, "connections_pending": 1}
    v = one.tick(100, 8)
    assert one.sent(v) == [(0, 1000), (0, 500), (1, 1000), (1, 500), (0, 1000)]
    assert one.pending() == [(1, 0)] and int(one.q["due_ms"][0]) == 200 == v.tail["next_due_ms"]
    assert int(one.q["bytes_this_quantum"][0]) == 1000 and int(one.q["quantum_start_ms"][0]) == 200
    assert v.descs["expected_pattern_offset"][:5].tolist() == [3500, 4500, 1500, 2500, 5000]


def test_pushpull_server_rate_by_hand():
    """Only the server is paced: 1 000 B per 100 ms. t = 0: the push segment goes out whole, pull 1000 fills the
    quantum, pull 500 waits for 100 on the server's entry (c + n_conns). t = 100: the held 500, the next push segment,
    pull 1000 (500 carried + 1000 = 1500), and the pull 500 behind it waits for 200."""
    one = _Table([PP], [({}, dict(bytes_per_second=10000, period_ms=100))])
    v = one.tick(0, 8)
    assert one.sent(v) == CYCLE[:4] and one.pending() == [(0, 1)]
    assert int(one.q["due_ms"][1]) == 100 == v.tail["next_due_ms"] and v.tail["connections_pending"] == 1
    assert np.array_equal(one.q[0], wl.tcp_sender_pace_entries([{}])[0])  # the client's entry has not moved
    v = one.tick(99, 8)
    assert v.codes.tolist() == [5]
    v = one.tick(100, 8)
    assert one.sent(v) == [(1, 500)] + CYCLE[:4] and one.pending() == [(0, 1)]
    assert int(one.q["due_ms"][1]) == 200 and int(one.q["bytes_this_quantum"][1]) == 1000


def test_pushpull_both_sides_with_different_periods_by_hand():
    """Client 3 000 B per 100 ms, server 1 000 B per 40 ms (25 000 B/s). t = 0: push 1000 1000 500, pull 1000, and
    the pull 500 waits for the server's quantum end at 40. t = 40: the 500, then push 1000 (client: 3500), and the
    next push waits for the client's quantum end at 100: the pending entry has changed sides. t = 100: push 1000,
    push 500 (client: 2000), pull 1000 (the server at 100 is past its quantum [40, 80]: one quantum on, to 80, and
    500 + 1000 - 1000 = 500), pull 500 (1000), push 1000 (3000), and the next push waits for 200."""
    one = _Table([PP], [(dict(bytes_per_second=30000, period_ms=100), dict(bytes_per_second=25000, period_ms=40))])
    v = one.tick(0, 8)
    assert one.sent(v) == CYCLE[:4] and one.pending() == [(0, 1)] and v.tail["next_due_ms"] == 40
    v = one.tick(40, 8)
    assert one.sent(v) == [(1, 500), (0, 1000)] and one.pending() == [(1, 0)] and v.tail["next_due_ms"] == 100
    assert v.tail["connections_pending"] == 1
    v = one.tick(100, 8)
    assert one.sent(v) == [(0, 1000), (0, 500), (1, 1000), (1, 500), (0, 1000)]
    assert one.pending() == [(1, 0)] and v.tail["next_due_ms"] == 200
    assert int(one.q["quantum_start_ms"][1]) == 80 and int(one.q["bytes_this_quantum"][1]) == 1000


def test_pushpull_burst_on_one_side_by_hand():
    """-BurstCount 2 -BurstDelay 30 on the client only: every second client task waits 30 ms; the server's sends
    between them do not count. t = 0: push 1000, and the second push waits for 30. t = 30: it goes out, push 500
    (burst 2 -> 1), pulls 1000 500, and push 1000 (1 -> 0) waits for 60."""
    one = _Table([PP], [(dict(burst_count=2, burst_delay_ms=30), {})])
    v = one.tick(0, 8)
    assert one.sent(v) == CYCLE[:1] and one.pending() == [(1, 0)] and v.tail["next_due_ms"] == 30
    v = one.tick(30, 8)
    assert one.sent(v) == CYCLE[1:] and one.pending() == [(1, 0)] and v.tail["next_due_ms"] == 60
    assert int(one.q["burst_left"][0]) == 0 and int(one.q["burst_left"][1]) == 0 == int(one.q["burst_count"][1])


def test_pushpull_transfer_ends_inside_a_pull_segment_by_hand():
    """T = 4000 + 2500 + 700: the ninth buffer is a pull of 700. Server burst 2 / 5 ms: pulls 1 and 2 of the first
    cycle are tasks 1 and 2 (the second waits), the last pull is task 3."""
    one = _Table([(PUSHPULL, 7200, 1000, 2500, 1500)], [({}, dict(burst_count=2, burst_delay_ms=5))], capacity=16)
    assert int(one.e["total_buffers"][0]) == 9
    v = one.tick(0, 16)
    assert one.sent(v) == CYCLE[:4] and one.pending() == [(0, 1)] and v.tail["next_due_ms"] == 5
    v = one.tick(5, 16)
    assert one.sent(v) == [(1, 500)] + CYCLE[:3] + [(1, 700)] and v.codes.tolist() == [1]
    assert one.pending() == [(0, 0)] and v.tail == NO_TAIL and int(one.q["burst_left"][1]) == 1
    assert v.entries["bytes_sent"].tolist() == [[5000, 2200]] and int(v.entries["finished"][0]) == 1
    assert one.tick(6, 16).codes.tolist() == [2]


def test_duplex_rate_on_direction_0_holds_direction_1_by_hand():
    """Duplex, 5 000 B each way in buffers of 1 000; the client sends 2 000 B per 100 ms, the server is not paced.
    t = 0: d0 d1 d0 d1, then the client's third buffer waits for 100, and with it the server's third, which the
    reference's server could have sent. t = 100: d0 d1 d0 d1, and the client's fifth waits for 200."""
    one = _Table([(DUPLEX, 10000, 1000)], [(dict(bytes_per_second=20000, period_ms=100), {})])
    v = one.tick(0, 8)
    assert one.sent(v) == [(0, 1000), (1, 1000)] * 2 and one.pending() == [(1, 0)] and v.tail["next_due_ms"] == 100
    assert v.entries["bytes_sent"].tolist() == [[2000, 2000]]
    v = one.tick(100, 8)
    assert one.sent(v) == [(0, 1000), (1, 1000)] * 2 and v.tail["next_due_ms"] == 200
    v = one.tick(200, 8)
    assert one.sent(v) == [(0, 1000), (1, 1000)] and v.codes.tolist() == [1] and v.tail == NO_TAIL


def test_pull_reads_only_the_servers_entry():
    """Pull: entry c + n_conns paces, entry c is neither read nor written, whatever it holds. Push: the reverse."""
    for pattern, used in ((PULL, 1), (PUSH, 0)):
        one = _Table([(pattern, 10000, 1000)], [({}, {})])
        one.q[used] = wl.tcp_sender_pace_entries([dict(burst_count=3, burst_delay_ms=7)])[0]
        junk = one.q[1 - used].copy()
        junk["bytes_per_quantum"], junk["pending"], junk["due_ms"], junk["burst_count"] = 5, 1, 10 ** 9, 1
        one.q[1 - used] = junk
        v = one.tick(0, 8)
        assert one.sent(v) == [(used, 1000)] * 2 and int(one.q["pending"][used]) == 1
        assert v.tail == {"next_due_ms": 7, "connections_waiting": 0, "connections_pending": 1}
        assert np.array_equal(one.q[1 - used], junk)
        v = one.tick(7, 8)
        assert one.sent(v) == [(used, 1000)] * 3 and v.tail["next_due_ms"] == 14
        assert np.array_equal(one.q[1 - used], junk)


def test_capacity_cut_in_the_middle_of_a_segment_flip():
    """Client burst 4 / 9 ms, server burst 3 / 5 ms: a connection wants push push push pull pull (client tasks 1-3,
    server tasks 1-2) and its sixth buffer, the client's fourth task, is created and waits. Capacity 9: connection 0
    takes its 5, connection 1 is cut to 4, three pushes and the first pull: its entries are those of four steps from
    the stored ones (client 4 -> 1, server 3 -> 2) and no task beyond the fourth has been created; connection 2 finds
    no room and keeps all three entries; connection 3 (client burst 1) waits whatever the room."""
    pace = [(dict(burst_count=4, burst_delay_ms=9), dict(burst_count=3, burst_delay_ms=5))] * 3 + \
           [(dict(burst_count=1, burst_delay_ms=9), {})]
    tab = _Table([PP] * 4, pace, capacity=9)
    before_e, before_q = tab.e.copy(), tab.q.copy()
    v = tab.tick(0, 8)
    assert v.wanted.tolist() == [5, 5, 5, 0] and v.taken.tolist() == [5, 4, 0, 0] and v.codes.tolist() == [0, 0, 3, 5]
    assert tab.sent(v) == CYCLE + CYCLE[:4]
    n = tab.n
    assert tab.q["burst_left"][:n].tolist() == [0, 1, 4, 0] and tab.q["burst_left"][n:].tolist() == [1, 2, 3, 0]
    assert tab.pending() == [(1, 0), (0, 0), (0, 0), (1, 0)]
    assert tab.q["due_ms"][:n].tolist() == [9, 0, 0, 9]
    for k in (2, 2 + n):
        assert np.array_equal(tab.q[k], before_q[k])
    assert np.array_equal(tab.e[2], before_e[2]) and np.array_equal(tab.e[3], before_e[3])
    assert v.entries["bytes_sent"].tolist()[:2] == [[2500, 1500], [2500, 1000]]
    assert v.tail == {"next_due_ms": 9, "connections_waiting": 1, "connections_pending": 2}
    assert v.tick["connections_no_room"] == 1 and v.tick["buffers"] == 9
    # capacity 0: the waiting connections are still code 5, the others find no room, nothing moves
    e1, q1 = tab.e.copy(), tab.q.copy()
    v0 = tab.tick(5, 8, capacity=0)
    assert v0.codes.tolist() == [5, 3, 3, 5] and v0.tick["buffers"] == 0
    assert np.array_equal(tab.e, e1) and np.array_equal(tab.q, q1)
    assert v0.tail == {"next_due_ms": 9, "connections_waiting": 2, "connections_pending": 2}
    # connection 1 goes on from where four steps left it: the second pull, then the client's fourth task waits
    v = tab.tick(5, 8, ids=[1])
    assert [(int(c), int(ln)) for c, ln in zip(v.descs["conn_index"][:1], v.descs["length"][:1])] == [(1 + n, 500)]
    assert v.tick["buffers"] == 1 and tab.pending()[1] == (1, 0)
    assert int(tab.q["due_ms"][1]) == 14


# ---- the two equalities, model against model -----------------------------------------------------------------------
SETTINGS = [(PUSHPULL, 20_000, 1000, 2500, 1500), (PULL, 5000, 1000), (DUPLEX, 999, 1000), (PUSH, 5000, 1000),
            (PUSHPULL, 100, 10, 25, 5), (PUSH, 10, 10), (PUSHPULL, 100, 10, 25, 5), (DUPLEX, 9000, 1000)]


def test_unpaced_entries_give_the_plain_exchange_tick():
    """Mixed ids with one out of range, a finished entry and two malformed entries (their pace entries hold junk that
    is never read): arena, descriptors, codes, entries, the tick's fields and the sent block are tcp_exchange_view's,
    the pace table is untouched and the tail is {INT64_MAX, 0, 0}. max_buffers = 2^31 is no walk."""
    entries = wl.tcp_exchange_entries(SETTINGS)
    entries["finished"][3] = 1
    entries["pattern"][5] = 4
    entries["pull_bytes"][6] = 0
    n = len(SETTINGS)
    q = wl.tcp_exchange_pace_entries([({}, {})] * n, 3)
    for c in (3, 5, 6):
        for k in (c, c + n):
            q[k]["pending"], q[k]["bytes_per_quantum"], q[k]["due_ms"] = 1, 7, 1
    q[1]["pending"], q[1]["burst_count"] = 1, 1  # a Pull connection's client entry is not used either
    stride, first_slot, capacity = 1008, 3, 11
    arena = np.full((first_slot + capacity + 2) * stride, 0xA5, dtype=np.uint8)
    prior = np.zeros(capacity, dtype=DESC_DTYPE)
    prior["length"] = 77
    ids = [9, 0, 1, 3, 5, 6, 2, 4, 7, 0xFFFFFFFF]
    counters = None
    for now, max_buffers in ((3, 4), (3, 1), (1000, 1 << 31), (1000, 3)):
        plain = wl.tcp_exchange_view(entries, stride, arena, first_slot, capacity, ids, max_buffers, descs=prior,
                                     counters=counters)
        paced = wl.tcp_paced_exchange_view(entries, q, now, stride, arena, first_slot, capacity, ids, max_buffers,
                                           descs=prior, counters=counters)
        for f in ("arena", "descs", "codes", "entries", "prefix", "taken", "direction"):
            assert np.array_equal(getattr(plain, f), getattr(paced, f)), f
        assert plain.tick == paced.tick and plain.counters == paced.counters
        assert np.array_equal(paced.pace, q) and paced.tail == NO_TAIL
        assert paced.tick["buffers"] == min(capacity, int(paced.wanted.sum()))
        entries, counters = paced.entries, paced.counters
    assert {2, 4}.issubset(set(paced.codes.tolist()))


def test_push_entries_give_the_paced_senders_tick():
    """A table of Push entries: arena, descriptors, codes, pace entries [0, n_conns), the tick's first 32 bytes, the
    tail and the sent block are tcp_paced_sender_view's, tick after tick; the entries [n_conns, 2 n_conns) hold junk
    and are never touched."""
    settings = [(10 * 1024 + 1, 1024), (5000, 2000), (999, 1000), (5000, 1000), (100, 10), (30000, 1500)]
    pace = [dict(bytes_per_second=20480, period_ms=100), dict(burst_count=2, burst_delay_ms=15), {},
            dict(burst_count=1, burst_delay_ms=1), dict(bytes_per_second=999, period_ms=1, burst_count=3,
                                                        burst_delay_ms=4),
            dict(bytes_per_second=150_000, period_ms=10)]
    n = len(settings)
    stride, first_slot, capacity = 1504, 2, 3
    s_entries = wl.tcp_sender_entries(settings)
    x_entries = wl.tcp_exchange_entries([(PUSH, T, B) for T, B in settings])
    s_entries["finished"][3] = x_entries["finished"][3] = 1
    s_q = wl.tcp_sender_pace_entries(pace, 5)
    x_q = np.concatenate([s_q, s_q])
    x_q["pending"][n:], x_q["due_ms"][n:] = 1, 99
    junk = x_q[n:].copy()
    arena = np.full((first_slot + capacity + 1) * stride, 0xA5, dtype=np.uint8)
    ids = [7, 0, 1, 3, 2, 4, 5, 0xFFFFFFFF]
    sc = xc = None
    seen = set()
    for now in (5, 5, 9, 20, 20, 55, 105, 106, 240, 1000):
        s = wl.tcp_paced_sender_view(s_entries, s_q, now, stride, arena, first_slot, capacity, ids, 4, counters=sc)
        x = wl.tcp_paced_exchange_view(x_entries, x_q, now, stride, arena, first_slot, capacity, ids, 4, counters=xc)
        assert np.array_equal(s.arena, x.arena) and np.array_equal(s.descs, x.descs)
        assert np.array_equal(s.codes, x.codes) and np.array_equal(s.prefix, x.prefix)
        assert np.array_equal(s.taken, x.taken) and np.array_equal(s.wanted, x.wanted) and s.counters == x.counters
        assert s.tick == {f: x.tick[f] for f in wl.TCP_SENDER_TICK_FIELDS} and s.tail == x.tail
        assert x.tick["bytes_dir"] == [s.tick["bytes"], 0]
        assert np.array_equal(s.pace, x.pace[:n]) and np.array_equal(x.pace[n:], junk)
        assert np.array_equal(s.entries["bytes_sent"], x.entries["bytes_sent"][:, 0])
        s_entries, x_entries, s_q, x_q, sc, xc = s.entries, x.entries, s.pace, x.pace, s.counters, x.counters
        seen |= set(s.codes.tolist())
    assert seen == {0, 1, 2, 3, 4, 5}


# ---- the model against the ctsIoPattern mirror -------------------------------------------------------------------
class _Clock:
    def __init__(self, t):
        self.t = t

    def __call__(self):
        return self.t


def _oracle_verifier(arena, descs):
    return oracle.verify_batch(arena, descs)[0]


class _Side:
    """One side's ctsIoPattern past its connection id, with the receives it has posted."""

    def __init__(self, pattern, listening, T, B, P, Q, pace):
        mirror = {PUSH: A.PATTERN_PUSH, PULL: A.PATTERN_PULL, PUSHPULL: A.PATTERN_PUSHPULL, DUPLEX: A.PATTERN_DUPLEX}
        self.p = IoPattern.MakeIoPattern(
            PatternConfig(io_pattern=mirror[pattern], listening=listening, verify_buffers=True,
                          verify_mode=A.VERIFY_SYNC, pre_post_recvs=1, pre_post_sends=1, buffer_size=B,
                          transfer_size=T, push_bytes=P, pull_bytes=Q,
                          tcp_bytes_per_second=pace.get("bytes_per_second", 0),
                          tcp_bytes_per_second_period=pace.get("period_ms", 0),
                          burst_count=pace.get("burst_count", 0), burst_delay=pace.get("burst_delay_ms", 0)),
            None, verifier=_oracle_verifier)
        t = self.p.InitiateIo()  # the connection id: the server sends it, the client receives it
        assert t.io_action == (A.TASK_SEND if listening else A.TASK_RECV)
        assert t.buffer_length == A.CONNECTION_ID_LENGTH and t.time_offset_ms == 0
        assert self.p.CompleteIo(t, A.CONNECTION_ID_LENGTH, 0) == A.IO_CONTINUE
        self.posted = []
        self.held, self.held_due = None, None

    def next_send(self):
        """The side's next send task; receives it hands out on the way are posted."""
        while True:
            t = self.p.InitiateIo()
            if t.io_action == A.TASK_RECV:
                self.posted.append(t)
                continue
            assert t.io_action == A.TASK_SEND
            return t

    def receive(self, length):
        t = self.posted.pop(0) if self.posted else self.p.InitiateIo()
        assert t.io_action == A.TASK_RECV and t.buffer_length >= length
        IoPattern.recv_from_wire(t, length)
        self.p.CompleteIo(t, length, 0)
        return t.expected_pattern_offset


def _against_the_mirrors(setting, pace, start, steps, max_buffers):
    """Tick by tick along run_x: the side that sends the next buffer is asked for a task; a task with a time offset is
    held until the clock reaches it and goes out first; a released send is completed, then received and completed by
    the other side. Per tick the count, every (direction, length, pattern offset), which side holds a task and its
    due time, and both bytes_sent are the model's."""
    pattern, T, B = setting[:3]
    P, Q = (tuple(setting[3:5]) + (0, 0))[:2]
    shared_buffer_attach(_SENDER)
    clock = _Clock(start)
    clock_set(clock)
    sides = []
    try:
        sides = [_Side(pattern, listening, T, B, P, Q, pace[int(listening)]) for listening in (False, True)]
        tab = _Table([setting], [pace], start=start, capacity=max_buffers, stride=B + (-B) % 16)
        N = int(tab.e["total_buffers"][0])
        total = int(tab.e["transfer_bytes"][0])
        m, counts, sent = 0, [], [0, 0]
        for step in steps:
            clock.t += step
            limit = min(max_buffers, N - m)
            got = []
            while len(got) < limit:
                d = wl.tcp_exchange_element(pattern, total, B, P, Q, m + len(got))[0]
                side = sides[d]
                if side.held is not None:
                    if clock.t < side.held_due:
                        break
                    task, side.held = side.held, None
                else:
                    task = side.next_send()
                    if task.time_offset_ms > 0:
                        side.held, side.held_due = task, clock.t + task.time_offset_ms
                        break
                side.p.CompleteIo(task, task.buffer_length, 0)
                assert sides[1 - d].receive(task.buffer_length) == task.buffer_offset
                got.append((d, task.buffer_length, task.buffer_offset))
                sent[d] += task.buffer_length
            v = tab.tick(clock.t, max_buffers)
            where = (setting, pace, clock.t, len(counts))
            n = v.tick["buffers"]
            assert n == len(got) == int(v.taken[0]), where
            model = [(int(x["conn_index"]), int(x["length"]), int(x["expected_pattern_offset"])) for x in v.descs[:n]]
            assert model == got, where
            m += n
            holds = tuple(int(s.held is not None) for s in sides)
            assert tab.pending() == [holds], where
            assert sum(holds) <= 1
            if any(holds):
                d = holds.index(1)
                assert int(tab.q["due_ms"][d]) == sides[d].held_due == v.tail["next_due_ms"], where
                assert v.tail["connections_pending"] == 1
            else:
                assert v.tail["next_due_ms"] == I64_MAX and v.tail["connections_pending"] == 0
            assert tab.e["bytes_sent"][0].tolist() == sent, where
            if n:
                assert [s.p.stats()["bytes_sent"] for s in sides] == sent, where
            counts.append(n)
            if m == N:
                break
        assert all(s.p.stats()["buffers_failed"] == 0 for s in sides)
        return counts, m == N
    finally:
        for s in sides:
            s.p.close()
        clock_set(None)


def _random_pace(rng):
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return {}
    if kind == 1:
        return dict(burst_count=int(rng.integers(1, 6)), burst_delay_ms=int(rng.choice([1, 4, 20, 50])))
    if kind == 2:  # a rate that rounds to 0 bytes per quantum: the burst settings are in charge
        return dict(bytes_per_second=int(rng.choice([1, 999])), period_ms=1, burst_count=2, burst_delay_ms=7)
    return dict(bytes_per_second=int(rng.choice([1, 100_000, 655_360, 3_000_000, 50_000_000])),
                period_ms=int(rng.choice([1, 10, 100, 250])))


@pytest.mark.parametrize("max_buffers", [1, 3, 8])
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("pattern", [PUSH, PULL, PUSHPULL, DUPLEX])
def test_model_against_the_pattern_mirrors_random(pattern, seed, max_buffers):
    rng = np.random.default_rng(1000 * pattern + seed)
    B = int(rng.integers(1000, 30000))
    P, Q = (int(rng.integers(1, 4 * B)), int(rng.integers(1, 4 * B))) if pattern == PUSHPULL else (0, 0)
    pace = (_random_pace(rng), _random_pace(rng))
    if pace == ({}, {}):
        pace = (dict(bytes_per_second=655_360, period_ms=100), {})
    # every other seed's transfer ends inside the run
    T = int(rng.integers(20 * B, 60 * B)) if seed % 2 else 1 << 40
    periods = [p.get("period_ms", 0) or 100 for p in pace]
    period = int(rng.choice(periods))
    start = int(rng.integers(0, 10 ** 6))
    # the clock stands, moves inside a quantum, by one quantum, by several and one
    steps = [int(rng.choice([0, 0, 1, period // 2, period, 3 * period + 1, 17])) for _ in range(240)]
    counts, ended = _against_the_mirrors((pattern, T, B, P, Q), pace, start, steps, max_buffers)
    assert len(counts) == 240 or ended


@pytest.mark.parametrize("setting,pace,max_buffers", [
    (PP[:1] + (40_500,) + PP[2:], (dict(bytes_per_second=30000, period_ms=100), {}), 8),
    (PP[:1] + (40_500,) + PP[2:], ({}, dict(bytes_per_second=10000, period_ms=100)), 8),
    (PP[:1] + (40_500,) + PP[2:], (dict(bytes_per_second=30000, period_ms=100),
                                   dict(bytes_per_second=25000, period_ms=40)), 8),
    (PP[:1] + (7200,) + PP[2:], ({}, dict(burst_count=2, burst_delay_ms=5)), 3),
    (PP, (dict(burst_count=4, burst_delay_ms=9), dict(burst_count=3, burst_delay_ms=5)), 8),
    ((DUPLEX, 10001, 1000), (dict(bytes_per_second=20000, period_ms=100), {}), 8),
    ((DUPLEX, 200_001, 65531), (dict(burst_count=1, burst_delay_ms=4), dict(bytes_per_second=655_360)), 3),
    ((PULL, 33 * 40 + 1, 33), ({}, dict(burst_count=1, burst_delay_ms=4)), 3),
    ((PULL, 65536 * 40 + 5, 65536), (dict(burst_count=1, burst_delay_ms=1), dict(bytes_per_second=655_360)), 3),
    ((PUSH, 300_000, 1000), (dict(bytes_per_second=10 ** 9, burst_count=1, burst_delay_ms=7), {}), 8),
    ((PUSHPULL, 1_000_000, 65536, 3 * 65536 + 100, 65529), (dict(bytes_per_second=3_000_000, period_ms=10),
                                                             dict(bytes_per_second=999, period_ms=1, burst_count=2,
                                                                  burst_delay_ms=7)), 8),
    ((PUSHPULL, 5000, 4096, 10, 300), (dict(burst_count=3, burst_delay_ms=2), dict(burst_count=2, burst_delay_ms=3)),
     3),
])
def test_model_against_the_pattern_mirrors_settings(setting, pace, max_buffers):
    """The hand-worked settings and their kin through the mirrors: each side's rate, both, bursts, a rate that rounds to
    nothing, a rate over a burst, segments shorter than a buffer, transfers that end inside a segment."""
    rng = np.random.default_rng(setting[2])
    steps = [int(x) for x in rng.choice([0, 1, 3, 10, 25, 50, 120], 300)]
    counts, ended = _against_the_mirrors(setting, pace, 1234, steps, max_buffers)
    assert sum(counts) > 0 and (ended or len(counts) == 300)
