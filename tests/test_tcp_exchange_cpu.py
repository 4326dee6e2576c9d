"""Push, Pull, PushPull and Duplex on the device-resident path, host side (include/cts_tcp_exchange.h): the struct
layouts, the entry helpers, every refused argument of the tick (nothing launches, so no device is needed), and the
model that the GPU tests compare against (ctstraffic_amd.workload.tcp_exchange_view) with its closed form held against
the step-by-step sequence, the ctsIoPattern mirror's tasks on both sides of a connection, and the oracle's pattern
bytes."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from ctstraffic_amd import _pattern_abi as A
from ctstraffic_amd import tcp_exchange as X
from ctstraffic_amd import workload as wl
from ctstraffic_amd._lib import CtsError, lib
from ctstraffic_amd.pattern import IoPattern, PatternConfig, shared_buffer_attach
from ctstraffic_amd.types import (DESC_DTYPE, TCP_EXCHANGE_DTYPE, TCP_EXCHANGE_DUPLEX, TCP_EXCHANGE_PULL,
                                  TCP_EXCHANGE_PUSH, TCP_EXCHANGE_PUSHPULL, TCP_EXCHANGE_TICK_DTYPE,
                                  TCP_SENDER_TICK_DTYPE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
_SENDER = oracle.sender_buffer(4 * 65536)
PUSH, PULL, PUSHPULL, DUPLEX = TCP_EXCHANGE_PUSH, TCP_EXCHANGE_PULL, TCP_EXCHANGE_PUSHPULL, TCP_EXCHANGE_DUPLEX

# (pattern, T, B, P, Q): segments that are and are not multiples of B, B above a segment, a transfer that ends inside a
# push segment, inside a pull segment and at a segment end, odd Duplex transfers, one byte
CASES = [(PUSH, 10 * 1024 + 1, 1024, 0, 0), (PULL, 200_000, 65531, 0, 0), (PULL, 1, 9, 0, 0),
         (PUSHPULL, 1_000_000, 65536, 3 * 65536 + 100, 65529), (PUSHPULL, 700_001, 65531, 200_000, 65531),
         (PUSHPULL, 100_000, 9000, 20000, 9001), (PUSHPULL, 3 * 5472, 1472, 4000, 1472),
         (PUSHPULL, 2 * 107 + 100, 33, 100, 7), (PUSHPULL, 2 * 107 + 103, 33, 100, 7), (PUSHPULL, 50, 33, 100, 7),
         (PUSHPULL, 1, 1, 1, 1), (PUSHPULL, 1000, 4096, 10, 300), (DUPLEX, 200_001, 65531, 0, 0),
         (DUPLEX, 10 * 1024, 1024, 0, 0), (DUPLEX, 1, 1024, 0, 0), (DUPLEX, 2 * 8193 * 3 + 14, 8193, 0, 0)]


def _init_c(pattern, T, B, P=0, Q=0):
    return X.exchange_init(pattern, T, B, P, Q)


def test_layouts_against_offsetof():
    probe = r"""
#include <stdio.h>
#include <stddef.h>
#include "cts_tcp_exchange.h"
#define O(T,f) printf("%s.%s %zu\n", #T, #f, offsetof(T,f))
int main(void){
 printf("sizeof %zu %zu\n", sizeof(cts_tcp_exchange_state), sizeof(cts_tcp_exchange_tick));
 O(cts_tcp_exchange_state,transfer_bytes); O(cts_tcp_exchange_state,total_buffers);
 O(cts_tcp_exchange_state,buffers_sent); O(cts_tcp_exchange_state,bytes_sent); O(cts_tcp_exchange_state,buffer_size);
 O(cts_tcp_exchange_state,pattern); O(cts_tcp_exchange_state,push_bytes); O(cts_tcp_exchange_state,pull_bytes);
 O(cts_tcp_exchange_state,finished); O(cts_tcp_exchange_state,reserved);
 O(cts_tcp_exchange_tick,tick); O(cts_tcp_exchange_tick,bytes_dir);
 printf("patterns %u %u %u %u\n", CTS_TCP_EXCHANGE_PUSH, CTS_TCP_EXCHANGE_PULL, CTS_TCP_EXCHANGE_PUSHPULL,
        CTS_TCP_EXCHANGE_DUPLEX);
 return 0; }
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(probe)
        exe = os.path.join(d, "p")
        subprocess.run(["gcc", "-std=c11", "-I", INCLUDE, c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert list(map(int, lines[0].split()[1:])) == [TCP_EXCHANGE_DTYPE.itemsize, TCP_EXCHANGE_TICK_DTYPE.itemsize] \
        == [64, 48]
    assert list(map(int, lines[-1].split()[1:])) == [PUSH, PULL, PUSHPULL, DUPLEX] == [0, 1, 2, 3]
    mirrors = {"cts_tcp_exchange_state": lambda f: TCP_EXCHANGE_DTYPE.fields[f][1],
               "cts_tcp_exchange_tick": lambda f: 0 if f == "tick" else TCP_EXCHANGE_TICK_DTYPE.fields[f][1]}
    for line in lines[1:-1]:
        name, off = line.split()
        struct, field = name.split(".")
        assert mirrors[struct](field) == int(off), name
    # the block's first 32 bytes are the senders' tick, field for field
    for f in TCP_SENDER_TICK_DTYPE.names:
        assert TCP_EXCHANGE_TICK_DTYPE.fields[f] == TCP_SENDER_TICK_DTYPE.fields[f]
    assert TCP_EXCHANGE_TICK_DTYPE.names[:6] + ("bytes_dir",) == wl.TCP_EXCHANGE_TICK_FIELDS


def test_init():
    for pattern, T, B, P, Q in CASES + [(PUSH, (1 << 64) - 1, (1 << 32) - 1, 0, 0),
                                        (PUSHPULL, (1 << 64) - 1, 1, (1 << 32) - 1, (1 << 32) - 1),
                                        (DUPLEX, (1 << 64) - 2, 1, 5, 6)]:
        e = _init_c(pattern, T, B, P, Q)
        Te = T + T % 2 if pattern == DUPLEX else T
        assert (int(e["transfer_bytes"]), int(e["buffers_sent"]), e["bytes_sent"].tolist(), int(e["buffer_size"]),
                int(e["pattern"]), int(e["push_bytes"]), int(e["pull_bytes"]), int(e["finished"]),
                int(e["reserved"])) == (Te, 0, [0, 0], B, pattern, P, Q, 0, 0)
        assert int(e["total_buffers"]) == wl.tcp_exchange_total_buffers(pattern, T, B, P, Q)
        assert e == wl.tcp_exchange_entries([(pattern, T, B, P, Q)])[0]
    for pattern, T, B, P, Q in CASES:
        assert int(_init_c(pattern, T, B, P, Q)["total_buffers"]) == \
            sum(1 for _ in wl.tcp_exchange_sequence(pattern, T, B, P, Q))
    out = np.zeros(1, dtype=TCP_EXCHANGE_DTYPE)
    L = lib()
    assert L.cts_tcp_exchange_init(PUSH, 1, 1, 0, 0, None) == -1
    for bad in [(PUSH, 0, 1, 0, 0), (PULL, 1, 0, 0, 0), (4, 1, 1, 1, 1), (0xFFFFFFFF, 1, 1, 1, 1),
                (PUSHPULL, 1, 1, 0, 1), (PUSHPULL, 1, 1, 1, 0), (DUPLEX, (1 << 64) - 1, 1, 0, 0)]:
        assert L.cts_tcp_exchange_init(*bad, out.ctypes.data) == -1, bad
        with pytest.raises(CtsError):
            X.exchange_init(*bad)
        with pytest.raises(ValueError):
            wl.tcp_exchange_entries([bad])
    assert not out.view(np.uint8).any()
    assert L.cts_tcp_exchange_init(PUSHPULL, 1, 1, 1, 1, out.ctypes.data) == 0


def test_seek_where_direction_bytes_edges():
    L = lib()
    assert L.cts_tcp_exchange_seek(None, 0) == -1 and L.cts_tcp_exchange_where(None, None, None) == -1
    assert L.cts_tcp_exchange_direction_bytes(None, 0) == 0
    e = _init_c(PUSHPULL, 2 * 107 + 100, 33, 100, 7)  # ends exactly at a push segment's end
    N = int(e["total_buffers"])
    assert N == 2 * 5 + 4
    with pytest.raises(CtsError):
        X.exchange_seek(e, N + 1)
    with pytest.raises(CtsError):
        X.exchange_seek(e, (1 << 64) - 1)
    malformed = e.copy()
    malformed["total_buffers"] = N + 1
    with pytest.raises(CtsError):
        X.exchange_seek(malformed, 0)
    with pytest.raises(CtsError):
        X.exchange_where(malformed)
    assert X.exchange_direction_bytes(malformed, 0) == 0
    assert X.exchange_direction_bytes(e, 2) == 0
    assert (X.exchange_direction_bytes(e, 0), X.exchange_direction_bytes(e, 1)) == (300, 14)
    assert X.exchange_where(e) == (0, 0)
    assert X.exchange_where(X.exchange_seek(e, 3)) == (0, 99)   # the push segment's last buffer is 1 byte
    assert X.exchange_where(X.exchange_seek(e, 4)) == (1, 0)
    assert X.exchange_where(X.exchange_seek(e, 5)) == (0, 0)
    end = X.exchange_seek(e, N)
    assert int(end["finished"]) == 1 and end["bytes_sent"].tolist() == [300, 14]
    assert X.exchange_where(end) == (1, 0)  # the full last segment has flipped the turn
    assert int(X.exchange_seek(end, 0)["finished"]) == 0 and X.exchange_seek(end, 0) == e
    # a transfer that ends inside a pull segment, and inside a push segment
    end = X.exchange_seek(_init_c(PUSHPULL, 2 * 107 + 103, 33, 100, 7), 15)
    assert X.exchange_where(end) == (1, 3) and end["bytes_sent"].tolist() == [300, 17]
    end = X.exchange_seek(_init_c(PUSHPULL, 50, 33, 100, 7), 2)
    assert X.exchange_where(end) == (0, 50) and end["bytes_sent"].tolist() == [50, 0]
    # null outputs of where
    one = np.array([e], dtype=TCP_EXCHANGE_DTYPE)
    assert L.cts_tcp_exchange_where(one.ctypes.data, None, None) == 0
    # Push, Pull, Duplex
    assert X.exchange_where(_init_c(PUSH, 10, 3)) == (0, 0) and X.exchange_where(_init_c(PULL, 10, 3)) == (1, 0)
    d = _init_c(DUPLEX, 13, 3)
    assert int(d["transfer_bytes"]) == 14 and int(d["total_buffers"]) == 6
    assert [X.exchange_where(X.exchange_seek(d, m)) for m in range(7)] == [(m & 1, 0) for m in range(7)]
    assert [X.exchange_seek(d, m)["bytes_sent"].tolist() for m in range(7)] == \
        [[0, 0], [3, 0], [3, 3], [6, 3], [6, 6], [7, 6], [7, 7]]
    assert X.exchange_direction_bytes(d, 0) == X.exchange_direction_bytes(d, 1) == 7
    assert [X.exchange_direction_bytes(_init_c(PUSH, 10, 3), k) for k in (0, 1)] == [10, 0]
    assert [X.exchange_direction_bytes(_init_c(PULL, 10, 3), k) for k in (0, 1)] == [0, 10]


def test_scratch_bytes_grow_with_n():
    b = [X.exchange_scratch_bytes(n) for n in (0, 1, 256, 257, 65536, 0xFFFFFFFF)]
    assert all(x % 8 == 0 for x in b) and b == sorted(b)
    assert b[1] >= 8 * 2 + 8 + 8 + 48 and b[-1] >= 16 * 0xFFFFFFFF


def test_refused_arguments():
    """Every argument check comes before the engine is used: with a null engine, and with a non-null one that is
    never dereferenced because an argument is refused first."""
    L = lib()
    mem = np.zeros(1 << 16, dtype=np.uint8)
    base = (mem.ctypes.data + 63) & ~63  # a 64-byte aligned address inside host memory: only ever compared
    fake_engine = base
    good = dict(engine=fake_engine, arena=base + 4096, arena_bytes=8 * 1488, stride=1488, first_slot=0, capacity=8,
                ids=base + 64, n=2, max_buffers=3, entries=base + 128, n_conns=2, descs=base + 256, codes=base + 512,
                tick=base + 576, sent=base + 640, scratch=base + 1024, scratch_bytes=X.exchange_scratch_bytes(2))

    def send(**over):
        a = dict(good, **over)
        return L.cts_tcp_exchange_send(a["engine"], a["arena"], a["arena_bytes"], a["stride"], a["first_slot"],
                                       a["capacity"], a["ids"], a["n"], a["max_buffers"], a["entries"], a["n_conns"],
                                       a["descs"], a["codes"], a["tick"], a["sent"], a["scratch"], a["scratch_bytes"],
                                       None)

    assert send(engine=None) == -1
    assert send(engine=None, n=0) == -1            # a null engine is refused before n == 0 is looked at
    assert send(n=0, stride=7, arena=None) == 0    # n == 0 is CTS_OK whatever else is passed
    bad = [dict(stride=1480), dict(stride=0), dict(stride=8), dict(stride=(16 << 20) + 16), dict(max_buffers=0),
           dict(arena=None), dict(arena=good["arena"] + 8),
           dict(first_slot=1), dict(capacity=9), dict(first_slot=9, capacity=0), dict(first_slot=(1 << 64) - 1),
           dict(first_slot=(1 << 64) - 4, capacity=8), dict(arena_bytes=8 * 1488 - 1),
           dict(ids=None), dict(ids=good["ids"] + 2), dict(entries=None), dict(entries=good["entries"] + 4),
           dict(descs=None), dict(descs=good["descs"] + 4), dict(codes=good["codes"] + 2),
           dict(tick=good["tick"] + 4), dict(sent=good["sent"] + 4), dict(scratch=None),
           dict(scratch=good["scratch"] + 4), dict(scratch_bytes=good["scratch_bytes"] - 1), dict(scratch_bytes=0),
           dict(scratch_bytes=X.exchange_scratch_bytes(2) - 16),  # the senders' scratch is 16 bytes too small
           dict(n_conns=(1 << 31) + 1), dict(n_conns=0xFFFFFFFF)]
    for kw in bad:
        assert send(**kw) == -1, kw
    assert not mem.any()


def _segment_sizes(B):
    return sorted({1, B, B + 1, max(1, 2 * B - 1), 3 * B, 3 * B + 1})


def test_closed_form_against_the_sequence_sweep():
    """B in 1..40; P and Q in 1..3B+1 (1, B, B+1, 2B-1, 3B, 3B+1: multiples of B and not, below it and above); every T
    up to three cycles and a byte. For every T the walked sequence has N elements and every element m is the closed
    form's, through the numpy form that the tick's model runs; and the bytes by direction before every m are the closed
    form's position, which covers every (m0, t) split: the bytes of buffers m0 .. m0 + t are position(m0 + t) -
    position(m0)."""
    u = np.uint64
    for B in range(1, 41):
        for P in _segment_sizes(B):
            for Q in _segment_sizes(B):
                want, params, ms, before = [], [], [], []
                for T in range(1, 3 * (P + Q) + 2):
                    seq = list(wl.tcp_exchange_sequence(PUSHPULL, T, B, P, Q))
                    assert len(seq) == wl.tcp_exchange_total_buffers(PUSHPULL, T, B, P, Q), (B, P, Q, T)
                    sent = [0, 0]
                    for m, (d, pos, length, intra) in enumerate(seq):
                        assert pos == sent[d]
                        before.append((sent[0], sent[1]))
                        sent[d] += length
                    assert sent[0] + sent[1] == T
                    assert wl.tcp_exchange_position(PUSHPULL, T, B, P, Q, len(seq)) == sent, (B, P, Q, T)
                    want += [s[:3] for s in seq]
                    ms += range(len(seq))
                    params += [T] * len(seq)
                E = np.zeros(len(ms), dtype=TCP_EXCHANGE_DTYPE)
                E["transfer_bytes"], E["buffer_size"], E["pattern"], E["push_bytes"], E["pull_bytes"] = \
                    params, B, PUSHPULL, P, Q
                d, pos, length = wl._exchange_elements(E, np.array(ms, dtype=u))
                got = np.stack([d, pos, length], axis=1)
                assert np.array_equal(got, np.array(want, dtype=u)), (B, P, Q)
                # position(m) for m < N: direction d stands at pos, the other where the walk left it
                b = np.array(before, dtype=u)
                assert np.array_equal(np.where(d == 0, b[:, 0], b[:, 1]), pos), (B, P, Q)
        # the Python-integer closed form, the one the 2^50 test runs, and the C helpers, on this B's last shape
        for T in (1, P, P + Q, 2 * (P + Q) + P, 3 * (P + Q) + 1):
            e = _init_c(PUSHPULL, T, B, P, Q)
            sent = [0, 0]
            for m, s in enumerate(wl.tcp_exchange_sequence(PUSHPULL, T, B, P, Q)):
                assert wl.tcp_exchange_element(PUSHPULL, T, B, P, Q, m) == s
                assert wl.tcp_exchange_position(PUSHPULL, T, B, P, Q, m) == sent
                at = X.exchange_seek(e, m)
                assert at["bytes_sent"].tolist() == sent and X.exchange_where(at) == (s[0], s[3])
                sent[s[0]] += s[2]
            assert X.exchange_seek(e, m + 1)["bytes_sent"].tolist() == sent
            assert [X.exchange_direction_bytes(e, k) for k in (0, 1)] == sent


@pytest.mark.parametrize("pattern,T,B,P,Q", CASES)
def test_closed_form_and_helpers_against_the_sequence(pattern, T, B, P, Q):
    """All four patterns: every element, every position, seek, where and direction_bytes against the walk."""
    e = _init_c(pattern, T, B, P, Q)
    seq = list(wl.tcp_exchange_sequence(pattern, T, B, P, Q))
    assert len(seq) == int(e["total_buffers"])
    sent = [0, 0]
    for m, s in enumerate(seq):
        assert wl.tcp_exchange_element(pattern, T + (T % 2 if pattern == DUPLEX else 0), B, P, Q, m) == s, m
        assert wl.tcp_exchange_position(pattern, T, B, P, Q, m) == sent, m
        at = X.exchange_seek(e, m)
        assert at["bytes_sent"].tolist() == sent and int(at["buffers_sent"]) == m and int(at["finished"]) == 0
        assert X.exchange_where(at) == (s[0], s[3]), m
        assert at == wl.tcp_exchange_entries([(pattern, T, B, P, Q)], seek=[m])[0]
        sent[s[0]] += s[2]
    assert [X.exchange_direction_bytes(e, k) for k in (0, 1)] == sent
    assert sum(sent) == int(e["transfer_bytes"])


def _ticks(settings, stride, max_buffers, capacity, ids=None, first_slot=0, seek=None, max_ticks=100000):
    """Ticks of the model until nothing is sent. Returns per connection its (direction, length, offset) list and the
    views."""
    entries = wl.tcp_exchange_entries(settings, seek=seek)
    ids = list(range(len(settings))) if ids is None else ids
    arena = np.full((first_slot + capacity) * stride, 0xA5, dtype=np.uint8)
    sends = [[] for _ in settings]
    views, counters = [], None
    n_conns = len(settings)
    for _ in range(max_ticks):
        v = wl.tcp_exchange_view(entries, stride, arena, first_slot, capacity, ids, max_buffers, counters=counters)
        views.append(v)
        entries, counters = v.entries, v.counters
        for d in v.descs[: v.tick["buffers"]]:
            c, k = int(d["conn_index"]) % n_conns, int(d["conn_index"]) // n_conns
            sends[c].append((k, int(d["length"]), int(d["expected_pattern_offset"])))
        if v.tick["buffers"] == 0:
            break
    return sends, views


@pytest.mark.parametrize("max_buffers", [1, 3, 1000])
def test_model_ticks_against_the_sequence(max_buffers):
    """All CASES as connections of one table, in a shuffled list, with a capacity that cuts ticks short, so that
    every (m0, t) split that these ticks make is summed by the model's move: every connection's buffers are the
    walk's, in order, and the entries stay what seek gives."""
    stride = 65536
    ids = [int(x) for x in np.random.default_rng(max_buffers).permutation(len(CASES))]
    sends, views = _ticks(CASES, stride, max_buffers, capacity=7, ids=ids, first_slot=2)
    for c, case in enumerate(CASES):
        assert sends[c] == [(d, ln, pos % 65536) for d, pos, ln, _ in wl.tcp_exchange_sequence(*case)], case
    last = views[-1]
    assert (last.entries["finished"] == 1).all() and set(last.codes.tolist()) == {2}
    assert np.array_equal(last.entries["buffers_sent"], last.entries["total_buffers"])
    assert np.array_equal(last.entries["bytes_sent"].sum(axis=1), last.entries["transfer_bytes"])
    assert last.counters["bytes_sent"] == int(last.entries["transfer_bytes"].sum())
    assert last.counters["buffers_sent"] == sum(len(s) for s in sends)
    assert last.counters["connections_finished"] == len(CASES)
    assert any(3 in v.codes.tolist() for v in views) and all(v.tick["buffers"] <= 7 for v in views)
    for v in views:
        assert np.array_equal(v.entries, wl.tcp_exchange_entries(CASES, seek=v.entries["buffers_sent"]))
        n = v.tick["buffers"]
        assert v.tick["bytes"] == int(v.descs["length"][:n].sum()) == sum(v.tick["bytes_dir"])
        assert v.tick["bytes_dir"][1] == int(v.descs["length"][:n][v.descs["conn_index"][:n] >= len(CASES)].sum())
        assert v.tick["connections_no_room"] == v.codes.tolist().count(3)
        assert v.tick["connections_skipped"] == v.codes.tolist().count(2) + v.codes.tolist().count(4)
        assert v.tick["connections_finished"] == v.codes.tolist().count(1)


def test_closed_form_past_2_pow_33_buffers():
    """T about 2^50 with m0 beyond 2^33, in Python integers: the closed form at m0 .. m0 + t against the walk started
    from the cycle's first buffer (a cycle starts where the closed form says, which the sweep has held against the
    walk), the model's tick over a seeked entry, and the C helpers at the same position."""
    B, P, Q = 65531, 200_003, 70_001
    T = (1 << 50) + 12345
    kp, kq, C = -(-P // B), -(-Q // B), P + Q
    K = kp + kq
    N = wl.tcp_exchange_total_buffers(PUSHPULL, T, B, P, Q)
    assert N > 1 << 33
    for m0 in ((1 << 33) + 5, (1 << 33) + K * 1000 + kp - 1, N - 4):
        y = m0 // K
        # the walk over the three cycles from cycle y on is the walk of a transfer of what is left, shifted
        left = min(T - y * C, 3 * C)
        walk = list(wl.tcp_exchange_sequence(PUSHPULL, left, B, P, Q))
        for j in range(min(3 * K, N - y * K)):
            d, pos, length, intra = walk[j]
            assert wl.tcp_exchange_element(PUSHPULL, T, B, P, Q, y * K + j) == (d, pos + y * (P, Q)[d], length, intra)
        e = _init_c(PUSHPULL, T, B, P, Q)
        at = X.exchange_seek(e, m0)
        assert at == wl.tcp_exchange_entries([(PUSHPULL, T, B, P, Q)], seek=[m0])[0]
        d0, pos0, _, intra0 = wl.tcp_exchange_element(PUSHPULL, T, B, P, Q, m0)
        assert X.exchange_where(at) == (d0, intra0) and int(at["bytes_sent"][d0]) == pos0
        v = wl.tcp_exchange_view(np.array([at]), 65536, np.zeros(8 * 65536, dtype=np.uint8), 0, 8, [0], 6)
        t = min(6, N - m0)
        assert v.tick["buffers"] == t and int(v.entries["buffers_sent"][0]) == m0 + t
        for j in range(t):
            d, pos, length, _ = wl.tcp_exchange_element(PUSHPULL, T, B, P, Q, m0 + j)
            assert (int(v.descs["conn_index"][j]), int(v.descs["length"][j]),
                    int(v.descs["expected_pattern_offset"][j])) == (d, length, pos % 65536)
        assert v.entries[0] == X.exchange_seek(e, m0 + t)
    end = X.exchange_seek(e, N)
    assert int(end["bytes_sent"].sum()) == T and int(end["finished"]) == 1
    # Duplex and Pull that far out
    for pattern in (PULL, DUPLEX):
        e = _init_c(pattern, T, B)
        m0 = (1 << 33) + 7
        at = X.exchange_seek(e, m0)
        assert at == wl.tcp_exchange_entries([(pattern, T, B)], seek=[m0])[0]
        d, pos, length, _ = wl.tcp_exchange_element(pattern, int(e["transfer_bytes"]), B, 0, 0, m0)
        assert int(at["bytes_sent"][d]) == pos and length == B


def _oracle_verifier(arena, descs):
    return oracle.verify_batch(arena, descs)[0]


def _drive(pattern, listening, T, B, P, Q):
    """One side's ctsIoPattern through initiate_io / complete_io, one task at a time, every task completed in full:
    the side's tasks as (action, length, pattern offset, bytes completed in the current run of that action before the
    task), up to the end of the transfer."""
    mirror = {PUSH: A.PATTERN_PUSH, PULL: A.PATTERN_PULL, PUSHPULL: A.PATTERN_PUSHPULL, DUPLEX: A.PATTERN_DUPLEX}
    p = IoPattern.MakeIoPattern(PatternConfig(io_pattern=mirror[pattern], listening=listening, verify_buffers=True,
                                              verify_mode=A.VERIFY_SYNC, pre_post_recvs=1, pre_post_sends=1,
                                              buffer_size=B, transfer_size=T, push_bytes=P, pull_bytes=Q), None,
                                verifier=_oracle_verifier)
    try:
        t = p.InitiateIo()  # the connection id: the server sends it, the client receives it
        assert t.io_action == (A.TASK_SEND if listening else A.TASK_RECV)
        assert t.buffer_length == A.CONNECTION_ID_LENGTH
        assert p.CompleteIo(t, A.CONNECTION_ID_LENGTH, 0) == A.IO_CONTINUE
        total = T + (T % 2 if pattern == DUPLEX else 0)
        tasks, done, run, last = [], 0, 0, None
        while done < total:
            t = p.InitiateIo()
            assert t.io_action in (A.TASK_SEND, A.TASK_RECV)
            if t.io_action != last:
                run, last = 0, t.io_action
            offset = t.buffer_offset if t.io_action == A.TASK_SEND else t.expected_pattern_offset
            tasks.append((t.io_action, t.buffer_length, offset, run))
            if t.io_action == A.TASK_RECV:
                IoPattern.recv_from_wire(t, t.buffer_length)  # the bytes the other side's model sends
            assert p.CompleteIo(t, t.buffer_length, 0) == A.IO_CONTINUE
            done += t.buffer_length
            run += t.buffer_length
        s = p.stats()
        assert s["buffers_failed"] == 0
        return tasks, s["bytes_sent"], s["bytes_recv"]
    finally:
        p.close()


@pytest.mark.parametrize("pattern,T,B,P,Q", CASES)
def test_sequence_against_the_pattern_mirror(pattern, T, B, P, Q):
    """A client and a server ctsIoPattern of the pattern, no engine. Direction 0 is what the client sends and the
    server receives, direction 1 the reverse: each side's sends, and its receives, have the model's lengths and
    pattern offsets for their direction, in the model's order; for PushPull, which has one task at a time, the whole
    task order is the model's and cts_tcp_exchange_where at every position is the mirror's turn (which action it
    hands out, and how many bytes of the segment it has completed)."""
    shared_buffer_attach(_SENDER)
    seq = list(wl.tcp_exchange_sequence(pattern, T, B, P, Q))
    e = _init_c(pattern, T, B, P, Q)
    for listening in (False, True):
        tasks, bytes_sent, bytes_recv = _drive(pattern, listening, T, B, P, Q)
        sends_dir = 1 if listening else 0
        for action, d in ((A.TASK_SEND, sends_dir), (A.TASK_RECV, 1 - sends_dir)):
            got = [(ln, off) for a, ln, off, _ in tasks if a == action]
            assert got == [(ln, pos % 65536) for k, pos, ln, _ in seq if k == d], (listening, action)
        assert bytes_sent == X.exchange_direction_bytes(e, sends_dir)
        assert bytes_recv == X.exchange_direction_bytes(e, 1 - sends_dir)
        if pattern != DUPLEX:
            assert len(tasks) == len(seq)
            for m, (action, ln, off, run) in enumerate(tasks):
                direction, intra = X.exchange_where(X.exchange_seek(e, m))
                sending = action == A.TASK_SEND
                assert sending == (direction == sends_dir), (listening, m)
                if pattern == PUSHPULL:
                    assert intra == run, (listening, m)


def test_payload_bytes_against_the_oracle():
    """Every written slot holds g_senderSharedBuffer[offset .. offset + length), nothing else is touched, and the
    oracle's fill over the model's descriptors writes the same arena."""
    settings = [(PUSHPULL, 700_001, 65531, 200_000, 65531), (DUPLEX, 5 * 8193 - 7, 8193), (PUSHPULL, 500, 33, 100, 7),
                (PULL, 70_001 * 2 + 5, 70_001), (PUSH, 1, 9)]
    stride, first_slot, capacity = 70_016, 1, 9
    S = oracle.sender_buffer(70_001)
    entries = wl.tcp_exchange_entries(settings)
    for tick in range(4):
        arena = np.full((first_slot + capacity + 1) * stride, 0xA5, dtype=np.uint8)
        v = wl.tcp_exchange_view(entries, stride, arena, first_slot, capacity, [3, 0, 4, 2, 1], 3)
        n = v.tick["buffers"]
        assert n > 0
        want = arena.copy()
        for d in v.descs[:n]:
            o, ln, off = int(d["byte_offset"]), int(d["length"]), int(d["expected_pattern_offset"])
            assert o % stride == 0 and first_slot <= o // stride < first_slot + n
            want[o:o + ln] = S[off:off + ln]
        assert np.array_equal(v.arena, want)
        filled = arena.copy()
        oracle.fill(filled, np.ascontiguousarray(v.descs[:n]))
        assert np.array_equal(v.arena, filled)
        results, counters, _ = oracle.verify_batch(v.arena, np.ascontiguousarray(v.descs[:n]))
        assert results["pass"].all() and counters["bytes_ok"] == v.tick["bytes"]
        entries = v.entries


def test_model_of_push_entries_is_the_senders_model():
    """A table of Push entries: arena, descriptors, codes, the tick's six fields, the sent block, prefix and taken are
    tcp_sender_view's, tick after tick, with ids out of range, a finished entry and a B above the stride among
    them."""
    settings = [(10 * 1024 + 1, 1024), (5000, 2000), (999, 1000), (5000, 1000), (100, 10), (3000, 1500)]
    stride, first_slot, capacity = 1504, 2, 6
    s_entries = wl.tcp_sender_entries(settings)
    x_entries = wl.tcp_exchange_entries([(PUSH, T, B) for T, B in settings])
    s_entries["finished"][3] = 1
    x_entries["finished"][3] = 1
    arena = np.full((first_slot + capacity + 1) * stride, 0xA5, dtype=np.uint8)
    prior = np.zeros(capacity, dtype=DESC_DTYPE)
    prior["length"] = 77
    ids = [7, 0, 1, 3, 2, 4, 5, 0xFFFFFFFF]
    sc = xc = None
    for _ in range(8):
        s = wl.tcp_sender_view(s_entries, stride, arena, first_slot, capacity, ids, 4, descs=prior, counters=sc)
        x = wl.tcp_exchange_view(x_entries, stride, arena, first_slot, capacity, ids, 4, descs=prior, counters=xc)
        assert np.array_equal(s.arena, x.arena) and np.array_equal(s.descs, x.descs)
        assert np.array_equal(s.codes, x.codes) and np.array_equal(s.prefix, x.prefix)
        assert np.array_equal(s.taken, x.taken) and s.counters == x.counters
        assert s.tick == {f: x.tick[f] for f in wl.TCP_SENDER_TICK_FIELDS} and x.tick["bytes_dir"] == [s.tick["bytes"], 0]
        for f in ("buffers_sent", "finished", "transfer_bytes", "buffer_size"):
            assert np.array_equal(s.entries[f], x.entries[f])
        assert np.array_equal(s.entries["bytes_sent"], x.entries["bytes_sent"][:, 0])
        s_entries, x_entries, sc, xc = s.entries, x.entries, s.counters, x.counters
    assert s.tick["buffers"] == 0 and 4 in s.codes.tolist() and 2 in s.codes.tolist()


def test_model_skips_and_capacity():
    """Codes and slots by hand: an id beyond the table, B above the stride, an unknown pattern, a PushPull entry
    without a pull segment, a finished entry, a partial take across a segment end and NO_ROOM behind it."""
    entries = wl.tcp_exchange_entries([(PUSHPULL, 5000, 1000, 2500, 1000), (PULL, 5000, 2000), (DUPLEX, 999, 1000),
                                       (PUSH, 5000, 1000), (PUSHPULL, 100, 10, 25, 5), (PUSH, 10, 10),
                                       (PUSHPULL, 100, 10, 25, 5)])
    entries["finished"][3] = 1
    entries["pattern"][5] = 4
    entries["pull_bytes"][6] = 0
    stride, first_slot, capacity = 1008, 3, 7
    arena = np.full((first_slot + capacity + 2) * stride, 0xA5, dtype=np.uint8)
    v = wl.tcp_exchange_view(entries, stride, arena, first_slot, capacity, [9, 0, 1, 3, 5, 6, 2, 4, 0xFFFFFFFF], 4)
    assert v.codes.tolist() == [4, 0, 4, 2, 4, 4, 1, 0, 4]
    assert v.prefix.tolist() == [0, 0, 4, 4, 4, 4, 4, 6, 10] and v.taken.tolist() == [0, 4, 0, 0, 0, 0, 2, 1, 0]
    # connection 0: 1000, 1000, 500 pushed, then the pull segment's 1000; connection 2: 500 each way; 4: 10 pushed
    assert v.descs["conn_index"].tolist() == [0, 0, 0, 0 + 7, 2, 2 + 7, 4]
    assert v.descs["length"].tolist() == [1000, 1000, 500, 1000, 500, 500, 10]
    assert v.descs["expected_pattern_offset"].tolist() == [0, 1000, 2000, 0, 0, 0, 0]
    assert v.tick == {"bytes": 4510, "buffers": 7, "connections_sent": 3, "connections_finished": 1,
                      "connections_no_room": 0, "connections_skipped": 6, "bytes_dir": [3010, 1500]}
    assert v.entries["bytes_sent"].tolist() == [[2500, 1000], [0, 0], [500, 500], [0, 0], [10, 0], [0, 0], [0, 0]]
    rows = v.arena.reshape(-1, stride)
    assert (rows[:3] == 0xA5).all() and (rows[10:] == 0xA5).all() and (rows[3:5, 1000:] == 0xA5).all()
    assert (rows[5, 500:] == 0xA5).all() and (rows[9, 10:] == 0xA5).all()
    v0 = wl.tcp_exchange_view(v.entries, stride, arena, first_slot, 0, [0, 4], 4)
    assert v0.codes.tolist() == [3, 3] and np.array_equal(v0.arena, arena) and np.array_equal(v0.entries, v.entries)
    assert v0.tick["connections_no_room"] == 2 and v0.tick["bytes_dir"] == [0, 0]
