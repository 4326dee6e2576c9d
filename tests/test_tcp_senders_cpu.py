"""TCP senders on the device-resident path, host side (include/cts_tcp_senders.h): the entry initialiser, the struct
layouts, every refused argument of the tick (nothing launches, so no device is needed), and the model that the GPU
tests compare against (ctstraffic_amd.workload.tcp_sender_view) held against the reference's send arithmetic, the
ctsIoPattern mirror's send tasks and the oracle's pattern bytes."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from ctstraffic_amd import _pattern_abi as A
from ctstraffic_amd import distributed as D
from ctstraffic_amd import tcp_senders as T
from ctstraffic_amd import workload as wl
from ctstraffic_amd._lib import CtsCountersSent, CtsError, lib
from ctstraffic_amd.pattern import IoPattern, PatternConfig, shared_buffer_attach
from ctstraffic_amd.types import (DESC_DTYPE, SENT_FIELDS, TCP_SENDER_DTYPE, TCP_SENDER_TICK_DTYPE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
_SENDER = oracle.sender_buffer(4 * 65536)

# transfers that are and are not multiples of B, B odd and even, B above 65 536, a transfer of one byte
CASES = [(10 * 1024, 1024), (10 * 1024 + 1, 1024), (1, 1024), (1, 1), (65536 * 3, 65536), (200_000, 65531),
         (5 * 8193 - 7, 8193), (70_001 * 3 + 5, 70_001), (33 * 700 + 32, 33), (131072 + 9000, 9000), (1472, 1472),
         (100_000 * 2, 100_000)]


def _one_send_at_a_time(transfer, B):
    """ctsIOPattern.cpp:550-575, 676-697: (length, m_sendPatternOffset) of every send of one connection."""
    out, remaining, offset = [], transfer, 0
    while remaining:
        n = min(B, remaining)
        out.append((n, offset))
        offset += n
        offset %= 65536
        remaining -= n
    return out


def _run(settings, stride, max_buffers, capacity, ids=None, first_slot=0, max_ticks=100000):
    """Ticks of the model until every listed connection has ended. Returns per connection its (length, offset) list,
    and the views."""
    entries = wl.tcp_sender_entries(settings)
    ids = list(range(len(settings))) if ids is None else ids
    arena = np.full((first_slot + capacity) * stride, 0xA5, dtype=np.uint8)
    sends = [[] for _ in settings]
    views, counters = [], None
    for _ in range(max_ticks):
        v = wl.tcp_sender_view(entries, stride, arena, first_slot, capacity, ids, max_buffers, counters=counters)
        views.append(v)
        entries, counters = v.entries, v.counters
        for d in v.descs[: v.tick["buffers"]]:
            sends[int(d["conn_index"])].append((int(d["length"]), int(d["expected_pattern_offset"])))
        if v.tick["buffers"] == 0:
            break
    return sends, views


def test_layouts_against_offsetof():
    probe = r"""
#include <stdio.h>
#include <stddef.h>
#include "cts_tcp_senders.h"
#define O(T,f) printf("%s.%s %zu\n", #T, #f, offsetof(T,f))
int main(void){
 printf("sizeof %zu %zu %zu\n", sizeof(cts_tcp_sender_state), sizeof(cts_tcp_sender_tick), sizeof(cts_counters_sent));
 O(cts_tcp_sender_state,bytes_sent); O(cts_tcp_sender_state,transfer_bytes); O(cts_tcp_sender_state,buffers_sent);
 O(cts_tcp_sender_state,buffer_size); O(cts_tcp_sender_state,finished);
 O(cts_tcp_sender_tick,bytes); O(cts_tcp_sender_tick,buffers); O(cts_tcp_sender_tick,connections_sent);
 O(cts_tcp_sender_tick,connections_finished); O(cts_tcp_sender_tick,connections_no_room);
 O(cts_tcp_sender_tick,connections_skipped); O(cts_tcp_sender_tick,reserved);
 O(cts_counters_sent,bytes_sent); O(cts_counters_sent,buffers_sent); O(cts_counters_sent,connections_finished);
 return 0; }
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(probe)
        exe = os.path.join(d, "p")
        subprocess.run(["gcc", "-std=c11", "-I", INCLUDE, c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert list(map(int, lines[0].split()[1:])) == [TCP_SENDER_DTYPE.itemsize, TCP_SENDER_TICK_DTYPE.itemsize,
                                                    ctypes.sizeof(CtsCountersSent)] == [32, 32, 48]
    mirrors = {"cts_tcp_sender_state": lambda f: TCP_SENDER_DTYPE.fields[f][1],
               "cts_tcp_sender_tick": lambda f: TCP_SENDER_TICK_DTYPE.fields[f][1],
               "cts_counters_sent": lambda f: getattr(CtsCountersSent, f).offset}
    for line in lines[1:]:
        name, off = line.split()
        struct, field = name.split(".")
        assert mirrors[struct](field) == int(off), name
    assert tuple(f for f, _ in CtsCountersSent._fields_) == SENT_FIELDS == D.SENT_FIELDS == wl.SENT_FIELDS
    assert TCP_SENDER_TICK_DTYPE.names[:6] == wl.TCP_SENDER_TICK_FIELDS


def test_init():
    for transfer, B in CASES + [((1 << 64) - 1, (1 << 32) - 1)]:
        e = T.sender_init(transfer, B)
        assert (int(e["bytes_sent"]), int(e["transfer_bytes"]), int(e["buffers_sent"]), int(e["buffer_size"]),
                int(e["finished"])) == (0, transfer, 0, B, 0)
        assert e == wl.tcp_sender_entries([(transfer, B)])[0]
    out = np.zeros(1, dtype=TCP_SENDER_DTYPE)
    L = lib()
    assert L.cts_tcp_sender_init(1, 1, None) == -1
    assert L.cts_tcp_sender_init(0, 1, out.ctypes.data) == -1
    assert L.cts_tcp_sender_init(1, 0, out.ctypes.data) == -1
    assert L.cts_tcp_sender_init(1, 1, out.ctypes.data) == 0
    for bad in [(0, 1024), (1024, 0)]:
        with pytest.raises(CtsError):
            T.sender_init(*bad)
        with pytest.raises(ValueError):
            wl.tcp_sender_entries([bad])


def test_scratch_bytes_grow_with_n():
    b = [T.senders_scratch_bytes(n) for n in (0, 1, 256, 257, 65536, 0xFFFFFFFF)]
    assert all(x % 8 == 0 for x in b) and b == sorted(b)
    assert b[1] >= 8 * 2 + 8 + 8 + 32 and b[-1] >= 16 * 0xFFFFFFFF


def test_refused_arguments():
    """Every argument check comes before the engine is used: with a null engine, and with a non-null one that is
    never dereferenced because an argument is refused first."""
    L = lib()
    mem = np.zeros(1 << 16, dtype=np.uint8)
    base = (mem.ctypes.data + 63) & ~63  # a 64-byte aligned address inside host memory: only ever compared
    fake_engine = base
    good = dict(engine=fake_engine, arena=base + 4096, arena_bytes=8 * 1488, stride=1488, first_slot=0, capacity=8,
                ids=base + 64, n=2, max_buffers=3, senders=base + 128, n_conns=2, descs=base + 256, codes=base + 512,
                tick=base + 576, sent=base + 640, scratch=base + 1024, scratch_bytes=T.senders_scratch_bytes(2))

    def send(**over):
        a = dict(good, **over)
        return L.cts_tcp_senders_send(a["engine"], a["arena"], a["arena_bytes"], a["stride"], a["first_slot"],
                                      a["capacity"], a["ids"], a["n"], a["max_buffers"], a["senders"], a["n_conns"],
                                      a["descs"], a["codes"], a["tick"], a["sent"], a["scratch"], a["scratch_bytes"],
                                      None)

    assert send(engine=None) == -1
    assert send(engine=None, n=0) == -1            # a null engine is refused before n == 0 is looked at
    assert send(n=0, stride=7, arena=None) == 0    # n == 0 is CTS_OK whatever else is passed
    bad = [dict(stride=1480), dict(stride=0), dict(stride=8), dict(stride=(16 << 20) + 16), dict(max_buffers=0),
           dict(arena=None), dict(arena=good["arena"] + 8),
           dict(first_slot=1), dict(capacity=9), dict(first_slot=9, capacity=0), dict(first_slot=(1 << 64) - 1),
           dict(first_slot=(1 << 64) - 4, capacity=8), dict(arena_bytes=8 * 1488 - 1),
           dict(ids=None), dict(ids=good["ids"] + 2), dict(senders=None), dict(senders=good["senders"] + 4),
           dict(descs=None), dict(descs=good["descs"] + 4), dict(codes=good["codes"] + 2),
           dict(tick=good["tick"] + 4), dict(sent=good["sent"] + 4), dict(scratch=None),
           dict(scratch=good["scratch"] + 4), dict(scratch_bytes=good["scratch_bytes"] - 1), dict(scratch_bytes=0)]
    for kw in bad:
        assert send(**kw) == -1, kw
    assert not mem.any()
    out = CtsCountersSent()
    assert L.cts_counters_read_sent(None, None, ctypes.byref(out), None) == -1
    assert L.cts_counters_read_sent(fake_engine, base, None, None) == -1
    assert L.cts_counters_read_multi_sent(None, None, None, 1, None) == -1
    assert L.cts_counters_allreduce_sent(None, None, None, 1, None) == -1


@pytest.mark.parametrize("max_buffers", [1, 3, 1000])
def test_model_against_the_reference_arithmetic(max_buffers):
    """All CASES as connections of one table, in a shuffled list, with a capacity that cuts ticks short: every
    connection's sends are the one-send-at-a-time loop's, in order."""
    stride = 100_000 + 16 - 100_000 % 16
    ids = [int(x) for x in np.random.default_rng(max_buffers).permutation(len(CASES))]
    sends, views = _run(CASES, stride, max_buffers, capacity=7, ids=ids, first_slot=2)
    for c, (transfer, B) in enumerate(CASES):
        assert sends[c] == _one_send_at_a_time(transfer, B), (transfer, B)
    last = views[-1]
    assert (last.entries["finished"] == 1).all() and set(last.codes.tolist()) == {2}
    assert np.array_equal(last.entries["bytes_sent"], last.entries["transfer_bytes"])
    assert last.counters["bytes_sent"] == sum(t for t, _ in CASES)
    assert last.counters["buffers_sent"] == sum(len(s) for s in sends) == int(last.entries["buffers_sent"].sum())
    assert last.counters["connections_finished"] == len(CASES)
    assert any(3 in v.codes.tolist() for v in views) and all(v.tick["buffers"] <= 7 for v in views)
    for v in views:
        took = v.taken > 0
        assert v.tick["connections_sent"] == int(took.sum())
        assert v.tick["bytes"] == int(v.descs["length"][: v.tick["buffers"]].sum())
        assert v.tick["connections_no_room"] == v.codes.tolist().count(3)
        assert v.tick["connections_skipped"] == v.codes.tolist().count(2) + v.codes.tolist().count(4)
        assert v.tick["connections_finished"] == v.codes.tolist().count(1)


def test_model_skips_and_capacity():
    """Codes and slots by hand: an id beyond the table, B above the stride, a finished entry, a partial take and
    NO_ROOM behind it; nothing outside the written bytes changes."""
    entries = wl.tcp_sender_entries([(5000, 1000), (5000, 2000), (999, 1000), (5000, 1000), (100, 10)])
    entries["finished"][3] = 1
    stride, first_slot, capacity = 1008, 3, 6
    arena = np.full((first_slot + capacity + 2) * stride, 0xA5, dtype=np.uint8)
    prior = np.zeros(capacity, dtype=DESC_DTYPE)
    prior["length"] = 77
    v = wl.tcp_sender_view(entries, stride, arena, first_slot, capacity, [7, 0, 1, 3, 2, 4, 0xFFFFFFFF], 4,
                           descs=prior)
    assert v.codes.tolist() == [4, 0, 4, 2, 1, 0, 4]
    assert v.prefix.tolist() == [0, 0, 4, 4, 4, 5, 9] and v.taken.tolist() == [0, 4, 0, 0, 1, 1, 0]
    assert v.tick == {"bytes": 4000 + 999 + 10, "buffers": 6, "connections_sent": 3, "connections_finished": 1,
                      "connections_no_room": 0, "connections_skipped": 4}
    assert v.descs["conn_index"].tolist() == [0, 0, 0, 0, 2, 4]
    assert v.descs["byte_offset"].tolist() == [(3 + g) * 1008 for g in range(6)]
    assert v.descs["expected_pattern_offset"].tolist() == [0, 1000, 2000, 3000, 0, 0]
    rows = v.arena.reshape(-1, stride)
    assert (rows[:3] == 0xA5).all() and (rows[9:] == 0xA5).all() and (rows[3:7, 1000:] == 0xA5).all()
    assert (rows[7, 999:] == 0xA5).all() and (rows[8, 10:] == 0xA5).all()
    # the next tick: connection 4 wants 4 of the 2 slots left behind connection 0's one
    v2 = wl.tcp_sender_view(v.entries, stride, arena, first_slot, 3, [0, 4, 2, 1], 4)
    assert v2.codes.tolist() == [1, 0, 2, 4] and v2.taken.tolist() == [1, 2, 0, 0]
    v3 = wl.tcp_sender_view(v.entries, stride, arena, first_slot, 1, [0, 4], 4)
    assert v3.codes.tolist() == [1, 3] and v3.tick["connections_no_room"] == 1
    v0 = wl.tcp_sender_view(v.entries, stride, arena, first_slot, 0, [0, 4], 4, descs=prior)
    assert v0.codes.tolist() == [3, 3] and np.array_equal(v0.arena, arena) and np.array_equal(v0.descs, prior)
    assert np.array_equal(v0.entries, v.entries)


@pytest.mark.parametrize("transfer,B", CASES)
def test_model_against_the_pattern_mirror(transfer, B):
    """A sending ctsIoPattern (a Pull server, no engine): its send tasks' buffer_length and buffer_offset are the
    model's length and expected_pattern_offset, one after the other."""
    shared_buffer_attach(_SENDER)
    p = IoPattern.MakeIoPattern(PatternConfig(io_pattern=A.PATTERN_PULL, listening=True, verify_buffers=True,
                                              pre_post_recvs=1, pre_post_sends=1, buffer_size=B,
                                              transfer_size=transfer), None)
    try:
        t = p.InitiateIo()
        assert t.io_action == A.TASK_SEND and t.buffer_length == A.CONNECTION_ID_LENGTH
        assert p.CompleteIo(t, A.CONNECTION_ID_LENGTH, 0) == A.IO_CONTINUE
        stride = B + (-B) % 16
        sends, views = _run([(transfer, B)], stride, max_buffers=3, capacity=5)
        base = IoPattern.AccessSharedBuffer()
        for length, offset in sends[0]:
            t = p.InitiateIo()
            assert (t.io_action, t.buffer_length, t.buffer_offset) == (A.TASK_SEND, length, offset)
            assert t.buffer == base
            assert p.CompleteIo(t, length, 0) == A.IO_CONTINUE
        assert p.stats()["bytes_sent"] == transfer == int(views[-1].entries["bytes_sent"][0])
        assert p.stats()["send_pattern_offset"] == transfer % 65536
    finally:
        p.close()


def test_payload_bytes_against_the_oracle():
    """Every written slot holds g_senderSharedBuffer[offset .. offset + length), nothing else is touched, and the
    oracle's fill over the model's descriptors writes the same arena."""
    settings = [(200_000, 65531), (5 * 8193 - 7, 8193), (33 * 20 + 1, 33), (70_001 * 2 + 5, 70_001), (1, 9)]
    stride, first_slot, capacity = 70_016, 1, 9
    S = oracle.sender_buffer(70_001)
    entries = wl.tcp_sender_entries(settings)
    for tick in range(4):
        arena = np.full((first_slot + capacity + 1) * stride, 0xA5, dtype=np.uint8)
        v = wl.tcp_sender_view(entries, stride, arena, first_slot, capacity, [3, 0, 4, 2, 1], 2)
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


def test_model_64_bit_sums():
    for start, B in [((1 << 32) - 3 * 1000, 1000), ((1 << 53) - 33, 33), ((1 << 63) + 5, 65531)]:
        entries = wl.tcp_sender_entries([(start + 10 * B + 1, B)])
        entries["bytes_sent"][0] = start
        arena = np.zeros(8 * 65536, dtype=np.uint8)
        v = wl.tcp_sender_view(entries, 65536, arena, 0, 8, [0], 6)
        assert v.descs["length"][:6].tolist() == [B] * 6
        assert v.descs["expected_pattern_offset"][:6].tolist() == [(start + j * B) % 65536 for j in range(6)]
        assert int(v.entries["bytes_sent"][0]) == start + 6 * B and v.codes.tolist() == [0]
        v = wl.tcp_sender_view(v.entries, 65536, arena, 0, 8, [0], 6)
        assert v.descs["length"][:5].tolist() == [B] * 4 + [1] and v.codes.tolist() == [1]
        assert int(v.entries["bytes_sent"][0]) == start + 10 * B + 1


def test_sent_view_of_a_counter_block():
    """distributed.fold_counters with SENT_FIELDS over a block as the tick leaves it (one process; the all-reduce
    over ranks is the six-word sum of the other views)."""
    import torch

    block = torch.zeros(64 * D.COUNTER_SLOTS, dtype=torch.int64)
    block.view(-1, D.COUNTER_SLOTS)[3, :3] = torch.tensor([1 << 40, 7, 2])
    block.view(-1, D.COUNTER_SLOTS)[63, :3] = torch.tensor([5, 1, 0])
    got = D.counters_dict(D.fold_counters(block, D.SENT_FIELDS), D.SENT_FIELDS)
    assert got == {"bytes_sent": (1 << 40) + 5, "buffers_sent": 8, "connections_finished": 2, "reserved0": 0,
                   "reserved1": 0, "reserved2": 0}
