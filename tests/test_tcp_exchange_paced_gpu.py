"""GPU: send pacing for every pattern on the device-resident path (cts_tcp_exchange_send_paced,
include/cts_tcp_exchange.h) against the model workload.tcp_paced_exchange_view, which is itself held against a client
and a server ctsIoPattern mirror and hand-worked sequences in tests/test_tcp_exchange_paced_cpu.py. The arena is
pre-filled with 0xA5 and every byte of it is compared, so stray writes show; entries, all 2 x n_conns pace entries,
codes, the whole 64-byte tick block, descriptors and the sent block are compared field by field after every tick. Every
comparison is exact.
"""
import numpy as np
import pytest
import torch

from ctstraffic_amd import tcp_exchange as X
from ctstraffic_amd import tcp_senders as T
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import (CONN_RESULT_DTYPE, DESC_DTYPE, TCP_EXCHANGE_DTYPE, TCP_EXCHANGE_DUPLEX,
                                  TCP_EXCHANGE_PACED_TICK_DTYPE, TCP_EXCHANGE_PULL, TCP_EXCHANGE_PUSH,
                                  TCP_EXCHANGE_PUSHPULL, TCP_SENDER_PACE_DTYPE, TCP_SENDER_TICK_DTYPE)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EMPTY = 0xFFFFFFFF
NO_DUE = (1 << 63) - 1
NO_TAIL = {"next_due_ms": NO_DUE, "connections_waiting": 0, "connections_pending": 0}
DATA_ERROR = W.STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN
PUSH, PULL, PUSHPULL, DUPLEX = TCP_EXCHANGE_PUSH, TCP_EXCHANGE_PULL, TCP_EXCHANGE_PUSHPULL, TCP_EXCHANGE_DUPLEX


def _ids(ids):
    return torch.from_numpy(np.asarray(list(ids), dtype=np.uint32).view(np.int32).copy()).to(DEV)


def _u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(DEV)


class Pair:
    """A device table with its pace table, and the model's state over the same entries and an arena of 0xA5."""

    def __init__(self, engine, settings, pace_settings, stride, capacity, start_ms=0, arena_slots=None,
                 max_listed=None, entries=None, pace=None):
        self.table = X.PacedExchangeTable(engine, settings, pace_settings, stride, capacity, start_ms=start_ms,
                                          arena_slots=arena_slots, fill=0xA5, max_listed=max_listed)
        assert np.array_equal(self.table.fresh, W.tcp_exchange_entries(settings))
        assert np.array_equal(self.table.fresh_pace, W.tcp_exchange_pace_entries(pace_settings, start_ms))
        if entries is not None:
            self.table.load(entries)
        if pace is not None:
            self.table.load_pace(pace)
        self.entries = np.array(self.table.fresh if entries is None else entries, copy=True)
        self.pace = np.array(self.table.fresh_pace if pace is None else pace, copy=True)
        self.arena = np.full(self.table.arena.numel(), 0xA5, dtype=np.uint8)
        self.descs = np.zeros(capacity, dtype=DESC_DTYPE)
        self.counters = None
        self.stride, self.capacity = stride, capacity
        self.view = None

    def model(self, ids, max_buffers, now, first_slot=0, capacity=None):
        cap = self.capacity if capacity is None else capacity
        v = W.tcp_paced_exchange_view(self.entries, self.pace, now, self.stride, self.arena, first_slot, cap, ids,
                                      max_buffers, descs=self.descs[:cap], counters=self.counters)
        self.entries, self.pace, self.arena, self.counters, self.view = v.entries, v.pace, v.arena, v.counters, v
        self.descs[: len(v.descs)] = v.descs
        return v

    def same(self, n_listed, where=""):
        torch.cuda.synchronize()
        entries, codes, tick = self.table.read()
        for f in TCP_EXCHANGE_DTYPE.names:
            assert np.array_equal(entries[f], self.entries[f]), (where, f)
        pace = self.table.read_pace()
        for f in TCP_SENDER_PACE_DTYPE.names:
            assert np.array_equal(pace[f], self.pace[f]), (where, f)
        assert np.array_equal(codes[:n_listed], self.view.codes), where
        for f in W.TCP_SENDER_TICK_FIELDS:
            assert int(tick[f]) == self.view.tick[f], (where, f)
        assert tick["bytes_dir"].tolist() == self.view.tick["bytes_dir"], where
        assert int(tick["reserved"]) == 0
        for f in W.TCP_SENDER_PACED_TAIL_FIELDS:
            assert int(tick[f]) == self.view.tail[f], (where, f)
        arena, descs = self.table.read_arena()
        for f in DESC_DTYPE.names:
            assert np.array_equal(descs[f], self.descs[f]), (where, f)
        assert np.array_equal(arena, self.arena), where
        assert self.table.read_sent() == self.counters, where

    def tick(self, ids, max_buffers, now, first_slot=0, capacity=None, where=""):
        self.table.send(_ids(ids), max_buffers, now, first_slot=first_slot, capacity=capacity)
        v = self.model(ids, max_buffers, now, first_slot=first_slot, capacity=capacity)
        self.same(len(ids), where)
        return v


# per-connection pace settings (client, server): none, client only, server only, both with different periods, bursts
def _pace_kinds(B):
    rate = dict(bytes_per_second=150 * B, period_ms=10)     # 1.5 buffers per 10 ms quantum
    slow = dict(bytes_per_second=40 * B, period_ms=25)      # one buffer per 25 ms quantum
    burst = dict(burst_count=2, burst_delay_ms=7)           # two sends, then 7 ms
    return [({}, {}), (rate, {}), ({}, rate), (rate, slow), (burst, dict(burst_count=3, burst_delay_ms=4))]


def _mixed_table(n_conns, B, seed):
    """All four patterns against all five pace kinds (c % 4 and c % 5), transfers of 1 to 20 buffers, PushPull
    segments that are not multiples of B."""
    rng = np.random.default_rng(seed)
    kinds = _pace_kinds(B)
    settings, pace = [], []
    for c in range(n_conns):
        k = 1 + int(rng.integers(0, 20))
        T_ = int(rng.integers((k - 1) * B + 1, k * B + 1))
        settings.append((c % 4, T_, B, 2 * B + B // 2, B + B // 2))
        pace.append(kinds[c % 5])
    return settings, pace


_SETTINGS_600, _PACE_600 = _mixed_table(600, 1000, 15)


# ---- 1: the list -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_buffers", [1, 3, 8])
@pytest.mark.parametrize("n_listed", [1, 63, 64, 65, 255, 256, 257, 513])
def test_shuffled_lists(engine, n_listed, max_buffers):
    """A shuffled list out of a table of 600 (B = 1000 under stride 1008) mixing the four patterns and the five pace
    kinds, some entries finished, one malformed, two ids beyond the table; four ticks whose clock stands, moves inside
    a quantum and skips several. 63/64/65 listed: a wave edge; 255/256/257: a tile edge; 513: three tiles."""
    settings = _SETTINGS_600
    entries = W.tcp_exchange_entries(settings)
    entries["finished"][::7] = 1
    entries["pull_bytes"][22] = 0  # a malformed PushPull entry
    rng = np.random.default_rng(n_listed)
    ids = [int(x) for x in rng.permutation(len(settings))][:n_listed]
    if n_listed >= 63:
        ids[5], ids[n_listed // 2] = 600, 0xFFFFFFFF
        if 22 not in ids:
            ids[9] = 22
    capacity = max_buffers * n_listed - (n_listed > 1)  # the last running connection may be cut
    p = Pair(engine, settings, _PACE_600, 1008, capacity, start_ms=100, max_listed=n_listed, entries=entries)
    seen, pending = set(), 0
    for t, now in enumerate([100, 100, 104, 146]):
        v = p.tick(ids, max_buffers, now, where="tick %d" % t)
        seen |= set(v.codes.tolist())
        pending += v.tail["connections_pending"]
    if n_listed >= 63:
        assert {0, 2, 4, 5} <= seen and pending > 0
        assert set(v.direction.tolist()) == {0, 1} or max_buffers == 1


@pytest.mark.parametrize("n_listed,max_buffers", [(1, 3), (65, 3), (257, 8)])
def test_64k_buffers(engine, n_listed, max_buffers):
    """B = 65536 under stride 65536: the fill takes its piece-order path. The capacity holds 40 buffers, so most of a
    long list finds no room."""
    settings, pace = _mixed_table(300, 65536, 64)
    ids = [int(x) for x in np.random.default_rng(n_listed).permutation(300)][:n_listed]
    capacity = min(40, max_buffers * n_listed)
    p = Pair(engine, settings, pace, 65536, capacity, start_ms=0, max_listed=n_listed)
    for t, now in enumerate([0, 10, 35]):
        v = p.tick(ids, max_buffers, now, where="tick %d" % t)
    assert v.tick["buffers"] > 0


# ---- 2: the hand-worked sequences --------------------------------------------------------------------------------
PP = (PUSHPULL, 1 << 30, 1000, 2500, 1500)


@pytest.mark.parametrize("setting,pace,times,counts,dues", [
    (PP, (dict(bytes_per_second=30000, period_ms=100), {}), [0, 50, 100], [6, 0, 5], [100, 100, 200]),
    (PP, ({}, dict(bytes_per_second=10000, period_ms=100)), [0, 99, 100], [4, 0, 5], [100, 100, 200]),
    (PP, (dict(bytes_per_second=30000, period_ms=100), dict(bytes_per_second=25000, period_ms=40)), [0, 40, 100],
     [4, 2, 5], [40, 100, 200]),
    (PP, (dict(burst_count=2, burst_delay_ms=30), {}), [0, 30], [1, 4], [30, 60]),
    ((DUPLEX, 10000, 1000), (dict(bytes_per_second=20000, period_ms=100), {}), [0, 100, 200], [4, 4, 2],
     [100, 200, NO_DUE]),
    ((PULL, 10000, 1000), ({}, dict(burst_count=3, burst_delay_ms=7)), [0, 7, 14], [2, 3, 3], [7, 14, 21]),
])
def test_hand_worked_sequences(engine, setting, pace, times, counts, dues):
    """The sequences of tests/test_tcp_exchange_paced_cpu.py, where they are worked out: per tick the buffers that
    leave and the time of the next deferred send."""
    p = Pair(engine, [setting], [pace], 1008, 8)
    for k, now in enumerate(times):
        v = p.tick([0], 8, now, where="tick %d" % k)
        assert v.tick["buffers"] == counts[k] and v.tail["next_due_ms"] == dues[k], k


# ---- 3: the host timer's number ----------------------------------------------------------------------------------
def test_ticks_driven_by_next_due_ms_read_back(engine):
    """Consecutive ticks, each at the next_due_ms the device's tick block of the previous one holds: the one number the
    host timer needs. Every connection is paced; a tick in which every connection stopped at max_buffers leaves no due
    time, and the next one follows at once."""
    kinds = _pace_kinds(1000)[1:]
    settings = [(c % 4, 7000 + 501 * c, 1000, 2500, 1500) for c in range(40)]
    pace = [kinds[c % 4] for c in range(40)]
    p = Pair(engine, settings, pace, 1008, 40 * 3, start_ms=50)
    now, ticks, timed = 50, 0, 0
    while not (p.entries["finished"] == 1).all():
        v = p.tick(range(40), 3, now, where="tick %d at %d" % (ticks, now))
        ticks += 1
        due = int(p.table.read()[2]["next_due_ms"])
        assert due == v.tail["next_due_ms"] and ticks < 200
        if due != NO_DUE:
            assert due > now
            now, timed = due, timed + 1
    assert due == NO_DUE and timed > 10


# ---- 4: capacity -------------------------------------------------------------------------------------------------
def test_capacity_cut_in_the_middle_of_a_segment_flip(engine):
    """Client burst 4 / 9 ms, server burst 3 / 5 ms (tests/test_tcp_exchange_paced_cpu.py works it out): connection 1
    is cut to four of its five buffers, three pushes and the first pull, and its entries are those of four steps;
    connection 2 keeps all three entries; connection 3 waits whatever the room. Then capacity 0."""
    pace = [(dict(burst_count=4, burst_delay_ms=9), dict(burst_count=3, burst_delay_ms=5))] * 3 + \
           [(dict(burst_count=1, burst_delay_ms=9), {})]
    p = Pair(engine, [PP] * 4, pace, 1008, 9, arena_slots=11)
    before = p.pace.copy()
    v = p.tick([0, 1, 2, 3], 8, 0, where="cut")
    assert v.wanted.tolist() == [5, 5, 5, 0] and v.taken.tolist() == [5, 4, 0, 0] and v.codes.tolist() == [0, 0, 3, 5]
    assert p.pace["burst_left"].tolist() == [0, 1, 4, 0, 1, 2, 3, 0]
    assert p.pace["pending"].tolist() == [1, 0, 0, 1] + [0] * 4
    assert np.array_equal(p.pace[2], before[2]) and np.array_equal(p.pace[6], before[6])
    assert p.entries["bytes_sent"].tolist()[:3] == [[2500, 1500], [2500, 1000], [0, 0]]
    assert v.tail == {"next_due_ms": 9, "connections_waiting": 1, "connections_pending": 2}
    v = p.tick([0, 1, 2, 3], 8, 5, capacity=0, where="capacity 0")
    assert v.codes.tolist() == [5, 3, 3, 5] and v.tick["buffers"] == 0
    assert v.tail == {"next_due_ms": 9, "connections_waiting": 2, "connections_pending": 2}
    v = p.tick([3, 1], 8, 9, first_slot=2, where="the rest of the cycle")
    assert v.taken.tolist() == [1, 1] and v.descs["conn_index"][:2].tolist() == [3, 1 + 4]
    # a cut inside a rate-limited quantum, every buffer a flip: 2 000 B per quantum let push pull push pull out and
    # hold the third push (the client carries its 1000, the server's quantum is full); connection 1 takes one push
    rate = dict(bytes_per_second=200_000, period_ms=10)
    settings = [(PUSHPULL, 1 << 20, 1000, 1000, 1000)] * 3
    p = Pair(engine, settings, [(rate, rate)] * 3, 1008, 5)
    v = p.tick([2, 1, 0], 8, 0, where="rate cut")
    assert v.wanted.tolist() == [4, 4, 4] and v.taken.tolist() == [4, 1, 0] and v.codes.tolist() == [0, 0, 3]
    assert p.pace["bytes_this_quantum"].tolist() == [0, 1000, 1000, 0, 0, 2000]
    assert p.pace["pending"].tolist() == [0, 0, 1, 0, 0, 0]


# ---- 5: the two equalities on the device -------------------------------------------------------------------------
@pytest.mark.parametrize("stride,B", [(65536, 65536), (1008, 1000), (48, 33)])
def test_unpaced_table_equals_the_plain_exchange_tick(engine, stride, B):
    settings = [(c % 4, 5 * B + 3 * c + 1, B, 2 * B + 7, B - 1) for c in range(23)]
    capacity = 23 * 3 - 4  # the last connections are cut and left without room
    plain = X.ExchangeTable(engine, settings, stride, capacity, fill=0xA5)
    p = Pair(engine, settings, [({}, {})] * 23, stride, capacity, start_ms=7)
    order = [int(x) for x in np.random.default_rng(7).permutation(23)]
    for t in range(2):
        plain.send(_ids(order), 3)
        v = p.tick(order, 3, 7 + 1000 * t, where="tick %d" % t)
        assert torch.equal(plain.arena, p.table.arena) and torch.equal(plain.descs, p.table.descs)
        assert torch.equal(plain.entries, p.table.entries) and torch.equal(plain.codes, p.table.codes)
        assert torch.equal(plain.tick, p.table.tick[:6]) and torch.equal(plain.sent, p.table.sent)
        assert v.tail == NO_TAIL and 3 in v.codes.tolist()
    assert np.array_equal(p.table.read_pace(), p.table.fresh_pace)
    # max_buffers = 2^31 is not a walk
    p.tick(order, 1 << 31, 5000, where="2^31")


@pytest.mark.parametrize("stride,B", [(65536, 65531), (1488, 1472)])
def test_push_table_equals_the_paced_senders_tick(engine, stride, B):
    """The same transfers and pace settings through cts_tcp_senders_send_paced and, as Push entries with the pace
    entries [0, n_conns), through cts_tcp_exchange_send_paced: the arena, the descriptors, the codes, the pace entries,
    the tick's first 32 bytes, its tail and the sent block are the same bytes. The entries [n_conns, 2 n_conns) hold
    junk and stay as they are."""
    n = 23
    plain = [(5 * B + 3 * c + 1, B) for c in range(n)]
    kinds = [{}, dict(bytes_per_second=150 * B, period_ms=10), dict(burst_count=2, burst_delay_ms=7)]
    pace = [kinds[c % 3] for c in range(n)]
    capacity = 30
    s = T.PacedSenderTable(engine, plain, pace, stride, capacity, start_ms=3, fill=0xA5, max_listed=25)
    x = X.PacedExchangeTable(engine, [(PUSH, t, b) for t, b in plain], [(q, {}) for q in pace], stride, capacity,
                             start_ms=3, fill=0xA5, max_listed=25)
    junk = x.fresh_pace.copy()
    junk["pending"][n:], junk["due_ms"][n:], junk["bytes_per_quantum"][n:] = 1, 1 << 40, 5
    x.load_pace(junk)
    ids = _ids([int(i) for i in np.random.default_rng(7).permutation(n)] + [n, 0xFFFFFFFF])
    codes = set()
    for t, now in enumerate([3, 3, 8, 13, 40]):
        s.send(ids, 3, now)
        x.send(ids, 3, now)
        torch.cuda.synchronize()
        assert torch.equal(s.arena, x.arena) and torch.equal(s.descs, x.descs) and torch.equal(s.codes, x.codes), t
        assert torch.equal(s.tick[:4], x.tick[:4]) and torch.equal(s.tick[4:6], x.tick[6:8]), t
        assert torch.equal(s.sent, x.sent), t
        xq = x.read_pace()
        assert np.array_equal(s.read_pace(), xq[:n]) and np.array_equal(xq[n:], junk[n:]), t
        a, b = s.read()[0], x.read()[0]
        assert np.array_equal(a["bytes_sent"], b["bytes_sent"][:, 0]) and not b["bytes_sent"][:, 1].any()
        assert np.array_equal(a["buffers_sent"], b["buffers_sent"]) and np.array_equal(a["finished"], b["finished"])
        codes |= set(s.read()[1][:25].tolist())
    assert {0, 3, 4, 5} <= codes


# ---- 6: null outputs ---------------------------------------------------------------------------------------------
def test_null_outputs(engine):
    """Each optional output null in turn: the others are written as ever."""
    settings = [(PUSHPULL, 3000 * 9, 1400, 3000, 1500), (DUPLEX, 100 * 9, 60), (PULL, 5000, 1000)]
    pace = [(dict(burst_count=2, burst_delay_ms=5), {}), ({}, {}), ({}, dict(bytes_per_second=10 ** 9))]
    p = Pair(engine, settings, pace, 1408, 8, arena_slots=12)
    v = p.tick([1, 2], 2, 0, where="nothing pending")
    assert v.tail["next_due_ms"] == NO_DUE and v.tick["buffers"] == 4
    table, ids = p.table, _ids([0, 1, 2])
    for t, null in enumerate(["codes", "tick", "sent"]):
        before = {k: getattr(table, k).clone() for k in ("codes", "tick", "sent")}
        out = dict(codes=table.codes, tick=table.tick, sent_counters=table.sent)
        out["sent_counters" if null == "sent" else null] = None
        X.exchange_send_paced(engine, table.arena, 1408, 4 * (t % 2), 8, ids, 2, table.entries, table.pace, 3, 5 * t,
                              table.descs, table.scratch, **out)
        v = p.model([0, 1, 2], 2, 5 * t, first_slot=4 * (t % 2))
        torch.cuda.synchronize()
        assert torch.equal(getattr(table, null), before[null]), null
        entries, codes, tick = table.read()
        arena, descs = table.read_arena()
        assert np.array_equal(entries, p.entries) and np.array_equal(arena, p.arena), null
        assert np.array_equal(descs, p.descs) and np.array_equal(table.read_pace(), p.pace), null
        if null != "codes":
            assert np.array_equal(codes[:3], v.codes)
        if null != "tick":
            assert all(int(tick[f]) == v.tick[f] for f in W.TCP_SENDER_TICK_FIELDS)
            assert tick["bytes_dir"].tolist() == v.tick["bytes_dir"]
            assert all(int(tick[f]) == v.tail[f] for f in W.TCP_SENDER_PACED_TAIL_FIELDS)
        if null == "sent":
            p.counters["bytes_sent"] -= v.tick["bytes"]
            p.counters["buffers_sent"] -= v.tick["buffers"]
            p.counters["connections_finished"] -= v.tick["connections_finished"]
        assert table.read_sent() == p.counters, null
        assert v.tick["buffers"] > 0


# ---- 7: the loop the feature exists for --------------------------------------------------------------------------
def chain_settings():
    """13 connections of the four patterns with transfers of 3 to 39 buffers; every connection paced on one side or
    both, at rates that end the longest in about 40 quanta."""
    B = 1000
    settings = [(c % 4, 3000 * (c + 1) + 17 * c + 1, B, 2500, 1001) for c in range(13)]
    rate = dict(bytes_per_second=300_000, period_ms=10)   # three buffers per 10 ms quantum
    kinds = [(rate, {}), ({}, rate), (rate, rate), (dict(burst_count=3, burst_delay_ms=10), rate),
             (rate, dict(burst_count=2, burst_delay_ms=10))]
    return settings, [kinds[c % 5] for c in range(13)]


def _loop(engine, corrupt=None):
    """Per tick paced send -> verify_at -> accounting over the tick's own descriptors and 2 x n_conns receivers, all on
    one stream with nothing read back: the host's clock is the model's next_due_ms. Then the close of every receiver
    against cts_tcp_exchange_direction_bytes. corrupt: (tick, tick-local slot) whose first byte is flipped between
    the tick and the verify. The device's tick blocks are kept (device copies) and compared at the end."""
    stride, max_buffers, start = 1008, 3, 1000
    settings, pace_settings = chain_settings()
    n_conns = len(settings)
    capacity = n_conns * max_buffers
    table = X.PacedExchangeTable(engine, settings, pace_settings, stride, capacity, start_ms=start, fill=0xA5)
    n_recv = table.n_receivers
    ids = list(range(n_conns))
    dev_ids = _ids(ids)
    cff = torch.full((n_recv,), -1, dtype=torch.int32, device=DEV)
    state, ref, ctr, block = (engine.new_conn_state(n_recv), engine.new_counters(), engine.new_counters(),
                              engine.new_counters())
    results = engine.new_conn_results(n_recv)
    entries = W.tcp_exchange_entries(settings)
    pace = W.tcp_exchange_pace_entries(pace_settings, start)
    arena = np.zeros(capacity * stride, dtype=np.uint8)
    base, now, first_fail, recv_until, dev_ticks, model_ticks = 0, start, {}, {}, [], []
    while int(entries["finished"].sum()) < n_conns:
        assert len(model_ticks) < 60
        v = W.tcp_paced_exchange_view(entries, pace, now, stride, arena, 0, capacity, ids, max_buffers)
        entries, pace, n = v.entries, v.pace, v.tick["buffers"]
        table.send(dev_ids, max_buffers, now)
        dev_ticks.append(table.tick.clone())
        model_ticks.append(v)
        if corrupt is not None and corrupt[0] == len(model_ticks) - 1:
            g = corrupt[1]
            table.arena[g * stride] ^= 0xFF
            first_fail[int(v.descs["conn_index"][g])] = base + g
        if n:
            descs = table.descs_of(n)
            engine.verify(table.arena, descs, max_length_hint=stride, counters=ctr, conn_first_fail=cff,
                          base_index=base)
            engine.refview_conns(table.arena.numel(), descs, ref, state, base_index=base, conn_first_fail=cff)
        for g in range(n):  # what each receiver has received up to and including its first failing buffer
            r = int(v.descs["conn_index"][g])
            if r not in first_fail or base + g <= first_fail[r]:
                recv_until[r] = recv_until.get(r, 0) + int(v.descs["length"][g])
        base += n
        if v.tail["next_due_ms"] != NO_DUE:  # the one host timer: sleep until the next deferred send
            assert v.tail["next_due_ms"] > now
            now = v.tail["next_due_ms"]
    expected = table.expected_bytes()
    engine.conns_close(_ids(range(n_recv)), _u64(expected), cff, state, block, results=results)
    torch.cuda.synchronize()
    res = results.cpu().numpy().view(CONN_RESULT_DTYPE)
    dev_entries, _, _ = table.read()
    assert np.array_equal(dev_entries, entries) and np.array_equal(table.read_pace(), pace)
    # the device went through the model's ticks: every tick block is the model's, the due times included
    for k, (d, v) in enumerate(zip(dev_ticks, model_ticks)):
        tick = d.cpu().numpy().view(TCP_EXCHANGE_PACED_TICK_DTYPE)[0]
        assert all(int(tick[f]) == v.tick[f] for f in W.TCP_SENDER_TICK_FIELDS), k
        assert tick["bytes_dir"].tolist() == v.tick["bytes_dir"], k
        assert all(int(tick[f]) == v.tail[f] for f in W.TCP_SENDER_PACED_TAIL_FIELDS), k
    assert expected.tolist() == entries["bytes_sent"][:, 0].tolist() + entries["bytes_sent"][:, 1].tolist()
    sent = table.read_sent()
    assert sent["bytes_sent"] == int(expected.sum()) and sent["buffers_sent"] == base
    assert sent["connections_finished"] == n_conns
    return settings, expected, res, engine.read_counters_close(block), first_fail, recv_until, model_ticks


def test_paced_send_verify_account_close(engine):
    settings, expected, res, close, _, recv, ticks = _loop(engine)
    assert (res["status"] == 0).all() and (res["first_fail"] == EMPTY).all() and (res["flags"] == 0).all()
    assert res["bytes_recv"].tolist() == expected.tolist() == [recv.get(r, 0) for r in range(26)]
    assert close["connections_closed"] == close["successful"] == 26
    assert close["bytes_recv"] == int(expected.sum())
    assert 13 <= len(ticks) <= 45 and ticks[-1].tail["next_due_ms"] == NO_DUE
    assert sum(1 for v in ticks if v.tail["connections_pending"]) >= len(ticks) - 2
    assert any(v.tail["connections_waiting"] for v in ticks)


def test_paced_send_verify_account_close_with_a_corrupt_pull_buffer(engine):
    """Tick 1, slot 4: connection 2 (PushPull) sends its first pull buffer there, so the buffer is receiver 2 + 13's:
    that client receiver, and only it, closes as a data mismatch with the buffer's stream ordinal."""
    settings, expected, res, close, first_fail, recv, ticks = _loop(engine, corrupt=(1, 4))
    assert list(first_fail) == [2 + 13] and settings[2][0] == PUSHPULL
    for r in range(26):
        if r == 15:
            assert int(res["status"][r]) == DATA_ERROR and int(res["first_fail"][r]) == first_fail[r]
            assert int(res["bytes_recv"][r]) == recv[r] < int(expected[r])
        else:
            assert int(res["status"][r]) == 0 and int(res["first_fail"][r]) == EMPTY, r
            assert int(res["bytes_recv"][r]) == int(expected[r]), r
    assert int(res["conn_index"][15]) == 15 and int(res["bytes_recv"][2]) == int(expected[2]) > 0
    assert close["data_errors"] == 1 and close["successful"] == 25


def test_tick_block_prefix_is_the_plain_ticks(engine):
    """tcp_exchange_descs and the fill read the first 48 and 32 bytes of the 64-byte block: field for field they are
    the plain blocks'."""
    for f in TCP_SENDER_TICK_DTYPE.names:
        assert TCP_EXCHANGE_PACED_TICK_DTYPE.fields[f] == TCP_SENDER_TICK_DTYPE.fields[f]
    assert TCP_EXCHANGE_PACED_TICK_DTYPE.fields["bytes_dir"][1] == 32
