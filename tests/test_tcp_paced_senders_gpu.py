"""GPU: send pacing on the device-resident path (cts_tcp_senders_send_paced, include/cts_tcp_senders.h) against the
model workload.tcp_paced_sender_view, which is itself held against the ctsIoPattern mirror and hand-worked sequences
in tests/test_tcp_paced_senders_cpu.py. The arena is pre-filled with 0xA5 and every byte of it is compared, so stray
writes show; entries, pace entries, codes, the whole 48-byte tick block, descriptors and the sent block are compared
field by field after every tick. Every comparison is exact.
"""
import numpy as np
import pytest
import torch

from ctstraffic_amd import tcp_senders as T
from ctstraffic_amd import workload as W
from ctstraffic_amd._lib import CtsError
from ctstraffic_amd.types import (CONN_RESULT_DTYPE, DESC_DTYPE, TCP_SENDER_DTYPE, TCP_SENDER_PACE_DTYPE,
                                  TCP_SENDER_PACED_TICK_DTYPE)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EMPTY = 0xFFFFFFFF
NO_DUE = (1 << 63) - 1
DATA_ERROR = W.STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN


def _ids(ids):
    return torch.from_numpy(np.asarray(list(ids), dtype=np.uint32).view(np.int32).copy()).to(DEV)


def _u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(DEV)


class Pair:
    """A device table with its pace table, and the model's state over the same entries and an arena of 0xA5."""

    def __init__(self, engine, settings, pace_settings, stride, capacity, start_ms=0, arena_slots=None,
                 max_listed=None, entries=None, pace=None):
        self.table = T.PacedSenderTable(engine, settings, pace_settings, stride, capacity, start_ms=start_ms,
                                        arena_slots=arena_slots, fill=0xA5, max_listed=max_listed)
        assert np.array_equal(self.table.fresh, W.tcp_sender_entries(settings))
        assert np.array_equal(self.table.fresh_pace, W.tcp_sender_pace_entries(pace_settings, start_ms))
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
        capacity = self.capacity if capacity is None else capacity
        v = W.tcp_paced_sender_view(self.entries, self.pace, now, self.stride, self.arena, first_slot, capacity, ids,
                                    max_buffers, descs=self.descs[:capacity], counters=self.counters)
        self.entries, self.pace, self.arena, self.counters, self.view = v.entries, v.pace, v.arena, v.counters, v
        self.descs[: len(v.descs)] = v.descs
        return v

    def same(self, n_listed, where=""):
        torch.cuda.synchronize()
        entries, codes, tick = self.table.read()
        for f in TCP_SENDER_DTYPE.names:
            assert np.array_equal(entries[f], self.entries[f]), (where, f)
        pace = self.table.read_pace()
        for f in TCP_SENDER_PACE_DTYPE.names:
            assert np.array_equal(pace[f], self.pace[f]), (where, f)
        assert np.array_equal(codes[:n_listed], self.view.codes), where
        for f in W.TCP_SENDER_TICK_FIELDS:
            assert int(tick[f]) == self.view.tick[f], (where, f)
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


# ---- 1: unpaced entries are the plain tick ---------------------------------------------------------------------
@pytest.mark.parametrize("stride,B", [(65536, 65531), (16384, 9000), (1488, 1472), (48, 33)])
def test_unpaced_table_equals_the_plain_tick(engine, stride, B):
    settings = [(5 * B + 3 * c + 1, B) for c in range(23)]
    capacity = 23 * 3 - 4  # the last connections are cut and left without room
    plain = T.SenderTable(engine, settings, stride, capacity, fill=0xA5)
    p = Pair(engine, settings, [{}] * 23, stride, capacity, start_ms=7)
    order = [int(x) for x in np.random.default_rng(7).permutation(23)]
    for t in range(2):
        plain.send(_ids(order), 3)
        v = p.tick(order, 3, 7 + 1000 * t, where="tick %d" % t)
        assert torch.equal(plain.arena, p.table.arena) and torch.equal(plain.descs, p.table.descs)
        assert torch.equal(plain.senders, p.table.senders) and torch.equal(plain.codes, p.table.codes)
        assert torch.equal(plain.tick, p.table.tick[:4]) and torch.equal(plain.sent, p.table.sent)
        assert v.tail == {"next_due_ms": NO_DUE, "connections_waiting": 0, "connections_pending": 0}
        assert 3 in v.codes.tolist()
    assert np.array_equal(p.table.read_pace(), p.table.fresh_pace)


# ---- 2: the hand-worked sequences ------------------------------------------------------------------------------
@pytest.mark.parametrize("pace,start,B,max_buffers,times,counts,dues", [
    (dict(bytes_per_second=655360, period_ms=100), 5000, 65536, 8,
     [5000, 5000, 5050, 5100, 5100, 5350, 5350, 5400], [1, 0, 0, 1, 0, 2, 0, 1],
     [5100, 5100, 5100, 5200, 5200, 5400, 5400, 5500]),
    (dict(burst_count=3, burst_delay_ms=50), 0, 1000, 8, [0, 10, 50, 50, 100, 1000], [2, 0, 3, 0, 3, 3],
     [50, 50, 100, 100, 150, 1050]),
    (dict(bytes_per_second=250_000, period_ms=10), 0, 1000, 3, list(range(0, 101, 5)), [3, 0, 2, 0] * 5 + [3], None),
])
def test_hand_worked_sequences(engine, pace, start, B, max_buffers, times, counts, dues):
    p = Pair(engine, [(1 << 40, B)], [pace], B + (-B) % 16, 8, start_ms=start)
    got, got_due = [], []
    for k, now in enumerate(times):
        v = p.tick([0], max_buffers, now, where="tick %d" % k)
        got.append(v.tick["buffers"])
        got_due.append(int(p.pace["due_ms"][0]))
    assert got == counts and sum(got) == int(p.entries["buffers_sent"][0])
    assert dues is None or got_due == dues


# ---- 3: the list -----------------------------------------------------------------------------------------------
def _table_1500():
    rng = np.random.default_rng(15)
    settings, pace = [], []
    for c in range(1500):
        B = int(rng.integers(1, 129))
        k = 1 + c % 7
        settings.append((int(rng.integers((k - 1) * B + 1, k * B + 1)), B))
        # unpaced; 1.5 buffers per 10 ms quantum; two sends, then 7 ms
        pace.append([{}, dict(bytes_per_second=150 * B, period_ms=10), dict(burst_count=2, burst_delay_ms=7)][c % 3])
    settings[11] = (1000, 200)   # B above the stride of 128
    settings[700] = (5000, 129)
    return settings, pace


_SETTINGS_1500, _PACE_1500 = _table_1500()


@pytest.mark.parametrize("max_buffers", [1, 3])
@pytest.mark.parametrize("n_listed", [1, 255, 256, 257, 1100])
def test_shuffled_lists(engine, n_listed, max_buffers):
    """A shuffled list out of a table of 1 500 with unpaced, rate-limited and burst connections, some already
    finished, two ids beyond the table, two with B above the stride; five ticks whose clock stands, moves inside a
    quantum and skips several."""
    settings = _SETTINGS_1500
    entries = W.tcp_sender_entries(settings)
    entries["finished"][::7] = 1
    rng = np.random.default_rng(n_listed)
    ids = [int(x) for x in rng.permutation(len(settings)) if x not in (11, 700)][:n_listed]
    if n_listed >= 255:
        ids[5], ids[n_listed // 2], ids[9], ids[n_listed - 1] = 1500, 0xFFFFFFFF, 11, 700
    capacity = max_buffers * n_listed
    p = Pair(engine, settings, _PACE_1500, 128, capacity, start_ms=100, max_listed=n_listed, entries=entries)
    seen, pending = set(), 0
    for t, now in enumerate([100, 100, 104, 145, 146]):
        v = p.tick(ids, max_buffers, now, where="tick %d" % t)
        seen |= set(v.codes.tolist())
        pending += v.tail["connections_pending"]
    if n_listed >= 255:
        assert {0, 1, 2, 4, 5} <= seen and pending > 0


# ---- 4: capacity -----------------------------------------------------------------------------------------------
def test_capacity_cuts(engine):
    """A cut inside a burst moves the pace entry by the taken steps and creates no pending task; a connection with
    room for none keeps both entries; at capacity 0 a waiting connection is still code 5."""
    pace = [dict(burst_count=4, burst_delay_ms=9)] * 3 + [dict(burst_count=1, burst_delay_ms=9)]
    p = Pair(engine, [(100_000, 1000)] * 4, pace, 1008, 5, arena_slots=7)
    before = p.pace.copy()
    v = p.tick([0, 1, 2, 3], 8, 0, where="cut")
    assert v.wanted.tolist() == [3, 3, 3, 0] and v.taken.tolist() == [3, 2, 0, 0] and v.codes.tolist() == [0, 0, 3, 5]
    assert p.pace["burst_left"].tolist() == [0, 2, 4, 0] and p.pace["pending"].tolist() == [1, 0, 0, 1]
    assert np.array_equal(p.pace[2], before[2]) and int(p.entries["bytes_sent"][2]) == 0
    assert v.tail == {"next_due_ms": 9, "connections_waiting": 1, "connections_pending": 2}
    v = p.tick([0, 1, 2, 3], 8, 5, capacity=0, where="capacity 0")
    assert v.codes.tolist() == [5, 3, 3, 5] and v.tick["buffers"] == 0
    # a cut inside a rate-limited quantum: connection 1 takes 1 of the 2 its quantum lets out
    rate = dict(bytes_per_second=200_000, period_ms=10)
    p = Pair(engine, [(100_000, 1000)] * 3, [rate] * 3, 1008, 3)
    v = p.tick([2, 1, 0], 8, 0, where="rate cut")
    assert v.wanted.tolist() == [2, 2, 2] and v.taken.tolist() == [2, 1, 0] and v.codes.tolist() == [0, 0, 3]
    assert p.pace["bytes_this_quantum"].tolist() == [0, 1000, 1000] and p.pace["pending"].tolist() == [0, 0, 1]
    v = p.tick([0, 1, 2], 8, 3, where="rate cut, the rest")
    assert v.taken.tolist() == [2, 1, 0] and v.codes.tolist() == [0, 0, 5]


# ---- 5: one connection, a long loop ------------------------------------------------------------------------------
def test_one_connection_stopped_in_the_middle_of_700(engine):
    """max_buffers 700: a lane whose rate stops it at a buffer in the middle, next to an unpaced one."""
    settings = [(48 * 2000, 48), (33 * 5, 33)]
    pace = [dict(bytes_per_second=48 * 3000 + 200, period_ms=100), {}]
    p = Pair(engine, settings, pace, 48, 705)
    v = p.tick([0, 1], 700, 0, where="stopped")
    assert 100 < int(v.taken[0]) < 600 and int(v.taken[1]) == 5 and v.codes.tolist() == [0, 1]
    assert v.tail["connections_pending"] == 1
    v = p.tick([0], 700, v.tail["next_due_ms"], where="the next quantum")
    assert 100 < int(v.taken[0]) < 600


# ---- 6: wide values ------------------------------------------------------------------------------------------------
def test_wide_values(engine):
    """now_ms above 2^41, bytes_per_quantum above 2^32, bytes_sent across 2^32, a skip of more than 2^20 quanta."""
    B, T0 = 65531, 1 << 41
    settings = [((1 << 33) + 7, B), (1 << 50, B)]
    pace_settings = [dict(bytes_per_second=10 * ((1 << 33) + 5), period_ms=100),
                     dict(bytes_per_second=3 * B * 1000, period_ms=1)]
    entries = W.tcp_sender_entries(settings)
    entries["bytes_sent"][0], entries["buffers_sent"][0] = (1 << 32) - 3 * B, (1 << 32) - 2
    pace = W.tcp_sender_pace_entries(pace_settings, T0)
    assert int(pace["bytes_per_quantum"][0]) == (1 << 33) + 5
    pace["bytes_this_quantum"][0] = (1 << 33) + 5 - 4 * B  # four more buffers fill this quantum
    p = Pair(engine, settings, pace_settings, 65536, 16, start_ms=T0, entries=entries, pace=pace)
    taken = []
    for k, now in enumerate([T0, T0 + 1, T0 + 99, T0 + 100, T0 + (1 << 21) + 4, T0 + (1 << 21) + 4]):
        v = p.tick([0, 1], 6, now, where="tick %d" % k)
        taken.append(v.taken.tolist())
    assert taken[0] == [4, 3] and taken[1][0] == 0 and taken[3][0] == 6
    assert int(p.entries["bytes_sent"][0]) > 1 << 32 and int(p.entries["buffers_sent"][0]) > 1 << 32
    assert int(p.pace["quantum_start_ms"][1]) > T0 + (1 << 21)


# ---- 7: next_due_ms ------------------------------------------------------------------------------------------------
def test_next_due_is_the_minimum_over_the_tiles(engine):
    """600 listed connections in three tiles, each left with a pending send; the earliest is the last one listed."""
    n = 600
    pace = [dict(burst_count=1, burst_delay_ms=5000 - c) for c in range(n)]
    p = Pair(engine, [(10_000, 100)] * n, pace, 112, 8)
    v = p.tick(range(n), 2, 10, where="all pending")
    assert v.tail == {"next_due_ms": 10 + 5000 - 599, "connections_waiting": n, "connections_pending": n}
    v = p.tick(range(n), 2, v.tail["next_due_ms"], where="the first goes out")
    assert v.tick["buffers"] == 1 and int(v.descs["conn_index"][0]) == 599
    assert v.tail == {"next_due_ms": 10 + 5000 - 598, "connections_waiting": n - 1, "connections_pending": n}


def test_null_outputs(engine):
    """No pending send: next_due_ms is INT64_MAX. Then each optional output null in turn: the others are written as
    ever."""
    settings = [(3000 * 9, 1400), (100 * 9, 60), (5000, 1000)]
    pace = [dict(burst_count=2, burst_delay_ms=5), {}, dict(bytes_per_second=10 ** 9)]
    p = Pair(engine, settings, pace, 1408, 8, arena_slots=12)
    v = p.tick([1, 2], 2, 0, where="nothing pending")
    assert v.tail["next_due_ms"] == NO_DUE and v.tick["buffers"] == 4
    table, ids = p.table, _ids([0, 1, 2])
    for t, null in enumerate(["codes", "tick", "sent"]):
        before = {k: getattr(table, k).clone() for k in ("codes", "tick", "sent")}
        out = dict(codes=table.codes, tick=table.tick, sent_counters=table.sent)
        out["sent_counters" if null == "sent" else null] = None
        T.senders_send_paced(engine, table.arena, 1408, 4 * (t % 2), 8, ids, 2, table.senders, table.pace, 3, 5 * t,
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
            assert all(int(tick[f]) == v.tail[f] for f in W.TCP_SENDER_PACED_TAIL_FIELDS)
        if null == "sent":
            p.counters["bytes_sent"] -= v.tick["bytes"]
            p.counters["buffers_sent"] -= v.tick["buffers"]
            p.counters["connections_finished"] -= v.tick["connections_finished"]
        assert table.read_sent() == p.counters, null
        assert v.tick["buffers"] > 0


# ---- 8: arguments ------------------------------------------------------------------------------------------------
def test_refused_arguments(engine):
    settings = [(3000 * 9, 1400), (100 * 9, 60)]
    p = Pair(engine, settings, [dict(burst_count=2, burst_delay_ms=5), {}], 1408, 8, arena_slots=12)
    table = p.table
    ids = _ids([0, 1])
    ptr = {k: getattr(table, k).data_ptr() for k in ("arena", "senders", "pace", "descs", "codes", "tick", "sent",
                                                     "scratch")}
    arena_bytes, scratch_bytes = table.arena.numel(), table.scratch.numel() * 8

    def send(now=3, n=2, n_conns=2, stride=1408, sbytes=scratch_bytes, **over):
        a = dict(ptr, **over)
        T.senders_send_paced(engine, a["arena"], stride, 0, 8, ids.data_ptr(), 2, a["senders"], a["pace"], n_conns,
                             now, a["descs"], a["scratch"], codes=a["codes"], tick=a["tick"], sent_counters=a["sent"],
                             n=n, arena_bytes=arena_bytes, scratch_bytes=sbytes)

    bad = [dict(pace=ptr["pace"] + 4), dict(pace=None), dict(now=-1), dict(now=-(1 << 63)),
           dict(tick=ptr["tick"] + 4), dict(sbytes=T.senders_paced_scratch_bytes(2) - 1),
           dict(sbytes=T.senders_scratch_bytes(2)), dict(stride=1400), dict(senders=None), dict(descs=None)]
    for kw in bad:
        with pytest.raises(CtsError) as e:
            send(**kw)
        assert e.value.status == -1, kw
    send(n=0, now=-1, pace=None, stride=7)  # n == 0 is CTS_OK and does nothing, whatever else is passed
    send(n=0)
    torch.cuda.synchronize()
    entries, _, tick = table.read()
    assert np.array_equal(entries, table.fresh) and np.array_equal(table.read_pace(), table.fresh_pace)
    assert not tick.tobytes().strip(b"\0") and (table.arena.cpu().numpy() == 0xA5).all()
    assert table.read_sent()["bytes_sent"] == 0 and not table.descs.any()


# ---- 9: the loop the feature exists for ------------------------------------------------------------------------
def _loop(engine, corrupt=()):
    """37 connections with transfers of 1 to 40 buffers and mixed pacing; every tick lists all of them at the time the
    model's next_due_ms names; per tick send -> verify_at -> accounting over the tick's own descriptors, all on one
    stream with nothing read back; then the close. corrupt: (tick, tick-local slot) pairs whose first byte is flipped
    between the tick and the verify. The device's tick blocks are kept (device copies) and compared at the end."""
    n_conns, B, stride, max_buffers = 37, 1000, 1008, 3
    rng = np.random.default_rng(9)
    settings = [(int(rng.integers((k - 1) * B + 1, k * B + 1)), B) for k in [1, 40] + list(rng.integers(1, 41, 35))]
    pace_settings = [[{}, dict(bytes_per_second=250_000, period_ms=10), dict(burst_count=3, burst_delay_ms=11),
                      dict(bytes_per_second=100_000, period_ms=20)][c % 4] for c in range(n_conns)]
    buffers = [-(-t // B) for t, _ in settings]
    capacity = n_conns * max_buffers
    start = 1000
    table = T.PacedSenderTable(engine, settings, pace_settings, stride, capacity, start_ms=start, fill=0xA5)
    ids = list(range(n_conns))
    dev_ids = _ids(ids)
    cff = torch.full((n_conns,), -1, dtype=torch.int32, device=DEV)
    state, ref, ctr, block = (engine.new_conn_state(n_conns), engine.new_counters(), engine.new_counters(),
                              engine.new_counters())
    results = engine.new_conn_results(n_conns)
    entries, pace = W.tcp_sender_entries(settings), W.tcp_sender_pace_entries(pace_settings, start)
    arena = np.zeros(capacity * stride, dtype=np.uint8)
    base, now, first_fail, recv_until, dev_ticks, model_ticks = 0, start, {}, {}, [], []
    while int(entries["finished"].sum()) < n_conns:
        assert len(model_ticks) < 2000
        v = W.tcp_paced_sender_view(entries, pace, now, stride, arena, 0, capacity, ids, max_buffers)  # the host's clock
        entries, pace, n = v.entries, v.pace, v.tick["buffers"]
        table.send(dev_ids, max_buffers, now)
        dev_ticks.append(table.tick.clone())
        model_ticks.append(v)
        for (ct, g) in corrupt:
            if ct == len(model_ticks) - 1:
                table.arena[g * stride] ^= 0xFF
                c = int(v.descs["conn_index"][g])
                first_fail.setdefault(c, base + g)
        if n:
            descs = table.descs_of(n)
            engine.verify(table.arena, descs, max_length_hint=stride, counters=ctr, conn_first_fail=cff,
                          base_index=base)
            engine.refview_conns(table.arena.numel(), descs, ref, state, base_index=base, conn_first_fail=cff)
        for g in range(n):  # what each connection has received up to and including its first failing buffer
            c = int(v.descs["conn_index"][g])
            if c not in first_fail or base + g <= first_fail[c]:
                recv_until[c] = recv_until.get(c, 0) + int(v.descs["length"][g])
        base += n
        # the one host timer: sleep until the next deferred send (unpaced connections send in every tick)
        if v.tail["next_due_ms"] != NO_DUE and v.tick["connections_sent"] == 0:
            assert v.tail["next_due_ms"] > now
            now = v.tail["next_due_ms"]
    engine.conns_close(dev_ids, _u64([t for t, _ in settings]), cff, state, block, results=results)
    torch.cuda.synchronize()
    res = results.cpu().numpy().view(CONN_RESULT_DTYPE)
    dev_entries, _, _ = table.read()
    assert np.array_equal(dev_entries, entries) and np.array_equal(table.read_pace(), pace)
    # the device went through the model's ticks: every tick block is the model's, the due times included
    for k, (d, v) in enumerate(zip(dev_ticks, model_ticks)):
        tick = d.cpu().numpy().view(TCP_SENDER_PACED_TICK_DTYPE)[0]
        assert all(int(tick[f]) == v.tick[f] for f in W.TCP_SENDER_TICK_FIELDS), k
        assert all(int(tick[f]) == v.tail[f] for f in W.TCP_SENDER_PACED_TAIL_FIELDS), k
    assert any(v.tick["buffers"] == 0 for v in model_ticks) and len(model_ticks) > max(buffers) // max_buffers
    sent = table.read_sent()
    assert sent["bytes_sent"] == sum(t for t, _ in settings) and sent["buffers_sent"] == sum(buffers) == base
    assert sent["connections_finished"] == n_conns
    return settings, res, engine.read_counters_close(block), first_fail, recv_until, model_ticks


def test_paced_send_verify_account_close(engine):
    settings, res, close, _, recv, ticks = _loop(engine)
    assert (res["status"] == 0).all() and (res["first_fail"] == EMPTY).all() and (res["flags"] == 0).all()
    assert res["bytes_recv"].tolist() == [t for t, _ in settings]
    assert close["connections_closed"] == close["successful"] == 37
    assert close["bytes_recv"] == sum(t for t, _ in settings)
    assert any(v.tail["connections_waiting"] for v in ticks) and ticks[-1].tail["next_due_ms"] == NO_DUE


def test_paced_send_verify_account_close_with_a_data_error(engine):
    # tick 2, slot 1: a buffer in the middle of a transfer
    settings, res, close, first_fail, recv, ticks = _loop(engine, corrupt=[(2, 1)])
    assert len(first_fail) == 1
    (c, ordinal), = first_fail.items()
    assert ticks[2].tick["buffers"] > 1 and ordinal == ticks[0].tick["buffers"] + ticks[1].tick["buffers"] + 1
    for k in range(37):
        if k == c:
            assert int(res["status"][k]) == DATA_ERROR and int(res["first_fail"][k]) == ordinal
            assert int(res["bytes_recv"][k]) == recv[k]
        else:
            assert int(res["status"][k]) == 0 and int(res["bytes_recv"][k]) == settings[k][0], k
    assert close["data_errors"] == 1 and close["successful"] == 36
