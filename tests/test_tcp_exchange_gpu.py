"""GPU: Push, Pull, PushPull and Duplex on the device-resident path (include/cts_tcp_exchange.h) against the model
workload.tcp_exchange_view, which is itself held against the step-by-step sequence, the ctsIoPattern mirror and the
oracle in tests/test_tcp_exchange_cpu.py. The arena is pre-filled with 0xA5 and every byte of it is compared, so stray
writes show; entries, codes, the tick block, descriptors and the sent block are compared field by field. Every
comparison is exact, and every shape stays inside its arena.
"""
import numpy as np
import pytest
import torch

from ctstraffic_amd import _lib
from ctstraffic_amd import tcp_exchange as X
from ctstraffic_amd import tcp_senders as T
from ctstraffic_amd import workload as W
from ctstraffic_amd._lib import CtsError
from ctstraffic_amd.types import (CONN_RESULT_DTYPE, DESC_DTYPE, TCP_EXCHANGE_DTYPE, TCP_EXCHANGE_DUPLEX,
                                  TCP_EXCHANGE_PULL, TCP_EXCHANGE_PUSH, TCP_EXCHANGE_PUSHPULL, TCP_SENDER_TICK_DTYPE)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EMPTY = 0xFFFFFFFF
DATA_ERROR = W.STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN
PUSH, PULL, PUSHPULL, DUPLEX = TCP_EXCHANGE_PUSH, TCP_EXCHANGE_PULL, TCP_EXCHANGE_PUSHPULL, TCP_EXCHANGE_DUPLEX


def _ids(ids):
    return torch.from_numpy(np.asarray(list(ids), dtype=np.uint32).view(np.int32).copy()).to(DEV)


def _u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(DEV)


class Pair:
    """A device table and the model's state over the same entries and an arena of 0xA5."""

    def __init__(self, engine, settings, stride, capacity, arena_slots=None, max_listed=None, entries=None):
        self.table = X.ExchangeTable(engine, settings, stride, capacity, arena_slots=arena_slots, fill=0xA5,
                                     max_listed=max_listed)
        assert np.array_equal(self.table.fresh, W.tcp_exchange_entries(settings))
        if entries is not None:
            self.table.load(entries)
        self.entries = np.array(self.table.fresh if entries is None else entries, copy=True)
        self.arena = np.full(self.table.arena.numel(), 0xA5, dtype=np.uint8)
        self.descs = np.zeros(capacity, dtype=DESC_DTYPE)
        self.counters = None
        self.stride, self.capacity = stride, capacity
        self.view = None

    def model(self, ids, max_buffers, first_slot=0, capacity=None):
        cap = self.capacity if capacity is None else capacity
        v = W.tcp_exchange_view(self.entries, self.stride, self.arena, first_slot, cap, ids, max_buffers,
                                descs=self.descs[:cap], counters=self.counters)
        self.entries, self.arena, self.counters, self.view = v.entries, v.arena, v.counters, v
        self.descs[: len(v.descs)] = v.descs
        return v

    def same(self, n_listed, where=""):
        torch.cuda.synchronize()
        entries, codes, tick = self.table.read()
        for f in TCP_EXCHANGE_DTYPE.names:
            assert np.array_equal(entries[f], self.entries[f]), (where, f)
        assert np.array_equal(codes[:n_listed], self.view.codes), where
        for f in W.TCP_SENDER_TICK_FIELDS:
            assert int(tick[f]) == self.view.tick[f], (where, f)
        assert tick["bytes_dir"].tolist() == self.view.tick["bytes_dir"], where
        assert int(tick["reserved"]) == 0
        arena, descs = self.table.read_arena()
        for f in DESC_DTYPE.names:
            assert np.array_equal(descs[f], self.descs[f]), (where, f)
        assert np.array_equal(arena, self.arena), where
        assert self.table.read_sent() == self.counters, where

    def tick(self, ids, max_buffers, first_slot=0, capacity=None, where=""):
        self.table.send(_ids(ids), max_buffers, first_slot=first_slot, capacity=capacity)
        v = self.model(ids, max_buffers, first_slot=first_slot, capacity=capacity)
        self.same(len(ids), where)
        return v

    def to_the_end(self, ids, max_buffers, first_slot=0, capacity=None, limit=200):
        views = []
        for t in range(limit):
            views.append(self.tick(ids, max_buffers, first_slot=first_slot, capacity=capacity, where="tick %d" % t))
            if views[-1].tick["buffers"] == 0:
                return views
        raise AssertionError("the model has not ended after %d ticks" % limit)


# ---- 1: the edges of a buffer in its slot, and of a segment in its buffers -----------------------------------------
@pytest.mark.parametrize("stride,B,P,Q", [(65536, 65536, 3 * 65536 + 100, 65529), (65536, 65531, 200000, 65531),
                                          (16384, 9000, 20000, 9001), (1488, 1472, 4000, 1472), (48, 33, 100, 7)])
@pytest.mark.parametrize("first_slot", [0, 3])
def test_buffer_edges(engine, stride, B, P, Q, first_slot):
    """One connection per pattern, ticked to the end three buffers at a time: the transfers end inside a pull segment
    (PushPull), in a short buffer (Push, Pull) and, odd, in a short buffer each way (Duplex); segment ends fall inside
    a tick's burst, and both directions' offsets walk both byte phases."""
    T_pp = 2 * (P + Q) + P + Q // 2 + 1
    settings = [(PUSH, 3 * B + 1, B), (PULL, 2 * B + B // 2 + 1, B), (PUSHPULL, T_pp, B, P, Q),
                (DUPLEX, 5 * B + 3, B)]
    capacity = 11
    p = Pair(engine, settings, stride, capacity, arena_slots=first_slot + capacity + 2)
    views = p.to_the_end([2, 0, 3, 1], 3, first_slot=first_slot)
    assert views[0].tick["buffers"] == capacity and views[0].taken.tolist() == [3, 3, 3, 2]  # the one partly served
    assert views[-1].codes.tolist() == [2, 2, 2, 2] and (p.entries["finished"] == 1).all()
    assert p.entries["bytes_sent"].sum(axis=1).tolist() == [3 * B + 1, 2 * B + B // 2 + 1, T_pp,
                                                            5 * B + 3 + (5 * B + 3) % 2]
    assert all(v.tick["bytes_dir"][0] and v.tick["bytes_dir"][1] for v in views[:2])
    assert p.counters["bytes_sent"] == int(p.entries["transfer_bytes"].sum())


# ---- 2: the list ---------------------------------------------------------------------------------------------------
def _table_1100():
    rng = np.random.default_rng(11)
    settings = []
    for c in range(1100):
        B = int(rng.integers(1, 129))
        k = 1 + c % 6
        T_ = int(rng.integers((k - 1) * B + 1, k * B + 1))
        settings.append((c % 4, T_, B, int(rng.integers(1, 3 * B + 2)), int(rng.integers(1, 3 * B + 2))))
    settings[11] = (PUSHPULL, 1000, 200, 300, 100)   # B above the stride of 128
    settings[700] = (DUPLEX, 5000, 129)
    return settings


_SETTINGS_1100 = _table_1100()


@pytest.mark.parametrize("max_buffers", [1, 3, 7])
@pytest.mark.parametrize("n_listed", [1, 255, 256, 257, 1100])
def test_shuffled_lists(engine, n_listed, max_buffers):
    """A shuffled list out of a table of 1 100 that mixes the four patterns, some connections already finished, two
    ids beyond the table, two with B above the stride, one entry with an unknown pattern; ticked to the end,
    everything compared after each tick."""
    settings = _SETTINGS_1100
    entries = W.tcp_exchange_entries(settings)
    entries["finished"][::7] = 1
    entries["pattern"][13] = 4
    rng = np.random.default_rng(n_listed)
    ids = [int(x) for x in rng.permutation(len(settings))][:n_listed]
    if n_listed >= 255:
        ids[5], ids[n_listed // 2] = 1100, 0xFFFFFFFF
        for pos, c in ((9, 11), (n_listed - 1, 700), (17, 13)):
            if c in ids:
                ids[ids.index(c)] = ids[pos]
            ids[pos] = c
        assert len(set(ids)) == n_listed
    wants = sum(min(max_buffers, int(entries["total_buffers"][c])) for c in ids
                if c < 1100 and c not in (11, 700, 13) and not entries["finished"][c])
    capacity = max(1, wants - 3)  # the first tick's last connections find no room
    p = Pair(engine, settings, 128, capacity, max_listed=n_listed, entries=entries)
    views = p.to_the_end(ids, max_buffers)
    if n_listed >= 255:
        assert views[0].tick["buffers"] == capacity == wants - 3 and {2, 4} <= set(views[-1].codes.tolist())
        assert views[0].tick["connections_skipped"] >= 5 and len(views) >= 6 // max_buffers + 1
        listed = np.array([c for c in ids if c < 1100 and c not in (11, 700, 13)])
        assert (p.entries["finished"][listed] == 1).all()


# ---- 3: capacity -----------------------------------------------------------------------------------------------------
def test_capacity_inside_a_segment_at_its_end_and_zero(engine):
    """Connections of P = 2500, Q = 1000 in buffers of 1000: a cycle is the buffers 1000, 1000, 500 | 1000. Twenty of
    them want 6 each. The capacity ends after connection 12's second buffer (inside its push segment), then after
    another's third (exactly at the segment's end), then is zero: the partly served connection, and code 3 behind
    it."""
    settings = [(PUSHPULL, 20 * 3500 + c, 1000, 2500, 1000) for c in range(20)]
    ids = list(range(20))
    p = Pair(engine, settings, 1008, 120, arena_slots=123)
    v = p.tick(ids, 6, capacity=12 * 6 + 2, where="inside a segment")
    assert v.codes.tolist() == [0] * 13 + [3] * 7 and v.taken.tolist() == [6] * 12 + [2] + [0] * 7
    assert p.entries["bytes_sent"][12].tolist() == [2000, 0] and X.exchange_where(p.entries[12]) == (0, 2000)
    assert (p.entries["buffers_sent"][13:] == 0).all() and v.tick["connections_no_room"] == 7
    # connection 12 first: it completes its push segment with one buffer of 500, and the capacity ends there
    v = p.tick([12, 13, 14], 6, capacity=1, first_slot=2, where="at a segment's end")
    assert v.codes.tolist() == [0, 3, 3] and v.descs["length"][0] == 500
    assert p.entries["bytes_sent"][12].tolist() == [2500, 0] and X.exchange_where(p.entries[12]) == (1, 0)
    v = p.tick([12, 13, 14], 6, capacity=0, where="zero")
    assert v.codes.tolist() == [3, 3, 3] and v.tick["buffers"] == 0 and v.tick["connections_no_room"] == 3
    # and on: its next buffer is the pull segment's
    v = p.tick([12, 13], 2, where="on")
    assert v.descs["conn_index"][:4].tolist() == [12 + 20, 12, 13, 13] and v.descs["length"][0] == 1000


# ---- 4: positions beyond 2^33 buffers ----------------------------------------------------------------------------------
def test_seeked_past_2_pow_33(engine):
    """T about 2^50 at B = 65531 with P and Q no multiples of B: entries seeked to m0 > 2^33 (the start of a cycle,
    the last buffer of a push segment, inside a pull segment, four buffers before the end; Pull and Duplex as far
    out), one tick of a few buffers each. The kernels' closed forms cost what they cost at m = 0."""
    B, P, Q = 65531, 200_003, 70_001
    T_ = (1 << 50) + 12345
    K = -(-P // B) + -(-Q // B)
    settings = [(PUSHPULL, T_, B, P, Q)] * 4 + [(PULL, T_, B), (DUPLEX, T_, B)]
    N = W.tcp_exchange_total_buffers(PUSHPULL, T_, B, P, Q)
    y = ((1 << 33) + 999) // K + 1
    seek = [y * K, y * K + -(-P // B) - 1, y * K + K - 1, N - 4, (1 << 33) + 7, (1 << 34) + 1]
    assert min(seek) > 1 << 33
    entries = W.tcp_exchange_entries(settings, seek=seek)
    for c in range(6):
        assert entries[c] == X.exchange_seek(X.exchange_init(*settings[c]), seek[c])
    p = Pair(engine, settings, 65536, 34, entries=entries)
    v = p.tick([3, 0, 5, 1, 4, 2], 6, where="one tick")
    assert v.codes.tolist() == [1, 0, 0, 0, 0, 0] and v.taken.tolist() == [4, 6, 6, 6, 6, 6]
    assert p.entries["buffers_sent"].tolist() == [m + 6 for m in seek[:3]] + [N] + [m + 6 for m in seek[4:]]
    assert int(p.entries["bytes_sent"][3].sum()) == T_ and len(set(v.descs["length"][:34].tolist())) > 3
    for c in range(6):
        assert p.entries[c] == X.exchange_seek(X.exchange_init(*settings[c]), int(p.entries["buffers_sent"][c]))


# ---- 5: the scan's second pass -------------------------------------------------------------------------------------
def test_65537_listed_connections(engine):
    """65 537 listed one-buffer connections at stride 16: 257 tiles, so tick_plan_scan takes a second pass of one
    tile; the patterns by turns, a pull or an odd direction in every tile."""
    n = 65537
    settings = [(c % 4, 1 + c % 16, 16, 1 + c % 5, 1 + c % 3) for c in range(n)]
    p = Pair(engine, settings, 16, n)
    ids = [int(x) for x in np.random.default_rng(65537).permutation(n)]
    v = p.tick(ids, 1, where="65537")
    assert v.tick["buffers"] == n and int(v.prefix[-1]) == n - 1 and v.tick["bytes_dir"][1] > 0


# ---- 6: tcp_exchange_descs past its first grid-stride pass ---------------------------------------------------------
def test_descs_in_two_passes():
    """An engine of its own with blocks-per-CU 1: tcp_exchange_descs' grid is at most one workgroup per CU, and the
    tick's buffers, sized from the CU count, are more than its lanes. The capacity lies above the total: descriptors
    past the total keep a marker."""
    from ctstraffic_amd import Engine

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lanes = cus * 256
    conns = 300
    max_buffers = (lanes + 333) // (conns - 30) + 1
    settings = [(c % 4, 16 * max_buffers * 2 - 5, 16 if c % 10 else 13, 16 * 3 + 5, 7) for c in range(conns)]
    ids = [int(x) for x in np.random.default_rng(5).permutation(conns)]
    eng = Engine(0)
    try:
        eng.set_attr(_lib.ATTR_BLOCKS_PER_CU, 1)
        assert eng.get_attr(_lib.ATTR_BLOCKS_PER_CU) == 1
        total = sum(min(max_buffers, int(n)) for n in W.tcp_exchange_entries(settings)["total_buffers"])
        assert total > lanes + 256
        p = Pair(eng, settings, 16, total + 1000)
        p.descs["length"] = 0xA5A5A5A5
        p.table.descs.copy_(torch.from_numpy(p.descs.view(np.int64).copy()))
        v = p.tick(ids, max_buffers, where="two passes")
        assert v.tick["buffers"] == total
        assert (p.descs["length"][total:] == 0xA5A5A5A5).all() and (p.descs["length"][:total] <= 16).all()
        first, later = p.descs["conn_index"][:lanes], p.descs["conn_index"][lanes:total]
        assert len(set(later.tolist()) - set(first.tolist())) > 20
    finally:
        eng.close()


# ---- 7: a Push table is the senders' tick --------------------------------------------------------------------------
@pytest.mark.parametrize("stride,B", [(65536, 65531), (1488, 1472), (48, 33)])
def test_push_table_is_the_senders_tick_byte_for_byte(engine, stride, B):
    """The same transfers through cts_tcp_senders_send and, as Push entries, through cts_tcp_exchange_send, three ticks
    with a finished entry, an id out of range and a capacity that cuts the first: the arena, the descriptors, the
    codes, the tick's first 32 bytes and the sent block are the same bytes."""
    plain = [(5 * B + 3 * c + 1, B) for c in range(23)]
    capacity = 23 * 3 - 4
    s = T.SenderTable(engine, plain, stride, capacity, fill=0xA5, max_listed=25)
    x = X.ExchangeTable(engine, [(PUSH, t, b) for t, b in plain], stride, capacity, fill=0xA5, max_listed=25)
    se, xe = s.fresh.copy(), x.fresh.copy()
    se["finished"][4] = xe["finished"][4] = 1
    s.load(se)
    x.load(xe)
    ids = _ids([int(i) for i in np.random.default_rng(7).permutation(23)] + [23, 0xFFFFFFFF])
    for t in range(3):
        s.send(ids, 3)
        x.send(ids, 3)
        torch.cuda.synchronize()
        assert torch.equal(s.arena, x.arena) and torch.equal(s.descs, x.descs) and torch.equal(s.codes, x.codes), t
        assert torch.equal(s.tick, x.tick[: TCP_SENDER_TICK_DTYPE.itemsize // 8]), t
        assert torch.equal(s.sent, x.sent), t
        a, b = s.read()[0], x.read()[0]
        assert np.array_equal(a["bytes_sent"], b["bytes_sent"][:, 0]) and not b["bytes_sent"][:, 1].any()
        assert np.array_equal(a["buffers_sent"], b["buffers_sent"]) and np.array_equal(a["finished"], b["finished"])
        assert t or int(x.read()[2]["buffers"]) == capacity == 22 * 3 - 1  # cut: one connection partly served


# ---- 8: arguments ----------------------------------------------------------------------------------------------------
def test_argument_edges_and_null_outputs(engine):
    settings = [(PUSHPULL, 3000 * 9, 1400, 3000, 1500), (DUPLEX, 100 * 9, 60)]
    p = Pair(engine, settings, 1408, 8, arena_slots=12)
    table = p.table
    ids = _ids([0, 1])
    ptr = {k: getattr(table, k).data_ptr() for k in ("arena", "entries", "descs", "codes", "tick", "sent", "scratch")}
    arena_bytes, scratch_bytes = table.arena.numel(), table.scratch.numel() * 8

    def send(stride=1408, first_slot=0, capacity=8, conn_ids=ids.data_ptr(), n=2, n_conns=2, max_buffers=2,
             arena_bytes=arena_bytes, sbytes=scratch_bytes, **over):
        a = dict(ptr, **over)
        X.exchange_send(engine, a["arena"], stride, first_slot, capacity, conn_ids, max_buffers, a["entries"], n_conns,
                        a["descs"], a["scratch"], codes=a["codes"], tick=a["tick"], sent_counters=a["sent"], n=n,
                        arena_bytes=arena_bytes, scratch_bytes=sbytes)

    bad = [dict(stride=1400), dict(stride=0), dict(stride=(16 << 20) + 16), dict(max_buffers=0),
           dict(arena=ptr["arena"] + 8), dict(arena=None), dict(first_slot=5), dict(capacity=13),
           dict(first_slot=13, capacity=0), dict(first_slot=(1 << 64) - 4, capacity=8),
           dict(arena_bytes=8 * 1408 - 1), dict(entries=ptr["entries"] + 4), dict(entries=None),
           dict(descs=ptr["descs"] + 4), dict(descs=None), dict(tick=ptr["tick"] + 4), dict(sent=ptr["sent"] + 4),
           dict(scratch=ptr["scratch"] + 4), dict(scratch=None), dict(conn_ids=ids.data_ptr() + 2),
           dict(conn_ids=None), dict(codes=ptr["codes"] + 2), dict(sbytes=X.exchange_scratch_bytes(2) - 1),
           dict(n_conns=(1 << 31) + 1)]
    for kw in bad:
        with pytest.raises(CtsError) as e:
            send(**kw)
        assert e.value.status == -1, kw
    send(n=0, stride=7, arena=None)  # n == 0 is CTS_OK and does nothing, whatever else is passed
    torch.cuda.synchronize()
    entries, _, tick = table.read()
    assert np.array_equal(entries, table.fresh) and int(tick["buffers"]) == 0
    assert (table.arena.cpu().numpy() == 0xA5).all() and table.read_sent()["bytes_sent"] == 0

    # each optional output null in turn: the others are written as ever
    for t, null in enumerate(["codes", "tick", "sent"]):
        before = {k: getattr(table, k).clone() for k in ("codes", "tick", "sent")}
        send(first_slot=4 * (t % 2), **{null: None})
        v = p.model([0, 1], 2, first_slot=4 * (t % 2))
        torch.cuda.synchronize()
        assert torch.equal(getattr(table, null), before[null]), null
        entries, codes, tick = table.read()
        arena, descs = table.read_arena()
        assert np.array_equal(entries, p.entries) and np.array_equal(arena, p.arena), null
        assert np.array_equal(descs, p.descs), null
        if null != "codes":
            assert np.array_equal(codes[:2], v.codes)
        if null != "tick":
            assert all(int(tick[f]) == v.tick[f] for f in W.TCP_SENDER_TICK_FIELDS)
            assert tick["bytes_dir"].tolist() == v.tick["bytes_dir"]
        if null == "sent":
            p.counters["bytes_sent"] -= v.tick["bytes"]
            p.counters["buffers_sent"] -= v.tick["buffers"]
        assert table.read_sent() == p.counters, null


def test_two_ticks_on_one_stream(engine):
    """Two ticks queued back to back into different slots, nothing read between them; the second starts where the
    first left every connection, across a segment end."""
    settings = [(PUSHPULL, 10 * 9000 + c, 9000, 20000, 9001) for c in range(5)] + [(DUPLEX, 70001, 9000),
                                                                                  (PULL, 50000, 9000)]
    p = Pair(engine, settings, 16384, 14, arena_slots=28)
    ids = _ids(range(7))
    p.table.send(ids, 2, first_slot=0)
    first = p.table.descs.clone()  # queued on the same stream, between the ticks
    p.table.send(ids, 2, first_slot=14)
    v1 = p.model(range(7), 2, first_slot=0)
    d1 = v1.descs.copy()
    v2 = p.model(range(7), 2, first_slot=14)
    p.same(7, "second tick")
    assert np.array_equal(first.cpu().numpy().view(DESC_DTYPE)[:14], d1)
    assert v2.descs["conn_index"][:2].tolist() == [0, 7] and v2.descs["length"][:2].tolist() == [2000, 9000]


# ---- 9: the loop the feature exists for ----------------------------------------------------------------------------
def _loop(engine, corrupt=None):
    """13 connections of the four patterns; per tick send -> verify_at -> accounting over the tick's own descriptors
    and 2 x n_conns receivers, all on one stream with nothing read back; then the close of every receiver against
    cts_tcp_exchange_direction_bytes. corrupt: (tick, tick-local slot) whose first byte is flipped between the tick
    and the verify."""
    B, stride, max_buffers = 1000, 1008, 3
    settings = [(c % 4, 3000 * (c + 1) + 17 * c + 1, B, 2500, 1001) for c in range(13)]
    n_conns = len(settings)
    capacity = n_conns * max_buffers
    table = X.ExchangeTable(engine, settings, stride, capacity, fill=0xA5)
    n_recv = table.n_receivers
    ids = list(range(n_conns))
    dev_ids = _ids(ids)
    cff = torch.full((n_recv,), -1, dtype=torch.int32, device=DEV)
    state, ref, ctr, block = (engine.new_conn_state(n_recv), engine.new_counters(), engine.new_counters(),
                              engine.new_counters())
    results = engine.new_conn_results(n_recv)
    entries = W.tcp_exchange_entries(settings)
    arena = np.zeros(capacity * stride, dtype=np.uint8)
    base, first_fail, recv_until, t = 0, {}, {}, 0
    while True:
        v = W.tcp_exchange_view(entries, stride, arena, 0, capacity, ids, max_buffers)  # the host's own arithmetic
        entries, n = v.entries, v.tick["buffers"]
        if n == 0:
            break
        table.send(dev_ids, max_buffers)
        if corrupt is not None and corrupt[0] == t:
            g = corrupt[1]
            table.arena[g * stride] ^= 0xFF
            first_fail[int(v.descs["conn_index"][g])] = base + g
        descs = table.descs_of(n)
        engine.verify(table.arena, descs, max_length_hint=stride, counters=ctr, conn_first_fail=cff, base_index=base)
        engine.refview_conns(table.arena.numel(), descs, ref, state, base_index=base, conn_first_fail=cff)
        for g in range(n):  # what each receiver has received up to and including its first failing buffer
            r = int(v.descs["conn_index"][g])
            if r not in first_fail or base + g <= first_fail[r]:
                recv_until[r] = recv_until.get(r, 0) + int(v.descs["length"][g])
        base += n
        t += 1
    expected = table.expected_bytes()
    engine.conns_close(_ids(range(n_recv)), _u64(expected), cff, state, block, results=results)
    torch.cuda.synchronize()
    res = results.cpu().numpy().view(CONN_RESULT_DTYPE)
    dev_entries, _, _ = table.read()
    assert np.array_equal(dev_entries, entries) and (entries["finished"] == 1).all()
    assert expected.tolist() == entries["bytes_sent"][:, 0].tolist() + entries["bytes_sent"][:, 1].tolist()
    sent = table.read_sent()
    assert sent["bytes_sent"] == int(expected.sum()) and sent["buffers_sent"] == base
    assert sent["connections_finished"] == n_conns
    return settings, expected, res, engine.read_counters_close(block), first_fail, recv_until, v


def test_send_verify_account_close(engine):
    settings, expected, res, close, _, recv, _ = _loop(engine)
    assert (res["status"] == 0).all() and (res["first_fail"] == EMPTY).all() and (res["flags"] == 0).all()
    assert res["bytes_recv"].tolist() == expected.tolist() == [recv.get(r, 0) for r in range(26)]
    assert close["connections_closed"] == close["successful"] == 26
    assert close["bytes_recv"] == int(expected.sum())


def test_send_verify_account_close_with_a_corrupt_pull_buffer(engine):
    """Tick 1, slot 4: connection 2 (PushPull) is in its pull segment there, so the buffer is receiver 2 + 13's: that
    receiver reports the buffer's stream ordinal and the data error, receiver 2, the same connection's other
    direction, closes clean, and both closes took cts_tcp_exchange_direction_bytes as their expectation."""
    settings, expected, res, close, first_fail, recv, _ = _loop(engine, corrupt=(1, 4))
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
