"""GPU: TCP senders on the device-resident path (include/cts_tcp_senders.h) against the model
workload.tcp_sender_view, which is itself held against the reference's send arithmetic, the ctsIoPattern mirror and
the oracle in tests/test_tcp_senders_cpu.py. The arena is pre-filled with 0xA5 and every byte of it is compared, so
stray writes show; entries, codes, the tick block, descriptors and the sent block are compared field by field. Every
comparison is exact.
"""
import numpy as np
import pytest
import torch

import launch_depths as L
from ctstraffic_amd import tcp_senders as T
from ctstraffic_amd import workload as W
from ctstraffic_amd._lib import CtsError
from ctstraffic_amd.types import CONN_RESULT_DTYPE, DESC_DTYPE, TCP_SENDER_DTYPE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EMPTY = 0xFFFFFFFF
DATA_ERROR, NOT_ALL_DATA = W.STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN, W.STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED


def _ids(ids):
    return torch.from_numpy(np.asarray(list(ids), dtype=np.uint32).view(np.int32).copy()).to(DEV)


def _u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(DEV)


class Pair:
    """A device table and the model's state over the same entries and an arena of 0xA5."""

    def __init__(self, engine, settings, stride, capacity, arena_slots=None, max_listed=None, entries=None):
        self.table = T.SenderTable(engine, settings, stride, capacity, arena_slots=arena_slots, fill=0xA5,
                                   max_listed=max_listed)
        assert np.array_equal(self.table.fresh, W.tcp_sender_entries(settings))
        if entries is not None:
            self.table.load(entries)
        self.entries = np.array(self.table.fresh if entries is None else entries, copy=True)
        self.arena = np.full(self.table.arena.numel(), 0xA5, dtype=np.uint8)
        self.descs = np.zeros(capacity, dtype=DESC_DTYPE)
        self.counters = None
        self.stride, self.capacity = stride, capacity
        self.view = None

    def model(self, ids, max_buffers, first_slot=0, capacity=None):
        v = W.tcp_sender_view(self.entries, self.stride, self.arena, first_slot,
                              self.capacity if capacity is None else capacity, ids, max_buffers,
                              descs=self.descs[: self.capacity if capacity is None else capacity],
                              counters=self.counters)
        self.entries, self.arena, self.counters, self.view = v.entries, v.arena, v.counters, v
        self.descs[: len(v.descs)] = v.descs
        return v

    def same(self, n_listed, where=""):
        torch.cuda.synchronize()
        entries, codes, tick = self.table.read()
        for f in TCP_SENDER_DTYPE.names:
            assert np.array_equal(entries[f], self.entries[f]), (where, f)
        assert np.array_equal(codes[:n_listed], self.view.codes), where
        for f in W.TCP_SENDER_TICK_FIELDS:
            assert int(tick[f]) == self.view.tick[f], (where, f)
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


# ---- 1: the edges of a buffer in its slot ----------------------------------------------------------------------
@pytest.mark.parametrize("stride,B", [(65536, 65536), (65536, 65531), (65536, 8193), (16384, 9000), (1488, 1472),
                                      (1488, 33), (48, 33), (48, 48)])
@pytest.mark.parametrize("first_slot", [0, 3])
def test_buffer_edges(engine, stride, B, first_slot):
    """Transfers that end in a 1-byte buffer, in a full one and in between; an odd B walks both byte phases, and the
    offsets wrap past 65 536 inside a tick (connection 3 starts 2 B - 1 below a multiple of 65 536)."""
    settings = [(3 * B + 1, B), (4 * B, B), (2 * B + B // 2 + 1, B), (1 << 40, B), (1, B)]
    entries = W.tcp_sender_entries(settings)
    entries["bytes_sent"][3] = 7 * 65536 - 2 * B + 1
    capacity = 3 + 3 + 3 + 3 + 1
    p = Pair(engine, settings, stride, capacity, arena_slots=first_slot + capacity + 2, entries=entries)
    v = p.tick([3, 0, 4, 1, 2], 3, first_slot=first_slot, where="tick 0")
    assert v.tick["buffers"] == capacity and v.codes.tolist() == [0, 0, 1, 0, 1]
    offs = v.descs["expected_pattern_offset"][:3].astype(np.int64)
    assert B == 65536 or (offs[1:] < offs[:-1]).any()  # wrapped
    v = p.tick([3, 0, 4, 1, 2], 3, first_slot=first_slot, where="tick 1")
    assert v.codes.tolist() == [0, 1, 2, 1, 2] and v.descs["length"][3] == 1
    assert v.descs["length"][4] == B  # connection 1 ends in a full buffer


# ---- 2: the list -----------------------------------------------------------------------------------------------
def _table_1500():
    rng = np.random.default_rng(15)
    settings = []
    for c in range(1500):
        B = int(rng.integers(1, 129))
        k = 1 + c % 7
        settings.append((int(rng.integers((k - 1) * B + 1, k * B + 1)), B))
    settings[11] = (1000, 200)   # B above the stride of 128
    settings[700] = (5000, 129)
    return settings


_SETTINGS_1500 = _table_1500()


@pytest.mark.parametrize("max_buffers", [1, 3])
@pytest.mark.parametrize("n_listed", [1, 255, 256, 257, 1100])
def test_shuffled_lists(engine, n_listed, max_buffers):
    """A shuffled list out of a table of 1 500, some connections already finished, two ids beyond the table, two with
    B above the stride; three ticks, everything compared after each."""
    settings = _SETTINGS_1500
    entries = W.tcp_sender_entries(settings)
    entries["finished"][::7] = 1
    rng = np.random.default_rng(n_listed)
    ids = [int(x) for x in rng.permutation(len(settings)) if x not in (11, 700)][:n_listed]
    if n_listed >= 255:
        ids[5], ids[n_listed // 2], ids[9], ids[n_listed - 1] = 1500, 0xFFFFFFFF, 11, 700
    capacity = max_buffers * n_listed
    p = Pair(engine, settings, 128, capacity, max_listed=n_listed, entries=entries)
    for t in range(3):
        v = p.tick(ids, max_buffers, where="tick %d" % t)
    if n_listed >= 255:
        assert {2, 4} <= set(v.codes.tolist()) and 0 < v.tick["buffers"] < capacity
        assert v.tick["connections_skipped"] >= 4


# ---- 3: capacity -----------------------------------------------------------------------------------------------
def test_capacity_cuts_a_burst(engine):
    settings = [(10 * 1000 + c, 1000) for c in range(40)]
    ids = list(range(40))
    capacity = 25 * 4 + 2  # in the middle of connection 25's burst of 4
    p = Pair(engine, settings, 1008, capacity, arena_slots=capacity + 3)
    v = p.tick(ids, 4, where="cut")
    assert v.codes.tolist() == [0] * 26 + [3] * 14 and v.taken.tolist() == [4] * 25 + [2] + [0] * 14
    assert v.tick["buffers"] == capacity and v.tick["connections_no_room"] == 14
    assert (p.entries["bytes_sent"][26:] == 0).all() and int(p.entries["bytes_sent"][25]) == 2000
    # the next tick lists the rest first
    v = p.tick(ids[25:] + ids[:25], 4, where="rest")
    assert v.codes.tolist()[:15] == [0] * 15 and 3 in v.codes.tolist()


def test_capacity_exact_zero_and_far_above(engine):
    settings = [(3 * 700 + 5 * c, 700) for c in range(9)]
    need = sum(min(2, -(-t // b)) for t, b in settings)
    p = Pair(engine, settings, 704, need)
    v = p.tick(range(9), 2, where="exact")
    assert v.tick["buffers"] == need and v.tick["connections_no_room"] == 0
    p = Pair(engine, settings, 704, 4)
    v = p.tick(range(9), 2, capacity=0, where="zero")
    assert v.codes.tolist() == [3] * 9 and v.tick["buffers"] == 0
    # far above the total: the grids come from the capacity; slots and descriptors past the total stay as they were
    p = Pair(engine, settings, 704, 5000)
    p.descs["length"] = 0xA5A5A5A5
    p.table.descs.copy_(torch.from_numpy(p.descs.view(np.int64).copy()))
    v = p.tick(range(9), 2, where="far above")
    assert v.tick["buffers"] == need and (p.descs["length"][need:] == 0xA5A5A5A5).all()
    # the same on the workgroup path
    settings = [(3 * 9000 + c, 9000) for c in range(5)]
    p = Pair(engine, settings, 16384, 900)
    v = p.tick(range(5), 2, where="far above, pieces")
    assert v.tick["buffers"] == 10


# ---- 4: one connection, many buffers ---------------------------------------------------------------------------
def test_one_connection_many_buffers(engine):
    p = Pair(engine, [(48 * 2000, 48), (33 * 5, 33)], 48, 705)
    v = p.tick([0, 1], 700, where="700 of one")
    assert v.taken.tolist() == [700, 5] and v.tick["buffers"] == 705
    v = p.tick([0], 700, where="700 more")
    assert v.taken.tolist() == [700]


# ---- 5: 64-bit sums ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start_of,B,stride", [(lambda B: (1 << 32) - 3 * B, 65531, 65536),
                                               (lambda B: (1 << 53) - B, 1471, 1488),
                                               (lambda B: (1 << 32) - 3 * B, 33, 48)])
def test_wide_sums(engine, start_of, B, stride):
    start = start_of(B)
    settings = [(start + 100 * B + 7, B), ((1 << 63) + 5 * B, B)]
    entries = W.tcp_sender_entries(settings)
    entries["bytes_sent"][0], entries["buffers_sent"][0] = start, (1 << 32) - 2
    entries["bytes_sent"][1] = 1 << 63
    p = Pair(engine, settings, stride, 12, entries=entries)
    for t, codes in enumerate([[0, 1], [0, 2], [0, 2]]):
        v = p.tick([0, 1], 5, where="tick %d" % t)
        assert v.codes.tolist() == codes
    assert int(p.entries["bytes_sent"][0]) == start + 15 * B and int(p.entries["buffers_sent"][0]) == (1 << 32) + 13
    d = p.descs[:5]
    assert d["expected_pattern_offset"].tolist() == [(start + (10 + j) * B) % 65536 for j in range(5)]
    assert int(p.entries["bytes_sent"][1]) == (1 << 63) + 5 * B


# ---- 6: past the first loop pass -------------------------------------------------------------------------------
def test_pieces_past_the_first_batch(engine):
    """600 x 64 KiB at one workgroup per CU (the engine's default fill grid cap): more pieces than workgroups x 16, so
    every workgroup decodes a second batch; the depth comes from the piece-fill model over the capacity."""
    from ctstraffic_amd._lib import ATTR_FILL_BLOCKS_PER_CU

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    fill_bpc = engine.get_attr(ATTR_FILL_BLOCKS_PER_CU)
    n = 600
    settings = [(65536 * 3 + 17 * c, 65536 if c % 3 else 65531) for c in range(n // 2)]
    p = Pair(engine, settings, 65536, n)
    ids = [int(x) for x in np.random.default_rng(6).permutation(n // 2)]
    p.table.send(_ids(ids), 2)
    v = p.model(ids, 2)
    assert v.tick["buffers"] == n
    depth = L.piece_fill_depth(v.descs, 65536, cus, fill_bpc, p.table.arena.numel())
    assert depth["ppb"] == 8 and depth["batches_max"] >= 2, depth
    p.same(len(ids), "600 x 64 KiB")


def test_small_path_in_two_passes(engine):
    """The wave-per-buffer path at a capacity its grid rule takes in two passes (grid_for over the capacity at the
    engine's small-buffer blocks per CU)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    from ctstraffic_amd._lib import ATTR_SMALL_BLOCKS_PER_CU

    bpc = engine.get_attr(ATTR_SMALL_BLOCKS_PER_CU)
    one_pass = 4 * cus * bpc
    conns = 120
    per = -(-(one_pass + one_pass // 3) // conns)
    capacity = conns * per
    depth = L.team_fill_depth(capacity, 64, cus, bpc)
    assert depth["passes_max"] >= 2 and depth["passes_min"] >= 1, depth
    settings = [(33 * per + 1, 33) for _ in range(conns)]
    p = Pair(engine, settings, 48, capacity)
    v = p.tick(range(conns), per, where="two passes")
    assert v.tick["buffers"] == capacity


# ---- 7: against the host-fed path ------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,B", [(65536, 65531), (16384, 9000), (1488, 1472), (48, 33)])
def test_same_arena_as_the_host_fed_fill(engine, stride, B):
    settings = [(5 * B + 3 * c + 1, B) for c in range(23)]
    capacity = 23 * 3
    p = Pair(engine, settings, stride, capacity)
    order = [int(x) for x in np.random.default_rng(7).permutation(23)]
    for t in range(2):
        p.arena[:] = 0xA5
        p.table.arena.fill_(0xA5)
        p.table.send(_ids(order), 3)
        v = p.model(order, 3)
        n = v.tick["buffers"]
        host_fed = torch.full((capacity * stride,), 0xA5, dtype=torch.uint8, device=DEV)
        dd = torch.from_numpy(np.ascontiguousarray(v.descs[:n]).view(np.uint8).copy()).to(DEV)
        engine.fill(host_fed, dd, max_length_hint=stride)
        torch.cuda.synchronize()
        assert torch.equal(p.table.arena, host_fed)
        assert np.array_equal(host_fed.cpu().numpy(), v.arena)


# ---- 8: arguments ------------------------------------------------------------------------------------------------
def test_argument_edges_and_null_outputs(engine):
    settings = [(3000 * 9, 1400), (100 * 9, 60)]
    p = Pair(engine, settings, 1408, 8, arena_slots=12)
    table = p.table
    ids = _ids([0, 1])
    ptr = {k: getattr(table, k).data_ptr() for k in ("arena", "senders", "descs", "codes", "tick", "sent", "scratch")}
    arena_bytes, scratch_bytes = table.arena.numel(), table.scratch.numel() * 8

    def send(stride=1408, first_slot=0, capacity=8, conn_ids=ids.data_ptr(), n=2, n_conns=2, max_buffers=2,
             arena_bytes=arena_bytes, sbytes=scratch_bytes, **over):
        a = dict(ptr, **over)
        T.senders_send(engine, a["arena"], stride, first_slot, capacity, conn_ids, max_buffers, a["senders"], n_conns,
                       a["descs"], a["scratch"], codes=a["codes"], tick=a["tick"], sent_counters=a["sent"], n=n,
                       arena_bytes=arena_bytes, scratch_bytes=sbytes)

    bad = [dict(stride=1400), dict(stride=0), dict(stride=(16 << 20) + 16), dict(max_buffers=0),
           dict(arena=ptr["arena"] + 8), dict(arena=None), dict(first_slot=5), dict(capacity=13),
           dict(first_slot=13, capacity=0), dict(first_slot=(1 << 64) - 4, capacity=8),
           dict(arena_bytes=8 * 1408 - 1), dict(senders=ptr["senders"] + 4), dict(senders=None),
           dict(descs=ptr["descs"] + 4), dict(descs=None), dict(tick=ptr["tick"] + 4), dict(sent=ptr["sent"] + 4),
           dict(scratch=ptr["scratch"] + 4), dict(scratch=None), dict(conn_ids=ids.data_ptr() + 2),
           dict(conn_ids=None), dict(codes=ptr["codes"] + 2), dict(sbytes=T.senders_scratch_bytes(2) - 1)]
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
        if null == "sent":
            p.counters["bytes_sent"] -= v.tick["bytes"]
            p.counters["buffers_sent"] -= v.tick["buffers"]
        assert table.read_sent() == p.counters, null


def test_two_ticks_on_one_stream(engine):
    """Two ticks queued back to back into different slots, nothing read between them."""
    settings = [(10 * 9000 + c, 9000) for c in range(7)]
    p = Pair(engine, settings, 16384, 14, arena_slots=28)
    ids = _ids(range(7))
    p.table.send(ids, 2, first_slot=0)
    first = p.table.descs.clone()  # queued on the same stream, between the ticks
    p.table.send(ids, 2, first_slot=14)
    v1 = p.model(range(7), 2, first_slot=0)
    d1 = v1.descs.copy()
    p.model(range(7), 2, first_slot=14)
    p.same(7, "second tick")
    assert np.array_equal(first.cpu().numpy().view(DESC_DTYPE)[:14], d1)


# ---- 9: the loop the feature exists for ------------------------------------------------------------------------
def _loop(engine, corrupt=(), close_early=None):
    """37 connections with transfers of 1 to 40 buffers; per tick send -> verify_at -> accounting over the tick's own
    descriptors, all on one stream with nothing read back; then the close. corrupt: (tick, tick-local slot) pairs
    whose first byte is flipped between the tick and the verify."""
    n_conns, B, stride, max_buffers = 37, 1000, 1008, 3
    rng = np.random.default_rng(9)
    settings = [(int(rng.integers((k - 1) * B + 1, k * B + 1)), B) for k in [1, 40] + list(rng.integers(1, 41, 35))]
    buffers = [-(-t // B) for t, _ in settings]
    capacity = n_conns * max_buffers
    table = T.SenderTable(engine, settings, stride, capacity, fill=0xA5)
    ids = list(range(n_conns))
    dev_ids = _ids(ids)
    cff = torch.full((n_conns,), -1, dtype=torch.int32, device=DEV)
    state, ref, ctr, block = (engine.new_conn_state(n_conns), engine.new_counters(), engine.new_counters(),
                              engine.new_counters())
    results = engine.new_conn_results(n_conns)
    entries = W.tcp_sender_entries(settings)
    arena = np.zeros(capacity * stride, dtype=np.uint8)
    base, first_fail, recv_until = 0, {}, {}
    ticks_needed = max(-(-b // max_buffers) for b in buffers)
    closed_early = {}
    for t in range(ticks_needed):
        v = W.tcp_sender_view(entries, stride, arena, 0, capacity, ids, max_buffers)  # the host's own arithmetic
        entries, n = v.entries, v.tick["buffers"]
        table.send(dev_ids, max_buffers)
        for (ct, g) in corrupt:
            if ct == t:
                table.arena[g * stride] ^= 0xFF
                c = int(v.descs["conn_index"][g])
                first_fail.setdefault(c, base + g)
        descs = table.descs_of(n)
        engine.verify(table.arena, descs, max_length_hint=stride, counters=ctr, conn_first_fail=cff, base_index=base)
        engine.refview_conns(table.arena.numel(), descs, ref, state, base_index=base, conn_first_fail=cff)
        for g in range(n):  # what each connection has received up to and including its first failing buffer
            c = int(v.descs["conn_index"][g])
            if c not in first_fail or base + g <= first_fail[c]:
                recv_until[c] = recv_until.get(c, 0) + int(v.descs["length"][g])
        base += n
        if close_early is not None and t == ticks_needed - 2:
            closed_early = dict(recv_until)
            early = engine.new_conn_results(1)
            engine.conns_close(_ids([close_early]), _u64([settings[close_early][0]]), cff, state, block, results=early)
    assert int(entries["finished"].sum()) == n_conns
    engine.conns_close(dev_ids, _u64([t for t, _ in settings]), cff, state, block, results=results)
    torch.cuda.synchronize()
    res = results.cpu().numpy().view(CONN_RESULT_DTYPE)
    dev_entries, _, _ = table.read()
    assert np.array_equal(dev_entries, entries)
    sent = table.read_sent()
    assert sent["bytes_sent"] == sum(t for t, _ in settings) and sent["buffers_sent"] == sum(buffers) == base
    assert sent["connections_finished"] == n_conns
    early_res = early.cpu().numpy().view(CONN_RESULT_DTYPE)[0] if close_early is not None else None
    return settings, res, engine.read_counters_close(block), first_fail, recv_until, early_res, closed_early


def test_send_verify_account_close(engine):
    settings, res, close, _, recv, _, _ = _loop(engine)
    assert (res["status"] == 0).all() and (res["first_fail"] == EMPTY).all() and (res["flags"] == 0).all()
    assert res["bytes_recv"].tolist() == [t for t, _ in settings]
    assert close["connections_closed"] == close["successful"] == 37
    assert close["bytes_recv"] == sum(t for t, _ in settings)


def test_send_verify_account_close_with_two_data_errors(engine):
    # tick 0 slot 4 (connection 2's first burst) and tick 2 slot 1 (connection 1's third burst)
    settings, res, close, first_fail, recv, _, _ = _loop(engine, corrupt=[(0, 4), (2, 1)])
    assert len(first_fail) == 2
    for c in range(37):
        if c in first_fail:
            assert int(res["status"][c]) == DATA_ERROR and int(res["first_fail"][c]) == first_fail[c], c
            assert int(res["bytes_recv"][c]) == recv[c], c
        else:
            assert int(res["status"][c]) == 0 and int(res["bytes_recv"][c]) == settings[c][0], c
    assert int(res["bytes_recv"][1]) == 8000 < settings[1][0]  # its 8th buffer failed; 32 more were verified
    assert int(res["buffers_after_failure"][1]) == 32
    assert close["data_errors"] == 2 and close["successful"] == 35


def test_send_verify_account_close_one_early(engine):
    settings, res, close, _, recv, early, recv_early = _loop(engine, close_early=1)  # connection 1: 40 buffers
    assert int(early["status"]) == NOT_ALL_DATA and int(early["conn_index"]) == 1
    assert int(early["bytes_recv"]) == recv_early[1] < settings[1][0]
    # its last buffer arrived in the recycled slot: a second, short connection
    assert int(res["status"][1]) == NOT_ALL_DATA and int(res["bytes_recv"][1]) == settings[1][0] - 39000
    assert close["not_all_data"] == 2 and close["successful"] == 36 and close["connections_closed"] == 38
