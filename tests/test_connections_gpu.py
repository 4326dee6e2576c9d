"""GPU: connections on the device (include/cts_connections.h): the reference view per connection
(cts_refview_accumulate_conns), the close that classifies, reports and recycles connection slots (cts_conns_close),
the slot rebase (cts_conn_slots_rebase) and the *_close reads, against the models of ctstraffic_amd.workload
(connection_view, close_results, rebase_slots).

The plans and their arenas are those of tests/test_refview_gpu.py (its cache is shared); the failed mask behind every
model always comes from oracle.verify_batch on the materialised bytes. Integer work: every comparison is exact.
"""
import numpy as np
import pytest

import connection_plans as C
import oracle
import refview_plans as P
import test_refview_gpu as R
from ctstraffic_amd import _lib
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import CONN_RESULT_DTYPE, CONN_RESULT_FLAG_BAD_CONN, CONN_STATE_DTYPE, DESC_DTYPE

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
EMPTY = 0xFFFFFFFF
_dev, _slots, _u32 = R._dev, R._slots, R._u32


def _table(t):
    return t.cpu().numpy().view(CONN_STATE_DTYPE)


def _results(t):
    return t.cpu().numpy().view(CONN_RESULT_DTYPE)


def _u32_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(DEV)


def _u64_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(DEV)


_plans = {}


def _plan(engine, name):
    """A plan of tests/test_refview_gpu.py on the device, with its ordinals and the model's table."""
    if name not in _plans:
        w, launches, arena, dd, octr, sums, slots, facts = R._materialised(engine, name)
        ordinals = np.zeros(w.n, dtype=np.int64)
        for d, base, idx in launches:
            ordinals[idx] = base + np.arange(len(idx))
        table, _ = W.connection_view(w.descs, None, ordinals, w.n_conns, slots=slots)
        for f in CONN_STATE_DTYPE.names:
            assert int(table[f].sum()) == sums[f]
        _plans[name] = (w, launches, arena, dd, ordinals, sums, slots, table, facts)
    return _plans[name]


def _run(engine, w, arena, launches, dd, variant="queued", ordinal_shift=0, tables=None, only=None):
    """Verify + the _conns pass over a plan's launches; returns the device objects (ctr, ref, cff, state)."""
    ctr, ref, cff, state = tables or (engine.new_counters(), engine.new_counters(), _slots(w.n_conns),
                                      engine.new_conn_state(w.n_conns))
    kw = dict(max_length_hint=w.max_length, counters=ctr, conn_first_fail=cff)
    order = list(range(len(launches))) if only is None else list(only)
    if variant == "reverse":  # every verify first, latest ordinals first, then the passes
        for k in reversed(order):
            engine.verify(arena, dd[k], base_index=launches[k][1] + ordinal_shift, **kw)
        for k in order:
            engine.refview_conns(w.arena_bytes, dd[k], ref, state, base_index=launches[k][1] + ordinal_shift,
                                 conn_first_fail=cff)
    else:
        for k in order:
            engine.verify(arena, dd[k], base_index=launches[k][1] + ordinal_shift, **kw)
            engine.refview_conns(w.arena_bytes, dd[k], ref, state, base_index=launches[k][1] + ordinal_shift,
                                 conn_first_fail=cff)
    return ctr, ref, cff, state


# ---- 1. the three plans ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ("queued", "reverse"))
@pytest.mark.parametrize("name", ("wg", "ragged", "quad"))
def test_plans_table_and_block(engine, name, variant):
    """The plans of the reference-view tests in their launches: the table equals connection_view, the block equals
    reference_view and, word for word, what cts_refview_accumulate gives over the same launches."""
    w, launches, arena, dd, ordinals, sums, slots, table, facts = _plan(engine, name)
    ctr, ref, cff, state = _run(engine, w, arena, launches, dd, variant)
    plain = engine.new_counters()
    for k, (_, base, _) in enumerate(launches):
        engine.refview(w.arena_bytes, dd[k], plain, base_index=base, conn_first_fail=cff)
    torch.cuda.synchronize()
    view = engine.read_counters_ref(ref)
    print(name, variant, view)
    assert np.array_equal(_u32(cff), slots)
    assert np.array_equal(_table(state), table)
    assert view == sums == engine.read_counters_ref(plain)
    assert view["buffers_failed"] == engine.read_counters_ex(ctr)["connections_failed"] == facts["failed"]


# ---- 2. no runs -----------------------------------------------------------------------------------------------------
def test_buffer_major_order_has_no_runs(engine):
    """The wg descriptors buffer-major (buffer k of every connection, then k + 1), ordinals = positions: neighbouring
    lanes always differ in connection, and the table and the block are the plan's."""
    w, launches, arena, dd, ordinals, sums, slots, table, facts = _plan(engine, "wg")
    order = C.buffer_major(w.n_conns, 48)
    d = w.descs[order]
    assert (d["conn_index"][1:] != d["conn_index"][:-1]).all()
    want_slots = C.slots_under(slots, ordinals, order)
    t2, _ = W.connection_view(d, None, np.arange(w.n), w.n_conns, slots=want_slots)
    assert np.array_equal(t2, table)
    ctr, ref, cff, state = _run(engine, w, arena, [(d, 0, order)], [_dev(d)])
    torch.cuda.synchronize()
    assert np.array_equal(_u32(cff), want_slots)
    assert np.array_equal(_table(state), table)
    assert engine.read_counters_ref(ref) == sums


# ---- 3. ragged runs -------------------------------------------------------------------------------------------------
def test_ragged_runs_and_partial_last_tiles(engine):
    """The quad plan with a seeded third of its descriptors dropped (a connection's order kept, ordinals = positions):
    run lengths vary and runs straddle tiles, wave spans and workgroups; at n, n - 1, n - 63, n - 64 and n - 65
    descriptors the last tile of the last span is partial in every way."""
    w, launches, arena, dd, ordinals, sums, slots, table, facts = _plan(engine, "quad")
    keep = np.random.default_rng(0xD209).random(w.n) >= 1.0 / 3.0
    d = np.ascontiguousarray(w.descs[keep])
    n = len(d)
    assert 0.6 * w.n < n < 0.72 * w.n
    res, _, _ = oracle.verify_batch(arena.cpu().numpy(), d, n_conns=w.n_conns)
    failed = (res["pass"] == 0) & (res["flags"] == 0)
    assert failed.sum() > 40
    lens = np.diff(np.nonzero(np.r_[True, d["conn_index"][1:] != d["conn_index"][:-1], True])[0])
    assert lens.min() < 35 and lens.max() > 50 and len(lens) == w.n_conns
    for m in (n, n - 1, n - 63, n - 64, n - 65):
        sub = d[:m]
        want, want_slots = W.reference_view(sub, failed[:m], np.arange(m), w.n_conns)
        want_table, _ = W.connection_view(sub, failed[:m], np.arange(m), w.n_conns)
        ctr, ref, cff, state = _run(engine, w, arena, [(sub, 0, None)], [_dev(sub)])
        torch.cuda.synchronize()
        assert np.array_equal(_u32(cff), want_slots), m
        assert np.array_equal(_table(state), want_table), m
        assert engine.read_counters_ref(ref) == want, m


# ---- 4. one long run, the pass alone --------------------------------------------------------------------------------
def test_one_connection_ring_the_pass_alone(engine):
    """A strided ring of 1 000 003 lengths of one connection and synthetic slots (failing ordinal in the middle, at the
    first ordinal, at the last one, none): every wave's span is one run that is carried from tile to tile."""
    rng = np.random.default_rng(0xC0221)
    n, stride, skip, base = 1000003, 1536, 26, 5000
    lens = rng.integers(0, stride + 40, size=n).astype(np.uint32)  # some below skip, some above the stride: bad
    ring_bytes = n * stride
    sd = np.zeros(n, dtype=DESC_DTYPE)
    sd["byte_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    sd["length"], sd["skip_head"], sd["conn_index"] = lens, skip, 1
    bad = W.descs_bad(sd, ring_bytes) | (lens > stride)
    assert 1000 < bad.sum() < n // 10
    lens_d = torch.from_numpy(lens.view(np.int32).copy()).to(DEV)
    g = base + np.arange(n)
    for slot in (base + n // 2, base, base + n - 1, EMPTY):
        slots = np.array([7, slot, EMPTY], dtype=np.uint32)
        want, _ = W.reference_view(sd, None, g, 3, bad=bad, slots=slots)
        want_table, _ = W.connection_view(sd, None, g, 3, bad=bad, slots=slots)
        assert want_table["buffers_recv"][1] + want_table["buffers_after_failure"][1] == int((~bad).sum())
        for nt in (1, 0):
            engine.set_attr(_lib.ATTR_NT_LOADS, nt)
            try:
                ref, state, cff = engine.new_counters(), engine.new_conn_state(3), _u32_dev(slots)
                engine.refview_conns_strided(ring_bytes, stride, lens_d, ref, state, skip_head=skip, conn_index=1,
                                             base_index=base, conn_first_fail=cff)
                torch.cuda.synchronize()
            finally:
                engine.set_attr(_lib.ATTR_NT_LOADS, 1)
            assert np.array_equal(_table(state), want_table), (slot, nt)
            assert engine.read_counters_ref(ref) == want, (slot, nt)
            assert np.array_equal(_u32(cff), slots)  # the pass only reads the slots
    # a ring whose connection has no slot counts in the block and in no entry
    ref, state = engine.new_counters(), engine.new_conn_state(3)
    engine.refview_conns_strided(ring_bytes, stride, lens_d, ref, state, skip_head=skip, conn_index=3, base_index=base,
                                 conn_first_fail=_u32_dev([0, 0, 0]))
    got = engine.read_counters_ref(ref)
    assert got["buffers_recv"] == int((~bad).sum()) and got["buffers_after_failure"] == 0
    assert not _table(state).view(np.uint64).any()


def test_seven_connections_in_long_runs_the_pass_alone(engine):
    """1 000 003 synthetic descriptors of 7 connections in runs of 1 to 200 000, no arena behind them."""
    rng = np.random.default_rng(0x7C0)
    n, n_conns, base, arena_bytes = 1000003, 7, 77, 1 << 40
    d = np.zeros(n, dtype=DESC_DTYPE)
    d["conn_index"] = C.runs_of(n, n_conns, 200000, rng)
    assert len(np.unique(d["conn_index"])) == n_conns
    d["length"] = rng.integers(0, 70000, size=n)
    d["expected_pattern_offset"] = rng.integers(0, 65536, size=n)
    d["byte_offset"] = rng.integers(0, arena_bytes - 70000, size=n).astype(np.uint64)
    g = base + np.arange(n)
    at = [np.nonzero(d["conn_index"] == c)[0] for c in range(n_conns)]
    # empty; a connection's first buffer, its last, one inside; below the batch, above it; one inside
    slots = np.array([EMPTY, g[at[1][0]], g[at[2][-1]], g[at[3][len(at[3]) // 2]], 3, base + n,
                      g[at[6][len(at[6]) // 3]]], dtype=np.uint32)
    want, _ = W.reference_view(d, None, g, n_conns, slots=slots)
    want_table, _ = W.connection_view(d, None, g, n_conns, slots=slots)
    assert min(want.values()) > 0
    ref, state = engine.new_counters(), engine.new_conn_state(n_conns)
    engine.refview_conns(arena_bytes, _dev(d), ref, state, base_index=base, conn_first_fail=_u32_dev(slots))
    torch.cuda.synchronize()
    assert np.array_equal(_table(state), want_table)
    assert engine.read_counters_ref(ref) == want


# ---- 5. bad descriptors and slotless connections --------------------------------------------------------------------
def test_bad_descriptors_and_slotless_connections(engine):
    """Buffers with conn_index >= n_conns count in the block and in no entry; bad descriptors count nowhere; then one
    descriptor, and 63."""
    rng = np.random.default_rng(0xBADC)
    arena_bytes, n_conns, base = 1 << 40, 5000, 123457
    d, bad, g, slots = R._synthetic(100003, n_conns, base, rng, arena_bytes)
    assert bad.sum() > 500 and (d["conn_index"] >= n_conns).sum() > 100
    want, _ = W.reference_view(d, None, g, n_conns, bad=bad, slots=slots)
    want_table, _ = W.connection_view(d, None, g, n_conns, bad=bad, slots=slots)
    vlen = d["length"].astype(np.int64) - d["skip_head"].astype(np.int64)
    inside = ~bad & (d["conn_index"] < n_conns)
    assert int(want_table["bytes_recv"].sum() + want_table["bytes_after_failure"].sum()) == int(vlen[inside].sum())
    assert want["bytes_recv"] + want["bytes_after_failure"] == int(vlen[~bad].sum()) > int(vlen[inside].sum())
    ref, plain, state = engine.new_counters(), engine.new_counters(), engine.new_conn_state(n_conns)
    cff, dd = _u32_dev(slots), _dev(d)
    engine.refview_conns(arena_bytes, dd, ref, state, base_index=base, conn_first_fail=cff)
    engine.refview(arena_bytes, dd, plain, base_index=base, conn_first_fail=cff)
    torch.cuda.synchronize()
    assert np.array_equal(_table(state), want_table)
    assert engine.read_counters_ref(ref) == want == engine.read_counters_ref(plain)
    for m in (1, 63):
        sub = d[~bad][:m].copy()
        sub["conn_index"] = 2
        ref, state = engine.new_counters(), engine.new_conn_state(4)
        engine.refview_conns(arena_bytes, _dev(sub), ref, state, base_index=10,
                             conn_first_fail=_u32_dev([EMPTY, EMPTY, 10, EMPTY]))
        v = sub["length"].astype(np.int64) - sub["skip_head"].astype(np.int64)
        assert [tuple(int(x) for x in r) for r in _table(state)] == \
            [(0,) * 4, (0,) * 4, (int(v[0]), 1, int(v[1:].sum()), m - 1), (0,) * 4]
        assert engine.read_counters_ref(ref)["buffers_failed"] == 1


# ---- 6. close -------------------------------------------------------------------------------------------------------
def _closed_plan(engine):
    w, launches, arena, dd, ordinals, sums, slots, table, facts = _plan(engine, "wg")
    ctr, ref, cff, state = _run(engine, w, arena, launches, dd)
    return w, slots, table, C.expected_bytes(table, slots), cff, state


def _check_close(engine, got, model, cff, state, blk):
    res, counts, state2, slots2 = model
    torch.cuda.synchronize()
    if got is not None:
        assert np.array_equal(_results(got), res)
    assert engine.read_counters_close(blk) == counts
    assert np.array_equal(_u32(cff), slots2) and np.array_equal(_table(state), state2)


def test_close_all_connections(engine):
    """After the wg plan, all 96 connections closed in one call: results, the close block and the emptied slots and
    entries equal close_results; all four classes occur."""
    w, slots, table, want, cff, state = _closed_plan(engine)
    ids = np.arange(w.n_conns, dtype=np.uint32)
    model = W.close_results(table, slots, ids, want)
    counts = model[1]
    print(counts)
    assert min(counts[f] for f in ("successful", "data_errors", "not_all_data", "too_much_data")) > 0
    assert counts["connections_closed"] == 96 and counts["data_errors"] == 73
    blk, out = engine.new_counters(), engine.new_conn_results(len(ids))
    engine.conns_close(_u32_dev(ids), _u64_dev(want), cff, state, blk, results=out)
    _check_close(engine, out, model, cff, state, blk)
    assert (_u32(cff) == EMPTY).all() and not _table(state).view(np.uint64).any()
    # closing the emptied slots again: 96 fresh connections that received nothing
    engine.conns_close(_u32_dev(ids), None, cff, state, blk, results=out)
    torch.cuda.synchronize()
    again = engine.read_counters_close(blk)
    assert again["connections_closed"] == 192 and again["successful"] == counts["successful"] + 96
    assert again["bytes_recv"] == counts["bytes_recv"] and not _results(out)["status"].any()


def test_close_without_sizes(engine):
    w, slots, table, want, cff, state = _closed_plan(engine)
    ids = np.arange(w.n_conns, dtype=np.uint32)[::-1]
    model = W.close_results(table, slots, ids, None)
    assert model[1]["not_all_data"] == model[1]["too_much_data"] == 0 and model[1]["successful"] == 23
    blk, out = engine.new_counters(), engine.new_conn_results(len(ids))
    engine.conns_close(_u32_dev(ids), None, cff, state, blk, results=out)
    _check_close(engine, out, model, cff, state, blk)


def test_close_with_an_id_that_has_no_slot(engine):
    w, slots, table, want, cff, state = _closed_plan(engine)
    ids = np.r_[np.arange(40), 96, np.arange(40, 96), EMPTY].astype(np.uint32)
    exp = np.r_[want[:40], 5, want[40:], 5].astype(np.uint64)
    model = W.close_results(table, slots, ids, exp)
    assert model[1]["connections_closed"] == 96
    assert model[0]["flags"].tolist() == [0] * 40 + [CONN_RESULT_FLAG_BAD_CONN] + [0] * 56 + [CONN_RESULT_FLAG_BAD_CONN]
    blk, out = engine.new_counters(), engine.new_conn_results(len(ids))
    engine.conns_close(_u32_dev(ids), _u64_dev(exp), cff, state, blk, results=out)
    _check_close(engine, out, model, cff, state, blk)
    assert tuple(int(x) for x in _results(out)[40]) == (0, 0, 0, 0, 0, 0, 96, CONN_RESULT_FLAG_BAD_CONN)


def test_close_without_results(engine):
    w, slots, table, want, cff, state = _closed_plan(engine)
    ids = np.arange(w.n_conns, dtype=np.uint32)
    blk = engine.new_counters()
    engine.conns_close(_u32_dev(ids), _u64_dev(want), cff, state, blk)
    _check_close(engine, None, W.close_results(table, slots, ids, want), cff, state, blk)


def test_close_a_subset_leaves_the_others(engine):
    w, slots, table, want, cff, state = _closed_plan(engine)
    ids = np.random.default_rng(5).permutation(w.n_conns)[:31].astype(np.uint32)
    model = W.close_results(table, slots, ids, want[ids])
    keep = np.ones(w.n_conns, bool)
    keep[ids] = False
    assert (model[3][keep] != EMPTY).any() and (model[3][~keep] == EMPTY).all()
    blk, out = engine.new_counters(), engine.new_conn_results(len(ids))
    engine.conns_close(_u32_dev(ids), _u64_dev(want[ids]), cff, state, blk, results=out)
    _check_close(engine, out, model, cff, state, blk)
    assert np.array_equal(_u32(cff)[keep], slots[keep]) and np.array_equal(_table(state)[keep], table[keep])
    # the rest, later: the block then holds every connection once
    rest = np.nonzero(keep)[0].astype(np.uint32)
    m2 = W.close_results(model[2], model[3], rest, want[rest])
    engine.conns_close(_u32_dev(rest), _u64_dev(want[rest]), cff, state, blk)
    torch.cuda.synchronize()
    assert engine.read_counters_close(blk) == {f: model[1][f] + m2[1][f] for f in model[1]} == \
        W.close_results(table, slots, np.arange(w.n_conns), want)[1]


# ---- 7. recycling ---------------------------------------------------------------------------------------------------
_gen2 = {}


def _second_generation(engine):
    """The wg shapes with another seed_corrupt: the connections that take over the slots."""
    if not _gen2:
        kw, parts, _ = P.PLANS["wg"]
        w = W.connection_streams(**dict(kw, seed_corrupt=0x2BAD))
        launches = W.stream_launches(w.descs, kw["buffers_per_conn"], parts)
        arena, _ = W.materialize(engine, w)
        torch.cuda.synchronize()
        res, _, _ = oracle.verify_batch(arena.cpu().numpy(), w.descs, n_conns=w.n_conns, nthreads=8)
        _gen2["v"] = (w, launches, arena, [_dev(d) for d, _, _ in launches], (res["pass"] == 0) & (res["flags"] == 0))
    return _gen2["v"]


def test_recycled_slots_carry_the_next_connections(engine):
    """The plan, everything closed, then the same shapes with other corruptions through the same slots (ordinals go on
    from the first generation's count), closed again: each generation's results equal its own model,
    connections_failed adds up over both and the close block holds both."""
    w, launches, arena, dd, ordinals, sums, slots, table, facts = _plan(engine, "wg")
    w2, launches2, arena2, dd2, failed2 = _second_generation(engine)
    ordinals2 = np.zeros(w2.n, dtype=np.int64)
    for d, base, idx in launches2:
        ordinals2[idx] = w.n + base + np.arange(len(idx))
    sums2, slots2 = W.reference_view(w2.descs, failed2, ordinals2, w2.n_conns)
    table2, _ = W.connection_view(w2.descs, failed2, ordinals2, w2.n_conns)
    f1, f2 = facts["failed"], int((slots2 != EMPTY).sum())
    assert f2 > 0 and not np.array_equal(slots2 == EMPTY, slots == EMPTY)  # other connections fail
    ids = np.arange(w.n_conns, dtype=np.uint32)
    blk = engine.new_counters()
    tables = _run(engine, w, arena, launches, dd)
    ctr, ref, cff, state = tables
    want1 = C.expected_bytes(table, slots)
    m1 = W.close_results(table, slots, ids, want1)
    out1 = engine.new_conn_results(len(ids))
    engine.conns_close(_u32_dev(ids), _u64_dev(want1), cff, state, blk, results=out1)
    _run(engine, w2, arena2, launches2, dd2, ordinal_shift=w.n, tables=tables)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(cff), slots2) and np.array_equal(_table(state), table2)
    want2 = C.expected_bytes(table2, slots2)
    m2 = W.close_results(table2, slots2, ids, want2)
    out2 = engine.new_conn_results(len(ids))
    engine.conns_close(_u32_dev(ids), _u64_dev(want2), cff, state, blk, results=out2)
    torch.cuda.synchronize()
    assert np.array_equal(_results(out1), m1[0]) and np.array_equal(_results(out2), m2[0])
    assert engine.read_counters_ex(ctr)["connections_failed"] == f1 + f2
    assert engine.read_counters_ref(ref) == {f: sums[f] + sums2[f] for f in sums}
    both = {f: m1[1][f] + m2[1][f] for f in m1[1]}
    assert engine.read_counters_close(blk) == both and both["data_errors"] == f1 + f2
    assert (_u32(cff) == EMPTY).all() and not _table(state).view(np.uint64).any()


# ---- 8. rebase ------------------------------------------------------------------------------------------------------
def test_rebase_between_launches(engine):
    """wg launches 1 and 2, a rebase by 3 071, then launch 3 with base_index 1: the slots are rebase_slots of the
    unrebased run's, the block and the table the unrebased run's."""
    w, launches, arena, dd, ordinals, sums, slots, table, facts = _plan(engine, "wg")
    assert launches[2][1] == 3072
    tables = _run(engine, w, arena, launches, dd, only=(0, 1))
    ctr, ref, cff, state = tables
    engine.slots_rebase(cff, 3071)
    engine.verify(arena, dd[2], base_index=1, max_length_hint=w.max_length, counters=ctr, conn_first_fail=cff)
    engine.refview_conns(w.arena_bytes, dd[2], ref, state, base_index=1, conn_first_fail=cff)
    torch.cuda.synchronize()
    want = W.rebase_slots(slots, 3071)
    assert (want[slots != EMPTY] < 1537).all() and (want == 0).sum() == 34 + 24  # launches 1 and 2's failures
    assert np.array_equal(_u32(cff), want)
    assert np.array_equal(_table(state), table)
    assert engine.read_counters_ref(ref) == sums
    assert engine.read_counters_ex(ctr)["connections_failed"] == facts["failed"]


def test_rebase_kernel_alone(engine):
    """Synthetic slots: empty, 0, delta - 1, delta, 0xFFFFFFFE, for deltas up to 0xFFFFFFFE; more slots than a
    workgroup, and more than the grid's lanes."""
    rng = np.random.default_rng(0x2EBA)
    for delta in (1, 2, 3071, 1 << 31, EMPTY - 1):
        s = np.array([EMPTY, 0, delta - 1, delta, EMPTY - 1, EMPTY, min(delta + 1, EMPTY - 1)], dtype=np.uint32)
        t = _u32_dev(s)
        engine.slots_rebase(t, delta)
        assert _u32(t).tolist() == W.rebase_slots(s, delta).tolist()
        assert _u32(t).tolist()[:5] == [EMPTY, 0, 0, 0, EMPTY - 1 - delta]
    for n in (257, 700001):
        s = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        s[rng.random(n) < 0.3] = EMPTY
        t = _u32_dev(s)
        engine.slots_rebase(t, 1 << 30)
        assert np.array_equal(_u32(t), W.rebase_slots(s, 1 << 30))
    t = _u32_dev(s)
    engine.slots_rebase(t, 0)
    assert np.array_equal(_u32(t), s)


# ---- 9. folds -------------------------------------------------------------------------------------------------------
def _folds_main(q):
    """Close blocks of two engines on this GPU through the three reads; run in a child so RCCL's threads end with
    it."""
    try:
        from ctstraffic_amd import Engine
        from ctstraffic_amd.engine import (counters_allreduce_close, counters_allreduce_release,
                                           counters_read_multi_close)

        torch.cuda.set_device(0)
        out = {}
        with Engine(0) as e0, Engine(0) as e1:
            blocks, exps = [], []
            for k, eng in enumerate((e0, e1)):
                w = W.connection_streams(world=2, rank=k, n_conns=64, buffers_per_conn=8, length=65536,
                                         corrupt_rate=9 + k)
                arena, _ = W.materialize(eng, w, device="cuda:0")
                res, _, _ = oracle.verify_batch(arena.cpu().numpy(), w.descs, n_conns=w.n_conns)
                failed = (res["pass"] == 0) & (res["flags"] == 0)
                ctr, ref, blk = eng.new_counters(), eng.new_counters(), eng.new_counters()
                cff = torch.full((w.n_conns,), -1, dtype=torch.int32, device="cuda:0")
                state = eng.new_conn_state(w.n_conns)
                dd = _dev(w.descs)
                eng.verify(arena, dd, max_length_hint=65536, counters=ctr, conn_first_fail=cff)
                eng.refview_conns(w.arena_bytes, dd, ref, state, conn_first_fail=cff)
                table, slots = W.connection_view(w.descs, failed, np.arange(w.n), w.n_conns)
                ids = np.unique(w.descs["conn_index"]).astype(np.uint32)  # this rank's connections
                want = C.expected_bytes(table, slots)[ids]
                eng.conns_close(_u32_dev(ids), _u64_dev(want), cff, state, blk)
                torch.cuda.synchronize()
                blocks.append(blk)
                exps.append(W.close_results(table, slots, ids, want)[1])
            both = {f: exps[0][f] + exps[1][f] for f in exps[0]}
            out["read"] = (e0.read_counters_close(blocks[0]), exps[0])
            out["multi"] = (counters_read_multi_close([e0, e1], blocks), both)
            try:
                out["allreduce"] = (counters_allreduce_close([e0, e1], blocks), both)
                out["allreduce_one"] = (counters_allreduce_close([e1], blocks[1:]), exps[1])
                counters_allreduce_release()
            except _lib.CtsError as e:
                if e.status != _lib.CTS_E_UNAVAILABLE:
                    raise
                out["allreduce"] = None
        q.put(out)
    except Exception as e:  # pragma: no cover
        import traceback

        q.put(("error", repr(e) + traceback.format_exc()))


def test_close_blocks_through_the_three_folds():
    """read_counters_close, counters_read_multi_close and counters_allreduce_close (the RCCL all-reduce of count 6) over
    close blocks agree with the model, with one engine and with two engines on one device."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_folds_main, args=(q,), daemon=True)
    p.start()
    try:
        r = q.get(timeout=100)
        p.join(15)
    finally:
        if p.is_alive():
            p.kill()
            p.join(5)
    assert not (isinstance(r, tuple) and r[0] == "error"), r[1]
    got, exp = r["read"]
    assert got == exp and exp["data_errors"] > 0 and exp["connections_closed"] == sum(
        exp[f] for f in ("successful", "data_errors", "not_all_data", "too_much_data"))
    got, exp = r["multi"]
    assert got == exp and exp["connections_closed"] == 64
    assert p.exitcode == 0
    if r["allreduce"] is None:
        pytest.skip("RCCL is not available: the all-reduce of the close blocks was not run")
    got, exp = r["allreduce"]
    assert got == exp
    got, exp = r["allreduce_one"]
    assert got == exp


# ---- 10. the status line --------------------------------------------------------------------------------------------
def test_status_line_from_the_close_block(engine):
    """Two status ticks on the device-resident path, a group of connections closed before each: Completed and DataError
    of the TCP status line (ctsSocketState.cpp:221-228) are the close block's successful and data_errors + not_all_data
    + too_much_data, added as deltas; the lines equal the ones built from the model's counts."""
    from ctstraffic_amd import status as S

    w, slots, table, want, cff, state = _closed_plan(engine)
    groups = [np.arange(0, 40, dtype=np.uint32), np.arange(40, 96, dtype=np.uint32)]
    blk = engine.new_counters()
    last = dict.fromkeys(W.CLOSE_FIELDS, 0)
    st = dict(successful=0, protocol_errors=0)
    m_state, m_slots, m_ok, m_err = table, slots, 0, 0
    for tick, ids in enumerate(groups):
        engine.conns_close(_u32_dev(ids), _u64_dev(want[ids]), cff, state, blk)
        node = engine.read_counters_close(blk)
        st["successful"] += node["successful"] - last["successful"]
        st["protocol_errors"] += sum(node[f] - last[f] for f in ("data_errors", "not_all_data", "too_much_data"))
        d_bytes = node["bytes_recv"] - last["bytes_recv"]
        last = node
        line = S.line(S.CSV, current_time_ms=1000 * (tick + 1), start_time_ms=1000 * tick,
                      end_time_ms=1000 * (tick + 1), bytes_sent=0, bytes_recv=d_bytes,
                      active_connections=96 - node["connections_closed"], connection_errors=0, **st)
        _, counts, m_state, m_slots = W.close_results(m_state, m_slots, ids, want[ids])
        m_ok += counts["successful"]
        m_err += counts["data_errors"] + counts["not_all_data"] + counts["too_much_data"]
        done = sum(len(g) for g in groups[:tick + 1])
        assert m_ok + m_err == done and m_ok > 0 and m_err > 0
        assert line == "%d.000,0,%d,%d,%d,0,%d\r\n" % (tick + 1, counts["bytes_recv"], 96 - done, m_ok, m_err)
    total = W.close_results(table, slots, np.arange(96), want)[1]
    assert (st["successful"], st["protocol_errors"]) == (total["successful"], 96 - total["successful"])
    assert st["protocol_errors"] > engine.read_counters_close(blk)["data_errors"] == 73  # not only data mismatches
    s = S.summary(st["successful"], 0, st["protocol_errors"], total["bytes_recv"], 0)
    assert "ProtocolErrors [%d]" % st["protocol_errors"] in s and "Total Bytes Recv : %d" % total["bytes_recv"] in s
