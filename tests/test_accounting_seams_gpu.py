"""GPU: the accounting kernels (refview_accumulate, conn_accumulate, conn_close, ms_conn_accumulate, ms_conn_render,
ms_conn_close) where the older tests do not reach: wave spans of five tiles, so that parked sums are joined inside a
wave's loop, and values of 2^32 and more in every on-chip sum.

The batches come from tests/accounting_plans.py, built for the device's own count of compute units; every test first
asserts, with the walk of that module, that its batch takes every path of a wave's walk, then compares with the models
of ctstraffic_amd.workload and the numpy restatements of accounting_plans (held to Python-integer loops and to the
MediaStream connection view in tests/test_accounting_seams_cpu.py). None of these passes reads an arena: the
descriptors are synthetic. Integer work: every comparison is exact.
"""
import numpy as np
import pytest

import accounting_plans as A
from ctstraffic_amd import _lib
from ctstraffic_amd import media_stream as M
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import (CONN_RESULT_DTYPE, CONN_STATE_DTYPE, DESC_DTYPE, MS_CONN_RESULT_DTYPE,
                                  MS_CONN_STATE_DTYPE)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EMPTY = A.KNONE


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bytes_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)


def _u32_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(DEV)


def _u64_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(DEV)


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _nt(engine, on):
    engine.set_attr(_lib.ATTR_NT_LOADS, on)


_expected = {}


def _plan(tail):
    """The plan for this device, with the models' view of it: computed once."""
    if tail not in _expected:
        p = A.plan(_cus(), tail)
        ref, _ = W.reference_view(p.descs, None, p.ordinals, p.n_conns, bad=p.bad, slots=p.slots)
        table, _ = W.connection_view(p.descs, None, p.ordinals, p.n_conns, bad=p.bad, slots=p.slots)
        _expected[tail] = (p, ref, table)
    return _expected[tail]


# ---- 1. conn_accumulate over the plan -------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", (1, 0))
@pytest.mark.parametrize("tail", ("run", "mixed"))
def test_connections_over_long_spans(engine, tail, nt):
    """cts_refview_accumulate_conns over plan(cus, tail): spans of five tiles with every transition of the walk, lengths
    up to 2^32 - 1. The table equals connection_view, the block reference_view and what cts_refview_accumulate gives
    over the same descriptors, and the slots are only read."""
    p, want, want_table = _plan(tail)
    counts = p.walked["counts"]
    print(tail, nt, p.n, counts, want)
    assert p.walked["span"] == 320 and A.covered(counts) == []
    assert min(want.values()) > 0 and want["bytes_recv"] > 1 << 46
    # a switch inside a parked tile, at a seam: the received and the after-failure sums both grow there
    assert (want_table["bytes_recv"][3:] > 1 << 40).all() and (want_table["bytes_after_failure"][3:] > 1 << 40).all()
    dd, cff = _bytes_dev(p.descs), _u32_dev(p.slots)
    ref, plain, state = engine.new_counters(), engine.new_counters(), engine.new_conn_state(p.n_conns)
    _nt(engine, nt)
    try:
        engine.refview_conns(p.arena_bytes, dd, ref, state, base_index=p.base_index, conn_first_fail=cff)
        engine.refview(p.arena_bytes, dd, plain, base_index=p.base_index, conn_first_fail=cff)
        torch.cuda.synchronize()
    finally:
        _nt(engine, 1)
    got_table = _host(state, CONN_STATE_DTYPE)
    for f in CONN_STATE_DTYPE.names:
        assert got_table[f].tolist() == want_table[f].tolist(), f
    assert engine.read_counters_ref(ref) == want
    assert engine.read_counters_ref(plain) == want
    assert np.array_equal(_host(cff, np.uint32), p.slots)


def test_connections_without_slots_over_long_spans(engine):
    """The same batch with five slots: connections 5 and 6 count in the block and in no entry, and never fail."""
    p, _, _ = _plan("mixed")
    slots = p.slots[:5]
    want, _ = W.reference_view(p.descs, None, p.ordinals, 5, bad=p.bad, slots=slots)
    want_table, _ = W.connection_view(p.descs, None, p.ordinals, 5, bad=p.bad, slots=slots)
    ref, state = engine.new_counters(), engine.new_conn_state(5 + 2)
    engine.refview_conns(p.arena_bytes, _bytes_dev(p.descs), ref, state[:5 * 4], base_index=p.base_index,
                         conn_first_fail=_u32_dev(slots))
    torch.cuda.synchronize()
    got = _host(state, CONN_STATE_DTYPE)
    assert np.array_equal(got[:5], want_table) and not got[5:].view(np.uint64).any()
    assert engine.read_counters_ref(ref) == want


# ---- 2. the strided form --------------------------------------------------------------------------------------------
def test_one_ring_over_long_spans(engine):
    """cts_refview_accumulate_conns_strided: one connection, a stride of 2^32 - 1 and lengths up to it, so every parked
    tile holds per-lane sums that the 32-bit range cannot. Slots: mid-batch, on a span seam, its neighbour, none."""
    cus = _cus()
    lens, bad, keys, walked = A.strided_lengths(cus)
    n, span, base, counts = len(lens), walked["span"], A.BASE_INDEX, walked["counts"]
    print(n, counts)
    assert span == 320
    # one connection: the transitions a single key can reach (bad descriptors break the run now and then)
    for f in ("first_pure", "first_mixed", "parked_tile", "parked_twice", "unpark_mixed_merge", "carry_merge_mixed",
              "end_parked", "end_scan", "join_1", "join_3", "join_break_notwhole", "empty_wave"):
        assert counts[f] >= 4, f
    assert counts["scan_partial"] == 1
    ring_bytes = n * A.STRIDE
    sd = np.zeros(n, dtype=DESC_DTYPE)
    sd["byte_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(A.STRIDE)
    sd["length"], sd["skip_head"], sd["conn_index"] = lens, A.STRIDED_SKIP, 1
    assert np.array_equal(W.descs_bad(sd, ring_bytes), bad) and 100 < bad.sum() < n // 200
    g = base + np.arange(n, dtype=np.int64)
    lens_d = _u32_dev(lens)
    seam = base + (walked["grid"] * 2 + 1) * span      # the first ordinal of a span in the middle of the batch
    for slot in (base + n // 2 + 17, seam, seam - 1, EMPTY):
        slots = np.array([5, slot, EMPTY], dtype=np.uint32)
        want, _ = W.reference_view(sd, None, g, 3, bad=bad, slots=slots)
        want_table, _ = W.connection_view(sd, None, g, 3, bad=bad, slots=slots)
        assert want["bytes_recv"] > 1 << 46
        for nt in (1, 0):
            ref, plain, state, cff = engine.new_counters(), engine.new_counters(), engine.new_conn_state(3), _u32_dev(slots)
            _nt(engine, nt)
            try:
                engine.refview_conns_strided(ring_bytes, A.STRIDE, lens_d, ref, state, skip_head=A.STRIDED_SKIP,
                                             conn_index=1, base_index=base, conn_first_fail=cff)
                engine.refview_strided(ring_bytes, A.STRIDE, lens_d, plain, skip_head=A.STRIDED_SKIP, conn_index=1,
                                       base_index=base, conn_first_fail=cff)
                torch.cuda.synchronize()
            finally:
                _nt(engine, 1)
            got = _host(state, CONN_STATE_DTYPE)
            for f in CONN_STATE_DTYPE.names:
                assert got[f].tolist() == want_table[f].tolist(), (slot, nt, f)
            assert engine.read_counters_ref(ref) == want, (slot, nt)
            assert engine.read_counters_ref(plain) == want, (slot, nt)
            assert np.array_equal(_host(cff, np.uint32), slots)


# ---- 3. ms_conn_accumulate over the same connection plan ------------------------------------------------------------
@pytest.mark.parametrize("nt", (1, 0))
@pytest.mark.parametrize("tail", ("run", "mixed"))
def test_media_stream_over_long_spans(engine, tail, nt):
    """cts_media_stream_conns_accumulate over the plan's connections with synthetic statuses: completed bytes up to
    2^32 - 1 (bits above 2^32 per datagram), windows of 600 frames, sequence numbers outside the window, ID datagrams and
    a connection without an entry; slots as in the plan. Entries, rings, the sticky flags, the latched errors and the
    UDP block equal the numpy restatement."""
    p, _, _ = _plan(tail)
    conn, st = A.ms_batch(p)
    walked = A.walk(conn, p.cus)
    print(tail, nt, walked["counts"])
    assert walked["span"] == 320 and A.covered(walked["counts"]) == []
    table = M.ConnectionTable(engine, [A.MS_WINDOW] * p.n_conns)
    assert table.frame_elems == 600 * p.n_conns
    want, want_ring, want_udp = A.ms_accumulate_model(table.fresh, table.frame_elems, p.slots, conn, st, p.base_index)
    # what the batch is there for
    outside = (st["kind"] == W.DGRAM_DATA) & ((st["sequence_number"] < 1) | (st["sequence_number"] > 600))
    assert 0.015 < outside.mean() < 0.025 and 0.007 < (st["kind"] == W.DGRAM_ID).mean() < 0.013
    assert (conn >= p.n_conns).sum() > 100 and want_udp["bits_received"] > 1 << 50
    assert (want["error_frames"][[0, 2, 3, 4, 5, 6]] > 100).all() and want["error_frames"][1] == 0
    assert want["has_failure"].tolist() == [0, 0, 0, 1, 1, 1, 1] and want["received_any"].tolist() == [1, 0, 1, 1, 1, 1, 1]
    assert (want["datagrams_after_end"][[1, 3, 4, 5, 6]] > 1000).all()
    assert want_ring.reshape(p.n_conns, 600)[[0, 2, 3, 4, 5, 6]].min() > 1 << 32 and not want_ring[600:1200].any()
    descs = np.zeros(p.n, dtype=DESC_DTYPE)
    descs["conn_index"], descs["length"] = conn, st["completed_bytes"]
    table.slots.copy_(_u32_dev(p.slots))
    _nt(engine, nt)
    try:
        table.accumulate(p.arena_bytes, _bytes_dev(descs), _bytes_dev(st), p.base_index)
        torch.cuda.synchronize()
    finally:
        _nt(engine, 1)
    entries, ring, slots = table.read()
    for f in MS_CONN_STATE_DTYPE.names:
        assert entries[f].tolist() == want[f].tolist(), f
    assert np.array_equal(ring, want_ring)
    assert np.array_equal(slots, p.slots)
    assert table.read_udp() == want_udp


# ---- 4. conn_close on preset tables ---------------------------------------------------------------------------------
@pytest.mark.parametrize("with_results", (True, False))
def test_close_preset_tables(engine, with_results):
    """cts_conns_close over 8 x CUs x 256 + 257 ids (every lane takes a second grid-stride step, 257 a third):
    bytes_recv around 2^32 and at 2^40 + 5 against expected sizes that are equal, one off, or off in the high word only;
    failed slots; ids without a slot. Results, class counts, the byte sum and the emptied tables equal close_results."""
    n = 8 * _cus() * 256 + 257
    state, slots, ids, want = A.close_cases(n)
    res, counts, state2, slots2 = W.close_results(state, slots, ids, want)
    print(n, counts)
    assert min(counts.values()) > 1000 and counts["bytes_recv"] > 1 << 50
    got = state["bytes_recv"][np.minimum(ids, len(slots) - 1)]
    assert (((got ^ want) & np.uint64(0xFFFFFFFF)) == 0).sum() > n // 2  # the low words alone decide nothing
    cff, table, blk = _u32_dev(slots), _u64_dev(state.view(np.uint64)), engine.new_counters()
    out = engine.new_conn_results(n) if with_results else None
    for nt in (1, 0):
        _nt(engine, nt)
        try:
            engine.conns_close(_u32_dev(ids), _u64_dev(want), cff, table, blk, results=out)
            torch.cuda.synchronize()
        finally:
            _nt(engine, 1)
        if nt == 1:
            if with_results:
                got_res = _host(out, CONN_RESULT_DTYPE)
                for f in CONN_RESULT_DTYPE.names:
                    assert np.array_equal(got_res[f], res[f]), f
            assert engine.read_counters_close(blk) == counts
            assert np.array_equal(_host(cff, np.uint32), slots2)
            assert np.array_equal(_host(table, CONN_STATE_DTYPE), state2)
            assert (slots2 == EMPTY).all() and not state2.view(np.uint64).any()
            # the tables again for the plain-load form
            cff.copy_(_u32_dev(slots))
            table.copy_(_u64_dev(state.view(np.uint64)))
        else:
            both = {f: 2 * counts[f] for f in counts}
            assert engine.read_counters_close(blk) == both
            if with_results:
                assert np.array_equal(_host(out, CONN_RESULT_DTYPE), res)
            assert (_host(cff, np.uint32) == EMPTY).all() and not _host(table, np.uint64).any()


# ---- 5. ms_conn_render and ms_conn_close on preset entries ----------------------------------------------------------
def _ms_table(engine, n):
    """A ConnectionTable of n connections with rings of two frames of 2^32 - 1 bytes. The entries are cts_ms_conn_init's
    (ConnectionTable lays out the first 1 024; the others repeat that entry with the ring bases going on two by two,
    which is the same layout without a host call per connection), and every ring lies inside the ring array."""
    few = 1024
    table = M.ConnectionTable(engine, [(A.MS_FRAME_SIZE, 1, 3)] * few)
    fresh = np.repeat(table.fresh[:1], n)
    fresh["frame_base"] = 2 * np.arange(n, dtype=np.uint64)
    assert np.array_equal(fresh[:few], table.fresh) and table.frame_elems == 2 * few
    assert int((fresh["frame_base"] + fresh["frames"]).max()) == 2 * n
    table.fresh, table.n_conns, table.frame_elems = fresh, n, 2 * n
    return table


def _ms_upload(table, entries, ring, slots):
    assert np.array_equal(entries["frame_base"], table.fresh["frame_base"])
    assert np.array_equal(entries["frames"], table.fresh["frames"]) and len(ring) == table.frame_elems
    table.conns = torch.from_numpy(entries.view(np.int64).copy()).to(DEV)
    table.frame_bytes = _u64_dev(ring)
    table.slots = _u32_dev(slots)


def _same_ms(table, entries, ring, slots, where):
    got_e, got_ring, got_slots = table.read()
    for f in MS_CONN_STATE_DTYPE.names:
        assert np.array_equal(got_e[f], entries[f]), (where, f)
    assert np.array_equal(got_ring, ring), where
    assert np.array_equal(got_slots, slots), where


def test_render_and_close_preset_entries(engine):
    """cts_media_stream_conns_render over 8 x CUs x 256 + 257 connections (a second grid-stride step for every lane):
    head frames holding 2^32 - 2, 2^32 - 1, 2^32 and 2^33 - 1 bytes against a frame size of 2^32 - 1, FatalAborts that
    drop up to 2^32 - 1 frames each, connections ended or failed earlier, ids without an entry. Then
    cts_media_stream_conns_close over 8 x CUs x 4 x 2 + 5 of them (every wave closes two, five a third) with more than
    2^35 bits each and every status class."""
    cus = _cus()
    n = 8 * cus * 256 + 257
    table = _ms_table(engine, n - 300)
    entries, ring, kind, slots = A.ms_preset_entries(table.fresh)
    _ms_upload(table, entries, ring, slots)
    rng = np.random.default_rng(0x1D5)
    ids = rng.permutation(np.r_[np.arange(n - 300), n + rng.choice(1 << 20, size=300, replace=False)]).astype(np.uint32)
    want_e, want_ring, want_codes, want_udp = A.ms_render_model(entries, ring, ids)
    print(n, want_udp, np.bincount(want_codes))
    assert min(want_udp[f] for f in ("successful_frames", "dropped_frames", "duplicate_frames")) > n // 20
    assert want_udp["dropped_frames"] > 1 << 44 and np.bincount(want_codes).min() > n // 20
    # in one wave of 64 neighbouring ids the dropped frames alone pass 2^32
    fatal = np.where(ids < len(entries), kind[np.minimum(ids, len(entries) - 1)] == 0, False)
    per_wave = np.add.reduceat(np.where(fatal, entries["final_frame"][np.minimum(ids, len(entries) - 1)], 0),
                               np.arange(0, n, 64))
    assert (per_wave > 1 << 32).mean() > 0.9
    codes = torch.full((n,), 77, dtype=torch.int32, device=DEV)
    table.render(_u32_dev(ids), codes)
    torch.cuda.synchronize()
    assert np.array_equal(_host(codes, np.uint32), want_codes)
    _same_ms(table, want_e, want_ring, slots, "render")
    assert table.read_udp() == want_udp
    # the close: a seeded pick of the rendered entries, every class among them
    m = 8 * cus * 4 * 2 + 5
    close_ids = np.r_[rng.choice(n - 300, size=m - 3, replace=False), [n, n + 1, EMPTY]].astype(np.uint32)
    close_ids = rng.permutation(close_ids)
    res, e2, ring2, slots2, counts = A.ms_close_model(want_e, want_ring, slots, close_ids)
    print(m, counts)
    assert counts["connections_closed"] == m - 3 and counts["bytes_recv"] > m << 32
    assert min(counts[f] for f in ("successful", "data_errors", "not_all_data")) > 100
    assert set(np.unique(res["flags"]).tolist()) == {0, 1, 2, 4} and (res["bits_received"][res["flags"] != 1] > 1 << 35).all()
    block, out = engine.new_counters(), table.new_results(m)
    table.close(_u32_dev(close_ids), block, results=out)
    torch.cuda.synchronize()
    got = _host(out, MS_CONN_RESULT_DTYPE)
    for f in MS_CONN_RESULT_DTYPE.names:
        assert np.array_equal(got[f], res[f]), f
    _same_ms(table, e2, ring2, slots2, "close")
    assert engine.read_counters_close(block) == counts
    assert table.read_udp() == want_udp


# ---- 6. counter reads at large totals -------------------------------------------------------------------------------
def _large_blocks():
    """Two counter blocks (64 shards of 8 words) whose six sums lie between 2^53 and 2^62, and the sums."""
    rng = np.random.default_rng(0xB10C)
    blocks = rng.integers(1 << 47, 1 << 55, size=(2, 64, 8), dtype=np.uint64)
    blocks[:, :, 6:] = 0
    sums = [[sum(int(x) for x in b[:, k]) for k in range(6)] for b in blocks]
    assert all(1 << 53 <= s < 1 << 62 for row in sums for s in row)
    return blocks, sums


def _reads_main(q):
    """The reads of two engines' blocks on this GPU; run in a child so RCCL's threads end with it."""
    try:
        from ctstraffic_amd import Engine
        from ctstraffic_amd import engine as E

        torch.cuda.set_device(0)
        blocks, _ = _large_blocks()
        out = {}
        with Engine(0) as e0, Engine(0) as e1:
            dev = [_u64_dev(b.reshape(-1)) for b in blocks]
            for kind in ("ref", "close", "udp"):
                out["read_" + kind] = [getattr(e, "read_counters_" + kind)(d) for e, d in zip((e0, e1), dev)]
                out["multi_" + kind] = getattr(E, "counters_read_multi_" + kind)([e0, e1], dev)
            try:
                for kind in ("ref", "close", "udp"):
                    out["allreduce_" + kind] = getattr(E, "counters_allreduce_" + kind)([e0, e1], dev)
                    out["allreduce_one_" + kind] = getattr(E, "counters_allreduce_" + kind)([e1], dev[1:])
                E.counters_allreduce_release()
            except _lib.CtsError as e:
                if e.status != _lib.CTS_E_UNAVAILABLE:
                    raise
                out["allreduce_ref"] = None
        q.put(out)
    except Exception as e:  # pragma: no cover
        import traceback

        q.put(("error", repr(e) + traceback.format_exc()))


def test_counter_reads_at_large_totals():
    """Blocks written from the host, every sum between 2^53 and 2^62 (past what a double holds exactly): the plain
    reads, the read_multi forms over two engines and the all-reduce forms give the integer sums."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_reads_main, args=(q,), daemon=True)
    p.start()
    try:
        r = q.get(timeout=100)
        p.join(15)
    finally:
        if p.is_alive():
            p.kill()
            p.join(5)
    assert not (isinstance(r, tuple) and r[0] == "error"), r[1]
    assert p.exitcode == 0
    _, sums = _large_blocks()
    fields = {"ref": W.REF_FIELDS, "close": W.CLOSE_FIELDS, "udp": W.UDP_FIELDS}
    for kind, names in fields.items():
        one = [dict(zip(names, row)) for row in sums]
        both = {f: one[0][f] + one[1][f] for f in names}
        assert r["read_" + kind] == one, kind
        assert r["multi_" + kind] == both, kind
    if r["allreduce_ref"] is None:
        return  # RCCL is not available (CTS_E_UNAVAILABLE): the two host folds stand alone
    for kind, names in fields.items():
        one = [dict(zip(names, row)) for row in sums]
        assert r["allreduce_" + kind] == {f: one[0][f] + one[1][f] for f in names}, kind
        assert r["allreduce_one_" + kind] == one[1], kind
