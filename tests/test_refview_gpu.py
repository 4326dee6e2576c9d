"""GPU: stream ordinals in the first-failure slots (cts_verify_at / cts_verify_strided_at) and the reference view of
the device counters (cts_refview_accumulate, the *_ref reads) against workload.reference_view.

ctsTraffic fails a connection on the completion whose VerifyBuffer failed (ctsIOPattern.cpp:486-489 -> FailedIo):
nothing after a connection's first failing buffer is received or counted. The failed mask the model gets always
comes from oracle.verify_batch on the materialised arena's bytes. Integer work: bit-exact.
"""
import numpy as np
import pytest

import oracle
import refview_plans as P
from ctstraffic_amd import _lib
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import DESC_DTYPE

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
EMPTY = 0xFFFFFFFF


def _slots(n):
    return torch.full((n,), -1, dtype=torch.int32, device=DEV)


def _dev(descs):
    return torch.from_numpy(np.ascontiguousarray(descs, dtype=DESC_DTYPE).view(np.uint8).copy()).to(DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


_cache = {}


def _materialised(engine, name):
    """A plan on the device, the oracle's verdict on its bytes and the model's view of it: computed once."""
    if name not in _cache:
        w, launches, ordinals, facts = P.plan(name)
        arena, _ = W.materialize(engine, w)
        torch.cuda.synchronize()
        res, octr, _ = oracle.verify_batch(arena.cpu().numpy(), w.descs, n_conns=w.n_conns, nthreads=8)
        failed = (res["pass"] == 0) & (res["flags"] == 0)
        sums, slots = P.check_facts(w, launches, ordinals, failed, facts, P.PLANS[name][0]["buffers_per_conn"])
        dd = [_dev(d) for d, _, _ in launches]
        _cache[name] = (w, launches, arena, dd, octr, sums, slots, facts)
    return _cache[name]


VARIANTS = ("host_sync", "queued", "reverse")


def _run_plan(engine, name, variant):
    w, launches, arena, dd, octr, sums, slots, facts = _materialised(engine, name)
    ctr, ref, cff = engine.new_counters(), engine.new_counters(), _slots(w.n_conns)
    torch.cuda.synchronize()
    kw = dict(max_length_hint=w.max_length, counters=ctr, conn_first_fail=cff)
    order = range(len(launches))
    if variant == "reverse":  # every verify first, latest ordinals first, then the passes
        for k in reversed(order):
            engine.verify(arena, dd[k], base_index=launches[k][1], **kw)
        for k in order:
            engine.refview(w.arena_bytes, dd[k], ref, base_index=launches[k][1], conn_first_fail=cff)
    else:
        for k in order:
            engine.verify(arena, dd[k], base_index=launches[k][1], **kw)
            if variant == "host_sync":
                torch.cuda.synchronize()
            engine.refview(w.arena_bytes, dd[k], ref, base_index=launches[k][1], conn_first_fail=cff)
            if variant == "host_sync":
                torch.cuda.synchronize()
    torch.cuda.synchronize()
    got_slots = _u32(cff)
    got = engine.read_counters_ex(ctr)
    view = engine.read_counters_ref(ref)
    print(name, variant, view, got)
    assert np.array_equal(got_slots, slots)  # the global first failing ordinals
    assert view == sums
    assert view["buffers_failed"] == got["connections_failed"] == facts["failed"]
    assert view["bytes_recv"] + view["bytes_after_failure"] == got["bytes_checked"]
    assert view["buffers_recv"] + view["buffers_after_failure"] == got["buffers_checked"]
    assert {k: got[k] for k in octr} == octr  # the ordinary five counters, as before
    return got_slots


@pytest.mark.parametrize("variant", VARIANTS)
def test_workgroup_path_three_launches(engine, variant):
    """96 connections x 48 x 64 KiB, one buffer in 37 corrupt, each stream cut in thirds (base_index 0 / 1536 / 3072):
    73 connections fail, 134 676 480 of the 301 989 888 verified bytes come after a connection's first failure."""
    w = _materialised(engine, "wg")[0]
    assert w.max_length > engine.get_attr(3) and [b for _, b, _ in _materialised(engine, "wg")[1]] == [0, 1536, 3072]
    _run_plan(engine, "wg", variant)
    view = _materialised(engine, "wg")[5]
    assert view["bytes_recv"] == 167313408 and view["bytes_after_failure"] == 134676480


@pytest.mark.parametrize("variant", VARIANTS)
def test_ragged_workgroup_path(engine, variant):
    """Ragged completions of up to 64 KiB packed at every alignment, three launches."""
    assert _materialised(engine, "ragged")[0].max_length > engine.get_attr(3)
    _run_plan(engine, "ragged", variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_quad_path_two_launches(engine, variant):
    """Ragged completions of at most 1472 bytes: the four-buffers-per-wave kernel carries the ordinals."""
    assert _materialised(engine, "quad")[0].max_length <= engine.get_attr(3)  # CTS_ATTR_SMALL_THRESHOLD
    _run_plan(engine, "quad", variant)


def _ring():
    """The ring of tests/test_data_error_gpu.py::test_strided_ring_counts_its_one_connection_once."""
    n, stride, skip = 4096, 1536, 26
    rng = np.random.default_rng(0x5EED)
    lens = rng.integers(skip + 1, stride + 1, size=n).astype(np.uint32)
    ring = np.zeros(n * stride, dtype=np.uint8)
    pat = oracle.sender_buffer(stride)
    for i in range(n):
        ring[i * stride + skip:i * stride + lens[i]] = pat[:lens[i] - skip]
    clean = ring.copy()
    bad = rng.choice(n, size=40, replace=False)
    for i in bad:
        ring[i * stride + skip + rng.integers(0, lens[i] - skip)] ^= 0x5A
    return n, stride, skip, lens, ring, clean, np.sort(bad)


def test_strided_ring_two_launches(engine):
    """4096 x 1536-byte slots, 40 bad datagrams, skip_head 26, as two launches of 2048 over one slot: the slot is the
    global ordinal of the first bad datagram, the reference view the ring's prefix through it."""
    n, stride, skip, lens, ring, clean, bad = _ring()
    conn, half = 2, 2048
    d = np.zeros(n, dtype=DESC_DTYPE)
    d["byte_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    d["length"], d["skip_head"], d["conn_index"] = lens, skip, conn
    lens_d = [torch.from_numpy(lens[k * half:(k + 1) * half].copy()).to(DEV) for k in range(2)]
    for arena_np, first_bad in ((ring, int(bad[0])), (clean, None)):
        res, octr, _ = oracle.verify_batch(arena_np, d, n_conns=3)
        failed = (res["pass"] == 0) & (res["flags"] == 0)
        assert (np.nonzero(failed)[0].tolist() == bad.tolist()) if first_bad is not None else not failed.any()
        sums, slots = W.reference_view(d, failed, np.arange(n), 3)
        arena = torch.from_numpy(arena_np).to(DEV)
        halves = [arena[k * half * stride:(k + 1) * half * stride] for k in range(2)]
        for order in ((0, 1), (1, 0)):
            ctr, ref, cff = engine.new_counters(), engine.new_counters(), _slots(3)
            for k in order:
                engine.verify_strided(halves[k], stride, lens_d[k], skip_head=skip, conn_index=conn, counters=ctr,
                                      conn_first_fail=cff, base_index=k * half)
            for k in order:
                engine.refview_strided(half * stride, stride, lens_d[k], ref, skip_head=skip, conn_index=conn,
                                       base_index=k * half, conn_first_fail=cff)
            torch.cuda.synchronize()
            view, got = engine.read_counters_ref(ref), engine.read_counters_ex(ctr)
            print(order, view, got)
            assert np.array_equal(_u32(cff), slots)
            assert view == sums and {k: got[k] for k in octr} == octr
            vlen = lens.astype(np.int64) - skip
            if first_bad is None:
                assert _u32(cff).tolist() == [EMPTY] * 3 and got["connections_failed"] == 0
                assert view["bytes_after_failure"] == 0 == view["buffers_failed"]
                assert view["bytes_recv"] == view["bytes_ok"] == int(vlen.sum())
            else:
                assert first_bad >= 1 and _u32(cff).tolist() == [EMPTY, EMPTY, first_bad]
                assert got["connections_failed"] == 1 == view["buffers_failed"] and got["buffers_failed"] == 40
                assert view["bytes_recv"] == int(vlen[:first_bad + 1].sum())
                assert view["bytes_ok"] == int(vlen[:first_bad].sum())
                assert view["buffers_recv"] == first_bad + 1


def _synthetic(n, n_conns, base, rng, arena_bytes):
    """n descriptors, connection-major over n_conns + 40 connections (the last 40 have no slot), with some of every
    bad-descriptor kind, and hand-written slots: empty, a connection's first ordinal, its last, one inside, one
    below the batch, one above it."""
    d = np.zeros(n, dtype=DESC_DTYPE)
    d["conn_index"] = np.sort(rng.integers(0, n_conns + 40, size=n)).astype(np.uint32)
    d["length"] = rng.integers(0, 70000, size=n)
    d["skip_head"] = np.where(rng.random(n) < 0.5, 26, 0)  # skip_head above a short length: bad
    d["expected_pattern_offset"] = rng.integers(0, 65536, size=n)
    d["byte_offset"] = rng.integers(0, arena_bytes - 70000, size=n).astype(np.uint64)
    kind = rng.integers(0, 400, size=n)
    d["expected_pattern_offset"][kind == 0] = 65536 + rng.integers(0, 1000)
    d["byte_offset"][kind == 1] = arena_bytes + 1                               # starts past the arena
    d["byte_offset"][kind == 2] = arena_bytes - 1                               # leaves it
    d["length"][kind == 2] = np.maximum(d["length"][kind == 2], 2)
    d["skip_head"][kind == 3] = d["length"][kind == 3] + 1                      # header longer than the transfer
    d["byte_offset"][kind == 4] = np.uint64(1) << np.uint64(63)
    bad = W.descs_bad(d, arena_bytes)
    g = base + np.arange(n, dtype=np.int64)
    conn = d["conn_index"].astype(np.int64)
    slots = np.full(n_conns, EMPTY, dtype=np.uint32)
    present = np.unique(conn[conn < n_conns])
    firsts = np.searchsorted(conn, present, side="left")
    lasts = np.searchsorted(conn, present, side="right") - 1
    how = rng.integers(0, 6, size=len(present))
    inside = firsts + ((lasts - firsts) * rng.random(len(present))).astype(np.int64)
    val = np.select([how == 0, how == 1, how == 2, how == 3, how == 4],
                    [np.full(len(present), EMPTY), g[firsts], g[lasts], g[inside], np.full(len(present), max(base - 1, 0))],
                    default=g[-1] + 1)
    slots[present] = val.astype(np.uint32)
    return d, bad, g, slots


def test_the_pass_alone_never_touches_an_arena(engine):
    """1 000 003 synthetic descriptors over 5 000 connections (more than one grid of lanes, no multiple of 64 or 256),
    an arena that does not exist, hand-written slots and a nonzero base_index; then n = 1, and n = 63 with every
    buffer after its slot; then a strided ring with lengths above the stride and a tail that leaves the arena."""
    rng = np.random.default_rng(0x7EF)
    arena_bytes, n_conns, base = 1 << 40, 5000, 123457
    d, bad, g, slots = _synthetic(1000003, n_conns, base, rng, arena_bytes)
    assert bad.sum() > 5000 and (d["conn_index"] >= n_conns).sum() > 1000
    assert {int((slots == EMPTY).sum()) > 0, int(np.isin(slots, g).sum()) > 0} == {True}
    want, _ = W.reference_view(d, np.zeros(len(d), bool), g, n_conns, bad=bad, slots=slots)
    assert min(want.values()) > 0
    cff = torch.from_numpy(slots.view(np.int32).copy()).to(DEV)
    for nt in (1, 0):
        engine.set_attr(_lib.ATTR_NT_LOADS, nt)
        try:
            ref = engine.new_counters()
            engine.refview(arena_bytes, _dev(d), ref, base_index=base, conn_first_fail=cff)
            torch.cuda.synchronize()
            view = engine.read_counters_ref(ref)
        finally:
            engine.set_attr(_lib.ATTR_NT_LOADS, 1)
        print(nt, view)
        assert view == want
    assert np.array_equal(_u32(cff), slots)  # the pass only reads the slots
    # one descriptor, at its connection's slot
    one = d[~bad][:1].copy()
    one["conn_index"] = 7
    ref = engine.new_counters()
    engine.refview(arena_bytes, _dev(one), ref, base_index=99, conn_first_fail=torch.full((8,), 99, dtype=torch.int32,
                                                                                         device=DEV))
    v = int(one["length"][0]) - int(one["skip_head"][0])
    assert engine.read_counters_ref(ref) == {"bytes_recv": v, "bytes_ok": 0, "buffers_recv": 1, "buffers_failed": 1,
                                             "bytes_after_failure": 0, "buffers_after_failure": 0}
    # 63 descriptors, every one after its connection's slot
    late = d[~bad][:63].copy()
    late["conn_index"] = np.arange(63) % 5
    ref = engine.new_counters()
    engine.refview(arena_bytes, _dev(late), ref, base_index=100, conn_first_fail=torch.zeros(5, dtype=torch.int32,
                                                                                            device=DEV))
    v = int((late["length"].astype(np.int64) - late["skip_head"].astype(np.int64)).sum())
    assert engine.read_counters_ref(ref) == {"bytes_recv": 0, "bytes_ok": 0, "buffers_recv": 0, "buffers_failed": 0,
                                             "bytes_after_failure": v, "buffers_after_failure": 63}
    # a strided ring: length > stride and slots that leave the arena are bad descriptors
    n, stride, skip = 70001, 1536, 26
    lens = rng.integers(0, stride + 40, size=n).astype(np.uint32)
    lens[-3] = 500  # starts inside the arena, 100 bytes before its end
    ring_bytes = (n - 3) * stride + 100
    sd = np.zeros(n, dtype=DESC_DTYPE)
    sd["byte_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    sd["length"], sd["skip_head"], sd["conn_index"] = lens, skip, 1
    sbad = W.descs_bad(sd, ring_bytes) | (lens > stride)
    assert (lens > stride).sum() > 100 and (lens < skip).sum() > 100 and sbad[-3:].all()
    for slot in (EMPTY, 5000 + 31337, 5000, 5000 + n - 1):
        want, _ = W.reference_view(sd, np.zeros(n, bool), 5000 + np.arange(n), 2, bad=sbad,
                                   slots=np.array([0, slot], dtype=np.uint32))
        ref = engine.new_counters()
        engine.refview_strided(ring_bytes, stride, torch.from_numpy(lens.copy()).to(DEV), ref, skip_head=skip,
                               conn_index=1, base_index=5000,
                               conn_first_fail=torch.from_numpy(np.array([0, slot], np.uint32).view(np.int32)).to(DEV))
        assert engine.read_counters_ref(ref) == want, slot


def test_ordinal_limits(engine):
    """base_index + n == 0xFFFFFFFF is the last launch a slot array takes (ordinal 0xFFFFFFFF stays the empty slot);
    one more is CTS_E_INVALID from all four entry points with nothing launched; cts_verify keeps launch-local
    indices."""
    from ctstraffic_amd._lib import CtsError

    w = W.tcp_resident(n_buffers=64, corrupt_rate=8)  # one buffer per connection: slot[c] = ordinal of buffer c
    arena, descs = W.materialize(engine, w)
    _, _, ec, ecff = W.expected_results(w)
    failed = ecff != EMPTY
    assert failed.sum() == 8
    top = EMPTY - w.n
    for hint in (65536, 0):  # the workgroup kernel by hint and without one
        ctr, cff = engine.new_counters(), _slots(w.n_conns)
        engine.verify(arena, descs, max_length_hint=hint, counters=ctr, conn_first_fail=cff, base_index=top)
        torch.cuda.synchronize()
        assert np.array_equal(_u32(cff), np.where(failed, (top + ecff.astype(np.int64)) & EMPTY, EMPTY))
        assert _u32(cff).max() == EMPTY and _u32(cff)[failed].min() >= top
        got = engine.read_counters_ex(ctr)
        assert {k: got[k] for k in ec} == ec and got["connections_failed"] == 8
        ref = engine.new_counters()
        engine.refview(w.arena_bytes, descs, ref, base_index=top, conn_first_fail=cff)
        view = engine.read_counters_ref(ref)
        assert view["buffers_failed"] == 8 and view["buffers_after_failure"] == 0 and view["buffers_recv"] == 64
        assert view["bytes_ok"] == ec["bytes_ok"] and view["bytes_recv"] == ec["bytes_checked"]
    # the quad kernel and the strided ring at the top of the range
    n, stride = 256, 1024
    ring = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)  # zeros: every datagram fails
    lens = torch.full((n,), stride, dtype=torch.int32, device=DEV)
    sd = np.zeros(n, dtype=DESC_DTYPE)
    sd["byte_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    sd["length"], sd["conn_index"] = stride, np.arange(n) % 4
    stop = EMPTY - n
    ctr, cff = engine.new_counters(), _slots(4)
    engine.verify(ring, _dev(sd), max_length_hint=stride, counters=ctr, conn_first_fail=cff, base_index=stop)
    assert _u32(cff).tolist() == [stop, stop + 1, stop + 2, stop + 3]
    cff1 = _slots(1)
    engine.verify_strided(ring, stride, lens, expected_offset=2, counters=ctr, conn_first_fail=cff1, base_index=stop)
    assert _u32(cff1).tolist() == [stop]
    ref = engine.new_counters()
    engine.refview_strided(n * stride, stride, lens, ref, base_index=stop, conn_first_fail=cff1)
    assert engine.read_counters_ref(ref)["buffers_after_failure"] == n - 1
    # one ordinal too many: refused before anything is launched
    before = engine.read_counters_ex(ctr)
    ref, slots_before = engine.new_counters(), _u32(cff).copy()
    calls = (lambda: engine.verify(arena, descs, max_length_hint=65536, counters=ctr, conn_first_fail=cff,
                                   base_index=top + 1),
             lambda: engine.verify_strided(ring, stride, lens, counters=ctr, conn_first_fail=cff,
                                           base_index=stop + 1),
             lambda: engine.refview(w.arena_bytes, descs, ref, base_index=top + 1, conn_first_fail=cff),
             lambda: engine.refview_strided(n * stride, stride, lens, ref, base_index=stop + 1, conn_first_fail=cff),
             lambda: engine.refview(w.arena_bytes, descs, ref, base_index=EMPTY, conn_first_fail=cff))
    for call in calls:
        with pytest.raises(CtsError) as err:
            call()
        assert err.value.status == _lib.CTS_E_INVALID
    torch.cuda.synchronize()
    assert engine.read_counters_ex(ctr) == before and np.array_equal(_u32(cff), slots_before)
    assert set(engine.read_counters_ref(ref).values()) == {0}
    # cts_verify, and cts_verify_at with base 0, write launch-local indices
    for at in (False, True):
        cff = _slots(w.n_conns)
        if at:
            _lib.check("cts_verify_at", _lib.lib().cts_verify_at(
                engine._h, arena.data_ptr(), arena.numel(), descs.data_ptr(), w.n, 65536, 0, None, None,
                cff.data_ptr(), w.n_conns, torch.cuda.current_stream().cuda_stream))
        else:
            engine.verify(arena, descs, max_length_hint=65536, conn_first_fail=cff)
        torch.cuda.synchronize()
        assert np.array_equal(_u32(cff), ecff)


def _folds_main(q):
    """Reference-view blocks of two engines on this GPU through the three reads; run in a child so RCCL's threads end
    with it."""
    try:
        import refview_plans as P
        from ctstraffic_amd import Engine
        from ctstraffic_amd.engine import counters_allreduce_ref, counters_allreduce_release, counters_read_multi_ref

        torch.cuda.set_device(0)
        out = {}
        with Engine(0) as e0, Engine(0) as e1:
            blocks, exps = [], []
            for k, eng in enumerate((e0, e1)):
                w = W.connection_streams(world=2, rank=k, n_conns=64, buffers_per_conn=8, length=65536,
                                         corrupt_rate=5 + k)
                arena, _ = W.materialize(eng, w, device="cuda:0")
                res, _, _ = oracle.verify_batch(arena.cpu().numpy(), w.descs, n_conns=w.n_conns)
                launches = W.stream_launches(w.descs, 8, 2)
                ordinals = np.zeros(w.n, dtype=np.int64)
                ctr, ref = eng.new_counters(), eng.new_counters()
                cff = torch.full((w.n_conns,), -1, dtype=torch.int32, device="cuda:0")
                for d, base, idx in launches:
                    ordinals[idx] = base + np.arange(len(idx))
                    dd = _dev(d)
                    eng.verify(arena, dd, max_length_hint=65536, counters=ctr, conn_first_fail=cff, base_index=base)
                    eng.refview(w.arena_bytes, dd, ref, base_index=base, conn_first_fail=cff)
                torch.cuda.synchronize()
                blocks.append(ref)
                exps.append(W.reference_view(w.descs, (res["pass"] == 0) & (res["flags"] == 0), ordinals,
                                             w.n_conns)[0])
            both = {f: exps[0][f] + exps[1][f] for f in exps[0]}
            out["read"] = (e0.read_counters_ref(blocks[0]), exps[0])
            out["multi"] = (counters_read_multi_ref([e0, e1], blocks), both)
            try:
                out["allreduce"] = (counters_allreduce_ref([e0, e1], blocks), both)
                out["allreduce_one"] = (counters_allreduce_ref([e1], blocks[1:]), exps[1])
                counters_allreduce_release()
            except _lib.CtsError as e:
                if e.status != _lib.CTS_E_UNAVAILABLE:
                    raise
                out["allreduce"] = None
        q.put(out)
    except Exception as e:  # pragma: no cover
        q.put(("error", repr(e)))


def test_reference_view_blocks_through_the_three_folds():
    """read_counters_ref, counters_read_multi_ref and counters_allreduce_ref (the RCCL all-reduce of count 6) over
    reference-view blocks agree with the model."""
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
    assert got == exp and exp["buffers_failed"] > 0 and exp["bytes_after_failure"] > 0
    got, exp = r["multi"]
    assert got == exp
    assert p.exitcode == 0
    if r["allreduce"] is None:
        pytest.skip("RCCL is not available: the all-reduce of the reference view was not run")
    got, exp = r["allreduce"]
    assert got == exp
    got, exp = r["allreduce_one"]
    assert got == exp
