"""CPU: what tests/test_accounting_seams_gpu.py rests on (tests/accounting_plans.py).

1. geometry() is the launchers' span arithmetic: tests/cpp/spans_check.cpp, built here with g++ over
   ctstraffic_amd/csrc/cts_spans.hpp (the header launch_conn_accumulate_src and launch_ms_conn_accumulate use), prints
   the same grid and span.
2. The plans reach every transition of a wave's walk in at least 4 waves (scan_partial: once per launch) at 64, 256 and
   304 compute units, and the largest batches of the older accounting tests reach none of the un-park transitions at
   256: the gap the seam tests close.
3. workload.reference_view, connection_view and close_results hold at these values: compared with one-descriptor-at-a-
   time loops in Python integers.
"""
import os
import subprocess

import numpy as np
import pytest

import accounting_plans as A
import connection_plans as C
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import CONN_STATE_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = (64, 256, 304)
TAILS = ("run", "mixed")


# ---- 1. the geometry ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spans_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spans") / "spans_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ctstraffic_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "spans_check.cpp"), "-o", exe], check=True)
    return exe


def test_geometry_is_the_launchers(spans_check):
    sizes = [1, 63, 64, 65, 256, 257, 1048576, 1048577, (1 << 32) - 2] + [A.plan_size(c) for c in (1,) + CUS]
    pairs = [(n, cus) for n in sizes for cus in (1,) + CUS]
    out = subprocess.run([spans_check] + [str(x) for p in pairs for x in p], check=True, capture_output=True,
                         text=True).stdout.split("\n")
    got = [tuple(int(x) for x in line.split()) for line in out if line]
    assert got == [(n, cus) + A.geometry(n, cus) for n, cus in pairs]
    # the figures the tests are built on: two tiles up to 1 Mi descriptors on 256 CUs, three past it, five for the plans
    assert A.geometry(1000003, 256) == (2048, 128) and A.geometry(594288, 256) == (2048, 128)
    assert A.geometry(1048576, 256) == (2048, 128) and A.geometry(1048577, 256) == (2048, 192)
    for cus in (1,) + CUS:
        assert A.geometry(A.plan_size(cus), cus) == (8 * cus, 320)
    assert A.geometry((1 << 32) - 2, 1)[1] % 64 == 0 and A.geometry((1 << 32) - 2, 1)[1] * 32 >= (1 << 32) - 2
    # a launcher never sees fewer than one compute unit
    assert subprocess.run([spans_check, "1000", "0"], check=True, capture_output=True,
                          text=True).stdout.split() == ["1000", "0", "4", "64"]
    assert subprocess.run([spans_check, "0", "4"], capture_output=True).returncode == 2


# ---- 2. the walk ----------------------------------------------------------------------------------------------------
def _tile_by_tile(keys, cus):
    """The walk of accounting_plans.walk as plain loops, one wave and one tile at a time: events per wave."""
    n = len(keys)
    grid, span = A.geometry(n, cus)
    events, tails = [], []
    for w in range(grid * 4):
        lo, hi = w * span, min(w * span + span, n)
        ev, ckey, whole, parked = set(), A.KNONE, True, False
        for t in range(lo, hi, 64):
            k = [int(keys[i]) if i < hi else A.KNONE for i in range(t, t + 64)]
            heads = sum(1 for j in range(64) if j == 0 or k[j] != k[j - 1])
            merge = k[0] == ckey
            if heads == 1 and merge:
                ev.add("parked_twice" if parked else "parked_tile")
                ev.add("parked_tile")
                parked = True
                continue
            if t == lo:
                ev.add("first_pure" if heads == 1 else "first_mixed")
            elif parked:
                ev.add("unpark_pure_other" if heads == 1 else
                       "unpark_mixed_merge" if merge else "unpark_mixed_nomerge")
            else:
                ev.add("carry_merge_mixed" if merge else "carry_end")
            if t + 64 > n:
                ev.add("scan_partial")
            parked = False
            whole = whole and heads == 1 and (merge or t == lo)
            ckey = k[63]
        ev.add("empty_wave" if lo >= hi else "end_parked" if parked else "end_scan")
        events.append(ev)
        tails.append((ckey, whole, lo < hi))
    joins = {1: 0, 2: 0, 3: 0}
    for b in range(grid):
        key, chain = tails[4 * b][0], 1
        for w in range(1, 4):
            k, whole, nonempty = tails[4 * b + w]
            if not whole or k != key:
                if nonempty:
                    events[4 * b + w].add("join_break_key" if whole else "join_break_notwhole")
                if chain > 1 and key != A.KNONE:
                    joins[chain - 1] += 1
                key, chain = k, 1
            else:
                chain += 1
        if chain > 1 and key != A.KNONE:
            joins[chain - 1] += 1
    counts = {name: sum(1 for ev in events if name in ev) for name in A.TRANSITIONS if not name[5:6].isdigit()}
    counts.update({"join_%d" % k: v for k, v in joins.items()})
    return counts


def test_the_walk_against_plain_loops():
    """The vectorised walk equals a tile-by-tile loop on a small device (2 CUs: 64 waves of five tiles) for both
    tails, on a batch with a partial last tile only, and on batches shorter than the grid."""
    rng = np.random.default_rng(7)
    for tail in TAILS:
        conn, bad = A.connection_keys(2, tail, rng)
        keys = np.where(bad, A.KNONE, conn).astype(np.uint32)
        walked = A.walk(keys, 2)
        assert walked["span"] == 320 and walked["counts"]["parked_twice"] > 4
        assert walked["counts"] == _tile_by_tile(keys, 2)
    for n, cus in ((1, 4), (63, 4), (257, 1), (5000, 1), (20001, 2)):
        keys = np.repeat(rng.integers(0, 3, size=n), rng.choice([1, 64, 130], size=n))[:n].astype(np.uint32)
        keys[rng.random(n) < 0.01] = A.KNONE
        assert A.walk(keys, cus)["counts"] == _tile_by_tile(keys, cus), (n, cus)


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("cus", CUS)
def test_plans_reach_every_transition(cus, tail):
    p = A.plan(cus, tail)
    counts = p.walked["counts"]
    print(cus, tail, counts)
    assert p.n == 8 * cus * 4 * 256 + 1003 and p.walked["span"] == 320 and p.walked["parked"].shape[1] == 5
    assert A.covered(counts) == []
    assert set(counts) == set(A.TRANSITIONS)
    # the plan as the issue of the seam tests states it
    conn = p.descs["conn_index"]
    assert set(np.unique(conn).tolist()) == set(range(A.N_CONNS))
    starts = np.nonzero(np.r_[True, conn[1:] != conn[:-1]])[0]
    lens = np.diff(np.r_[starts, p.n])
    half = p.n // 2 // 64 * 64
    tail_len = 900 if tail == "run" else 40
    first = lens[starts + lens < half]
    assert set(first.tolist()) <= set(A.FIRST_HALF_RUNS.tolist()) and len(set(first.tolist())) == 18
    second = (starts >= half) & (starts + lens < p.n - tail_len)
    assert (starts[second] % 64 == 0).all() and set(lens[second].tolist()) == set(A.SECOND_HALF_RUNS.tolist())
    assert (lens[-1] == 900) if tail == "run" else (lens[-40:] == 1).all()
    assert 0.5 < p.bad[:half].mean() * 1500 < 1.5 and 0.5 < p.bad[half:].mean() * 6000 < 1.6
    # the values
    length, skip = p.descs["length"].astype(np.int64), p.descs["skip_head"].astype(np.int64)
    for v in A.VALUE_CLASSES.tolist():
        assert (length == v).sum() > p.n // 40
    live = ~p.bad
    assert ((skip[live] == 0) | (skip[live] == 26) | (skip[live] == length[live])).all()
    assert ((skip == length + 1) & p.bad).sum() > 10 and ((p.descs["expected_pattern_offset"] >= 65536) & p.bad).sum() > 10
    assert (p.descs["byte_offset"] < 1 << 61).all() and p.arena_bytes == 1 << 62
    assert int((length - skip)[live].sum()) < 1 << 63 and p.base_index + p.n <= 0xFFFFFFFF
    # a tile's sum leaves 32 bits almost everywhere: the per-lane values alone do
    assert ((length - skip)[live] >= 1 << 31).mean() > 0.25
    # the slots: one kind per connection, the ordinals where the walk says
    s, base, span, parked = p.slots.astype(np.int64), p.base_index, p.walked["span"], p.walked["parked"]
    assert s[0] == A.KNONE and s[1] < base and s[2] >= base + p.n
    for c in (3, 4, 5, 6):
        i = int(s[c]) - base
        assert p.keys[i] == c
        w, t, lane = i // span, i % span // 64, i % 64
        if c in (3, 4):
            assert parked[w, t] and parked[w, t + 1] and lane == (0 if c == 3 else 63)
        else:
            assert i % span == (0 if c == 5 else span - 1)


def _older_batches():
    """The keys of the largest batches of the older accounting tests, built as those tests build them."""
    rng = np.random.default_rng(0x7C0)      # test_seven_connections_in_long_runs_the_pass_alone
    yield "seven connections", C.runs_of(1000003, 7, 200000, rng)
    rng = np.random.default_rng(0xC0221)    # test_one_connection_ring_the_pass_alone
    lens = rng.integers(0, 1536 + 40, size=1000003)
    yield "one ring", np.where((lens < 26) | (lens > 1536), A.KNONE, 1).astype(np.uint32)
    i = np.arange(2048 * 256 + 70000)       # test_accumulate_long_spans
    yield "long spans", np.where(i < 300000, 0, np.where(i < 400000, 1 + i % 3, (i // 777) % 4)).astype(np.uint32)


def test_older_batches_never_leave_a_parked_stretch():
    """At 256 compute units the older tests' batches give spans of two tiles: a parked tile is always a span's last
    one, so no wave ever joins parked sums inside its loop or parks twice."""
    for name, keys in _older_batches():
        walked = A.walk(keys, 256)
        counts = walked["counts"]
        print(name, len(keys), counts)
        assert walked["span"] == 128, name
        assert counts["parked_tile"] > 100 and counts["end_parked"] == counts["parked_tile"], name
        for f in ("parked_twice", "unpark_pure_other", "unpark_mixed_merge", "unpark_mixed_nomerge"):
            assert counts[f] == 0, (name, f)


# ---- 3. the models --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", TAILS)
def test_views_in_python_integers(tail):
    """reference_view and connection_view over the plan's first 40 000 descriptors, with slots that switch inside
    them, against one-descriptor-at-a-time sums in Python integers."""
    p = A.plan(256, tail)
    m = 40000
    d, bad, g = p.descs[:m], p.bad[:m], p.ordinals[:m]
    at = [np.nonzero(p.keys[:m] == c)[0] for c in range(A.N_CONNS)]
    assert min(len(a) for a in at) > 1000
    slots = np.array([A.KNONE, 3, p.base_index + p.n, g[at[3][len(at[3]) // 2]], g[at[4][0]], g[at[5][-1]],
                      g[at[6][len(at[6]) // 3]]], dtype=np.uint32)
    want_ref, want_table = A.exact_views(d, bad, g, A.N_CONNS, slots)
    assert want_ref["bytes_recv"] > 1 << 44 and want_ref["bytes_after_failure"] > 1 << 43
    ref, _ = W.reference_view(d, None, g, A.N_CONNS, bad=bad, slots=slots)
    assert ref == want_ref
    table, _ = W.connection_view(d, None, g, A.N_CONNS, bad=bad, slots=slots)
    for c in range(A.N_CONNS):
        assert {f: int(table[f][c]) for f in CONN_STATE_DTYPE.names} == want_table[c], c
    # fewer slots than connections: the others count in the block and in no entry
    ref5, _ = W.reference_view(d, None, g, 5, bad=bad, slots=slots[:5])
    table5, _ = W.connection_view(d, None, g, 5, bad=bad, slots=slots[:5])
    want_ref5, want_table5 = A.exact_views(d, bad, g, 5, slots[:5])
    assert ref5 == want_ref5
    assert [{f: int(table5[f][c]) for f in CONN_STATE_DTYPE.names} for c in range(5)] == want_table5


@pytest.mark.parametrize("with_sizes", (True, False))
def test_close_in_python_integers(with_sizes):
    state, slots, ids, want = A.close_cases(2000)
    expected = want if with_sizes else None
    statuses, counts = A.exact_close(state, slots, ids, expected)
    res, got_counts, state2, slots2 = W.close_results(state, slots, ids, expected)
    assert got_counts == counts and counts["bytes_recv"] > 1 << 42
    if with_sizes:
        assert min(counts.values()) > 50
    inside = ids < len(slots)
    assert 20 < (~inside).sum() < 100 and int(ids.max()) == A.KNONE
    assert res["status"][inside].tolist() == [s for s in statuses if s is not None]
    assert not res["status"][~inside].any() and (res["flags"][~inside] == 1).all()
    for f in CONN_STATE_DTYPE.names:
        assert np.array_equal(res[f][inside], state[f][ids[inside]])
    assert np.array_equal(res["first_fail"][inside], slots[ids[inside]])
    assert (slots2 == A.KNONE).all() and not state2.view(np.uint64).any()
    # equal low words, other high words: the cases a 32-bit comparison gets wrong
    got = state["bytes_recv"][ids[inside]]
    high_only = ((got ^ want[inside]) & np.uint64(0xFFFFFFFF) == 0) & (got != want[inside])
    assert high_only.sum() > 100


# ---- 4. the MediaStream restatements ----------------------------------------------------------------------------------
def test_ms_restatements_against_the_connection_view():
    """The numpy restatements the GPU tests compare with (accumulate, render, close) against
    workload.MediaStreamConnectionView, which the MediaStream CPU tests hold to the reference client: the first 30 000
    datagrams of a plan, and 3 000 preset entries rendered and closed."""
    from ctstraffic_amd.types import MS_CONN_RESULT_DTYPE, MS_CONN_STATE_DTYPE

    p = A.plan(64, "mixed")
    conn, st = A.ms_batch(p)
    m = 30000
    fresh, elems = W.media_stream_conn_entries([A.MS_WINDOW] * A.N_CONNS)
    at = [np.nonzero(p.keys[:m] == c)[0] for c in range(A.N_CONNS)]
    slots = np.array([A.KNONE, 3, p.base_index + p.n] + [p.base_index + at[c][len(at[c]) // 2] for c in (3, 4, 5, 6)],
                     dtype=np.uint32)
    view = W.media_stream_connection_view(fresh, elems, slots=slots)
    view.accumulate(conn[:m], st[:m], p.base_index)
    e, ring, udp = A.ms_accumulate_model(fresh, elems, slots, conn[:m], st[:m], p.base_index)
    for f in MS_CONN_STATE_DTYPE.names:
        assert np.array_equal(e[f], view.entries[f]), f
    assert np.array_equal(ring, view.ring) and udp == view.udp
    assert e["error_frames"].min(initial=9, where=slots != 3) > 0 and (e["has_failure"] == 1).sum() == 4
    assert udp["bits_received"] > 1 << 45 and (conn[:m] >= A.N_CONNS).sum() > 5
    # render and close
    n = 3000
    fresh, elems = W.media_stream_conn_entries([(A.MS_FRAME_SIZE, 1, 3)] * n)
    entries, ring0, kind, slots = A.ms_preset_entries(fresh)
    assert elems == 2 * n and len(np.unique(kind)) == len(A.MS_RENDER_KINDS)
    rng = np.random.default_rng(3)
    ids = np.r_[rng.permutation(n)[: n - 100], [n, n + 7, A.KNONE]]
    view = W.media_stream_connection_view(entries, elems, slots=slots)
    view.ring[:] = ring0
    want_codes = view.render(ids)
    e, ring, codes, udp = A.ms_render_model(entries, ring0, ids)
    assert np.array_equal(codes, want_codes) and set(codes.tolist()) == {0, 1, 2}
    for f in MS_CONN_STATE_DTYPE.names:
        assert np.array_equal(e[f], view.entries[f]), f
    assert np.array_equal(ring, view.ring) and udp == view.udp
    assert min(udp[f] for f in ("successful_frames", "dropped_frames", "duplicate_frames")) > 100
    assert udp["dropped_frames"] > 1 << 36
    close_ids = np.r_[rng.permutation(n)[:1500], [n + 1]]
    want = view.close(close_ids)
    res, e2, ring2, slots2, counts = A.ms_close_model(e, ring, slots, close_ids)
    for f in MS_CONN_RESULT_DTYPE.names:
        assert np.array_equal(res[f], want[f]), f
    for f in MS_CONN_STATE_DTYPE.names:
        assert np.array_equal(e2[f], view.entries[f]), f
    assert np.array_equal(ring2, view.ring) and np.array_equal(slots2, view.slots) and counts == view.close_block
    assert min(counts[f] for f in ("successful", "data_errors", "not_all_data")) > 50 and counts["bytes_recv"] > 1 << 40
