"""CPU: what tests/test_exchange_edges_gpu.py rests on (tests/exchange_edges.py, plan_depths.exchange_tick).

1. The case list holds what it exists for: K, P + Q and P + B - 1 above 2^32, transfers above 2^63, positions above
   2^62, y * C above 2^63, and the named corners.
2. The Python-integer closed forms (workload.tcp_exchange_element, tcp_exchange_position) equal the step-by-step walk
   (workload.tcp_exchange_sequence) started far out, at every edge shape: from the start of a cycle, from the start of
   the last whole cycle to the transfer's end, and where a cycle is astronomically long, at its start, around its
   turn and over the transfer's last 64 buffers.
3. Each modelled defect of the device build (kp32, c32, k32, m48, n32) changes something the GPU test compares.
4. The host C helpers equal the Python integers on every case.
5. The numpy model workload.tcp_exchange_view equals exchange_tick on every case, which is what lets
   tests/far_offsets.py keep the numpy model for its exchange plans.
"""
import numpy as np
import pytest

import exchange_edges as E
import plan_depths as P
from ctstraffic_amd import tcp_exchange as X
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import TCP_EXCHANGE_DTYPE

PUSH, PULL, PUSHPULL, DUPLEX = E.PUSH, E.PULL, E.PUSHPULL, E.DUPLEX


# ---- 1. the case list ------------------------------------------------------------------------------------------------
def test_the_case_list_holds_its_corners():
    cases = E.all_cases()
    assert 1900 <= len(E.cases(1)) <= 2100 and 50 <= len(E.cases(2)) <= 70
    pp = [c for c in cases if c["pattern"] == PUSHPULL]
    have = {"K >= 2^32": sum(1 for c in pp if c["K"] >= 1 << 32),
            "P + Q >= 2^32": sum(1 for c in pp if c["C"] >= 1 << 32),
            "P + B - 1 >= 2^32, B >= 2": sum(1 for c in pp if c["B"] >= 2 and c["P"] + c["B"] - 1 >= 1 << 32),
            "T >= 2^63": sum(1 for c in cases if c["T"] >= 1 << 63),
            "m >= 2^62": sum(1 for c in cases if c["m"] >= 1 << 62),
            "y (P + Q) >= 2^63": sum(1 for c in pp if c["y"] * c["C"] >= 1 << 63)}
    assert all(v >= 20 for v in have.values()), have
    assert any(c["pattern"] == DUPLEX and c["T"] == E.TOP - 2 for c in cases)
    assert any(c["pattern"] == PUSH and c["N"] == E.TOP - 1 and c["m"] == c["N"] - 3 for c in cases)
    assert any(c["pattern"] == PUSHPULL and c["K"] == (1 << 33) - 2 for c in cases)
    for table in (1, 2):
        mine = E.cases(table)
        assert {c["pattern"] for c in mine} == {PUSH, PULL, PUSHPULL, DUPLEX}
        assert {c["B"] for c in mine} == set(E.TABLES[table]["sizes"])
        assert {c["kind"] for c in mine} >= set(E.SEEK_KINDS) - ({"zero", "random"} if table == 2 else set())
        # what the seek kinds promise of a tick of MAX_BUFFERS
        for c in mine:
            if c["kind"] in ("cycle_last", "cycle_far"):
                assert (c["m"] + 2) % c["K"] == 0 and c["m"] + E.MAX_BUFFERS <= c["N"], c
                assert c["kind"] == "cycle_last" or c["y"] >= (1 << 40) // c["K"], c
            elif c["kind"] == "turn":
                assert c["m"] % c["K"] == c["kp"] - 2 and c["m"] + E.MAX_BUFFERS <= c["N"], c
        assert any(c["kind"] == "end_short" and c["N"] - c["m"] == 3 for c in mine)
        assert any(c["kind"] == "end_exact" and c["N"] - c["m"] == E.MAX_BUFFERS for c in mine)
    # the values the shapes are a product of are all drawn
    table1 = E.cases(1)
    assert {c["P"] for c in table1 if c["pattern"] == PUSHPULL} >= {1, 1 << 31, (1 << 31) + 1, (1 << 32) - 2,
                                                                    (1 << 32) - 1}
    for T in (E.TOP - 1, E.TOP - 2, 1 << 63, (1 << 63) + 1, (1 << 62) + 12345):
        assert any(c["T"] == T for c in table1), T
    assert any(c["T"] == 7 * c["B"] + 1 for c in table1) and any(c["T"] == E.TOP - c["B"] - 1 for c in table1)
    assert any(c["pattern"] == PUSHPULL and c["T"] == 10 * c["C"] + c["P"] for c in table1)


def test_the_ticks_cut_and_finish():
    for table in (1, 2):
        ids, capacities = E.ticks_of(table)
        first, second = E.reference(table)
        n = len(ids)
        assert sorted(ids) == list(range(n)) and ids != sorted(ids)
        assert first["tick"]["buffers"] == capacities[0] and 3 not in first["codes"][:-12]
        assert first["codes"][-2:] == [3, 3] and 0 < first["taken"][first["codes"].index(3) - 1] < E.MAX_BUFFERS
        assert 0 in first["codes"] and 1 in first["codes"]
        assert second["tick"]["buffers"] == capacities[1] - 3 and 3 not in second["codes"] and 2 in second["codes"]
        assert first["bytes_dir"][0] and first["bytes_dir"][1]
        # receivers of both directions, full and short buffers, offsets in both byte phases
        slots = first["slots"] + second["slots"]
        assert {r // n for r, _, _ in slots} == {0, 1} and len({ln for _, ln, _ in slots}) >= 3
        assert {off % 2 for _, _, off in slots} == {0, 1}
        assert max(E.TABLES[table]["sizes"]) == max(ln for _, ln, _ in slots) <= E.TABLES[table]["stride"]


# ---- 2. the closed forms against the walk, far out -------------------------------------------------------------------
def _same_as_the_walk(shape, m, count, to_the_end=False):
    """Buffers m .. m + count (to_the_end: and no buffer behind them) by the walk and by the closed forms: direction,
    position, length, intra, and the bytes both directions have sent before every buffer and after the last."""
    pattern, T, B, Pb, Qb = shape
    Te = T + (T % 2 if pattern == DUPLEX else 0)
    got, sent = E.walk_span(pattern, T, B, Pb, Qb, m, count + (1 if to_the_end else 0))
    assert len(got) == count, (shape, m, count, len(got))
    for j, (d, pos, length, intra) in enumerate(got):
        assert W.tcp_exchange_element(pattern, Te, B, Pb, Qb, m + j) == (d, pos, length, intra), (shape, m, j)
        assert W.tcp_exchange_position(pattern, Te, B, Pb, Qb, m + j) == sent, (shape, m, j)
        assert sent[d] == pos and 0 < length <= B
        sent[d] += length
    assert W.tcp_exchange_position(pattern, Te, B, Pb, Qb, m + count) == sent, (shape, m)
    if to_the_end:
        assert sum(sent) == Te and m + count == E.total_buffers(pattern, T, B, Pb, Qb), (shape, m)
    return got


def test_closed_forms_are_the_walk_at_the_edge_shapes():
    shapes = {}
    for c in E.all_cases():
        shapes.setdefault((c["pattern"], c["T"], c["B"], c["P"], c["Q"]), []).append(c)
    assert len(shapes) > 500
    long_cycles = turns_crossed = ends = 0
    for shape, mine in shapes.items():
        pattern, T, B, Pb, Qb = shape
        N = mine[0]["N"]
        far = max(c["m"] for c in mine)
        if pattern != PUSHPULL:
            step = 2 if pattern == DUPLEX else 1
            m = far - far % step
            _same_as_the_walk(shape, m, min(64, N - m), to_the_end=N - m <= 64)
            m = max(N - 64, 0)
            _same_as_the_walk(shape, m, N - m, to_the_end=True)
            continue
        kp, kq, K, C = E.counts(B, Pb, Qb)
        y_far, y_last = far // K, max(T // C - 1, 0)
        for y in {y_far, y_last}:  # from a cycle's start
            got = _same_as_the_walk(shape, y * K, min(2 * K, 64, N - y * K), to_the_end=N - y * K <= min(2 * K, 64))
            assert got[0][0] == 0 and got[0][3] == 0
            turns_crossed += len({d for d, _, _, _ in got}) == 2
        if N - y_last * K <= E.WALK_REACH:  # the last whole cycle and the tail behind it
            _same_as_the_walk(shape, y_last * K, N - y_last * K, to_the_end=True)
            ends += 1
        if K > E.WALK_REACH:
            y = y_far if (y_far + 1) * K <= N else max(y_far - 1, 0)
            if y * K + kp + 64 <= N:  # (a transfer of 7B + 1 ends before its first turn)
                long_cycles += 1
                if kp > 32:  # the 64 around the push-to-pull turn, and the pull segment from its turn on
                    got = _same_as_the_walk(shape, y * K + kp - 32, min(64, 32 + kq))
                    assert [d for d, _, _, _ in got[:33]] == [0] * 32 + [1] and got[32][3] == 0
                got = _same_as_the_walk(shape, y * K + kp, 64)
                assert got[0][0] == 1 and got[0][3] == 0
            m = max(N - 64, 0)
            _same_as_the_walk(shape, m, N - m, to_the_end=True)
            ends += 1
    assert long_cycles >= 20 and turns_crossed >= 100 and ends >= 100, (long_cycles, turns_crossed, ends)


# ---- 3. sensitivity --------------------------------------------------------------------------------------------------
def test_every_defect_of_the_closed_forms_shows():
    good = [E.compared(r) for table in (1, 2) for r in E.reference(table)]
    for defect in P.X_DEFECTS:
        bad = [E.compared(r) for table in (1, 2) for r in E.reference(table, defect)]
        changed = [k for k in range(5) if any(g[k] != b[k] for g, b in zip(good, bad))]
        assert changed, defect
        # and it shows in what a descriptor, a code or an entry holds, not in a sum alone
        assert set(changed) & {0, 1, 2}, (defect, changed)
    # a shape without wide quantities tells none of them apart
    small = [(PUSHPULL, 100_000, 1000, 2500, 1001), (DUPLEX, 9001, 1000), (PUSH, 3001, 1000)]
    for defect in (None,) + P.X_DEFECTS:
        state = P.exchange_state(small, seek=[7, 3, 1])
        got = E.compared(P.exchange_tick(state, [2, 0, 1], 1008, 12, 5, 3, defect))
        assert defect is None or got == plain, defect
        plain = got


# ---- 4. the host helpers ---------------------------------------------------------------------------------------------
def test_host_helpers_are_the_python_integers():
    for table in (1, 2):
        settings, seeks = E.settings_of(table), E.seeks_of(table)
        entries = W.tcp_exchange_entries(settings, seek=seeks)
        assert np.array_equal(entries, P.exchange_records(P.exchange_state(settings, seeks)))
        for c, case in zip(range(len(settings)), E.cases(table)):
            pattern, T, B, Pb, Qb = settings[c]
            Te = T + (T % 2 if pattern == DUPLEX else 0)
            fresh = X.exchange_init(*settings[c])
            assert int(fresh["total_buffers"]) == case["N"] and int(fresh["transfer_bytes"]) == Te, case
            at = X.exchange_seek(fresh, case["m"])
            assert at == entries[c], case
            d, _, _, intra = W.tcp_exchange_element(pattern, Te, B, Pb, Qb, case["m"])
            assert X.exchange_where(at) == (d, intra), case
            end = W.tcp_exchange_position(pattern, Te, B, Pb, Qb, case["N"])
            assert [X.exchange_direction_bytes(at, k) for k in (0, 1)] == end and sum(end) == Te, case
            last = X.exchange_seek(at, case["N"])
            assert last["bytes_sent"].tolist() == end and int(last["finished"]) == 1, case
            # the position five buffers on, where the device's move lands
            on = min(case["m"] + E.MAX_BUFFERS, case["N"])
            assert X.exchange_seek(at, on)["bytes_sent"].tolist() == W.tcp_exchange_position(pattern, Te, B, Pb, Qb, on)


# ---- 5. the numpy model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [1, 2])
def test_the_numpy_model_is_exchange_tick(table):
    stride = E.TABLES[table]["stride"]
    ids, capacities = E.ticks_of(table)
    entries = W.tcp_exchange_entries(E.settings_of(table), seek=E.seeks_of(table))
    n = len(entries)
    arena = np.full(max(capacities) * stride, 0xA5, dtype=np.uint8)
    mine = arena.copy()
    counters = None
    for t, (capacity, ref) in enumerate(zip(capacities, E.reference(table))):
        v = W.tcp_exchange_view(entries, stride, arena, 0, capacity, ids, E.MAX_BUFFERS, counters=counters)
        entries, arena, counters = v.entries, v.arena, v.counters
        total = ref["tick"]["buffers"]
        assert v.codes.tolist() == ref["codes"], t
        assert [int(x) for x in v.prefix] == ref["prefix"] and [int(x) for x in v.taken] == ref["taken"], t
        assert v.tick == dict(ref["tick"], bytes_dir=ref["bytes_dir"]), t
        got = list(zip(v.descs["conn_index"][:total].tolist(), v.descs["length"][:total].tolist(),
                       v.descs["expected_pattern_offset"][:total].tolist()))
        assert got == ref["slots"], t
        assert v.descs["byte_offset"][:total].tolist() == [g * stride for g in range(total)]
        assert np.array_equal(entries, P.exchange_records(ref["entries"])), t
        assert np.array_equal(arena, E.arena_after(mine, ref["slots"], 0, stride)), t
    assert counters["bytes_sent"] == sum(r["tick"]["bytes"] for r in E.reference(table))
    assert entries.dtype == TCP_EXCHANGE_DTYPE and n == len(ids)
