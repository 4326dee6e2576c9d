"""CPU: connections on the device (include/cts_connections.h) without a device: the struct layouts against the numpy
mirrors, the argument checks of every new entry point (they come before the engine is used), and the three model
functions of ctstraffic_amd.workload (connection_view, close_results, rebase_slots) on the reference-view plans."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import connection_plans as C
import refview_plans as P
from ctstraffic_amd import _lib
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import CLOSE_FIELDS, CONN_RESULT_DTYPE, CONN_RESULT_FLAG_BAD_CONN, CONN_STATE_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
EMPTY = 0xFFFFFFFF


def test_struct_layouts_match_c():
    """Compile a probe against include/cts_connections.h and compare sizeof/offsetof and the status values."""
    state_f, result_f = CONN_STATE_DTYPE.names, CONN_RESULT_DTYPE.names
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"cts_connections.h\"\nint main(void){\n"
    probe += ' printf("%zu %zu %zu\\n", sizeof(cts_conn_state), sizeof(cts_conn_result), sizeof(cts_counters_close));\n'
    for struct, fields in (("cts_conn_state", state_f), ("cts_conn_result", result_f), ("cts_counters_close", CLOSE_FIELDS)):
        probe += ' printf("%s\\n", %s);\n' % (" ".join(["%zu"] * len(fields)),
                                             ", ".join("offsetof(%s,%s)" % (struct, f) for f in fields))
    probe += (' printf("%u %u %u %u\\n", CTS_STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN, '
              "CTS_STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED, CTS_STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED, "
              "CTS_CONN_RESULT_FLAG_BAD_CONN);\n return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(probe)
        exe = os.path.join(d, "p")
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INCLUDE, c, "-o", exe], check=True)
        lines = [list(map(int, ln.split())) for ln in
                 subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")]
    assert lines[0] == [CONN_STATE_DTYPE.itemsize, CONN_RESULT_DTYPE.itemsize, ctypes.sizeof(_lib.CtsCountersClose)]
    assert lines[0] == [32, 48, 48]
    assert lines[1] == [CONN_STATE_DTYPE.fields[f][1] for f in state_f]
    assert lines[2] == [CONN_RESULT_DTYPE.fields[f][1] for f in result_f]
    assert lines[3] == [getattr(_lib.CtsCountersClose, f).offset for f in CLOSE_FIELDS] == [8 * k for k in range(6)]
    assert [f for f, _ in _lib.CtsCountersClose._fields_] == list(CLOSE_FIELDS) == list(W.CLOSE_FIELDS)
    assert lines[4] == [_lib.STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN, _lib.STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED,
                        _lib.STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED, CONN_RESULT_FLAG_BAD_CONN]
    assert lines[4][:3] == [W.STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN, W.STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED,
                            W.STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED] == [2**31 - 4, 2**31 - 3, 2**31 - 2]
    from ctstraffic_amd.distributed import CLOSE_FIELDS as D_CLOSE

    assert D_CLOSE == CLOSE_FIELDS


def test_entry_points_refuse_bad_arguments_without_a_device():
    """A null engine, a null or misaligned slot array or entry table with n_conns != 0, and base_index + n past
    0xFFFFFFFF are CTS_E_INVALID from every new entry point before anything touches the engine or a device (the
    engine handle below is never dereferenced: the checks come first)."""
    L = _lib.lib()
    INV = _lib.CTS_E_INVALID
    buf = (ctypes.c_uint64 * 16)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    eng = p + 64  # a non-null handle that is no engine
    acc = L.cts_refview_accumulate_conns
    accs = L.cts_refview_accumulate_conns_strided
    close, rebase = L.cts_conns_close, L.cts_conn_slots_rebase
    # a null engine
    assert acc(None, 64, p, 1, 0, p, 1, p, p, None) == INV
    assert accs(None, 64, 64, p, 1, 0, 0, 0, p, 1, p, p, None) == INV
    assert close(None, p, p, 1, p, p, 1, p, p, None) == INV
    assert rebase(None, p, 1, 1, None) == INV
    out = _lib.CtsCountersClose()
    assert L.cts_counters_read_close(None, p, ctypes.byref(out), None) == INV
    assert L.cts_counters_read_close(None, p, None, None) == INV
    assert L.cts_counters_read_multi_close(None, None, None, 1, ctypes.byref(out)) == INV
    assert L.cts_counters_allreduce_close(None, None, None, 1, ctypes.byref(out)) == INV
    # the tables: null or misaligned with n_conns != 0
    for slots, state in ((None, p), (p, None), (p + 2, p), (p, p + 4)):
        assert acc(eng, 64, p, 1, 0, slots, 1, p, state, None) == INV
        assert accs(eng, 64, 64, p, 1, 0, 0, 0, slots, 1, p, state, None) == INV
        assert close(eng, p, p, 1, slots, state, 1, p, p, None) == INV
    assert rebase(eng, None, 1, 1, None) == INV and rebase(eng, p + 2, 1, 1, None) == INV
    # the other pointers
    assert acc(eng, 64, None, 1, 0, p, 1, p, p, None) == INV and acc(eng, 64, p + 4, 1, 0, p, 1, p, p, None) == INV
    assert acc(eng, 64, p, 1, 0, p, 1, None, p, None) == INV and acc(eng, 64, p, 1, 0, p, 1, p + 4, p, None) == INV
    assert accs(eng, 64, 64, None, 1, 0, 0, 0, p, 1, p, p, None) == INV
    assert accs(eng, 64, 0, p, 1, 0, 0, 0, p, 1, p, p, None) == INV  # stride 0
    assert close(eng, None, p, 1, p, p, 1, p, p, None) == INV and close(eng, p + 2, p, 1, p, p, 1, p, p, None) == INV
    assert close(eng, p, p + 4, 1, p, p, 1, p, p, None) == INV and close(eng, p, p, 1, p, p, 1, p + 4, p, None) == INV
    assert close(eng, p, p, 1, p, p, 1, p, None, None) == INV and close(eng, p, p, 1, p, p, 1, p, p + 4, None) == INV
    # the ordinal limit: base_index + n == 0xFFFFFFFF is the last launch, one more is refused
    assert acc(eng, 64, p, 2, EMPTY - 1, p, 1, p, p, None) == INV
    assert acc(eng, 64, p, 1, EMPTY, p, 1, p, p, None) == INV
    assert accs(eng, 64, 64, p, 2, 0, 0, EMPTY - 1, p, 1, p, p, None) == INV
    assert accs(eng, 64, 64, p, EMPTY, 0, 0, 1, p, 1, p, p, None) == INV
    # nothing to do is CTS_OK, still without a device
    assert acc(eng, 64, p, 0, 0, p, 1, p, p, None) == _lib.CTS_OK
    assert accs(eng, 64, 64, p, 0, 0, 0, 0, p, 1, p, p, None) == _lib.CTS_OK
    assert close(eng, p, p, 0, p, p, 1, p, p, None) == _lib.CTS_OK
    assert rebase(eng, p, 0, 5, None) == _lib.CTS_OK and rebase(eng, p, 5, 0, None) == _lib.CTS_OK
    assert not any(buf)


PLAN_NAMES = ("wg", "ragged", "quad")


@pytest.mark.parametrize("name", PLAN_NAMES)
def test_connection_view_sums_to_the_reference_view(name):
    w, launches, ordinals, facts = P.plan(name)
    failed = P.plan_failed_mask(w)
    sums, slots = W.reference_view(w.descs, failed, ordinals, w.n_conns)
    table, tslots = W.connection_view(w.descs, failed, ordinals, w.n_conns)
    assert table.dtype == CONN_STATE_DTYPE and table.shape == (w.n_conns,) and np.array_equal(tslots, slots)
    for f in CONN_STATE_DTYPE.names:
        assert int(table[f].sum()) == sums[f], f
    assert int((slots != EMPTY).sum()) == facts["failed"]
    # a clean connection received everything; a failed one its prefix through the failing buffer
    bpc = P.PLANS[name][0]["buffers_per_conn"]
    vlen = (w.descs["length"].astype(np.int64) - w.descs["skip_head"].astype(np.int64)).reshape(-1, bpc)
    grid = failed.reshape(-1, bpc)
    for c in range(w.n_conns):
        k = int(grid[c].argmax()) + 1 if grid[c].any() else bpc
        assert (int(table["bytes_recv"][c]), int(table["buffers_recv"][c])) == (int(vlen[c, :k].sum()), k)
        assert (int(table["bytes_after_failure"][c]), int(table["buffers_after_failure"][c])) == \
            (int(vlen[c, k:].sum()), bpc - k)
    # launch by launch with the final slots, the tables add up to the whole
    acc = np.zeros(w.n_conns, dtype=CONN_STATE_DTYPE)
    for d, base, idx in launches:
        t, _ = W.connection_view(d, None, base + np.arange(len(d)), w.n_conns, slots=slots)
        for f in CONN_STATE_DTYPE.names:
            acc[f] += t[f]
    assert np.array_equal(acc, table)


def test_a_connection_failing_on_its_first_buffer_holds_exactly_that_buffer():
    w, _, ordinals, facts = P.plan("wg")
    failed = P.plan_failed_mask(w)
    table, slots = W.connection_view(w.descs, failed, ordinals, w.n_conns)
    first = np.nonzero(failed.reshape(-1, 48)[:, 0])[0]
    assert len(first) == facts["first_buffer"] == 2
    for c in first:
        assert slots[c] == ordinals[c * 48]
        assert tuple(int(x) for x in table[c]) == (65536, 1, 47 * 65536, 47)


def test_connection_view_leaves_out_slotless_connections_and_bad_descriptors():
    w, _, ordinals, _ = P.plan("quad")
    failed = P.plan_failed_mask(w)
    n_conns = 150  # connections 150..199 have no slot
    bad = np.zeros(w.n, dtype=bool)
    bad[::11] = True
    sums, slots = W.reference_view(w.descs, failed, ordinals, n_conns, bad=bad)
    table, _ = W.connection_view(w.descs, failed, ordinals, n_conns, bad=bad)
    inside = (w.descs["conn_index"] < n_conns) & ~bad
    vlen = w.descs["length"].astype(np.int64) - w.descs["skip_head"].astype(np.int64)
    assert int(table["bytes_recv"].sum() + table["bytes_after_failure"].sum()) == int(vlen[inside].sum())
    assert int(table["buffers_recv"].sum() + table["buffers_after_failure"].sum()) == int(inside.sum())
    assert sums["buffers_recv"] + sums["buffers_after_failure"] == int((~bad).sum()) > int(inside.sum())


def test_close_results_classes_partition_the_closed_connections():
    w, _, ordinals, facts = P.plan("wg")
    table, slots = W.connection_view(w.descs, P.plan_failed_mask(w), ordinals, w.n_conns)
    want = C.expected_bytes(table, slots)
    ids = np.arange(w.n_conns)[::-1]
    res, counts, state2, slots2 = W.close_results(table, slots, ids, want[ids])
    assert res.dtype == CONN_RESULT_DTYPE and list(res["conn_index"]) == list(ids)
    classes = [counts[f] for f in ("successful", "data_errors", "not_all_data", "too_much_data")]
    assert sum(classes) == counts["connections_closed"] == w.n_conns and min(classes) > 0
    assert counts["data_errors"] == facts["failed"] and counts["bytes_recv"] == int(table["bytes_recv"].sum())
    by_status = {0: "successful", W.STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN: "data_errors",
                 W.STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED: "not_all_data",
                 W.STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED: "too_much_data"}
    for s, f in by_status.items():
        assert int((res["status"] == s).sum()) == counts[f]
    # the data error wins: a failed connection short of its size is still a data error
    failed_short = (res["first_fail"] != EMPTY) & (res["bytes_recv"] < want[ids])
    assert failed_short.any() and (res["status"][failed_short] == W.STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN).all()
    assert (res["first_fail"] == slots[ids]).all() and (res["bytes_recv"] == table["bytes_recv"][ids]).all()
    assert (slots2 == EMPTY).all() and not state2.view(np.uint64).any()
    assert (slots != EMPTY).any() and table.view(np.uint64).any()  # the inputs are left alone
    # no sizes: only data errors and successes
    _, c2, _, _ = W.close_results(table, slots, ids, None)
    assert (c2["not_all_data"], c2["too_much_data"]) == (0, 0) and c2["successful"] == facts["clean"]
    # a subset, and an id without a slot
    sub = np.array([5, 200, 7])
    r3, c3, st3, sl3 = W.close_results(table, slots, sub, want[[5, 0, 7]])
    assert c3["connections_closed"] == 2 and r3["flags"].tolist() == [0, CONN_RESULT_FLAG_BAD_CONN, 0]
    assert tuple(int(x) for x in r3[1]) == (0, 0, 0, 0, 0, 0, 200, CONN_RESULT_FLAG_BAD_CONN)
    keep = np.ones(w.n_conns, bool)
    keep[[5, 7]] = False
    assert np.array_equal(sl3[keep], slots[keep]) and np.array_equal(st3[keep], table[keep])
    assert (sl3[~keep] == EMPTY).all() and not st3[~keep].view(np.uint64).any()


def test_rebase_slots_keeps_empty_slots_and_clamps_at_zero():
    s = np.array([EMPTY, 0, 9, 10, 11, EMPTY - 1], dtype=np.uint32)
    assert W.rebase_slots(s, 10).tolist() == [EMPTY, 0, 0, 0, 1, EMPTY - 11]
    assert W.rebase_slots(s, 0).tolist() == s.tolist()
    assert W.rebase_slots(s, EMPTY - 1).tolist() == [EMPTY, 0, 0, 0, 0, 0]
    assert W.rebase_slots(s, 10).dtype == np.uint32
    # a rebased run classifies as the unrebased one: ordinals and slots drop together
    w, launches, ordinals, _ = P.plan("wg")
    failed = P.plan_failed_mask(w)
    table, slots = W.connection_view(w.descs, failed, ordinals, w.n_conns)
    delta = launches[2][1] - 1  # strictly below the lowest ordinal of launch 3
    d3, _, idx3 = launches[2]
    before = np.concatenate([idx for _, _, idx in launches[:2]])
    _, slots12 = W.reference_view(w.descs[before], failed[before], ordinals[before], w.n_conns)
    t12, _ = W.connection_view(w.descs[before], None, ordinals[before], w.n_conns, slots=slots12)
    slots3 = np.minimum(W.rebase_slots(slots12, delta),
                        W.reference_view(d3, failed[idx3], 1 + np.arange(len(d3)), w.n_conns)[1])
    t3, _ = W.connection_view(d3, None, 1 + np.arange(len(d3)), w.n_conns, slots=slots3)
    # (launch 1-2 entries were added under slots12, which launch 3 can only lower to ordinals above theirs)
    for f in CONN_STATE_DTYPE.names:
        assert np.array_equal(t12[f] + t3[f], table[f]), f
    assert np.array_equal(slots3, W.rebase_slots(slots, delta))


# INTEGRATION.md "Connection close on the device-resident path": first line of each block -> the parameters that
# declare its free variables (compiled as tests/test_integration_snippets.py compiles the other fragments)
CLOSE_FRAGMENTS = {
    "per_batch": ("// device-resident receive with connections, per batch k",
                  "cts_engine* e, const void* arena, uint64_t arena_bytes, const cts_buf_desc* descs_k, uint32_t n_k, "
                  "uint32_t ordinal, cts_verify_result* results_k, void* ctr, uint32_t* conn_first_fail, "
                  "uint32_t n_conns, void* refs, cts_conn_state* conn_state, void* stream"),
    "close": ("// ctsSocketState.cpp:221-232, where closed sockets update ConnectionStatusDetails",
              "cts_engine* e, const uint32_t* closing, const uint64_t* transfer, uint32_t n_closing, "
              "uint32_t* conn_first_fail, cts_conn_state* conn_state, uint32_t n_conns, cts_conn_result* close_results, "
              "void* closes, void* stream, cts_engine* const* engines, const void* const* close_blocks, "
              "void* const* streams, uint32_t gpu_count, bool rccl"),
    "rebase": ("// now and then (for instance when ordinal passes 2^31)",
               "cts_engine* e, uint32_t* conn_first_fail, uint32_t n_conns, uint32_t delta, uint32_t ordinal, "
               "void* stream"),
}


@pytest.mark.parametrize("name", sorted(CLOSE_FRAGMENTS))
def test_integration_close_fragment_compiles(name):
    import test_integration_snippets as T

    first, params = CLOSE_FRAGMENTS[name]
    found = [c for c in T._all_blocks() if c.startswith(first)]
    assert len(found) == 1, "INTEGRATION.md lost the %s block" % name
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, name + ".cpp")
        with open(src, "w", encoding="utf-8") as f:
            f.write(T.FRAGMENT_PRELUDE + '#include "cts_connections.h"\nvoid snippet(' + params + ")\n{\n" +
                    found[0] + "\n}\n")
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                            "-I", INCLUDE, src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
