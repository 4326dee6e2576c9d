"""CPU: MediaStream connections on the device-resident path (include/cts_media_stream_conns.h): the numpy model
workload.media_stream_connection_view against the two checkers (oracle.media_stream.ClientModel and the C
MediaStreamClient, one per connection), the plans' coverage, cts_ms_conn_init, the struct layouts, the argument
checks, the kernels' symbol inventory, the INTEGRATION.md fragment and the world-2 all-reduce of a UDP block.

The kernels are checked against the same model in tests/test_media_stream_conns_gpu.py. All comparisons are exact.
"""
import ctypes
import os
import re
import socket
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ms_conn_plans as P
from oracle import media_stream as OM
from ctstraffic_amd import _lib
from ctstraffic_amd import distributed as D
from ctstraffic_amd import media_stream as M
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import (MS_CONN_RESULT_DTYPE, MS_CONN_RESULT_FLAG_HAS_FAILURE, MS_CONN_RESULT_FLAG_RUNNING,
                                  MS_CONN_STATE_DTYPE, UDP_FIELDS)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("bits_received", "successful_frames", "dropped_frames", "duplicate_frames", "error_frames", "datagrams",
         "last_error", "finished", "head_sequence_number")


def _checkers(p, statuses):
    """One ClientModel and one C MediaStreamClient per connection, driven batch by batch: the connection's datagrams
    in ordinal order, then the batch's ticks (a failed connection is not rendered again)."""
    oms = [OM.ClientModel(*s) for s in p.settings]
    cms = [M.MediaStreamClient(s[0], s[1], s[2], datagram_max_size=p.max_datagram) for s in p.settings]
    for b, st in zip(p.batches, statuses):
        conn = b.descs["conn_index"]
        for c in range(p.n_conns):
            mine = st[conn == c]
            for d in mine:
                oms[c].complete(int(d["kind"]), int(d["sequence_number"]), int(d["completed_bytes"]), bool(d["pass"]))
            cms[c].complete_status(mine)
        for _ in range(b.ticks):
            for c in range(p.n_conns):
                if oms[c].last_error == P.RUNNING:
                    oms[c].render()
                if cms[c].stats()["last_error"] == P.RUNNING:
                    cms[c].render()
    return oms, cms


@pytest.mark.parametrize("name", sorted(P.PLANS))
def test_model_agrees_with_both_clients(name):
    p, statuses = P.plan(name), P.plan_statuses(name)
    view = P.run_model(p, statuses)
    oms, cms = _checkers(p, statuses)
    e = view.entries
    for c in range(p.n_conns):
        mine = {f: int(e[f][c]) for f in STATS}
        assert mine == oms[c].stats(), (name, c, p.roles[c])
        cs = cms[c].stats()
        assert mine == {f: cs[f] for f in STATS}, (name, c, p.roles[c])
        assert bool(e["has_failure"][c]) == bool(cs["has_failure"]) == (oms[c].fail_datagram is not None)
        if cs["has_failure"]:
            assert int(e["datagrams"][c]) - 1 == cs["fail_datagram"] == oms[c].fail_datagram
    # the node-wide block is the sum of the entries (every connection has a slot here)
    for f in UDP_FIELDS:
        assert view.udp[f] == int(e[f].sum()), f
    # the close: the entry's status, a running stream NotAllData; every slot and ring empty afterwards
    before = view.entries.copy()
    res = view.close(np.arange(p.n_conns))
    running = before["last_error"] == P.RUNNING
    assert np.array_equal(res["status"], np.where(running, P.NOT_ALL_DATA, before["last_error"]))
    assert np.array_equal((res["flags"] & MS_CONN_RESULT_FLAG_RUNNING) != 0, running)
    assert np.array_equal((res["flags"] & MS_CONN_RESULT_FLAG_HAS_FAILURE) != 0, before["has_failure"] != 0)
    assert (view.slots == W.EMPTY_SLOT).all() and not view.ring.any() and (view.entries["finished"] != 0).all()
    assert view.close_block["connections_closed"] == p.n_conns
    assert view.close_block["bytes_recv"] == int((before["bits_received"] // 8).sum())
    assert (view.close_block["successful"] + view.close_block["data_errors"] + view.close_block["not_all_data"]
            == p.n_conns) and view.close_block["too_much_data"] == 0


@pytest.mark.parametrize("name", ["mixed", "mixed_interleaved"])
def test_plans_hold_every_outcome_and_every_class(name):
    """Nothing above passes vacuously: the mixed plans end connections in every way and carry every class of
    datagram; exceptions sit in several connections, some with more than one, one in a batch's first datagram and one
    in a batch's last."""
    p, statuses = P.plan(name), P.plan_statuses(name)
    classes, exceptions = [], []

    def on_batch(view, k, conn, st):
        classes.extend(P.classify(view, conn, st, p.batches[k].base_index))
        exceptions.append((conn, W.datagram_exceptions(st["kind"], st["pass"])))

    view = P.run_model(p, statuses, on_batch)
    e = view.entries
    by_datagram = e["has_failure"] != 0
    assert ((e["finished"] == 1) & (e["last_error"] == 0)).any()                       # finished successfully
    assert (by_datagram & (e["last_error"] == P.DATA_MISMATCH)).any()                  # data mismatch
    assert (by_datagram & (e["last_error"] == P.NOT_ALL_DATA)).any()                   # short, unknown or zero
    assert ((e["finished"] == 2) & (e["last_error"] == P.NOT_ALL_DATA) & ~by_datagram).any()  # FatalAbort
    assert (e["last_error"] == P.RUNNING).any()                                        # still running at close
    for cls in ("in_window", "stale", "future", "past_final", "id", "after_end", "fails_stream"):
        assert cls in classes, cls
    assert (e["duplicate_frames"] > 0).any()                                           # duplicate-making
    assert ((e["dropped_frames"] > 0) & (e["finished"] != 2)).any()                    # a frame left short
    kinds = np.concatenate([st["kind"] for st in statuses])
    assert set(kinds.tolist()) == {W.DGRAM_DATA, W.DGRAM_ID, W.DGRAM_ZERO, W.DGRAM_SHORT, W.DGRAM_UNKNOWN,
                                   W.DGRAM_BAD_DESC}
    per_conn = np.zeros(p.n_conns, dtype=np.int64)
    for conn, exc in exceptions:
        np.add.at(per_conn, conn[exc], 1)
    assert (per_conn > 0).sum() >= 5 and (per_conn > 1).any()
    if name == "mixed":
        assert exceptions[0][1][0] and exceptions[-1][1][-1]
    assert {2, 8, 600} <= set(e["frames"].tolist())
    assert 5000 <= sum(len(b.descs) for b in p.batches) <= 7000
    lens = np.concatenate([b.descs["length"] for b in p.batches])
    assert lens.max() == 1472 and len(set(lens.tolist())) > 6


def test_interleaved_neighbours_differ_and_orders_agree():
    """The interleaved order puts no two datagrams of one connection side by side while several connections still
    have datagrams, keeps every connection's own order, and so ends every connection exactly as connection-major."""
    a, b = P.plan("mixed"), P.plan("mixed_interleaved")
    conn = P.plan("bulk_interleaved").batches[0].descs["conn_index"]
    assert (conn[1:] != conn[:-1]).all()
    va, vb = P.run_model(a, P.plan_statuses("mixed")), P.run_model(b, P.plan_statuses("mixed_interleaved"))
    for f in MS_CONN_STATE_DTYPE.names:
        assert np.array_equal(va.entries[f], vb.entries[f]), f
    assert np.array_equal(va.ring, vb.ring) and va.udp == vb.udp


SETTINGS_CASES = [
    (4000, 4, 100, True), (1500, 1, 1, True), (1500, 300, 7, True), (1, 1, 0xFFFFFFFF, True),
    (0, 4, 100, False), (4000, 0, 100, False), (4000, 4, 0, False), (4000, 4, -3, False),
    (4000, 4, 0x100000000, False),
]


@pytest.mark.parametrize("frame,buffered,length,ok", SETTINGS_CASES)
def test_conn_init_follows_client_create(frame, buffered, length, ok):
    """cts_ms_conn_init accepts and refuses what cts_media_stream_client_create does, and opens the same window."""
    if not ok:
        with pytest.raises(_lib.CtsError):
            M.MediaStreamClient(frame, buffered, length)
        with pytest.raises(_lib.CtsError):
            M.conn_init(frame, buffered, length)
        with pytest.raises(ValueError):
            W.media_stream_conn_entries([(frame, buffered, length)])
        return
    cm = M.MediaStreamClient(frame, buffered, length)
    w = cm.window()
    e = M.conn_init(frame, buffered, length, frame_base=12345)
    assert (e["head_sequence_number"], e["final_frame"], e["frames"]) == (w.head_sequence_number, w.final_frame,
                                                                          w.frames)
    assert e["frames"] == 2 * min(length, buffered) and e["initial_buffer_frames"] == e["timer_wheel_offset"]
    assert e["frame_base"] == 12345 and e["last_error"] == P.RUNNING and e["frame_size_bytes"] == frame
    model, elems = W.media_stream_conn_entries([(7, 1, 1), (frame, buffered, length)])
    assert elems == 2 + e["frames"] and model[1]["frame_base"] == 2
    for f in MS_CONN_STATE_DTYPE.names:
        if f != "frame_base":
            assert model[1][f] == e[f], f
    s = M.Settings(frame, 1400, 0, buffered, length)  # frames_per_second 0: refused as by the client
    assert _lib.lib().cts_ms_conn_init(ctypes.addressof(s), 0, np.zeros(1, MS_CONN_STATE_DTYPE).ctypes.data) == \
        _lib.CTS_E_INVALID
    assert _lib.lib().cts_ms_conn_init(None, 0, None) == _lib.CTS_E_INVALID


def test_struct_layouts_match_c():
    """cts_ms_conn_state is 112 bytes and cts_ms_conn_result 88, 8-byte aligned, field for field as the dtypes; a UDP
    block names six u64."""
    assert MS_CONN_STATE_DTYPE.itemsize == 112 and MS_CONN_RESULT_DTYPE.itemsize == 88
    assert ctypes.sizeof(_lib.CtsCountersUdp) == 48
    assert tuple(f for f, _ in _lib.CtsCountersUdp._fields_) == UDP_FIELDS == W.UDP_FIELDS == D.UDP_FIELDS
    fields = [("cts_ms_conn_state", f) for f in MS_CONN_STATE_DTYPE.names] + \
             [("cts_ms_conn_result", f) for f in MS_CONN_RESULT_DTYPE.names] + \
             [("cts_counters_udp", f) for f in UDP_FIELDS]
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "cts_media_stream_conns.h"\nint main(void){\n'
    probe += ' printf("%zu %zu %zu %zu %zu\\n", sizeof(cts_ms_conn_state), sizeof(cts_ms_conn_result), ' \
             'sizeof(cts_counters_udp), _Alignof(cts_ms_conn_state), _Alignof(cts_ms_conn_result));\n'
    for t, f in fields:
        probe += ' printf("%%zu\\n", offsetof(%s, %s));\n' % (t, f)
    probe += " return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        with open(c, "w") as f:
            f.write(probe)
        exe = os.path.join(d, "p")
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    assert got[:5] == [112, 88, 48, 8, 8]
    want = [MS_CONN_STATE_DTYPE.fields[f][1] for f in MS_CONN_STATE_DTYPE.names] + \
           [MS_CONN_RESULT_DTYPE.fields[f][1] for f in MS_CONN_RESULT_DTYPE.names] + [8 * k for k in range(6)]
    assert got[5:] == want


def test_entry_points_refuse_bad_arguments_before_the_engine():
    """Every argument check comes before the engine is used: with no engine every call is CTS_E_INVALID, and with a
    stand-in engine pointer that must never be read, a null or misaligned argument is CTS_E_INVALID and n == 0 is
    CTS_OK."""
    L, INV = _lib.lib(), _lib.CTS_E_INVALID
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    assert p % 16 == 0 or (p + 8) % 16 == 0
    a16 = p if p % 16 == 0 else p + 8
    for e in (None, a16):
        bad = e is None
        # n == 0: CTS_OK with any engine, CTS_E_INVALID without one
        assert L.cts_media_stream_verify_status_at(e, a16, 64, a16, 0, 0, a16, a16, a16, 1, None) == (INV if bad else 0)
        assert L.cts_media_stream_conns_accumulate(e, 64, a16, a16, 0, 0, a16, a16, a16, 1, 1, a16, None) == \
            (INV if bad else 0)
        assert L.cts_media_stream_conns_render(e, a16, 0, a16, a16, 1, a16, None, None) == (INV if bad else 0)
        assert L.cts_media_stream_conns_close(e, a16, 0, a16, a16, a16, 1, None, a16, None) == (INV if bad else 0)
        V = L.cts_media_stream_verify_status_at
        assert V(e, None, 64, a16, 1, 0, a16, a16, a16, 1, None) == INV          # no arena
        assert V(e, a16 + 8, 64, a16, 1, 0, a16, a16, a16, 1, None) == INV       # arena not 16-byte aligned
        assert V(e, a16, 64, None, 1, 0, a16, a16, a16, 1, None) == INV          # no descriptors
        assert V(e, a16, 64, a16 + 4, 1, 0, a16, a16, a16, 1, None) == INV       # descriptors not 8-byte aligned
        assert V(e, a16, 64, a16, 1, 0, a16 + 2, a16, a16, 1, None) == INV       # statuses
        assert V(e, a16, 64, a16, 1, 0, a16, a16 + 4, a16, 1, None) == INV       # counters
        assert V(e, a16, 64, a16, 1, 0, a16, a16, a16 + 2, 1, None) == INV       # slots
        assert V(e, a16, 64, a16, 1, 0, a16, a16, None, 1, None) == INV          # connections without slots
        assert V(e, a16, 64, a16, 2, 0xFFFFFFFE, a16, a16, a16, 1, None) == INV  # the ordinal limit
        A = L.cts_media_stream_conns_accumulate
        assert A(e, 64, None, a16, 1, 0, a16, a16, a16, 1, 1, a16, None) == INV
        assert A(e, 64, a16 + 4, a16, 1, 0, a16, a16, a16, 1, 1, a16, None) == INV
        assert A(e, 64, a16, None, 1, 0, a16, a16, a16, 1, 1, a16, None) == INV
        assert A(e, 64, a16, a16 + 4, 1, 0, a16, a16, a16, 1, 1, a16, None) == INV
        assert A(e, 64, a16, a16, 1, 0, None, a16, a16, 1, 1, a16, None) == INV
        assert A(e, 64, a16, a16, 1, 0, a16 + 2, a16, a16, 1, 1, a16, None) == INV
        assert A(e, 64, a16, a16, 1, 0, a16, None, a16, 1, 1, a16, None) == INV
        assert A(e, 64, a16, a16, 1, 0, a16, a16 + 4, a16, 1, 1, a16, None) == INV
        assert A(e, 64, a16, a16, 1, 0, a16, a16, None, 1, 1, a16, None) == INV
        assert A(e, 64, a16, a16, 1, 0, a16, a16, a16 + 4, 1, 1, a16, None) == INV
        assert A(e, 64, a16, a16, 1, 0, a16, a16, a16, 1, 1, None, None) == INV
        assert A(e, 64, a16, a16, 1, 0, a16, a16, a16, 1, 1, a16 + 4, None) == INV
        assert A(e, 64, a16, a16, 2, 0xFFFFFFFE, a16, a16, a16, 1, 1, a16, None) == INV
        R = L.cts_media_stream_conns_render
        assert R(e, None, 1, a16, a16, 1, a16, None, None) == INV
        assert R(e, a16 + 2, 1, a16, a16, 1, a16, None, None) == INV
        assert R(e, a16, 1, None, a16, 1, a16, None, None) == INV
        assert R(e, a16, 1, a16 + 4, a16, 1, a16, None, None) == INV
        assert R(e, a16, 1, a16, None, 1, a16, None, None) == INV
        assert R(e, a16, 1, a16, a16 + 4, 1, a16, None, None) == INV
        assert R(e, a16, 1, a16, a16, 1, None, None, None) == INV
        assert R(e, a16, 1, a16, a16, 1, a16 + 4, None, None) == INV
        assert R(e, a16, 1, a16, a16, 1, a16, a16 + 2, None) == INV
        C = L.cts_media_stream_conns_close
        assert C(e, None, 1, a16, a16, a16, 1, None, a16, None) == INV
        assert C(e, a16 + 2, 1, a16, a16, a16, 1, None, a16, None) == INV
        assert C(e, a16, 1, None, a16, a16, 1, None, a16, None) == INV
        assert C(e, a16, 1, a16 + 2, a16, a16, 1, None, a16, None) == INV
        assert C(e, a16, 1, a16, None, a16, 1, None, a16, None) == INV
        assert C(e, a16, 1, a16, a16 + 4, a16, 1, None, a16, None) == INV
        assert C(e, a16, 1, a16, a16, None, 1, None, a16, None) == INV
        assert C(e, a16, 1, a16, a16, a16 + 4, 1, None, a16, None) == INV
        assert C(e, a16, 1, a16, a16, a16, 1, a16 + 4, a16, None) == INV
        assert C(e, a16, 1, a16, a16, a16, 1, None, None, None) == INV
        assert C(e, a16, 1, a16, a16, a16, 1, None, a16 + 4, None) == INV
    out = _lib.CtsCountersUdp()
    assert L.cts_counters_read_udp(None, p, ctypes.byref(out), None) == INV
    assert L.cts_counters_read_udp(None, p, None, None) == INV
    assert L.cts_counters_read_multi_udp(None, None, None, 1, ctypes.byref(out)) == INV
    assert L.cts_counters_allreduce_udp(None, None, None, 1, ctypes.byref(out)) == INV


def test_product_library_carries_the_media_stream_connection_kernels():
    """Next to the kernels tests/test_abi.py and tests/test_refview_cpu.py list, the library holds the status-form
    receive pass with ordinals and the accounting pass, each for nontemporal and plain loads, the tick and the close,
    and nothing else of theirs."""
    blob = open(_lib.LIB_PATH, "rb").read()
    got = sorted(set(m.decode() for m in re.findall(rb"_ZN3cts\d+ms_(?:verify_status_ordinal|conn_)[A-Za-z0-9_]*\.kd",
                                                     blob)))
    want = sorted(
        ["_ZN3cts24ms_verify_status_ordinalILb%dEEEvPKhmNS_8MsSourceEjPvPmjNS_10MsOrdinalsE.kd" % nt for nt in (0, 1)] +
        ["_ZN3cts18ms_conn_accumulateILb%dEEEvPK12cts_buf_descPK19cts_datagram_statusjjPKjP17cts_ms_conn_statePmmjSB_j.kd"
         % nt for nt in (0, 1)] +
        ["_ZN3cts14ms_conn_renderEPKjjP17cts_ms_conn_statePmjS4_Pj.kd",
         "_ZN3cts13ms_conn_closeEPKjjPjP17cts_ms_conn_statePmjP18cts_ms_conn_resultS5_.kd"])
    assert got == want


def test_integration_media_stream_connections_fragment_compiles():
    """INTEGRATION.md's per-batch sequence for MediaStream connections compiles against the header, receive pass
    before accounting pass before tick before close."""
    text = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    assert "## MediaStream connections on the device-resident path" in text
    found = [c for lang, c in re.findall(r"```(\w*)\n(.*?)```", text, re.S)
             if lang == "cpp" and c.startswith("// device-resident MediaStream receive, per batch k")]
    assert len(found) == 1
    order = [found[0].index(s) for s in ("cts_media_stream_verify_status_at(", "cts_media_stream_conns_accumulate(",
                                         "cts_media_stream_conns_render(", "cts_media_stream_conns_close(",
                                         "cts_counters_read_udp(")]
    assert order == sorted(order)
    params = ("cts_engine* e, const void* arena, uint64_t arena_bytes, const cts_buf_desc* descs_k, uint32_t n_k, "
              "uint32_t& ordinal, cts_datagram_status* status_k, void* ctr, uint32_t* conn_first_fail, "
              "uint32_t n_conns, cts_ms_conn_state* conns, uint64_t* frame_bytes, uint64_t frame_elems, void* udp, "
              "const uint32_t* due, uint32_t n_due, uint32_t* render_codes, const uint32_t* closing, "
              "uint32_t n_closing, cts_ms_conn_result* ms_results, void* closes, void* stream")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "f.cpp")
        with open(src, "w", encoding="utf-8") as f:
            f.write('#include "cts_media_stream_conns.h"\nvoid snippet(' + params + ")\n{\n" + found[0] + "\n}\n")
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]


# ---- world 2 over gloo: a UDP block folds and all-reduces like a counter block ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_udp(rank):
    name = ("mixed", "bulk_interleaved")[rank]
    return P.run_model(P.plan(name), P.plan_statuses(name)).udp


def _rank_main(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    try:
        D.init("gloo")
        sums = _rank_udp(rank)
        # a device-shaped block: 64 shards x 8 u64, this rank's UDP counters spread over two shards
        block = torch.zeros(64 * 8, dtype=torch.int64)
        for k, f in enumerate(D.UDP_FIELDS):
            block[8 * 5 + k] = sums[f] // 3
            block[8 * 62 + k] = sums[f] - sums[f] // 3
        c = D.fold_counters(block, D.UDP_FIELDS)
        assert D.counters_dict(c, D.UDP_FIELDS) == sums
        D.allreduce_counters(c)
        q.put((rank, "ok", D.counters_dict(c, D.UDP_FIELDS), sums))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        q.put((rank, "error", repr(e), None))


def test_world2_udp_block_allreduce():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = {}
    for _ in range(world):
        r = q.get(timeout=240)
        out[r[0]] = r
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in range(world):
        assert out[r][1] == "ok", out[r][2]
    total = {f: sum(out[r][3][f] for r in range(world)) for f in D.UDP_FIELDS}
    assert out[0][2] == out[1][2] == total
    exp = {f: sum(_rank_udp(r)[f] for r in range(world)) for f in D.UDP_FIELDS}
    assert total == exp and all(total[f] > 0 for f in D.UDP_FIELDS)
