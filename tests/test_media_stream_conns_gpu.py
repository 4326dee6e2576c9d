"""GPU: MediaStream connections on the device-resident path (include/cts_media_stream_conns.h) against the model
workload.media_stream_connection_view, whose kind and pass inputs come from the oracle verifier (the checker reads the
arena bytes). Device entries, rings, slots, results, the UDP block and the close block are compared field by field;
every comparison is exact. The model itself is checked against oracle.media_stream.ClientModel and the C client in
tests/test_media_stream_conns_cpu.py; the C++ sample of the same calls runs in tests/test_cpp_ms_connections.py.
"""
import numpy as np
import pytest
import torch

import ms_conn_plans as P
from ctstraffic_amd import _lib
from ctstraffic_amd import media_stream as M
from ctstraffic_amd import status as S
from ctstraffic_amd import workload as W
from ctstraffic_amd.engine import descs_to_device
from ctstraffic_amd.types import (CONN_RESULT_DTYPE, DESC_DTYPE, DGRAM_STATUS_DTYPE, MS_CONN_RESULT_DTYPE,
                                  MS_CONN_STATE_DTYPE, UDP_FIELDS)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EMPTY = W.EMPTY_SLOT


def _status_buf(n):
    return torch.zeros(max(1, n) * DGRAM_STATUS_DTYPE.itemsize, dtype=torch.uint8, device=DEV)


def _status_host(buf, n):
    return buf[: n * DGRAM_STATUS_DTYPE.itemsize].cpu().numpy().view(DGRAM_STATUS_DTYPE)


def _same_status(got, want):
    for f in ("completed_bytes", "kind", "pass"):
        assert np.array_equal(got[f], want[f]), f
    data = want["kind"] == W.DGRAM_DATA
    assert np.array_equal(got["sequence_number"][data], want["sequence_number"][data])


def _same_state(table, view, where):
    torch.cuda.synchronize()
    entries, ring, slots = table.read()
    for f in MS_CONN_STATE_DTYPE.names:
        assert np.array_equal(entries[f], view.entries[f]), (where, f)
    assert np.array_equal(ring, view.ring), where
    assert np.array_equal(slots, view.slots), where
    assert table.read_udp() == view.udp, where


def _ids(ids):
    return torch.tensor(list(ids), dtype=torch.int32, device=DEV)


def _run_batch(table, view, b, st, ctr=None):
    """One batch on the device and in the model: receive pass, accounting pass."""
    n = len(b.descs)
    arena, descs, sbuf = torch.from_numpy(b.arena).to(DEV), descs_to_device(b.descs, DEV), _status_buf(n)
    table.verify(arena, descs, b.base_index, status=sbuf, counters=ctr)
    table.accumulate(len(b.arena), descs, sbuf, b.base_index)
    torch.cuda.synchronize()
    _same_status(_status_host(sbuf, n), st)
    conn = b.descs["conn_index"]
    view.receive(conn, st["kind"], st["pass"], b.base_index)
    view.accumulate(conn, st, b.base_index)


def _tick(table, view, ids):
    codes = torch.full((len(ids),), 77, dtype=torch.int32, device=DEV)
    table.render(_ids(ids), codes)
    torch.cuda.synchronize()
    assert np.array_equal(codes.cpu().numpy().view(np.uint32), view.render(ids))


def _close(engine, table, view, ids, block):
    res = table.new_results(len(ids))
    table.close(_ids(ids), block, results=res)
    torch.cuda.synchronize()
    got, want = res.cpu().numpy().view(MS_CONN_RESULT_DTYPE), view.close(ids)
    for f in MS_CONN_RESULT_DTYPE.names:
        assert np.array_equal(got[f], want[f]), f
    return got


# ---- case 1: mixed outcomes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mixed_interleaved"])
def test_mixed_outcomes_three_batches(engine, name):
    """37 connections, about 6 000 datagrams, windows of 2, 8 and 600 frames, three batches with a tick after each,
    then the close of every connection and of one id without a slot: every outcome and every class of datagram
    (tests/test_media_stream_conns_cpu.py asserts the plan holds them)."""
    p, statuses = P.plan(name), P.plan_statuses(name)
    table, view = M.ConnectionTable(engine, p.settings), P.fresh_view(p)
    assert table.frame_elems == len(view.ring)
    for f in MS_CONN_STATE_DTYPE.names:
        assert np.array_equal(table.fresh[f], view.entries[f]), f
    ctr, ctr_today = engine.new_counters(), engine.new_counters()
    ids = list(range(p.n_conns))
    for k, (b, st) in enumerate(zip(p.batches, statuses)):
        _run_batch(table, view, b, st, ctr)
        _same_state(table, view, ("batch", k))
        for _ in range(b.ticks):
            _tick(table, view, ids)
        _same_state(table, view, ("tick", k))
        # the verify-counter block is fed as cts_media_stream_verify_status feeds it
        M.verify_status(engine, torch.from_numpy(b.arena).to(DEV), descs_to_device(b.descs, DEV), counters=ctr_today)
    torch.cuda.synchronize()
    assert engine.read_counters_ex(ctr) == engine.read_counters_ex(ctr_today)
    assert engine.read_counters_ex(ctr)["connections_failed"] == 0 and engine.read_counters(ctr)["buffers_failed"] > 0
    block = engine.new_counters()
    res = _close(engine, table, view, ids + [p.n_conns + 5], block)
    _same_state(table, view, "close")
    assert engine.read_counters_close(block) == view.close_block
    assert view.close_block["connections_closed"] == p.n_conns and min(
        view.close_block[f] for f in ("successful", "data_errors", "not_all_data")) > 0
    assert res["flags"][-1] == 1 and (view.slots == EMPTY).all() and not view.ring.any()


# ---- case 2: orderings and odd sizes -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 257, 1100])
@pytest.mark.parametrize("name", ["mixed", "mixed_interleaved", "single"])
def test_orderings_and_odd_sizes(engine, name, n):
    """Batches cut to n datagrams (1, under a wave, over a workgroup's 256, and 1100: no multiple of 64, 256 or 1024),
    connection-major, fully interleaved and one connection only (its run spans waves and workgroups)."""
    p, statuses = P.plan(name, n), P.plan_statuses(name, n)
    assert all(len(b.descs) == n for b in p.batches)
    table, view = M.ConnectionTable(engine, p.settings), P.fresh_view(p)
    for k, (b, st) in enumerate(zip(p.batches, statuses)):
        _run_batch(table, view, b, st)
        _tick(table, view, list(range(p.n_conns)))
        _same_state(table, view, (name, n, k))
    assert view.udp["datagrams"] > 0


def test_accumulate_long_spans(engine):
    """Over 2048 x 256 datagrams a wave's span is longer than one tile of 64: runs carried from tile to tile, tiles
    that are nothing but the open run, runs joined across a workgroup's waves. 594 288 synthetic statuses of four
    connections (one long run, an interleaved stretch, blocks of 777), every datagram clean DATA inside a window of
    600 frames, connection 2 stopped by a preset slot in the blocks; the expectation is computed with numpy masks.
    On 256 compute units the span is two tiles, so a parked tile is always a span's last one; spans of five tiles, with
    parked sums joined inside the loop, are in tests/test_accounting_seams_gpu.py."""
    n, base = 2048 * 256 + 70000, 1000
    i = np.arange(n)
    conn = np.where(i < 300000, 0, np.where(i < 400000, 1 + i % 3, (i // 777) % 4)).astype(np.uint32)
    st = np.zeros(n, dtype=DGRAM_STATUS_DTYPE)
    st["kind"], st["pass"] = W.DGRAM_DATA, 1
    st["sequence_number"] = 1 + i % 600
    st["completed_bytes"] = 100 + i % 1373
    at = int(np.nonzero((conn == 2) & (i > 450000))[0][5])
    st["pass"][at] = 0
    descs = np.zeros(n, dtype=DESC_DTYPE)
    descs["conn_index"], descs["length"] = conn, st["completed_bytes"]
    table = M.ConnectionTable(engine, [(3000, 300, 1000)] * 4)
    table.slots[2] = base + at
    table.accumulate(1 << 40, descs_to_device(descs, DEV),
                     torch.from_numpy(st.view(np.uint8).copy()).to(DEV), base)
    torch.cuda.synchronize()
    entries, ring, slots = table.read()
    g, first = base + i, np.where(conn == 2, base + at, EMPTY).astype(np.int64)
    applied, after = g < first, g > first
    comp = st["completed_bytes"].astype(np.int64)
    want_ring = np.bincount((conn.astype(np.int64) * 600 + i % 600)[applied], weights=comp[applied], minlength=2400)
    assert np.array_equal(ring, want_ring.astype(np.uint64))
    for c in range(4):
        mine = conn == c
        assert entries["bits_received"][c] == 8 * int(comp[mine & applied].sum())
        assert entries["datagrams"][c] == int((mine & ~after).sum())
        assert entries["datagrams_after_end"][c] == int((mine & after).sum()) and entries["error_frames"][c] == 0
        assert entries["received_any"][c] == 1 and entries["has_failure"][c] == (c == 2)
        assert entries["last_error"][c] == (P.DATA_MISMATCH if c == 2 else P.RUNNING)
    assert entries["datagrams_after_end"][2] > 1000 and slots.tolist() == [EMPTY, EMPTY, base + at, EMPTY]
    assert table.read_udp() == {"bits_received": 8 * int(comp[applied].sum()), "successful_frames": 0,
                                "dropped_frames": 0, "duplicate_frames": 0, "error_frames": 0,
                                "datagrams": int((~after).sum())}


# ---- case 3: launch order ------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
def test_receive_passes_in_any_launch_order(engine, reverse):
    """The receive passes of three batches queued on one stream, in order and in reverse, the accounting passes after
    all of them: the slots are the global first-exception ordinals either way, and the books those of the model (the
    ticks left out: the window does not move)."""
    p, statuses = P.plan("mixed"), P.plan_statuses("mixed")
    table, view = M.ConnectionTable(engine, p.settings), P.fresh_view(p)
    dev = [(torch.from_numpy(b.arena).to(DEV), descs_to_device(b.descs, DEV), _status_buf(len(b.descs)))
           for b in p.batches]
    order = list(range(len(p.batches)))
    for k in (order[::-1] if reverse else order):
        table.verify(dev[k][0], dev[k][1], p.batches[k].base_index, status=dev[k][2])
    for b, st in zip(p.batches, statuses):
        view.receive(b.descs["conn_index"], st["kind"], st["pass"], b.base_index)
    torch.cuda.synchronize()
    assert np.array_equal(table.read()[2], view.slots) and (view.slots != EMPTY).sum() >= 5
    for k in order:
        table.accumulate(len(p.batches[k].arena), dev[k][1], dev[k][2], p.batches[k].base_index)
        view.accumulate(p.batches[k].descs["conn_index"], statuses[k], p.batches[k].base_index)
    _same_state(table, view, reverse)


# ---- case 4: argument edges ----------------------------------------------------------------------------------
def test_argument_edges(engine):
    """A connection without a slot counts in the node block only; a bad descriptor fails its stream; a datagram whose
    ring element would fall outside frame_elems is never written (an error frame); the ordinal limit is CTS_E_INVALID
    with nothing launched; n == 0 is CTS_OK."""
    p = W.media_stream_connections(n_conns=4, batches=1, roles=["bulk", "bad_desc", "bulk", "bulk"], bulk_frames=3)
    b = p.batches[0]
    st = P.batch_status(b)
    # two slots only: connections 2 and 3 have none
    table = M.ConnectionTable(engine, p.settings[:2])
    view = W.media_stream_connection_view(table.fresh, table.frame_elems)
    # connection 0's ring is cut short: frame_elems = 2, so frames 3.. of its window of 600 have no element
    table.frame_elems = 2
    view.ring = view.ring[:2]
    _run_batch(table, view, b, st)
    torch.cuda.synchronize()
    entries, ring, slots = table.read()
    assert np.array_equal(entries, view.entries) and np.array_equal(ring, view.ring)
    assert entries["error_frames"][0] > 0 and entries["last_error"][1] == P.NOT_ALL_DATA
    assert np.array_equal(slots, view.slots) and slots[0] == EMPTY and slots[1] != EMPTY
    assert not table.frame_bytes.cpu().numpy()[2:].any()
    assert table.read_udp() == view.udp and view.udp["datagrams"] > int(entries["datagrams"].sum())
    # the ordinal limit, and n == 0
    L, h = engine._L, engine._h
    arena, descs, sbuf = torch.from_numpy(b.arena).to(DEV), descs_to_device(b.descs, DEV), _status_buf(len(b.descs))
    before = table.read()
    ptr = lambda t: t.data_ptr()
    assert L.cts_media_stream_verify_status_at(h, ptr(arena), len(b.arena), ptr(descs), 2, 0xFFFFFFFE, ptr(sbuf), None,
                                               ptr(table.slots), 2, None) == _lib.CTS_E_INVALID
    assert L.cts_media_stream_conns_accumulate(h, len(b.arena), ptr(descs), ptr(sbuf), 2, 0xFFFFFFFE, ptr(table.slots),
                                               ptr(table.conns), ptr(table.frame_bytes), 2, 2, ptr(table.udp),
                                               None) == _lib.CTS_E_INVALID
    assert L.cts_media_stream_verify_status_at(h, ptr(arena), len(b.arena), ptr(descs), 0, 0, ptr(sbuf), None,
                                               ptr(table.slots), 2, None) == _lib.CTS_OK
    assert L.cts_media_stream_conns_accumulate(h, len(b.arena), ptr(descs), ptr(sbuf), 0, 0, ptr(table.slots),
                                               ptr(table.conns), ptr(table.frame_bytes), 2, 2, ptr(table.udp),
                                               None) == _lib.CTS_OK
    assert L.cts_media_stream_conns_render(h, ptr(table.slots), 0, ptr(table.conns), ptr(table.frame_bytes), 2,
                                           ptr(table.udp), None, None) == _lib.CTS_OK
    assert L.cts_media_stream_conns_close(h, ptr(table.slots), 0, ptr(table.slots), ptr(table.conns),
                                          ptr(table.frame_bytes), 2, None, ptr(table.udp), None) == _lib.CTS_OK
    torch.cuda.synchronize()
    after = table.read()
    assert all(np.array_equal(x, y) for x, y in zip(before, after)) and table.read_udp() == view.udp
    # the last ordinal the limit allows: 0xFFFFFFFE for the second of two datagrams
    two = W.media_stream_connections(n_conns=1, batches=1, roles=["bulk"], bulk_frames=1, limit=2)
    bt = two.batches[0]
    bt.arena[int(bt.descs["byte_offset"][1]) + 100] ^= 0x40  # the second datagram fails its stream
    t2 = M.ConnectionTable(engine, two.settings)
    v2 = W.media_stream_connection_view(t2.fresh, t2.frame_elems)
    bt.base_index = 0xFFFFFFFD
    _run_batch(t2, v2, bt, P.batch_status(bt))
    _same_state(t2, v2, "top of the ordinal range")
    assert v2.slots[0] == 0xFFFFFFFE and v2.entries["has_failure"][0] == 1


# ---- case 5: reuse -------------------------------------------------------------------------------------------
def test_two_generations_through_the_same_slots(engine):
    """Close, late datagrams, fresh entries, reuse: the late datagrams count only as after the end; a
    cts_conn_slots_rebase between the second generation's batches keeps failed connections failed."""
    p, statuses = P.plan("mixed"), P.plan_statuses("mixed")
    table, view = M.ConnectionTable(engine, p.settings), P.fresh_view(p)
    ids, block = list(range(p.n_conns)), engine.new_counters()
    for b, st in zip(p.batches[:2], statuses[:2]):
        _run_batch(table, view, b, st)
        _tick(table, view, ids)
    _close(engine, table, view, ids, block)
    _same_state(table, view, "first close")
    # the third batch arrives after the close, before the fresh entries
    before = view.entries.copy()
    _run_batch(table, view, p.batches[2], statuses[2])
    _same_state(table, view, "late")
    late = np.bincount(p.batches[2].descs["conn_index"], minlength=p.n_conns)
    assert np.array_equal(view.entries["datagrams_after_end"], before["datagrams_after_end"] + late)
    for f in ("datagrams", "bits_received", "error_frames", "last_error"):
        assert np.array_equal(view.entries[f], before[f]), f
    assert not view.ring.any()
    # the receive pass of the late batch lowered slots of closed connections: the caller empties them with the entries
    table.reinit(ids)
    table.slots.fill_(-1)
    view.reinit(ids, table.fresh)
    view.slots[:] = EMPTY
    base = p.batches[2].base_index + len(p.batches[2].descs)
    delta = 0
    for k, (b, st) in enumerate(zip(p.batches, statuses)):
        shifted = W.MsConnBatch(b.descs, b.arena, base + b.base_index - delta, b.ticks)
        _run_batch(table, view, shifted, st)
        _tick(table, view, ids)
        _same_state(table, view, ("second generation", k))
        if k == 0:
            delta = base + p.batches[1].base_index - 1   # below every ordinal still to come
            engine.slots_rebase(table.slots, delta)
            view.rebase(delta)
            assert (view.slots[view.slots != EMPTY] == 0).all() and (view.slots != EMPTY).any()
    first = P.run_model(p, statuses)
    for f in MS_CONN_STATE_DTYPE.names:
        assert np.array_equal(view.entries[f], first.entries[f]), f   # the second generation ends as a first one does
    _close(engine, table, view, ids, block)
    assert engine.read_counters_close(block) == view.close_block
    assert view.close_block["connections_closed"] == 2 * p.n_conns


# ---- case 6: the block reads ---------------------------------------------------------------------------------
def _two_engines(q):
    try:
        from ctstraffic_amd import Engine
        from ctstraffic_amd.engine import (counters_allreduce_release, counters_allreduce_udp,
                                           counters_read_multi_udp)

        torch.cuda.set_device(0)
        out = {}
        with Engine(0) as e0, Engine(0) as e1:
            blocks, exps = [], []
            for eng, name in ((e0, "bulk_interleaved"), (e1, "single")):
                p, statuses = P.plan(name), P.plan_statuses(name)
                table, view = M.ConnectionTable(eng, p.settings), P.fresh_view(p)
                for b, st in zip(p.batches, statuses):
                    _run_batch(table, view, b, st)
                    _tick(table, view, list(range(p.n_conns)))
                blocks.append(table.udp)
                exps.append(view.udp)
            both = {f: exps[0][f] + exps[1][f] for f in UDP_FIELDS}
            out["read"] = (e0.read_counters_udp(blocks[0]), exps[0])
            out["multi"] = (counters_read_multi_udp([e0, e1], blocks), both)
            try:
                out["allreduce"] = (counters_allreduce_udp([e0, e1], blocks), both)
                out["allreduce_one"] = (counters_allreduce_udp([e1], blocks[1:]), exps[1])
                counters_allreduce_release()
            except _lib.CtsError as e:
                if e.status != _lib.CTS_E_UNAVAILABLE:
                    raise
                out["allreduce"] = out["allreduce_one"] = "unavailable"
        q.put(out)
    except Exception as e:  # pragma: no cover
        import traceback

        q.put({"error": repr(e) + "\n" + traceback.format_exc()})


def test_udp_blocks_through_the_three_folds():
    """read_counters_udp, counters_read_multi_udp and counters_allreduce_udp (the RCCL all-reduce of count 6) over UDP
    blocks agree with the model, with one engine and with two engines on one device. Where RCCL is not installed the
    all-reduce answers CTS_E_UNAVAILABLE and the two host folds stand alone."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    proc = ctx.Process(target=_two_engines, args=(q,))
    proc.start()
    r = q.get(timeout=240)
    proc.join(60)
    assert "error" not in r, r.get("error")
    assert proc.exitcode == 0
    for key in ("read", "multi"):
        got, exp = r[key]
        assert got == exp and exp["datagrams"] > 0 and exp["bits_received"] > 0, key
    for key in ("allreduce", "allreduce_one"):
        if r[key] != "unavailable":
            got, exp = r[key]
            assert got == exp, key


def test_status_line_from_the_block_and_a_close_block_shared_with_tcp(engine):
    """The UDP status line and exit summary print from two reads of the UDP block as from the host's
    UdpStatusDetails; one close block takes MediaStream closes and TCP closes (cts_conns_close) alike."""
    p, statuses = P.plan("mixed"), P.plan_statuses("mixed")
    table, view = M.ConnectionTable(engine, p.settings), P.fresh_view(p)
    ids, reads = list(range(p.n_conns)), [dict.fromkeys(UDP_FIELDS, 0)]
    for b, st in zip(p.batches, statuses):
        _run_batch(table, view, b, st)
        _tick(table, view, ids)
        reads.append(table.read_udp())
    assert reads[-1] == view.udp
    frames = ("bits_received", "successful_frames", "dropped_frames", "duplicate_frames", "error_frames")
    for k in (1, 2, 3):
        slice_ = {f: reads[k][f] - reads[k - 1][f] for f in frames}
        line = S.udp_line(S.CSV, current_time_ms=1000 * k, start_time_ms=1000 * (k - 1), end_time_ms=1000 * k,
                          active_streams=p.n_conns, **slice_)
        cells = line.strip().split(",")
        assert cells[1] == str(slice_["bits_received"]) and cells[2] == str(p.n_conns)  # one second: bits per second
        assert [int(c) for c in cells[3:7]] == [slice_[f] for f in frames[1:]]
    assert sum(reads[3][f] for f in frames[1:]) > 0
    block = engine.new_counters()
    _close(engine, table, view, ids, block)
    ms = dict(view.close_block)
    # a TCP close into the same block: four connections, one of them with a failing ordinal
    slots = torch.tensor([-1, 7, -1, -1], dtype=torch.int32, device=DEV)
    state = engine.new_conn_state(4)
    state.view(4, 4)[:, 0] = torch.tensor([100, 200, 300, 400], device=DEV)
    res = engine.new_conn_results(4)
    engine.conns_close(_ids(range(4)), torch.tensor([100, 200, 300, 500], dtype=torch.int64, device=DEV), slots,
                       state, block, results=res)
    torch.cuda.synchronize()
    got = engine.read_counters_close(block)
    assert got == {"connections_closed": ms["connections_closed"] + 4, "successful": ms["successful"] + 2,
                   "data_errors": ms["data_errors"] + 1, "not_all_data": ms["not_all_data"] + 1, "too_much_data": 0,
                   "bytes_recv": ms["bytes_recv"] + 1000}
    assert res.cpu().numpy().view(CONN_RESULT_DTYPE)["status"].tolist() == [0, P.DATA_MISMATCH, 0, P.NOT_ALL_DATA]
    text = S.udp_summary(got["successful"], 0, got["data_errors"] + got["not_all_data"], *(reads[3][f] for f in frames))
    assert str(reads[3]["bits_received"] // 8) in text


# ---- case 7: equivalence with today's path -------------------------------------------------------------------
def test_one_clean_connection_equals_verify_frames_and_the_host_client(engine):
    """One connection without exceptions: entry and ring after batch plus tick equal cts_media_stream_verify_frames
    plus complete_frames plus render on the same datagrams, batch after batch."""
    p = W.media_stream_connections(n_conns=1, batches=3, roles=["bulk"], bulk_frames=30)
    table = M.ConnectionTable(engine, p.settings)
    client = M.MediaStreamClient(*p.settings[0], datagram_max_size=p.max_datagram)
    carried = {}  # sequence number -> bytes earlier batches left in frames that are still in the window
    for b in p.batches:
        n = len(b.descs)
        arena, descs, sbuf = torch.from_numpy(b.arena).to(DEV), descs_to_device(b.descs, DEV), _status_buf(n)
        table.verify(arena, descs, b.base_index, status=sbuf)
        table.accumulate(len(b.arena), descs, sbuf, b.base_index)
        w = client.window()
        sums = M.FrameSums(w.frames, device=DEV)
        M.verify_frames(engine, arena, descs, w, sums)
        torch.cuda.synchronize()
        totals, fb = sums.read()
        assert totals.exceptions == 0 and client.complete_frames(w, totals, fb, n) == 0
        entries, ring, slots = table.read()
        # today's sums hold this batch alone, indexed from the head; the device ring holds the window, indexed by
        # (sequence number - 1) mod frames
        seqs = w.head_sequence_number + np.arange(w.frames)
        held = np.array([carried.get(int(q), 0) for q in seqs], dtype=np.uint64) + fb
        assert np.array_equal(ring[(seqs - 1) % w.frames], held) and held.any()
        carried = {int(q): int(v) for q, v in zip(seqs[1:], held[1:])}  # the tick renders and clears the head frame
        codes = torch.zeros(1, dtype=torch.int32, device=DEV)
        table.render(_ids([0]), codes)
        torch.cuda.synchronize()
        assert int(codes[0]) == client.render()
        entries = table.read()[0]
        s = client.stats()
        for f in ("bits_received", "successful_frames", "dropped_frames", "duplicate_frames", "error_frames",
                  "datagrams", "last_error", "finished", "head_sequence_number"):
            assert int(entries[f][0]) == s[f], f
        assert slots[0] == EMPTY
    assert s["successful_frames"] + s["duplicate_frames"] == 3 and s["bits_received"] > 0

