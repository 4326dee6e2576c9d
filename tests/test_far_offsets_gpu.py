"""GPU: rings, descriptors and ticks across the 4 GiB byte offset, against the oracle and the models over the plans of
tests/far_offsets.py (tests/test_far_offsets_cpu.py shows what each plan tells apart).

Every test allocates one arena of 4.0 to 4.1 GiB (one of them 16 GiB + 64 MiB), filled with the sentinel 0xA5 on the
device; only the live spans come from the host, and only the plan's windows go back. Every comparison is exact: all n
rows of a ring's outputs are compared on the device against the oracle's rows for the live slots and its row for a
zero-length slot everywhere else; the counters, first-failure slots and frame sums are the oracle's; every window of
a filled arena equals the oracle's bytes and is the sentinel around them and at the aliases mod 2^32. One test holds
a dense arena instead: an exchange tick that moves 5.6 GiB, so that its byte sums need more than 32 bits.
"""
import numpy as np
import pytest
import torch

import far_offsets as F
import oracle
from ctstraffic_amd import _lib
from ctstraffic_amd import media_stream as M
from ctstraffic_amd import tcp_exchange as X
from ctstraffic_amd import tcp_senders as T
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import (CONN_RESULT_DTYPE, CONN_STATE_DTYPE, DESC_DTYPE, DGRAM_HEADER_DTYPE,
                                  DGRAM_RECORD_DTYPE, DGRAM_STATUS_DTYPE, MS_CONN_RESULT_DTYPE, MS_SERVER_STATE_DTYPE,
                                  RESULT_DTYPE, TCP_EXCHANGE_DTYPE, TCP_SENDER_DTYPE, TCP_SENDER_PACE_DTYPE)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEAM = F.SEAM
BASE = 1 << 20  # the stream ordinal of buffer 0 in the _at forms


def _dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def _ids(ids):
    return torch.from_numpy(np.asarray(list(ids), dtype=np.uint32).view(np.int32).copy()).to(DEV)


def _arena(nbytes: int):
    """nbytes of sentinel on the device (a failed allocation fails the test)."""
    return torch.full(((nbytes + 15) // 16 * 16 + 16,), F.BACKGROUND, dtype=torch.uint8, device=DEV)[:nbytes]


def _upload(arena, ring: F.SparseRing, ranges=None) -> None:
    for a, b in ring.touched() if ranges is None else ranges:
        b = min(b, arena.numel())
        arena[a:b] = torch.from_numpy(ring.read(a, b - a)).to(DEV)


def _windows_equal(arena, ring: F.SparseRing, windows, where="") -> None:
    for a, b in windows:
        got, want = arena[a:b].cpu().numpy(), ring.read(a, b - a)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (where, (a, b), (a + bad[:8]).tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def _rows_equal(got, live, rows: np.ndarray, dead, n: int, where) -> None:
    """All n rows of a device output: `rows` at the slots `live`, the row `dead` everywhere else; compared on the
    device, the differing rows (if any) brought back for the message."""
    size = rows.dtype.itemsize
    want = _dev(np.array([dead], dtype=rows.dtype)).repeat(n).view(n, size)
    want[torch.from_numpy(np.asarray(live, dtype=np.int64)).to(DEV)] = _dev(rows).view(len(rows), size)
    got = got[: n * size].view(n, size)
    if not torch.equal(got, want):
        at = (got != want).any(dim=1).nonzero().flatten()[:8]
        raise AssertionError((where, at.tolist(), got[at].cpu().numpy().view(rows.dtype).tolist(),
                              want[at].cpu().numpy().view(rows.dtype).tolist()))


def _set_nt(engine, nt):
    engine.set_attr(_lib.ATTR_NT_LOADS, nt)


def _lengths(p: F.RingPlan):
    lens = torch.zeros(p.n, dtype=torch.int32, device=DEV)
    lens[torch.from_numpy(p.live).to(DEV)] = torch.from_numpy(p.lens.view(np.int32).copy()).to(DEV)
    return lens


def _slots_at(cff: np.ndarray, base: int) -> np.ndarray:
    return np.where(cff == F.EMPTY, F.EMPTY, cff.astype(np.int64) + base).astype(np.uint32)


# ---- 1. cts_verify_strided and cts_verify_strided_at ---------------------------------------------------------------
@pytest.mark.parametrize("skip,expected", [(0, 0), (3, 65535)])
@pytest.mark.parametrize("stride", F.VERIFY_STRIDES)
def test_verify_strided_across_the_seam(engine, stride, skip, expected):
    p = F.RingPlan(stride, "tcp", skip=skip, expected=expected)
    out = p.outcome()
    arena, lens = _arena(p.arena_bytes), _lengths(p)
    _upload(arena, p.ring)
    try:
        for nt in (1, 0):
            _set_nt(engine, nt)
            for base in (0, BASE):
                res, ctr = engine.new_results(p.n), engine.new_counters()
                cff = torch.full((p.n_conns,), -1, dtype=torch.int32, device=DEV)
                engine.verify_strided(arena, stride, lens, skip_head=skip, expected_offset=expected, conn_index=p.conn,
                                      results=res, counters=ctr, conn_first_fail=cff, base_index=base)
                torch.cuda.synchronize()
                _rows_equal(res, p.live, out["results"], out["dead_result"], p.n, (nt, base))
                assert engine.read_counters(ctr) == out["counters"], (nt, base)
                assert np.array_equal(cff.cpu().numpy().view(np.uint32), _slots_at(out["cff"], base)), (nt, base)
                del res
    finally:
        _set_nt(engine, 1)
    del arena, lens
    torch.cuda.empty_cache()


# ---- 2. the MediaStream receive over a ring: records, statuses, frames ----------------------------------------------
@pytest.mark.parametrize("stride", F.VERIFY_STRIDES)
def test_media_stream_receive_strided_across_the_seam(engine, stride):
    p = F.RingPlan(stride, "ms")
    out = p.outcome()
    arena, lens = _arena(p.arena_bytes), _lengths(p)
    _upload(arena, p.ring)
    try:
        for nt in (1, 0):
            _set_nt(engine, nt)
            recs = torch.zeros(p.n * DGRAM_RECORD_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
            res, ctr = engine.new_results(p.n), engine.new_counters()
            M.verify_strided(engine, arena, stride, lens, records=recs, results=res, counters=ctr)
            torch.cuda.synchronize()
            _rows_equal(recs, p.live, out["records"], out["dead_record"], p.n, (nt, "records"))
            _rows_equal(res, p.live, out["results"], out["dead_result"], p.n, (nt, "results"))
            assert engine.read_counters(ctr) == out["counters"], nt
            del recs, res
            st, ctr = torch.zeros(p.n * DGRAM_STATUS_DTYPE.itemsize, dtype=torch.uint8, device=DEV), engine.new_counters()
            M.verify_strided_status(engine, arena, stride, lens, status=st, counters=ctr)
            torch.cuda.synchronize()
            _rows_equal(st, p.live, out["status"], out["dead_status"], p.n, (nt, "status"))
            assert engine.read_counters(ctr) == out["counters"], nt
            del st
            for finished in (False, True):
                w = p.window(finished)
                want, want_fb = p.frames(out, finished)
                sums, ctr = M.FrameSums(w["frames"], device=DEV), engine.new_counters()
                M.verify_strided_frames(engine, arena, stride, lens,
                                        M.FrameWindow(w["head"], w["final"], w["frames"], w["finished"]), sums, ctr)
                torch.cuda.synchronize()
                t, fb = sums.read()
                assert t.as_dict() == want, (nt, finished)
                assert np.array_equal(fb[: w["frames"]], want_fb), (nt, finished)
                assert engine.read_counters(ctr) == out["counters"], (nt, finished)
    finally:
        _set_nt(engine, 1)
    del arena, lens
    torch.cuda.empty_cache()


# ---- 3. cts_media_stream_fill_strided -------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", F.RING_FILL_STRIDES)
def test_media_stream_fill_strided_across_the_seam(engine, stride):
    """Both store loops (strides below 1024 and from 1024 on), the in-arena bound of the last slot, and the run of
    full slots around the seam; every window against the oracle's datagrams, the rest of it the sentinel."""
    p = F.RingPlan(stride, "fill")
    want, windows = p.outcome()["ring"], p.windows()
    arena, lens = _arena(p.arena_bytes), _lengths(p)
    hdrs = torch.zeros(p.n * DGRAM_HEADER_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    hdrs.view(p.n, DGRAM_HEADER_DTYPE.itemsize)[torch.from_numpy(p.live).to(DEV)] = _dev(p.headers()).view(
        len(p.live), DGRAM_HEADER_DTYPE.itemsize)
    blank = F.SparseRing(p.arena_bytes)
    default = engine.get_attr(_lib.ATTR_FILL_NT)
    try:
        for fill_nt in (0, 1):
            engine.set_attr(_lib.ATTR_FILL_NT, fill_nt)
            M.fill_strided(engine, arena, stride, lens, hdrs)
            torch.cuda.synchronize()
            _windows_equal(arena, want, windows, fill_nt)
            _upload(arena, blank, windows)  # back to the sentinel
    finally:
        engine.set_attr(_lib.ATTR_FILL_NT, default)
    del arena, lens, hdrs
    torch.cuda.empty_cache()


# ---- 4. descriptors at far offsets: the verifies ---------------------------------------------------------------------
def _verify_descs(engine, arena, p: F.DescPlan):
    out, n = p.outcome(), len(p.descs)
    d = _dev(p.descs)
    for nt in (1, 0):
        _set_nt(engine, nt)
        for hint in (0, 1472):  # a workgroup per buffer, four buffers per wave
            for base in (0, BASE):
                res, ctr = engine.new_results(n), engine.new_counters()
                cff = torch.full((p.n_conns,), -1, dtype=torch.int32, device=DEV)
                engine.verify(arena, d, max_length_hint=hint, results=res, counters=ctr, conn_first_fail=cff,
                              base_index=base)
                torch.cuda.synchronize()
                got = res.cpu().numpy().view(RESULT_DTYPE)
                for f in RESULT_DTYPE.names:
                    assert np.array_equal(got[f], out["results"][f]), (p.variant, nt, hint, base, f)
                assert engine.read_counters(ctr) == out["counters"], (p.variant, nt, hint, base)
                assert np.array_equal(cff.cpu().numpy().view(np.uint32), _slots_at(out["cff"], base)), (nt, hint, base)


def _receive_descs(engine, arena, p: F.DescPlan):
    out, n = p.outcome(), len(p.descs)
    d = _dev(p.descs)
    conn = p.descs["conn_index"]
    for nt in (1, 0):
        _set_nt(engine, nt)
        recs = torch.zeros(n * DGRAM_RECORD_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
        res, ctr = engine.new_results(n), engine.new_counters()
        M.verify(engine, arena, d, records=recs, results=res, counters=ctr)
        st, ctr2 = torch.zeros(n * DGRAM_STATUS_DTYPE.itemsize, dtype=torch.uint8, device=DEV), engine.new_counters()
        M.verify_status(engine, arena, d, status=st, counters=ctr2)
        table = M.ConnectionTable(engine, [(4000, 4, 100)] * p.n_conns)
        st_at, ctr3 = torch.zeros_like(st), engine.new_counters()
        table.verify(arena, d, BASE, status=st_at, counters=ctr3)
        w = dict(head=int(p.headers["sequence_number"][0]) + 1, final=1 << 41, frames=16, finished=0)
        sums = M.FrameSums(16, device=DEV)
        M.verify_frames(engine, arena, d, M.FrameWindow(w["head"], w["final"], w["frames"], 0), sums)
        torch.cuda.synchronize()
        for got, want in ((recs.cpu().numpy().view(DGRAM_RECORD_DTYPE), out["records"]),
                          (res.cpu().numpy().view(RESULT_DTYPE), out["results"]),
                          (st.cpu().numpy().view(DGRAM_STATUS_DTYPE), out["status"]),
                          (st_at.cpu().numpy().view(DGRAM_STATUS_DTYPE), out["status"])):
            for f in want.dtype.names:
                assert np.array_equal(got[f], want[f]), (p.variant, nt, want.dtype.names[0], f)
        for c in (ctr, ctr2, ctr3):
            assert engine.read_counters(c) == out["counters"], (p.variant, nt)
        view = W.media_stream_connection_view(W.media_stream_conn_entries([(4000, 4, 100)] * p.n_conns)[0], 8 * p.n_conns)
        view.receive(conn, out["status"]["kind"], out["status"]["pass"], BASE)
        assert np.array_equal(table.read()[2], view.slots), (p.variant, nt)
        want_t, want_fb = F.frame_sums(out["status"], np.arange(n), w)
        t, fb = sums.read()
        assert t.as_dict() == want_t and np.array_equal(fb[:16], want_fb), (p.variant, nt)


@pytest.mark.parametrize("kind", ["tcp", "ms"])
@pytest.mark.parametrize("variant", [v for v in F.DESC_VARIANTS if v != "big"])
def test_descriptor_verifies_across_the_seam(engine, variant, kind):
    p = F.DescPlan(variant, kind)
    arena = _arena(p.arena_bytes)
    _upload(arena, p.ring)
    try:
        (_verify_descs if kind == "tcp" else _receive_descs)(engine, arena, p)
    finally:
        _set_nt(engine, 1)
    del arena
    torch.cuda.empty_cache()


# ---- 5. descriptors at far offsets: cts_fill's three paths and cts_media_stream_fill ---------------------------------
def _fill_descs(engine, arena, p: F.DescPlan):
    want, windows = p.outcome(what="fill")["ring"], p.windows()
    blank = F.SparseRing(p.arena_bytes)
    d = _dev(p.descs)
    hdrs = _dev(p.headers)
    default = engine.get_attr(_lib.ATTR_FILL_NT)
    try:
        for fill_nt in (0, 1):
            engine.set_attr(_lib.ATTR_FILL_NT, fill_nt)
            for hint in (0, 1472, 65536) if p.kind == "tcp" else (None,):
                if p.kind == "tcp":
                    engine.fill(arena, d, max_length_hint=hint)
                else:
                    M.fill(engine, arena, d, hdrs)
                torch.cuda.synchronize()
                _windows_equal(arena, want, windows, (p.variant, fill_nt, hint))
                _upload(arena, blank, windows)
    finally:
        engine.set_attr(_lib.ATTR_FILL_NT, default)


@pytest.mark.parametrize("kind", ["tcp", "ms"])
@pytest.mark.parametrize("variant", [v for v in F.DESC_VARIANTS if v != "big"])
def test_descriptor_fills_across_the_seam(engine, variant, kind):
    p = F.DescPlan(variant, kind, corrupt=None)
    arena = _arena(p.arena_bytes)
    _fill_descs(engine, arena, p)
    del arena
    torch.cuda.empty_cache()


def test_descriptors_above_16_gib(engine):
    """One arena of 16 GiB + 64 MiB: a descriptor above 16 GiB beside one across 4 GiB, through both fills and the
    three verifies. The alias of the far one is four seams below it."""
    arena = _arena(F.DescPlan("big", corrupt=None).arena_bytes)
    try:
        for kind in ("tcp", "ms"):
            _fill_descs(engine, arena, F.DescPlan("big", kind, corrupt=None))
            p = F.DescPlan("big", kind)
            _upload(arena, p.ring)
            (_verify_descs if kind == "tcp" else _receive_descs)(engine, arena, p)
            _upload(arena, F.SparseRing(p.arena_bytes), p.ring.touched())
    finally:
        _set_nt(engine, 1)
    del arena
    torch.cuda.empty_cache()


# ---- 6. the servers' tick and the clients' receive half over its descriptors -----------------------------------------
def _dirty(p: F.TickPlan, arena, ring: F.SparseRing) -> None:
    """One bit flipped just above the seam and the clean bytes at the alias, in the model's ring and (unless None) in
    the arena."""
    _, g, at = p.seam_hit()
    d = p.ticks()[0]["descs"][g]
    off, length = int(d["byte_offset"]), int(d["length"])
    clean = p.outcome(n_ticks=1)["ring"].read(off, length)
    lo = max(off, SEAM)
    ring.write(lo - SEAM, clean[lo - off:])
    ring.write(at, clean[at - off:at - off + 1] ^ np.uint8(0x04))
    if arena is not None:
        _upload(arena, ring, [(lo - SEAM, off + length - SEAM), (at, at + 1)])


@pytest.mark.parametrize("stride", F.SERVER_STRIDES)
def test_server_ticks_across_the_seam(engine, stride):
    p = F.TickPlan("server", stride)
    windows, blank = p.windows(), F.SparseRing(p.arena_bytes)
    arena = _arena(p.arena_bytes)
    n_conns, ids = len(p.settings), _ids(p.ids)
    client_settings = [(f, 2, final) for f, _, final in p.settings]
    for dirty in (False, True):
        table = M.ServerTable(engine, p.settings, stride, p.capacity, ring_slots=1, fill=F.BACKGROUND)
        clients = M.ConnectionTable(engine, client_settings)
        view = W.media_stream_connection_view(*W.media_stream_conn_entries(client_settings))
        status = torch.zeros(p.capacity * DGRAM_STATUS_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
        base = 0
        for k, t in enumerate(p.ticks()):
            M.servers_send(engine, arena, stride, t["first_slot"], p.capacity, ids, table.servers, n_conns, F.QPC + k,
                           F.QPF, table.scratch, descs=table.descs, lengths=table.lengths, codes=table.codes,
                           tick=table.tick, udp_counters=table.udp)
            torch.cuda.synchronize()
            entries, codes, tick = table.read()
            for f in MS_SERVER_STATE_DTYPE.names:
                assert np.array_equal(entries[f], t["entries"][f]), (k, f)
            assert np.array_equal(codes[: len(p.ids)], t["codes"]), k
            assert {f: int(tick[f]) for f in W.MS_SERVER_TICK_FIELDS} == t["tick"] and int(tick["reserved"]) == 0, k
            descs, model = table.descs.cpu().numpy().view(DESC_DTYPE)[: p.capacity], p.outcome(n_ticks=k + 1)
            for f in DESC_DTYPE.names:
                assert np.array_equal(descs[f], model["descs"][k][f]), (k, f)
            assert np.array_equal(table.lengths.cpu().numpy().view(np.uint32)[: p.capacity], t["lengths"]), k
            assert table.read_udp() == t["udp"], k
            ring = model["ring"]
            if dirty and k > 0:
                _dirty(p, None, ring)  # the first tick's flip is still there
            _windows_equal(arena, ring, windows, ("tick", k))
            # the receive half over the tick's own descriptors, at their far offsets
            if dirty and k == 0:
                _dirty(p, arena, ring)
            n = t["written"]
            clients.verify(arena, table.descs_of(n), base, status=status)
            clients.accumulate(arena.numel(), table.descs_of(n), status, base)
            torch.cuda.synchronize()
            c_arena, c_descs = F.compact_view(ring, t["descs"][:n], p.arena_bytes)
            recs, res, _ = oracle.media_stream_verify(c_arena, c_descs)
            want = F.status_of(recs, res)
            got = status.cpu().numpy().view(DGRAM_STATUS_DTYPE)[:n]
            for f in DGRAM_STATUS_DTYPE.names:
                assert np.array_equal(got[f], want[f]), (dirty, k, f)
            assert (want["pass"] == 0).sum() == (1 if dirty and k == 0 else 0)
            view.receive(t["descs"]["conn_index"][:n], want["kind"], want["pass"], base)
            view.accumulate(t["descs"]["conn_index"][:n], want, base)
            base += n
        block, results = engine.new_counters(), clients.new_results(n_conns)
        clients.close(_ids(range(n_conns)), block, results=results)
        torch.cuda.synchronize()
        want = view.close(list(range(n_conns)))
        got = results.cpu().numpy().view(MS_CONN_RESULT_DTYPE)
        for f in MS_CONN_RESULT_DTYPE.names:
            assert np.array_equal(got[f], want[f]), (dirty, f)
        assert (got["first_fail"] != F.EMPTY).sum() == int(dirty)
        assert engine.read_counters_close(block) == view.close_block and clients.read_udp() == view.udp, dirty
        _upload(arena, blank, windows)
    del arena
    torch.cuda.empty_cache()


# ---- 7. the TCP senders' ticks, plain and paced, the exchange tick, and the receive half over their descriptors ------
def _tcp_ticks(engine, p: F.TickPlan):
    """kind "exchange": the receivers are 2 x the connections (direction d of connection c is receiver c + d x the
    table's size), the entries are the 64-byte ones and the tick block has its bytes by direction."""
    stride, n_senders = p.stride, len(p.settings)
    windows, blank = p.windows(), F.SparseRing(p.arena_bytes)
    arena = _arena(p.arena_bytes)
    ids, paced, exchange = _ids(p.ids), p.kind == "paced", p.kind == "exchange"
    n_conns = 2 * n_senders if exchange else n_senders
    for dirty in (False, True):
        if exchange:
            table = X.ExchangeTable(engine, p.settings, stride, p.capacity, arena_slots=1, fill=F.BACKGROUND)
        elif paced:
            table = T.PacedSenderTable(engine, p.settings, p.pace_settings, stride, p.capacity, start_ms=1000,
                                       arena_slots=1, fill=F.BACKGROUND)
            assert np.array_equal(table.fresh_pace, p.pace)
        else:
            table = T.SenderTable(engine, p.settings, stride, p.capacity, arena_slots=1, fill=F.BACKGROUND)
        table.load(p.entries)
        paths = [dict(hint=h, cff=torch.full((n_conns,), -1, dtype=torch.int32, device=DEV), ctr=engine.new_counters())
                 for h in (0, 1472)]  # the workgroup path and the quad path
        state, ref = engine.new_conn_state(n_conns), engine.new_counters()
        base, all_descs, failed = 0, [], []
        sums = dict.fromkeys(oracle.COUNTER_FIELDS, 0)
        for k, t in enumerate(p.ticks()):
            if exchange:
                X.exchange_send(engine, arena, stride, t["first_slot"], p.capacity, ids, p.max_buffers, table.entries,
                                n_senders, table.descs, table.scratch, codes=table.codes, tick=table.tick,
                                sent_counters=table.sent)
            elif paced:
                T.senders_send_paced(engine, arena, stride, t["first_slot"], p.capacity, ids, p.max_buffers,
                                     table.senders, table.pace, n_conns, p.now[k], table.descs, table.scratch,
                                     codes=table.codes, tick=table.tick, sent_counters=table.sent)
            else:
                T.senders_send(engine, arena, stride, t["first_slot"], p.capacity, ids, p.max_buffers, table.senders,
                               n_conns, table.descs, table.scratch, codes=table.codes, tick=table.tick,
                               sent_counters=table.sent)
            torch.cuda.synchronize()
            entries, codes, tick = table.read()
            for f in (TCP_EXCHANGE_DTYPE if exchange else TCP_SENDER_DTYPE).names:
                assert np.array_equal(entries[f], t["entries"][f]), (k, f)
            assert np.array_equal(codes[: len(p.ids)], t["codes"]), k
            got_tick = {f: int(tick[f]) for f in W.TCP_SENDER_TICK_FIELDS}
            if exchange:
                got_tick["bytes_dir"] = tick["bytes_dir"].tolist()
            assert got_tick == t["tick"] and int(tick["reserved"]) == 0, k
            if paced:
                assert {f: int(tick[f]) for f in W.TCP_SENDER_PACED_TAIL_FIELDS} == t["tail"], k
                pace = table.read_pace()
                for f in TCP_SENDER_PACE_DTYPE.names:
                    assert np.array_equal(pace[f], t["pace"][f]), (k, f)
            descs, model = table.descs.cpu().numpy().view(DESC_DTYPE)[: p.capacity], p.outcome(n_ticks=k + 1)
            for f in DESC_DTYPE.names:
                assert np.array_equal(descs[f], model["descs"][k][f]), (k, f)
            assert table.read_sent() == t["counters"], k
            ring = model["ring"]
            if dirty and k > 0:
                _dirty(p, None, ring)  # the first tick's flip is still there
            _windows_equal(arena, ring, windows, ("tick", k))
            # the receive half: cts_verify_at on both paths, the accounting pass, over the tick's own descriptors
            if dirty and k == 0:
                _dirty(p, arena, ring)
            n = t["written"]
            c_arena, c_descs = F.compact_view(ring, t["descs"][:n], p.arena_bytes)
            want, ctr, _ = oracle.verify_batch(c_arena, c_descs)
            for path in paths:
                res = engine.new_results(n)
                engine.verify(arena, table.descs_of(n), max_length_hint=path["hint"], results=res,
                              counters=path["ctr"], conn_first_fail=path["cff"], base_index=base)
                torch.cuda.synchronize()
                got = res.cpu().numpy().view(RESULT_DTYPE)
                for f in RESULT_DTYPE.names:
                    assert np.array_equal(got[f], want[f]), (dirty, k, path["hint"], f)
            assert (want["pass"] == 0).sum() == (1 if dirty and k == 0 else 0)
            engine.refview_conns(arena.numel(), table.descs_of(n), ref, state, base_index=base,
                                 conn_first_fail=paths[0]["cff"])
            sums = {f: sums[f] + ctr[f] for f in sums}
            all_descs.append(t["descs"][:n])
            failed.append(want["pass"] == 0)
            base += n
        torch.cuda.synchronize()
        all_descs, failed = np.concatenate(all_descs), np.concatenate(failed)
        g = np.arange(base, dtype=np.int64)
        want_ref, slots = W.reference_view(all_descs, failed, g, n_conns)
        want_table, _ = W.connection_view(all_descs, failed, g, n_conns)
        for path in paths:
            assert np.array_equal(path["cff"].cpu().numpy().view(np.uint32), slots), (dirty, path["hint"])
            assert engine.read_counters(path["ctr"]) == sums, (dirty, path["hint"])
        assert (slots != F.EMPTY).sum() == int(dirty)
        assert engine.read_counters_ref(ref) == want_ref, dirty
        got = state.cpu().numpy().view(CONN_STATE_DTYPE)
        for f in CONN_STATE_DTYPE.names:
            assert np.array_equal(got[f], want_table[f]), (dirty, f)
        if exchange:  # what the two ticks carried to each receiver, the direction-0 receivers first
            carried = p.ticks()[-1]["entries"]["bytes_sent"] - p.entries["bytes_sent"]
            expected_bytes = np.concatenate([carried[:, 0], carried[:, 1]]).astype(np.uint64)
            assert int(expected_bytes.sum()) == sum(t["tick"]["bytes"] for t in p.ticks())
        else:
            expected_bytes = np.array([min(t, 6 * p.B) for t, _ in p.settings], dtype=np.uint64)
        block, results = engine.new_counters(), engine.new_conn_results(n_conns)
        engine.conns_close(_ids(range(n_conns)), torch.from_numpy(expected_bytes.view(np.int64).copy()).to(DEV),
                           paths[0]["cff"], state, block, results=results)
        torch.cuda.synchronize()
        want_res, want_block, _, _ = W.close_results(want_table, slots, list(range(n_conns)), expected_bytes)
        got = results.cpu().numpy().view(CONN_RESULT_DTYPE)
        for f in CONN_RESULT_DTYPE.names:
            assert np.array_equal(got[f], want_res[f]), (dirty, f)
        assert engine.read_counters_close(block) == want_block, dirty
        _upload(arena, blank, windows)
    del arena
    torch.cuda.empty_cache()


@pytest.mark.parametrize("stride,B", F.TCP_SHAPES)
def test_tcp_sender_ticks_across_the_seam(engine, stride, B):
    _tcp_ticks(engine, F.TickPlan("tcp", stride, B))


@pytest.mark.parametrize("pace", ["cut", "unpaced"])
@pytest.mark.parametrize("stride,B", F.TCP_SHAPES)
def test_paced_sender_ticks_across_the_seam(engine, stride, B, pace):
    _tcp_ticks(engine, F.TickPlan("paced", stride, B, pace=pace))


@pytest.mark.parametrize("stride,B", F.TCP_SHAPES)
def test_exchange_ticks_across_the_seam(engine, stride, B):
    """Push, Pull, two PushPull (one seeked past 2^33 buffers, its turn inside the first tick), Duplex and one that
    finds no room: tcp_exchange_descs' (first_slot + g) * stride and the senders' fill over the 48-byte tick block,
    then cts_verify_at and the accounting over 12 receivers."""
    _tcp_ticks(engine, F.TickPlan("exchange", stride, B))


def test_one_exchange_tick_moves_more_than_4_gib(engine):
    """360 buffers of 16 MiB - 5 bytes in one tick: tick.bytes, bytes_dir[0] and the sent block hold values above
    2^32 (tcp_exchange_apply's two wave_sum64, the dir[][] words in LDS, one atomic per direction per tile), and the
    slots run from byte 0 across byte 2^32 to 5.6 GiB. The expectation is plan_depths.exchange_tick's; the arena is
    checked on the device by cts_verify over the tick's own descriptors, and three slots (four with the one that ends
    at byte 2^32) are compared on the host."""
    import plan_depths as P

    case = F.big_exchange_tick()
    stride, B, capacity = case["stride"], case["B"], case["capacity"]
    need = capacity * stride + (1 << 30)
    free = torch.cuda.mem_get_info(0)[0]
    if free < need:
        pytest.skip("the device has %d bytes free, the arena and 1 GiB are %d" % (free, need))
    state = P.exchange_state(case["settings"])
    n_conns = len(state)
    want = P.exchange_tick(state, case["ids"], stride, capacity, case["max_buffers"], n_conns)
    assert want["bytes_dir"][0] >= SEAM and want["tick"]["bytes"] >= SEAM and want["bytes_dir"][1] > 0
    table = X.ExchangeTable(engine, case["settings"], stride, capacity, fill=F.BACKGROUND)
    table.send(_ids(case["ids"]), case["max_buffers"])
    torch.cuda.synchronize()
    entries, codes, tick = table.read()
    expected = P.exchange_records(want["entries"])
    for f in TCP_EXCHANGE_DTYPE.names:
        assert np.array_equal(entries[f], expected[f]), f
    assert codes[:n_conns].tolist() == want["codes"]
    assert {f: int(tick[f]) for f in W.TCP_SENDER_TICK_FIELDS} == want["tick"] and int(tick["reserved"]) == 0
    assert tick["bytes_dir"].tolist() == want["bytes_dir"]
    sent = dict.fromkeys(W.SENT_FIELDS, 0)
    sent.update(bytes_sent=want["tick"]["bytes"], buffers_sent=capacity)
    assert table.read_sent() == sent
    descs = table.descs.cpu().numpy().view(DESC_DTYPE)[:capacity]
    assert descs["byte_offset"].tolist() == [g * stride for g in range(capacity)]
    assert list(zip(descs["conn_index"].tolist(), descs["length"].tolist(),
                    descs["expected_pattern_offset"].tolist())) == want["slots"]
    assert not descs["skip_head"].any()
    # the arena: the device's verify over all 360 descriptors, then four slots and their tails on the host
    ctr, res = engine.new_counters(), engine.new_results(capacity)
    engine.verify(table.arena, table.descs_of(capacity), max_length_hint=stride, results=res, counters=ctr)
    torch.cuda.synchronize()
    got = res.cpu().numpy().view(RESULT_DTYPE)
    assert (got["pass"] == 1).all() and not got["flags"].any()
    total = want["tick"]["bytes"]
    assert engine.read_counters(ctr) == {"bytes_checked": total, "bytes_ok": total, "buffers_checked": capacity,
                                         "buffers_failed": 0, "mismatched_bytes": 0}
    assert SEAM // stride == 256
    for g in (0, 255, 256, capacity - 1):
        _, length, offset = want["slots"][g]
        slot = table.arena[g * stride:(g + 1) * stride].cpu().numpy()
        assert np.array_equal(slot[:length], F.pattern(offset, length)), g
        assert (slot[length:] == F.BACKGROUND).all() and stride - length == 5, g
    del table
    torch.cuda.empty_cache()


# ---- 8. the accounting passes over a ring of 4 GiB: no arena -------------------------------------------------------
@pytest.mark.parametrize("stride,skip", [(1472, 26), (1 << 20, 0)])
def test_accounting_strided_across_the_seam(engine, stride, skip):
    """cts_refview_accumulate_strided and _conns_strided read lengths and slots, never the arena: arena_bytes of
    4 GiB and a cut inside the last slot, nothing allocated."""
    p = F.RingPlan(stride, "tcp", skip=skip, base_index=BASE)
    lens = _lengths(p)
    for slot in (BASE + p.above, BASE + p.below, F.EMPTY):
        slots = np.array([5, slot, F.EMPTY], dtype=np.uint32)
        want, want_table = p.accounting(slots)
        try:
            for nt in (1, 0):
                _set_nt(engine, nt)
                ref, plain, state = engine.new_counters(), engine.new_counters(), engine.new_conn_state(p.n_conns)
                cff = _dev(slots).view(torch.int32)
                engine.refview_conns_strided(p.arena_bytes, stride, lens, ref, state, skip_head=skip, conn_index=p.conn,
                                             base_index=BASE, conn_first_fail=cff)
                engine.refview_strided(p.arena_bytes, stride, lens, plain, skip_head=skip, conn_index=p.conn,
                                       base_index=BASE, conn_first_fail=cff)
                torch.cuda.synchronize()
                got = state.cpu().numpy().view(CONN_STATE_DTYPE)
                for f in CONN_STATE_DTYPE.names:
                    assert got[f].tolist() == want_table[f].tolist(), (slot, nt, f)
                assert engine.read_counters_ref(ref) == want, (slot, nt)
                assert engine.read_counters_ref(plain) == want, (slot, nt)
                assert np.array_equal(cff.cpu().numpy().view(np.uint32), slots)
        finally:
            _set_nt(engine, 1)
    del lens
    torch.cuda.empty_cache()
