"""GPU: MediaStream servers on the device-resident path (include/cts_media_stream_servers.h) against the model
workload.media_stream_server_view, which is itself held against the oracle in tests/test_media_stream_servers_cpu.py.
The ring is pre-filled with 0xA5 and every byte of it is compared, so stray writes show; entries, codes, the tick
block, descriptors, lengths and the UDP block are compared field by field. Every comparison is exact.
"""
import os

import numpy as np
import pytest
import torch

from ctstraffic_amd import media_stream as M
from ctstraffic_amd import workload as W
from ctstraffic_amd._lib import CtsError
from ctstraffic_amd.types import (DESC_DTYPE, DGRAM_HEADER_DTYPE, DGRAM_STATUS_DTYPE, MS_CONN_RESULT_DTYPE,
                                  MS_SERVER_STATE_DTYPE)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
QPC, QPF = 0x0102030405060708, -0x1112131415161718  # every byte distinct, one of them negative


def _ids(ids):
    return torch.from_numpy(np.asarray(list(ids), dtype=np.uint32).view(np.int32).copy()).to(DEV)


def _pair(engine, settings, stride, capacity, ring_slots=None, max_listed=None, entries=None):
    """A device table and its model over the same entries and a ring of 0xA5."""
    table = M.ServerTable(engine, settings, stride, capacity, ring_slots=ring_slots, fill=0xA5, max_listed=max_listed)
    assert np.array_equal(table.fresh, W.media_stream_server_entries(settings))
    if entries is not None:
        table.load(entries)
    ring = np.full(table.ring.numel(), 0xA5, dtype=np.uint8)
    return table, W.media_stream_server_view(table.fresh if entries is None else entries, stride, ring, capacity)


def _same(table, view, n_listed, where=""):
    torch.cuda.synchronize()
    entries, codes, tick = table.read()
    for f in MS_SERVER_STATE_DTYPE.names:
        assert np.array_equal(entries[f], view.entries[f]), (where, f)
    assert np.array_equal(codes[:n_listed], view.codes), where
    for f in W.MS_SERVER_TICK_FIELDS:
        assert int(tick[f]) == view.tick[f], (where, f)
    assert int(tick["reserved"]) == 0
    ring, descs, lengths = table.read_ring()
    for f in DESC_DTYPE.names:
        assert np.array_equal(descs[f], view.descs[f]), (where, f)
    assert np.array_equal(lengths, view.lengths), where
    assert np.array_equal(ring, view.ring), where
    assert table.read_udp() == view.udp, where


def _tick(table, view, ids, qpc=QPC, qpf=QPF, first_slot=0, where=""):
    table.send(_ids(ids), qpc, qpf, first_slot=first_slot)
    view.send(ids, qpc, qpf, first_slot=first_slot)
    _same(table, view, len(ids), where)


def _residues(M_):
    return [27, M_ - 1, M_, M_ + 1, M_ + 26, M_ + 27, 2 * M_, 2 * M_ + 13, 3 * M_ + 500]


# ---- 1: the split's edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("M_,stride", [(1400, 1408), (53, 64), (1472, 1472)])
def test_split_edges(engine, M_, stride):
    """One connection per (F, M) pair; M = stride = 1472 is the `whole` fast path, every chunk of a slot stored."""
    settings = [(F, M_, 2) for F in _residues(M_)]
    capacity = sum(-(-F // M_) for F, _, _ in settings)
    table, view = _pair(engine, settings, stride, capacity, ring_slots=capacity + 2)
    _tick(table, view, range(len(settings)), where="frame 1")
    assert view.tick["datagrams"] == capacity and set(view.codes.tolist()) == {0}
    _tick(table, view, range(len(settings)), where="frame 2")
    assert set(view.codes.tolist()) == {1}


# ---- 2: strides on both sides of 1024, first_slot 0 and 3 ------------------------------------------------------
@pytest.mark.parametrize("stride", [64, 1008, 1024, 1408])
@pytest.mark.parametrize("first_slot", [0, 3])
def test_strides_and_first_slot(engine, stride, first_slot):
    big = min(stride, 1400)
    settings = [(3 * big + 5, big, 3), (27, 53, 3), (2 * 60 + 30, 60, 3), (big, big, 3), (5 * 53 + 10, 53, 3)]
    capacity = sum(-(-F // m) for F, m, _ in settings)
    table, view = _pair(engine, settings, stride, capacity, ring_slots=first_slot + capacity + 1)
    for t in range(2):
        _tick(table, view, [4, 0, 3, 1, 2], qpc=QPC + t, first_slot=first_slot, where="tick %d" % t)
    assert view.tick["datagrams"] == capacity


# ---- 3: prefix seams -------------------------------------------------------------------------------------------
def _mixed_settings(n, seed, finals=(1, 2, 3, 4)):
    """Each connection its own (F, M), 1..9 datagrams per frame, no two neighbours sharing a count."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        m = int(rng.integers(53, 113))
        k = 1 + (c * 4) % 9
        F = max(27, int(rng.integers((k - 1) * m + 1, k * m + 1)))
        out.append((F, m, int(finals[c % len(finals)])))
    return out


_SEAM_TABLE = _mixed_settings(1500, 3)


@pytest.mark.parametrize("n_listed", [1, 63, 64, 257, 1100])
def test_prefix_seams(engine, n_listed):
    """A shuffled, non-monotonic list out of a table of 1 500, some connections already finished, two ids beyond the
    table; three ticks, everything compared after each."""
    settings = _SEAM_TABLE
    entries = W.media_stream_server_entries(settings)
    entries["finished"][::7] = 1
    rng = np.random.default_rng(n_listed)
    ids = [int(x) for x in rng.permutation(len(settings))[:n_listed]]
    if n_listed >= 63:
        ids[5], ids[n_listed // 2] = 1500, 0xFFFFFFFF
    capacity = sum(int(entries["datagrams_per_frame"][c]) for c in ids if c < 1500)
    table, view = _pair(engine, settings, 128, capacity, max_listed=n_listed, entries=entries)
    for t in range(3):
        _tick(table, view, ids, qpc=QPC + t, where="tick %d" % t)
    if n_listed >= 63:
        assert {2, 4} <= set(view.codes.tolist()) and 0 < view.tick["datagrams"] < capacity


# ---- 4: capacity -----------------------------------------------------------------------------------------------
def test_capacity_cuts_the_list(engine):
    settings = _mixed_settings(40, 4, finals=(5,))
    k = [-(-F // m) for F, m, _ in settings]
    ids = list(range(40))
    cut = 25
    assert k[cut] >= 2
    capacity = sum(k[:cut]) + k[cut] - 1  # in the middle of connection 25's frame
    assert sum(k[cut:]) < capacity
    table, view = _pair(engine, settings, 128, capacity, ring_slots=sum(k[:cut]) + capacity + 1)
    _tick(table, view, ids, where="cut")
    assert view.codes.tolist() == [0] * cut + [3] * (40 - cut)
    assert view.tick["datagrams"] == sum(k[:cut]) and view.tick["connections_no_room"] == 40 - cut
    assert (view.entries["current_frame"][cut:] == 1).all()
    # the next tick, first_slot moved on, sends the rest first, then as many second frames as still fit
    first_slot = view.tick["datagrams"]
    _tick(table, view, ids[cut:] + ids[:cut], first_slot=first_slot, where="rest")
    assert view.codes.tolist()[: 40 - cut] == [0] * (40 - cut)
    assert (view.entries["current_frame"][cut:] == 2).all() and 3 in view.codes.tolist()


def test_capacity_exact_and_zero(engine):
    settings = _mixed_settings(9, 5, finals=(5,))
    need = sum(-(-F // m) for F, m, _ in settings)
    table, view = _pair(engine, settings, 128, need)
    _tick(table, view, range(9), where="exact")
    assert view.tick["datagrams"] == need and view.tick["connections_no_room"] == 0
    table, view = _pair(engine, settings, 128, 0, ring_slots=4)
    _tick(table, view, range(9), where="zero")
    assert view.codes.tolist() == [3] * 9 and view.tick["datagrams"] == 0


# ---- 5: the end of a stream ------------------------------------------------------------------------------------
def test_end_of_stream(engine):
    settings = [(3000, 1400, 1), (3000, 1400, 3), (27, 53, 1), (4300, 1400, 3)]
    table, view = _pair(engine, settings, 1408, 16)
    want = [[1, 0, 1, 0], [2, 0, 2, 0], [2, 1, 2, 1], [2, 2, 2, 2]]
    for t, codes in enumerate(want):
        _tick(table, view, range(4), qpc=QPC - t, where="tick %d" % t)
        assert view.codes.tolist() == codes
    assert view.tick["datagrams"] == 0 and view.tick["connections_skipped"] == 4
    assert view.entries["current_frame"].tolist() == [2, 4, 2, 4]


def test_wide_values(engine):
    """A sequence number with a high half in the header, and sums that cross 2^32 and 2^53."""
    settings = [(3000, 1400, 0xFFFFFFFF), (2900, 1472, 0xFFFFFFFF), (100, 60, 0xFFFFFFFF)]
    entries = W.media_stream_server_entries(settings)
    entries["current_frame"][0] = (1 << 32) - 2
    entries["bits_sent"][0], entries["datagrams_sent"][0] = (1 << 32) - 8, (1 << 32) - 1
    entries["current_frame"][1] = (1 << 32) - 1
    entries["bits_sent"][1], entries["datagrams_sent"][1] = (1 << 53) - 8, (1 << 53) - 1
    table, view = _pair(engine, settings, 1472, 8, entries=entries)
    for t, codes in enumerate([[0, 1, 0], [1, 2, 0], [2, 2, 0]]):
        _tick(table, view, range(3), qpc=-QPC, qpf=QPC ^ (t << 60), where="tick %d" % t)
        assert view.codes.tolist() == codes
    assert int(view.entries["bits_sent"][0]) == (1 << 32) - 8 + 2 * 8 * 3000
    assert int(view.entries["datagrams_sent"][1]) == (1 << 53) + 1
    assert int(view.entries["current_frame"][0]) == 1 << 32


# ---- 6: several batches per workgroup --------------------------------------------------------------------------
def test_several_batches_per_workgroup():
    """One workgroup per CU, 2 x 512 x CUs + 77 datagrams of 53 bytes at stride 64: every workgroup walks more than
    one batch and the last batch is ragged."""
    from ctstraffic_amd import Engine

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    total = 2 * 512 * cus + 77
    ks = [1, 511, 77, 1025, 2, 3 * 512]
    ks.append(total - sum(ks) - 9)
    ks += [9]
    settings = [(53 * k - (0 if c % 2 else 20), 53, 2) for c, k in enumerate(ks)]
    assert sum(-(-F // 53) for F, _, _ in settings) == total
    old = os.environ.get("CTS_RING_FILL_BLOCKS_PER_CU")
    os.environ["CTS_RING_FILL_BLOCKS_PER_CU"] = "1"
    try:
        eng = Engine(0)
    finally:
        if old is None:
            del os.environ["CTS_RING_FILL_BLOCKS_PER_CU"]
        else:
            os.environ["CTS_RING_FILL_BLOCKS_PER_CU"] = old
    try:
        table, view = _pair(eng, settings, 64, total)
        _tick(table, view, range(len(ks)), where="one workgroup per CU")
        assert view.tick["datagrams"] == total
    finally:
        eng.close()


def test_several_batches_per_workgroup_wide_slots():
    """The same at stride 1040, the store loop's wave-uniform form with 65 chunks per slot: one workgroup per CU,
    (512 + 19) x CUs datagrams, so every workgroup stages a second batch whose first ring chunk is not 0 and whose
    64-chunk rounds cross datagram boundaries; full slots, 1000-byte datagrams and short last ones."""
    import launch_depths as L
    from ctstraffic_amd import Engine

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    total = L.batched_n("ring1040", cus)
    depth = L.batch_fill_depth(total, L.RING_BATCH, cus, 1, 1040)
    assert L.batched_reaches("ring1040", depth) == [], depth
    ks = [1, 511, 77, 1025, 2, 3 * 512]
    ks.append(total - sum(ks) - 9)
    ks += [9]
    sizes = [1040, 1040, 1000, 1040, 1040, 1000, 1040, 1040]
    settings = [(m * k - (0 if c % 2 else 20), m, 2) for c, (k, m) in enumerate(zip(ks, sizes))]
    assert sum(-(-F // m) for F, m, _ in settings) == total
    old = os.environ.get("CTS_RING_FILL_BLOCKS_PER_CU")
    os.environ["CTS_RING_FILL_BLOCKS_PER_CU"] = "1"
    try:
        eng = Engine(0)
    finally:
        if old is None:
            del os.environ["CTS_RING_FILL_BLOCKS_PER_CU"]
        else:
            os.environ["CTS_RING_FILL_BLOCKS_PER_CU"] = old
    try:
        table, view = _pair(eng, settings, 1040, total)
        _tick(table, view, range(len(ks)), where="one workgroup per CU, stride 1040")
        assert view.tick["datagrams"] == total
    finally:
        eng.close()


# ---- 7: argument edges -----------------------------------------------------------------------------------------
def test_argument_edges(engine):
    settings = [(3000, 1400, 3), (100, 60, 3)]
    table, view = _pair(engine, settings, 1408, 8, ring_slots=12)
    ids = _ids([0, 1])
    p = {k: getattr(table, k).data_ptr() for k in ("ring", "servers", "descs", "lengths", "codes", "tick", "udp",
                                                   "scratch")}
    ring_bytes, scratch_bytes = table.ring.numel(), table.scratch.numel() * 8

    def send(stride=1408, first_slot=0, capacity=8, conn_ids=ids.data_ptr(), n=2, n_conns=2, arena_bytes=ring_bytes,
             sbytes=scratch_bytes, **over):
        a = dict(p, **over)
        M.servers_send(engine, a["ring"], stride, first_slot, capacity, conn_ids, a["servers"], n_conns, QPC, QPF,
                       a["scratch"], descs=a["descs"], lengths=a["lengths"], codes=a["codes"], tick=a["tick"],
                       udp_counters=a["udp"], n=n, arena_bytes=arena_bytes, scratch_bytes=sbytes)

    bad = [dict(stride=1400), dict(stride=16), dict(stride=(1 << 20) + 16), dict(stride=0),
           dict(ring=p["ring"] + 8), dict(ring=None),
           dict(first_slot=5), dict(capacity=13), dict(first_slot=13, capacity=0), dict(first_slot=(1 << 64) - 1),
           dict(first_slot=(1 << 64) - 4, capacity=8), dict(arena_bytes=8 * 1408 - 1),
           dict(servers=p["servers"] + 4), dict(servers=None), dict(descs=p["descs"] + 4), dict(tick=p["tick"] + 4),
           dict(udp=p["udp"] + 4), dict(scratch=p["scratch"] + 4), dict(scratch=None),
           dict(conn_ids=ids.data_ptr() + 2), dict(conn_ids=None), dict(lengths=p["lengths"] + 2),
           dict(codes=p["codes"] + 2), dict(sbytes=M.servers_scratch_bytes(2) - 1), dict(sbytes=0)]
    for kw in bad:
        with pytest.raises(CtsError) as e:
            send(**kw)
        assert e.value.status == -1, kw
    torch.cuda.synchronize()
    entries, _, tick = table.read()
    assert np.array_equal(entries, table.fresh) and int(tick["datagrams"]) == 0
    assert (table.ring.cpu().numpy() == 0xA5).all() and table.read_udp() == view.udp

    # n == 0 is CTS_OK and does nothing, whatever else is passed
    send(n=0, stride=7, ring=None)
    torch.cuda.synchronize()
    assert (table.ring.cpu().numpy() == 0xA5).all()

    # each output null in turn: the others are written as ever
    for t, null in enumerate(["descs", "lengths", "codes", "tick", "udp"]):
        before = {k: getattr(table, k).clone() for k in ("descs", "lengths", "codes", "tick", "udp")}
        send(first_slot=4 * (t % 2), **{null: None})
        view.send([0, 1], QPC, QPF, first_slot=4 * (t % 2))
        torch.cuda.synchronize()
        assert torch.equal(getattr(table, null), before[null]), null
        entries, codes, tick = table.read()
        ring, descs, lengths = table.read_ring()
        assert np.array_equal(entries, view.entries) and np.array_equal(ring, view.ring), null
        if null != "descs":
            assert np.array_equal(descs, view.descs)
        if null != "lengths":
            assert np.array_equal(lengths, view.lengths)
        if null != "codes":
            assert np.array_equal(codes[:2], view.codes)
        if null != "tick":
            assert all(int(tick[f]) == view.tick[f] for f in W.MS_SERVER_TICK_FIELDS)
        if null == "udp":
            view.udp["bits_received"] -= 8 * view.tick["bytes"]
            view.udp["datagrams"] -= view.tick["datagrams"]
        assert table.read_udp() == view.udp, null
        if t == 2:  # three frames sent: start the streams again for the last two rounds
            table.load(table.fresh)
            view.entries[:] = table.fresh


# ---- 8: the loop closed on the device --------------------------------------------------------------------------
def test_servers_into_clients_on_the_device(engine):
    """37 servers and their 37 clients: send -> receive pass -> accounting pass -> render per tick, n from the settings
    and nothing read back inside the loop; then the close."""
    n_conns = 37
    rng = np.random.default_rng(8)
    settings = []
    for c in range(n_conns):
        m = int(rng.integers(53, 1409))
        k = 1 + c % 5
        settings.append((max(27, int(rng.integers((k - 1) * m + 1, k * m + 1))), m, 1 + c % 4))
    per_frame = [-(-F // m) for F, m, _ in settings]
    capacity, stride = sum(per_frame), 1408
    servers = M.ServerTable(engine, settings, stride, capacity, fill=0xA5)
    clients = M.ConnectionTable(engine, [(F, 1 + c % 3, final) for c, (F, _, final) in enumerate(settings)])
    ids = _ids(range(n_conns))
    status = torch.zeros(capacity * DGRAM_STATUS_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    payload = engine.new_counters()
    base, payload_bytes = 0, 0
    for t in range(max(f for _, _, f in settings)):
        running = [c for c in range(n_conns) if t < settings[c][2]]
        n = sum(per_frame[c] for c in running)
        assert n == servers.datagrams_per_tick(running)
        servers.send(ids, 1000 + t, 10_000_000)
        descs = servers.descs_of(n)
        clients.verify(servers.ring, descs, base, status=status)
        clients.accumulate(servers.ring.numel(), descs, status, base)
        engine.verify(servers.ring, descs, counters=payload)
        clients.render(ids)
        base += n
        payload_bytes += sum(settings[c][0] - 26 * per_frame[c] for c in running)
    block, results = engine.new_counters(), clients.new_results(n_conns)
    clients.close(ids, block, results=results)
    torch.cuda.synchronize()
    res = results.cpu().numpy().view(MS_CONN_RESULT_DTYPE)
    entries, _, _ = servers.read()
    finals = np.array([f for _, _, f in settings], dtype=np.uint64)
    assert (res["status"] == 0).all() and (res["flags"] == 0).all() and (res["finished"] == 1).all()
    assert np.array_equal(res["successful_frames"], finals)
    for f in ("dropped_frames", "duplicate_frames", "error_frames", "datagrams_after_end"):
        assert (res[f] == 0).all(), f
    assert (entries["finished"] == 1).all()
    assert np.array_equal(res["bits_received"], entries["bits_sent"])
    assert np.array_equal(res["datagrams"], entries["datagrams_sent"])
    cu, su = clients.read_udp(), servers.read_udp()
    assert cu["bits_received"] == su["bits_received"] == int(entries["bits_sent"].sum())
    assert cu["datagrams"] == su["datagrams"] == int(entries["datagrams_sent"].sum()) == base
    assert cu["successful_frames"] == int(finals.sum()) and cu["dropped_frames"] == cu["error_frames"] == 0
    close = engine.read_counters_close(block)
    assert close["connections_closed"] == close["successful"] == n_conns
    got = engine.read_counters(payload)
    assert got["bytes_checked"] == got["bytes_ok"] == payload_bytes and got["buffers_failed"] == 0
    assert got["buffers_checked"] == base


# ---- 9: the device-written ring against the host-fed one -------------------------------------------------------
@pytest.mark.parametrize("stride", [64, 1472])
def test_same_ring_as_the_host_fed_fill(engine, stride):
    big = min(stride, 1472)
    settings = [(3 * big, big, 2), (27, 53, 2), (2 * big + 13, big, 2), (big + 27, big, 2), (7 * 53 + 1, 53, 2)] * 9
    capacity = sum(-(-F // m) for F, m, _ in settings)
    table, view = _pair(engine, settings, stride, capacity)
    order = list(np.random.default_rng(9).permutation(len(settings)))
    for frame in (1, 2):
        table.send(_ids(order), QPC, QPF)
        view.send(order, QPC, QPF)
        headers = np.zeros(capacity, dtype=DGRAM_HEADER_DTYPE)
        headers["sequence_number"], headers["qpc"], headers["qpf"] = frame, QPC, QPF
        host_fed = torch.full((capacity * stride,), 0xA5, dtype=torch.uint8, device=DEV)
        M.fill_strided(engine, host_fed, stride, torch.from_numpy(view.lengths.view(np.int32).copy()).to(DEV),
                       torch.from_numpy(headers.view(np.uint8).copy()).to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(table.ring, host_fed)
        assert np.array_equal(host_fed.cpu().numpy(), view.ring)
