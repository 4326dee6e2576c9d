"""GPU: the MediaStream servers' timed tick (cts_media_stream_servers_send_at of include/cts_media_stream_servers.h)
against the model workload.MediaStreamServerView.send_at, which finds the frames that are out as the reference does,
one frame after the other, and is itself held against the plain tick's model and the host closed form in
tests/test_media_stream_servers_timed_cpu.py. The ring is pre-filled with 0xA5 and every byte of it is compared, so
stray writes show; entries, codes, the 48-byte tick block, descriptors, lengths and the UDP block are compared field
by field. Every comparison is exact.
"""
import struct

import numpy as np
import pytest
import torch

from ctstraffic_amd import media_stream as M
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import DESC_DTYPE, DGRAM_STATUS_DTYPE, MS_CONN_RESULT_DTYPE, MS_SERVER_STATE_DTYPE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
QPC, QPF = 0x0102030405060708, -0x1112131415161718  # every byte distinct, one of them negative
I64_MAX = (1 << 63) - 1
U32_MAX = 0xFFFFFFFF
LONG_DUE = 10**9  # a now_ms by which every frame of the tables below is out


def _ids(ids):
    return torch.from_numpy(np.asarray(list(ids), dtype=np.uint32).view(np.int32).copy()).to(DEV)


class _Pair:
    """A device table with its schedule and the model over the same entries, schedule and a ring of 0xA5."""

    def __init__(self, engine, settings, schedule, stride, capacity, ring_slots=None, max_listed=None, entries=None):
        self.schedule = (schedule if isinstance(schedule, np.ndarray) else W.media_stream_server_schedule(schedule))
        self.table = M.ServerTable(engine, settings, stride, capacity, ring_slots=ring_slots, fill=0xA5,
                                   max_listed=max_listed, schedule=self.schedule)
        if entries is not None:
            self.table.load(entries)
        ring = np.full(self.table.ring.numel(), 0xA5, dtype=np.uint8)
        self.view = W.media_stream_server_view(self.table.fresh if entries is None else entries, stride, ring,
                                               capacity)

    def tick(self, ids, now, max_frames, qpc=QPC, qpf=QPF, first_slot=0, where=""):
        """One timed tick on the device and in the model, everything compared. Returns (codes, tick) of the model."""
        self.table.send_at(_ids(ids), now, max_frames, qpc, qpf, first_slot=first_slot)
        codes, tick = self.view.send_at(ids, self.schedule, now, max_frames, qpc, qpf, first_slot=first_slot)
        self.same(len(ids), where)
        return codes, tick

    def same(self, n_listed, where=""):
        torch.cuda.synchronize()
        table, view = self.table, self.view
        entries, codes, tick = table.read_timed()
        for f in MS_SERVER_STATE_DTYPE.names:
            assert np.array_equal(entries[f], view.entries[f]), (where, f)
        assert np.array_equal(codes[:n_listed], view.codes), where
        for f in W.MS_SERVER_TIMED_TICK_FIELDS:
            assert int(tick[f]) == view.tick[f], (where, f)
        assert int(tick["reserved"]) == 0
        ring, descs, lengths = table.read_ring()
        for f in DESC_DTYPE.names:
            assert np.array_equal(descs[f], view.descs[f]), (where, f)
        assert np.array_equal(lengths, view.lengths), where
        assert np.array_equal(ring, view.ring), where
        assert table.read_udp() == view.udp, where


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


def _frame_settings(k, final, m=53):
    """A connection of k datagrams a frame, the last one short."""
    return (m * k - 20, m, final) if k > 1 else (m - 20, m, final)


# ---- 1: max_frames = 1 and every frame out is the plain tick ---------------------------------------------------
_SEAM_TABLE = _mixed_settings(1500, 3)


@pytest.mark.parametrize("n_listed", [1, 63, 64, 257, 1100])
def test_equivalence_with_the_plain_tick(engine, n_listed):
    """send_at on one table and send on its twin: entries, ring, descriptors, lengths, codes, the UDP block and the
    first 32 bytes of the tick block byte for byte, over three ticks of a shuffled list with finished connections and
    two ids beyond the table."""
    settings = _SEAM_TABLE
    entries = W.media_stream_server_entries(settings)
    entries["finished"][::7] = 1
    rng = np.random.default_rng(n_listed)
    ids = [int(x) for x in rng.permutation(len(settings))[:n_listed]]
    if n_listed >= 63:
        ids[5], ids[n_listed // 2] = 1500, U32_MAX
    capacity = sum(int(entries["datagrams_per_frame"][c]) for c in ids if c < 1500)
    schedule = [(1 + (c * 37) % 2000, 1000 + 13 * c) for c in range(len(settings))]
    timed = _Pair(engine, settings, schedule, 128, capacity, max_listed=n_listed, entries=entries)
    plain = M.ServerTable(engine, settings, 128, capacity, fill=0xA5, max_listed=n_listed)
    plain.load(entries)
    dev_ids = _ids(ids)
    for t in range(3):
        codes, tick = timed.tick(ids, LONG_DUE + t, 1, qpc=QPC + t, where="tick %d" % t)
        plain.send(dev_ids, QPC + t, QPF)
        torch.cuda.synchronize()
        for name in ("servers", "ring", "descs", "lengths", "udp"):
            assert torch.equal(getattr(timed.table, name), getattr(plain, name)), (t, name)
        assert torch.equal(timed.table.codes[:n_listed], plain.codes[:n_listed]), t
        assert torch.equal(timed.table.timed_tick[:4], plain.tick), t
        assert tick["frames"] == tick["connections_sent"] and tick["connections_waiting"] == 0
    if n_listed >= 63:
        assert {2, 4} <= set(codes.tolist()) and 0 < tick["datagrams"] < capacity


# ---- 2: catch-up across fill batches and workgroup ranges ------------------------------------------------------
def _sequence_numbers(ring, stride, n):
    return [struct.unpack_from("<Hqqq", ring, g * stride)[1] for g in range(n)]


@pytest.mark.parametrize("k", [3, 1, 7])
def test_catch_up_of_one_connection(engine, k):
    """400 frames of one connection are out at once: 400 k datagrams in one tick, batch after batch of 512."""
    frames = 400
    pair = _Pair(engine, [_frame_settings(k, 1000)], [(1000, 5000)], 64, frames * k)
    codes, tick = pair.tick([0], 5000 + frames - 1, 1000, where="k %d" % k)  # due(f) = 5000 + f: frames 1 .. 400
    assert codes.tolist() == [0] and tick["frames"] == frames and tick["datagrams"] == frames * k
    assert tick["next_due_ms"] == 5000 + frames + 1
    ring = pair.table.ring.cpu().numpy()
    assert _sequence_numbers(ring, 64, frames * k) == [1 + q // k for q in range(frames * k)]
    codes, tick = pair.tick([0], 5000 + frames - 1, 1000, where="again")
    assert codes.tolist() == [5] and tick["datagrams"] == 0 and tick["connections_waiting"] == 1


def test_catch_up_seams(engine):
    """Five connections whose takes are 511, 512, 513, 1025 and 1 datagrams, listed together: frame and connection
    seams fall before, on and after a batch edge. The sequence number of every datagram is checked on its own."""
    shapes = [(73, 7), (128, 4), (171, 3), (205, 5), (1, 1)]  # (frames out, k)
    assert [m * k for m, k in shapes] == [511, 512, 513, 1025, 1]
    settings = [_frame_settings(k, 5000, m=53 + c) for c, (_, k) in enumerate(shapes)]
    first = [1, 40, 1000, 7, 5000]  # each connection's current_frame
    entries = W.media_stream_server_entries(settings)
    entries["current_frame"] = first
    total = sum(m * k for m, k in shapes)
    now = 6000
    # at 1000 frames a second due(f) = base + f: frames first .. first + m - 1 are out at `now` when base + first + m - 1
    # = now + 1. Connection 4 sends its last frame, long due.
    schedule = [(1000, 0 if c == 4 else now + 1 - (first[c] + m - 1)) for c, (m, _) in enumerate(shapes)]
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0]):
        pair = _Pair(engine, settings, schedule, 64, total, entries=entries)
        codes, tick = pair.tick(order, now, U32_MAX, where=str(order))
        assert tick["datagrams"] == total and tick["frames"] == sum(m for m, _ in shapes)
        assert codes.tolist() == [1 if c == 4 else 0 for c in order]
        want = [first[c] + q // shapes[c][1] for c in order for q in range(shapes[c][0] * shapes[c][1])]
        assert _sequence_numbers(pair.table.ring.cpu().numpy(), 64, total) == want


# ---- 3: capacity -----------------------------------------------------------------------------------------------
def test_capacity_cuts_between_two_frames(engine):
    settings = _mixed_settings(12, 4, finals=(50,))
    k = [-(-F // m) for F, m, _ in settings]
    cut, t = 7, 2
    assert k[cut] >= 2
    out = 4  # frames of every connection out at now = 1003: due(f) = 1000 + f
    capacity = out * sum(k[:cut]) + t * k[cut] + (k[cut] - 1)
    pair = _Pair(engine, settings, [(1000, 1000)] * 12, 128, capacity, ring_slots=2 * out * sum(k))
    ids = list(range(12))
    codes, tick = pair.tick(ids, 1003, 100, where="cut")
    assert codes.tolist() == [0] * (cut + 1) + [3] * (11 - cut)
    assert tick["datagrams"] == out * sum(k[:cut]) + t * k[cut] == capacity - (k[cut] - 1)  # no gap, k - 1 slots spare
    assert tick["frames"] == out * cut + t and tick["connections_no_room"] == 11 - cut
    assert tick["next_due_ms"] <= 1003 + 1  # "tick again once the ring is drained"
    assert int(pair.view.entries["current_frame"][cut]) == 1 + t
    assert (pair.view.entries["current_frame"][cut + 1:] == 1).all()
    # the follow-up tick, first_slot moved on, sends the rest
    first_slot = tick["datagrams"]
    codes, tick = pair.tick(ids, 1003, 100, first_slot=first_slot, where="rest")
    assert codes.tolist() == [5] * cut + [0] * (12 - cut)
    assert tick["frames"] == (out - t) + out * (11 - cut) and tick["connections_waiting"] == cut
    assert (pair.view.entries["current_frame"] == 1 + out).all() and tick["next_due_ms"] == 1005


# ---- 4: time ---------------------------------------------------------------------------------------------------
def _time_run(engine, capacity, seen, max_frames=2):
    rng = np.random.default_rng(44)
    n = 300
    settings = _mixed_settings(n, 5, finals=(1, 2, 3, 6))
    rates = [1, 24, 30, 60, 1000, 1001]
    schedule = [(rates[int(rng.integers(0, 6))], 2000 + 7 * c + int(rng.integers(0, 500))) for c in range(n)]
    entries = W.media_stream_server_entries(settings)
    entries["finished"][5::50] = 1
    pair = _Pair(engine, settings, schedule, 128, capacity, max_listed=n + 2, entries=entries)
    ids = [int(x) for x in rng.permutation(n)] + [n, U32_MAX]
    ids[3], ids[-1] = ids[-1], ids[3]
    nothing_sent = 0
    codes, tick = pair.tick(ids, 0, max_frames, where="before every base")
    first_due = tick["next_due_ms"]
    assert tick["datagrams"] == 0 and tick["connections_waiting"] == n - 6 and 2000 < first_due < I64_MAX
    # the host's timer around the previous tick's next_due_ms: 2 ms early, 1 ms early (the reference's grace), exactly
    # on it, then a jump of 700 ms that leaves connections behind
    now, hits = 0, set()
    for step in range(12):
        offset = (-2, -1, 0, None)[step % 4]
        if offset is None:
            now += 700
        else:
            wanted = min(tick["next_due_ms"], now + 5000) + offset
            if wanted >= now and wanted == tick["next_due_ms"] + offset:
                hits.add(offset)  # exactly that far from the previous tick's next_due_ms
            now = max(now, wanted)
        codes, tick = pair.tick(ids, now, max_frames, qpc=QPC + step, where="step %d at %d" % (step, now))
        seen |= set(codes.tolist())
        assert tick["connections_waiting"] == codes.tolist().count(5)
        running = [c for c, code in zip(ids, codes.tolist()) if code in (0, 3, 5)]
        assert tick["next_due_ms"] == min(
            [W.media_stream_frame_due(schedule[c][1], schedule[c][0], int(pair.view.entries["current_frame"][c]))
             for c in running], default=I64_MAX)
        if step == 0:
            assert tick["datagrams"] == 0  # two milliseconds early is not "< 2"
        if step == 1:
            assert tick["connections_sent"] >= 1 and 5 in codes.tolist()  # one millisecond early is
        nothing_sent += tick["datagrams"] == 0
    return nothing_sent + 1, hits


def test_time(engine):
    """300 connections at six frame rates from staggered bases, stepped through 12 values of now_ms that include the
    previous tick's next_due_ms - 2, - 1 and next_due_ms itself; then the same with a capacity that cuts every tick."""
    seen = set()
    roomy = sum(-(-F // m) for F, m, _ in _mixed_settings(300, 5)) * 2
    nothing_sent, hits = _time_run(engine, roomy, seen)
    assert nothing_sent >= 2 and hits == {-2, -1, 0}
    assert seen == {0, 1, 2, 4, 5}
    _time_run(engine, 40, seen)
    assert seen == {0, 1, 2, 3, 4, 5}


# ---- 5: edges on the chip --------------------------------------------------------------------------------------
def test_edges(engine):
    """A base at the top of its range with the longest stream at the fastest rate near its end; a want past 2^32 slots;
    ids beyond the table and entries that are finished or too wide for the stride, whose schedule entries are 0xFF
    bytes. (Codes 2 and 4 are decided before a schedule entry could matter, so the 0xFF entries pin that such a
    connection's code, the tick block and next_due_ms do not depend on them; that the kernels do not load them is read
    off ms_server_timed_want and the `skipped == 0` guard in ms_server_timed_apply, not off this test.)"""
    top = (1 << 62) - 1 - 5000
    settings = [(3000, 1400, U32_MAX),      # 0: fps 2^32 - 1 from `top`, three frames from its end
                (100, 60, U32_MAX),         # 1: the same stream, 1 ms earlier on its clock
                (U32_MAX, 53, 1000),        # 2: 81 million datagrams a frame: its 1 000 frames want far more than
                                            #    2^32 slots
                (100, 60, 9),               # 3: listed after it
                (3000, 1400, 5),            # 4: finished
                (3000, 1472, 5),            # 5: wider than the stride
                (27, 53, 5)]                # 6: not due yet
    entries = W.media_stream_server_entries(settings)
    entries["current_frame"][0] = entries["current_frame"][1] = U32_MAX - 2
    entries["finished"][4] = 1
    schedule = W.media_stream_server_schedule([(U32_MAX, top), (U32_MAX, top + 1), (1000, top), (1000, top), (1, 0),
                                               (1, 0), (1, top + 5000)])
    schedule.view(np.uint8).reshape(-1, 16)[4:6] = 0xFF
    now = top + 999  # d = 1000 = final x 1000 / fps for connection 0, 999 for connection 1
    pair = _Pair(engine, settings, schedule, 1408, 16, max_listed=9, entries=entries)
    assert 1000 * int(entries["datagrams_per_frame"][2]) > U32_MAX
    ids = [7, 4, 0, 5, 1, U32_MAX, 6, 2, 3]
    codes, tick = pair.tick(ids, now, U32_MAX, where="top")
    assert codes.tolist() == [4, 2, 1, 4, 0, 4, 5, 3, 3]
    assert tick["frames"] == 3 + 2 and tick["datagrams"] == 3 * 3 + 2 * 2 and tick["connections_no_room"] == 2
    assert int(pair.view.entries["current_frame"][0]) == 1 << 32
    assert int(pair.view.entries["current_frame"][1]) == U32_MAX
    assert tick["next_due_ms"] == top + 1  # connection 2's first frame, which no capacity of this ring holds
    ring = pair.table.ring.cpu().numpy()
    assert _sequence_numbers(ring, 1408, 13) == [U32_MAX - 2] * 3 + [U32_MAX - 1] * 3 + [U32_MAX] * 3 + \
        [U32_MAX - 2] * 2 + [U32_MAX - 1] * 2
    # one frame each: connection 1 ends, and connection 2's one frame still pushes connection 3 past the capacity
    codes, tick = pair.tick(ids, now + 1, 1, first_slot=0, where="one frame each")
    assert codes.tolist() == [4, 2, 2, 4, 1, 4, 5, 3, 3]


# ---- 6: downstream ---------------------------------------------------------------------------------------------
def test_multi_frame_tick_into_the_clients(engine):
    """The descriptors of one tick that carries three frames of every connection go through the clients' receive pass
    and accounting pass as they are, and every frame comes out successful."""
    n_conns, frames = 5, 3
    settings = [(3000, 1400, frames), (27, 53, frames), (1427, 1400, frames), (4300, 1400, frames),
                (2800, 1400, frames)]
    per_frame = [-(-F // m) for F, m, _ in settings]
    capacity, stride = frames * sum(per_frame), 1408
    servers = M.ServerTable(engine, settings, stride, capacity, fill=0xA5, schedule=[(30, 1000)] * n_conns)
    clients = M.ConnectionTable(engine, [(F, 4, final) for F, _, final in settings])
    ids = _ids(range(n_conns))
    status = torch.zeros(capacity * DGRAM_STATUS_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
    payload = engine.new_counters()
    servers.send_at(ids, 5000, 8, 1000, 10_000_000)
    n = capacity  # from the settings: nothing is read back between the send and the receive pass
    descs = servers.descs_of(n)
    clients.verify(servers.ring, descs, 0, status=status)
    clients.accumulate(servers.ring.numel(), descs, status, 0)
    engine.verify(servers.ring, descs, counters=payload)
    for _ in range(frames):
        clients.render(ids)
    block, results = engine.new_counters(), clients.new_results(n_conns)
    clients.close(ids, block, results=results)
    torch.cuda.synchronize()
    entries, codes, tick = servers.read_timed()
    assert codes[:n_conns].tolist() == [1] * n_conns and int(tick["frames"]) == frames * n_conns
    assert int(tick["datagrams"]) == n and int(tick["next_due_ms"]) == I64_MAX
    res = results.cpu().numpy().view(MS_CONN_RESULT_DTYPE)
    assert (res["status"] == 0).all() and (res["flags"] == 0).all() and (res["finished"] == 1).all()
    assert (res["successful_frames"] == frames).all()
    for f in ("dropped_frames", "duplicate_frames", "error_frames", "datagrams_after_end"):
        assert (res[f] == 0).all(), f
    assert np.array_equal(res["bits_received"], entries["bits_sent"])
    assert np.array_equal(res["datagrams"], entries["datagrams_sent"])
    got = engine.read_counters(payload)
    assert got["buffers_checked"] == n and got["buffers_failed"] == 0
    assert got["bytes_checked"] == got["bytes_ok"] == frames * sum(F - 26 * k for (F, _, _), k in zip(settings, per_frame))
