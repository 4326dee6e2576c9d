"""MediaStream servers on the device-resident path, host side (include/cts_media_stream_servers.h): the entry
initialiser, the closed form of the datagram split that the fill kernel computes, and the model that the GPU tests
compare against (ctstraffic_amd.workload.media_stream_server_view) held against the oracle's split, pattern bytes,
MediaStream verify and client."""
import ctypes
import struct

import numpy as np
import pytest

import oracle
from ctstraffic_amd import media_stream as ms
from ctstraffic_amd import workload as wl
from ctstraffic_amd._lib import CtsError, lib
from ctstraffic_amd.types import MS_SERVER_STATE_DTYPE, MS_SERVER_TICK_DTYPE
from oracle import media_stream as oms


def test_layouts():
    assert MS_SERVER_STATE_DTYPE.itemsize == 48 and MS_SERVER_TICK_DTYPE.itemsize == 32
    assert MS_SERVER_STATE_DTYPE.fields["frame_size_bytes"][1] == 32
    assert MS_SERVER_TICK_DTYPE.fields["datagrams"][1] == 8


def test_init_arithmetic():
    for F, M, n in [(27, 53, 1), (1400, 1400, 7), (1401, 1400, 1), (65536, 1472, 0xFFFFFFFF), (3 * 1400 + 13, 1400, 9)]:
        e = ms.server_init(F, M, n)
        assert (int(e["bits_sent"]), int(e["datagrams_sent"]), int(e["current_frame"]), int(e["finished"])) == \
            (0, 0, 1, 0)
        assert (int(e["final_frame"]), int(e["frame_size_bytes"]), int(e["datagram_max_size"])) == (n, F, M)
        assert int(e["datagrams_per_frame"]) == -(-F // M) == len(oms.split(F, M))
        assert e == wl.media_stream_server_entries([(F, M, n)])[0]


@pytest.mark.parametrize("F,M,n,fps", [
    (26, 1400, 5, 60),          # the reference FAIL_FASTs: no payload byte
    (0, 1400, 5, 60),
    (3000, 52, 5, 60),          # the device's own bound
    (3000, 0, 5, 60),
    (3000, 1400, 0, 60),
    (3000, 1400, -1, 60),
    (3000, 1400, 0x100000000, 60),
    (3000, 1400, 5, 0),
])
def test_init_refuses(F, M, n, fps):
    with pytest.raises(CtsError):
        ms.server_init(F, M, n, frames_per_second=fps)
    if fps != 0:
        with pytest.raises(ValueError):
            wl.media_stream_server_entries([(F, M, n)])


def test_init_null_arguments():
    s = ms.Settings(3000, 1400, 60, 0, 5)
    out = np.zeros(1, dtype=MS_SERVER_STATE_DTYPE)
    assert lib().cts_ms_server_init(None, out.ctypes.data) == -1
    assert lib().cts_ms_server_init(ctypes.addressof(s), None) == -1
    assert lib().cts_ms_server_init(ctypes.addressof(s), out.ctypes.data) == 0


def test_scratch_bytes_grow_with_n():
    b = [ms.servers_scratch_bytes(n) for n in (0, 1, 256, 257, 65536, 0xFFFFFFFF)]
    assert all(x % 8 == 0 for x in b) and b == sorted(b)
    assert b[1] >= 8 * 2 + 8 + 32 and b[-1] >= 8 * 0xFFFFFFFF


def test_closed_form_against_split():
    """The sweep of the issue: every M in 53..199 and F in 27..5M+39, against the library's iteration of
    UpdateBufferLength (and, on a coarser grid, the oracle's)."""
    L = lib()
    buf = np.zeros(16, dtype=np.uint32)
    for M in range(53, 200):
        for F in range(27, 5 * M + 40):
            k = int(L.cts_media_stream_split(F, M, buf.ctypes.data, 16))
            assert wl.media_stream_frame_lengths(F, M) == buf[:k].tolist(), (F, M)
    for M in (53, 54, 79, 80, 199, 1400, 1472):
        for F in list(range(27, 3 * M + 40, 7)) + [M - 1, M, M + 1, M + 26, M + 27, 2 * M, 2 * M + 13, 3 * M + 500]:
            if F > 26:
                assert wl.media_stream_frame_lengths(F, M) == oms.split(F, M), (F, M)


def _settings(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        M = int(rng.integers(53, 300))
        k = 1 + (c % 9)
        F = int(rng.integers((k - 1) * M + 1, k * M + 1))
        out.append((max(F, 27), M, 1 + int(rng.integers(0, 4))))
    return out


def test_model_against_one_frame_loop():
    """Several ticks of a shuffled list with finished connections, bad ids and a capacity that cuts the list, against
    a loop that sends one frame of one connection at a time with nothing shared but split() and the pattern."""
    settings = _settings(40, 1)
    stride, capacity, first_slot = 304, 120, 2
    entries = wl.media_stream_server_entries(settings)
    ring0 = np.full((first_slot + capacity) * stride, 0xA5, dtype=np.uint8)
    view = wl.media_stream_server_view(entries, stride, ring0, capacity)
    state = [dict(frame=1, bits=0, dgrams=0, finished=0) for _ in settings]
    ring = ring0.copy()
    P = np.array([oracle.pattern_byte(i) for i in range(stride)], dtype=np.uint8)
    rng = np.random.default_rng(2)
    for tick in range(6):
        ids = [int(x) for x in rng.permutation(len(settings))[:33]] + [40, 1000]
        rng.shuffle(ids)
        qpc, qpf = 0x0102030405060708 + tick, -0x1112131415161718
        codes, t = view.send(ids, qpc, qpf, first_slot=first_slot)
        slot, want_codes, sent = 0, [], 0
        for c in ids:
            if c >= len(settings):
                want_codes.append(4)
                continue
            F, M, final = settings[c]
            s = state[c]
            if s["finished"]:
                want_codes.append(2)
                continue
            lens = oms.split(F, M)
            mine, slot = slot, slot + len(lens)
            if mine + len(lens) > capacity:
                want_codes.append(3)
                continue
            for j, n in enumerate(lens):
                o = (first_slot + mine + j) * stride
                ring[o:o + 26] = np.frombuffer(struct.pack("<Hqqq", 0, s["frame"], qpc, qpf), dtype=np.uint8)
                ring[o + 26:o + n] = P[: n - 26]
                d = view.descs[mine + j]
                assert (int(d["byte_offset"]), int(d["length"]), int(d["expected_pattern_offset"]),
                        int(d["conn_index"]), int(d["skip_head"])) == (o, n, 0, c, 26)
                assert int(view.lengths[mine + j]) == n
            s["frame"] += 1
            s["bits"] += 8 * F
            s["dgrams"] += len(lens)
            s["finished"] = int(s["frame"] > final)
            want_codes.append(s["finished"])
            sent += len(lens)
        assert codes.tolist() == want_codes
        assert t["datagrams"] == sent and t["connections_sent"] == sum(c in (0, 1) for c in want_codes)
        assert t["connections_no_room"] == want_codes.count(3)
        assert t["connections_skipped"] == want_codes.count(2) + want_codes.count(4)
        assert t["connections_finished"] == want_codes.count(1)
        assert np.array_equal(view.ring, ring)
        for c, s in enumerate(state):
            e = view.entries[c]
            assert (int(e["current_frame"]), int(e["bits_sent"]), int(e["datagrams_sent"]), int(e["finished"])) == \
                (s["frame"], s["bits"], s["dgrams"], s["finished"])
    assert any(s["finished"] for s in state) and view.udp["bits_received"] == sum(s["bits"] for s in state)
    assert view.udp["datagrams"] == sum(s["dgrams"] for s in state)


def test_model_ring_against_oracle_verify():
    """The oracle's MediaStream receive over the model's ring: every datagram is DATA and clean, and carries its
    frame's sequence number and the tick's timestamps where the client reads them."""
    settings = [(27, 53, 2), (1399, 1400, 2), (1400, 1400, 2), (1401, 1400, 2), (1426, 1400, 2), (1427, 1400, 2),
                (2800, 1400, 2), (2813, 1400, 2), (4700, 1400, 2), (3 * 1472, 1472, 2)]
    stride, capacity = 1472, 64
    view = wl.media_stream_server_view(wl.media_stream_server_entries(settings), stride,
                                       np.full(capacity * stride, 0xA5, dtype=np.uint8), capacity)
    ids = list(range(len(settings)))
    for frame in (1, 2):
        qpc, qpf = 0x1122334455667788 * frame % (1 << 63), 10_000_000
        codes, t = view.send(ids, qpc, qpf)
        n = t["datagrams"]
        assert n == sum(len(oms.split(F, M)) for F, M, _ in settings) and set(codes.tolist()) == {frame - 1}
        descs = np.ascontiguousarray(view.descs[:n])
        recs, results, counters = oracle.media_stream_verify(view.ring, descs)
        assert (recs["kind"] == 0).all() and (recs["flag"] == 0).all() and results["pass"].all()
        assert (recs["sequence_number"] == frame).all()
        assert (recs["completed_bytes"] == descs["length"]).all()
        assert counters["bytes_ok"] == counters["bytes_checked"] == int(descs["length"].sum()) - 26 * n
        # the header carries qpc at +10 and qpf at +18
        for d in descs:
            o = int(d["byte_offset"])
            assert struct.unpack_from("<Hqqq", view.ring, o) == (0, frame, qpc, qpf)
        # per connection the frame's datagrams add up to the frame (its bytes include the headers)
        for c, (F, M, _) in enumerate(settings):
            mine = descs[descs["conn_index"] == c]
            assert int(mine["length"].sum()) == F
    assert (view.entries["finished"] == 1).all()


def test_model_stream_into_oracle_client():
    """A model server's whole stream into the oracle's client, a render tick after every frame: final_frame
    successful frames and nothing else."""
    for F, M, final, buffered in [(3000, 1400, 5, 2), (27, 53, 1, 1), (1427, 1400, 9, 3), (4 * 1472 + 5, 1472, 4, 8)]:
        capacity = 8
        view = wl.media_stream_server_view(wl.media_stream_server_entries([(F, M, final)]), 1472,
                                           np.zeros(capacity * 1472, dtype=np.uint8), capacity)
        client = oms.ClientModel(F, buffered, final)
        ticks = 0
        while True:
            codes, t = view.send([0], 1, 2)
            if codes[0] == 2:
                break
            ticks += 1
            descs = np.ascontiguousarray(view.descs[: t["datagrams"]])
            recs, results, _ = oracle.media_stream_verify(view.ring, descs)
            for r, v in zip(recs, results):
                assert client.complete(int(r["kind"]), int(r["sequence_number"]), int(r["completed_bytes"]),
                                       bool(v["pass"]))
            client.render()
        assert ticks == final
        while client.render() == 0:
            pass
        s = client.stats()
        assert s["finished"] == 1 and s["last_error"] == 0
        assert (s["successful_frames"], s["dropped_frames"], s["duplicate_frames"], s["error_frames"]) == \
            (final, 0, 0, 0)
        assert s["bits_received"] == int(view.entries["bits_sent"][0]) == 8 * F * final
