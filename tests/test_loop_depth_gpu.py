"""GPU: the fill, verify and MediaStream kernels past the first pass of their outer loops, byte for byte.

Every data-path kernel has an outer loop whose grid is capped at CUs x blocks-per-CU, so the small exact tests stay in
the first pass on a 256-CU device (tests/test_launch_depths_cpu.py shows it). Here every shape is a function of the
device's compute units, and tests/launch_depths.py -- the launchers' grid rules (ctstraffic_amd/csrc/cts_grids.hpp)
with the loops' depths on top -- must show that the launch reaches the later passes before anything is launched: the
`cur = nxt` hand-over and ragged last batch of fill_pieces_kernel, the consumed descriptor prefetch of fill_kernel,
QuadWalk::next() into a block's next chunk, the in-loop flush and reuse of the MediaStream receive's output ring, the
LDS refill of the batched fills. All comparisons are exact and complete: every arena byte (untouched neighbours and a
tail behind the arena included), every result, record, status, counter and slot, against the oracle.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import launch_depths as L
import oracle
from ctstraffic_amd import _lib
from ctstraffic_amd import media_stream as M
from ctstraffic_amd.types import (DESC_DTYPE, DGRAM_HEADER_DTYPE, DGRAM_RECORD_DTYPE, DGRAM_STATUS_DTYPE,
                                  RESULT_DTYPE)
from test_media_stream import _status_of
from test_verify_gpu import _random_case, assert_results_equal

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"
EMPTY = 0xFFFFFFFF
SENTINEL = 0xA5
TAIL = 64  # output elements allocated behind the launch's, which must keep the sentinel


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


@contextlib.contextmanager
def attrs(engine, **values):
    """Engine attributes by name (ATTR_<NAME>), put back afterwards."""
    ids = {k: getattr(_lib, "ATTR_" + k.upper()) for k in values}
    before = {k: engine.get_attr(i) for k, i in ids.items()}
    try:
        for k, v in values.items():
            engine.set_attr(ids[k], v)
        yield
    finally:
        for k, v in before.items():
            engine.set_attr(ids[k], v)


@pytest.fixture(scope="module")
def ring1_engine():
    """An engine whose ring-fill cap (read at creation only) is one workgroup per CU."""
    from ctstraffic_amd import Engine

    old = os.environ.get("CTS_RING_FILL_BLOCKS_PER_CU")
    os.environ["CTS_RING_FILL_BLOCKS_PER_CU"] = "1"
    try:
        eng = Engine(0)
    finally:
        if old is None:
            del os.environ["CTS_RING_FILL_BLOCKS_PER_CU"]
        else:
            os.environ["CTS_RING_FILL_BLOCKS_PER_CU"] = old
    yield eng
    eng.close()


def _same_bytes(got, exp, what):
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (what, int(bad.size), bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())


# ---- A. fill_pieces_kernel -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _piece_arena(kind, cus):
    descs, arena_bytes = L.piece_case(kind, cus)
    init = np.random.default_rng(len(descs)).integers(0, 256, size=arena_bytes + 32, dtype=np.uint8)
    exp = init.copy()
    oracle.fill(exp[:arena_bytes], descs)
    assert not np.array_equal(exp, init)
    return descs, arena_bytes, init, exp


@pytest.mark.parametrize("fill_nt", [0, 1])
@pytest.mark.parametrize("kind", L.PIECE_KINDS)
def test_piece_fill_past_the_first_batch(engine, kind, fill_nt):
    """64k: aligned 64 KiB buffers (whole chunks) among ragged ones, bad descriptors in every batch. 70000: nine pieces
    per buffer, buffers across the batches' seams. 1m: a hint far above the lengths, most pieces empty, two buffers
    longer than the hint (a whole-chunk tail and an edge-chunk tail in one workgroup each). 9000: two pieces per buffer,
    the second taking the rest."""
    cus = _cus()
    descs, arena_bytes, init, exp = _piece_arena(kind, cus)
    depth = L.piece_fill_depth(descs, L.PIECE_HINT[kind], cus, 1, arena_bytes)
    assert L.piece_reaches(kind, depth) == [], depth
    base = to_dev(init)
    assert base.data_ptr() % 16 == 0
    with attrs(engine, fill_blocks_per_cu=1, fill_nt=fill_nt):
        engine.fill(base[:arena_bytes], to_dev(descs), max_length_hint=L.PIECE_HINT[kind])
        torch.cuda.synchronize()
    _same_bytes(base.cpu().numpy(), exp, kind)


# ---- B. fill_kernel --------------------------------------------------------------------------------------------------
def _team_fill_case(n, max_len, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, size=n)
    gaps = rng.integers(0, 17, size=n)
    off = np.cumsum(gaps + lens) - lens
    descs = np.zeros(n, dtype=DESC_DTYPE)
    descs["byte_offset"], descs["length"] = off, lens
    descs["expected_pattern_offset"] = rng.integers(0, 65536, size=n)
    descs["skip_head"] = np.minimum(lens, rng.integers(0, 31, size=n))
    arena_bytes = int(off[-1] + lens[-1])
    bad = rng.choice(n, size=max(8, n // 40), replace=False)  # scattered through every pass
    for k, i in enumerate(bad):
        if k % 3 == 0:
            descs[i]["expected_pattern_offset"] = 65536 + k
        elif k % 3 == 1:
            descs[i]["skip_head"] = int(descs[i]["length"]) + 1
        else:
            descs[i]["byte_offset"] = arena_bytes - 3
            descs[i]["length"] = 64 + k
    init = rng.integers(0, 256, size=arena_bytes + 32, dtype=np.uint8)
    exp = init.copy()
    oracle.fill(exp[:arena_bytes], descs)
    return descs, arena_bytes, init, exp


@pytest.mark.parametrize("fill_nt", [0, 1])
@pytest.mark.parametrize("hint,lanes,max_len", [(1472, 64, 1500), (8192, 64, 9000), (0, 256, 70000)])
def test_team_fill_takes_its_prefetched_descriptor(engine, hint, lanes, max_len, fill_nt):
    """fill_kernel<64> (hints up to 8192) and fill_kernel<kBlock> (hint 0) at one workgroup per CU: every team fills
    three buffers and most a fourth, each from the descriptor the pass before loaded."""
    cus = _cus()
    n = L.team_fill_n(lanes, cus)
    depth = L.team_fill_depth(n, lanes, cus, 1)
    assert L.team_fill_reaches(depth) == [], depth
    descs, arena_bytes, init, exp = _team_fill_case(n, max_len, hint + lanes)
    base = to_dev(init)
    with attrs(engine, small_blocks_per_cu=1, fill_blocks_per_cu=1, fill_nt=fill_nt):
        engine.fill(base[:arena_bytes], to_dev(descs), max_length_hint=hint)
        torch.cuda.synchronize()
    _same_bytes(base.cpu().numpy(), exp, (hint, lanes))


# ---- C. verify_quad_kernel -------------------------------------------------------------------------------------------
N_CONNS = 7
BASE_INDEX = 1000003


@functools.lru_cache(maxsize=None)
def _quad_case(n):
    rng = np.random.default_rng(n)
    arena, descs = _random_case(rng, n, 3000, corrupt_frac=0.2, skip=True)
    for k, i in enumerate(rng.choice(n, size=n // 50, replace=False)):  # bad descriptors in every chunk's reach
        if k % 3 == 0:
            descs[i]["expected_pattern_offset"] = 65536
        elif k % 3 == 1:
            descs[i]["skip_head"] = int(descs[i]["length"]) + 1
        else:
            descs[i]["byte_offset"] = arena.size - 1
            descs[i]["length"] = 2
    return arena, descs, oracle.verify_batch(arena, descs, n_conns=N_CONNS)


def _run_quad(engine, n, launch, exp, what):
    """launch(results, counters, slots); everything it wrote against exp = (results, counters, slots)."""
    res = torch.full(((n + TAIL) * RESULT_DTYPE.itemsize,), SENTINEL, dtype=torch.uint8, device=DEV)
    ctr = engine.new_counters()
    cff = torch.full((N_CONNS + TAIL,), -1, dtype=torch.int32, device=DEV)
    launch(res[:n * RESULT_DTYPE.itemsize], ctr, cff[:N_CONNS])
    torch.cuda.synchronize()
    got = res.cpu().numpy()
    assert_results_equal(got[:n * RESULT_DTYPE.itemsize].view(RESULT_DTYPE), exp[0], what)
    assert (got[n * RESULT_DTYPE.itemsize:] == SENTINEL).all(), what
    assert engine.read_counters(ctr) == exp[1], what
    slots = cff.cpu().numpy().view(np.uint32)
    assert np.array_equal(slots[:N_CONNS], exp[2]) and (slots[N_CONNS:] == EMPTY).all(), what


@pytest.mark.parametrize("nt", [1, 0])
def test_quad_verify_walks_rounds_and_chunks(engine, nt):
    """verify_quad_kernel at one workgroup per CU: four rounds per wave in one chunk (chunk 0), four chunks of one round
    (16), two chunks of three rounds (48); buffers up to 3000 bytes under hint 1472 (multi-round teams), corrupt ones,
    bad descriptors, seven connections' first failures; cts_verify and cts_verify_at."""
    cus = _cus()
    n = L.quad_n(cus)
    for chunk in L.QUAD_CHUNKS:
        depth = L.quad_walk_depth(n, cus, 1, chunk)
        assert L.quad_reaches(chunk, depth) == [], (chunk, depth)
    arena, descs, (er, ectr, ecff) = _quad_case(n)
    assert (ecff != EMPTY).all() and ectr["buffers_failed"] > n // 10
    a, d = to_dev(arena), to_dev(descs)
    ecff_at = np.where(ecff == EMPTY, EMPTY, ecff + np.uint32(BASE_INDEX)).astype(np.uint32)
    for chunk in L.QUAD_CHUNKS:
        with attrs(engine, small_blocks_per_cu=1, small_chunk=chunk, nt_loads=nt):
            _run_quad(engine, n, lambda r, c, s: engine.verify(a, d, max_length_hint=1472, results=r, counters=c,
                                                              conn_first_fail=s), (er, ectr, ecff), ("verify", chunk))
            _run_quad(engine, n, lambda r, c, s: engine.verify(a, d, max_length_hint=1472, results=r, counters=c,
                                                              conn_first_fail=s, base_index=BASE_INDEX),
                      (er, ectr, ecff_at), ("verify_at", chunk))


@functools.lru_cache(maxsize=None)
def _strided_case(n, stride, skip):
    rng = np.random.default_rng(n + stride)
    lens = rng.integers(0, stride + 1, size=n).astype(np.uint32)
    lens[rng.random(n) < 0.3] = stride
    long_ = rng.choice(n, size=n // 60, replace=False)
    lens[long_] = stride + 1 + rng.integers(0, 64, size=long_.size)
    descs = np.zeros(n, dtype=DESC_DTYPE)
    descs["byte_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    descs["length"], descs["skip_head"], descs["conn_index"] = lens, skip, 3
    descs["expected_pattern_offset"][long_] = 65536  # a completion longer than its slot: flagged, not read
    ring = np.full(n * stride + 64, 0xEE, dtype=np.uint8)
    fillable = descs.copy()
    fillable["length"] = np.minimum(lens, stride)
    fillable["expected_pattern_offset"] = 0
    oracle.fill(ring, fillable)
    ok = np.nonzero((lens > skip) & (lens <= stride))[0]
    hit = ok[rng.random(ok.size) < 0.1]
    pos = hit.astype(np.int64) * stride + skip + (rng.random(hit.size) * (lens[hit] - skip)).astype(np.int64)
    ring[pos] ^= rng.integers(1, 256, size=hit.size, dtype=np.uint8)
    return ring, lens, oracle.verify_batch(ring, descs, n_conns=N_CONNS)


@pytest.mark.parametrize("nt", [1, 0])
def test_quad_verify_strided_walks_rounds_and_chunks(engine, nt):
    """cts_verify_strided and _at over a ring of stride 1536, skip 26, under the same three walks; completions above
    the stride among them."""
    cus = _cus()
    n, stride, skip = L.quad_n(cus), 1536, 26
    for chunk in L.QUAD_CHUNKS:
        assert L.quad_reaches(chunk, L.quad_walk_depth(n, cus, 1, chunk)) == [], chunk
    ring, lens, (er, ectr, ecff) = _strided_case(n, stride, skip)
    assert ectr["buffers_failed"] > n // 20 and int((er["flags"] == 1).sum()) >= n // 60 and ecff[3] != EMPTY
    a, ld = to_dev(ring), to_dev(lens)
    ecff_at = np.where(ecff == EMPTY, EMPTY, ecff + np.uint32(BASE_INDEX)).astype(np.uint32)
    for chunk in L.QUAD_CHUNKS:
        with attrs(engine, small_blocks_per_cu=1, small_chunk=chunk, nt_loads=nt):
            for base, slots in ((0, ecff), (BASE_INDEX, ecff_at)):
                _run_quad(engine, n, lambda r, c, s: engine.verify_strided(
                    a, stride, ld, skip_head=skip, expected_offset=0, conn_index=3, results=r, counters=c,
                    conn_first_fail=s, base_index=base), (er, ectr, slots), ("strided", chunk, base))


# ---- D. the MediaStream receive's output ring ------------------------------------------------------------------------
CRAFTED = [b"\x00\x10" + b"x" * 37,    # id
           b"\x00\x10" + b"x" * 10,    # id, too short
           b"\x00\x00" + b"\x01" * 10,  # data, too short
           b"\x34\x12" + b"\x00" * 40,  # unknown flag
           b"", b"\x00"]               # zero bytes, one byte


def _datagrams(n, seed, stride=0):
    """n datagrams of 26 to 300 bytes with random 64-bit header fields, one in ten corrupt, the crafted kinds and a few
    descriptors outside the arena mixed in; packed from an odd offset, or (stride) one per ring slot.
    Returns (arena, descs)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(26, 301, size=n)
    lens[rng.random(n) < 0.02] = 26  # a header and no payload
    craft = np.nonzero(rng.random(n) < 0.05)[0]
    which = rng.integers(0, len(CRAFTED), size=craft.size)
    lens[craft] = [len(CRAFTED[k]) for k in which]
    if stride:
        off = np.arange(n, dtype=np.int64) * stride
        size = n * stride + 64
    else:
        off = 3 + np.cumsum(lens) - lens
        size = int(off[-1] + lens[-1]) + 64
    descs = np.zeros(n, dtype=DESC_DTYPE)
    descs["byte_offset"], descs["length"], descs["skip_head"] = off, lens, 26
    descs["conn_index"] = rng.integers(0, N_CONNS + 1, size=n)  # one index beyond the slots
    arena = np.full(size, 0xEE, dtype=np.uint8)
    oracle.fill(arena, descs)  # the payloads: P[0 .. length - 26)
    descs["skip_head"] = 0
    data = np.ones(n, dtype=bool)
    data[craft] = False
    data &= lens >= 26
    hdr = np.zeros(n, dtype=DGRAM_HEADER_DTYPE)
    hdr["sequence_number"] = rng.integers(-9, 1 << 40, size=n)
    hdr["qpc"], hdr["qpf"] = rng.integers(-(1 << 62), 1 << 62, size=n), rng.integers(0, 1 << 62, size=n)
    hb = np.zeros((n, 26), dtype=np.uint8)
    hb[:, 2:] = hdr.view(np.uint8).reshape(n, 24)
    at = off[data, None] + np.arange(26)[None, :]
    arena[at.reshape(-1)] = hb[data].reshape(-1)
    for i, k in zip(craft.tolist(), which.tolist()):
        arena[off[i]:off[i] + len(CRAFTED[k])] = np.frombuffer(CRAFTED[k], dtype=np.uint8)
    hit = np.nonzero(data & (lens > 26) & (rng.random(n) < 0.1))[0]
    pos = off[hit] + 26 + (rng.random(hit.size) * (lens[hit] - 26)).astype(np.int64)
    arena[pos] ^= rng.integers(1, 256, size=hit.size, dtype=np.uint8)
    if not stride:
        out = rng.choice(n, size=max(3, n // 500), replace=False)
        descs["byte_offset"][out[0::2]] = size + 1000
        descs["byte_offset"][out[1::2]] = size - 5
        descs["length"][out[1::2]] = 100
    return arena, descs


def _expected_slots(descs, recs, res, base):
    """The first-failure slots after cts_media_stream_verify_status_at: per connection the lowest base + i over the
    datagrams that fail their stream (anything but clean DATA and ID)."""
    fails = np.where(recs["kind"] == 0, res["pass"] == 0, recs["kind"] != 1)
    slots = np.full(N_CONNS, EMPTY, dtype=np.uint32)
    idx = np.nonzero(fails & (descs["conn_index"] < N_CONNS))[0]
    np.minimum.at(slots, descs["conn_index"][idx], (base + idx).astype(np.uint32))
    return slots


def _out(n, itemsize):
    return torch.full(((n + TAIL) * itemsize,), SENTINEL, dtype=torch.uint8, device=DEV)


def _same_fields(buf, n, dtype, exp, what):
    got = buf.cpu().numpy()
    assert (got[n * dtype.itemsize:] == SENTINEL).all(), (what, "tail")
    got = got[:n * dtype.itemsize].view(dtype)
    for f in dtype.names:
        bad = np.nonzero(got[f] != exp[f])[0]
        assert bad.size == 0, (what, f, int(bad.size), bad[:6].tolist(), got[f][bad[:6]].tolist(),
                               exp[f][bad[:6]].tolist())


def _status_at(engine, a, d, n, base, status, counters, slots):
    from ctstraffic_amd.engine import _ptr
    from ctstraffic_amd._lib import check

    check("cts_media_stream_verify_status_at",
          engine._L.cts_media_stream_verify_status_at(engine._h, _ptr(a), a.numel(), _ptr(d), n, base, _ptr(status),
                                                      _ptr(counters), _ptr(slots), N_CONNS, None))


def _receive_forms(engine, arena, descs, forms, what):
    n = len(descs)
    er, eres, ectr = oracle.media_stream_verify(arena, descs)
    assert set(er["kind"].tolist()) == {0, 1, 2, 3, 4, 5} and ectr["buffers_failed"] > n // 20
    es = _status_of(er, eres)
    a, d = to_dev(arena), to_dev(descs)
    if "records" in forms:
        recs, res, ctr = _out(n, 32), _out(n, 12), engine.new_counters()
        M.verify(engine, a, d, records=recs[:n * 32], results=res[:n * 12], counters=ctr)
        torch.cuda.synchronize()
        _same_fields(recs, n, DGRAM_RECORD_DTYPE, er, (what, "records"))
        _same_fields(res, n, RESULT_DTYPE, eres, (what, "results"))
        assert engine.read_counters(ctr) == ectr, what
    if "status" in forms:
        st, ctr = _out(n, 16), engine.new_counters()
        M.verify_status(engine, a, d, status=st[:n * 16], counters=ctr)
        torch.cuda.synchronize()
        _same_fields(st, n, DGRAM_STATUS_DTYPE, es, (what, "status"))
        assert engine.read_counters(ctr) == ectr, what
    if "status_at" in forms:
        st, ctr = _out(n, 16), engine.new_counters()
        slots = torch.full((N_CONNS + TAIL,), -1, dtype=torch.int32, device=DEV)
        _status_at(engine, a, d, n, BASE_INDEX, st[:n * 16], ctr, slots)
        torch.cuda.synchronize()
        _same_fields(st, n, DGRAM_STATUS_DTYPE, es, (what, "status_at"))
        assert engine.read_counters(ctr) == ectr, what
        got = slots.cpu().numpy().view(np.uint32)
        exp = _expected_slots(descs, er, eres, BASE_INDEX)
        assert (exp != EMPTY).all() and np.array_equal(got[:N_CONNS], exp) and (got[N_CONNS:] == EMPTY).all(), what


def test_receive_ring_wraps(engine):
    """Chunks of 133 rounds: three blocks whose waves flush the ring of 64 twice inside the loop and then five rounds
    more, a last block with five rounds only. All five forms of the receive."""
    cus = _cus()
    n = L.ring_n("d1", cus)
    depth = L.quad_walk_depth(n, cus, engine.get_attr(_lib.ATTR_SMALL_BLOCKS_PER_CU), L.RING_CHUNK_D1)
    assert L.ring_reaches("d1", depth) == [], depth
    arena, descs = _datagrams(n, 0xD1)
    with attrs(engine, small_chunk=L.RING_CHUNK_D1):
        _receive_forms(engine, arena, descs, ("records", "status", "status_at"), "d1")
        stride = 304
        ring, rdescs = _datagrams(n, 0xD15, stride=stride)
        er, eres, ectr = oracle.media_stream_verify(ring, rdescs)
        a, ld = to_dev(ring), to_dev(rdescs["length"].astype(np.uint32))
        recs, res, ctr = _out(n, 32), _out(n, 12), engine.new_counters()
        M.verify_strided(engine, a, stride, ld, records=recs[:n * 32], results=res[:n * 12], counters=ctr)
        st, ctr2 = _out(n, 16), engine.new_counters()
        M.verify_strided_status(engine, a, stride, ld, status=st[:n * 16], counters=ctr2)
        torch.cuda.synchronize()
        _same_fields(recs, n, DGRAM_RECORD_DTYPE, er, "strided records")
        _same_fields(res, n, RESULT_DTYPE, eres, "strided results")
        _same_fields(st, n, DGRAM_STATUS_DTYPE, _status_of(er, eres), "strided status")
        assert engine.read_counters(ctr) == ectr and engine.read_counters(ctr2) == ectr


def test_receive_ring_holds_rounds_of_several_chunks(engine):
    """One workgroup per CU and chunks of three rounds, 22 chunks and more per block: a wave's 64th round is a chunk's
    first, and the ring it flushes holds the rounds of 22 chunks that lie a grid apart."""
    cus = _cus()
    n = L.ring_n("d2", cus)
    depth = L.quad_walk_depth(n, cus, 1, 48)
    assert L.ring_reaches("d2", depth) == [], depth
    arena, descs = _datagrams(n, 0xD2)
    with attrs(engine, small_blocks_per_cu=1, small_chunk=48):
        _receive_forms(engine, arena, descs, ("records", "status_at"), "d2")


# ---- E. cts_media_stream_fill ----------------------------------------------------------------------------------------
def _fill_expected(arena, descs, hdrs):
    """What the MediaStream fills write: per datagram of 26 bytes and more that lies inside the arena the header
    {u16 0, i64 seq, i64 qpc, i64 qpf} and P[0 .. length - 26); nothing else."""
    d = descs.copy()
    d["skip_head"], d["expected_pattern_offset"] = 26, 0
    oracle.fill(arena, d)
    off, ln = d["byte_offset"].astype(np.int64), d["length"].astype(np.int64)
    ok = (ln >= 26) & (off + ln <= arena.size)
    hb = np.zeros((len(d), 26), dtype=np.uint8)
    hb[:, 2:] = hdrs.view(np.uint8).reshape(len(d), 24)
    arena[(off[ok, None] + np.arange(26)[None, :]).reshape(-1)] = hb[ok].reshape(-1)


def _headers(rng, n):
    hdrs = np.zeros(n, dtype=DGRAM_HEADER_DTYPE)
    for f in ("sequence_number", "qpc", "qpf"):
        hdrs[f] = rng.integers(-(1 << 62), 1 << 62, size=n)
    return hdrs


def test_batched_fill_refills_its_stage(ring1_engine):
    """cts_media_stream_fill at one workgroup per CU: every workgroup stages three batches, the last of 19 datagrams
    (four for its last wave). Datagrams of 26 to 200 bytes, two in three on 16-byte boundaries, sentinel gaps, lengths
    below 26 and descriptors past the arena among them; plain and nontemporal stores."""
    eng, cus = ring1_engine, _cus()
    n = L.batched_n("descs", cus)
    depth = L.batch_fill_depth(n, L.FILL_BATCH, cus, 1)
    assert L.batched_reaches("descs", depth) == [], depth
    rng = np.random.default_rng(0xE)
    lens = rng.integers(26, 201, size=n)
    short = rng.random(n) < 0.02
    lens[short] = rng.integers(0, 26, size=int(short.sum()))
    mis = np.where(np.arange(n) % 3 == 0, rng.integers(1, 16, size=n), 0)
    room = (mis + lens + rng.integers(0, 5, size=n) + 15) // 16 * 16 + 16 * rng.integers(0, 3, size=n)
    off = np.cumsum(room) - room + mis
    descs = np.zeros(n, dtype=DESC_DTYPE)
    descs["byte_offset"], descs["length"] = off, lens
    arena_bytes = int(room.sum())
    out = rng.choice(n, size=n // 100, replace=False)
    descs["byte_offset"][out[0::2]] = arena_bytes + 16
    descs["byte_offset"][out[1::2]] = arena_bytes - 20
    descs["length"][out[1::2]] = 40
    hdrs = _headers(rng, n)
    init = rng.integers(0, 256, size=arena_bytes + 32, dtype=np.uint8)
    exp = init.copy()
    _fill_expected(exp[:arena_bytes], descs, hdrs)
    d, h = to_dev(descs), to_dev(hdrs)
    for fill_nt in (0, 1):
        base = to_dev(init)
        with attrs(eng, fill_nt=fill_nt):
            M.fill(eng, base[:arena_bytes], d, h)
            torch.cuda.synchronize()
        _same_bytes(base.cpu().numpy(), exp, fill_nt)


# ---- F. cts_media_stream_fill_strided --------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,kind", [(64, "ring64"), (1040, "ring1040")])
def test_ring_fill_refills_its_stage(ring1_engine, stride, kind):
    """cts_media_stream_fill_strided at one workgroup per CU: three batches of the per-lane form (stride 64), two of
    the wave-uniform form (stride 1040, 65 chunks per slot: rounds cross datagram boundaries in the second batch, whose
    first ring chunk is not 0). Full slots, 26 bytes, below 26, above the stride; the arena ends 5 bytes short of its
    last slot, so the slots wholly inside it end in the last batch."""
    eng, cus = ring1_engine, _cus()
    n = L.batched_n(kind, cus)
    depth = L.batch_fill_depth(n, L.RING_BATCH, cus, 1, stride)
    assert L.batched_reaches(kind, depth) == [], depth
    rng = np.random.default_rng(stride)
    lens = np.full(n, stride, dtype=np.uint32)
    pick = rng.random(n)
    lens[pick < 0.3] = rng.integers(26, stride + 1, size=int((pick < 0.3).sum()))
    lens[(pick >= 0.3) & (pick < 0.35)] = 26
    lens[(pick >= 0.35) & (pick < 0.38)] = rng.integers(0, 26, size=int(((pick >= 0.35) & (pick < 0.38)).sum()))
    lens[(pick >= 0.38) & (pick < 0.40)] = stride + 1 + rng.integers(0, 64, size=int(((pick >= 0.38) & (pick < 0.40)).sum()))
    lens[-3:] = stride  # the last slot does not fit the arena any more, the two before it do
    arena_bytes = n * stride - 5
    hdrs = _headers(rng, n)
    init = rng.integers(0, 256, size=arena_bytes, dtype=np.uint8)
    exp = init.copy()
    descs = np.zeros(n, dtype=DESC_DTYPE)
    descs["byte_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    descs["length"] = lens
    over = lens > stride
    descs["length"][over] = 0  # above the stride: not written
    _fill_expected(exp, descs, hdrs)
    assert np.array_equal(exp[-(stride - 5):], init[-(stride - 5):]) and not np.array_equal(exp, init)
    ld, h = to_dev(lens), to_dev(hdrs)
    for fill_nt in (0, 1):
        a = to_dev(init)
        with attrs(eng, fill_nt=fill_nt):
            M.fill_strided(eng, a, stride, ld, h)
            torch.cuda.synchronize()
        _same_bytes(a.cpu().numpy(), exp, (stride, fill_nt))
