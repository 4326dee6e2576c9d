"""GPU: single-byte corruptions swept through every chunk role of the verifiers, exact against the oracle.

The verify kernels give the 16-byte chunks of a span different roles: byte-masked edge chunks, head chunks, the lanes of
full and of tail rounds, the exact re-read's own ownership rule, reductions over waves or team lanes, the mailbox's
4 KiB pieces. The other GPU tests place their corruptions at random, so a bug confined to one role (a tail predicate off by
one, a head chunk nobody owns, a wave's minimum lost, a wrong byte mask for one (lo, hi)) can pass them all. Here the
plans of tests/corruption_sweeps.py put one flipped bit at every byte of spans shaped from the kernels' constants -- one
buffer per position, among clean copies, shuffled -- plus pairs of flips at the roles' landmarks and buffers filled with
a shifted pattern, and every launch must give the oracle's exact outputs: every result field, the six counters, the
seven first-failure slots, and a sentinel tail behind the results. tests/test_corruption_sweeps_cpu.py shows that the
plans cover every role and that a verifier wrong in any one of them would fail here.
"""
import functools

import numpy as np
import pytest

import corruption_sweeps as S
import oracle
from ctstraffic_amd import media_stream as M
from ctstraffic_amd.types import DGRAM_RECORD_DTYPE, DGRAM_STATUS_DTYPE, RESULT_DTYPE
from test_loop_depth_gpu import BASE_INDEX, SENTINEL, TAIL, _out, _same_fields, attrs, to_dev
from test_media_stream import _status_of
from test_verify_gpu import assert_results_equal, host_path  # noqa: F401  (host_path: the fixture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"
RES = RESULT_DTYPE.itemsize


@pytest.fixture(scope="module", autouse=True)
def _release_arenas():
    """The plans (about 1.3 GB on the host and as much on the device) go when the module is done."""
    yield
    for cached in (_case, _ms_case, S.wg_plan, S.quad_plan, S.small_sweep, S.ms_plan):
        cached.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _case(path, name):
    """(plan, the oracle's (results, counters with connections_failed, slots), the arena and the descriptors -- for a
    ring the lengths -- on the device), built and uploaded once."""
    plan = S.wg_plan(name) if path == "wg" else S.quad_plan(name)
    er, ectr, ecff = oracle.verify_batch(plan.arena, plan.descs, n_conns=S.N_CONNS)
    ectr = dict(ectr, connections_failed=int(np.count_nonzero(ecff != S.EMPTY)))
    a = to_dev(plan.arena)
    assert a.data_ptr() % 128 == 0  # the plans' "start mod 128" is the address
    meta = to_dev(plan.descs) if plan.strided is None else to_dev(plan.descs["length"].astype(np.uint32))
    return plan, (er, ectr, ecff), a, meta


def _run(engine, n, launch, exp, base, what):
    """launch(results, counters, slots); everything it wrote against the oracle's exp = (results, counters, slots)."""
    res = torch.full(((n + TAIL) * RES,), SENTINEL, dtype=torch.uint8, device=DEV)
    ctr = engine.new_counters()
    cff = torch.full((S.N_CONNS + TAIL,), -1, dtype=torch.int32, device=DEV)
    launch(res[:n * RES], ctr, cff[:S.N_CONNS])
    torch.cuda.synchronize()
    got = res.cpu().numpy()
    assert_results_equal(got[:n * RES].view(RESULT_DTYPE), exp[0], what)
    assert (got[n * RES:] == SENTINEL).all(), what
    assert engine.read_counters_ex(ctr) == exp[1], what
    slots = cff.cpu().numpy().view(np.uint32)
    want = np.where(exp[2] == S.EMPTY, S.EMPTY, exp[2] + np.uint32(base)).astype(np.uint32)
    assert np.array_equal(slots[:S.N_CONNS], want) and (slots[S.N_CONNS:] == S.EMPTY).all(), what


# ---- a. the workgroup path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("name", S.WG_PLANS)
def test_workgroup_path(engine, name, nt):
    """verify_wg_kernel and verify_wg_ordinal (hint 0; cts_verify and cts_verify_at). small: every byte of every start
    0..127 at the degenerate chunk counts. ragged_*: scan_buffer and scan_exact_owned over edge, head, a full round
    and a partial tail round, odd and even byte phase, the 64 KiB wrap in the full and in the tail round. whole_*:
    scan_whole_exact likewise. prod: the 64 KiB buffer's eight full rounds at lanes 0, 63, 64 and 255. pairs_*: two
    dirty lanes, the minimum in any wave (block_reduce_mismatch). shifted_*: every lane dirty."""
    plan, exp, a, d = _case("wg", name)
    n = len(plan.descs)
    with attrs(engine, nt_loads=nt):
        for base in (0, BASE_INDEX):
            _run(engine, n, lambda r, c, s: engine.verify(a, d, max_length_hint=0, results=r, counters=c,
                                                          conn_first_fail=s, base_index=base), exp, base,
                 (name, nt, base))


# ---- b. the quad path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("name", S.QUAD_PLANS)
def test_quad_path(engine, name, nt):
    """verify_quad_kernel (hint 1472) over descriptors and (ring_*) strided rings; cts_verify / cts_verify_strided and
    their _at forms. small: the degenerate chunk counts at every cs. a: a 1472-byte datagram buffer past its header,
    one round. b, ring_b: 3000 bytes, all eight bits of every byte, two to three rounds from a negative first chunk.
    pairs: the minimum in any team lane (quad_team_reduce). shifted: every lane dirty."""
    plan, exp, a, meta = _case("quad", name)
    n = len(plan.descs)
    with attrs(engine, nt_loads=nt):
        for base in (0, BASE_INDEX):
            if plan.strided is None:
                def launch(r, c, s):
                    engine.verify(a, meta, max_length_hint=1472, results=r, counters=c, conn_first_fail=s,
                                  base_index=base)
            else:
                stride, skip, e, conn = plan.strided

                def launch(r, c, s):
                    engine.verify_strided(a, stride, meta, skip_head=skip, expected_offset=e, conn_index=conn,
                                          results=r, counters=c, conn_first_fail=s, base_index=base)
            _run(engine, n, launch, exp, base, (name, nt, base))


# ---- c. the host paths -----------------------------------------------------------------------------------------------
FIELDS = ("pass", "first_mismatch", "expected", "actual", "mismatch_bytes")


def _host_verify(engine, mailbox, arr, dev, at, n, e):
    """One buffer arr[at : at + n] of a pinned arena: through the mailbox in place (cts_verify_mapped), or through
    cts_verify_host's sliced launch. Returns (got, the oracle's)."""
    r = engine.verify_mapped(dev + at, n, e) if mailbox else engine.verify_host(arr[at:at + n], e)
    o = oracle.verify_buffer(arr[at:at + n].copy(), 0, e, n)
    return tuple(r[f] for f in FIELDS), tuple(o[f] for f in FIELDS)


def test_host_buffer_roles(host_path):
    """A 70 000-byte buffer at offset 5 of a pinned arena, odd expected offset, one call per corruption: every byte of
    chunk 0, of the last chunk, of both chunks at the piece seams 0|1, 3|4, 4|5, 15|16 and 16|17 (the next workgroup,
    the workgroup's next piece in flight, the next loop pass), of a chunk per data wave; every 37th byte; pairs across
    pieces, workgroups and passes. The mailbox folds through LDS atomics, part records and the host; the sliced launch
    through 64 descriptors and slice_merge."""
    from ctstraffic_amd import _lib

    engine = host_path
    mailbox = engine.get_attr(_lib.ATTR_SYNC_MAILBOX) == 1
    cases = S.mail_cases()
    assert len(cases) <= 6000
    arr, h, dev = engine.host_alloc(S.MAIL_LENGTH + 64)
    try:
        assert dev % 16 == 0
        at, n, e = S.MAIL_OFFSET, S.MAIL_LENGTH, S.MAIL_E
        arr[:] = S.GAP
        arr[at:at + n] = S.pattern(e + np.arange(n))
        got, want = _host_verify(engine, mailbox, arr, dev, at, n, e)
        assert got == want == (True, n, 0, 0, 0)
        for case in cases:
            for p, x in case:
                arr[at + p] ^= x
            got, want = _host_verify(engine, mailbox, arr, dev, at, n, e)
            for p, x in case:
                arr[at + p] ^= x
            assert got == want and want[1] == case[0][0] and want[4] == len(case), (case, got, want)
        got, want = _host_verify(engine, mailbox, arr, dev, at, n, e)
        assert got == want == (True, n, 0, 0, 0)
    finally:
        engine.host_free(h)


def test_host_buffer_small_lengths(host_path):
    """Lengths 1, 2, 15, 16, 17, 31, 32 and 33 at every offset 0..15 of a pinned arena (one chunk under both masks, two
    and three chunks), every byte corrupted, one call each. cts_verify_host stages its buffer at offset 0, so the
    sliced launch sees the offsets only as different bytes."""
    from ctstraffic_amd import _lib

    engine = host_path
    mailbox = engine.get_attr(_lib.ATTR_SYNC_MAILBOX) == 1
    cases = S.small_mail_cases()
    assert len(cases) <= 6000
    arr, h, dev = engine.host_alloc(128)
    try:
        assert dev % 16 == 0
        for lo, n, p in cases:
            e = (65536 - 7 + 5 * lo + n) & 0xFFFF  # the period wraps inside many of them
            if p == 0:
                arr[:] = S.GAP
                arr[lo:lo + n] = S.pattern(e + np.arange(n))
                got, want = _host_verify(engine, mailbox, arr, dev, lo, n, e)
                assert got == want == (True, n, 0, 0, 0), (lo, n)
            arr[lo + p] ^= 1 << int(S.sweep_bit(p + lo))
            got, want = _host_verify(engine, mailbox, arr, dev, lo, n, e)
            arr[lo + p] ^= 1 << int(S.sweep_bit(p + lo))
            assert got == want and want[:2] == (False, p) and want[4] == 1, (lo, n, p, got, want)
    finally:
        engine.host_free(h)


# ---- d. the MediaStream receive --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ms_case(strided):
    plan = S.ms_plan(strided)
    er, eres, ectr = oracle.media_stream_verify(plan.arena, plan.descs)
    a = to_dev(plan.arena)
    assert a.data_ptr() % 128 == 0
    meta = to_dev(plan.lengths) if strided else to_dev(plan.descs)
    return plan, (er, eres, ectr), a, meta


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("strided", [False, True], ids=["descs", "ring"])
def test_media_stream_receive(engine, strided, nt):
    """A 1472-byte datagram at every offset ho 0..15 (the ring: at every address mod 128) with each of its 1446 payload
    bytes corrupted, one datagram each; the same for 27, 41, 42 and 58 completed bytes; each bit of the flag bytes
    flipped (the kind must be the oracle's: an ID datagram, too short a one, an unknown flag); each bit of header bytes
    2..25 flipped (the record's fields change, the verdict does not). Records and results, the statuses, and the
    frames form's totals and counters, each against the oracle's per-datagram outputs."""
    plan, (er, eres, ectr), a, meta = _ms_case(strided)
    n = len(plan.descs)
    es = _status_of(er, eres)
    window = M.FrameWindow(S.MS_WINDOW[0], S.MS_WINDOW[1], S.MS_WINDOW[2], 0)
    esums, efb = S.ms_frame_sums(er, eres)
    assert esums["exceptions"] > n // 2 and ectr["mismatched_bytes"] == int((plan.flip_at >= S.HEADER).sum())
    with attrs(engine, nt_loads=nt):
        recs, res, ctr = _out(n, 32), _out(n, 12), engine.new_counters()
        st, ctr2 = _out(n, 16), engine.new_counters()
        sums, ctr3 = M.FrameSums(window.frames), engine.new_counters()
        if strided:
            M.verify_strided(engine, a, plan.stride, meta, records=recs[:n * 32], results=res[:n * 12], counters=ctr)
            M.verify_strided_status(engine, a, plan.stride, meta, status=st[:n * 16], counters=ctr2)
            M.verify_strided_frames(engine, a, plan.stride, meta, window, sums, counters=ctr3)
        else:
            M.verify(engine, a, meta, records=recs[:n * 32], results=res[:n * 12], counters=ctr)
            M.verify_status(engine, a, meta, status=st[:n * 16], counters=ctr2)
            M.verify_frames(engine, a, meta, window, sums, counters=ctr3)
        torch.cuda.synchronize()
    what = (strided, nt)
    _same_fields(recs, n, DGRAM_RECORD_DTYPE, er, (what, "records"))
    _same_fields(res, n, RESULT_DTYPE, eres, (what, "results"))
    _same_fields(st, n, DGRAM_STATUS_DTYPE, es, (what, "status"))
    t, fb = sums.read()
    assert t.as_dict() == esums, (what, t.as_dict(), esums)
    assert np.array_equal(fb[:window.frames], efb), what
    for c in (ctr, ctr2, ctr3):
        assert engine.read_counters(c) == ectr, what
