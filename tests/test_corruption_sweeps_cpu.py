"""CPU: what tests/test_corruption_sweeps_gpu.py rests on (tests/corruption_sweeps.py).

1. The role model is the kernels': its constants are the sources', and wg_roles / quad_roles agree with plain
   lane-by-lane walks of scan_buffer / scan_whole_exact and quad_scan_interior's loops; the large shapes are what their
   derivations say (one full round and a partial tail round, the period's wrap where it is meant to be, ...).
2. For every plan the oracle's records equal the closed form of the plan's flips and a plain numpy verifier over the
   arena, and the clean copies pass.
3. Coverage: every role of every shape owns buffers whose only corrupt byte is the first and the last byte of the role's
   first and last chunk; the pairs plans hold every ordered pair of waves.
4. Every broken verifier built from the role model -- one role ignored, a byte mask off by one, the last interior chunk
   dropped, a wave's minimum lost -- disagrees with the oracle on every plan it applies to. These stand in for "a kernel
   that is wrong in role R fails the GPU test".
"""
import os
import re

import numpy as np
import pytest

import corruption_sweeps as S
import oracle
from ctstraffic_amd.types import DESC_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ctstraffic_amd", "csrc")
FIELDS = ("first_mismatch", "mismatch_bytes", "expected", "actual", "pass", "flags")


def _same(got, exp, what):
    for f in FIELDS:
        bad = np.nonzero(got[f] != exp[f])[0]
        assert bad.size == 0, (what, f, int(bad.size), bad[:6].tolist(), got[f][bad[:6]].tolist(),
                               exp[f][bad[:6]].tolist())


@pytest.fixture(scope="module", autouse=True)
def _release_arenas():
    """The cached plans (about 1.3 GB) go when the module is done."""
    yield
    for cached in (S.wg_plan, S.quad_plan, S.small_sweep, S.ms_plan, S.mail_cases):
        cached.cache_clear()


# ---- 1. the model is the kernels' ------------------------------------------------------------------------------------
def _constant(file, name):
    text = open(os.path.join(CSRC, file)).read()
    m = re.search(r"(?:constexpr\s+\w+\s+%s\s*=|#define\s+%s)\s*(\d+)" % (name, name), text)
    assert m, (file, name)
    return int(m.group(1))


def test_constants_are_the_sources():
    assert S.BLOCK == _constant("cts_device_util.hpp", "kBlock")
    assert S.WG_LOADS == _constant("cts_verify.hip", "kWgLoads")
    assert S.QUAD_TEAM == _constant("cts_quad.hpp", "kQuadTeam")
    assert S.QUAD_LOADS == _constant("cts_quad.hpp", "kQuadLoads")
    assert S.MAIL_PIECE == _constant("cts_internal.hpp", "kMailPieceBytes")
    assert S.MAIL_GROUP == _constant("cts_internal.hpp", "CTS_MAIL_GROUP")
    # verify_wg_body re-reads a dirty lane's chunks with scan_exact_owned<kBlock, 2>: the fast pass's ownership only
    # while a chunk's lane is (chunk - cb0) mod kBlock in both, whatever the loads per round
    assert "scan_exact_owned<kBlock, 2, NT>" in open(os.path.join(CSRC, "cts_verify.hip")).read()


def test_shapes_are_what_their_derivations_say():
    bad = [k for k, ok in list(S.wg_shape_facts().items()) + list(S.quad_shape_facts().items()) if not ok]
    assert bad == []
    shapes = S.small_shapes()
    assert len(set(shapes)) == len(shapes) > 1500
    lo, nch, hi, cb0 = S.geometry(np.array([s for s, _ in shapes]), np.array([n for _, n in shapes]))
    # every range_mask(lo, hi) of a single chunk, and per start nchunks of 1, 2, 3 and cb0 .. cb0 + 3 ending 1 and 16 in
    assert {(a, b) for a in range(16) for b in range(a + 1, 17)} == \
        set(zip(lo[nch == 1].tolist(), hi[nch == 1].tolist()))
    for start in range(128):
        c = 8 - ((start >> 4) & 7)
        mine = np.array([s == start for s, _ in shapes])
        assert {(n, h) for n in {1, 2, 3, c, c + 1, c + 2, c + 3} - {1} for h in (1, 16)} <= \
            set(zip(nch[mine].tolist(), hi[mine].tolist())), start


def _walk_wg(start, length):
    """scan_buffer / scan_whole_exact lane by lane: {chunk: (kind, round, u, lane)}, every chunk owned once."""
    lo, nch, hi, cb0 = (int(x) for x in S.geometry(start, length))
    own = {}

    def give(c, role):
        assert c not in own and 0 <= c < nch, (start, length, c, role)
        own[c] = role
    whole = lo == 0 and hi == 16 and cb0 == 8
    if whole:
        cb, c_end = 0, nch
    else:
        for lane in range(S.BLOCK):  # edge_chunk_of / edge_chunk_used
            if lane == 0 and nch:
                give(0, (S.EDGE0, 0, 0, 0))
            elif lane == 1 and nch > 1:
                give(nch - 1, (S.LAST, 0, 0, 1))
            elif 2 <= lane <= 8 and lane - 1 < min(nch - 1, cb0):
                give(lane - 1, (S.HEAD, 0, 0, lane))
        cb, c_end = cb0, nch - 1
        if nch < 3:
            c_end = cb
    rnd = 0
    while cb + S.WG_ROUND <= c_end:
        for u in range(S.WG_LOADS):
            for lane in range(S.BLOCK):
                give(cb + u * S.BLOCK + lane, (S.FULL, rnd, u, lane))
        cb, rnd = cb + S.WG_ROUND, rnd + 1
    if cb < c_end:
        for u in range(S.WG_LOADS):
            for lane in range(S.BLOCK):
                if cb + u * S.BLOCK + lane < c_end:
                    give(cb + u * S.BLOCK + lane, (S.TAIL, 0, u, lane))
    assert sorted(own) == list(range(nch)), (start, length)
    return own


def _walk_quad(start, length):
    lo, nch, hi, cb0 = (int(x) for x in S.geometry(start, length))
    cs, c_hi = cb0 - 8, nch - 2
    own = {}
    if nch >= 1:
        own[0] = (S.EDGE0, 0, 0, 0)
    if nch >= 2:
        own[nch - 1] = (S.LAST, 0, 0, 1)
    r = 0
    while cs + r * S.QUAD_ROUND <= c_hi:
        for lane in range(S.QUAD_TEAM):
            for u in range(S.QUAD_LOADS):
                c = cs + r * S.QUAD_ROUND + lane + u * S.QUAD_TEAM
                if 1 <= c <= c_hi:
                    assert c not in own
                    own[c] = (S.ROUND, r, u, lane)
        r += 1
    assert sorted(own) == list(range(nch)), (start, length)
    return own


def test_role_model_follows_the_kernels_loops():
    shapes = S.small_shapes()[::7] + [(S.WG_START, S.WG_LENGTH), (0, S.WHOLE_LENGTH), (0, 65536), S.QUAD_A[:2],
                                      S.QUAD_B[:2], (7, 3000), (71, 3000), (0, 16 * 1024), (16, 16 * 520),
                                      (127, 9000), (0, 16 * 512), (0, 16 * 513), (1, 16 * 520)]
    for start, length in shapes:
        nch = int(S.geometry(start, length)[1])
        for walk, roles in ((_walk_wg, S.wg_roles), (_walk_quad, S.quad_roles)):
            own = walk(start, length)
            r = roles(start, length, np.arange(nch))
            got = list(zip(r["kind"].tolist(), r["round"].tolist(), r["u"].tolist(), r["lane"].tolist()))
            assert got == [own[c] for c in range(nch)], (start, length, walk.__name__)
            assert (roles(start, length, np.array([-1, nch]))["kind"] == -1).all()


# ---- 2. to 4. the plans ----------------------------------------------------------------------------------------------
def _oracle(plan):
    return oracle.verify_batch(plan.arena, plan.descs, n_conns=S.N_CONNS)


def _check_plan(plan, path, name, by_wave=True):
    er, ectr, eslots = _oracle(plan)
    n = len(plan.descs)
    assert (er["flags"] == 0).all() and ectr["buffers_checked"] == n
    row, pos = S.diff_entries(plan)
    res, ctr, slots = S.records(plan, row, pos)
    _same(res, er, (name, "plain verifier"))
    assert ctr == ectr and np.array_equal(slots, eslots), name
    # every connection fails (a ring is one connection's)
    assert (eslots != S.EMPTY).all() if plan.strided is None else eslots[plan.strided[3]] != S.EMPTY, name
    if plan.flips is not None:
        _same(S.closed_form(plan), er, (name, "closed form"))
        dirty = np.unique(plan.flips[0]).size
        per = np.bincount(np.bincount(plan.flips[0], minlength=n))
        assert per.size <= 3 and (per.size < 3 or per[1] == 0), name  # all single flips, or all pairs
    else:
        dirty = 4 * len(S.SHIFTS)
        assert int(er["mismatch_bytes"].max()) * 2 >= int(S.span_length(plan)[0]) - 16, name  # half the bytes at 512
    assert int(er["pass"].sum()) == n - dirty and 0.2 < (n - dirty) / n < 0.3, name
    # the clean copies are spread through the batch: no run of 16 buffers without a dirty one
    assert int(np.convolve(er["pass"].astype(np.int64), np.ones(16, dtype=np.int64), "valid").max()) < 16, name
    roles = S.entry_roles(plan, path, row, pos)
    muts = S.mutants(path, roles, by_wave=by_wave)
    if plan.flips is not None and per.size == 3:
        muts += S.lost_minimum_mutants(path, roles, row)
        assert S.wave_order_gaps(plan, path) == [], name
        assert (er["mismatch_bytes"][er["pass"] == 0] == 2).all()
    elif plan.flips is not None:
        assert S.coverage_gaps(plan, path, by_wave=by_wave) == [], name
    assert len(muts) >= 4, name
    passed = []
    for what, drop_first, drop_count in muts:
        mres, mctr, mslots = S.records(plan, row, pos, drop_first=drop_first, drop_count=drop_count)
        if all(np.array_equal(mres[f], er[f]) for f in FIELDS):
            passed.append(what)
    assert passed == [], (name, "the plan lets these broken verifiers through")
    return muts


@pytest.mark.parametrize("name", S.WG_PLANS)
def test_workgroup_plan(name):
    plan = S.wg_plan(name)
    muts = _check_plan(plan, "wg", name, by_wave=name != "prod")
    names = {m[0] for m in muts}
    if name == "ragged_odd":
        assert len(plan.descs) == S._with_clean(S.WG_LENGTH)
        assert {"ignores edge0", "ignores last", "ignores head", "drops the last interior chunk",
                "owns no head chunk 1"} | \
            {"ignores full(round=0, u=%d, wave=%d)" % (u, w) for u in range(2) for w in range(4)} | \
            {"ignores tail(u=0, wave=%d)" % w for w in range(4)} | {"ignores tail(u=1, wave=0)"} <= names
    if name == "whole_even":
        assert {"ignores tail(u=1, wave=0)", "ignores full(round=0, u=1, wave=3)"} <= names
        assert not any(k in names for k in ("ignores edge0", "ignores last", "ignores head"))
    if name == "prod":
        assert len(plan.flips[0]) == 1024
        assert {"ignores full(round=%d, u=%d, wave=0)" % (r, u) for r in range(8) for u in range(2)} <= names
    if name.startswith("pairs"):
        assert {"loses the minimum of wave %d" % w for w in range(4)} <= names
    if name == "small":
        assert {"ignores edge0", "ignores last", "ignores head", "ignores tail(u=0, wave=0)"} <= names


@pytest.mark.parametrize("name", S.QUAD_PLANS)
def test_quad_plan(name):
    plan = S.quad_plan(name)
    muts = _check_plan(plan, "quad", name)
    names = {m[0] for m in muts}
    if name in ("b", "ring_b"):
        assert len(plan.flips[0]) == 8 * 3000
        assert {"ignores round(round=%d, u=%d, wave=0)" % (r, u) for r in range(2) for u in range(6)} <= names
    if name == "b":
        assert "ignores round(round=2, u=0, wave=0)" in names
    if name == "ring_b":
        assert set(S.span_start(plan).tolist()) == {7, 71}
    if name == "pairs":
        assert {"loses the minimum of lane %d" % k for k in (0, 1, 15)} <= names
    if plan.strided is not None:
        stride, skip, e, conn = plan.strided
        d = plan.descs
        assert (d["byte_offset"] == np.arange(len(d)) * stride).all() and (d["skip_head"] == skip).all()
        assert (d["expected_pattern_offset"] == e).all() and (d["conn_index"] == conn).all()
        assert (d["length"] <= stride).all()


def test_a_thinned_plan_is_refused():
    """The checks above are not vacuous: the ragged sweep without the bytes of the tail round's partial load has a
    coverage gap there and lets the verifier that ignores that load through; the 64 KiB landmark set, read per wave,
    lacks wave 2."""
    lo, nch = 3, S.WG_NCHUNKS
    chunk = (lo + np.arange(S.WG_LENGTH)) >> 4
    r = S.wg_roles(S.WG_START, S.WG_LENGTH, chunk)
    thin = S.sweep(S.WG_START, S.WG_LENGTH, 17, S.WG_E_ODD, seed=11,
                   positions=np.nonzero(~((r["kind"] == S.TAIL) & (r["u"] == 1)))[0])
    assert {g[2] for g in S.coverage_gaps(thin, "wg")} == {"tail(u=1, wave=0)"}
    er = _oracle(thin)[0]
    row, pos = S.diff_entries(thin)
    full = S.entry_roles(S.wg_plan("ragged_odd"), "wg", *S.diff_entries(S.wg_plan("ragged_odd")))
    keys = np.unique(full["key"])
    roles = S.entry_roles(thin, "wg", row, pos)
    through = []
    for k in keys:
        m = roles["key"] == k
        if all(np.array_equal(S.records(thin, row, pos, drop_first=m, drop_count=m)[0][f], er[f]) for f in FIELDS):
            through.append(S.role_name(k))
    assert through == ["tail(u=1, wave=0)"]
    assert {g[2] for g in S.coverage_gaps(S.wg_plan("prod"), "wg", by_wave=True)} >= \
        {"full(round=%d, u=%d, wave=2)" % (rr, u) for rr in range(8) for u in range(2)}


def test_small_sweep_masks():
    """The small sweep as the byte masks see it: for every (lo, hi) of a single chunk a broken range_mask(lo, hi) -- one
    that drops its first or its last byte -- is caught, and so is, for every lo and every hi_last, a chunk 0 or a last
    chunk masked one byte short in a span of several chunks."""
    plan = S.small_sweep()
    er = _oracle(plan)[0]
    row, pos = S.diff_entries(plan)
    r = S.entry_roles(plan, "wg", row, pos)
    assert len(plan.descs) > 100000
    for lo in range(16):
        for hi in range(lo + 1, 17):
            one = (r["nch"] == 1) & (r["lo"] == lo) & (r["hi_last"] == hi)
            for m in (one & (r["byte"] == lo), one & (r["byte"] == hi - 1)):
                assert m.any()
                got = S.records(plan, row, pos, drop_first=m, drop_count=m)[0]
                assert not np.array_equal(got["pass"], er["pass"]), (lo, hi)
    ends = [(r["nch"] > 1) & (r["lo"] == lo) & (r["pos"] == 0) for lo in range(16)]
    ends += [(r["nch"] > 1) & (r["hi_last"] == hi) & (r["pos"] == r["length"] - 1) for hi in (1, 16)]
    for m in ends:
        got = S.records(plan, row, pos, drop_first=m, drop_count=m)[0]
        assert m.any() and not np.array_equal(got["pass"], er["pass"])


# ---- the host paths --------------------------------------------------------------------------------------------------
def test_host_cases_cover_the_mailbox_roles():
    cases = S.mail_cases()
    assert 1500 < len(cases) <= 6000
    lo, nch, _, _ = (int(x) for x in S.geometry(S.MAIL_OFFSET, S.MAIL_LENGTH))
    assert S.MAIL_E % 2 == 1 and -(-nch // S.MAIL_PIECE_CHUNKS) == 18
    singles = np.array([c[0][0] for c in cases if len(c) == 1])
    r = S.mail_roles(S.MAIL_OFFSET, S.MAIL_LENGTH, (lo + singles) >> 4)
    have = set(singles.tolist())
    last_chunk = range(S.MAIL_LENGTH - ((lo + S.MAIL_LENGTH - 1) % 16 + 1), S.MAIL_LENGTH)
    assert set(range(16 - lo)) <= have and set(last_chunk) <= have
    assert r["first"].any() and r["last"].any()
    for k in S.MAIL_SEAMS:  # both chunks of the seam, every byte
        seam = 16 * (k + 1) * S.MAIL_PIECE_CHUNKS - lo
        assert set(range(seam - 16, seam + 16)) <= have, k
    assert {(p, w) for p in range(18) for w in range(4) if p < 17 or w == 0} <= \
        set(zip(r["piece"].tolist(), r["wave"].tolist()))
    assert set(r["wg"].tolist()) == {0, 1, 2, 3} and set(r["pass"].tolist()) == {0, 1}
    both = [c for c in cases if len(c) == 2]
    a = S.mail_roles(S.MAIL_OFFSET, S.MAIL_LENGTH, (lo + np.array([c[0][0] for c in both])) >> 4)
    b = S.mail_roles(S.MAIL_OFFSET, S.MAIL_LENGTH, (lo + np.array([c[1][0] for c in both])) >> 4)
    assert all(c[0][0] < c[1][0] and c[0][1] != c[1][1] for c in both)
    # the earlier byte in the later workgroup, in the later wave, and in the earlier pass of another workgroup
    assert ((a["wg"] > b["wg"]) & (a["piece"] < b["piece"])).any() and (a["wave"] > b["wave"]).any()
    later_pass = a["pass"] < b["pass"]
    assert (later_pass & (a["wg"] != b["wg"])).any() and (later_pass & (a["wg"] == b["wg"])).any()
    for wg_a in range(4):
        for wg_b in range(4):
            if wg_a != wg_b:
                assert ((a["wg"] == wg_a) & (b["wg"] == wg_b)).any(), (wg_a, wg_b)
    # the oracle's records are the closed form, batch by batch
    clean = S.pattern(S.MAIL_E + np.arange(S.MAIL_LENGTH))
    slot = S.MAIL_LENGTH + 16
    for k in range(0, len(cases), 256):
        part = cases[k:k + 256]
        arena = np.full(len(part) * slot, S.GAP, dtype=np.uint8)
        descs = np.zeros(len(part), dtype=DESC_DTYPE)
        descs["byte_offset"] = np.arange(len(part)) * slot + S.MAIL_OFFSET
        descs["length"], descs["expected_pattern_offset"] = S.MAIL_LENGTH, S.MAIL_E
        rows = arena.reshape(len(part), slot)
        rows[:, S.MAIL_OFFSET:S.MAIL_OFFSET + S.MAIL_LENGTH] = clean
        for i, c in enumerate(part):
            for p, x in c:
                rows[i, S.MAIL_OFFSET + p] ^= x
        er = oracle.verify_batch(arena, descs)[0]
        first = np.array([c[0][0] for c in part])
        assert (er["first_mismatch"] == first).all() and (er["mismatch_bytes"] == [len(c) for c in part]).all()
        assert (er["expected"] == clean[first]).all()
        assert (er["actual"] == clean[first] ^ np.array([c[0][1] for c in part], dtype=np.uint8)).all()
    small = S.small_mail_cases()
    assert len(small) == 16 * sum(S.SMALL_LENGTHS) <= 6000


# ---- the MediaStream receive -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True])
def test_media_stream_plan(strided):
    plan = S.ms_plan(strided)
    n = len(plan.descs)
    recs, res, ctr = oracle.media_stream_verify(plan.arena, plan.descs)
    cf = S.ms_closed_form(plan)
    assert np.array_equal(recs["kind"], cf["kind"]) and set(cf["kind"].tolist()) == {0, 1, 3, 4}
    assert np.array_equal(recs["completed_bytes"], plan.completed)
    data = cf["kind"] == 0
    for f in ("pass", "first_mismatch", "mismatch_bytes", "expected", "actual"):
        assert np.array_equal(res[f][data], cf[f][data]), f
    assert (res["pass"][~data] == 0).all() and ctr["mismatched_bytes"] == int(cf["mismatch_bytes"].sum())
    # header bytes 2 .. 25: the record changes, the verdict does not
    hdr = (plan.flip_at >= 2) & (plan.flip_at < S.HEADER)
    assert int(hdr.sum()) == 16 * 8 * 24 and (res["pass"][hdr] == 1).all() and (recs["kind"][hdr] == 0).all()
    seq_flip = hdr & (plan.flip_at < 10)
    assert (recs["sequence_number"][seq_flip] != np.arange(n)[seq_flip] % 80).all()
    assert (recs["sequence_number"][~hdr & data] == np.arange(n)[~hdr & data] % 80).all()
    # every ho, every payload byte of every length; the ring's slots lie on every address mod 128
    ho = plan.ho
    for comp in (S.MS_DATAGRAM,) + S.MS_SHORT:
        m = (plan.completed == comp) & (plan.flip_at >= S.HEADER)
        assert set(zip(ho[m].tolist(), plan.flip_at[m].tolist())) == {(h, S.HEADER + p) for h in range(16)
                                                                      for p in range(comp - S.HEADER)}, comp
    start = (plan.descs["byte_offset"].astype(np.int64) + S.HEADER) % 128
    if strided:
        assert (plan.descs["byte_offset"] == np.arange(n) * S.MS_STRIDE).all()
        assert set(start.tolist()) == set(range(128))
    else:
        assert set(start.tolist()) == {S.HEADER + h for h in range(16)}
    # the quad roles of the payload spans: every role of every shape owns single-byte corruptions at its ends
    shape = S.Plan(plan.arena, plan.descs.copy(), plan.stride, None, None)
    shape.descs["skip_head"] = np.minimum(S.HEADER, plan.completed)
    pay = (plan.flip_at >= S.HEADER)
    shape = shape._replace(flips=(np.nonzero(pay)[0], plan.flip_at[pay] - S.HEADER, plan.flip_xor[pay]))
    keep = np.isin(plan.completed, (S.MS_DATAGRAM,) + S.MS_SHORT)  # the swept lengths
    sub = S.Plan(plan.arena, shape.descs[keep], plan.stride,
                 (np.cumsum(keep)[shape.flips[0]] - 1, shape.flips[1], shape.flips[2]), None)
    if not strided:  # (the ring's 128 starts each see a random third of the positions)
        assert S.coverage_gaps(sub, "quad") == []
    sums, fb = S.ms_frame_sums(recs, res)
    assert sums["exceptions"] > 0 and sums["error_frames"] > 0 and sums["datagrams"] > n // 4 and fb.all()
    assert 0.2 < np.count_nonzero(plan.flip_at < 0) / n < 0.3
