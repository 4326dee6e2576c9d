"""CPU: the plans of tests/far_offsets.py have power. For every plan and every fault that applies to it (a slot offset
mod 2^32, a wrapped ring base, a truncated descriptor offset, a 32-bit in-arena bound, an offset truncated after the
skip), the outcome differs from the correct one in a field, or in a byte of a window, that
tests/test_far_offsets_gpu.py compares; no faulty filler writes outside the windows; the seam slots are where the
plans say; the tick models rebased to first slot 1 equal the models at the true first slot; and the older GPU tests
stay below 2^32 with every byte offset, which is why this suite exists.
"""
import glob
import os
import re

import numpy as np
import pytest

import far_offsets as F
from ctstraffic_amd.types import DESC_DTYPE

SEAM = F.SEAM
RING_CASES = ([("tcp", s, 0, 0) for s in F.VERIFY_STRIDES] + [("tcp", s, 3, 65535) for s in F.VERIFY_STRIDES] +
              [("ms", s, 0, 0) for s in F.VERIFY_STRIDES])
TICK_CASES = ([("server", s, 0, "") for s in F.SERVER_STRIDES] + [("tcp", s, B, "") for s, B in F.TCP_SHAPES] +
              [("paced", s, B, p) for s, B in F.TCP_SHAPES for p in ("cut", "unpaced")] +
              [("exchange", s, B, "") for s, B in F.TCP_SHAPES])


def _rows_differ(x: dict, y: dict) -> list:
    """The compared fields in which two verify outcomes differ."""
    out = []
    for k in x:
        a, b = x[k], y[k]
        same = a == b if isinstance(a, dict) else np.array_equal(np.asarray(a), np.asarray(b))
        if not same:
            out.append(k)
    return out


# ---- 1. the sparse ring ---------------------------------------------------------------------------------------------
def test_sparse_ring_reads_writes_and_compacts():
    r = F.SparseRing(SEAM + 4096)
    assert r.read(SEAM - 4, 8).tolist() == [0xA5] * 8 and r.touched() == []
    r.write(SEAM - 3, bytes([1, 2, 3, 4, 5]))
    r.write(SEAM + 1, [9])                       # a later write wins
    r.write(10, np.arange(4, dtype=np.uint8))
    assert r.read(SEAM - 4, 8).tolist() == [0xA5, 1, 2, 3, 4, 9, 0xA5, 0xA5]
    assert r.touched() == [(10, 14), (SEAM - 3, SEAM + 2)]
    r.flip(SEAM, 0x80)
    assert int(r.read(SEAM, 1)[0]) == 4 ^ 0x80
    d = np.zeros(4, dtype=DESC_DTYPE)
    d["byte_offset"], d["length"] = [10, SEAM - 3, SEAM + 100, SEAM + 4090], [4, 5, 0, 7]
    arena, c = r.compact(d)
    assert c["byte_offset"].tolist()[:3] == [0, 16, 32] and len(arena) == 32
    assert int(c["byte_offset"][3]) > len(arena)  # it left the ring, it leaves the copy
    assert arena[:4].tolist() == [0, 1, 2, 3] and arena[16:21].tolist() == [1, 2, 3, 4 ^ 0x80, 9]
    assert F.merge_ranges([(5, 9), (0, 5), (20, 21), (8, 12)]) == [(0, 12), (20, 21)]


def test_the_arithmetic_of_the_issue():
    """The strides' seam slots, as computed by hand."""
    for stride, below, into in ((1472, 2_917_776, 1024), (3072, 1_398_101, 1024), (1040, 4_129_776, 256)):
        p = F.RingPlan(stride, "fill")
        assert (p.below, SEAM - p.below * stride) == (below, into) and p.n == SEAM // stride + 8
        assert p.seam_slots() == {"crossing": below, "at": None}
    for stride in (64, 1 << 20):
        p = F.RingPlan(stride, "fill")
        assert SEAM % stride == 0 and p.seam_slots() == {"crossing": None, "at": SEAM // stride}
        assert p.below == p.wholly_below == SEAM // stride - 1
    assert (F.RingPlan(1 << 20, "fill").above - 4096, SEAM // 65552, SEAM % 65552) == (0, 65520, 256)


# ---- 2. ring plans: cts_verify_strided(_at) and the MediaStream receive over a ring ----------------------------------
@pytest.mark.parametrize("kind,stride,skip,expected", RING_CASES)
def test_ring_plans_tell_the_defects(kind, stride, skip, expected):
    p = F.RingPlan(stride, kind, skip=skip, expected=expected, base_index=1 << 20)
    good = p.outcome()
    live = dict(zip(p.live.tolist(), range(len(p.live))))
    res = good["results"]
    # the plan's own shape: the flips fail their slots, the slots above them and the low aliases hold the opposite
    a, b = live[p.below], live[p.above]
    assert res["pass"][a] == 0 and res["first_mismatch"][a] == SEAM - 1 - p.below * stride - p.head
    assert res["pass"][b] == 0 and res["first_mismatch"][b] == 0 and res["mismatch_bytes"][b] >= 1
    assert res["pass"][live[p.above + 1]] == 1 and res["pass"][live[p.above + 2]] == 1
    assert res["flags"][live[p.n - 1]] == 1 and res["flags"][live[p.mid]] == 0  # arena_bytes ends in the last slot
    if SEAM % stride == 0:
        assert res["pass"][:3].tolist() == [1, 0, 0]  # slots 0, 1, 2 are the aliases themselves
    if kind == "tcp":
        assert good["cff"].tolist() == [F.EMPTY, (1 << 20) + min(i for i in p.live if res["pass"][live[i]] == 0
                                                                 and res["flags"][live[i]] == 0), F.EMPTY]
    told = {}
    for defect in "ade":
        bad = p.outcome(defect)
        told[defect] = _rows_differ(good, bad)
        assert "results" in told[defect] and "counters" in told[defect], (defect, told)
        if kind == "ms":
            assert p.frames(good) != p.frames(bad) or not np.array_equal(p.frames(good)[1], p.frames(bad)[1])
            assert "status" in told[defect]
    # a wrapped reader sees the first slot above the seam clean and its neighbours dirty
    wrapped = p.outcome("a")["results"]
    assert wrapped["pass"][b] == 1 and wrapped["pass"][live[p.above + 1]] == 0
    narrow = p.outcome("d")["results"]
    assert narrow["flags"][live[p.mid]] == 1 and narrow["flags"][live[p.wholly_below]] == (SEAM % stride != 0)


def test_ring_frames_window_holds_the_seam():
    p = F.RingPlan(1472, "ms")
    out = p.outcome()
    t, fb = p.frames(out)
    w = p.window()
    assert fb[0] == 1472 and fb[(p.above + 1) - p.wholly_below] == 1469 and fb.sum() == 1472 * 2 + 1469
    assert t["error_frames"] == 1 and t["first_exception"] == 0           # the middle slot is stale
    # slots 0-2 under the aliases (448 bytes into slot 0 at this stride), two flips, the last slot, every dead slot
    assert t["exceptions"] == p.n - len(p.live) + 6
    t2, _ = p.frames(out, finished=True)
    assert t2["exceptions"] == 6 and t2["first_exception"] == 0 and w["frames"] == 16


# ---- 3. ring fills: cts_media_stream_fill_strided --------------------------------------------------------------------
@pytest.mark.parametrize("stride", F.RING_FILL_STRIDES)
def test_ring_fill_plans_tell_the_defects(stride):
    p = F.RingPlan(stride, "fill")
    good, windows = p.outcome()["ring"], p.windows()
    assert len(good.touched()) >= 5 and all(F.in_ranges(windows, a, b) for a, b in good.touched())
    last = (p.n - 1) * stride
    assert not any(b > last for _, b in good.touched())  # the last slot leaves the arena: unwritten
    for defect in "ade":
        bad = p.outcome(defect)["ring"]
        assert F.ring_differs(good, bad, windows), defect
        assert all(F.in_ranges(windows, a, b) for a, b in bad.touched()), defect
    assert all(0 <= a < b <= p.arena_bytes for a, b in windows)
    assert sum(b - a for a, b in windows) < 64 * stride


# ---- 4. descriptor plans: cts_fill, cts_media_stream_fill, the workgroup, quad and MediaStream verifies ---------------
@pytest.mark.parametrize("kind", ["tcp", "ms"])
@pytest.mark.parametrize("variant", F.DESC_VARIANTS)
def test_descriptor_plans_tell_the_defects(variant, kind):
    p = F.DescPlan(variant, kind)
    good = p.outcome()
    assert 7 <= len(p.descs) <= 12
    for defect in "ade":
        told = _rows_differ(good, p.outcome(defect))
        assert "results" in told and "counters" in told, (defect, told)
    f = F.DescPlan(variant, kind, corrupt=None)
    filled, windows = f.outcome(what="fill")["ring"], f.windows()
    assert all(F.in_ranges(windows, a, b) for a, b in filled.touched())
    for defect in "ade":
        bad = f.outcome(defect, what="fill")["ring"]
        assert F.ring_differs(filled, bad, windows), defect
        assert all(F.in_ranges(windows, a, b) for a, b in bad.touched()), defect
    assert all(0 <= a < b <= p.arena_bytes for a, b in windows)


def test_descriptor_plans_hold_their_spans():
    spans = {v: F.DescPlan(v).seam_spans() for v in F.DESC_VARIANTS}
    assert spans["at"]["at"] and spans["crossing"]["crossing"] and spans["minus1"]["minus1"] and spans["plus1"]["plus1"]
    assert spans["big"]["above_16g"] and spans["big"]["crossing"] and all(s["leaves"] for s in spans.values())
    assert not any(spans[v]["above_16g"] for v in F.DESC_VARIANTS if v != "big")
    assert sum(len(F.DescPlan(v).descs) for v in F.DESC_VARIANTS if v != "big") >= 20
    for v in F.DESC_VARIANTS:
        p = F.DescPlan(v)
        want = SEAM + (1 << 26) + 1000 + (3 * SEAM if v == "big" else 0)
        assert p.arena_bytes == want and len(p.flips) >= 1
        res = p.outcome()["results"]
        assert (res["pass"] == 0).sum() >= 2 and (res["flags"] == 1).sum() == 1


# ---- 5. tick plans ---------------------------------------------------------------------------------------------------
def _tick_plan(kind, stride, B, pace, **kw):
    return F.TickPlan(kind, stride, B, pace=pace or "cut", **kw)


@pytest.mark.parametrize("kind,stride,B,pace", TICK_CASES)
def test_tick_plans_tell_the_defects(kind, stride, B, pace):
    p = _tick_plan(kind, stride, B, pace)
    assert p.first_slot == SEAM // stride - 3 and 12 <= p.capacity <= 16
    t0, t1 = p.ticks()
    assert t0["written"] >= 4 and t1["first_slot"] == p.first_slot + t0["written"] and t1["written"] >= 1
    assert t1["first_slot"] * stride >= SEAM > t0["first_slot"] * stride
    where = p.seam_slots()
    assert where["below"] and where["above"] and (where["at"] if SEAM % stride == 0 else where["crossing"])
    assert 4.0 <= p.arena_bytes / 2**30 <= 4.1
    if kind == "paced":
        assert (5 in t1["codes"].tolist()) == (pace == "cut")
        assert (t0["tail"]["connections_pending"] > 0) == (pace == "cut")
    if kind == "exchange":  # both directions in both ticks, and the seeked connection's turn inside the first
        n = len(p.settings)
        assert all(min(t["tick"]["bytes_dir"]) > 0 for t in (t0, t1)) and 3 in t0["codes"].tolist()
        mine = [int(r) % n == 2 for r in t0["descs"]["conn_index"][: t0["written"]]]
        assert t0["descs"]["conn_index"][: t0["written"]][mine].tolist() == [2, 2, 2 + n]
        assert int(p.entries["buffers_sent"][2]) > 1 << 33 and {s[0] for s in p.settings} == {0, 1, 2, 3}
    good, windows = p.outcome(), p.windows()
    assert all(F.in_ranges(windows, a, b) for a, b in good["ring"].touched())
    for defect in "ab":
        bad = p.outcome(defect)
        assert F.ring_differs(good["ring"], bad["ring"], windows), defect
        assert all(F.in_ranges(windows, a, b) for a, b in bad["ring"].touched()), defect
    # a wrapped ring base shows in the second tick alone, a wrapped slot offset in both
    first = p.outcome(n_ticks=1)["ring"]
    assert not F.ring_differs(first, p.outcome("b", 1)["ring"], windows)
    assert F.ring_differs(first, p.outcome("a", 1)["ring"], windows)
    tick, g, at = p.seam_hit()
    d = t0["descs"][g]
    assert tick == 0 and SEAM <= at < SEAM + 64 and int(d["byte_offset"]) <= at < int(d["byte_offset"]) + int(d["length"])
    cut = p.outcome("c")["descs"]
    for t in range(F.TICKS):
        same = np.array_equal(cut[t]["byte_offset"], good["descs"][t]["byte_offset"])
        assert not same, ("c", t)
    assert sum(b - a for a, b in windows) < 200 * stride


@pytest.mark.parametrize("kind,stride,B,pace", TICK_CASES)
def test_rebased_tick_models_are_the_models(kind, stride, B, pace):
    """On a scaled-down seam the models run at the true first slot over an arena from byte 0: the same state, the
    same descriptors and the same bytes as the rebased run. 2^16 where the stride allows (three slots below it)."""
    seam = max(1 << 16, 16 * stride)
    assert seam == 1 << 16 or stride > 4096
    near, far = _tick_plan(kind, stride, B, pace, seam=seam), _tick_plan(kind, stride, B, pace, seam=seam, rebase=False)
    assert near.base_slot == near.first_slot - 1 and far.base_slot == 0 and near.first_slot == seam // stride - 3
    shift = near.base_slot * stride
    for t, (x, y) in enumerate(zip(near.ticks(), far.ticks())):
        for k in x:
            if k == "host":
                assert np.array_equal(x[k], y[k][shift:]) and (y[k][:shift] == F.BACKGROUND).all(), t
            elif isinstance(x[k], dict) or x[k] is None or isinstance(x[k], int):
                assert x[k] == y[k], (t, k)
            else:
                assert np.array_equal(x[k], y[k]), (t, k)
    assert not F.ring_differs(near.outcome()["ring"], far.outcome()["ring"], [(0, near.arena_bytes)])


def test_one_exchange_tick_moves_more_than_4_gib():
    """What tests/test_far_offsets_gpu.py's big tick rests on, from plan_depths.exchange_tick: direction 0 and the
    tick's bytes need more than 32 bits, direction 1 is there, and a tick block or a sent block that keeps 32 bits of
    a sum holds other values."""
    import plan_depths as P

    case = F.big_exchange_tick()
    stride, B = case["stride"], case["B"]
    assert stride == 16 << 20 and B == stride - 5 and 256 * stride == SEAM < case["capacity"] * stride
    state = P.exchange_state(case["settings"])
    got = P.exchange_tick(state, case["ids"], stride, case["capacity"], case["max_buffers"], len(state))
    assert got["taken"] == [86] * 4 + [16] and got["codes"] == [0] * 5 and got["tick"]["buffers"] == 360
    d0, d1 = got["bytes_dir"]
    assert d0 >= SEAM and got["tick"]["bytes"] >= SEAM and d1 > 0 and d0 + d1 == got["tick"]["bytes"]
    assert (d0, d1) == (268 * B, 92 * B)
    narrow = [d0 % SEAM, d1 % SEAM]
    assert narrow != got["bytes_dir"] and sum(narrow) != got["tick"]["bytes"] != got["tick"]["bytes"] % SEAM
    # a wave that sums a direction in 32 bits: one PushPull connection alone stays below 2^32, two do not
    assert 65 * B < SEAM <= 4 * 65 * B and all(e[P.XS0] == 65 * B and e[P.XS1] == 21 * B for e in state[:4])
    lengths = {ln for _, ln, _ in got["slots"]}
    assert lengths == {B} and {r // 5 for r, _, _ in got["slots"]} == {0, 1}
    assert got["slots"][256][0] in range(10) and len(got["slots"]) == 360


# ---- 6. accounting ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,skip", [(1472, 26), (1 << 20, 0)])
def test_accounting_plans_tell_the_narrow_bound(stride, skip):
    p = F.RingPlan(stride, "tcp", skip=skip, base_index=1 << 20)
    slots = np.array([5, (1 << 20) + p.above, F.EMPTY], dtype=np.uint32)
    sums, table = p.accounting(slots)
    narrow, narrow_table = p.accounting(slots, "d")
    assert sums != narrow and not np.array_equal(table, narrow_table)
    lens = dict(zip(p.live.tolist(), p.lens.tolist()))
    before = [i for i in lens if i <= p.above]
    assert sums["bytes_recv"] == sum(lens[i] - skip for i in before)
    assert sums["buffers_failed"] == 1 and sums["bytes_after_failure"] == lens[p.above + 1] + lens[p.above + 2] - 2 * skip
    if skip == 0:  # every dead slot is a buffer of no bytes
        assert sums["buffers_recv"] + sums["buffers_after_failure"] == p.n - 1


# ---- 7. why this suite: the older GPU tests never reach 2^32 ---------------------------------------------------------
def test_older_gpu_tests_stay_below_the_seam():
    """Their first_slot literals are 0 and 3 in the parametrised tests and at most 14 anywhere (the refused ones
    aside), and their largest rings, restated here, end far below 2^32; only test_max_length_buffers and the
    full-size configurations (a sampled workgroup verify, a sampled payload fill and quad verify) go further."""
    here = os.path.dirname(os.path.abspath(__file__))
    seen, swept = set(), set()
    for path in glob.glob(os.path.join(here, "test_*.py")):
        if "far_offsets" in path:
            continue
        text = open(path).read()
        seen |= {int(x) for x in re.findall(r"first_slot=(\d+)", text)}
        for m in re.findall(r'parametrize\("first_slot", \[([0-9, ]+)\]', text):
            swept |= {int(x) for x in m.split(",")}
    assert swept == {0, 3} and max(seen) == 14, (swept, seen)
    assert 14 * (16 << 20) < SEAM  # even under the widest stride a tick accepts
    import test_media_stream_servers_gpu as ms_gpu
    import test_tcp_senders_gpu as tcp_gpu

    rings = [("test_verify_strided_matches_oracle", 6000, 9017), ("test_gpu_media_stream_verify_strided", 7000, 9017),
             ("test_gpu_media_stream_fill_strided", 3000, 4096), ("test_buffer_edges", 3 + 13 + 2, 65536),
             ("test_shuffled_lists", 3 * 1100, 128), ("test_one_connection_many_buffers", 705, 48),
             ("test_strides_and_first_slot", 3 + 40 + 1, 1408),
             ("test_prefix_seams", sum(-(-f // m) for f, m, _ in ms_gpu._SEAM_TABLE), 128),
             ("test_shuffled_lists, every connection", 7 * len(tcp_gpu._SETTINGS_1500), 128)]
    for name, slots, stride in rings:
        assert slots * stride < SEAM // 64, name
