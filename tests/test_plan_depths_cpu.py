"""CPU: what tests/test_plan_depth_gpu.py rests on (tests/plan_depths.py).

1. plan_depths.facts agrees with plain per-thread loops, one workgroup, batch and lane at a time, for the ring lookup
   of ms_server_fill and for tcp_sender_descs, on a small made-up device and on the idle-run case.
2. Every case of the GPU file reaches the facts it exists for at 64, 104, 228, 256 and 304 compute units.
3. The shapes of the older sender tests reach none of the five planner paths at 256 CUs and default attributes: the
   gap the plan-depth tests close.
4. Sensitivity: every defect of plan_depths is told from the defect-free planner by the case built for it, and the
   defect-free planner equals the numpy model on every case.
5. The numpy models at the long lists' size equal one-connection-at-a-time loops in Python integers.
6. The exchange tick's three cases reach the same facts, the planner's defects each change the outcome of one of them,
   and workload.tcp_exchange_view equals plan_depths.exchange_tick on all of them.
"""
import numpy as np
import pytest

import launch_depths as L
import plan_depths as P
from ctstraffic_amd import workload as W

CUS = L.CU_COUNTS


# ---- 1. facts against plain loops ------------------------------------------------------------------------------------
def _ring_by_loops(w, capacity, cus, ring_bpc):
    """ms_server_fill's lookup as the kernel states it: per workgroup, per batch, per thread its binary search of the
    513 staged prefixes and, from their end, of prefix[] itself. Returns (owners per datagram, per workgroup the
    batches as facts() lists them)."""
    n = len(w)
    prefix, total, p = [], 0, 0
    for want in w:
        prefix.append(p)
        if want and p + want <= capacity:
            total += want
        p += want
    prefix.append(p)
    total = min(total, capacity)
    grid = L.batch_fill_grid(capacity, L.RING_BATCH, cus, ring_bpc)
    even = (total + grid - 1) // grid
    per_wg = max(even, min(total, L.RING_BATCH))
    owners, workgroups = [None] * total, []
    for b in range(grid):
        g0 = b * per_wg
        if g0 >= total:
            continue
        g1 = min(g0 + per_wg, total)
        lo, hi = 0, n
        while hi - lo > 1:
            mid = lo + (hi - lo) // 2
            lo, hi = (mid, hi) if prefix[mid] <= g0 else (lo, mid)
        first_listed, from_search, batches = lo, False, []
        for d0 in range(g0, g1, L.RING_BATCH):
            nb = min(g1 - d0, L.RING_BATCH)
            i0 = first_listed
            ps = [prefix[i0 + t if i0 + t < n else n] for t in range(L.RING_BATCH + 1)]
            staged = fallback = moved = exact = 0
            handed, last_moved = from_search, False
            for t in range(nb):
                g = d0 + t
                lo, hi = 0, L.RING_BATCH + 1
                while hi - lo > 1:
                    mid = (lo + hi) >> 1
                    lo, hi = (mid, hi) if ps[mid] <= g else (lo, mid)
                staged = max(staged, sum(1 for x in ps if x <= g))
                assert sum(1 for x in ps if x <= g) == lo + 1
                i, searched = i0 + lo, False
                if lo == L.RING_BATCH and i + 1 < n:
                    fallback += 1
                    a, z = i, n
                    while z - a > 1:
                        mid = a + (z - a) // 2
                        a, z = (mid, z) if prefix[mid] <= g else (a, mid)
                    searched = a != i
                    moved += searched
                    exact += not searched
                    i = a
                assert i < n and prefix[i] <= g < prefix[i] + w[i]
                owners[g] = i
                if t == nb - 1:
                    first_listed, last_moved = i, searched
            batches.append((d0, nb, i0, staged, fallback, moved, exact, handed))
            from_search = last_moved
        workgroups.append(batches)
    return owners, workgroups


def _descs_by_loops(w, capacity, cus, bpc):
    """tcp_sender_descs as the kernel states it: (owners per slot, the most passes of a lane, slots of later passes,
    the longest search)."""
    n = len(w)
    prefix, p = [], 0
    for want in w:
        prefix.append(p)
        p += want
    total = min(p, capacity)
    grid = L.grid_for((capacity + 255) // 256, 1, cus, bpc)
    owners, passes_max, later, longest = [None] * total, 0, 0, 0
    for lane in range(grid * 256):
        g, passes = lane, 0
        while g < total:
            lo, hi, steps = 0, n, 0
            while hi - lo > 1:
                mid = lo + (hi - lo) // 2
                lo, hi = (mid, hi) if prefix[mid] <= g else (lo, mid)
                steps += 1
            owners[g], longest = lo, max(longest, steps)
            later += passes > 0
            passes += 1
            g += grid * 256
        passes_max = max(passes_max, passes)
    return owners, passes_max, later, longest


def _small_ms_wants():
    """A made-up list for a 4-CU device: frames of 1 to 9 datagrams with idle runs of 0 to 1 100 between them."""
    rng = np.random.default_rng(4)
    w = []
    for k in range(260):
        w.append(int(rng.integers(1, 10)) if k % 9 else 300)
        w += [0] * int(rng.choice([0, 0, 1, 3, 511, 512, 513, 1100], p=[.5, .2, .1, .1, .025, .025, .025, .025]))
    return w


@pytest.mark.parametrize("ring_bpc", [1, 4])
def test_ring_facts_are_the_loops(ring_bpc):
    cases = [(_small_ms_wants(), 4)]
    cases.append((cases[0][0], 4))
    small = P.idle_runs("ms", 64)
    cases.append((small["w"], 256))
    full = P.idle_runs_full("ms", 64, 4, ring_bpc)
    cases.append((full["w"], 4))
    for k, (w, cus) in enumerate(cases):
        capacity = sum(w) - (300 if k == 1 else 0)  # k == 1: the capacity cuts the list
        f = P.facts(w, capacity, "ms", cus, ring_bpc=ring_bpc)
        owners, workgroups = _ring_by_loops(w, capacity, cus, ring_bpc)
        assert f["ring_batches"] == workgroups, k
        assert owners == P.slot_owners(w, capacity, "ms", cus, ring_bpc), k
        assert f["fallback"] == sum(x[4] for b in workgroups for x in b) > 0, k
        assert f["moved"] > 0 and f["total"] == len(owners), k
    assert P.idle_reaches(P.facts(full["w"], full["capacity"], "ms", 4, ring_bpc=ring_bpc), True) == []


def test_descs_facts_are_the_loops():
    small = P.idle_runs("tcp", 64)
    two = P.descs_two_passes(4)
    for w, capacity, cus, bpc in [(small["w"], small["capacity"], 4, 4), (small["w"], 100, 4, 1),
                                  (two["w"], two["capacity"], 4, 1), (_small_ms_wants(), 3000, 4, 1)]:
        f = P.facts(w, capacity, "tcp", cus, blocks_per_cu=bpc)
        owners, passes, later, longest = _descs_by_loops(w, capacity, cus, bpc)
        assert (f["descs_passes_max"], f["descs_later_slots"], f["search_steps_max"]) == (passes, later, longest)
        assert owners == P.slot_owners(w, capacity, "tcp", cus, bpc) and None not in owners
    assert passes > 1


# ---- 2. every case reaches its facts at every CU count ---------------------------------------------------------------
@pytest.mark.parametrize("n_listed", P.LONG_LISTED)
def test_long_lists_reach_the_second_pass(n_listed):
    for case, kind in [(P.long_tcp(n_listed), "tcp"), (P.long_tcp(n_listed, paced=True), "tcp"),
                       (P.long_ms(n_listed), "ms")]:
        f = P.facts(case["w"], case["capacity"], kind)
        assert P.long_reaches(case, n_listed, f) == [], f
        assert (1 in P.reaches(f)) == (n_listed > 65_536)
        assert case["ids"].count(P.LONG_TABLE) == case["ids"].count(0xFFFFFFFF) == 1
        assert len(set(case["ids"])) == n_listed
    assert {11, 700} <= set(P.long_tcp(n_listed)["ids"])


@pytest.mark.parametrize("cus", CUS)
def test_descs_case_takes_two_passes(cus):
    case = P.descs_two_passes(cus)
    f = P.facts(case["w"], case["capacity"], "tcp", cus, blocks_per_cu=1)
    assert P.descs_reaches(f) == [] and 5 in P.reaches(f), f
    assert f["total"] > f["descs_grid"] * L.BLOCK and case["capacity"] * 16 < 8 << 20
    # at the default of four workgroups per CU the same tick stays in one pass
    assert P.facts(case["w"], case["capacity"], "tcp", cus)["descs_passes_max"] == 1


@pytest.mark.parametrize("cus", CUS)
def test_idle_runs_reach_the_fallback(cus):
    for stride in (64, 1040):
        small = P.idle_runs("ms", stride)
        for ring_bpc in (1, 4):
            f = P.facts(small["w"], small["capacity"], "ms", cus, ring_bpc=ring_bpc)
            assert P.idle_reaches(f, False) == [] and 4 in P.reaches(f), f
    for ring_bpc in (1, 4):
        full = P.idle_runs_full("ms", 64, cus, ring_bpc)
        f = P.facts(full["w"], full["capacity"], "ms", cus, ring_bpc=ring_bpc)
        assert P.idle_reaches(f, True) == [], {k: v for k, v in f.items() if k not in ("ring_batches", "prefixes")}
    tcp = P.idle_runs("tcp", 64)
    for w in (tcp["w"], tcp["w_paced"]):
        f = P.facts(w, tcp["capacity"], "tcp", cus)
        assert P.idle_descs_reaches(f) == [], f


def _wide_tcp_wants(paced):
    case = P.wide_tcp()
    state = P.tcp_state(case["settings"])
    cut = P.pace_cut(case["pace"], 0, 0) if paced else None
    return case, [P.tcp_tick(state, t["ids"], 16, t["capacity"], t["max_buffers"], cut) for t in case["ticks"]]


@pytest.mark.parametrize("paced", [False, True])
def test_wide_sums_reach_64_bits(paced):
    case, ticks = _wide_tcp_wants(paced)
    for k, (t, got) in enumerate(zip(case["ticks"], ticks)):
        f = P.facts(got["w"], t["capacity"], "tcp")
        assert P.wide_tcp_reaches(k, f) == [], (k, f)
    first = ticks[0]
    assert first["w"][:3] == [2, 1 << 31, 1 << 31] and first["taken"][:3] == [2, 5, 0]
    assert set(first["codes"][2:]) == {3} and first["prefix"][3] == 2 + (1 << 32)
    assert {2, 3} <= set(P.reaches(P.facts(first["w"], 7, "tcp")))
    if paced:  # the rate-limited lane wants what its quantum lets out, far below 2^31
        lane = case["pace"].index(dict(bytes_per_second=300, period_ms=10))
        assert 0 < first["w"][lane] < 10
    ms = P.wide_ms()
    got = P.ms_tick(P.ms_state(ms["settings"]), ms["ids"], 64, ms["capacity"])
    f = P.facts(got["w"], ms["capacity"], "ms")
    assert P.wide_ms_reaches(ms, f) == [], f
    assert P.HUGE_DATAGRAMS * 30 < 1 << 32 < P.HUGE_DATAGRAMS * 53  # why 60 are placed where 30 would do at M = 28
    assert got["codes"] == [0] * 4 + [3] * (len(ms["ids"]) - 4)


# ---- 3. the gap ------------------------------------------------------------------------------------------------------
def test_older_shapes_reach_none_of_the_paths():
    """test_shuffled_lists and test_prefix_seams at 1 100 listed, test_one_connection_many_buffers and test_wide_sums:
    five tiles, prefixes of a few thousand, wants of at most 700, idle runs of two, one pass of every launch."""
    import test_media_stream_servers_gpu as ms_gpu
    import test_tcp_senders_gpu as tcp_gpu

    shapes = []
    settings = tcp_gpu._SETTINGS_1500
    ids = [int(x) for x in np.random.default_rng(1100).permutation(1500) if x not in (11, 700)][:1100]
    ids[5], ids[550], ids[9], ids[1099] = 1500, 0xFFFFFFFF, 11, 700
    for max_buffers in (1, 3):
        got = P.tcp_tick(P.tcp_state(settings, range(0, 1500, 7)), ids, 128, max_buffers * 1100, max_buffers)
        shapes.append(("test_shuffled_lists", got["w"], max_buffers * 1100, "tcp"))
    settings = ms_gpu._SEAM_TABLE
    ids = [int(x) for x in np.random.default_rng(1100).permutation(1500)[:1100]]
    ids[5], ids[550] = 1500, 0xFFFFFFFF
    capacity = sum(-(-settings[c][0] // settings[c][1]) for c in ids if c < 1500)
    got = P.ms_tick(P.ms_state(settings, range(0, 1500, 7)), ids, 128, capacity)
    shapes.append(("test_prefix_seams", got["w"], capacity, "ms"))
    shapes.append(("test_one_connection_many_buffers", [700, 5], 705, "tcp"))
    shapes.append(("test_wide_sums", [5, 5], 12, "tcp"))
    for name, w, capacity, kind in shapes:
        f = P.facts(w, capacity, kind, 256)
        assert P.reaches(f) == [], (name, "reaches the planner paths", P.reaches(f))
        assert f["tiles"] <= 5 and f["carries"] == [0] and f["prefix_max"] < 6000 and f["limb_top"] <= 0, name
        assert f.get("ring_batches_max", 1) == 1 and f.get("descs_passes_max", 1) == 1, name
        idle = "".join("0" if x == 0 else "1" for x in w).split("1")
        assert max(len(run) for run in idle) <= 4, name


# ---- 4. sensitivity --------------------------------------------------------------------------------------------------
def _model_plan(case, w_tick, ids, max_buffers, capacity):
    entries = W.tcp_sender_entries(case["settings"])
    entries["finished"][list(case.get("finished", ()))] = 1
    v = W.tcp_sender_view(entries, case["stride"], np.zeros(capacity * case["stride"], dtype=np.uint8), 0, capacity,
                          ids, max_buffers)
    return [int(x) for x in v.prefix], [int(x) for x in v.taken]


def test_every_defect_is_told_apart():
    told = {}
    # the planners' defects, each on the case built for it; the defect-free plan is the numpy model's
    wide, wide_ticks = _wide_tcp_wants(False)
    long_case = P.long_tcp(65_537)
    last = wide["ticks"][3]  # its list over fresh entries, as _model_plan takes them
    fresh = P.tcp_tick(P.tcp_state(wide["settings"]), last["ids"], 16, 7, 0xFFFFFFFF)["w"]
    plans = {"prefix32": (wide_ticks[0]["w"], 7, wide, wide["ticks"][0]["ids"], 0x80000000),
             "limb_carry": (fresh, 7, wide, last["ids"], 0xFFFFFFFF),
             "no_carry": (long_case["w"], long_case["capacity"], long_case, long_case["ids"], 2)}
    for defect, (w, capacity, case, ids, max_buffers) in plans.items():
        good = P.plan(w, capacity)
        assert good == _model_plan(case, w, ids, max_buffers, capacity), defect
        told[defect] = P.plan(w, capacity, defect) != good
        for other in set(plans) - {defect}:  # and only by its own case's path, where the cases are apart
            if defect == "no_carry":
                assert P.plan(plans[other][0], plans[other][1], defect) == P.plan(plans[other][0], plans[other][1])
    # what the text of the wide case promises of a planner that keeps 32 bits of a prefix: the next small one sends
    assert P.plan(wide_ticks[0]["w"], 7, "prefix32")[1][3] == 2 and P.plan(wide_ticks[0]["w"], 7)[1][3] == 0
    ms = P.wide_ms()
    got = P.ms_tick(P.ms_state(ms["settings"]), ms["ids"], 64, ms["capacity"])
    assert P.plan(got["w"], 64, "prefix32", "ms")[1] != P.plan(got["w"], 64, None, "ms")[1]
    # the consumers' defects leave the plan alone and show in the slots' connections
    idle = P.idle_runs("ms", 64)
    good = P.slot_owners(idle["w"], idle["capacity"], "ms", 256, 4)
    assert P.plan(idle["w"], idle["capacity"], "staged_only", "ms") == P.plan(idle["w"], idle["capacity"], None, "ms")
    told["staged_only"] = P.slot_owners(idle["w"], idle["capacity"], "ms", 256, 4, "staged_only") != good
    two = P.descs_two_passes(4)
    good = P.slot_owners(two["w"], two["capacity"], "tcp", 4, 1)
    told["descs_one_pass"] = P.slot_owners(two["w"], two["capacity"], "tcp", 4, 1, "descs_one_pass") != good
    assert good == _descs_by_loops(two["w"], two["capacity"], 4, 1)[0]
    assert set(told) == set(P.DEFECTS)
    assert all(told.values()), told
    # the older shapes tell none of them apart
    for defect in P.DEFECTS:
        assert P.plan([700, 5], 705, defect) == P.plan([700, 5], 705)
        assert P.slot_owners([700, 5], 705, "tcp", 256, 4, defect) == P.slot_owners([700, 5], 705, "tcp", 256, 4)


def test_plan_is_the_model_on_every_tcp_case():
    cases = [(P.idle_runs("tcp", 64), None), (P.descs_two_passes(64), None)]
    cases += [(P.long_tcp(n), None) for n in P.LONG_LISTED]
    for case, _ in cases:
        assert P.plan(case["w"], case["capacity"]) == _model_plan(case, case["w"], case["ids"], case["max_buffers"],
                                                                   case["capacity"])
    wide, ticks = _wide_tcp_wants(False)
    entries = W.tcp_sender_entries(wide["settings"])
    for t, got in zip(wide["ticks"], ticks):
        v = W.tcp_sender_view(entries, 16, np.zeros(7 * 16, dtype=np.uint8), 0, t["capacity"], t["ids"],
                              t["max_buffers"])
        entries = v.entries
        assert ([int(x) for x in v.prefix], [int(x) for x in v.taken]) == (got["prefix"], got["taken"])
        assert v.codes.tolist() == got["codes"]


# ---- 5. the models at these sizes ------------------------------------------------------------------------------------
def test_tcp_model_on_a_long_list_is_the_loop():
    case = P.long_tcp(65_829)
    state = P.tcp_state(case["settings"], case["finished"])
    entries = W.tcp_sender_entries(case["settings"])
    entries["finished"][::7] = 1
    arena = np.zeros(case["capacity"] * 16, dtype=np.uint8)
    for t in range(2):
        got = P.tcp_tick(state, case["ids"], 16, case["capacity"], 2)
        v = W.tcp_sender_view(entries, 16, arena, 0, case["capacity"], case["ids"], 2)
        entries = v.entries
        assert v.codes.tolist() == got["codes"] and v.tick == got["tick"], t
        assert [int(x) for x in v.prefix] == got["prefix"] and [int(x) for x in v.taken] == got["taken"], t
        for k, f in enumerate(("transfer_bytes", "buffer_size", "bytes_sent", "buffers_sent", "finished")):
            assert entries[f].tolist() == [e[k] for e in state], (t, f)
        assert {0, 1, 2, 3, 4} <= set(got["codes"]) or t


def test_ms_model_on_a_long_list_is_the_loop():
    case = P.long_ms(65_829)
    state = P.ms_state(case["settings"], case["finished"])
    entries = W.media_stream_server_entries(case["settings"])
    entries["finished"][::7] = 1
    view = W.media_stream_server_view(entries, 64, np.zeros(case["capacity"] * 64, dtype=np.uint8), case["capacity"])
    seen = set()
    for t in range(2):
        got = P.ms_tick(state, case["ids"], 64, case["capacity"])
        seen |= set(got["codes"])
        codes, tick = view.send(case["ids"], 5, 7)
        assert codes.tolist() == got["codes"] and tick == got["tick"], t
        assert view.entries["current_frame"].tolist() == [e[3] for e in state]
        assert view.entries["finished"].tolist() == [e[5] for e in state]
    assert {0, 1, 2, 3, 4} <= seen


# ---- 6. the exchange tick on the same cases --------------------------------------------------------------------------
def _exchange_view_ticks(case, ticks, capacity_max):
    """The numpy model and exchange_tick side by side over a case's ticks (ids, max_buffers, capacity): yields
    (k, view, exchange_tick's result)."""
    state = P.exchange_case_state(case)
    entries = P.exchange_records(state)
    arena = np.zeros(max(1, capacity_max) * case["stride"], dtype=np.uint8)
    for k, (ids, max_buffers, capacity) in enumerate(ticks):
        v = W.tcp_exchange_view(entries, case["stride"], arena, 0, capacity, ids, max_buffers)
        got = P.exchange_tick(state, ids, case["stride"], capacity, max_buffers, len(state))
        entries = v.entries
        assert [int(x) for x in v.prefix] == got["prefix"] and [int(x) for x in v.taken] == got["taken"], k
        assert v.codes.tolist() == got["codes"] and v.tick == dict(got["tick"], bytes_dir=got["bytes_dir"]), k
        d = v.descs[: got["tick"]["buffers"]]
        assert list(zip(d["conn_index"].tolist(), d["length"].tolist(),
                        d["expected_pattern_offset"].tolist())) == got["slots"], k
        assert np.array_equal(entries, P.exchange_records(got["entries"])), k
        yield k, v, got


@pytest.mark.parametrize("n_listed", P.LONG_LISTED)
def test_long_exchange_reaches_the_second_pass(n_listed):
    case = P.long_exchange(n_listed)
    f = P.facts(case["w"], case["capacity"], "tcp")
    assert P.long_reaches(case, n_listed, f) == [], f
    assert (1 in P.reaches(f)) == (n_listed > 65_536)
    ids = case["ids"]
    assert ids.count(P.LONG_TABLE) == ids.count(0xFFFFFFFF) == 1 and len(set(ids)) == n_listed
    assert {11, 700, 13} <= set(ids) and case["pattern4"] == (13,)
    state = P.exchange_case_state(case)
    assert {e[P.XP] for e in state} == {0, 1, 2, 3, 4} and sum(e[P.XFIN] for e in state) == len(P.LONG_FINISHED)
    assert [c for c, e in enumerate(state) if e[P.XB] > 16] == [11, 700]
    table = [e for c, e in enumerate(state) if c not in (11, 700)]
    assert {e[P.XN] for e in table} == {1, 2, 3}
    assert all(1 <= e[P.XPUSH] <= 3 * e[P.XB] + 1 and 1 <= e[P.XPULL] <= 3 * e[P.XB] + 1 for e in table)
    for defect in ("prefix32", "limb_carry"):  # a list of wants of 1 and 2 tells neither apart: the wide case does
        assert P.plan(case["w"], case["capacity"], defect) == P.plan(case["w"], case["capacity"])


def test_long_exchange_model_is_the_loop_to_the_end():
    case = P.long_exchange(65_829)
    ticks = [(case["ids"], 2, case["capacity"])] * 4
    seen = set()
    for k, v, got in _exchange_view_ticks(case, ticks, case["capacity"]):
        seen |= set(got["codes"])
        assert k or (got["codes"][-64:].count(3) >= 1 and got["tick"]["buffers"] == case["capacity"])
    assert {0, 1, 2, 3, 4} <= seen and got["tick"]["buffers"] == 0 and set(got["codes"]) == {2, 4}


@pytest.mark.parametrize("cus", CUS)
def test_idle_runs_exchange_reach_the_long_search(cus):
    case = P.idle_runs("exchange", 64)
    f = P.facts(case["w"], case["capacity"], "tcp", cus)
    assert P.idle_descs_reaches(f) == [], f
    if cus != CUS[0]:
        return
    state = P.exchange_case_state(case)
    idle = [state[c] for c, x in zip(case["ids"], case["w"]) if x == 0 and c < len(state)]
    assert sum(e[P.XFIN] for e in idle) > 500 and sum(e[P.XB] > 64 for e in idle) > 500
    assert sum(e[P.XPUSH] == 0 and e[P.XP] == P.PUSHPULL for e in idle) > 500
    assert sum(1 for c in case["ids"] if c >= len(state)) > 500
    ticks = [(case["ids"], 3, case["capacity"])] * 2
    for k, v, got in _exchange_view_ticks(case, ticks, case["capacity"]):
        assert got["w"] == case["w"] and got["tick"]["buffers"] == case["capacity"]
        assert set(got["codes"]) == {k, 2, 4}
        # every PushPull sender's three slots are both directions'
        n = len(state)
        for i, c in enumerate(case["ids"]):
            if case["w"][i] and state[c][P.XP] == P.PUSHPULL:
                mine = got["slots"][got["prefix"][i]: got["prefix"][i] + 3]
                assert {r for r, _, _ in mine} == {c, c + n}, (k, c, mine)


def test_wide_exchange_reaches_64_bits():
    case = P.wide_exchange()
    assert [t["capacity"] for t in case["ticks"]] == [7, 0, 7, 7]
    assert [t["max_buffers"] for t in case["ticks"]] == [0x80000000] + [0xFFFFFFFF] * 3
    state = P.exchange_case_state(case)
    huge = [e for e in state if e[P.XT] == P.HUGE_TRANSFER]
    assert {e[P.XP] for e in huge} == {0, 1, 2, 3} and all(e[P.XN] == 1 << 50 and e[P.XB] == 1 for e in huge)
    assert state[P.WIDE_TCP_LISTED][P.XP] == P.PUSHPULL and state[P.WIDE_TCP_LISTED][3:5] == [5, 3]
    ticks = [(t["ids"], t["max_buffers"], t["capacity"]) for t in case["ticks"]]
    for k, v, got in _exchange_view_ticks(case, ticks, 7):
        f = P.facts(got["w"], ticks[k][2], "tcp")
        assert P.wide_tcp_reaches(k, f) == [], (k, f)
        if k >= 2:
            first = ticks[k][0][0]
            assert got["taken"][0] == 7 and {r for r, _, _ in got["slots"]} == {first, first + len(state)}
    assert [r // len(state) for r, _, _ in got["slots"]] == [1, 0, 0, 0, 0, 0, 1]


def test_every_planner_defect_shows_in_an_exchange_case():
    """prefix32 and limb_carry on the wide case, no_carry on the long list, descs_one_pass on the long list at four
    compute units and one workgroup per CU: each changes what a GPU test compares."""
    told = {}
    wide = P.wide_exchange()
    for defect, k in (("prefix32", 0), ("limb_carry", 3)):
        outcomes = []
        for d in (None, defect):
            state = P.exchange_case_state(wide)
            for t in wide["ticks"][:k + 1]:
                got = P.exchange_tick(state, t["ids"], 16, t["capacity"], t["max_buffers"], len(state), d)
            outcomes.append((got["prefix"], got["taken"], got["codes"], got["slots"], got["entries"]))
        told[defect] = outcomes[0] != outcomes[1]
    long_case = P.long_exchange(65_537)
    outcomes = []
    for d in (None, "no_carry"):
        got = P.exchange_tick(P.exchange_case_state(long_case), long_case["ids"], 16, long_case["capacity"], 2,
                              P.LONG_TABLE, d)
        outcomes.append((got["prefix"], got["taken"], got["codes"], got["entries"]))
    told["no_carry"] = outcomes[0] != outcomes[1]
    w, capacity = long_case["w"], long_case["capacity"]
    good = P.slot_owners(w, capacity, "tcp", 4, 1)
    assert None not in good and P.facts(w, capacity, "tcp", 4, blocks_per_cu=1)["descs_passes_max"] > 1
    told["descs_one_pass"] = P.slot_owners(w, capacity, "tcp", 4, 1, "descs_one_pass") != good
    assert all(told.values()) and set(told) == set(P.DEFECTS) - {"staged_only"}, told
