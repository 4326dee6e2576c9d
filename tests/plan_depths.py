"""Shared by tests/test_plan_depths_cpu.py and tests/test_plan_depth_gpu.py (CPU only, no device, no torch).

The three device-resident senders (cts_media_stream_servers_send, cts_tcp_senders_send, cts_tcp_senders_send_paced)
plan a tick the same way: a sum of wants per tile of 256 listed connections, a single-workgroup scan of the tile sums
in passes of 256 tiles with a carry, and an apply pass that turns the 64-bit exclusive prefix into slots. Two consumers
search that prefix for the listed connection of every tick-local slot: ms_server_fill (513 staged prefixes per batch of
512 datagrams, prefix[] itself beyond them) and tcp_sender_descs (one lane per slot, grid-stride, a binary search of
all of prefix[]). This module restates that planning one item at a time in Python integers, so a test can assert which
of its paths a tick reaches before it compares a device result:

  1  the scan's second pass (more than 256 tiles: a non-zero carry, the tile scan called again)
  2  prefixes and wants above 2^32 beside a capacity below it
  3  16-bit limb sums of a wave of wants that carry into the next limb
  4  ms_server_fill's search of prefix[] beyond the staged window, and first_listed handed over from it
  5  tcp_sender_descs' second grid-stride pass, and its search over a long prefix[]

The grid rules are tests/launch_depths.py's (held against cts_grids.hpp there). The numpy models of
ctstraffic_amd/workload.py are the reference for outcomes and are not called here. The cases of the two test files
live here too.

The exchange tick (cts_tcp_exchange_send: tcp_exchange_sums / _scan / _apply and tcp_exchange_descs) plans the same
way and has its cases at the end: long_exchange, idle_runs("exchange", ...) and wide_exchange. Its reference is
exchange_tick, the whole tick one listed connection at a time in Python integers (buffers from
workload.tcp_exchange_element, positions from workload.tcp_exchange_position, never the numpy model), which
tests/exchange_edges.py uses as well.
"""
import bisect

import numpy as np

import launch_depths as L

TILE = 256           # listed connections per tile (kPlanTile)
SCAN_BLOCK = 256     # tile sums per pass of tick_plan_scan (kBlock)
WAVE = 64
RING_BATCH = L.RING_BATCH
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
DEFECTS = ("prefix32", "no_carry", "limb_carry", "staged_only", "descs_one_pass")
RING_BPC_DEFAULT, BLOCKS_PER_CU_DEFAULT = 4, 4  # LaunchGeometry's ring_fill_blocks_per_cu and blocks_per_cu


# ---- the planner -----------------------------------------------------------------------------------------------------
def _wave_sum(wants, defect=None):
    """A wave's exact 64-bit sum by a route of its own: four 16-bit limbs, each summed over the wave's lanes in 32
    bits. The kernels use wave_sum64."""
    s = 0
    for limb in range(4):
        lanes = sum((v >> (16 * limb)) & 0xFFFF for v in wants)
        if defect == "limb_carry":
            lanes &= 0xFFFF
        s += lanes << (16 * limb)
    return s & M64


def tile_sums(w, defect=None):
    """*_sums: sums[tile], the four waves' sums added."""
    out = []
    for t0 in range(0, len(w), TILE):
        waves = range(t0, min(t0 + TILE, len(w)), WAVE)
        out.append(sum(_wave_sum(w[v0:v0 + WAVE], defect) for v0 in waves) & M64)
    return out


def scan(sums, defect=None):
    """tick_plan_scan: (exclusive scan of the tile sums, the carry entering each pass, grand total)."""
    out, carries, carry = [], [], 0
    for base in range(0, len(sums), SCAN_BLOCK):
        if defect == "no_carry" and base > 0:
            carry = 0
        carries.append(carry)
        run = 0
        for v in sums[base:base + SCAN_BLOCK]:
            out.append((carry + run) & M64)
            run += v
        carry = (carry + run) & M64
    return out, carries, carry


def plan(w, capacity, defect=None, kind="tcp"):
    """(prefix, taken) per listed connection from its wants w, as *_apply leaves them. kind "tcp": a connection takes
    min(w, capacity - min(p, capacity)); "ms": all of w when p + w <= capacity, else nothing. defect: what a planner
    with that one fault would give. "staged_only" and "descs_one_pass" are faults of the consumers: the plan itself is
    the defect-free one, and slot_owners() shows them."""
    assert defect is None or defect in DEFECTS
    ex, _, _ = scan(tile_sums(w, defect), defect)
    prefix, taken = [], []
    for i, want in enumerate(w):
        if i % TILE == 0:
            p = ex[i // TILE]
        if defect == "prefix32":
            p &= M32
        prefix.append(p)
        if kind == "ms":
            taken.append(want if want and p + want <= capacity else 0)
        else:
            taken.append(min(want, capacity - min(p, capacity)))
        p = (p + want) & M64
    return prefix, taken


def _listed(prefix, lo, hi, g):
    """ms_server_listed: the last i in [lo, hi) with prefix[i] <= g, and the steps of its loop."""
    steps = 0
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if prefix[mid] <= g:
            lo = mid
        else:
            hi = mid
        steps += 1
    return lo, steps


def ring_split(total, capacity, cus, ring_bpc):
    """ms_server_fill's (grid, per_wg): ring_fill_grid over the capacity, at least a batch per workgroup."""
    grid = L.batch_fill_grid(capacity, RING_BATCH, cus, ring_bpc)
    even = (total + grid - 1) // grid if grid else 0
    return grid, max(even, min(total, RING_BATCH))


def slot_owners(w, capacity, kind, cus, bpc, defect=None):
    """The listed connection each tick-local slot's consumer finds, one workgroup, batch and lane at a time:
    ms_server_fill (kind "ms", bpc = the ring-fill blocks per CU) or tcp_sender_descs (kind "tcp", bpc = blocks per
    CU). None: the slot keeps its old descriptor."""
    prefix, taken = plan(w, capacity, None, kind)
    n, total = len(w), min(sum(taken), capacity)
    prefix = prefix + [sum(w) & M64]
    out = [None] * total
    if total == 0 or capacity == 0:
        return out
    if kind == "tcp":
        grid = L.grid_for((capacity + L.BLOCK - 1) // L.BLOCK, 1, cus, bpc)
        for lane in range(grid * L.BLOCK):
            for g in range(lane, total, grid * L.BLOCK):
                if defect == "descs_one_pass" and g != lane:
                    break
                out[g] = _listed(prefix, 0, n, g)[0]
        return out
    grid, per_wg = ring_split(total, capacity, cus, bpc)
    for b in range(grid):
        g0 = b * per_wg
        if g0 >= total:
            break
        g1 = min(g0 + per_wg, total)
        first_listed = _listed(prefix, 0, n, g0)[0]
        for d0 in range(g0, g1, RING_BATCH):
            nb = min(g1 - d0, RING_BATCH)
            i0 = first_listed
            ps = [prefix[min(i0 + t, n)] for t in range(RING_BATCH + 1)]
            for t in range(nb):
                g = d0 + t
                lo = _listed(ps, 0, RING_BATCH + 1, g)[0]
                i = i0 + lo
                if lo == RING_BATCH and i + 1 < n and defect != "staged_only":
                    i = _listed(prefix, i, n, g)[0]
                out[g] = i = min(i, n - 1)
                if t == nb - 1:
                    first_listed = i
    return out


def _search_steps(o, n):
    """Steps of ms_server_listed(prefix, 0, n, g) for a slot of listed connection o: the comparisons depend on o alone
    (prefix[mid] <= g exactly when mid <= o)."""
    lo, hi, steps = 0, n, 0
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if mid <= o:
            lo = mid
        else:
            hi = mid
        steps += 1
    return steps


def facts(w, capacity, kind="tcp", cus=None, ring_bpc=RING_BPC_DEFAULT, blocks_per_cu=BLOCKS_PER_CU_DEFAULT):
    """Which planner paths a tick of wants w reaches.

    tiles, scan_passes, carries          the scan: passes of 256 tiles, the carry entering each
    prefix_max, grand_total              the largest p_i and the sum of all wants
    wide_prefixes, beyond_capacity       listed connections with p_i >= 2^32, with capacity < p_i
    limb_top                             the highest non-zero 16-bit limb of any want (-1: all wants are 0)
    limb_carries                         the limbs whose 64-lane sum exceeds 0xFFFF in some wave
    prefixes                             every p_i
    total                                the tick's slots
    with cus, kind "ms" (ms_server_fill at ring_bpc):
      ring_grid, ring_per_wg, ring_batches_max
      ring_batches                       per workgroup with datagrams, per batch: (d0, nb, i0, staged_max, fallback,
                                         moved, exact, handed_over) -- staged_max the most staged prefixes <= g of any
                                         of its datagrams; fallback / moved / exact counts of its datagrams that enter
                                         the search of prefix[] (lo == 512 and i + 1 < n), that it moves past i0 + 512,
                                         that it leaves at i0 + 512; handed_over: i0 is a connection the search moved to
      fallback, moved, exact             their sums
      handovers                          batches with handed_over
      later_workgroup_moved              datagrams with `moved` in workgroups other than the first
    with cus, kind "tcp" (tcp_sender_descs at blocks_per_cu):
      descs_grid, descs_passes_max      the grid and the most slots any lane takes
      descs_later_slots                 slots taken in a lane's second and later passes
      search_steps_max                  the longest binary search of prefix[0 .. n)
      owner_gap_max                     the most listed positions between two neighbouring slots' connections
    """
    n = len(w)
    sums = tile_sums(w)
    _, carries, grand = scan(sums)
    prefix, taken = plan(w, capacity, None, kind)
    total = min(sum(taken), capacity)
    top, carrying = -1, set()
    for v0 in range(0, n, WAVE):
        for limb in range(4):
            lanes = [(v >> (16 * limb)) & 0xFFFF for v in w[v0:v0 + WAVE]]
            if any(lanes):
                top = max(top, limb)
            if sum(lanes) > 0xFFFF:
                carrying.add(limb)
    out = {"tiles": len(sums), "scan_passes": (len(sums) + SCAN_BLOCK - 1) // SCAN_BLOCK, "carries": carries,
           "prefix_max": max(prefix) if n else 0, "grand_total": grand,
           "wide_prefixes": sum(1 for p in prefix if p >= 1 << 32),
           "beyond_capacity": sum(1 for p in prefix if p > capacity), "limb_top": top,
           "limb_carries": sorted(carrying), "total": total, "prefixes": prefix}
    if cus is None or total == 0:
        return out
    owners = [i for i in range(n) if taken[i] > 0]  # their slots [prefix[i], prefix[i] + taken[i]) tile [0, total)
    starts = [prefix[i] for i in owners]
    if kind == "tcp":
        grid = L.grid_for((capacity + L.BLOCK - 1) // L.BLOCK, 1, cus, blocks_per_cu)
        out.update(descs_grid=grid, descs_passes_max=(total + grid * L.BLOCK - 1) // (grid * L.BLOCK),
                   descs_later_slots=max(0, total - grid * L.BLOCK),
                   search_steps_max=max(_search_steps(o, n) for o in owners),
                   owner_gap_max=max([b - a for a, b in zip(owners, owners[1:])] or [0]))
        return out
    grid, per_wg = ring_split(total, capacity, cus, ring_bpc)
    per_workgroup = []
    for b in range(grid):
        g0 = b * per_wg
        if g0 >= total:
            break
        g1 = min(g0 + per_wg, total)
        i0, found_by_search, batches = owners[bisect.bisect_right(starts, g0) - 1], False, []
        for d0 in range(g0, g1, RING_BATCH):
            d1 = min(d0 + RING_BATCH, g1)
            staged = fallback = moved = exact = 0
            k = bisect.bisect_right(starts, d0) - 1
            last_moved = False
            while k < len(owners) and starts[k] < d1:
                o = owners[k]
                count = min(d1, starts[k] + taken[o]) - max(d0, starts[k])
                rel = o - i0
                staged = max(staged, min(rel, RING_BATCH) + 1)
                last_moved = False
                if rel >= RING_BATCH and i0 + RING_BATCH + 1 < n:
                    fallback += count
                    if rel > RING_BATCH:
                        moved += count
                        last_moved = True
                    else:
                        exact += count
                k += 1
            batches.append((d0, d1 - d0, i0, staged, fallback, moved, exact, found_by_search))
            i0, found_by_search = owners[k - 1], last_moved
        per_workgroup.append(batches)
    flat = [x for batches in per_workgroup for x in batches]
    out.update(ring_grid=grid, ring_per_wg=per_wg, ring_batches=per_workgroup,
               ring_batches_max=max(len(x) for x in per_workgroup), fallback=sum(x[4] for x in flat),
               moved=sum(x[5] for x in flat), exact=sum(x[6] for x in flat), handovers=sum(1 for x in flat if x[7]),
               later_workgroup_moved=sum(x[5] for batches in per_workgroup[1:] for x in batches))
    return out


def reaches(f):
    """The paths 1 to 5 a tick's facts reach."""
    got = set()
    if f["scan_passes"] > 1:
        got.add(1)
    if f["wide_prefixes"] > 0:
        got.add(2)
    if f["limb_carries"]:
        got.add(3)
    if f.get("fallback", 0) > 0:
        got.add(4)
    if f.get("descs_passes_max", 1) > 1:
        got.add(5)
    return sorted(got)


# ---- one connection at a time: the wants, and the tick they lead to --------------------------------------------------
def tcp_tick(state, ids, stride, capacity, max_buffers, cut=None, defect=None):
    """One tick of cts_tcp_senders_send over state (a list of [transfer, B, bytes_sent, buffers_sent, finished], moved
    in place), one listed connection at a time. cut(c, limit, R, B) -> the slots pacing lets connection c want.
    Returns {"w", "prefix", "taken", "codes", "tick"}."""
    w, codes = [], []
    for c in ids:
        want, code = 0, 4
        if c < len(state):
            transfer, B, sent, _, finished = state[c]
            if 0 < B <= stride:
                code = 2
                if not finished and sent < transfer:
                    R = transfer - sent
                    want, code = min(-(-R // B), max_buffers), 0
                    if cut is not None:
                        want = cut(c, want, R, B)
                        code = 0 if want else 5
        w.append(want)
        codes.append(code)
    prefix, taken = plan(w, capacity, defect, "tcp")
    tick = dict.fromkeys(("bytes", "buffers", "connections_sent", "connections_finished", "connections_no_room",
                          "connections_skipped"), 0)
    for i, c in enumerate(ids):
        if codes[i] in (2, 4):
            tick["connections_skipped"] += 1
        elif codes[i] == 0 and taken[i] == 0:
            codes[i] = 3
            tick["connections_no_room"] += 1
        elif codes[i] == 0:
            e = state[c]
            moved = min(taken[i] * e[1], e[0] - e[2])
            e[2] += moved
            e[3] += taken[i]
            tick["bytes"] += moved
            tick["buffers"] += taken[i]
            tick["connections_sent"] += 1
            if e[2] == e[0]:
                e[4], codes[i] = 1, 1
                tick["connections_finished"] += 1
    return {"w": w, "prefix": prefix, "taken": taken, "codes": codes, "tick": tick}


def ms_tick(state, ids, stride, capacity, defect=None):
    """One tick of cts_media_stream_servers_send over state (a list of [F, M, k, current_frame, final_frame, finished],
    moved in place), one listed connection at a time."""
    w, codes = [], []
    for c in ids:
        want, code = 0, 4
        if c < len(state):
            _, M_, k, _, _, finished = state[c]
            if finished:
                code = 2
            elif M_ <= stride:
                want, code = k, 0
        w.append(want)
        codes.append(code)
    prefix, taken = plan(w, capacity, defect, "ms")
    tick = dict.fromkeys(("bytes", "datagrams", "connections_sent", "connections_finished", "connections_no_room",
                          "connections_skipped"), 0)
    for i, c in enumerate(ids):
        if codes[i] != 0:
            tick["connections_skipped"] += 1
        elif taken[i] == 0:
            codes[i] = 3
            tick["connections_no_room"] += 1
        else:
            e = state[c]
            e[3] += 1
            tick["bytes"] += e[0]
            tick["datagrams"] += e[2]
            tick["connections_sent"] += 1
            if e[3] > e[4]:
                e[5], codes[i] = 1, 1
                tick["connections_finished"] += 1
    return {"w": w, "prefix": prefix, "taken": taken, "codes": codes, "tick": tick}


def tcp_state(settings, finished=()):
    state = [[t, b, 0, 0, 0] for t, b in settings]
    for c in finished:
        state[c][4] = 1
    return state


def ms_state(settings, finished=()):
    state = [[F, m, -(-F // m), 1, final, 0] for F, m, final in settings]
    for c in finished:
        state[c][5] = 1
    return state


def pace_cut(pace_settings, start_ms, now_ms):
    """cut() of tcp_tick for a paced tick at now_ms over fresh pace entries: run(limit) of include/cts_tcp_senders.h,
    the per-connection Python-integer machine of ctstraffic_amd/workload.py (not one of its numpy models)."""
    from ctstraffic_amd import workload as W

    q = W.tcp_sender_pace_entries(pace_settings, start_ms)

    def cut(c, limit, R, B):
        e = {f: int(q[c][f]) for f in W._PACE_SCALARS}
        if e["bytes_per_quantum"] == 0 and e["burst_count"] == 0 and not e["pending"]:
            return limit
        return W._pace_run(e, now_ms, limit, R, B)

    return cut


def pace_by_turns(settings):
    """Pace settings beside (transfer, B) settings: unpaced, 1.5 buffers per 10 ms quantum, two sends then 7 ms, by
    turns (the table of tests/test_tcp_paced_senders_gpu.py's shuffled lists)."""
    return [[{}, dict(bytes_per_second=150 * B, period_ms=10), dict(burst_count=2, burst_delay_ms=7)][c % 3]
            for c, (_, B) in enumerate(settings)]


# ---- A. long lists ---------------------------------------------------------------------------------------------------
LONG_TABLE = 66_000
LONG_LISTED = (65_536, 65_537, 65_829)  # 256 full tiles; a second pass of one connection; of two tiles, the last ragged
LONG_FINISHED = range(0, LONG_TABLE, 7)


def _long_ids(n_listed, wide=()):
    rng = np.random.default_rng(n_listed)
    ids = [int(x) for x in rng.permutation(LONG_TABLE) if x not in wide][:n_listed]
    ids[5], ids[n_listed // 2] = LONG_TABLE, 0xFFFFFFFF
    for k, c in enumerate(wide):
        ids[9 + 20 * k] = c
    if n_listed > 65_536:  # a connection that sends (unpaced where there is a pace table) behind the scan's first pass
        listed = set(ids)
        ids[65_536] = next(c for c in range(3, LONG_TABLE, 3) if c % 7 and c not in wide and c not in listed)
    return ids


_LONG_CACHE = {}


def long_tcp(n_listed, paced=False):
    """Case A for the TCP senders: stride 16, B in 1..16, transfers of 1 to 3 buffers, max_buffers 2, two connections
    with B above the stride; the capacity is the first tick's wants less 5. Paced: unpaced, rate-limited and burst
    entries by turns, ticks at start and start + 4."""
    key = ("tcp", n_listed, paced)
    if key in _LONG_CACHE:
        return _LONG_CACHE[key]
    rng = np.random.default_rng(15)
    settings = []
    for c in range(LONG_TABLE):
        B = int(rng.integers(1, 17))
        k = 1 + c % 3
        settings.append((int(rng.integers((k - 1) * B + 1, k * B + 1)), B))
    settings[11], settings[700] = (1000, 200), (5000, 129)
    pace = pace_by_turns(settings)
    ids = _long_ids(n_listed, wide=(11, 700))
    case = {"settings": settings, "pace": pace, "finished": LONG_FINISHED, "ids": ids, "stride": 16, "max_buffers": 2,
            "start": 100, "times": (100, 104)}
    cut = pace_cut(pace, 100, 100) if paced else None
    first = tcp_tick(tcp_state(settings, LONG_FINISHED), ids, 16, M32, 2, cut)
    case["w"], case["capacity"] = first["w"], sum(first["w"]) - 5
    _LONG_CACHE[key] = case
    return case


def long_ms(n_listed):
    """Case A for the MediaStream servers: stride 64, M = 53, frames of 1 or 2 datagrams, streams of 1 to 4 frames; the
    capacity is the first tick's wants less 3."""
    key = ("ms", n_listed)
    if key in _LONG_CACHE:
        return _LONG_CACHE[key]
    rng = np.random.default_rng(16)
    settings = []
    for c in range(LONG_TABLE):
        k = 1 + c % 2
        settings.append((max(27, int(rng.integers((k - 1) * 53 + 1, k * 53 + 1))), 53, 1 + c % 4))
    ids = _long_ids(n_listed)
    first = ms_tick(ms_state(settings, LONG_FINISHED), ids, 64, M32)
    case = {"settings": settings, "finished": LONG_FINISHED, "ids": ids, "stride": 64, "w": first["w"],
            "capacity": sum(first["w"]) - 3}
    _LONG_CACHE[key] = case
    return case


def long_reaches(case, n_listed, f):
    """The facts case A exists for that f does not reach (empty: the test may run)."""
    passes = 1 if n_listed <= TILE * SCAN_BLOCK else 2
    want = {"scan_passes": f["scan_passes"] == passes, "tiles": f["tiles"] == -(-n_listed // TILE),
            "capacity_cuts_the_tail": 0 < f["total"] <= case["capacity"] < f["grand_total"]}
    if passes == 2:
        want.update(carry_is_not_zero=f["carries"][1] > 0, a_sender_behind_the_first_pass=any(case["w"][65_536:]),
                    prefixes_behind_the_first_pass=f["grand_total"] > f["carries"][1])
    return sorted(k for k, ok in want.items() if not ok)


def descs_two_passes(cus):
    """Path 5: 300 TCP connections at stride 16 on an engine with blocks-per-CU 1, each sending max_buffers buffers of
    16 bytes and less, so many that tcp_sender_descs' grid (at most cus workgroups) takes the tick's slots in more
    than one pass; the capacity lies 1 000 slots above the tick's total."""
    conns = 300
    max_buffers = (cus * L.BLOCK + 333) // (conns - 30) + 1
    settings = [(16 * max_buffers * 2 - 5, 16) if c % 10 else (13 * (c % 7 + 1), 13) for c in range(conns)]
    ids = [int(x) for x in np.random.default_rng(5).permutation(conns)]
    first = tcp_tick(tcp_state(settings), ids, 16, M32, max_buffers)
    return {"settings": settings, "ids": ids, "stride": 16, "max_buffers": max_buffers, "w": first["w"],
            "capacity": sum(first["w"]) + 1000, "blocks_per_cu": 1}


def descs_reaches(f):
    want = {"two_passes": f["descs_passes_max"] >= 2, "slots_in_the_second_pass": f["descs_later_slots"] > L.BLOCK,
            "capacity_above_the_total": f["total"] == f["grand_total"]}
    return sorted(k for k, ok in want.items() if not ok)


# ---- B. idle runs ----------------------------------------------------------------------------------------------------
IDLE_RUNS = (511, 512, 513, 1500)
S_SLOTS = 3


def idle_run_tokens(lead, total, filler, kinds=3):
    """The list of case B as tokens ("send", slots) and ("idle", kind): fillers that send `lead` slots in all, then
    [S, idle x 511, S, idle x 512, S, idle x 513, S, idle x 1500, S, S, idle x 700] with S sending 3 and the `kinds`
    idle kinds taking turns, then fillers up to `total` slots. A filler sends `filler` slots, the last of a stretch
    less."""
    def fill(slots):
        return [("send", filler)] * (slots // filler) + ([("send", slots % filler)] if slots % filler else [])

    out, kind = fill(lead), 0
    for run in IDLE_RUNS:
        out.append(("send", S_SLOTS))
        out += [("idle", (kind + j) % kinds) for j in range(run)]
        kind += run
    out += [("send", S_SLOTS), ("send", S_SLOTS)] + [("idle", j % kinds) for j in range(700)]
    return out + fill(total - lead - 6 * S_SLOTS)


def idle_runs(kind, stride, lead=0, total=6 * S_SLOTS + 170 * S_SLOTS, filler=S_SLOTS):
    """Case B: settings, ids and wants of idle_run_tokens. kind "ms": M = 53 at stride 64 and 1040 at 1040, a frame of
    `slots` datagrams, its last one short on every second connection. kind "tcp": B = stride - 3, max_buffers 3. The
    idle kinds: a finished connection, an id beyond the table, a datagram (or buffer) size above the stride. kind
    "exchange": see _idle_runs_exchange."""
    if kind == "exchange":
        return _idle_runs_exchange(stride, lead, total, filler)
    tokens = idle_run_tokens(lead, total, filler)
    settings, finished, ids, w = [], [], [], []
    beyond = 0
    m = 53 if stride < 1040 else 1040
    for what, x in tokens:
        c = len(settings)
        if what == "idle" and x == 1:
            ids.append(len(tokens) + beyond)  # beyond the table, which is shorter than the list
            beyond += 1
            w.append(0)
            continue
        ids.append(c)
        w.append(x if what == "send" else 0)
        slots = x if what == "send" else 2
        size = stride + 16 if what == "idle" and x == 2 else (m if kind == "ms" else stride - 3)
        if kind == "ms":
            settings.append((size * slots - (0 if c % 2 else 20), size, 2))
        else:
            settings.append((size * slots - c % 5, size))
        if what == "idle" and x == 0:
            finished.append(c)
    case = {"settings": settings, "finished": finished, "ids": ids, "stride": stride, "w": w, "capacity": total,
            "max_buffers": 3}
    if kind == "tcp":  # and what the pace table lets out of the same list at its start
        case["pace"], case["start"] = pace_by_turns(settings), 100
        paced = tcp_tick(tcp_state(settings, finished), ids, stride, total, 3, pace_cut(case["pace"], 100, 100))
        case["w_paced"] = paced["w"]
    return case


def idle_runs_full(kind, stride, cus, ring_bpc):
    """Case B with the runs at the start of the second workgroup's first batch, every workgroup walking a batch of 512
    and a short one: the last datagram of that batch lies behind all the runs, so the next batch starts from a
    first_listed the search of prefix[] produced."""
    total = RING_BATCH * cus * ring_bpc + 77
    _, per_wg = ring_split(total, total, cus, ring_bpc)
    return idle_runs(kind, stride, lead=per_wg, total=total, filler=128)


def idle_reaches(f, full):
    """The facts case B exists for that f does not reach: the search of prefix[] is entered, it moves i past the staged
    window, and one datagram's connection is the window's very last entry (the 513 staged prefixes all <= g after the
    run of 511 behind the batch's first connection; the search is entered and stays). full: a batch starts from a
    first_listed that the search moved, in a workgroup other than the first."""
    want = {"fallback_taken": f["fallback"] > 0, "fallback_moves": f["moved"] > 0,
            "window_of_513_exact": f["exact"] == S_SLOTS,
            "all_staged": any(x[3] == RING_BATCH + 1 for b in f["ring_batches"] for x in b)}
    if full:
        want.update(handover_from_the_fallback=f["handovers"] > 0, two_batches=f["ring_batches_max"] >= 2,
                    a_later_workgroup_searches=f["later_workgroup_moved"] > 0)
    return sorted(k for k, ok in want.items() if not ok)


def idle_descs_reaches(f):
    """Case B through tcp_sender_descs: the search runs over thousands of prefixes with every idle run between two
    slots' connections."""
    want = {"search_of_11_steps": f["search_steps_max"] >= 11, "runs_between_owners": f["owner_gap_max"] > 1500,
            "two_workgroups": f["descs_grid"] >= 2}
    return sorted(k for k, ok in want.items() if not ok)


# ---- C. wide sums ----------------------------------------------------------------------------------------------------
HUGE_TRANSFER = 1 << 50
WIDE_TCP_LISTED = 132


def wide_tcp():
    """Case C for the TCP senders: stride 16, B = 1; `small` connections want 2, `huge` ones (2^50 bytes) 2^31 at
    max_buffers 0x80000000 and 0xFFFFFFFF at max_buffers 0xFFFFFFFF. 296 connections: the list of tick 1 and 2 is
    [small, huge, huge] + [small, small, huge] x 43; connections 132..195 are 64 more huge ones, one wave of tick 3;
    196..295 are small. Tick 4 lists that wave first, then everything else: a tile sum only shows in the prefixes of
    the tiles behind it (and in prefix[n]), so the limb sums of the first tile's waves show in the second tile's.
    The first huge connection from 70 on is rate-limited to 3 bytes per 10 ms in the paced table."""
    kinds = ["s", "h", "h"] + ["s", "s", "h"] * 43
    settings = [(2, 1) if k == "s" else (HUGE_TRANSFER, 1) for k in kinds] + [(HUGE_TRANSFER, 1)] * 64 + [(2, 1)] * 100
    pace = [{} for _ in settings]
    pace[kinds.index("h", 70)] = dict(bytes_per_second=300, period_ms=10)
    ticks = [dict(ids=list(range(WIDE_TCP_LISTED)), max_buffers=0x80000000, capacity=7),
             dict(ids=list(range(WIDE_TCP_LISTED)), max_buffers=0xFFFFFFFF, capacity=0),
             dict(ids=list(range(WIDE_TCP_LISTED, WIDE_TCP_LISTED + 64)), max_buffers=0xFFFFFFFF, capacity=7),
             dict(ids=list(range(WIDE_TCP_LISTED, WIDE_TCP_LISTED + 64)) + list(range(WIDE_TCP_LISTED)) +
                  list(range(WIDE_TCP_LISTED + 64, len(settings))), max_buffers=0xFFFFFFFF, capacity=7)]
    return {"settings": settings, "pace": pace, "stride": 16, "ticks": ticks, "capacity": 7, "start": 0,
            "times": (0, 0, 0, 0)}


def wide_tcp_reaches(k, f):
    """The facts tick k of wide_tcp exists for that f does not reach."""
    if k == 0:    # [2, 2^31, 2^31, 2, 2, ...]: the two huge wants are 2^32 together
        want = {"prefixes_above_2^32": f["wide_prefixes"] >= WIDE_TCP_LISTED - 3, "seven_slots": f["total"] == 7,
                "all_but_two_beyond_the_capacity": f["beyond_capacity"] == WIDE_TCP_LISTED - 2,
                "limb_1_carries": f["limb_carries"] == [1], "three_waves": f["tiles"] == 1 and WIDE_TCP_LISTED > 128}
    elif k == 1:  # wants of 0xFFFFFFFF, capacity 0
        want = {"nothing_sent": f["total"] == 0, "limbs_0_and_1": f["limb_top"] == 1 and 1 in f["limb_carries"],
                "prefixes_above_2^32": f["wide_prefixes"] >= WIDE_TCP_LISTED - 5}
    elif k == 3:  # that wave in front of a second tile
        want = {"both_limbs_carry": f["limb_carries"] == [0, 1], "two_tiles": f["tiles"] == 2,
                "seven_slots": f["total"] == 7,
                "second_tile_above_2^32": min(f["prefixes"][TILE:]) > 64 * 0xFFFFFFFF}
    else:         # one wave of 0xFFFFFFFF: limbs 0 and 1 are 0xFFFF in every lane
        want = {"both_limbs_carry": f["limb_carries"] == [0, 1] and f["limb_top"] == 1, "seven_slots": f["total"] == 7,
                "grand_total": f["grand_total"] == 64 * 0xFFFFFFFF}
    return sorted(name for name, ok in want.items() if not ok)


def wide_ms_reaches(case, f):
    smalls_behind = sum(1 for k in case["kinds"][case["kinds"].index("h"):] if k == "s")
    want = {"prefixes_above_2^32": f["wide_prefixes"] >= 40, "leading_four_send": f["total"] == 8,
            "smalls_behind_a_huge_one": smalls_behind >= 50, "a_limb_carries": f["limb_carries"] != [],
            "prefix_mod_2^32_has_room": any(p >= 1 << 32 and (p & M32) + 2 <= case["capacity"] for p in f["prefixes"])}
    return sorted(name for name, ok in want.items() if not ok)


HUGE_FRAME, MIN_DATAGRAM = 0xFFFFFFFF, 53
HUGE_DATAGRAMS = -(-HUGE_FRAME // MIN_DATAGRAM)  # 81 037 119: 53 of them are 2^32 + 11


def wide_ms():
    """Case C for the MediaStream servers at stride 64: frames of 0xFFFFFFFF bytes in datagrams of 53 (the smallest
    the project takes; 53 such frames are 2^32 + 11 datagrams, so 60 are placed, not 30) between frames of 2
    datagrams. Four small ones lead and send; the capacity of 64 is far below any huge frame, so no huge one fits and
    every small one behind the first huge one gets code 3. Behind 53 huge ones the prefix modulo 2^32 is back under
    the capacity."""
    kinds = ["s"] * 4
    for j in range(60):
        kinds.append("h")
        if j % 10 == 9 or j == 52:
            kinds += ["s", "s"]
    kinds += ["s"] * 40
    settings = [(100, 53, 3) if k == "s" else (HUGE_FRAME, MIN_DATAGRAM, 3) for k in kinds]
    return {"settings": settings, "finished": (), "ids": list(range(len(kinds))), "stride": 64, "capacity": 64,
            "kinds": kinds}


# ---- the exchange tick (cts_tcp_exchange_send): Push, Pull, PushPull and Duplex --------------------------------------
# A connection is a list [pattern, T, B, P, Q, N, m, bytes of direction 0, of direction 1, finished] of Python integers.
XP, XT, XB, XPUSH, XPULL, XN, XM, XS0, XS1, XFIN = range(10)
PUSH, PULL, PUSHPULL, DUPLEX = range(4)
X_DEFECTS = ("kp32", "c32", "k32", "m48", "n32")
M48 = (1 << 48) - 1


def exchange_state(settings, seek=None, finished=(), pattern4=(), no_push=()):
    """The entries of cts_tcp_exchange_init (seek: then moved to that position) for (pattern, T, B[, P, Q]) settings.
    finished, pattern4, no_push: entries overwritten afterwards as finished, with pattern 4, with push_bytes 0."""
    from ctstraffic_amd import workload as W

    state = []
    for c, s in enumerate(settings):
        pattern, T, B = s[:3]
        Pb, Qb = (tuple(s[3:5]) + (0, 0))[:2]
        if pattern == DUPLEX:
            T += T % 2
        N = W.tcp_exchange_total_buffers(pattern, T, B, Pb, Qb)
        m = 0 if seek is None else int(seek[c])
        assert 0 <= m <= N, (c, m, N)
        s0, s1 = W.tcp_exchange_position(pattern, T, B, Pb, Qb, m)
        state.append([pattern, T, B, Pb, Qb, N, m, s0, s1, int(m == N)])
    for c in finished:
        state[c][XFIN] = 1
    for c in pattern4:
        state[c][XP] = 4
    for c in no_push:
        state[c][XPUSH] = 0
    return state


def exchange_case_state(case):
    return exchange_state(case["settings"], case.get("seek"), case.get("finished", ()), case.get("pattern4", ()),
                          case.get("no_push", ()))


def exchange_records(state):
    """state as TCP_EXCHANGE_DTYPE records."""
    from ctstraffic_amd.types import TCP_EXCHANGE_DTYPE

    out = np.zeros(len(state), dtype=TCP_EXCHANGE_DTYPE)
    for c, e in enumerate(state):
        out[c] = (e[XT], e[XN], e[XM], [e[XS0], e[XS1]], e[XB], e[XP], e[XPUSH], e[XPULL], e[XFIN], 0)
    return out


def _pushpull_counts(e, defect):
    """(kp, kq, K, the division's K, C) as a device build with that defect would hold them."""
    B, Pb, Qb = e[XB], e[XPUSH], e[XPULL]
    cut = M32 if defect == "kp32" else M64
    kp, kq = ((Pb + B - 1) & cut) // B, ((Qb + B - 1) & cut) // B
    K = kp + kq
    divisor = (K & M32) or 1 if defect == "k32" else K or 1
    return kp, kq, K, divisor, (Pb + Qb) & (M32 if defect == "c32" else M64)


def _exchange_element(e, m, defect=None):
    """(direction, stream position, length) of element m: workload.tcp_exchange_element, or with an X_DEFECTS defect
    what exchange_element of cts_tcp_exchange_math.hpp would give were that one quantity cut short (modulo 2^64,
    subtractions saturating, as there)."""
    from ctstraffic_amd import workload as W

    if defect == "m48":
        m &= M48
    if e[XP] != PUSHPULL or defect not in ("kp32", "c32", "k32"):
        return W.tcp_exchange_element(e[XP], e[XT], e[XB], e[XPUSH], e[XPULL], m)[:3]
    T, B, Pb, Qb = e[XT], e[XB], e[XPUSH], e[XPULL]
    kp, _, K, divisor, C = _pushpull_counts(e, defect)
    y = m // divisor
    r = (m - y * K) & M64
    push = r < kp
    in_seg = ((r if push else r - kp) * B) & M64
    seg = Pb if push else Qb
    G = (y * C + (0 if push else Pb) + in_seg) & M64
    return (0 if push else 1), (y * seg + in_seg) & M64, min(B, max(seg - in_seg, 0), max(T - G, 0))


def _exchange_position(e, m, defect=None):
    from ctstraffic_amd import workload as W

    if e[XP] != PUSHPULL or defect not in ("kp32", "k32") or m >= e[XN]:
        return W.tcp_exchange_position(e[XP], e[XT], e[XB], e[XPUSH], e[XPULL], m)
    B, Pb, Qb = e[XB], e[XPUSH], e[XPULL]
    kp, _, K, divisor, _ = _pushpull_counts(e, defect)
    y = m // divisor
    r = (m - y * K) & M64
    return [(y * Pb + (r * B if r < kp else Pb)) & M64, (y * Qb + (0 if r < kp else (r - kp) * B)) & M64]


def exchange_tick(state, ids, stride, capacity, max_buffers, n_conns, defect=None):
    """One tick of cts_tcp_exchange_send over state (exchange_state's lists, moved in place), one listed connection at
    a time in Python integers: the planner is plan(), a buffer is workload.tcp_exchange_element's and the position
    after the move workload.tcp_exchange_position's (the Python-integer forms, never the numpy model). defect: one of
    DEFECTS (the planner's) or X_DEFECTS (a quantity of the closed forms cut short: kp and kq from a 32-bit P + B - 1,
    C modulo 2^32, the division's K modulo 2^32, before + j cut to 48 bits, N - m cut to 32 bits before the min with
    max_buffers). Returns w, prefix, taken, codes, tick (six fields), bytes_dir, slots ((receiver, length, pattern
    offset) per written slot, None where a faulty plan leaves one out) and entries (copies, after the move)."""
    assert defect is None or defect in DEFECTS or defect in X_DEFECTS, defect
    w, codes = [], []
    for c in ids:
        want, code = 0, 4
        if c < n_conns:
            e = state[c]
            formed = e[XB] != 0 and e[XP] <= DUPLEX and (e[XP] != PUSHPULL or (e[XPUSH] != 0 and e[XPULL] != 0))
            if formed and e[XB] <= stride:
                code = 2
                if not e[XFIN] and e[XM] < e[XN]:
                    left = e[XN] - e[XM]
                    if defect == "n32":
                        left &= M32
                    want, code = min(left, max_buffers), 0
        w.append(want)
        codes.append(code)
    prefix, taken = plan(w, capacity, defect if defect in DEFECTS else None, "tcp")
    tick = dict.fromkeys(("bytes", "buffers", "connections_sent", "connections_finished", "connections_no_room",
                          "connections_skipped"), 0)
    bytes_dir, slots = [0, 0], {}
    for i, c in enumerate(ids):
        if codes[i] in (2, 4):
            tick["connections_skipped"] += 1
        elif taken[i] == 0:
            codes[i] = 3
            tick["connections_no_room"] += 1
        else:
            e = state[c]
            for j in range(taken[i]):
                d, pos, length = _exchange_element(e, e[XM] + j, defect)
                slots[prefix[i] + j] = (c + d * n_conns, length, pos % 65536)
                bytes_dir[d] += length
            e[XM] += taken[i]
            e[XS0], e[XS1] = _exchange_position(e, e[XM], defect)
            tick["buffers"] += taken[i]
            tick["connections_sent"] += 1
            if e[XM] == e[XN]:
                e[XFIN], codes[i] = 1, 1
                tick["connections_finished"] += 1
    tick["bytes"] = sum(bytes_dir)
    total = min(tick["buffers"], capacity)
    assert defect is not None or sorted(slots) == list(range(total))
    return {"w": w, "prefix": prefix, "taken": taken, "codes": codes, "tick": tick, "bytes_dir": bytes_dir,
            "slots": [slots.get(g) for g in range(total)], "entries": [list(e) for e in state]}


def long_exchange(n_listed):
    """Case A for the exchange tick: long_tcp's table with the patterns by turns, P and Q in 1..3B + 1, transfers of 1
    to 3 buffers (Duplex: 2, one each way), max_buffers 2, LONG_FINISHED, two ids beyond the table, two connections
    with B above the stride and one entry with pattern 4; the capacity is the first tick's wants less 5."""
    key = ("exchange", n_listed)
    if key in _LONG_CACHE:
        return _LONG_CACHE[key]
    settings = _long_exchange_settings()
    ids = _long_ids(n_listed, wide=(11, 700, 13))
    case = {"settings": settings, "finished": LONG_FINISHED, "pattern4": (13,), "ids": ids, "stride": 16,
            "max_buffers": 2}
    first = exchange_tick(exchange_case_state(case), ids, 16, M32, 2, LONG_TABLE)
    case["w"], case["capacity"] = first["w"], sum(first["w"]) - 5
    _LONG_CACHE[key] = case
    return case


def _long_exchange_settings():
    """long_exchange's table, the same for every list length."""
    from ctstraffic_amd import workload as W

    if "exchange settings" in _LONG_CACHE:
        return _LONG_CACHE["exchange settings"]
    rng = np.random.default_rng(17)
    settings = []
    for c in range(LONG_TABLE):
        B, k, pattern = int(rng.integers(1, 17)), 1 + c % 3, c % 4
        Pb, Qb = int(rng.integers(1, 3 * B + 2)), int(rng.integers(1, 3 * B + 2))
        if pattern in (PUSH, PULL):
            T = int(rng.integers((k - 1) * B + 1, k * B + 1))
        elif pattern == DUPLEX:
            T = int(rng.integers(1, 2 * B + 1))
        else:  # the first k buffers of the sequence, the last one cut short
            whole = sum(W.tcp_exchange_position(PUSHPULL, 1 << 40, B, Pb, Qb, k))
            T = whole - int(rng.integers(0, W.tcp_exchange_element(PUSHPULL, 1 << 40, B, Pb, Qb, k - 1)[2]))
        settings.append((pattern, T, B, Pb, Qb))
    settings[11], settings[700] = (PUSHPULL, 1000, 200, 300, 100), (DUPLEX, 5000, 129)
    _LONG_CACHE["exchange settings"] = settings
    return settings


def _idle_runs_exchange(stride, lead, total, filler):
    """Case B for the exchange tick: idle_run_tokens with four idle kinds (a finished connection, an id beyond the
    table, B above the stride, a PushPull entry with push_bytes 0), the patterns by turns, B = stride - 3, P = 2B + 1
    and Q = B - 1 (a cycle is the buffers B, B, 1 | B - 1). Every sender has six buffers from where it stands, so two
    ticks of max_buffers 3 send; a PushPull one stands at buffer 2, so its first three slots are the push segment's
    last byte, the pull segment and the next cycle's first buffer."""
    B = stride - 3
    Pb, Qb = 2 * B + 1, B - 1
    tokens = idle_run_tokens(lead, total, filler, kinds=4)
    settings, seek, finished, no_push, ids, w = [], [], [], [], [], []
    beyond = 0
    for what, x in tokens:
        c = len(settings)
        if what == "idle" and x == 1:
            ids.append(len(tokens) + beyond)
            beyond += 1
            w.append(0)
            continue
        ids.append(c)
        pattern = c % 4
        if what == "send":
            assert x == S_SLOTS, "the exchange case's senders all send %d" % S_SLOTS
            if pattern == PUSHPULL:
                settings.append((pattern, 2 * (Pb + Qb) - c % 5, B, Pb, Qb))
            else:
                settings.append((pattern, 6 * B - (2 if pattern == DUPLEX else 1) * (c % 5), B, Pb, Qb))
            seek.append(2 if pattern == PUSHPULL else 0)
            w.append(x)
            continue
        size = stride + 16 if x == 2 else B
        settings.append((PUSHPULL if x == 3 else pattern, 2 * size - c % 5, size, Pb, Qb))
        seek.append(0)
        w.append(0)
        if x == 0:
            finished.append(c)
        if x == 3:
            no_push.append(c)
    return {"settings": settings, "seek": seek, "finished": finished, "no_push": no_push, "ids": ids, "stride": stride,
            "w": w, "capacity": total, "max_buffers": 3}


def wide_exchange():
    """Case C for the exchange tick: wide_tcp's table, lists and four ticks at stride 16 and B = 1, P = 5, Q = 3. The
    huge connections (2^50 bytes, so 2^50 buffers whatever the pattern) are Push, Pull, PushPull and Duplex by turns,
    the first of the wave of 64 a PushPull one: the seven slots of ticks 3 and 4 are its, five of the push segment
    and two of the pull segment, then one, five and one. The small ones (2 bytes) take the patterns by turns too."""
    base = wide_tcp()
    settings, h = [], 0
    for c, (T, _) in enumerate(base["settings"]):
        if T == HUGE_TRANSFER:
            pattern = h % 4 if c < WIDE_TCP_LISTED else (PUSHPULL + c - WIDE_TCP_LISTED) % 4
            h += 1
        else:
            pattern = c % 4
        settings.append((pattern, T, 1, 5, 3))
    return {"settings": settings, "stride": 16, "ticks": base["ticks"], "capacity": 7}
