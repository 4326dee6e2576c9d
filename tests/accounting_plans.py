"""Shared by tests/test_accounting_seams_cpu.py and tests/test_accounting_seams_gpu.py (CPU only, no device).

The accounting passes conn_accumulate and ms_conn_accumulate give every wave of their grid one contiguous span of the
batch and walk it 64 descriptors (a tile) per step. What a wave does at a tile depends on what came before it in the
span: a tile that is nothing but the open run is "parked" (per-lane sums, no shuffle), and the parked sums join the
open run at the next tile that is not, or at the end of the span. `walk` replays those decisions over a batch's
per-descriptor keys and counts the transitions, so a test can assert that its batch takes every path before it compares
the device's sums; `plan` builds a batch that does, with lengths whose sums need the high word inside a tile.

geometry(n, cus) is span_geometry of ctstraffic_amd/csrc/cts_spans.hpp; the CPU test holds the two together.
"""
from dataclasses import dataclass

import numpy as np

from ctstraffic_amd import workload as W
from ctstraffic_amd.types import CONN_STATE_DTYPE, DESC_DTYPE, DGRAM_STATUS_DTYPE

KNONE = 0xFFFFFFFF
TILE, BLOCK, WAVES_PER_BLOCK, BLOCKS_PER_CU = 64, 256, 4, 8
N_CONNS = 7
ARENA_BYTES = 1 << 62
BASE_INDEX = 1000003

TRANSITIONS = ("first_pure", "first_mixed", "parked_tile", "parked_twice", "unpark_pure_other", "unpark_mixed_merge",
               "unpark_mixed_nomerge", "carry_merge_mixed", "carry_end", "end_parked", "end_scan", "scan_partial",
               "join_1", "join_2", "join_3", "join_break_key", "join_break_notwhole", "empty_wave")

# lengths whose sums leave 32 bits inside one tile, and the edges of the 32-bit range
VALUE_CLASSES = np.array([0, 1, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 1], dtype=np.uint64)


def geometry(n: int, cus: int):
    """(grid, span) of launch_conn_accumulate_src and launch_ms_conn_accumulate for n > 0 descriptors."""
    want = (n + BLOCK - 1) // BLOCK
    grid = min(want, max(cus, 1) * BLOCKS_PER_CU)
    waves = grid * WAVES_PER_BLOCK
    span = ((n + waves - 1) // waves + TILE - 1) // TILE * TILE
    return grid, span


def plan_size(cus: int) -> int:
    """One descriptor more than 256 per wave, and a partial last tile: span = 320, five tiles, at any CU count."""
    return BLOCKS_PER_CU * cus * WAVES_PER_BLOCK * 256 + 1003


def walk(keys, cus: int) -> dict:
    """Replay every wave's walk over keys (uint32 per descriptor: conn_index, or KNONE where the descriptor counts
    nowhere). Returns {"counts": {transition: number of waves it occurs in; join_k: number of joined runs},
    "grid", "span", "parked": bool[waves, tiles], "ntiles": tiles each wave walks}.

    first_pure / first_mixed     the span's first tile is one run / has more than one run head
    parked_tile, parked_twice    a tile goes on the open run whole; it does so while parked sums are already held
    unpark_pure_other            parked sums join the open run at a tile that is one run of another key
    unpark_mixed_merge/_nomerge  ... at a tile of several runs whose lane 0 goes on the open run / does not
    carry_merge_mixed, carry_end no parked sums: the open run goes on into lane 0's run of a mixed tile / ends
    end_parked, end_scan         the span ends with parked sums held / with a scanned tile
    scan_partial                 a scanned tile holds lanes past the end of the batch
    join_1 .. join_3             a run joined in LDS across 2, 3, 4 waves of a workgroup
    join_break_key / _notwhole   a wave's tail starts a new run in the join: another key / its span was not one run
    empty_wave                   a wave whose span starts at or past n
    """
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    n = len(keys)
    grid, span = geometry(n, cus)
    waves, tiles = grid * WAVES_PER_BLOCK, span // TILE
    assert waves * span >= n
    padded = np.full(waves * span, KNONE, dtype=np.uint32)
    padded[:n] = keys
    K = padded.reshape(waves, tiles, TILE)
    lo = np.arange(waves, dtype=np.int64) * span
    ntiles = np.clip((n - lo + TILE - 1) // TILE, 0, tiles)
    ev = {name: np.zeros(waves, dtype=bool) for name in TRANSITIONS if not name.startswith("join_") or
          name.startswith("join_break")}
    ckey = np.full(waves, KNONE, dtype=np.uint32)
    whole = np.ones(waves, dtype=bool)
    parked = np.zeros(waves, dtype=bool)
    parked_map = np.zeros((waves, tiles), dtype=bool)
    for t in range(tiles):
        act = ntiles > t
        k = K[:, t, :]
        pure = (k == k[:, :1]).all(axis=1)          # heads == 1
        merge = k[:, 0] == ckey
        park = act & pure & merge
        scan = act & ~park
        ev["parked_tile"] |= park
        ev["parked_twice"] |= park & parked
        parked_map[:, t] = park
        if t == 0:
            ev["first_pure"] |= scan & pure
            ev["first_mixed"] |= scan & ~pure
        else:
            up, cont = scan & parked, scan & ~parked
            ev["unpark_pure_other"] |= up & pure
            ev["unpark_mixed_merge"] |= up & ~pure & merge
            ev["unpark_mixed_nomerge"] |= up & ~pure & ~merge
            ev["carry_merge_mixed"] |= cont & merge
            ev["carry_end"] |= cont & ~merge
        ev["scan_partial"] |= scan & (lo + (t + 1) * TILE > n)
        whole = np.where(scan, whole & pure & (merge | (t == 0)), whole)
        ckey = np.where(scan, k[:, TILE - 1], ckey)
        parked = np.where(act, park, parked)
    nonempty = ntiles > 0
    ev["end_parked"] = nonempty & parked
    ev["end_scan"] = nonempty & ~parked
    ev["empty_wave"] = ~nonempty
    # the LDS join of a workgroup's four tails (thread 0 of the workgroup)
    tk, tw, ne = ckey.reshape(grid, 4), whole.reshape(grid, 4), nonempty.reshape(grid, 4)
    joins = {2: 0, 3: 0, 4: 0}
    key, chain = tk[:, 0].copy(), np.ones(grid, dtype=np.int64)

    def _record(sel):
        for length in joins:
            joins[length] += int((sel & (chain == length) & (key != KNONE)).sum())

    for w in range(1, WAVES_PER_BLOCK):
        brk = ~tw[:, w] | (tk[:, w] != key)
        ev["join_break_notwhole"].reshape(grid, 4)[:, w] = brk & ~tw[:, w] & ne[:, w]
        ev["join_break_key"].reshape(grid, 4)[:, w] = brk & tw[:, w] & ne[:, w]
        _record(brk)
        key = np.where(brk, tk[:, w], key)
        chain = np.where(brk, 1, chain + 1)
    _record(np.ones(grid, dtype=bool))
    counts = {name: int(v.sum()) for name, v in ev.items()}
    counts.update(join_1=joins[2], join_2=joins[3], join_3=joins[4])
    return {"counts": counts, "grid": grid, "span": span, "parked": parked_map, "ntiles": ntiles}


def covered(counts: dict) -> list:
    """The transitions a batch does not reach often enough: at least 4 waves each, scan_partial at least 1."""
    return [name for name in TRANSITIONS if counts[name] < (1 if name == "scan_partial" else 4)]


# ---- the batch ------------------------------------------------------------------------------------------------------
FIRST_HALF_RUNS = np.array([1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 320, 321, 640, 1000, 1281, 2600, 5000])
SECOND_HALF_RUNS = 64 * np.array([1, 1, 1, 2, 2, 3, 5, 8, 21])


def _runs(rng, total: int, choices, prev: int):
    """total keys in runs drawn from choices; a run never repeats the connection before it (prev at the start)."""
    lens = rng.choice(choices, size=int(total / choices.mean() * 1.2) + 64)
    while lens.sum() < total:
        lens = np.r_[lens, rng.choice(choices, size=len(lens))]
    conns = (prev + np.cumsum(rng.integers(1, N_CONNS, size=len(lens)))) % N_CONNS
    keys = np.repeat(conns, lens)[:total].astype(np.uint32)
    return keys, int(keys[-1])


def connection_keys(cus: int, tail: str, rng):
    """conn_index per descriptor, and the mask of descriptors to be made bad."""
    n = plan_size(cus)
    tail_len = {"run": 900, "mixed": 40}[tail]
    half = n // 2 // TILE * TILE
    first, prev = _runs(rng, half, FIRST_HALF_RUNS, 0)
    second, prev = _runs(rng, n - half - tail_len, SECOND_HALF_RUNS, prev)
    if tail == "run":
        end = np.full(tail_len, (prev + 1) % N_CONNS, dtype=np.uint32)
    else:
        end = np.where(np.arange(tail_len) % 2 == 0, (prev + 1) % N_CONNS, (prev + 2) % N_CONNS).astype(np.uint32)
    conn = np.r_[first, second, end]
    assert len(conn) == n
    make_bad = rng.random(n) < np.where(np.arange(n) < half, 1.0 / 1500, 1.0 / 6000)
    make_bad[n - tail_len:] = False
    return conn, make_bad


def draw_values(rng, n: int) -> np.ndarray:
    """uint32 lengths: three in ten from VALUE_CLASSES, the others uniform over the 32-bit range."""
    v = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    cls = rng.random(n) < 0.3
    v[cls] = rng.choice(VALUE_CLASSES, size=int(cls.sum()))
    return v.astype(np.uint32)


@dataclass
class Plan:
    cus: int
    tail: str
    descs: np.ndarray     # DESC_DTYPE
    bad: np.ndarray       # bool: the verify's bad-descriptor rule
    keys: np.ndarray      # uint32: conn_index, KNONE where bad
    slots: np.ndarray     # uint32[N_CONNS], one kind per connection
    walked: dict          # walk(keys, cus)
    base_index: int = BASE_INDEX
    arena_bytes: int = ARENA_BYTES
    n_conns: int = N_CONNS

    @property
    def n(self) -> int:
        return len(self.descs)

    @property
    def ordinals(self) -> np.ndarray:
        return self.base_index + np.arange(self.n, dtype=np.int64)


def _middle(candidates: np.ndarray, what: str) -> int:
    assert len(candidates) > 0, what
    return int(candidates[len(candidates) // 2])


def pick_slots(keys: np.ndarray, walked: dict, base: int) -> np.ndarray:
    """One kind of slot per connection, the ordinals taken from the walk: empty; below the batch; above it; lane 0 of
    a tile inside a parked stretch; lane 63 of such a tile; the first descriptor of a wave's span; the last one."""
    n, span, parked = len(keys), walked["span"], walked["parked"]
    waves, tiles = parked.shape
    inside = parked.copy()
    inside[:, :-1] &= parked[:, 1:]     # the next tile is parked too: the switch falls inside the stretch
    inside[:, -1] = False
    tile_start = (np.arange(waves)[:, None] * span + np.arange(tiles)[None, :] * TILE)
    slots = np.full(N_CONNS, KNONE, dtype=np.uint32)
    slots[1] = 3
    slots[2] = base + n
    for c, lane in ((3, 0), (4, TILE - 1)):
        at = tile_start[inside] + lane
        slots[c] = base + _middle(at[keys[at] == c], "a parked stretch of connection %d" % c)
    lo = np.arange(waves, dtype=np.int64) * span
    starts = lo[lo < n]
    slots[5] = base + _middle(starts[keys[starts] == 5], "a span that starts with connection 5")
    ends = lo[lo + span - 1 < n] + span - 1
    slots[6] = base + _middle(ends[keys[ends] == 6], "a span that ends with connection 6")
    return slots


_plans = {}


def plan(cus: int, tail: str) -> Plan:
    """The batch of the seam tests for a device of `cus` compute units (cached; do not modify)."""
    if (cus, tail) in _plans:
        return _plans[(cus, tail)]
    rng = np.random.default_rng([0xACC7, cus, {"run": 0, "mixed": 1}[tail]])
    conn, make_bad = connection_keys(cus, tail, rng)
    n = len(conn)
    d = np.zeros(n, dtype=DESC_DTYPE)
    d["conn_index"] = conn
    d["length"] = draw_values(rng, n)
    length = d["length"].astype(np.int64)
    skip = np.array([0, 26, -1])[rng.integers(0, 3, size=n)]
    skip = np.where(skip < 0, length, skip)
    d["skip_head"] = np.where(skip > length, 0, skip)
    d["expected_pattern_offset"] = rng.integers(0, 65536, size=n)
    d["byte_offset"] = rng.integers(0, 1 << 61, size=n, dtype=np.uint64)
    # bad descriptors: skip_head = length + 1, or (the others, and where length + 1 does not fit) a pattern offset
    # of 65536 or more
    by_skip = make_bad & (rng.random(n) < 0.5) & (length < 0xFFFFFFFF)
    d["skip_head"][by_skip] = (length[by_skip] + 1).astype(np.uint32)
    by_offset = make_bad & ~by_skip
    d["expected_pattern_offset"][by_offset] = rng.integers(65536, 1 << 32, size=int(by_offset.sum()))
    bad = W.descs_bad(d, ARENA_BYTES)
    assert np.array_equal(bad, make_bad)
    keys = np.where(bad, KNONE, conn).astype(np.uint32)
    walked = walk(keys, cus)
    p = Plan(cus, tail, d, bad, keys, pick_slots(keys, walked, BASE_INDEX), walked)
    for a in (p.descs, p.bad, p.keys, p.slots):
        a.setflags(write=False)
    _plans[(cus, tail)] = p
    return p


# ---- the models in Python integers -----------------------------------------------------------------------------------
def exact_views(descs, bad, ordinals, n_conns: int, slots):
    """reference_view and connection_view one descriptor at a time in Python integers: ({REF_FIELDS: int},
    [{CONN_STATE field: int}] per connection)."""
    ref = dict.fromkeys(W.REF_FIELDS, 0)
    table = [dict.fromkeys(CONN_STATE_DTYPE.names, 0) for _ in range(n_conns)]
    for i in range(len(descs)):
        if bad[i]:
            continue
        c, g = int(descs["conn_index"][i]), int(ordinals[i])
        first = int(slots[c]) if c < n_conns else KNONE
        vlen = int(descs["length"][i]) - int(descs["skip_head"][i])
        assert vlen >= 0
        if g <= first:
            ref["bytes_recv"] += vlen
            ref["buffers_recv"] += 1
            if g < first:
                ref["bytes_ok"] += vlen
            else:
                ref["buffers_failed"] += 1
        else:
            ref["bytes_after_failure"] += vlen
            ref["buffers_after_failure"] += 1
        if c < n_conns:
            e = table[c]
            if g <= first:
                e["bytes_recv"] += vlen
                e["buffers_recv"] += 1
            else:
                e["bytes_after_failure"] += vlen
                e["buffers_after_failure"] += 1
    return ref, table


# ---- close cases -----------------------------------------------------------------------------------------------------
CLOSE_BYTES = np.array([0, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 5], dtype=np.uint64)


def close_cases(n_ids: int, seed: int = 0xC105E):
    """Preset tables for cts_conns_close: (state CONN_STATE_DTYPE[n_conns], slots, ids, expected). bytes_recv from
    CLOSE_BYTES; the expected size equal, one off either way, or 2^32 off either way (the low words equal); about one
    slot in nine failed; about one id in forty at or past n_conns. ids are distinct, in a seeded order."""
    rng = np.random.default_rng(seed)
    n_conns = n_ids - n_ids // 40
    state = np.zeros(n_conns, dtype=CONN_STATE_DTYPE)
    state["bytes_recv"] = rng.choice(CLOSE_BYTES, size=n_conns)
    state["buffers_recv"] = rng.integers(0, 1 << 33, size=n_conns, dtype=np.uint64)
    state["bytes_after_failure"] = rng.integers(0, 1 << 50, size=n_conns, dtype=np.uint64)
    state["buffers_after_failure"] = rng.integers(0, 1 << 20, size=n_conns, dtype=np.uint64)
    slots = np.full(n_conns, KNONE, dtype=np.uint32)
    failed = rng.random(n_conns) < 1.0 / 9
    slots[failed] = rng.integers(0, KNONE, size=int(failed.sum()), dtype=np.uint64)
    outside = n_conns + rng.choice(1 << 20, size=n_ids - n_conns, replace=False)
    outside[0] = KNONE
    ids = rng.permutation(np.r_[np.arange(n_conns), outside]).astype(np.uint32)
    got = np.zeros(n_ids, dtype=np.int64)
    inside = ids < n_conns
    got[inside] = state["bytes_recv"][ids[inside]].astype(np.int64)
    delta = np.array([0, 1, -1, 1 << 32, -(1 << 32)])[rng.integers(0, 5, size=n_ids)]
    want = got + delta
    want = np.where(want < 0, got, want)
    return state, slots, ids, want.astype(np.uint64)


def exact_close(state, slots, ids, expected):
    """close_results' statuses and counts in Python integers: ([status per id, None for an id without a slot],
    {CLOSE_FIELDS: int})."""
    counts, out = dict.fromkeys(W.CLOSE_FIELDS, 0), []
    for i, c in enumerate(int(x) for x in ids):
        if c >= len(slots):
            out.append(None)
            continue
        got = int(state["bytes_recv"][c])
        if int(slots[c]) != KNONE:
            status, cls = W.STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN, "data_errors"
        elif expected is not None and got > int(expected[i]):
            status, cls = W.STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED, "too_much_data"
        elif expected is not None and got < int(expected[i]):
            status, cls = W.STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED, "not_all_data"
        else:
            status, cls = 0, "successful"
        counts["connections_closed"] += 1
        counts[cls] += 1
        counts["bytes_recv"] += got
        out.append(status)
    return out, counts


# ---- MediaStream statuses over the connection plan -----------------------------------------------------------------
MS_WINDOW = (3000, 300, 1000)   # frame size, buffered frames, stream length: a window of 600 frames, head 1
MS_NO_ENTRY = 9                 # a conn_index past the table


def ms_batch(p: Plan):
    """Synthetic statuses for the plan's descriptors: (conn uint32, DGRAM_STATUS_DTYPE). The plan's bad descriptors
    become datagrams of a connection without an entry; most datagrams are clean DATA with sequence number 1 + i % 600
    (inside the window); about 2 % carry a sequence number outside it, about 1 % are ID datagrams."""
    rng = np.random.default_rng([0x4D53, p.cus, len(p.tail)])
    n = p.n
    i = np.arange(n)
    conn = np.where(p.bad, MS_NO_ENTRY, p.descs["conn_index"]).astype(np.uint32)
    st = np.zeros(n, dtype=DGRAM_STATUS_DTYPE)
    st["kind"], st["pass"] = W.DGRAM_DATA, 1
    st["sequence_number"] = 1 + i % 600
    st["completed_bytes"] = draw_values(rng, n)
    r = rng.random(n)
    out = r < 0.02
    st["sequence_number"][out] = rng.choice(np.array([0, -5, 601, 1000, 1001, 1 << 40], dtype=np.int64),
                                            size=int(out.sum()))
    ident = (r >= 0.02) & (r < 0.03)
    st["kind"][ident] = W.DGRAM_ID
    st["sequence_number"][ident] = 0
    return conn, st


# ---- MediaStream render and close on preset entries ----------------------------------------------------------------
MS_FRAME_SIZE = (1 << 32) - 1
MS_HEAD_BYTES = np.array([(1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 33) - 1], dtype=np.uint64)  # dropped,
#                                                                            successful, duplicate, duplicate
MS_RENDER_KINDS = ("fatal", "ended", "failed", "past_final", "last_frame", "frame")


def ms_preset_entries(fresh: np.ndarray, seed: int = 0x3E7D):
    """Entries for the render and close tests over `fresh` (cts_ms_conn_init entries with rings of 2 frames and
    frame_size_bytes = 2^32 - 1, laid out one after the other): only the counters, the ring contents, head, final_frame,
    the timer fields, received_any and the status fields are written; frame_base and frames stay as laid out.
    Returns (entries, ring uint64[2 * n], kind per entry as an index into MS_RENDER_KINDS, slots)."""
    rng = np.random.default_rng(seed)
    n = len(fresh)
    assert (fresh["frames"] == 2).all() and (fresh["frame_size_bytes"] == MS_FRAME_SIZE).all()
    assert np.array_equal(fresh["frame_base"], 2 * np.arange(n, dtype=np.uint64))
    e = fresh.copy()
    ring = rng.integers(1, 1 << 34, size=2 * n, dtype=np.uint64)
    kind = rng.choice(len(MS_RENDER_KINDS), size=n, p=[0.2, 0.08, 0.08, 0.08, 0.16, 0.4])
    is_ = {name: kind == k for k, name in enumerate(MS_RENDER_KINDS)}
    for f, top in (("successful_frames", 1 << 40), ("dropped_frames", 1 << 40), ("duplicate_frames", 1 << 40),
                   ("error_frames", 1 << 33), ("datagrams", 1 << 33), ("datagrams_after_end", 1 << 33)):
        e[f] = rng.integers(1, top, size=n, dtype=np.uint64)
    e["bits_received"] = rng.integers(1 << 35, 1 << 44, size=n, dtype=np.uint64)
    e["timer_wheel_offset"] = rng.integers(1, 1 << 31, size=n)
    e["received_any"] = 1
    e["final_frame"] = 1000
    e["head_sequence_number"] = rng.integers(1, 4, size=n)
    # FatalAbort: nothing received, head 1, final_frame of every size up to 2^32 - 1
    m = is_["fatal"]
    e["received_any"][m], e["head_sequence_number"][m] = 0, 1
    final = rng.integers(1, 1 << 32, size=n)
    pick = rng.integers(0, 4, size=n)
    final = np.where(pick == 0, 1, np.where(pick == 1, 1 << 31, np.where(pick == 2, (1 << 32) - 1, final)))
    e["final_frame"][m] = final[m]
    # ended or failed at an earlier tick: not rendered again
    e["last_error"][is_["ended"]], e["finished"][is_["ended"]] = 0, 1
    e["last_error"][is_["failed"]] = W.STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN
    e["has_failure"][is_["failed"]] = 1
    # the head already past the final frame; the head on the final frame
    e["final_frame"][is_["past_final"]], e["head_sequence_number"][is_["past_final"]] = 3, 4
    m = is_["last_frame"]
    e["final_frame"][m] = e["head_sequence_number"][m]
    # the head's ring element
    at = e["frame_base"] + ((e["head_sequence_number"] - 1) % 2).astype(np.uint64)
    ring[at] = rng.choice(MS_HEAD_BYTES, size=n)
    slots = np.full(n, KNONE, dtype=np.uint32)
    slots[is_["failed"]] = rng.integers(0, KNONE, size=int(is_["failed"].sum()), dtype=np.uint64)
    return e, ring, kind, slots


def ms_render_model(entries, ring, ids):
    """cts_media_stream_conns_render's rules (include/cts_media_stream_conns.h) with numpy masks over the distinct ids.
    Returns (entries after, ring after, codes, {UDP_FIELDS: int})."""
    e, ring = entries.copy(), ring.copy()
    ids = np.asarray(ids, dtype=np.int64)
    codes = np.zeros(len(ids), dtype=np.uint32)
    where = np.nonzero(ids < len(e))[0]
    c = ids[where]
    assert len(np.unique(c)) == len(c)
    running = (e["last_error"][c] == W.STATUS_IO_RUNNING) & (e["frames"][c] != 0)
    codes[where[~running]] = e["finished"][c[~running]]
    where, c = where[running], c[running]
    e["timer_wheel_offset"][c] += 1
    head, final = e["head_sequence_number"][c], e["final_frame"][c]
    due = (e["timer_wheel_offset"][c] >= e["initial_buffer_frames"][c]) & (head <= final)
    fatal = due & (e["received_any"][c] == 0) & (head == 1)
    cf = c[fatal]
    e["dropped_frames"][cf] += final[fatal].astype(np.uint64)
    e["finished"][cf] = 2
    e["last_error"][cf] = W.STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED
    codes[where[fatal]] = 2
    udp = dict.fromkeys(W.UDP_FIELDS, 0)
    udp["dropped_frames"] = sum(int(x) for x in final[fatal])
    frame = due & ~fatal
    cr = c[frame]
    at = (e["frame_base"][cr] + ((head[frame] - 1) % e["frames"][cr].astype(np.int64)).astype(np.uint64)).astype(np.int64)
    got, want = ring[at], e["frame_size_bytes"][cr].astype(np.uint64)
    for f, sel in (("successful_frames", got == want), ("dropped_frames", got < want), ("duplicate_frames", got > want)):
        e[f][cr[sel]] += np.uint64(1)
        udp[f] += int(sel.sum())
    ring[at] = 0
    e["head_sequence_number"][cr] += 1
    done = ~fatal & (e["head_sequence_number"][c] > final)
    e["finished"][c[done]] = 1
    e["last_error"][c[done]] = 0
    codes[where[done]] = 1
    return e, ring, codes, udp


def ms_close_model(entries, ring, slots, ids):
    """cts_media_stream_conns_close's rules with numpy masks over the distinct ids. Returns (MS_CONN_RESULT_DTYPE
    results, entries after, ring after, slots after, {CLOSE_FIELDS: int})."""
    from ctstraffic_amd.types import MS_CONN_RESULT_DTYPE

    e, ring, slots = entries.copy(), ring.copy(), np.array(slots, dtype=np.uint32, copy=True)
    ids = np.asarray(ids, dtype=np.int64)
    res = np.zeros(len(ids), dtype=MS_CONN_RESULT_DTYPE)
    res["conn_index"], res["fail_datagram"] = ids, KNONE
    inside = ids < len(e)
    res["flags"][~inside] = 1
    where, c = np.nonzero(inside)[0], ids[inside]
    assert len(np.unique(c)) == len(c)
    status = e["last_error"][c].copy()
    was_running = status == W.STATUS_IO_RUNNING
    status[was_running] = W.STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED
    for f in ("bits_received", "successful_frames", "dropped_frames", "duplicate_frames", "error_frames", "datagrams",
              "datagrams_after_end", "head_sequence_number", "finished"):
        res[f][where] = e[f][c]
    failed = e["has_failure"][c] != 0
    res["fail_datagram"][where[failed]] = (e["datagrams"][c[failed]] - np.uint64(1)).astype(np.uint32)
    res["flags"][where] = np.where(was_running, 4, 0) | np.where(failed, 2, 0)
    res["first_fail"][where], res["status"][where] = slots[c], status
    counts = dict.fromkeys(W.CLOSE_FIELDS, 0)
    counts["connections_closed"] = len(c)
    counts["successful"] = int((status == 0).sum())
    counts["data_errors"] = int((status == W.STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN).sum())
    counts["not_all_data"] = len(c) - counts["successful"] - counts["data_errors"]
    counts["bytes_recv"] = sum(int(x) // 8 for x in e["bits_received"][c])
    slots[c] = KNONE
    for k in range(int(e["frames"][c].max()) if len(c) else 0):
        sel = e["frames"][c] > k
        ring[(e["frame_base"][c[sel]] + np.uint64(k)).astype(np.int64)] = 0
    e["last_error"][c] = status
    e["finished"][c] = np.where(e["finished"][c] != 0, e["finished"][c], 3)
    return res, e, ring, slots, counts


def ms_accumulate_model(entries, frame_elems: int, slots, conn, st, base_index: int):
    """cts_media_stream_conns_accumulate's rules with numpy masks, for entries that are all still running. Sums are
    integer adds (np.add.at on uint64), never float weights. Returns (entries after, ring, {UDP_FIELDS: int})."""
    e = entries.copy()
    n_conns, n = len(e), len(conn)
    assert not e["finished"].any()
    conn = np.asarray(conn, dtype=np.int64)
    has = conn < n_conns
    cc = np.where(has, conn, 0)
    g = base_index + np.arange(n, dtype=np.int64)
    first = np.where(has, np.asarray(slots, dtype=np.uint32)[cc].astype(np.int64), KNONE)
    after = has & (g > first)
    counted = ~after
    at_first = has & (g == first)
    clean = (st["kind"] == W.DGRAM_DATA) & (st["pass"] != 0) & counted & ~at_first
    completed = st["completed_bytes"].astype(np.uint64)
    seq = st["sequence_number"].astype(np.int64)
    head, final, frames = e["head_sequence_number"][cc], e["final_frame"][cc], e["frames"][cc].astype(np.int64)
    ring_at = e["frame_base"][cc].astype(np.int64) + (seq - 1) % np.maximum(frames, 1)
    inside = (seq <= final) & (seq >= head) & (seq - head < frames) & (ring_at < frame_elems)
    booked, err = clean & has & inside, clean & has & ~inside
    ring = np.zeros(frame_elems, dtype=np.uint64)
    np.add.at(ring, ring_at[booked], completed[booked])
    np.add.at(e["bits_received"], cc[clean & has], completed[clean & has] * np.uint64(8))
    e["error_frames"] += np.bincount(cc[err], minlength=n_conns).astype(np.uint64)
    e["datagrams"] += np.bincount(cc[counted & has], minlength=n_conns).astype(np.uint64)
    e["datagrams_after_end"] += np.bincount(cc[after], minlength=n_conns).astype(np.uint64)
    e["received_any"][np.unique(cc[booked])] = 1
    for i in np.nonzero(at_first)[0]:
        e["last_error"][cc[i]] = (W.STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN if st["kind"][i] == W.DGRAM_DATA
                                  else W.STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED)
        e["has_failure"][cc[i]] = 1
    udp = dict.fromkeys(W.UDP_FIELDS, 0)
    udp["bits_received"] = 8 * sum(int(x) for x in completed[clean])
    udp["error_frames"] = int(err.sum())
    udp["datagrams"] = int(counted.sum())
    return e, ring, udp


# ---- the strided form ----------------------------------------------------------------------------------------------
STRIDE = (1 << 32) - 1
STRIDED_SKIP = 26


def strided_lengths(cus: int):
    """Lengths of a one-connection ring of plan_size(cus) slots of 2^32 - 1 bytes, from the value classes (none is
    above the stride); about one in a thousand is below the skipped header, a bad descriptor. Returns (lengths uint32,
    bad, keys of connection 1, walk)."""
    rng = np.random.default_rng([0x57D, cus])
    n = plan_size(cus)
    lens = draw_values(rng, n)
    small = lens < STRIDED_SKIP
    lens[small & (rng.random(n) >= 0.01)] = 65536
    bad = lens < STRIDED_SKIP
    keys = np.where(bad, KNONE, 1).astype(np.uint32)
    return lens, bad, keys, walk(keys, cus)
