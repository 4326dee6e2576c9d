"""Shared by tests/test_launch_depths_cpu.py and tests/test_loop_depth_gpu.py (CPU only, no device).

Every data-path kernel has an outer loop whose grid is capped at CUs x blocks-per-CU, and state that matters only from
the loop's second pass on: a prefetched descriptor, a refilled LDS stage, an output ring that wraps. This module
restates the launchers' grid rules (ctstraffic_amd/csrc/cts_grids.hpp; the CPU test holds the two together through
tests/cpp/grids_check.cpp) and, on top of them, how deep each kernel's loop runs for a given launch, so a test can
assert that its shape reaches the later passes before it compares a device result. The depth functions follow the
kernels of ctstraffic_amd/csrc/cts_verify.hip, cts_media_stream_recv.hip and cts_fill.hip line by line; each names the
loop it models.
"""
import numpy as np

BLOCK = 256          # lanes of a workgroup
QUAD_TEAMS = 16      # buffers per workgroup and round of the four-buffers-per-wave kernels; a wave holds four
FILL_PIECE = 8192    # bytes per piece of fill_pieces_kernel
PIECE_CHUNKS = FILL_PIECE // 16
PIECE_BATCH = 16     # pieces a workgroup decodes together
FILL_BATCH = 256     # datagrams per LDS batch of fill_batched_kernel
RING_BATCH = 512     # datagrams per LDS batch of media_stream_fill_ring_kernel and ms_server_fill
MS_RING = 64         # rounds a wave of the MediaStream receive stages before it writes them
SCALAR_STRIDE = 1024  # ring fills: from this stride on the wave tracks its datagram as a wave-uniform value


# ---- the grid rules (cts_grids.hpp) ----------------------------------------------------------------------------------
def grid_for(n: int, teams_per_block: int, cus: int, bpc: int) -> int:
    want = (n + teams_per_block - 1) // teams_per_block
    cap = cus * (bpc if bpc > 0 else 8)
    per = 1 if want <= cap else (want + cap - 1) // cap
    return max(1, (want + per - 1) // per)


def contig_grid(n: int, cus: int, small_bpc: int, small_chunk: int):
    """(grid, per) of the quad walks: block b walks the chunks b, b + grid, ... of `per` buffers each."""
    g = grid_for(n, QUAD_TEAMS, cus, small_bpc)
    if small_chunk > 0:
        per = (small_chunk + QUAD_TEAMS - 1) // QUAD_TEAMS * QUAD_TEAMS
        return min((n + per - 1) // per, g), per
    groups = (n + QUAD_TEAMS - 1) // QUAD_TEAMS
    per = (groups + g - 1) // g * QUAD_TEAMS
    return (n + per - 1) // per, per


def batch_fill_grid(n: int, batch: int, cus: int, ring_bpc: int) -> int:
    return min((n + batch - 1) // batch, cus * (ring_bpc if ring_bpc > 0 else 4))


def piece_fill_grid(n: int, hint: int, cus: int, fill_bpc: int):
    """(grid, ppb) of fill_pieces_kernel."""
    ppb = (hint + FILL_PIECE - 1) // FILL_PIECE
    return min(n * ppb, cus * (fill_bpc if fill_bpc > 0 else 1)), ppb


def rules(n: int, cus: int, bpc: int, chunk: int, hint: int):
    """One line of grids_check: every rule at one tuple."""
    return ((n, cus, bpc, chunk, hint) + tuple(grid_for(n, t, cus, bpc) for t in (1, 4, 16)) +
            contig_grid(n, cus, bpc, chunk) + (batch_fill_grid(n, FILL_BATCH, cus, bpc),
                                               batch_fill_grid(n, RING_BATCH, cus, bpc)) +
            piece_fill_grid(n, hint, cus, bpc))


# ---- fill_pieces_kernel ----------------------------------------------------------------------------------------------
def desc_bad(descs, arena_bytes: int):
    off, ln = descs["byte_offset"].astype(np.uint64), descs["length"].astype(np.uint64)
    return ((descs["expected_pattern_offset"] >= 65536) | (descs["length"] < descs["skip_head"]) |
            (off > np.uint64(arena_bytes)) | (off + ln > np.uint64(arena_bytes)))


def piece_fill_depth(descs, hint: int, cus: int, fill_bpc: int, arena_bytes: int) -> dict:
    """fill_pieces_kernel over descs (the arena 16-byte aligned). Piece v = ppb * buffer + piece goes to workgroup
    v mod grid as its (v div grid)-th piece; a workgroup decodes its pieces PIECE_BATCH at a time (the v0 loop), the
    next batch before the current one's stores (`cur = nxt`).

    batches_min / batches_max    passes of the v0 loop over the workgroups
    ragged_workgroups            workgroups whose last batch has lanes with v >= total
    split_buffers                buffers whose pieces fall into two batches (of the grid: v div (16 x grid) differs)
    batches_with_bad             batch indices that hold a piece of a bad descriptor
    empty_pieces                 pieces of a good, non-empty buffer that lie past its end (cb >= nchunks)
    rest_pieces                  last pieces that take more than a piece: the buffer is longer than the hint
    rest_whole / rest_edge       ... of a span of whole 16-byte chunks / of a span with edge chunks
    last_piece_ends_buffer       buffers that end inside their last piece (it "takes the rest", no more than a piece)
    """
    n = len(descs)
    grid, ppb = piece_fill_grid(n, hint, cus, fill_bpc)
    total = n * ppb
    per_batch = PIECE_BATCH * grid
    pieces_of = (total - np.arange(grid, dtype=np.int64) + grid - 1) // grid  # pieces of workgroup b
    batches = (pieces_of + PIECE_BATCH - 1) // PIECE_BATCH
    first = np.arange(n, dtype=np.int64) * ppb
    bad = desc_bad(descs, arena_bytes)
    length = descs["length"].astype(np.int64) - descs["skip_head"].astype(np.int64)
    good = ~bad & (length > 0)
    sp = descs["byte_offset"].astype(np.int64) + descs["skip_head"].astype(np.int64)
    lo = sp & 15
    nchunks = np.where(good, (lo + length + 15) >> 4, 0)
    hi_last = lo + length - 16 * (nchunks - 1)
    whole = (lo == 0) & (hi_last == 16)
    pc = np.arange(ppb, dtype=np.int64)[None, :]
    cb = pc * PIECE_CHUNKS
    live = good[:, None] & (cb < nchunks[:, None])
    rest = live & (pc == ppb - 1) & (nchunks[:, None] > cb + PIECE_CHUNKS)
    v_batch = (first[:, None] + pc) // per_batch
    return {
        "grid": grid, "ppb": ppb, "total": total,
        "batches_min": int(batches.min()), "batches_max": int(batches.max()),
        "ragged_workgroups": int(np.count_nonzero(pieces_of % PIECE_BATCH)),
        "split_buffers": int(np.count_nonzero(first // per_batch != (first + ppb - 1) // per_batch)),
        "batches_with_bad": sorted(set(v_batch[bad].reshape(-1).tolist())),
        "empty_pieces": int(np.count_nonzero(good[:, None] & ~live)),
        "live_pieces": int(np.count_nonzero(live)),
        "rest_pieces": int(np.count_nonzero(rest)),
        "rest_whole": int(np.count_nonzero(rest & whole[:, None])),
        "rest_edge": int(np.count_nonzero(rest & ~whole[:, None])),
        "last_piece_ends_buffer": int(np.count_nonzero(live[:, -1] & ~rest[:, -1])),
    }


# ---- fill_kernel<TEAM> -----------------------------------------------------------------------------------------------
def team_fill_depth(n: int, team_lanes: int, cus: int, bpc: int) -> dict:
    """fill_kernel<team_lanes>: BLOCK / team_lanes teams per workgroup, team slot t takes buffers t, t + step, ...,
    each pass loading the next pass's descriptor (`dn = descs[i + step]`) before its stores. bpc: small_blocks_per_cu
    for the 64-lane form, fill_blocks_per_cu for the workgroup form."""
    teams = BLOCK // team_lanes
    grid = grid_for(n, teams, cus, bpc)
    step = grid * teams
    return {"grid": grid, "step": step, "passes_max": (n + step - 1) // step, "passes_min": n // step,
            "ragged_last": n % step != 0}


# ---- QuadWalk: verify_quad_kernel and the MediaStream receive --------------------------------------------------------
def quad_walk_depth(n: int, cus: int, small_bpc: int, small_chunk: int) -> dict:
    """The walk of verify_quad_kernel and ms_verify_quad_body: wave w of block b visits, in the block's chunks b,
    b + grid, ..., the rounds r with chunk * per + 16 r + 4 w < n (its first team's buffer is inside the launch).

    rounds[b, w]                 rounds of the wave's loop
    chunks[b]                    chunks the block walks
    crossing_waves               waves whose QuadWalk::next() moves on to a live buffer of the block's next chunk
    full_flushes[b, w]           MS_RING-round flushes inside the loop (the MediaStream receive)
    partial_after_full           waves that flush a partial ring after a full one
    partial_only                 waves that only ever flush a partial ring
    flush_mid_chunk              full flushes that fall on a round that is not its chunk's last
    flush_on_chunk_first_round   ... on a chunk's first round, the ring then holding rounds of earlier chunks
    flush_spans_chunks           full flushes whose ring holds rounds of more than one chunk
    """
    grid, per = contig_grid(n, cus, small_bpc, small_chunk)
    rpc = per // QUAD_TEAMS
    nchunks = (n + per - 1) // per
    c = np.arange(nchunks, dtype=np.int64)
    w = np.arange(BLOCK // 64, dtype=np.int64)
    left = n - c[:, None] * per - 4 * w[None, :]
    r_c = np.clip((left + QUAD_TEAMS - 1) // QUAD_TEAMS, 0, rpc)           # [chunk, wave]
    depth = (nchunks + grid - 1) // grid                                    # chunks of block 0
    padded = np.zeros((depth * grid, 4), dtype=np.int64)
    padded[:nchunks] = r_c
    by_block = padded.reshape(depth, grid, 4)                               # [ordinal, block, wave]
    rounds = by_block.sum(axis=0)
    end = by_block.cumsum(axis=0)                                           # rounds done after each chunk
    start = end - by_block
    chunks = np.minimum(depth, (nchunks - np.arange(grid) + grid - 1) // grid)
    full = rounds // MS_RING
    mid = first = spans = 0
    for k in range(1, int(full.max()) + 1 if full.size else 1):
        at = k * MS_RING                                                    # the flush follows the wave's at-th round
        holds = (start < at) & (end >= at)                                  # the chunk that round lies in
        has = full >= k
        mid += int(np.count_nonzero(holds & (end != at) & has[None]))
        first += int(np.count_nonzero(holds & (start == at - 1) & has[None]))
        spans += int(np.count_nonzero(holds & (start > at - MS_RING) & has[None]))
    return {
        "grid": grid, "per": per, "rounds_per_chunk": rpc, "rounds": rounds, "chunks": chunks,
        "rounds_max": int(rounds.max()),
        "crossing_waves": int(np.count_nonzero((by_block > 0).sum(axis=0) > 1)),
        "full_flushes": full,
        "partial_after_full": int(np.count_nonzero((full > 0) & (rounds % MS_RING > 0))),
        "partial_only": int(np.count_nonzero((full == 0) & (rounds > 0))),
        "flush_mid_chunk": mid, "flush_on_chunk_first_round": first, "flush_spans_chunks": spans,
    }


# ---- the batched fills -----------------------------------------------------------------------------------------------
def _later_crossings(count: int, batch: int, cps: int) -> int:
    """cts_ring_store_loop.hpp, the wave-uniform form, for a workgroup of `count` datagrams: the rounds with
    `crosses` (lane 0's chunk cb + 63 >= cps) over the four waves' runs of every batch after the first."""
    crossing = 0
    for k in range(1, (count + batch - 1) // batch):
        nk = min(batch, count - k * batch) * cps
        per_w = (((nk + 3) // 4) + 63) & ~63
        for wave in range(4):
            kl = np.arange(wave * per_w, min(wave * per_w + per_w, nk), 64, dtype=np.int64)
            crossing += int(np.count_nonzero(kl % cps + 63 >= cps))
    return crossing


def batch_fill_depth(n: int, batch: int, cus: int, ring_bpc: int, stride: int = 0) -> dict:
    """fill_batched_kernel (batch = FILL_BATCH) and media_stream_fill_ring_kernel / ms_server_fill (RING_BATCH, n = the
    capacity): workgroup b stages its datagrams [b * per_wg, (b + 1) * per_wg) in LDS `batch` at a time, a barrier
    before each refill; each of the four waves takes a quarter of the staged batch.

    batches_min / batches_max    passes of the d0 loop over the workgroups that have datagrams
    last_batch                   datagrams in the last batch of workgroup 0 (every workgroup but the last)
    last_wave_share, share       fill_batched_kernel: datagrams the last wave takes of that batch, and a full share
    with stride >= SCALAR_STRIDE (the wave-uniform form of the store loop, cps = stride / 16 chunks per slot):
    crossing_rounds_later        64-chunk rounds that cross a datagram boundary in a batch with d0 > 0
    """
    grid = batch_fill_grid(n, batch, cus, ring_bpc)
    per_wg = (n + grid - 1) // grid
    g0 = np.arange(grid, dtype=np.int64) * per_wg
    count = np.clip(n - g0, 0, per_wg)
    batches = (count + batch - 1) // batch
    last = int(count[0] - (batches[0] - 1) * batch)
    share = (last + 3) // 4
    out = {"grid": grid, "per_wg": per_wg, "batches_min": int(batches[count > 0].min()),
           "batches_max": int(batches.max()), "last_batch": last, "share": share,
           "last_wave_share": max(0, last - 3 * share)}
    if stride >= SCALAR_STRIDE:
        values, times = np.unique(count, return_counts=True)
        crossing = sum(_later_crossings(int(c), batch, stride // 16) * int(t) for c, t in zip(values, times))
        out["crossing_rounds_later"] = crossing
    return out


# ---- the shapes of tests/test_loop_depth_gpu.py, as functions of the device's compute units --------------------------
# Each *_reaches function returns the names of the depth facts its shape does NOT reach (empty: the test may run).
CU_COUNTS = (64, 104, 228, 256, 304)

PIECE_KINDS = ("64k", "70000", "1m", "9000")
PIECE_HINT = {"64k": 65536, "70000": 70000, "1m": 1 << 20, "9000": 9000}


def piece_n(kind: str, cus: int) -> int:
    """Buffers of a piece-fill case at fill_blocks_per_cu = 1 (a batch is 16 x cus pieces)."""
    if kind == "64k":   # 8 pieces per buffer: two and a half batches
        return (2 * 16 * cus + 8 * cus) // 8 + 3
    if kind == "70000":  # 9 pieces per buffer, which does not divide a batch: buffers lie across the batches' seams
        return (2 * 16 * cus + 8 * cus) // 9 + 3
    if kind == "1m":    # 128 pieces per buffer: three batches and more
        return cus * 16 * 3 // 128 + 5
    return 16 * cus * 5 // 4 + 5  # 2 pieces per buffer: two and a half batches


def piece_case(kind: str, cus: int):
    """(descs, arena_bytes) of a piece-fill case. The arena the fill is given ends at arena_bytes; a test allocates a
    tail behind it that must stay untouched."""
    from ctstraffic_amd.types import DESC_DTYPE

    n = piece_n(kind, cus)
    rng = np.random.default_rng(0xF111 + cus + PIECE_KINDS.index(kind))
    descs = np.zeros(n, dtype=DESC_DTYPE)
    off = 0
    for i in range(n):
        off += int(rng.integers(0, 17))
        skip = 0
        if kind in ("64k", "70000") and i % 3 == 0:  # an aligned 64 KiB buffer: whole chunks, whole pieces
            off += (-off) % 16
            ln = 65536
        elif kind == "1m" and i == n // 3:      # longer than the hint, edge chunks
            off += (-off) % 16 + 3
            ln = (1 << 20) + 5
        elif kind == "1m" and i == 2 * n // 3:  # longer than the hint, whole chunks
            off += (-off) % 16
            ln = 3 << 19
        elif kind == "9000":                    # three in five reach into the second (last) piece
            ln = int(rng.integers(8193, 12001)) if rng.random() < 0.6 else int(rng.integers(0, 8193))
            skip = int(rng.integers(0, min(ln, 30) + 1))
        else:
            ln = int(rng.integers(0, 70001))
            skip = int(rng.integers(0, min(ln, 30) + 1))
        descs[i] = (off, ln, int(rng.integers(0, 65536)), i % 7, skip)
        off += ln
    arena_bytes = off
    # 2 %: the reference's FAIL_FAST shapes and buffers that leave the arena, spread over every batch
    for k, i in enumerate(np.linspace(1, n - 2, max(4, n // 50)).astype(int)):
        if i % 3 == 0 and kind in ("64k", "70000") or kind == "1m" and i in (n // 3, 2 * n // 3):
            i += 1
        if k % 4 == 0:
            descs[i]["expected_pattern_offset"] = 65536 + k
        elif k % 4 == 1:
            descs[i]["skip_head"] = int(descs[i]["length"]) + 1
        elif k % 4 == 2:
            descs[i]["byte_offset"] = arena_bytes + 16 * k            # wholly past the end
            descs[i]["length"] = max(1, int(descs[i]["length"]))
        else:
            descs[i]["byte_offset"] = arena_bytes - 7                 # straddles the end
            descs[i]["length"] = 4096 + 16 * k
    return descs, arena_bytes


def piece_reaches(kind: str, d: dict) -> list:
    want = {"three_batches": d["batches_max"] >= 3, "ragged_last_batch": d["ragged_workgroups"] > 0,
            "bad_in_every_batch": d["batches_with_bad"] == list(range(d["batches_max"]))}
    if kind == "64k":
        # 8 pieces per buffer divide a batch of 16 x grid pieces: no buffer lies across a seam at this hint
        want["whole_64k_buffers"] = d["split_buffers"] == 0
    elif kind == "70000":
        want["buffers_split_across_batches"] = d["split_buffers"] >= d["batches_max"] - 1
    elif kind == "1m":
        want.update(most_pieces_empty=d["empty_pieces"] > d["live_pieces"], whole_tail=d["rest_whole"] > 0,
                    edge_tail=d["rest_edge"] > 0)
    else:
        want.update(two_full_batches=d["batches_min"] >= 2,
                    last_piece_takes_the_rest=2 * d["last_piece_ends_buffer"] > d["total"] // d["ppb"])
    return sorted(k for k, ok in want.items() if not ok)


def team_fill_n(team_lanes: int, cus: int) -> int:
    """fill_kernel at one workgroup per CU: three full passes and a ragged fourth."""
    return 4 * cus * 3 + 5 if team_lanes == 64 else 3 * cus + cus // 2 + 3


def team_fill_reaches(d: dict) -> list:
    want = {"three_passes": d["passes_min"] >= 3, "ragged_last_pass": d["ragged_last"]}
    return sorted(k for k, ok in want.items() if not ok)


def quad_n(cus: int) -> int:
    """verify_quad_kernel at small_blocks_per_cu = 1."""
    return 16 * cus * 3 + 21


QUAD_CHUNKS = (0, 16, 48)


def quad_reaches(chunk: int, d: dict) -> list:
    full_blocks = d["rounds"][:-1]  # every block but the last, which holds the launch's ragged end
    if chunk == 0:
        want = {"three_rounds_per_wave": full_blocks.min() >= 3, "one_chunk": int(d["chunks"].max()) == 1}
    elif chunk == 16:
        want = {"three_chunks_per_block": int(d["chunks"][:-1].min()) >= 3, "next_crosses": d["crossing_waves"] > 0,
                "one_round_per_chunk": d["rounds_per_chunk"] == 1}
    else:
        want = {"two_chunks_of_three_rounds": d["rounds_per_chunk"] == 3 and int((d["rounds"].min(axis=1) >= 6).sum()) > 0,
                "next_crosses": d["crossing_waves"] > 0}
    return sorted(k for k, ok in want.items() if not ok)


RING_CHUNK_D1 = 16 * 133


def ring_n(case: str, cus: int) -> int:
    """The MediaStream receive. d1: four chunks of 133 rounds (the last one 77 datagrams), whatever the device. d2:
    small_blocks_per_cu = 1 and chunks of 48, 22 chunks and more per block."""
    if case == "d1":
        return 3 * RING_CHUNK_D1 + 77
    return 48 * 22 * cus + 48 * 5 + 21


def ring_reaches(case: str, d: dict) -> list:
    if case == "d1":
        want = {"two_full_flushes_then_five": bool((d["rounds"][:3] == 2 * MS_RING + 5).all()),
                "last_block_partial_only": bool((d["full_flushes"][3] == 0).all() and d["rounds"][3].max() == 5),
                "four_blocks": d["grid"] == 4, "flush_inside_chunk": d["flush_mid_chunk"] > 0}
    else:
        want = {"22_chunks_per_block": int(d["chunks"].min()) >= 22, "three_rounds_per_chunk": d["rounds_per_chunk"] == 3,
                "flush_on_a_chunk_first_round": d["flush_on_chunk_first_round"] >= 4 * (d["grid"] - 1),
                "ring_holds_several_chunks": d["flush_spans_chunks"] > 0, "several_blocks": d["grid"] > 1}
    return sorted(k for k, ok in want.items() if not ok)


def batched_n(kind: str, cus: int) -> int:
    """The batched fills at ring_fill_blocks_per_cu = 1. kind: "descs" (cts_media_stream_fill), "ring64" and "ring1040"
    (cts_media_stream_fill_strided and ms_server_fill at those strides)."""
    if kind == "descs":
        return cus * (2 * FILL_BATCH + 19)
    return cus * ((2 if kind == "ring64" else 1) * RING_BATCH + 19)


def batched_reaches(kind: str, d: dict) -> list:
    if kind == "descs":
        want = {"three_batches": d["batches_min"] == 3, "last_batch_of_19": d["last_batch"] == 19,
                "short_last_wave": 0 < d["last_wave_share"] < d["share"]}
    elif kind == "ring64":
        want = {"three_batches": d["batches_min"] == 3, "last_batch_of_19": d["last_batch"] == 19}
    else:
        want = {"two_batches": d["batches_min"] == 2, "last_batch_of_19": d["last_batch"] == 19,
                "crossing_rounds_past_the_first_batch": d["crossing_rounds_later"] > 0}
    return sorted(k for k, ok in want.items() if not ok)
