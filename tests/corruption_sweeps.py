"""Shared by tests/test_corruption_sweeps_cpu.py and tests/test_corruption_sweeps_gpu.py (CPU only, no device).

The verify kernels cut a span into 16-byte chunks aligned in memory and do not treat the chunks alike: each path gives
them roles (an edge chunk under a byte mask, a head chunk, a lane of a full or of a tail round, a piece of the
mailbox), and a bug confined to one role passes every test that places its corruptions at random. This module restates
the roles in plain numpy, from the rules of ctstraffic_amd/csrc/cts_verify.hip (make_span, scan_buffer, scan_rounds,
scan_whole_exact, mailbox_kernel), cts_quad.hpp (quad_span, quad_scan_interior) and cts_internal.hpp (mail_parts), and
builds the sweeps: one buffer per verified byte of a span, each with one flipped bit; pairs of flips at the roles'
landmarks; buffers filled with a shifted pattern. The CPU test shows, through the role model, that every role of every
shape owns buffers whose only corrupt byte lies in it, and that a verifier ignoring one role disagrees with the oracle
on the plan; the GPU test then holds the kernels to the oracle's exact records on the same plans.

The shapes follow from the kernels' constants below. tests/test_corruption_sweeps_cpu.py reads the same constants out
of the sources, so a change of kWgLoads or kQuadLoads fails there first, and the shapes' own assertions (wg_shape_facts,
quad_shape_facts) say which derivation no longer holds.
"""
import collections
import functools

import numpy as np

from ctstraffic_amd.types import DESC_DTYPE, DGRAM_HEADER_DTYPE, RESULT_DTYPE

BLOCK = 256                       # kBlock: lanes of a workgroup
WG_LOADS = 2                      # kWgLoads: loads per lane and round of verify_wg_*
WG_ROUND = BLOCK * WG_LOADS       # chunks of a full round
QUAD_TEAM = 16                    # kQuadTeam
QUAD_LOADS = 6                    # kQuadLoads
QUAD_ROUND = QUAD_TEAM * QUAD_LOADS
MAIL_PIECE = 4096                 # kMailPieceBytes
MAIL_PIECE_CHUNKS = MAIL_PIECE // 16
MAIL_GROUP = 4                    # kMailGroup: workgroups of a mailbox group; piece u goes to workgroup u mod 4
MAIL_FLIGHT = 4                   # pieces a workgroup has in flight: a loop pass covers MAIL_GROUP * MAIL_FLIGHT pieces
PERIOD = 65536
N_CONNS = 7
GAP = 0xEE
EMPTY = 0xFFFFFFFF
HEADER = 26                       # CTS_UDP_DATA_HEADER_LENGTH

EDGE0, LAST, HEAD, FULL, TAIL, ROUND = 0, 1, 2, 3, 4, 5
KIND_NAMES = {EDGE0: "edge0", LAST: "last", HEAD: "head", FULL: "full", TAIL: "tail", ROUND: "round"}


def pattern(pos):
    """P(j) of ctsIOPattern.cpp:55-80: the little-endian u16 ramp 0..32767, every 64 KiB."""
    pos = np.asarray(pos, dtype=np.int64) & 0xFFFF
    return np.where(pos & 1, pos >> 9, (pos >> 1) & 0xFF).astype(np.uint8)


# ---- the role model --------------------------------------------------------------------------------------------------
def geometry(start, length):
    """make_span / quad_span for a span whose first byte lies at address `start` (mod 128): (lo, nchunks, hi_last,
    cb0). cb0 is verify_wg's first line-aligned interior chunk; the quad path's cs is cb0 - 8."""
    start, length = np.asarray(start, dtype=np.int64), np.asarray(length, dtype=np.int64)
    lo = start & 15
    nch = np.where(length == 0, 0, (lo + length + 15) >> 4)
    hi_last = np.where(length == 0, 0, lo + length - 16 * (nch - 1))
    cb0 = 8 - ((start >> 4) & 7)
    return lo, nch, hi_last, cb0


def whole_lines(start, length):
    """span_whole_lines: the span takes scan_whole_exact."""
    lo, _, hi_last, cb0 = geometry(start, length)
    return (lo == 0) & (hi_last == 16) & (cb0 == 8)


def wg_roles(start, length, chunk):
    """verify_wg_body: the role of chunk `chunk` of the span (start mod 128, length); arrays broadcast.

    scan_buffer (ragged spans): chunk 0 is edge0 (lane 0, masked by lo; by hi_last too when it is the only chunk), chunk
    nchunks - 1 is last (lane 1), chunks [1, min(cb0, nchunks - 1)) are head chunks (lane chunk + 1); the interior
    [cb0, nchunks - 1) goes k = chunk - cb0 at a time: full rounds of WG_ROUND chunks while they fit, then one tail
    round. In either, the chunk is load u = (k mod WG_ROUND) div BLOCK of lane k mod BLOCK. scan_exact_owned re-derives
    the same ownership (its rounds are 2 x BLOCK as well). scan_whole_exact (whole-line spans): the same rounds over
    [0, nchunks), no edges.
    Returns kind (EDGE0, LAST, HEAD, FULL, TAIL; -1 outside the span), round, u, lane, wave."""
    start, length, chunk = np.broadcast_arrays(np.asarray(start, dtype=np.int64), np.asarray(length, dtype=np.int64),
                                               np.asarray(chunk, dtype=np.int64))
    lo, nch, hi_last, cb0 = geometry(start, length)
    whole = (lo == 0) & (hi_last == 16) & (cb0 == 8)
    c_beg = np.where(whole, 0, cb0)
    c_end = np.where(whole, nch, nch - 1)
    n_int = np.maximum(c_end - c_beg, 0)
    k = chunk - c_beg
    full_end = n_int // WG_ROUND * WG_ROUND
    interior = (chunk >= c_beg) & (chunk < c_end) & (whole | (nch >= 3))
    kind = np.full(chunk.shape, -1, dtype=np.int64)
    kind[interior & (k < full_end)] = FULL
    kind[interior & (k >= full_end)] = TAIL
    edges = ~whole & (chunk >= 0) & (chunk < nch)
    kind[edges & (chunk >= 1) & (chunk < np.minimum(cb0, nch - 1))] = HEAD
    kind[edges & (chunk == nch - 1) & (nch > 1)] = LAST
    kind[edges & (chunk == 0)] = EDGE0
    streamed = (kind == FULL) | (kind == TAIL)
    rnd = np.where(kind == FULL, k // WG_ROUND, 0)
    u = np.where(streamed, (k % WG_ROUND) // BLOCK, 0)
    lane = np.where(streamed, k % BLOCK, np.where(kind == HEAD, chunk + 1, np.where(kind == LAST, 1, 0)))
    return {"kind": kind, "round": rnd, "u": u, "lane": lane, "wave": lane // 64}


def quad_roles(start, length, chunk):
    """verify_quad_kernel and the MediaStream receive (cts_quad.hpp): chunk 0 is edge0 (team lane 0), chunk nch - 1
    last (team lane 1); the interior [1, nch - 2] is covered by rounds of QUAD_ROUND chunks that start at chunk
    cs = -(chunk 0's slot in its 128-byte line): chunk c is load u = ((c - cs) mod QUAD_ROUND) div 16 of team lane
    (c - cs) mod 16 in round (c - cs) div QUAD_ROUND. quad_scan_exact re-reads cs + lane, cs + lane + 16, ...: the same
    owner. Returns kind (EDGE0, LAST, ROUND; -1 outside), round, u, lane."""
    start, length, chunk = np.broadcast_arrays(np.asarray(start, dtype=np.int64), np.asarray(length, dtype=np.int64),
                                               np.asarray(chunk, dtype=np.int64))
    _, nch, _, cb0 = geometry(start, length)
    cs = cb0 - 8
    k = chunk - cs
    kind = np.full(chunk.shape, -1, dtype=np.int64)
    kind[(chunk >= 1) & (chunk <= nch - 2)] = ROUND
    kind[(chunk == nch - 1) & (nch > 1)] = LAST
    kind[(chunk == 0) & (nch > 0)] = EDGE0
    inner = kind == ROUND
    return {"kind": kind, "round": np.where(inner, k // QUAD_ROUND, 0),
            "u": np.where(inner, (k % QUAD_ROUND) // QUAD_TEAM, 0),
            "lane": np.where(inner, k % QUAD_TEAM, np.where(kind == LAST, 1, 0)),
            "wave": np.zeros(chunk.shape, dtype=np.int64)}


def mail_roles(start, length, chunk):
    """mailbox_kernel: the buffer's chunks (of the 16-byte aligned base) go in pieces of MAIL_PIECE_CHUNKS; piece p is
    read by workgroup p mod MAIL_GROUP in its loop pass p div (MAIL_GROUP * MAIL_FLIGHT), chunk c of it by thread
    c mod 256 (data wave thread div 64). Only the buffer's chunk 0 and its last chunk are masked.
    Returns piece, wg, pass, wave, first, last."""
    start, length, chunk = np.broadcast_arrays(np.asarray(start, dtype=np.int64), np.asarray(length, dtype=np.int64),
                                               np.asarray(chunk, dtype=np.int64))
    _, nch, _, _ = geometry(start, length)
    piece = chunk // MAIL_PIECE_CHUNKS
    return {"piece": piece, "wg": piece % MAIL_GROUP, "pass": piece // (MAIL_GROUP * MAIL_FLIGHT),
            "wave": (chunk % MAIL_PIECE_CHUNKS) // 64, "first": chunk == 0, "last": chunk == nch - 1}


def role_key(r, by_wave=True):
    """One integer per role: kind, round, u and (by_wave) the wave."""
    return ((r["kind"] << 40) | (r["round"] << 20) | (r["u"] << 8) | (r["wave"] if by_wave else 0)).astype(np.int64)


def role_name(key) -> str:
    key = int(key)
    kind, rnd, u, wave = key >> 40, (key >> 20) & 0xFFFFF, (key >> 8) & 0xFFF, key & 0xFF
    if kind in (EDGE0, LAST, HEAD):
        return KIND_NAMES[kind]
    if kind == TAIL:
        return "tail(u=%d, wave=%d)" % (u, wave)
    return "%s(round=%d, u=%d, wave=%d)" % (KIND_NAMES[kind], rnd, u, wave)


ROLES = {"wg": wg_roles, "quad": quad_roles}


# ---- plans -----------------------------------------------------------------------------------------------------------
# arena, descs: what is verified. slot: the arena is rows of `slot` bytes, buffer i in row i. flips: (row, position
# in the verified span, xor value) of every corrupted byte, or None for a plan that is not made of flips. strided: the
# (stride, skip_head, expected_offset, conn_index) of a ring plan, else None.
Plan = collections.namedtuple("Plan", "arena descs slot flips strided")


def _uniform(a):
    return bool((a == a[0]).all())


def _columns(off, skip, length, e, slot, fn, block=8192):
    """fn(rows lo..hi, cols, mask, expected): per block of rows, the column grid relative to each row's span, the
    mask of the span's columns and the expected bytes there."""
    cols0 = np.arange(slot, dtype=np.int32)[None, :]
    for k in range(0, len(off), block):
        c0 = (off[k:k + block] + skip[k:k + block]).astype(np.int32)[:, None]
        cols = cols0 - c0
        mask = (cols >= 0) & (cols < length[k:k + block].astype(np.int32)[:, None])
        fn(k, min(k + block, len(off)), cols, mask, pattern(e[k:k + block, None] + cols))


def assemble(off, skip, length, e, flips, slot, seed, conn=None, strided=None, order=None):
    """The arena and descriptors of n items. Item k: a buffer at byte `off[k]` of its row, `skip[k]` skipped head bytes,
    `length[k]` verified bytes at pattern offset `e[k]`; flips = (item, position, xor) arrays. The items are laid into
    the rows in a seeded random order (order: a given one); rows' other bytes hold GAP."""
    off, skip, length, e = (np.asarray(x, dtype=np.int64) for x in (off, skip, length, e))
    n = len(off)
    assert int((off + skip + length).max()) < slot or strided is not None and int((off + skip + length).max()) <= slot
    row_of = np.random.default_rng(seed).permutation(n) if order is None else np.asarray(order, dtype=np.int64)
    item_of = np.empty(n, dtype=np.int64)
    item_of[row_of] = np.arange(n)
    off, skip, length, e = off[item_of], skip[item_of], length[item_of], e[item_of]
    arena = np.full(n * slot + 64, GAP, dtype=np.uint8)
    rows = arena[:n * slot].reshape(n, slot)
    if _uniform(off) and _uniform(skip) and _uniform(length) and _uniform(e):
        c0 = int(off[0] + skip[0])
        rows[:, c0:c0 + int(length[0])] = pattern(int(e[0]) + np.arange(int(length[0])))
    else:
        def put(lo, hi, cols, mask, exp):
            rows[lo:hi][mask] = exp[mask]
        _columns(off, skip, length, e, slot, put)
    fr = row_of[np.asarray(flips[0], dtype=np.int64)]
    fp, fx = np.asarray(flips[1], dtype=np.int64), np.asarray(flips[2], dtype=np.uint8)
    assert ((fp >= 0) & (fp < length[fr]) & (fx != 0)).all()
    at = fr * slot + off[fr] + skip[fr] + fp
    assert np.unique(at).size == at.size
    arena[at] ^= fx
    descs = np.zeros(n, dtype=DESC_DTYPE)
    descs["byte_offset"] = np.arange(n, dtype=np.int64) * slot + off
    descs["length"], descs["skip_head"], descs["expected_pattern_offset"] = skip + length, skip, e
    descs["conn_index"] = np.arange(n) % N_CONNS if conn is None else conn
    return Plan(arena, descs, slot, (fr, fp, fx), strided)


def span_start(plan):
    """Address mod 128 of every buffer's first verified byte (the arena on a 128-byte boundary)."""
    return ((plan.descs["byte_offset"].astype(np.int64) + plan.descs["skip_head"]) % 128).astype(np.int64)


def span_length(plan):
    return plan.descs["length"].astype(np.int64) - plan.descs["skip_head"]


def sweep_bit(i):
    """The bit flipped at span position i: over eight consecutive chunks every (byte in chunk, bit) pair occurs."""
    i = np.asarray(i, dtype=np.int64)
    return (i + i // 16) % 8


def _with_clean(n_dirty):
    """About one buffer in four is a clean copy."""
    return n_dirty + (n_dirty + 2) // 3


def sweep(start, length, skip_head, e, positions=None, all_bits=False, seed=1, stride=0, conn=None):
    """One buffer per verified position i (default: every byte of the span) with bit sweep_bit(i) flipped there
    (all_bits: eight buffers, one per bit), among clean copies. The span's first byte lies at `start` mod 128.
    stride: a ring of that stride, buffer i at i * stride (start is then skip_head, plus 64 in every other slot when
    the stride is an odd multiple of 64)."""
    pos = np.arange(length, dtype=np.int64) if positions is None else np.asarray(sorted(positions), dtype=np.int64)
    if all_bits:
        pos, bit = np.repeat(pos, 8), np.tile(np.arange(8), pos.size)
    else:
        bit = sweep_bit(pos)
    n = _with_clean(pos.size)
    if stride:
        assert start == skip_head and stride % 64 == 0
        off, slot = 0, stride
        strided = (stride, skip_head, e, N_CONNS // 2 if conn is None else conn)
        conn = strided[3]
    else:
        off = (start - skip_head) % 128
        slot = (off + skip_head + length + 1 + 127) // 128 * 128
        strided = None
    ones = np.ones(n, dtype=np.int64)
    return assemble(off * ones, skip_head * ones, length * ones, e * ones,
                    (np.arange(pos.size), pos, (1 << bit).astype(np.uint8)), slot, seed, conn=conn, strided=strided)


def pairs(start, length, skip_head, e, landmarks, seed=2):
    """One buffer per unordered pair of landmark positions, the two bytes flipped by different values."""
    lm = np.asarray(sorted(set(int(x) for x in landmarks)), dtype=np.int64)
    a, b = np.triu_indices(lm.size, 1)
    k = np.arange(a.size)
    xa = (1 << (k % 8)).astype(np.uint8)
    n = _with_clean(a.size)
    off = (start - skip_head) % 128
    slot = (off + skip_head + length + 1 + 127) // 128 * 128
    ones = np.ones(n, dtype=np.int64)
    return assemble(off * ones, skip_head * ones, length * ones, e * ones,
                    (np.concatenate([k, k]), np.concatenate([lm[a], lm[b]]), np.concatenate([xa, xa ^ 0xFF])),
                    slot, seed)


SHIFTS = (1, 2, 3, 16, 256, 512, 32768, 65535)


def shifted(start, length, skip_head, e, seed=3):
    """Buffers filled at pattern offset e + delta and verified at e, for delta in SHIFTS, among clean copies: every
    lane is dirty, the counts are large (at 512 half the bytes differ). Four buffers per delta, so that every
    connection fails and a workgroup meets dirty buffers back to back."""
    deltas = SHIFTS * 4
    n = _with_clean(len(deltas))
    off = (start - skip_head) % 128
    slot = (off + skip_head + length + 1 + 127) // 128 * 128
    ones = np.ones(n, dtype=np.int64)
    none = np.zeros(0, dtype=np.int64)
    plan = assemble(off * ones, skip_head * ones, length * ones, e * ones, (none, none, none), slot, seed)
    row_of = np.random.default_rng(seed).permutation(n)
    c0 = off + skip_head
    for k, delta in enumerate(deltas):
        plan.arena[row_of[k] * slot + c0:row_of[k] * slot + c0 + length] = pattern(e + delta + np.arange(length))
    return plan._replace(flips=None)


def small_shapes():
    """(start, length) of the small-shape sweep: every start 0..127 with the lengths that make nchunks one of 1, 2, 3,
    cb0, cb0 + 1, cb0 + 2, cb0 + 3 -- no interior, head chunks only, an empty tail, exactly one interior chunk and up
    to three -- each ending 1 and 16 bytes into its last chunk; for one chunk every end, so that every
    range_mask(lo, hi) of a single chunk occurs."""
    out = []
    for start in range(128):
        lo, cb0 = start & 15, 8 - ((start >> 4) & 7)
        for nch in sorted({1, 2, 3, cb0, cb0 + 1, cb0 + 2, cb0 + 3}):
            for hi in (range(lo + 1, 17) if nch == 1 else (1, 16)):
                out.append((start, 16 * (nch - 1) + hi - lo))
    return out


@functools.lru_cache(maxsize=None)
def small_sweep(seed=4):
    """Every byte of every small shape corrupted, one buffer each, among clean copies of the shapes; skipped heads of
    0 to 26 bytes and expected offsets that put the 64 KiB period's wrap inside one shape in five."""
    shapes = small_shapes()
    start = np.array([s for s, _ in shapes], dtype=np.int64)
    length = np.array([ln for _, ln in shapes], dtype=np.int64)
    shape_of = np.repeat(np.arange(len(shapes)), length)
    pos = np.concatenate([np.arange(ln) for ln in length])
    n_clean = (pos.size + 2) // 3
    shape_of = np.concatenate([shape_of, np.arange(n_clean) % len(shapes)])
    s, ln = start[shape_of], length[shape_of]
    skip = np.minimum(s, (s * 5 + ln) % 27)
    e = (s * 521 + ln * 77) & 0xFFFF
    wrap = (s + ln) % 5 == 0
    e[wrap] = (PERIOD - ln[wrap] // 2 - (s[wrap] & 1)) & 0xFFFF
    return assemble(s - skip, skip, ln, e, (np.arange(pos.size), pos, (1 << sweep_bit(pos)).astype(np.uint8)), 384,
                    seed)


# ---- the large shapes ------------------------------------------------------------------------------------------------
# Workgroup path, ragged (scan_buffer): the span starts 3 bytes into slot 5 of its 128-byte line, so cb0 = 8 - 5 = 3
# (head chunks 1 and 2); the interior is one full round and a tail round whose load u = 0 is whole and whose u = 1 is
# partial: WG_ROUND + BLOCK + 20 chunks; then the last chunk, 5 bytes of it.
WG_START = 5 * 16 + 3
WG_TAIL_PARTIAL = 20
WG_NCHUNKS = 3 + WG_ROUND + BLOCK + WG_TAIL_PARTIAL + 1
WG_LENGTH = 16 * (WG_NCHUNKS - 1) + 5 - 3
# the expected offsets: the pattern position of chunk 0 is (e - lo) mod 65536, and the 64 KiB period wraps before chunk
# c when that position + 16 c reaches 65536. Odd phase, the wrap in the full round (chunk 3 + 300); even phase, the wrap
# in the tail round (chunk 3 + WG_ROUND + BLOCK + 7, in its partial load).
WG_E_ODD = (PERIOD - 16 * (3 + 300) + 3 + 7) % PERIOD
WG_E_EVEN = (PERIOD - 16 * (3 + WG_ROUND + BLOCK + 7) + 3 + 8) % PERIOD
# Whole lines (scan_whole_exact): 128-aligned, a full round and a tail round of BLOCK + 20 chunks.
WHOLE_LENGTH = 16 * (WG_ROUND + BLOCK + WG_TAIL_PARTIAL)
WHOLE_E_EVEN = (PERIOD - 16 * 300 + 8) % PERIOD            # the wrap in the full round
WHOLE_E_ODD = (PERIOD - 16 * (WG_ROUND + 100) + 9) % PERIOD  # ... in the tail round
# The production shape: 64 KiB on a line, 4096 chunks = eight full rounds, no tail round.
PROD_LENGTH = 65536
PROD_LANES = (0, 63, 64, 255)
PROD_E = 4096 + 2 * 16  # even; the wrap in round 7
# Quad path: a 1472-byte datagram buffer verified past its 26-byte header (one round), and 3000 bytes starting 7
# bytes into slot 6 of a line: cs = -6, chunks -6 .. 89 in round 0, 90 .. 185 in round 1, the last interior chunk 186
# alone in round 2.
QUAD_A = (HEADER, 1472 - HEADER, HEADER, 0)
QUAD_B_START = 6 * 16 + 7
QUAD_B = (QUAD_B_START, 3000, 9, 65536 - 1234)  # odd phase ((e - lo) & 1), the period's wrap in round 0
# ... and through rings: stride 1536 (twelve lines: every slot alike), and stride 3008 (23.5 lines: the slots
# alternate between cs = 0 and cs = -4), 3000 bytes after 7 skipped ones.
RING_A = (1536, HEADER, 1472 - HEADER, 0)
RING_B = (3008, 7, 3000, 65536 - 1234)


def wg_shape_facts():
    """What the large workgroup shapes rest on; each entry must be true."""
    lo, nch, hi_last, cb0 = (int(x) for x in geometry(WG_START, WG_LENGTH))
    r = wg_roles(WG_START, WG_LENGTH, np.arange(nch))
    tail_u = [int(np.count_nonzero((r["kind"] == TAIL) & (r["u"] == u))) for u in range(WG_LOADS)]
    w = wg_roles(0, WHOLE_LENGTH, np.arange(WHOLE_LENGTH // 16))
    p = wg_roles(0, PROD_LENGTH, np.arange(PROD_LENGTH // 16))

    def wrap_chunk(start, e):  # the chunk that holds the byte at which the pattern position is 0 again
        return (PERIOD - (e - (start & 15)) % PERIOD) // 16
    return {
        "ragged: lo 3, cb0 3, 5 bytes of the last chunk": (lo, cb0, hi_last, nch) == (3, 3, 5, WG_NCHUNKS),
        "ragged: not a whole-line span": not bool(whole_lines(WG_START, WG_LENGTH)),
        "ragged: one full round": int(r["round"][r["kind"] == FULL].max()) == 0
        and int(np.count_nonzero(r["kind"] == FULL)) == WG_ROUND,
        "ragged: tail round, u = 0 whole and u = 1 partial": tail_u[0] == BLOCK and 0 < tail_u[-1] < BLOCK
        and WG_LOADS == 2,
        "ragged: odd phase wraps in the full round": (WG_E_ODD - 3) % 2 == 1
        and int(r["kind"][wrap_chunk(WG_START, WG_E_ODD)]) == FULL,
        "ragged: even phase wraps in the tail round": (WG_E_EVEN - 3) % 2 == 0
        and int(r["kind"][wrap_chunk(WG_START, WG_E_EVEN)]) == TAIL,
        "whole: takes scan_whole_exact": bool(whole_lines(0, WHOLE_LENGTH)) and bool(whole_lines(0, PROD_LENGTH)),
        "whole: a full round and a partial tail round": int(np.count_nonzero(w["kind"] == FULL)) == WG_ROUND
        and int(np.count_nonzero(w["kind"] == TAIL)) == BLOCK + WG_TAIL_PARTIAL and not (w["kind"] < FULL).any(),
        "whole: even phase wraps in the full round, odd in the tail": WHOLE_E_EVEN % 2 == 0 and WHOLE_E_ODD % 2 == 1
        and int(w["kind"][wrap_chunk(0, WHOLE_E_EVEN)]) == FULL and int(w["kind"][wrap_chunk(0, WHOLE_E_ODD)]) == TAIL,
        "64 KiB: full rounds only": bool((p["kind"] == FULL).all())
        and int(p["round"].max()) == PROD_LENGTH // 16 // WG_ROUND - 1,
    }


def quad_shape_facts():
    def rounds(start, length):
        _, nch, _, _ = geometry(start, length)
        return sorted(set(quad_roles(start, length, np.arange(1, int(nch) - 1))["round"].tolist()))
    return {
        "1472 after 26: one round": rounds(QUAD_A[0], QUAD_A[1]) == [0],
        "3000 at slot 6 + 7: cs -6, three rounds": int(geometry(QUAD_B[0], QUAD_B[1])[3]) - 8 == -6
        and rounds(QUAD_B[0], QUAD_B[1]) == [0, 1, 2],
        "ring 3008: the slots alternate between two line slots": {int(geometry((i * RING_B[0] + RING_B[1]) % 128, 1)[3])
                                                                 for i in range(4)} == {8, 4},
        "ring 3008: two rounds and more": rounds(RING_B[1], RING_B[2])[-1] >= 1
        and rounds(RING_B[1] + 64, RING_B[2])[-1] >= 1,
    }


def landmarks(path, start, length):
    """About 30 positions of a span: its first and last byte, one byte in a head chunk, lanes 0, 63, 64, 127, 128 and
    255 of each (round, u) of the workgroup path (team lanes 0, 1, 15 of the quad path), the first and the last chunk
    of the last round, and chunk nchunks - 2. The byte within a chunk varies with the chunk."""
    lo, nch, _, _ = (int(x) for x in geometry(start, length))
    chunks = np.arange(nch)
    r = ROLES[path](start, length, chunks)
    picks = set()
    lanes = (0, 63, 64, 127, 128, 255) if path == "wg" else (0, 1, 15)
    streamed = r["kind"] >= FULL
    for key in np.unique(role_key(r, by_wave=False)[streamed]):
        mine = streamed & (role_key(r, by_wave=False) == key)
        picks.update(int(c) for c in chunks[mine & np.isin(r["lane"], lanes)])
    if streamed.any():
        last_round = streamed & (r["kind"] == r["kind"][streamed][-1]) & (r["round"] == r["round"][streamed][-1])
        picks.update((int(chunks[last_round][0]), int(chunks[last_round][-1])))
    if (r["kind"] == HEAD).any():
        picks.add(int(chunks[r["kind"] == HEAD][0]))
    picks.add(max(nch - 2, 0))
    pos = {min(max(16 * c + (5 * c + 3) % 16 - lo, 0), length - 1) for c in picks}
    return sorted(pos | {0, length - 1})


@functools.lru_cache(maxsize=None)
def wg_plan(name):
    """The plans of the workgroup path (hint 0)."""
    if name == "small":
        return small_sweep()
    if name == "ragged_odd":
        return sweep(WG_START, WG_LENGTH, 17, WG_E_ODD, seed=11)
    if name == "ragged_even":
        return sweep(WG_START, WG_LENGTH, 0, WG_E_EVEN, seed=12)
    if name == "whole_even":
        return sweep(0, WHOLE_LENGTH, 0, WHOLE_E_EVEN, seed=13)
    if name == "whole_odd":
        return sweep(0, WHOLE_LENGTH, 0, WHOLE_E_ODD, seed=14)
    if name == "prod":  # every byte of the chunks at PROD_LANES of each (round, u)
        c = np.arange(PROD_LENGTH // 16)
        at = c[np.isin(wg_roles(0, PROD_LENGTH, c)["lane"], PROD_LANES)]
        return sweep(0, PROD_LENGTH, 0, PROD_E, positions=(at[:, None] * 16 + np.arange(16)).reshape(-1), seed=15)
    if name == "pairs_ragged":
        return pairs(WG_START, WG_LENGTH, 17, WG_E_ODD, landmarks("wg", WG_START, WG_LENGTH), seed=16)
    if name == "pairs_whole":
        return pairs(0, WHOLE_LENGTH, 0, WHOLE_E_ODD, landmarks("wg", 0, WHOLE_LENGTH), seed=17)
    if name == "shifted_ragged":
        return shifted(WG_START, WG_LENGTH, 17, WG_E_ODD, seed=18)
    if name == "shifted_whole":
        return shifted(0, WHOLE_LENGTH, 0, WHOLE_E_EVEN, seed=19)
    raise KeyError(name)


WG_PLANS = ("small", "ragged_odd", "ragged_even", "whole_even", "whole_odd", "prod", "pairs_ragged", "pairs_whole",
            "shifted_ragged", "shifted_whole")


@functools.lru_cache(maxsize=None)
def quad_plan(name):
    """The plans of the quad path (hint 1472): descriptors, and (ring_*) strided rings."""
    if name == "small":
        return small_sweep()
    if name == "a":
        return sweep(*QUAD_A, seed=21)
    if name == "b":
        return sweep(*QUAD_B, all_bits=True, seed=22)
    if name == "pairs":
        return pairs(*QUAD_B, landmarks("quad", QUAD_B[0], QUAD_B[1]), seed=23)
    if name == "shifted":
        return shifted(*QUAD_B, seed=24)
    if name == "ring_a":
        return sweep(RING_A[1], RING_A[2], RING_A[1], RING_A[3], stride=RING_A[0], seed=25)
    if name == "ring_b":
        return sweep(RING_B[1], RING_B[2], RING_B[1], RING_B[3], stride=RING_B[0], all_bits=True, seed=26)
    raise KeyError(name)


QUAD_PLANS = ("small", "a", "b", "pairs", "shifted", "ring_a", "ring_b")


# ---- a plain verifier over the plans, and its broken forms -----------------------------------------------------------
def diff_entries(plan):
    """(row, position) of every byte of a verified span that differs from the pattern, in row-major order."""
    d = plan.descs
    n = len(d)
    off = d["byte_offset"].astype(np.int64) - np.arange(n, dtype=np.int64) * plan.slot
    skip, length, e = d["skip_head"].astype(np.int64), span_length(plan), d["expected_pattern_offset"].astype(np.int64)
    rows = plan.arena[:n * plan.slot].reshape(n, plan.slot)
    if _uniform(off) and _uniform(skip) and _uniform(length) and _uniform(e):
        c0 = int(off[0] + skip[0])
        return np.nonzero(rows[:, c0:c0 + int(length[0])] != pattern(int(e[0]) + np.arange(int(length[0])))[None, :])
    out = []

    def take(lo, hi, cols, mask, exp):
        r, c = np.nonzero(mask & (rows[lo:hi] != exp))
        out.append((r + lo, cols[r, c].astype(np.int64)))
    _columns(off, skip, length, e, plan.slot, take)
    return np.concatenate([r for r, _ in out]), np.concatenate([p for _, p in out])


def records(plan, row, pos, drop_first=None, drop_count=None):
    """The verifier's outputs from the differing bytes (row, pos): (results, counters, first-failure slots).
    drop_first / drop_count: masks of entries a broken verifier does not see when it takes the minimum / the count."""
    d = plan.descs
    n = len(d)
    length = span_length(plan)
    kf = slice(None) if drop_first is None else ~drop_first
    kc = slice(None) if drop_count is None else ~drop_count
    first = np.full(n, 1 << 40, dtype=np.int64)
    np.minimum.at(first, row[kf], pos[kf])
    count = np.bincount(row[kc], minlength=n)
    bad = (first < (1 << 40)) | (count > 0)
    first = np.where(first < (1 << 40), first, 0)
    res = np.zeros(n, dtype=RESULT_DTYPE)
    res["first_mismatch"] = np.where(bad, first, length)
    res["mismatch_bytes"] = np.where(bad, count, 0)
    res["expected"] = np.where(bad, pattern(d["expected_pattern_offset"].astype(np.int64) + first), 0)
    res["actual"] = np.where(bad, plan.arena[d["byte_offset"].astype(np.int64) + d["skip_head"] + first], 0)
    res["pass"] = ~bad
    return (res,) + summary(d, res)


def summary(descs, res):
    """The counter block and the first-failure slots that follow from per-buffer results."""
    length = descs["length"].astype(np.int64) - descs["skip_head"]
    ok = res["pass"] == 1
    ctr = {"bytes_checked": int(length.sum()), "bytes_ok": int(length[ok].sum()), "buffers_checked": len(descs),
           "buffers_failed": int(np.count_nonzero(~ok)), "mismatched_bytes": int(res["mismatch_bytes"].sum())}
    slots = np.full(N_CONNS, EMPTY, dtype=np.uint32)
    idx = np.nonzero(~ok & (descs["conn_index"] < N_CONNS))[0]
    np.minimum.at(slots, descs["conn_index"][idx], idx.astype(np.uint32))
    return ctr, slots


def closed_form(plan):
    """The records of a plan of flips, without looking at the arena: first = the lowest flipped position, count = the
    flips, expected = P(e + first), actual = expected ^ the flip there."""
    fr, fp, fx = plan.flips
    d = plan.descs
    n = len(d)
    length = span_length(plan)
    first = np.full(n, 1 << 40, dtype=np.int64)
    np.minimum.at(first, fr, fp)
    bad = first < (1 << 40)
    x_first = np.zeros(n, dtype=np.uint8)
    lowest = fp == first[fr]
    x_first[fr[lowest]] = fx[lowest]
    exp = pattern(d["expected_pattern_offset"].astype(np.int64) + np.where(bad, first, 0))
    res = np.zeros(n, dtype=RESULT_DTYPE)
    res["first_mismatch"] = np.where(bad, first, length)
    res["mismatch_bytes"] = np.bincount(fr, minlength=n)
    res["expected"] = np.where(bad, exp, 0)
    res["actual"] = np.where(bad, exp ^ x_first, 0)
    res["pass"] = ~bad
    return res


def entry_roles(plan, path, row, pos):
    """The role model at the entries (row, pos): the roles' arrays plus lo, hi_last, nch, chunk and byte (in chunk)."""
    start, length = span_start(plan)[row], span_length(plan)[row]
    lo, nch, hi_last, _ = geometry(start, length)
    chunk = (lo + pos) >> 4
    r = dict(ROLES[path](start, length, chunk))
    r.update(lo=lo, hi_last=hi_last, nch=nch, chunk=chunk, byte=(lo + pos) & 15, pos=pos, length=length,
             whole=whole_lines(start, length))
    r["key"] = role_key(r, by_wave=path == "wg")
    return r


def mutants(path, r, by_wave=True):
    """Broken verifiers for the entries' roles r, as (name, drop_first, drop_count): one per role that ignores the
    role's chunks; off-by-one byte masks at the span's two ends; a tail or last round that stops one chunk early; a
    first head chunk nobody owns; and, per wave (team lane of the quad path), a reduction that loses that wave's
    minimum when another wave is dirty too (first only; caught by plans with two dirty waves)."""
    out = []
    key = r["key"] if by_wave else role_key(r, by_wave=False)
    for k in np.unique(key):
        m = key == k
        out.append(("ignores " + role_name(k), m, m))
    m = r["pos"] == 0
    out.append(("masks the first byte", m, m))
    m = r["pos"] == r["length"] - 1
    out.append(("masks the last byte", m, m))
    inner = r["kind"] >= FULL
    if inner.any():
        # (a whole-line span of the workgroup path has no last chunk of its own: it streams up to nch - 1)
        m = inner & (r["chunk"] == np.where(r["whole"] & (path == "wg"), r["nch"] - 1, r["nch"] - 2))
        out.append(("drops the last interior chunk", m, m))
    if (r["kind"] == HEAD).any():
        m = (r["kind"] == HEAD) & (r["chunk"] == 1)
        out.append(("owns no head chunk 1", m, m))
    return out


def lost_minimum_mutants(path, r, row):
    """Per wave (team lane): the reduction loses that wave's minimum in buffers where another wave is dirty as well."""
    who = r["wave"] if path == "wg" else r["lane"]
    n = int(row.max()) + 1 if row.size else 0
    out = []
    for w in np.unique(who):
        others = np.bincount(row[who != w], minlength=n) > 0
        out.append(("loses the minimum of %s %d" % ("wave" if path == "wg" else "lane", int(w)),
                    (who == w) & others[row], None))
    return out


def coverage_gaps(plan, path, by_wave=True):
    """Roles without their buffers: for every shape of the plan and every role of the shape, the first and the last
    verified byte of the first and of the last chunk of the role's chunk range must each be the only corrupt byte of
    some buffer. Returns the missing (start, length, role, position) facts."""
    fr, fp, _ = plan.flips
    single = np.bincount(fr, minlength=len(plan.descs)) == 1
    start, length = span_start(plan), span_length(plan)
    keep = single[fr]
    have = set(zip(start[fr[keep]].tolist(), length[fr[keep]].tolist(), fp[keep].tolist()))
    gaps = []
    for s, ln in sorted(set(zip(start.tolist(), length.tolist()))):
        lo, nch, _, _ = (int(x) for x in geometry(s, ln))
        chunks = np.arange(nch)
        r = ROLES[path](s, ln, chunks)
        key = role_key(r, by_wave=by_wave and path == "wg")
        assert (r["kind"] >= 0).all()
        for k in np.unique(key):
            mine = chunks[key == k]
            assert mine[-1] - mine[0] + 1 == mine.size or not by_wave  # a role's chunks are one range
            for c in (int(mine[0]), int(mine[-1])):
                for p in (max(16 * c - lo, 0), min(16 * c + 15 - lo, ln - 1)):
                    if (s, ln, p) not in have:
                        gaps.append((s, ln, role_name(k), p))
    return gaps


def wave_order_gaps(plan, path):
    """The pairs plan: ordered pairs (a, b), a != b, of waves (team lanes 0, 1, 15 of the quad path) for which no
    buffer has its earlier byte in a and its later byte in b."""
    fr, fp, _ = plan.flips
    two = np.nonzero(np.bincount(fr, minlength=len(plan.descs)) == 2)[0]
    order = np.lexsort((fp, fr))
    fr, fp = fr[order], fp[order]
    r = entry_roles(plan, path, fr, fp)
    who = r["wave"] if path == "wg" else r["lane"]
    sel = np.isin(fr, two)
    w = who[sel].reshape(-1, 2)
    have = set(map(tuple, w.tolist()))
    ids = sorted(set(who.tolist())) if path == "wg" else [0, 1, QUAD_TEAM - 1]
    return [(a, b) for a in ids for b in ids if a != b and (a, b) not in have]


# ---- the host paths: one call per corrupted buffer -------------------------------------------------------------------
MAIL_OFFSET = 5          # the buffer's offset in its pinned arena (lo of its chunk 0)
MAIL_LENGTH = 70000
MAIL_E = 60001           # odd; the period wraps in piece 1
MAIL_SEAMS = (0, 3, 4, 15, 16)
MAIL_WAVE_PIECE = 9
MAIL_STRIDE = 37
SMALL_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33)


def _chunk_bytes(lo, length, c):
    return list(range(max(16 * c - lo, 0), min(16 * c + 16 - lo, length)))


@functools.lru_cache(maxsize=None)
def mail_cases():
    """The corruptions of the 70 000-byte host buffer, each a tuple of (position, xor) pairs: every byte of chunk 0, of
    the last chunk, of the last chunk of piece k and the first of piece k + 1 for k in MAIL_SEAMS, of one chunk per
    data wave of piece MAIL_WAVE_PIECE; every MAIL_STRIDE-th byte of the rest; pairs across pieces, workgroups and
    loop passes (the earlier byte in the later workgroup, wave or pass among them)."""
    lo, nch, _, _ = (int(x) for x in geometry(MAIL_OFFSET, MAIL_LENGTH))
    chunks = {0, nch - 1}
    for k in MAIL_SEAMS:
        chunks.update(((k + 1) * MAIL_PIECE_CHUNKS - 1, (k + 1) * MAIL_PIECE_CHUNKS))
    chunks.update(MAIL_WAVE_PIECE * MAIL_PIECE_CHUNKS + 64 * w + 7 * w + 1 for w in range(4))
    pos = set()
    for c in chunks:
        pos.update(_chunk_bytes(lo, MAIL_LENGTH, c))
    pos.update(range(0, MAIL_LENGTH, MAIL_STRIDE))
    singles = [((p, 1 << int(sweep_bit(p))),) for p in sorted(pos)]

    def at(piece, chunk_in_piece, byte):
        return 16 * (piece * MAIL_PIECE_CHUNKS + chunk_in_piece) + byte - lo
    marks = [at(0, 0, 5), at(0, 255, 15), at(1, 0, 0), at(1, 64, 3), at(2, 130, 9), at(3, 200, 1), at(4, 10, 0),
             at(5, 70, 7), at(6, 33, 6), at(15, 255, 15), at(16, 0, 0), at(16, 100, 2), at(17, 5, 4), MAIL_LENGTH - 1]
    both = [((a, 0x01 << (k % 8)), (b, 0xFF ^ (0x01 << (k % 8))))
            for k, (a, b) in enumerate((a, b) for i, a in enumerate(marks) for b in marks[i + 1:])]
    return tuple(singles + both)


def small_mail_cases():
    """(lo, length, position) for every byte of the lengths SMALL_LENGTHS at every offset lo 0..15."""
    return [(lo, n, p) for lo in range(16) for n in SMALL_LENGTHS for p in range(n)]


# ---- the MediaStream receive -----------------------------------------------------------------------------------------
MS_DATAGRAM = 1472
MS_SHORT = (27, 41, 42, 58)
MS_SLOT = 1536           # descriptor form: one datagram per 1536-byte row, at byte ho of it
MS_STRIDE = 1489         # strided form: odd, so slot i lies at ho = (i * 1489) mod 16 and every ho occurs equally often
MS_WINDOW = (3, 10 ** 12, 64)  # head sequence number, final frame, window slots of the frames form
MsPlan = collections.namedtuple("MsPlan", "arena descs lengths stride ho completed flip_at flip_xor")


def _ms_items():
    """Per ho 0..15 the same items (completed bytes, flipped datagram byte or -1, xor): every payload byte of a
    1472-byte datagram and of the lengths MS_SHORT; each bit of header bytes 0..1 (at 1472 and at 30 completed bytes:
    flag 0x1000 makes the first an ID datagram, the second too short for one); each bit of header bytes 2..25; clean
    copies."""
    items = []
    for comp in (MS_DATAGRAM,) + MS_SHORT:
        p = np.arange(comp - HEADER)
        items += [(comp, HEADER + int(i), 1 << int(b)) for i, b in zip(p, sweep_bit(p))]
    for comp in (MS_DATAGRAM, 30):
        items += [(comp, byte, 1 << bit) for byte in (0, 1) for bit in range(8)]
    items += [(MS_DATAGRAM, byte, 1 << bit) for byte in range(2, HEADER) for bit in range(8)]
    clean = (MS_DATAGRAM,) + MS_SHORT + (HEADER,)  # (26 completed bytes: a header and no payload)
    return items + [(clean[k % len(clean)], -1, 0) for k in range((len(items) + 2) // 3)]


@functools.lru_cache(maxsize=None)
def ms_plan(strided, seed=31):
    """The datagrams of the MediaStream sweep as descriptors (one per MS_SLOT-byte row, at byte ho) or as a ring of
    stride MS_STRIDE. Headers: flag 0, sequence numbers around the frames window, nonzero qpc / qpf."""
    items = _ms_items()
    m = len(items)
    n = 16 * m
    comp = np.tile(np.array([c for c, _, _ in items], dtype=np.int64), 16)
    flip_at = np.tile(np.array([a for _, a, _ in items], dtype=np.int64), 16)
    flip_x = np.tile(np.array([x for _, _, x in items], dtype=np.uint8), 16)
    ho = np.repeat(np.arange(16), m)
    rng = np.random.default_rng(seed)
    row_of = np.empty(n, dtype=np.int64)
    if strided:
        slot_ho = (np.arange(n, dtype=np.int64) * MS_STRIDE) & 15
        for h in range(16):  # the items of an ho go, shuffled, to the slots that lie at that ho
            rows = np.nonzero(slot_ho == h)[0]
            assert rows.size == m
            row_of[h * m:(h + 1) * m] = rng.permutation(rows)
        stride, off = MS_STRIDE, np.zeros(n, dtype=np.int64)
    else:
        row_of[:] = rng.permutation(n)
        stride, off = MS_SLOT, ho
    item_of = np.empty(n, dtype=np.int64)
    item_of[row_of] = np.arange(n)
    comp, flip_at, flip_x, off = comp[item_of], flip_at[item_of], flip_x[item_of], off[item_of]
    arena = np.full(n * stride + 64, GAP, dtype=np.uint8)
    base = np.arange(n, dtype=np.int64) * stride + off
    hdr = np.zeros(n, dtype=DGRAM_HEADER_DTYPE)
    hdr["sequence_number"] = np.arange(n) % 80  # MS_WINDOW holds 3 .. 66: some fall outside it
    hdr["qpc"], hdr["qpf"] = 10 ** 15 + 977 * np.arange(n), 10 ** 7 + np.arange(n)
    hb = np.zeros((n, HEADER), dtype=np.uint8)
    hb[:, 2:] = hdr.view(np.uint8).reshape(n, 24)
    body = np.concatenate([hb, np.broadcast_to(pattern(np.arange(MS_DATAGRAM - HEADER)), (n, MS_DATAGRAM - HEADER))],
                          axis=1)
    cols = np.arange(MS_DATAGRAM)[None, :]
    live = cols < comp[:, None]
    arena[(base[:, None] + cols)[live]] = body[live]
    hit = flip_at >= 0
    assert (flip_at[hit] < comp[hit]).all()
    arena[base[hit] + flip_at[hit]] ^= flip_x[hit]
    descs = np.zeros(n, dtype=DESC_DTYPE)
    descs["byte_offset"], descs["length"], descs["conn_index"] = base, comp, np.arange(n) % N_CONNS
    return MsPlan(arena, descs, comp.astype(np.uint32), stride, (base & 15), comp, flip_at, flip_x)


def ms_closed_form(plan):
    """(kind, pass, first_mismatch, mismatch_bytes, expected, actual) of every datagram of an ms_plan: a payload flip
    fails the datagram at that byte; flag bit 12 alone makes an ID datagram (too short below 39 bytes), any other flag
    bit an unknown one; a flip in header bytes 2..25 changes no verdict."""
    at, x, comp = plan.flip_at, plan.flip_xor.astype(np.int64), plan.completed
    flag = np.where(at == 0, x, np.where(at == 1, x << 8, 0))
    kind = np.where(flag == 0, 0, np.where(flag == 0x1000, np.where(comp < 39, 3, 1), 4))
    payload = (at >= HEADER) & (kind == 0)
    exp = pattern(np.where(payload, at - HEADER, 0))
    return {"kind": kind, "pass": ((kind == 0) & ~payload).astype(np.uint8),
            "first_mismatch": np.where(kind == 0, np.where(payload, at - HEADER, comp - HEADER), 0),
            "mismatch_bytes": payload.astype(np.int64), "expected": np.where(payload, exp, 0),
            "actual": np.where(payload, exp ^ plan.flip_xor, 0)}


def ms_frame_sums(recs, res, window=MS_WINDOW):
    """What the frames form sums for a batch under `window` (not finished), from per-datagram records and results:
    (totals dict, bytes per window slot)."""
    head, final, frames = window
    clean = (recs["kind"] == 0) & (res["pass"] == 1)
    seq = recs["sequence_number"].astype(np.int64)[clean]
    comp = recs["completed_bytes"].astype(np.int64)[clean]
    k = seq - head
    err = (seq > final) | (k < 0) | (k >= frames)
    fb = np.zeros(frames, dtype=np.uint64)
    np.add.at(fb, k[~err], comp[~err].astype(np.uint64))
    exc = np.nonzero(~clean)[0]
    return {"bits_received": int(8 * comp.sum()), "error_frames": int(np.count_nonzero(err)),
            "datagrams": int(np.count_nonzero(clean)), "first_exception": int(exc[0]) if exc.size else EMPTY,
            "exceptions": int(exc.size)}, fb
