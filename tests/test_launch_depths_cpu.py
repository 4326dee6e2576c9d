"""CPU: what tests/test_loop_depth_gpu.py rests on (tests/launch_depths.py).

1. The model's grid rules are the launchers': tests/cpp/grids_check.cpp, built here with g++ over
   ctstraffic_amd/csrc/cts_grids.hpp (the header the launchers of the kernel units call), prints the same numbers, at,
   one below and one above every cap, for 64, 104, 228, 256 and 304 compute units.
2. Every shape of the loop-depth tests reaches its depth facts at each of those CU counts, and the depth functions
   agree with plain one-item-at-a-time loops on a small device.
3. The shapes of the older small exact tests reach none of them at 256 CUs and default attributes: the gap the
   loop-depth tests close. Where a shape does reach something, the assertion says what.
"""
import os
import subprocess

import numpy as np
import pytest

import launch_depths as L
from ctstraffic_amd.types import DESC_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = L.CU_COUNTS


# ---- 1. the grid rules -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grids_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grids") / "grids_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ctstraffic_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "grids_check.cpp"), "-o", exe], check=True)
    return exe


def _tuples():
    out = []
    for cus in CUS:
        for bpc in (0, 1, 4, 64):
            cap = cus * (bpc if bpc > 0 else 8)
            ring_cap = cus * (bpc if bpc > 0 else 4)
            for chunk, hint in ((0, 0), (16, 9000), (48, 65536), (L.RING_CHUNK_D1, 1 << 20), (200, 70000)):
                ppb = max(1, (hint + L.FILL_PIECE - 1) // L.FILL_PIECE)
                per = max(16, (chunk + 15) // 16 * 16)
                at = {cap, 4 * cap, 16 * cap, 2 * 16 * cap, per * cap, ring_cap * L.FILL_BATCH,
                      ring_cap * L.RING_BATCH, cus * max(bpc, 1) // ppb, cus * max(bpc, 1) * 16 // ppb}
                ns = {1, 15, 16, 17, (1 << 32) - 1} | {n + d for n in at for d in (-1, 0, 1)}
                out += [(n, cus, bpc, chunk, hint) for n in sorted(ns) if 0 < n < 1 << 32]
    return out


def test_rules_are_the_launchers(grids_check):
    tuples = _tuples()
    assert len(tuples) > 2000
    got = []
    for k in range(0, len(tuples), 500):  # a few hundred tuples per command line
        out = subprocess.run([grids_check] + [str(x) for t in tuples[k:k + 500] for x in t], check=True,
                             capture_output=True, text=True).stdout.split("\n")
        got += [tuple(int(x) for x in line.split()) for line in out if line]
    assert got == [L.rules(*t) for t in tuples]
    # the figures the issue's reading rests on, at 256 CUs and default attributes
    assert L.piece_fill_grid(400, 65536, 256, 1) == (256, 8) and L.piece_fill_grid(101, 1 << 20, 256, 1) == (256, 128)
    assert L.grid_for(400, 4, 256, 64) == 100 and L.grid_for(4 * 16384 + 1, 4, 256, 64) == 8193
    assert L.contig_grid(262144, 256, 64, 0) == (16384, 16) and L.contig_grid(1000, 256, 1, 16) == (63, 16)
    assert L.batch_fill_grid(315, L.FILL_BATCH, 256, 4) == 2 and L.batch_fill_grid(3000, L.RING_BATCH, 256, 4) == 6
    assert subprocess.run([grids_check, "0", "4", "1", "0", "0"], capture_output=True).returncode == 2
    assert subprocess.run([grids_check, "5", "4", "1"], capture_output=True).returncode == 2


# ---- 2. the depth functions against plain loops, and the new shapes --------------------------------------------------
def _pieces_by_loops(descs, hint, cus, arena_bytes):
    """fill_pieces_kernel's loops, one workgroup, batch and lane at a time."""
    n = len(descs)
    G, ppb = L.piece_fill_grid(n, hint, cus, 1)
    total = n * ppb
    batches, ragged, where = [], 0, {}
    empty = live = rest = 0
    for b in range(G):
        v0, nb, rag = b, 0, False
        while v0 < total:
            for m in range(L.PIECE_BATCH):
                v = v0 + m * G
                if v >= total:
                    rag = True
                    continue
                i, pc = divmod(v, ppb)
                where.setdefault(i, set()).add(nb)
                d = descs[i]
                off, ln, sk = int(d["byte_offset"]), int(d["length"]), int(d["skip_head"])
                if int(d["expected_pattern_offset"]) >= 65536 or ln < sk or off > arena_bytes or arena_bytes - off < ln \
                        or ln == sk:
                    continue
                nchunks = (((off + sk) & 15) + ln - sk + 15) >> 4
                if pc * L.PIECE_CHUNKS >= nchunks:
                    empty += 1
                    continue
                live += 1
                rest += pc + 1 == ppb and nchunks > (pc + 1) * L.PIECE_CHUNKS
            v0 += L.PIECE_BATCH * G
            nb += 1
        batches.append(nb)
        ragged += rag
    return {"batches_min": min(batches), "batches_max": max(batches), "ragged_workgroups": ragged,
            "split_buffers": sum(1 for s in where.values() if len(s) > 1), "empty_pieces": empty, "live_pieces": live,
            "rest_pieces": rest}


@pytest.mark.parametrize("kind", L.PIECE_KINDS)
def test_piece_depth_against_plain_loops(kind):
    descs, arena_bytes = L.piece_case(kind, 6)
    d = L.piece_fill_depth(descs, L.PIECE_HINT[kind], 6, 1, arena_bytes)
    loops = _pieces_by_loops(descs, L.PIECE_HINT[kind], 6, arena_bytes)
    assert {k: d[k] for k in loops} == loops
    assert d["rest_whole"] + d["rest_edge"] == d["rest_pieces"]


def _quad_by_loops(n, cus, sbpc, chunk):
    """QuadWalk as the kernels run it: every team's i and next(), the wave's loop while any team is inside."""
    grid, per = L.contig_grid(n, cus, sbpc, chunk)
    rounds = np.zeros((grid, 4), dtype=np.int64)
    crossing, full = 0, np.zeros((grid, 4), dtype=np.int64)
    for b in range(grid):
        for w in range(4):
            cbase = [b * per] * 4
            i = [min(b * per + 4 * w + t, n) for t in range(4)]
            crossed, rs = False, 0
            while any(x < n for x in i):
                rounds[b, w] += 1
                for t in range(4):
                    nx = i[t] + L.QUAD_TEAMS
                    if nx - cbase[t] >= per:
                        cbase[t] += grid * per
                        nx = cbase[t] + 4 * w + t
                        crossed = crossed or (t == 0 and nx < n)
                    i[t] = min(nx, n)
                rs += 1
                if rs == L.MS_RING:
                    full[b, w] += 1
                    rs = 0
            crossing += crossed
    return rounds, crossing, full


@pytest.mark.parametrize("n,cus,sbpc,chunk", [(16 * 2 * 3 + 21, 2, 1, 0), (16 * 2 * 3 + 21, 2, 1, 16),
                                              (16 * 2 * 3 + 21, 2, 1, 48), (48 * 22 * 2 + 48 * 5 + 21, 2, 1, 48),
                                              (3 * 2128 + 77, 2, 64, 2128), (1000, 3, 2, 48), (5009, 4, 1, 200)])
def test_quad_depth_against_plain_loops(n, cus, sbpc, chunk):
    d = L.quad_walk_depth(n, cus, sbpc, chunk)
    rounds, crossing, full = _quad_by_loops(n, cus, sbpc, chunk)
    assert np.array_equal(d["rounds"], rounds) and d["crossing_waves"] == crossing
    assert np.array_equal(d["full_flushes"], full)
    assert d["partial_after_full"] == int(((full > 0) & (rounds % L.MS_RING > 0)).sum())


@pytest.mark.parametrize("cus", CUS)
def test_new_shapes_reach_their_depths(cus):
    for kind in L.PIECE_KINDS:
        descs, arena_bytes = L.piece_case(kind, cus)
        assert len(descs) == L.piece_n(kind, cus)
        assert L.piece_reaches(kind, L.piece_fill_depth(descs, L.PIECE_HINT[kind], cus, 1, arena_bytes)) == [], kind
    for lanes in (64, 256):
        assert L.team_fill_reaches(L.team_fill_depth(L.team_fill_n(lanes, cus), lanes, cus, 1)) == [], lanes
    for chunk in L.QUAD_CHUNKS:
        assert L.quad_reaches(chunk, L.quad_walk_depth(L.quad_n(cus), cus, 1, chunk)) == [], chunk
    assert L.ring_reaches("d1", L.quad_walk_depth(L.ring_n("d1", cus), cus, 64, L.RING_CHUNK_D1)) == []
    assert L.ring_reaches("d2", L.quad_walk_depth(L.ring_n("d2", cus), cus, 1, 48)) == []
    for kind, batch, stride in (("descs", L.FILL_BATCH, 0), ("ring64", L.RING_BATCH, 64),
                                ("ring1040", L.RING_BATCH, 1040)):
        assert L.batched_reaches(kind, L.batch_fill_depth(L.batched_n(kind, cus), batch, cus, 1, stride)) == [], kind


def test_sizes_at_256_compute_units():
    """The sizes the tests run at on an MI355X: a few seconds each."""
    assert [L.piece_n(k, 256) for k in L.PIECE_KINDS] == [1283, 1140, 101, 5125]
    assert (L.team_fill_n(64, 256), L.team_fill_n(256, 256), L.quad_n(256)) == (3077, 899, 12309)
    assert (L.ring_n("d1", 256), L.ring_n("d2", 256)) == (6461, 270597)
    assert [L.batched_n(k, 256) for k in ("descs", "ring64", "ring1040")] == [135936, 267008, 135936]


# ---- 3. the older small tests stay in the first pass -----------------------------------------------------------------
def _uniform_descs(n, length):
    d = np.zeros(n, dtype=DESC_DTYPE)
    d["length"] = length
    d["byte_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(length)
    return d


def test_older_shapes_stay_in_the_first_pass():
    cus = 256
    # fill_pieces_kernel: _fill_vs_oracle (400 buffers, hints 65536 / 70000 / 9000) and test_fill_skips_bad_descriptors
    # (300), fill_blocks_per_cu 1: one batch, so `cur = nxt` never hands over a decoded piece. (The single batch is
    # ragged: lanes with v >= total are reached, in the first batch.)
    for n, hint in ((400, 65536), (400, 70000), (400, 9000), (300, 65536), (300, 9000)):
        d = L.piece_fill_depth(_uniform_descs(n, 60000), hint, cus, 1, n * 60000)
        assert d["batches_max"] == 1 and d["split_buffers"] == 0 and d["ragged_workgroups"] > 0, (n, hint)
    # fill_kernel<64>: 400 buffers at small_blocks_per_cu 64: no team takes a second buffer
    d = L.team_fill_depth(400, 64, cus, 64)
    assert d["passes_max"] == 1
    # (fill_kernel<kBlock> at hint 0 does take a second pass in _fill_vs_oracle: 400 buffers over 200 workgroups)
    assert L.team_fill_depth(400, 256, cus, 1)["passes_max"] == 2
    # verify_quad_kernel: test_small_path_parity, at most 1000 buffers: no block walks a second chunk at any
    # (sbpc, chunk) it sets, and one round per wave at chunk 0 and 16. At chunk 48 a wave does walk the three rounds of
    # its one chunk.
    for n in (301, 257, 120, 1000, 7):
        for sbpc, chunk in ((1, 0), (64, 0), (1, 16), (2, 48)):
            d = L.quad_walk_depth(n, cus, sbpc, chunk)
            assert d["crossing_waves"] == 0 and int(d["chunks"].max()) == 1, (n, sbpc, chunk)
            assert d["rounds_max"] == (1 if chunk != 48 else min(3, (n + 15) // 16)), (n, sbpc, chunk)
    d = L.quad_walk_depth(4099, cus, 2, 48)   # its udp_datagrams workload, under the attributes the loop left
    assert d["crossing_waves"] == 0 and d["rounds_max"] == 3
    d = L.quad_walk_depth(262144, cus, 64, 0)  # test_config3_scaled_vs_oracle
    assert d["rounds_max"] == 1 and d["crossing_waves"] == 0
    # the MediaStream receive: test_gpu_media_stream_verify_matches_oracle, 5009 datagrams: 13 rounds at the most, no
    # wave fills its ring of 64 (with chunk 16 a block does walk two chunks)
    deepest = 0
    for sbpc, chunk in ((1, 0), (64, 0), (1, 16), (2, 48), (1, 200), (64, 0)):
        d = L.quad_walk_depth(5009, cus, sbpc, chunk)
        assert int(d["full_flushes"].max()) == 0, (sbpc, chunk)
        deepest = max(deepest, d["rounds_max"])
    assert deepest == 13 and L.quad_walk_depth(5009, cus, 1, 16)["crossing_waves"] > 0
    assert int(L.quad_walk_depth(7000, cus, 64, 0)["full_flushes"].max()) == 0  # the strided receive test
    # the batched fills: 315 datagrams through descriptors, at most 3000 in a ring: one LDS batch per workgroup
    assert L.batch_fill_depth(315, L.FILL_BATCH, cus, 4)["batches_max"] == 1
    for n, stride in ((3000, 64), (700, 1024), (700, 4096)):
        d = L.batch_fill_depth(n, L.RING_BATCH, cus, 4, stride)
        assert d["batches_max"] == 1 and d.get("crossing_rounds_later", 0) == 0
    # ms_server_fill's several-batches test runs three batches, at stride 64 only
    d = L.batch_fill_depth(2 * 512 * cus + 77, L.RING_BATCH, cus, 1, 64)
    assert d["batches_max"] == 3 and "crossing_rounds_later" not in d
