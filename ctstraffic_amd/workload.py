"""Synthetic workloads for the BASELINE.json configs (host-side descriptor/corruption plans).

Everything here is deterministic from the seeds SURVEY.md §8(d) fixes:

* config 2 — 4096 x 64 KiB resident buffers; expected offsets 75 % phase 0,
  25 % uniform in [0, 65535] (seed 0xC75); 1 in 1024 buffers corrupted by XOR of
  one random byte with a nonzero random value (seed 0xBAD).
* config 3 — 16 M x 1472-byte MediaStream datagrams: 26-byte data header
  (u16 flag 0, i64 seq = i+1, i64 qpc 0, i64 qpf 0 — ctsMediaStreamProtocol.hpp:43-52)
  + P[0..1445]; the payload is verified at expected offset 0
  (ctsIOPatternMediaStream.cpp:185-192). Same corruption rate/seed.
* config 4/5 — 1024 connections x 1024 buffers per 1 M, sharded by
  hash(conn_index) mod G; expected offsets = per-connection exclusive prefix
  sum of lengths mod 65536 (ctsIOPattern.cpp:491-492).

A corruption plan is (buffer index, byte position inside the verified region,
xor value). Because every injected position is distinct per buffer and the xor
is nonzero, the exact reference outcome follows analytically:
first_mismatch = min position, mismatch_bytes = # positions, and the counters
(see :func:`expected_results`) — this is what the full-size GPU tests check.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from .types import DESC_DTYPE

PATTERN_PERIOD = 65536
UDP_DATA_HEADER_LENGTH = 26
SEED_OFFSETS = 0xC75
SEED_CORRUPT = 0xBAD


@dataclass
class Workload:
    name: str
    descs: np.ndarray                    # DESC_DTYPE
    arena_bytes: int
    max_length: int
    corrupt_buf: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    corrupt_pos: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))  # within verified region
    corrupt_xor: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint8))
    n_conns: int = 0
    datagram_headers: bool = False       # write the 26-byte MediaStream data header per buffer

    @property
    def n(self) -> int:
        return len(self.descs)

    def verified_bytes(self) -> int:
        d = self.descs
        return int((d["length"].astype(np.int64) - d["skip_head"].astype(np.int64)).sum())

    def corrupt_abs_offsets(self) -> np.ndarray:
        """Arena byte offsets of the injected corruptions."""
        d = self.descs[self.corrupt_buf]
        return (d["byte_offset"].astype(np.int64) + d["skip_head"].astype(np.int64) + self.corrupt_pos)


def fmix32(x: np.ndarray) -> np.ndarray:
    """murmur3 finaliser: the connection hash used for sharding (hash(conn_index) mod G)."""
    x = np.asarray(x, dtype=np.uint32).astype(np.uint64)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def shard_of(conn_index: np.ndarray, world: int) -> np.ndarray:
    return (fmix32(conn_index) % np.uint32(world)).astype(np.int64)


def _corruption_plan(lengths: np.ndarray, rate: int, seed: int, rng_count: Optional[int] = None):
    """Choose n // rate distinct buffers (none when rate <= 0), one corrupted byte each."""
    n = len(lengths)
    rng = np.random.default_rng(seed)
    if rate <= 0 or n == 0:
        k = 0
    else:
        k = (n // rate) if rng_count is None else rng_count
    eligible = np.nonzero(lengths > 0)[0]
    k = min(k, len(eligible))
    bufs = np.sort(rng.choice(eligible, size=k, replace=False)) if k else np.zeros(0, np.int64)
    pos = (rng.random(k) * lengths[bufs]).astype(np.int64) if k else np.zeros(0, np.int64)
    xor = rng.integers(1, 256, size=k, dtype=np.uint8) if k else np.zeros(0, np.uint8)
    return bufs.astype(np.int64), pos, xor


def tcp_resident(n_buffers: int = 4096, length: int = 65536, corrupt_rate: int = 1024,
                 random_phase_frac: float = 0.25, seed_offsets: int = SEED_OFFSETS,
                 seed_corrupt: int = SEED_CORRUPT, name: str = "config2", conn_base: int = 0) -> Workload:
    """Config 2: n x 64 KiB device-resident buffers, mixed phases, sparse corruption."""
    rng = np.random.default_rng(seed_offsets)
    d = np.zeros(n_buffers, dtype=DESC_DTYPE)
    d["byte_offset"] = np.arange(n_buffers, dtype=np.uint64) * np.uint64(length)
    d["length"] = length
    rand = rng.random(n_buffers) < random_phase_frac
    offs = rng.integers(0, PATTERN_PERIOD, size=n_buffers)
    d["expected_pattern_offset"] = np.where(rand, offs, 0).astype(np.uint32)
    d["conn_index"] = np.arange(n_buffers, dtype=np.uint32) + np.uint32(conn_base)  # rank-disjoint connections
    d["skip_head"] = 0
    lens = d["length"].astype(np.int64)
    cb, cp, cx = _corruption_plan(lens, corrupt_rate, seed_corrupt)
    return Workload(name, d, n_buffers * length, length, cb, cp, cx, n_conns=n_buffers)


def udp_datagrams(n_datagrams: int = 16 * 1024 * 1024, datagram: int = 1472, corrupt_rate: int = 1024,
                  seed_corrupt: int = SEED_CORRUPT, name: str = "config3") -> Workload:
    """Config 3: n x 1472-byte MediaStream datagrams (26-byte header + P[0..1445])."""
    d = np.zeros(n_datagrams, dtype=DESC_DTYPE)
    d["byte_offset"] = np.arange(n_datagrams, dtype=np.uint64) * np.uint64(datagram)
    d["length"] = datagram
    d["expected_pattern_offset"] = 0
    d["conn_index"] = 0
    d["skip_head"] = UDP_DATA_HEADER_LENGTH
    payload = np.full(n_datagrams, datagram - UDP_DATA_HEADER_LENGTH, dtype=np.int64)
    cb, cp, cx = _corruption_plan(payload, corrupt_rate, seed_corrupt)
    return Workload(name, d, n_datagrams * datagram, datagram, cb, cp, cx, n_conns=1, datagram_headers=True)


def connection_streams(n_conns: int = 1024, buffers_per_conn: int = 1024, length: int = 65536,
                       ragged: bool = False, corrupt_rate: int = 1024, seed: int = SEED_OFFSETS,
                       seed_corrupt: int = SEED_CORRUPT, world: int = 1, rank: int = 0,
                       align: int = 16, name: str = "config4") -> Workload:
    """Configs 4/5: per-connection streams, offsets = exclusive prefix sums mod 65536.

    ``ragged`` draws each completion length uniformly in [1, length] (the
    ``-buffer:[lo,hi]`` / partial-completion case); otherwise every completion
    is a full ``length``. Only the connections with hash(conn) mod world == rank
    are materialised; their buffers are packed contiguously in the rank's arena
    (``align``-byte aligned; align=1 packs them tightly so buffer starts take
    every alignment), connection-major in stream order, so
    ``conn_first_fail`` (min failing buffer index per connection) gives the
    first failing buffer in stream order.
    """
    rng = np.random.default_rng(seed)
    conns = np.arange(n_conns, dtype=np.uint32)
    mine = conns[shard_of(conns, world) == rank] if world > 1 else conns
    if ragged:
        all_lens = rng.integers(1, length + 1, size=(n_conns, buffers_per_conn)).astype(np.int64)
    else:
        all_lens = np.full((n_conns, buffers_per_conn), length, dtype=np.int64)
    lens = all_lens[mine]                              # [mine, bpc]
    excl = np.cumsum(lens, axis=1) - lens              # exclusive prefix sum per connection
    offs = (excl % PATTERN_PERIOD).astype(np.uint32)
    n = lens.size
    d = np.zeros(n, dtype=DESC_DTYPE)
    flat_lens = lens.reshape(-1)
    slot = (flat_lens + align - 1) // align * align
    starts = np.cumsum(slot) - slot
    d["byte_offset"] = starts.astype(np.uint64)
    d["length"] = flat_lens.astype(np.uint32)
    d["expected_pattern_offset"] = offs.reshape(-1)
    d["conn_index"] = np.repeat(mine, buffers_per_conn)
    d["skip_head"] = 0
    arena = int(slot.sum()) if n else 16
    cb, cp, cx = _corruption_plan(flat_lens, corrupt_rate, seed_corrupt + rank)
    return Workload(name, d, arena, int(flat_lens.max()) if n else 0, cb, cp, cx, n_conns=n_conns)


def expected_results(w: Workload):
    """Analytic reference outcome of a workload whose only defects are its corruption plan.

    Returns (fail_first[n] int64 (-1 = pass), fail_count[n] int64, counters dict,
    conn_first_fail uint32[n_conns]).
    """
    n = w.n
    first = np.full(n, -1, dtype=np.int64)
    count = np.zeros(n, dtype=np.int64)
    if len(w.corrupt_buf):
        order = np.lexsort((w.corrupt_pos, w.corrupt_buf))
        b, p = w.corrupt_buf[order], w.corrupt_pos[order]
        uniq, idx, cnt = np.unique(b, return_index=True, return_counts=True)
        first[uniq] = p[idx]
        # distinct positions per buffer
        pairs = np.unique(np.stack([b, p], axis=1), axis=0)
        ub, ucnt = np.unique(pairs[:, 0], return_counts=True)
        count[ub] = ucnt
    vlen = w.descs["length"].astype(np.int64) - w.descs["skip_head"].astype(np.int64)
    failed = first >= 0
    counters = {
        "bytes_checked": int(vlen.sum()),
        "bytes_ok": int(vlen[~failed].sum()),
        "buffers_checked": int(n),
        "buffers_failed": int(failed.sum()),
        "mismatched_bytes": int(count.sum()),
    }
    cff = np.full(w.n_conns, 0xFFFFFFFF, dtype=np.uint32)
    if failed.any() and w.n_conns:
        fi = np.nonzero(failed)[0]
        conns = w.descs["conn_index"][fi].astype(np.int64)
        keep = conns < w.n_conns
        np.minimum.at(cff, conns[keep], fi[keep].astype(np.uint32))
    return first, count, counters, cff


REF_FIELDS = ("bytes_recv", "bytes_ok", "buffers_recv", "buffers_failed", "bytes_after_failure",
              "buffers_after_failure")
EMPTY_SLOT = 0xFFFFFFFF


def descs_bad(descs: np.ndarray, arena_bytes: int) -> np.ndarray:
    """The verify's bad-descriptor rule (CTS_RESULT_FLAG_BAD_DESC) as a mask: expected offset >= 65536, length below
    skip_head, or a buffer that leaves the arena."""
    off = descs["byte_offset"].astype(np.uint64)
    length = descs["length"].astype(np.uint64)
    inside = off <= np.uint64(arena_bytes)
    room = np.where(inside, np.uint64(arena_bytes) - np.where(inside, off, np.uint64(0)), np.uint64(0))
    return ((descs["expected_pattern_offset"] >= PATTERN_PERIOD) | (descs["length"] < descs["skip_head"]) |
            ~inside | (room < length))


def reference_view(descs: np.ndarray, failed_mask, ordinals, n_conns: int, *, bad=None, slots=None):
    """The counters as ctsTraffic itself would hold them: a failed VerifyBuffer fails the connection on that
    completion (ctsIOPattern.cpp:486-489 -> FailedIo), so each connection stops at its first failing ordinal.

    descs: DESC_DTYPE, one per buffer; failed_mask[i]: buffer i did not match; ordinals[i]: its stream ordinal
    (increasing along each connection's stream; the base_index + i of the launch that held it). ``bad`` marks
    descriptors the verify refuses (they count nowhere and fail nothing); ``slots`` replaces the first-failure
    slots derived from failed_mask (uint32[n_conns], 0xFFFFFFFF = empty).

    Returns ({REF_FIELDS: int}, slots uint32[n_conns]): with F the slot of a buffer's connection (empty when the
    connection has none, conn_index >= n_conns) and g its ordinal, a buffer is received when g <= F, clean when
    g < F, the failing one when g == F and never received when g > F.
    """
    descs = np.asarray(descs)
    g = np.asarray(ordinals, dtype=np.int64)
    failed = np.asarray(failed_mask, dtype=bool)
    live = np.ones(len(descs), dtype=bool) if bad is None else ~np.asarray(bad, dtype=bool)
    conn = descs["conn_index"].astype(np.int64)
    has_slot = conn < n_conns
    if slots is None:
        slots = np.full(n_conns, EMPTY_SLOT, dtype=np.uint32)
        pick = failed & live & has_slot
        np.minimum.at(slots, conn[pick], g[pick].astype(np.uint32))
    else:
        slots = np.asarray(slots, dtype=np.uint32)
        assert slots.shape == (n_conns,)
    first = np.full(len(descs), EMPTY_SLOT, dtype=np.int64)
    first[has_slot] = slots[conn[has_slot]].astype(np.int64)
    vlen = descs["length"].astype(np.int64) - descs["skip_head"].astype(np.int64)
    recv, ok, at, after = live & (g <= first), live & (g < first), live & (g == first), live & (g > first)
    sums = {
        "bytes_recv": int(vlen[recv].sum()),
        "bytes_ok": int(vlen[ok].sum()),
        "buffers_recv": int(recv.sum()),
        "buffers_failed": int(at.sum()),
        "bytes_after_failure": int(vlen[after].sum()),
        "buffers_after_failure": int(after.sum()),
    }
    return sums, slots


CLOSE_FIELDS = ("connections_closed", "successful", "data_errors", "not_all_data", "too_much_data", "bytes_recv")
STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN = 2147483644  # ctsIOPattern.h:46-50
STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED = 2147483645
STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED = 2147483646


def connection_view(descs: np.ndarray, failed_mask, ordinals, n_conns: int, bad=None, slots=None):
    """reference_view per connection: the table cts_refview_accumulate_conns keeps (include/cts_connections.h).

    Arguments as reference_view. Returns (CONN_STATE_DTYPE[n_conns], slots uint32[n_conns]): entry c holds the bytes
    and buffers of connection c with g <= F (received) and with g > F (after its failure). Buffers of connections
    without a slot (conn_index >= n_conns) are in no entry, bad descriptors nowhere; the column sums equal
    reference_view's bytes_recv, buffers_recv, bytes_after_failure and buffers_after_failure when every connection has
    a slot."""
    from .types import CONN_STATE_DTYPE

    descs = np.asarray(descs)
    g = np.asarray(ordinals, dtype=np.int64)
    _, slots = reference_view(descs, failed_mask, ordinals, n_conns, bad=bad, slots=slots)
    live = np.ones(len(descs), dtype=bool) if bad is None else ~np.asarray(bad, dtype=bool)
    conn = descs["conn_index"].astype(np.int64)
    live &= conn < n_conns
    conn, g = conn[live], g[live]
    vlen = (descs["length"].astype(np.int64) - descs["skip_head"].astype(np.int64))[live]
    recv = g <= slots[conn].astype(np.int64)
    table = np.zeros(n_conns, dtype=CONN_STATE_DTYPE)
    for sel, fb, fn in ((recv, "bytes_recv", "buffers_recv"), (~recv, "bytes_after_failure", "buffers_after_failure")):
        np.add.at(table[fb], conn[sel], vlen[sel].astype(np.uint64))
        table[fn] = np.bincount(conn[sel], minlength=n_conns).astype(np.uint64)
    return table, slots


def close_results(state: np.ndarray, slots: np.ndarray, conn_ids, expected_bytes):
    """cts_conns_close as a model: close the distinct connections conn_ids of a table (connection_view) and its slots
    against expected_bytes (one per id; None = no byte-count check).

    Returns (CONN_RESULT_DTYPE[len(conn_ids)], {CLOSE_FIELDS: int}, state after, slots after). The data error wins
    over the byte-count errors; an id >= len(slots) is flagged, counted nowhere and resets nothing."""
    from .types import CONN_RESULT_DTYPE, CONN_RESULT_FLAG_BAD_CONN

    ids = np.asarray(conn_ids, dtype=np.int64)
    assert len(np.unique(ids)) == len(ids)
    state, slots = np.array(state, copy=True), np.array(slots, dtype=np.uint32, copy=True)
    res = np.zeros(len(ids), dtype=CONN_RESULT_DTYPE)
    res["conn_index"] = ids
    good = ids < len(slots)
    res["flags"][~good] = CONN_RESULT_FLAG_BAD_CONN
    c = ids[good]
    for f in state.dtype.names:
        res[f][good] = state[f][c]
    res["first_fail"][good] = slots[c]
    got = state["bytes_recv"][c]
    status = np.zeros(len(c), dtype=np.uint32)
    if expected_bytes is not None:
        want = np.asarray(expected_bytes, dtype=np.uint64)[good]
        status[got < want] = STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED
        status[got > want] = STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED
    status[slots[c] != EMPTY_SLOT] = STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN
    res["status"][good] = status
    counts = {
        "connections_closed": int(len(c)),
        "successful": int((status == 0).sum()),
        "data_errors": int((status == STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN).sum()),
        "not_all_data": int((status == STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED).sum()),
        "too_much_data": int((status == STATUS_ERROR_TOO_MUCH_DATA_TRANSFERRED).sum()),
        "bytes_recv": int(got.astype(np.uint64).sum()),
    }
    slots[c] = EMPTY_SLOT
    state[c] = 0
    return res, counts, state, slots


def rebase_slots(slots: np.ndarray, delta: int) -> np.ndarray:
    """cts_conn_slots_rebase as a model: non-empty slots drop by delta, clamped at 0; empty slots stay empty."""
    s = np.asarray(slots, dtype=np.uint32).astype(np.int64)
    return np.where(s == EMPTY_SLOT, EMPTY_SLOT, np.maximum(s - int(delta), 0)).astype(np.uint32)


def stream_launches(descs: np.ndarray, buffers_per_conn: int, parts: int):
    """Cut every connection's stream of a connection-major workload (connection_streams) into ``parts`` consecutive
    pieces: launch k holds piece k of every connection, connection-major, and its base_index is the number of buffers
    in the launches before it, so a connection's ordinals (base_index + i) increase along its stream.

    Returns [(descs_k, base_index_k, index_k)]: index_k = the positions of the launch's buffers in ``descs``."""
    n = len(descs)
    assert n % buffers_per_conn == 0
    grid = np.arange(n, dtype=np.int64).reshape(-1, buffers_per_conn)
    cuts = [buffers_per_conn * k // parts for k in range(parts + 1)]
    out, base = [], 0
    for k in range(parts):
        idx = grid[:, cuts[k]:cuts[k + 1]].reshape(-1)
        out.append((np.ascontiguousarray(descs[idx]), base, idx))
        base += len(idx)
    return out


def header_bytes(seq: np.ndarray) -> np.ndarray:
    """26-byte MediaStream data headers: u16 flag 0, i64 seq, i64 qpc 0, i64 qpf 0."""
    seq = np.asarray(seq, dtype="<i8")
    h = np.zeros((len(seq), UDP_DATA_HEADER_LENGTH), dtype=np.uint8)
    h[:, 2:10] = seq.view(np.uint8).reshape(-1, 8)
    return h


def materialize(engine, w: Workload, device: str = "cuda", fill_stream=None):
    """Build a workload on the device: arena (the sender's bytes as received,
    produced by the product fill kernel), MediaStream headers, injected
    corruptions. Returns (arena uint8 tensor, descs uint8 tensor)."""
    import torch

    from .engine import descs_to_device

    arena = torch.zeros(((w.arena_bytes + 15) // 16) * 16 + 16, dtype=torch.uint8, device=device)
    arena = arena[: w.arena_bytes] if w.arena_bytes else arena[:16]
    descs = descs_to_device(w.descs, device)
    engine.fill(arena, descs, max_length_hint=w.max_length, stream=fill_stream)
    if w.datagram_headers and w.n:
        dg = int(w.descs["length"][0])
        assert np.all(w.descs["byte_offset"] == np.arange(w.n, dtype=np.uint64) * np.uint64(dg))
        a2 = arena[: w.n * dg].view(w.n, dg)
        seq = torch.arange(1, w.n + 1, dtype=torch.int64, device=device)
        a2[:, 0:2] = 0
        a2[:, 2:10] = seq.view(torch.uint8).view(w.n, 8)
        a2[:, 10:UDP_DATA_HEADER_LENGTH] = 0
    if len(w.corrupt_buf):
        pos = torch.from_numpy(w.corrupt_abs_offsets()).to(device)
        xor = torch.from_numpy(w.corrupt_xor).to(device)
        arena[pos] = arena[pos] ^ xor
    return arena, descs
