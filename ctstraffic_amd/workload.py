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


# ---- MediaStream connections on the device-resident path (include/cts_media_stream_conns.h) -------------------
UDP_FIELDS = ("bits_received", "successful_frames", "dropped_frames", "duplicate_frames", "error_frames", "datagrams")
STATUS_IO_RUNNING = 2147483647  # c_statusIoRunning, ctsIOPattern.h:46
DGRAM_DATA, DGRAM_ID, DGRAM_ZERO, DGRAM_SHORT, DGRAM_UNKNOWN, DGRAM_BAD_DESC = range(6)


def media_stream_conn_entries(settings):
    """cts_ms_conn_init as a model, for a list of (frame_size_bytes, buffered_frames, stream_length_frames): fresh
    entries with their rings laid out one after the other. Returns (MS_CONN_STATE_DTYPE[len(settings)], frame_elems).
    Raises ValueError where cts_ms_conn_init returns CTS_E_INVALID."""
    from .types import MS_CONN_STATE_DTYPE

    e = np.zeros(len(settings), dtype=MS_CONN_STATE_DTYPE)
    base = 0
    for c, (frame_size, buffered, length) in enumerate(settings):
        if frame_size <= 0 or length <= 0 or length > 0xFFFFFFFF:
            raise ValueError("connection %d: frame size %d, stream length %d" % (c, frame_size, length))
        initial = min(length, buffered)
        if 2 * initial < 2 or 2 * initial > 0xFFFFFFFF:
            raise ValueError("connection %d: a queue of %d frames" % (c, 2 * initial))
        e[c]["head_sequence_number"] = 1
        e[c]["final_frame"] = length
        e[c]["frame_base"] = base
        e[c]["frames"] = 2 * initial
        e[c]["frame_size_bytes"] = frame_size
        e[c]["initial_buffer_frames"] = initial
        e[c]["timer_wheel_offset"] = initial
        e[c]["last_error"] = STATUS_IO_RUNNING
        base += 2 * initial
    return e, base


def datagram_exceptions(kind, passed) -> np.ndarray:
    """The datagrams that fail their stream: anything but an ID datagram and a DATA datagram whose payload verified."""
    kind = np.asarray(kind)
    return np.where(kind == DGRAM_DATA, ~np.asarray(passed, dtype=bool), kind != DGRAM_ID)


class MediaStreamConnectionView:
    """The device-resident MediaStream connections as a model: what cts_media_stream_verify_status_at does to the
    slots, and cts_media_stream_conns_accumulate, _render and _close to the entries, the rings, the UDP block and
    the close block. One jitter window per connection; a datagram's stream ordinal is base_index + its index."""

    def __init__(self, entries: np.ndarray, frame_elems: int, slots=None):
        from .types import MS_CONN_STATE_DTYPE

        self.entries = np.array(entries, dtype=MS_CONN_STATE_DTYPE, copy=True)
        self.n_conns = len(self.entries)
        self.ring = np.zeros(frame_elems, dtype=np.uint64)
        self.slots = (np.full(self.n_conns, EMPTY_SLOT, dtype=np.uint32) if slots is None
                      else np.array(slots, dtype=np.uint32, copy=True))
        self.udp = dict.fromkeys(UDP_FIELDS, 0)
        self.close_block = dict.fromkeys(CLOSE_FIELDS, 0)

    def receive(self, conn_index, kind, passed, base_index: int = 0) -> None:
        """The receive pass's slot claims: the lowest exception ordinal per connection with a slot."""
        conn = np.asarray(conn_index, dtype=np.int64)
        pick = datagram_exceptions(kind, passed) & (conn < self.n_conns)
        g = (base_index + np.arange(len(conn), dtype=np.int64)).astype(np.uint32)
        np.minimum.at(self.slots, conn[pick], g[pick])

    def accumulate(self, conn_index, status, base_index: int = 0) -> None:
        """The accounting pass over one batch: conn_index[i] and status[i] (DGRAM_STATUS_DTYPE) of datagram i. Every
        datagram is judged against its entry as the last tick left it and against the final slot."""
        e, conn = self.entries, np.asarray(conn_index, dtype=np.int64)
        for i in range(len(conn)):
            c, g = int(conn[i]), base_index + i
            kind, completed = int(status["kind"][i]), int(status["completed_bytes"][i])
            clean = kind == DGRAM_DATA and bool(status["pass"][i])
            if c >= self.n_conns:
                self.udp["datagrams"] += 1
                if clean:
                    self.udp["bits_received"] += 8 * completed
                continue
            first = int(self.slots[c])
            if e["finished"][c] != 0 or g > first:
                e["datagrams_after_end"][c] += 1
                continue
            e["datagrams"][c] += 1
            self.udp["datagrams"] += 1
            if g == first:
                e["last_error"][c] = (STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN if kind == DGRAM_DATA
                                      else STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED)
                e["has_failure"][c] = 1
            elif clean:
                e["bits_received"][c] += 8 * completed
                self.udp["bits_received"] += 8 * completed
                seq, head, frames = int(status["sequence_number"][i]), int(e["head_sequence_number"][c]), int(e["frames"][c])
                at = int(e["frame_base"][c]) + (seq - 1) % frames if frames else len(self.ring)
                if seq > int(e["final_frame"][c]) or seq < head or seq > head + frames - 1 or at >= len(self.ring):
                    e["error_frames"][c] += 1
                    self.udp["error_frames"] += 1
                else:
                    self.ring[at] += completed
                    e["received_any"][c] = 1

    def render(self, conn_ids) -> np.ndarray:
        """One render tick of the listed connections. Returns the codes: 0 keep, 1 finished, 2 fatal; a connection
        that is not rendered reports its entry's finished, an id without an entry 0."""
        e, codes = self.entries, np.zeros(len(conn_ids), dtype=np.uint32)
        for i, c in enumerate(int(x) for x in conn_ids):
            if c >= self.n_conns:
                continue
            if e["last_error"][c] != STATUS_IO_RUNNING or e["frames"][c] == 0:
                codes[i] = e["finished"][c]
                continue
            e["timer_wheel_offset"][c] += 1
            head, final = int(e["head_sequence_number"][c]), int(e["final_frame"][c])
            if e["timer_wheel_offset"][c] >= e["initial_buffer_frames"][c] and head <= final:
                if e["received_any"][c] == 0 and head == 1:
                    e["dropped_frames"][c] += final
                    self.udp["dropped_frames"] += final
                    e["finished"][c] = 2
                    e["last_error"][c] = STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED
                    codes[i] = 2
                    continue
                at = int(e["frame_base"][c]) + (head - 1) % int(e["frames"][c])
                got, want = int(self.ring[at]), int(e["frame_size_bytes"][c])
                f = "successful_frames" if got == want else "dropped_frames" if got < want else "duplicate_frames"
                e[f][c] += 1
                self.udp[f] += 1
                self.ring[at] = 0
                head += 1
                e["head_sequence_number"][c] = head
            if head > final:
                e["finished"][c] = 1
                e["last_error"][c] = 0
                codes[i] = 1
        return codes

    def close(self, conn_ids) -> np.ndarray:
        """Close the distinct connections conn_ids. Returns MS_CONN_RESULT_DTYPE[len(conn_ids)]."""
        from .types import (MS_CONN_CLOSED, MS_CONN_RESULT_DTYPE, MS_CONN_RESULT_FLAG_BAD_CONN,
                            MS_CONN_RESULT_FLAG_HAS_FAILURE, MS_CONN_RESULT_FLAG_RUNNING)

        e, res = self.entries, np.zeros(len(conn_ids), dtype=MS_CONN_RESULT_DTYPE)
        assert len(set(int(x) for x in conn_ids)) == len(conn_ids)
        for i, c in enumerate(int(x) for x in conn_ids):
            r = res[i]
            r["conn_index"], r["fail_datagram"] = c, EMPTY_SLOT
            if c >= self.n_conns:
                r["flags"] = MS_CONN_RESULT_FLAG_BAD_CONN
                continue
            status, flags = int(e["last_error"][c]), 0
            if status == STATUS_IO_RUNNING:
                status, flags = STATUS_ERROR_NOT_ALL_DATA_TRANSFERRED, MS_CONN_RESULT_FLAG_RUNNING
            for f in ("bits_received", "successful_frames", "dropped_frames", "duplicate_frames", "error_frames",
                      "datagrams", "datagrams_after_end", "head_sequence_number", "finished"):
                r[f] = e[f][c]
            if e["has_failure"][c]:
                flags |= MS_CONN_RESULT_FLAG_HAS_FAILURE
                r["fail_datagram"] = (int(e["datagrams"][c]) - 1) & 0xFFFFFFFF  # a 32-bit field: the low word
            r["first_fail"], r["status"], r["flags"] = self.slots[c], status, flags
            cls = ("successful" if status == 0 else
                   "data_errors" if status == STATUS_ERROR_DATA_DID_NOT_MATCH_BIT_PATTERN else "not_all_data")
            self.close_block["connections_closed"] += 1
            self.close_block[cls] += 1
            self.close_block["bytes_recv"] += int(e["bits_received"][c]) // 8
            self.slots[c] = EMPTY_SLOT
            b = int(e["frame_base"][c])
            self.ring[b:b + int(e["frames"][c])] = 0
            e["last_error"][c] = status
            if e["finished"][c] == 0:
                e["finished"][c] = MS_CONN_CLOSED
        return res

    def rebase(self, delta: int) -> None:
        self.slots = rebase_slots(self.slots, delta)

    def reinit(self, conn_ids, fresh: np.ndarray) -> None:
        """Fresh entries written over the listed ones (the caller's copy to the device)."""
        for c in conn_ids:
            self.entries[int(c)] = fresh[int(c)]


def media_stream_connection_view(entries: np.ndarray, frame_elems: int, slots=None) -> MediaStreamConnectionView:
    """A model of the device-resident MediaStream connections over `entries` (media_stream_conn_entries) and a ring
    array of frame_elems elements; see MediaStreamConnectionView."""
    return MediaStreamConnectionView(entries, frame_elems, slots)


_PATTERN_PREFIX = None


def _pattern_prefix(n: int) -> np.ndarray:
    """P[0 .. n): the bytes a MediaStream payload carries (every datagram starts at pattern offset 0)."""
    global _PATTERN_PREFIX
    if _PATTERN_PREFIX is None or len(_PATTERN_PREFIX) < n:
        from ._lib import lib

        L = lib()
        _PATTERN_PREFIX = np.array([L.cts_pattern_byte(i) for i in range(max(n, 2048))], dtype=np.uint8)
    return _PATTERN_PREFIX[:n]


@dataclass
class MsConnBatch:
    descs: np.ndarray   # DESC_DTYPE, conn_index = the connection
    arena: np.ndarray   # uint8: the datagrams as received
    base_index: int     # stream ordinal of datagram 0
    ticks: int          # render ticks after the batch


@dataclass
class MsConnPlan:
    settings: list      # (frame_size_bytes, buffered_frames, stream_length_frames) per connection
    roles: list         # what each connection's traffic is made to do
    batches: list       # MsConnBatch
    max_datagram: int

    @property
    def n_conns(self) -> int:
        return len(self.settings)


MS_CONN_ROLES = ("mismatch_first", "success", "duplicate", "dropped", "stale_future", "id_success", "short_unknown",
                 "unknown", "zero", "fatal", "window600", "bad_desc", "ends_early")


def _ms_role_settings(role: str, c: int):
    frame = (4000, 3044, 1500, 5000, 2944)[c % 5]
    if role in ("success", "id_success"):
        return frame, 1, 3       # a window of 2 frames, rendered to its end by three ticks
    if role == "ends_early":
        return frame, 1, 2       # ended by the second tick: the third batch arrives after the end
    if role in ("window600", "bulk"):
        return frame, 300, 1000  # a window of 600 frames
    return frame, 4, 100         # a window of 8 frames


def _ms_role_datagrams(role: str, k: int, head: int, cfg, lens, last_batch: bool, bulk_frames: int):
    """Batch k of one connection: [(kind, seq, length, corrupt)], in completion order. head: its window's head."""
    _, buffered, final = cfg
    whole = lambda s: [("data", s, int(ln), False) for ln in lens]
    if role == "fatal":
        return [] if k == 0 else whole(head)
    if role in ("window600", "bulk"):
        out = []
        for s in range(head, head + bulk_frames):
            out += whole(s)
        return out
    d = whole(min(head, final + 1) if role in ("success", "id_success") else head)
    if role == "mismatch_first" and k == 0:
        d[0] = ("data", head, d[0][2], True)   # the batch's first datagram, and a second exception behind it
        d.append(("data", head + 1, int(lens[0]), True))
    elif role == "duplicate":
        d.append(d[-1])
    elif role == "dropped":
        d = d[:-1] if len(d) > 1 else []
    elif role == "stale_future" and k >= 1:
        d += [("data", head - 1, int(lens[0]), False), ("data", head + 2 * buffered + 12, int(lens[0]), False),
              ("data", final + 1, int(lens[-1]), False)]
    elif role == "id_success" and k == 0:
        d.insert(0, ("id", 0, 39, False))
    elif role == "short_unknown" and k == 1:
        d.insert(1, ("short", 0, 10, False))
        d.append(("unknown", 0, 100, False))
    elif role == "unknown" and k == 2:
        d.insert(len(d) // 2, ("unknown", 0, 64, False))
    elif role == "unknown_last" and last_batch:
        d.append(("unknown", 0, 40, False))
    elif role == "zero" and k == 1:
        d.insert(0, ("zero", 0, 0, False))
    elif role == "bad_desc" and k == 0:
        d.append(("bad", 0, 100, False))
    elif role == "ends_early" and k == 2:
        d.append(("zero", 0, 0, False))     # after the end: lowers the slot, changes nothing
    return d


def media_stream_connections(n_conns: int = 37, batches: int = 3, ticks=None, order: str = "conn_major",
                             roles=None, bulk_frames: int = 2, limit: Optional[int] = None, max_datagram: int = 1472,
                             mutate_rate: int = 0, seed: int = SEED_CORRUPT, align: int = 1) -> MsConnPlan:
    """A plan of MediaStream traffic for n_conns device-resident connections: per connection its client settings and a
    role (MS_CONN_ROLES in turn, the last connection "unknown_last": an exception in the last batch's last datagram;
    or `roles`), and `batches` batches of datagrams, each followed by ticks[k] render ticks (default 1).

    order: "conn_major" (each connection's datagrams together), "interleaved" (round-robin over the connections, so
    neighbours differ while more than one connection has datagrams left). A connection's own datagrams keep their
    order. limit: keep only the first `limit` datagrams of every batch. mutate_rate > 0: about one datagram in
    mutate_rate of the "bulk" role is made corrupt, short, an ID datagram or stale (seeded).
    Every batch has an arena of its own with the datagrams packed `align`-byte aligned; a bad descriptor points past it.
    """
    from .media_stream import split

    rng = np.random.default_rng(seed)
    ticks = [1] * batches if ticks is None else list(ticks)
    if roles is None:
        roles = [MS_CONN_ROLES[c % len(MS_CONN_ROLES)] for c in range(n_conns)]
        if n_conns > len(MS_CONN_ROLES):
            roles[-1] = "unknown_last"
    settings = [_ms_role_settings(r, c) for c, r in enumerate(roles)]
    lens = [split(s[0], max_datagram) for s in settings]
    pattern = _pattern_prefix(max_datagram)
    out, base, rendered = [], 0, 0
    for k in range(batches):
        per_conn = []
        for c, role in enumerate(roles):
            head = min(1 + rendered, settings[c][2] + 1)
            d = _ms_role_datagrams(role, k, head, settings[c], lens[c], k == batches - 1, bulk_frames)
            if role == "bulk" and mutate_rate > 0:
                for j in range(len(d)):
                    if rng.integers(mutate_rate) == 0:
                        how = int(rng.integers(4))
                        d[j] = (("data", d[j][1], d[j][2], True), ("short", 0, 7, False), ("id", 0, 60, False),
                                ("data", 0, d[j][2], False))[how]
            per_conn.append([(c,) + x for x in d])
        if order == "conn_major":
            flat = [x for d in per_conn for x in d]
        elif order == "interleaved":
            flat, depth = [], max((len(d) for d in per_conn), default=0)
            for j in range(depth):
                flat += [d[j] for d in per_conn if j < len(d)]
        else:
            raise ValueError("order %r" % order)
        if limit is not None:
            flat = flat[:limit]
        n = len(flat)
        descs = np.zeros(n, dtype=DESC_DTYPE)
        length = np.array([x[3] for x in flat], dtype=np.int64)
        slot = (length + align - 1) // align * align
        start = np.cumsum(slot) - slot if n else np.zeros(0, np.int64)
        arena = np.zeros(int(slot.sum()) + 16, dtype=np.uint8)
        for i, (c, kind, seq, ln, corrupt) in enumerate(flat):
            o = int(start[i])
            if kind == "data":
                arena[o + 2:o + 10] = np.array([seq], dtype="<i8").view(np.uint8)
                arena[o + 26:o + ln] = pattern[:ln - 26]
                if corrupt:
                    arena[o + 26 + int(rng.integers(ln - 26))] ^= np.uint8(rng.integers(1, 256))
            elif kind == "id":
                arena[o:o + 2] = (0x00, 0x10)   # c_udpDatagramProtocolHeaderFlagId, little-endian
                arena[o + 2:o + ln] = 0x41
            elif kind == "unknown":
                arena[o:o + ln] = 0x22
            elif kind == "bad":
                start[i] = len(arena) + 1000
            # "short": ln < 26 zero bytes under flag 0; "zero": no bytes
        descs["byte_offset"] = start.astype(np.uint64)
        descs["length"] = length.astype(np.uint32)
        descs["conn_index"] = np.array([x[0] for x in flat], dtype=np.uint32)
        descs["skip_head"] = UDP_DATA_HEADER_LENGTH
        out.append(MsConnBatch(descs, arena, base, ticks[k]))
        base += n
        rendered += ticks[k]
    return MsConnPlan(settings, list(roles), out, max_datagram)


# ---- MediaStream servers on the device-resident path (include/cts_media_stream_servers.h) ---------------------
MS_SERVER_TICK_FIELDS = ("bytes", "datagrams", "connections_sent", "connections_finished", "connections_no_room",
                         "connections_skipped")


def media_stream_server_entries(settings):
    """cts_ms_server_init as a model, for a list of (frame_size_bytes, datagram_max_size, stream_length_frames).
    Returns MS_SERVER_STATE_DTYPE[len(settings)]; raises ValueError where cts_ms_server_init returns CTS_E_INVALID."""
    from .types import MS_SERVER_MIN_DATAGRAM, MS_SERVER_STATE_DTYPE

    e = np.zeros(len(settings), dtype=MS_SERVER_STATE_DTYPE)
    for c, (frame_size, datagram_max, length) in enumerate(settings):
        if frame_size <= UDP_DATA_HEADER_LENGTH or length <= 0 or length > 0xFFFFFFFF:
            raise ValueError("connection %d: frame size %d, stream length %d" % (c, frame_size, length))
        if datagram_max < MS_SERVER_MIN_DATAGRAM:
            raise ValueError("connection %d: datagrams of at most %d bytes" % (c, datagram_max))
        e[c]["current_frame"] = 1
        e[c]["final_frame"] = length
        e[c]["frame_size_bytes"] = frame_size
        e[c]["datagram_max_size"] = datagram_max
        e[c]["datagrams_per_frame"] = -(-frame_size // datagram_max)
    return e


def media_stream_frame_lengths(frame_size: int, datagram_max: int) -> list:
    """cts_media_stream_split's lengths in closed form, as the device computes them: with k = ceil(F / M) and r =
    F mod M a remainder of 1..26 bytes makes the last datagram 27 bytes and the one before it M - (27 - r)."""
    F, M = int(frame_size), int(datagram_max)
    k, r = -(-F // M), F % M
    lens = [M] * k
    tiny = 0 < r <= UDP_DATA_HEADER_LENGTH
    if k >= 2 and tiny:
        lens[k - 2] = M - (UDP_DATA_HEADER_LENGTH + 1 - r)
    lens[k - 1] = M if r == 0 else (UDP_DATA_HEADER_LENGTH + 1 if tiny and k > 1 else r)
    return lens


def media_stream_datagram(length: int, seq: int, qpc: int, qpf: int) -> np.ndarray:
    """One data datagram's bytes: the packed 26-byte header {u16 0, i64 seq, i64 qpc, i64 qpf} and P[0 .. length - 26)."""
    import struct

    d = np.empty(length, dtype=np.uint8)
    d[:UDP_DATA_HEADER_LENGTH] = np.frombuffer(struct.pack("<Hqqq", 0, seq, qpc, qpf), dtype=np.uint8)
    d[UDP_DATA_HEADER_LENGTH:] = _pattern_prefix(length - UDP_DATA_HEADER_LENGTH)
    return d


class MediaStreamServerView:
    """The device-resident MediaStream servers as a model, one connection at a time in Python integers: what
    cts_media_stream_servers_send does to the entries, the codes, the tick block, the UDP block, the ring, the
    descriptors and the lengths. ring is the caller's array of bytes (what the device ring held before the tick);
    slots the tick does not write keep their bytes, descriptors and lengths beyond the tick's datagrams theirs."""

    def __init__(self, entries: np.ndarray, stride: int, ring: np.ndarray, capacity: int):
        from .types import MS_SERVER_STATE_DTYPE

        self.entries = np.array(entries, dtype=MS_SERVER_STATE_DTYPE, copy=True)
        self.n_conns, self.stride, self.capacity = len(self.entries), stride, capacity
        self.ring = np.array(ring, dtype=np.uint8, copy=True)
        self.descs = np.zeros(capacity, dtype=DESC_DTYPE)
        self.lengths = np.zeros(capacity, dtype=np.uint32)
        self.udp = dict.fromkeys(UDP_FIELDS, 0)
        self.codes = np.zeros(0, dtype=np.uint32)
        self.tick = dict.fromkeys(MS_SERVER_TICK_FIELDS, 0)

    def send(self, conn_ids, qpc: int, qpf: int, first_slot: int = 0, capacity: int = None):
        """One tick of the distinct connections conn_ids. Returns (codes, tick)."""
        from .media_stream import split

        capacity = self.capacity if capacity is None else capacity
        e, tick = self.entries, dict.fromkeys(MS_SERVER_TICK_FIELDS, 0)
        codes, p = np.zeros(len(conn_ids), dtype=np.uint32), 0
        for i, c in enumerate(int(x) for x in conn_ids):
            if c >= self.n_conns or int(e["finished"][c]) != 0 or int(e["datagram_max_size"][c]) > self.stride:
                codes[i] = 2 if c < self.n_conns and int(e["finished"][c]) != 0 else 4
                tick["connections_skipped"] += 1
                continue
            F, M, k = (int(e[f][c]) for f in ("frame_size_bytes", "datagram_max_size", "datagrams_per_frame"))
            first, p = p, p + k
            if first + k > capacity:
                codes[i] = 3
                tick["connections_no_room"] += 1
                continue
            lens = [int(x) for x in split(F, M)]
            assert len(lens) == k and sum(lens) == F  # a frame's bytes include its datagrams' headers
            seq = int(e["current_frame"][c])
            # the leading run of equal lengths as one block of rows, the rest one datagram at a time
            run = next((j for j, x in enumerate(lens) if x != lens[0]), k)
            s0 = first_slot + first
            if len(self.ring) % self.stride == 0:
                self.ring.reshape(-1, self.stride)[s0:s0 + run, :lens[0]] = media_stream_datagram(lens[0], seq, qpc, qpf)
            else:
                run = 0
            for j in range(run, k):
                o = (s0 + j) * self.stride
                self.ring[o:o + lens[j]] = media_stream_datagram(lens[j], seq, qpc, qpf)
            d = self.descs[first:first + k]
            d["byte_offset"] = (s0 + np.arange(k, dtype=np.uint64)) * np.uint64(self.stride)
            d["length"], d["expected_pattern_offset"], d["conn_index"], d["skip_head"] = lens, 0, c, UDP_DATA_HEADER_LENGTH
            self.lengths[first:first + k] = lens
            e["bits_sent"][c] = int(e["bits_sent"][c]) + 8 * F
            e["datagrams_sent"][c] = int(e["datagrams_sent"][c]) + k
            e["current_frame"][c] = seq + 1
            if seq + 1 > int(e["final_frame"][c]):
                e["finished"][c] = 1
                tick["connections_finished"] += 1
                codes[i] = 1
            tick["bytes"] += F
            tick["datagrams"] += k
            tick["connections_sent"] += 1
            self.udp["bits_received"] += 8 * F
            self.udp["datagrams"] += k
        self.codes, self.tick = codes, tick
        return codes, tick

    def send_at(self, conn_ids, schedule: np.ndarray, now_ms: int, max_frames: int, qpc: int, qpf: int,
                first_slot: int = 0, capacity: int = None):
        """One timed tick (cts_media_stream_servers_send_at) of the distinct connections conn_ids at now_ms over
        `schedule` (media_stream_server_schedule). The frames that are out are found as the reference finds them, one
        frame after the other by its own expression and its "< 2" rule (media_stream_frames_out), not by the device's
        closed form. Returns (codes, tick), the tick with MS_SERVER_TIMED_TICK_FIELDS."""
        from .media_stream import split

        capacity = self.capacity if capacity is None else capacity
        e, tick = self.entries, dict.fromkeys(MS_SERVER_TIMED_TICK_FIELDS, 0)
        tick["next_due_ms"] = INT64_MAX
        codes, p = np.zeros(len(conn_ids), dtype=np.uint32), 0
        for i, c in enumerate(int(x) for x in conn_ids):
            if c >= self.n_conns or int(e["finished"][c]) != 0 or int(e["datagram_max_size"][c]) > self.stride:
                codes[i] = 2 if c < self.n_conns and int(e["finished"][c]) != 0 else 4
                tick["connections_skipped"] += 1
                continue
            F, M, k = (int(e[f][c]) for f in ("frame_size_bytes", "datagram_max_size", "datagrams_per_frame"))
            base, fps = int(schedule["base_time_ms"][c]), int(schedule["frames_per_second"][c])
            seq, final = int(e["current_frame"][c]), int(e["final_frame"][c])
            wf = media_stream_frames_out(base, fps, seq, final, now_ms, max_frames)
            t = 0
            if wf == 0:
                codes[i] = 5
                tick["connections_waiting"] += 1
            else:
                first, p = p, p + min(wf * k, 0xFFFFFFFF)
                t = min(wf, (capacity - min(first, capacity)) // k)
                if t == 0:
                    codes[i] = 3
                    tick["connections_no_room"] += 1
            if t:
                lens = [int(x) for x in split(F, M)]
                assert len(lens) == k and sum(lens) == F
                for f in range(t):
                    s0 = first_slot + first + f * k
                    for j in range(k):
                        o = (s0 + j) * self.stride
                        self.ring[o:o + lens[j]] = media_stream_datagram(lens[j], seq + f, qpc, qpf)
                d = self.descs[first:first + t * k]
                d["byte_offset"] = (first_slot + first + np.arange(t * k, dtype=np.uint64)) * np.uint64(self.stride)
                d["length"], d["expected_pattern_offset"], d["conn_index"] = lens * t, 0, c
                d["skip_head"] = UDP_DATA_HEADER_LENGTH
                self.lengths[first:first + t * k] = lens * t
                e["bits_sent"][c] = int(e["bits_sent"][c]) + 8 * t * F
                e["datagrams_sent"][c] = int(e["datagrams_sent"][c]) + t * k
                e["current_frame"][c] = seq + t
                if seq + t > final:
                    e["finished"][c] = 1
                    tick["connections_finished"] += 1
                    codes[i] = 1
                tick["bytes"] += t * F
                tick["datagrams"] += t * k
                tick["frames"] += t
                tick["connections_sent"] += 1
                self.udp["bits_received"] += 8 * t * F
                self.udp["datagrams"] += t * k
            if codes[i] != 1:  # left running: when its next frame is due
                tick["next_due_ms"] = min(tick["next_due_ms"], media_stream_frame_due(base, fps, seq + t))
        self.codes, self.tick = codes, tick
        return codes, tick


INT64_MAX = (1 << 63) - 1
MS_SERVER_TIMED_TICK_FIELDS = MS_SERVER_TICK_FIELDS + ("next_due_ms", "connections_waiting", "frames")


def media_stream_server_schedule(settings):
    """cts_ms_server_schedule_init as a model, for a list of (frames_per_second, base_time_ms). Returns
    MS_SERVER_SCHEDULE_DTYPE[len(settings)]; raises ValueError where cts_ms_server_schedule_init returns
    CTS_E_INVALID."""
    from .types import MS_SERVER_SCHEDULE_DTYPE

    q = np.zeros(len(settings), dtype=MS_SERVER_SCHEDULE_DTYPE)
    for c, (fps, base) in enumerate(settings):
        if fps == 0 or fps > 0xFFFFFFFF or not 0 <= base < (1 << 62):
            raise ValueError("connection %d: %d frames per second from %d ms" % (c, fps, base))
        q[c]["base_time_ms"], q[c]["frames_per_second"] = base, fps
    return q


def media_stream_frame_due(base_time_ms: int, frames_per_second: int, frame: int) -> int:
    """When the reference sends frame `frame`: m_baseTimeMilliseconds + m_currentFrame * 1000LL / m_frameRateFps
    (ctsIOPattern.cpp:1136-1150)."""
    return base_time_ms + frame * 1000 // frames_per_second


def media_stream_frames_out(base_time_ms: int, frames_per_second: int, current_frame: int, final_frame: int,
                            now_ms: int, max_frames: int) -> int:
    """How many frames from current_frame on the reference's server sends at now_ms without arming its timer, at most
    max_frames: it sends the next frame at once while that frame's time offset is below 2
    (ctsMediaStreamServerConnectedSocket.cpp:62-74). One frame after the other, as the reference goes."""
    f = current_frame
    while (f <= final_frame and f - current_frame < max_frames
           and media_stream_frame_due(base_time_ms, frames_per_second, f) - now_ms < 2):
        f += 1
    return f - current_frame


def media_stream_server_view(entries: np.ndarray, stride: int, ring: np.ndarray,
                             capacity: int) -> MediaStreamServerView:
    """A model of the device-resident MediaStream servers over `entries` (media_stream_server_entries) and a ring of
    stride-byte slots; see MediaStreamServerView."""
    return MediaStreamServerView(entries, stride, ring, capacity)


# ---- TCP senders on the device-resident path (include/cts_tcp_senders.h) ----------------------------------------
TCP_SENDER_TICK_FIELDS = ("bytes", "buffers", "connections_sent", "connections_finished", "connections_no_room",
                          "connections_skipped")
SENT_FIELDS = ("bytes_sent", "buffers_sent", "connections_finished", "reserved0", "reserved1", "reserved2")


def tcp_sender_entries(settings):
    """cts_tcp_sender_init as a model, for a list of (transfer_bytes, buffer_size). Returns
    TCP_SENDER_DTYPE[len(settings)]; raises ValueError where cts_tcp_sender_init returns CTS_E_INVALID."""
    from .types import TCP_SENDER_DTYPE

    e = np.zeros(len(settings), dtype=TCP_SENDER_DTYPE)
    for c, (transfer, buffer_size) in enumerate(settings):
        if transfer <= 0 or buffer_size <= 0 or transfer >= 1 << 64 or buffer_size >= 1 << 32:
            raise ValueError("connection %d: transfer %d, buffer size %d" % (c, transfer, buffer_size))
        e[c]["transfer_bytes"] = transfer
        e[c]["buffer_size"] = buffer_size
    return e


@dataclass
class TcpSenderTickView:
    """What one cts_tcp_senders_send leaves behind (tcp_sender_view)."""
    arena: np.ndarray     # the arena's bytes after the tick
    descs: np.ndarray     # DESC_DTYPE[capacity]: [0, total) the tick's, the rest as before
    codes: np.ndarray     # uint32 per listed id
    tick: dict            # TCP_SENDER_TICK_FIELDS
    counters: dict        # SENT_FIELDS: the sent block after the tick
    entries: np.ndarray   # TCP_SENDER_DTYPE after the tick
    prefix: np.ndarray    # uint64 per listed id: its first tick-local slot
    taken: np.ndarray     # uint64 per listed id: the slots it took


def tcp_sender_view(entries: np.ndarray, stride: int, arena: np.ndarray, first_slot: int, capacity: int, ids,
                    max_buffers: int, descs: np.ndarray = None, counters: dict = None) -> TcpSenderTickView:
    """One tick of cts_tcp_senders_send as a model, in numpy closed forms over the listed connections and over the
    tick's buffers (the only Python loop runs over the distinct buffer lengths). arena, descs (what dev_descs held
    before, default zeros) and counters (the sent block before, default zeros) are not modified; the results are
    copies."""
    return _tcp_sender_tick(entries, stride, arena, first_slot, capacity, ids, max_buffers, descs, counters, None)


def _tcp_sender_tick(entries, stride, arena, first_slot, capacity, ids, max_buffers, descs, counters, cut):
    """tcp_sender_view's tick. cut (None for the plain tick): cut(i, c, limit, R, B) -> the slots that listed
    connection i (slot c, running, wanting `limit`) wants after pacing; a running connection cut to 0 gets code 5."""
    from .types import TCP_SENDER_DTYPE

    e = np.array(entries, dtype=TCP_SENDER_DTYPE, copy=True)
    ids = np.array([int(x) for x in ids], dtype=np.uint64)
    n, n_conns = len(ids), len(e)
    table = e if n_conns else np.zeros(1, dtype=TCP_SENDER_DTYPE)
    valid = ids < np.uint64(n_conns)
    c = np.where(valid, ids, np.uint64(0)).astype(np.int64)
    B = table["buffer_size"][c].astype(np.uint64)
    sent, transfer = table["bytes_sent"][c].astype(np.uint64), table["transfer_bytes"][c].astype(np.uint64)
    skipped = ~valid | (B == 0) | (B > np.uint64(stride))
    ended = ~skipped & ((table["finished"][c] != 0) | (sent >= transfer))
    running = ~skipped & ~ended
    Bd = np.where(B == 0, np.uint64(1), B)
    R = np.where(running, transfer - np.where(running, sent, np.uint64(0)), np.uint64(0))
    k = R // Bd + (R % Bd != 0).astype(np.uint64)
    w = np.where(running, np.minimum(k, np.uint64(max_buffers)), np.uint64(0))
    waiting = np.zeros(n, dtype=bool)
    if cut is not None:
        for i in np.nonzero(running)[0]:
            w[i] = cut(int(i), int(c[i]), int(w[i]), int(R[i]), int(B[i]))
        waiting = running & (w == 0)
    p = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(w, dtype=np.uint64)])[:n]
    cap = np.uint64(capacity)
    t = np.minimum(w, cap - np.minimum(p, cap))
    moved = np.minimum(t * B, R)
    finished = running & (t > 0) & (moved == R)
    codes = np.zeros(n, dtype=np.uint32)
    codes[skipped], codes[ended], codes[running & (t == 0)], codes[finished] = 4, 2, 3, 1
    codes[waiting] = 5
    took = running & (t > 0)
    total = int(t.sum())
    tick = {"bytes": int(moved[took].sum()), "buffers": total, "connections_sent": int(took.sum()),
            "connections_finished": int(finished.sum()), "connections_no_room": int((running & (t == 0) & ~waiting).sum()),
            "connections_skipped": int((skipped | ended).sum())}
    # the buffers: listed connection `owner` of tick-local slot g, its buffer j
    owner = np.repeat(np.arange(n, dtype=np.int64), t.astype(np.int64))
    g = np.arange(total, dtype=np.uint64)
    j = g - p[owner]
    start = sent[owner] + j * B[owner]
    length = np.minimum(B[owner], transfer[owner] - start)
    offset = start & np.uint64(PATTERN_PERIOD - 1)
    out_descs = np.zeros(capacity, dtype=DESC_DTYPE) if descs is None else np.array(descs, dtype=DESC_DTYPE, copy=True)
    d = out_descs[:total]
    d["byte_offset"] = (np.uint64(first_slot) + g) * np.uint64(stride)
    d["length"], d["expected_pattern_offset"], d["conn_index"], d["skip_head"] = length, offset, ids[owner], 0
    out = np.array(arena, dtype=np.uint8, copy=True)
    rows = out[: len(out) // stride * stride].reshape(-1, stride)
    P = _pattern_prefix(PATTERN_PERIOD)
    for L in np.unique(length):
        L = int(L)
        mine = np.nonzero(length == np.uint64(L))[0]
        tiled = np.tile(P, (PATTERN_PERIOD + L - 1) // PATTERN_PERIOD + 1)[: PATTERN_PERIOD + L - 1]
        windows = np.lib.stride_tricks.sliding_window_view(tiled, L)
        rows[first_slot + mine, :L] = windows[offset[mine].astype(np.int64)]
    e["bytes_sent"][c[took]] = sent[took] + moved[took]
    e["buffers_sent"][c[took]] = e["buffers_sent"][c[took]] + t[took]
    e["finished"][c[finished]] = 1
    after = dict.fromkeys(SENT_FIELDS, 0) if counters is None else dict(counters)
    after["bytes_sent"] += tick["bytes"]
    after["buffers_sent"] += total
    after["connections_finished"] += tick["connections_finished"]
    return TcpSenderTickView(out, out_descs, codes, tick, after, e, p, t)


# ---- send pacing on the device-resident path (cts_tcp_senders_send_paced) -----------------------------------------
TCP_SENDER_PACED_TAIL_FIELDS = ("next_due_ms", "connections_waiting", "connections_pending")
TCP_SENDER_NO_DUE = (1 << 63) - 1


def tcp_sender_pace_entries(settings, start_ms: int = 0):
    """cts_tcp_sender_pace_init as a model, for a list of dicts with the keys bytes_per_second, period_ms,
    burst_count, burst_delay_ms (each optional, default 0; {} = unpaced). Returns
    TCP_SENDER_PACE_DTYPE[len(settings)]; raises ValueError where cts_tcp_sender_pace_init returns CTS_E_INVALID."""
    from .types import TCP_SENDER_PACE_DTYPE

    q = np.zeros(len(settings), dtype=TCP_SENDER_PACE_DTYPE)
    for c, s in enumerate(settings):
        unknown = set(s) - {"bytes_per_second", "period_ms", "burst_count", "burst_delay_ms"}
        if unknown:
            raise ValueError("connection %d: unknown pace settings %s" % (c, sorted(unknown)))
        bps, period = s.get("bytes_per_second", 0), s.get("period_ms", 0) or 100
        if start_ms < 0 or start_ms >= 1 << 63 or bps < 0 or bps * period >= 1 << 63:
            raise ValueError("connection %d: rate %d, period %d, start %d" % (c, bps, period, start_ms))
        q[c]["bytes_per_quantum"] = bps * period // 1000
        q[c]["quantum_start_ms"] = start_ms
        q[c]["quantum_period_ms"] = period
        q[c]["burst_count"] = q[c]["burst_left"] = s.get("burst_count", 0)
        q[c]["burst_delay_ms"] = s.get("burst_delay_ms", 0)
    return q


def _pace_step(q: dict, now: int, size: int) -> int:
    """CreateNewTask's send branch (ctsIOPattern.cpp:593-674) over a pace entry held as a dict of Python ints: the
    task's time offset."""
    off = 0
    per, period = q["bytes_per_quantum"], q["quantum_period_ms"]
    if per > 0:
        if q["bytes_this_quantum"] < per:
            q["bytes_this_quantum"] += size
            if now > q["quantum_start_ms"] + period:
                skipped = (now - q["quantum_start_ms"]) // period
                q["quantum_start_ms"] += skipped * period
                adjust = per * skipped
                q["bytes_this_quantum"] = 0 if adjust > q["bytes_this_quantum"] else q["bytes_this_quantum"] - adjust
        else:
            ahead = q["bytes_this_quantum"] // per
            skip = (ahead - 1) * period
            q["bytes_this_quantum"] += size - per * ahead
            if now < q["quantum_start_ms"] + period:
                off = q["quantum_start_ms"] + period - now
            off += skip
            q["quantum_start_ms"] += skip + period
    elif q["burst_count"]:
        if q["burst_left"] == 0:
            q["burst_left"] = q["burst_count"]
        q["burst_left"] -= 1
        if q["burst_left"] == 0:
            off = q["burst_delay_ms"]
    return off


def _pace_run(q: dict, now: int, cap: int, R: int, B: int) -> int:
    """run(cap) of include/cts_tcp_senders.h over q (moved in place): the sends that go out at `now`."""
    if q["bytes_per_quantum"] == 0 and q["burst_count"] == 0 and not q["pending"]:
        return min(cap, -(-R // B))  # unpaced: no step moves the entry or defers a send (a cap of 2^31 is no loop)
    count = 0
    while count < cap and R - count * B > 0:
        if q["pending"]:
            if now < q["due_ms"]:
                break
            q["pending"] = 0
        else:
            off = _pace_step(q, now, min(B, R - count * B))
            if off > 0:
                q["pending"], q["due_ms"] = 1, now + off
                break
        count += 1
    return count


_PACE_SCALARS = ("bytes_per_quantum", "bytes_this_quantum", "quantum_start_ms", "due_ms", "quantum_period_ms",
                 "burst_count", "burst_left", "burst_delay_ms", "pending")


@dataclass
class TcpPacedSenderTickView(TcpSenderTickView):
    """What one cts_tcp_senders_send_paced leaves behind (tcp_paced_sender_view): a TcpSenderTickView (codes with 5 =
    waiting), and"""
    pace: np.ndarray = None     # TCP_SENDER_PACE_DTYPE after the tick
    waiting: np.ndarray = None  # the listed positions with code 5
    tail: dict = None           # TCP_SENDER_PACED_TAIL_FIELDS
    wanted: np.ndarray = None   # uint64 per listed id: w, the slots pacing lets it want


def tcp_paced_sender_view(entries: np.ndarray, pace: np.ndarray, now_ms: int, stride: int, arena: np.ndarray,
                          first_slot: int, capacity: int, ids, max_buffers: int, descs: np.ndarray = None,
                          counters: dict = None) -> TcpPacedSenderTickView:
    """One tick of cts_tcp_senders_send_paced as a model: tcp_sender_view with every running listed connection's
    wanted slots cut by run(limit) over its pace entry (a plain Python loop per connection), the pace entries moved
    as the header states (run(limit), or run(t) for the one connection the capacity cuts; untouched with code 3),
    and the tick's tail. Nothing passed in is modified."""
    from .types import TCP_SENDER_PACE_DTYPE

    q_out = np.array(pace, dtype=TCP_SENDER_PACE_DTYPE, copy=True)
    if len(q_out) != len(entries):
        raise ValueError("%d pace entries beside %d sender entries" % (len(q_out), len(entries)))
    moved, asked = {}, {}

    def stored(c):
        return {f: int(q_out[c][f]) for f in _PACE_SCALARS}

    def cut(i, c, limit, R, B):
        q = stored(c)
        w = _pace_run(q, now_ms, limit, R, B)
        moved[i], asked[i] = q, (c, R, B, w)
        return w

    v = _tcp_sender_tick(entries, stride, arena, first_slot, capacity, ids, max_buffers, descs, counters, cut)
    wanted = np.zeros(len(v.codes), dtype=np.uint64)
    due = []
    for i, (c, R, B, w) in asked.items():  # q_out[c] is still the entry from before the tick: the ids are distinct
        t, code = int(v.taken[i]), int(v.codes[i])
        wanted[i] = w
        if code == 3:       # no room: the stored entry stays
            q = stored(c)
        elif 0 < t < w:     # cut by the capacity: t steps, and no task beyond the t-th
            q = stored(c)
            if _pace_run(q, now_ms, t, R, B) != t:
                raise AssertionError("run(t) stopped before t")
        else:               # code 5 (w == 0), or everything it wanted
            q = moved[i]
        for f in ("bytes_this_quantum", "quantum_start_ms", "due_ms", "burst_left", "pending"):
            q_out[c][f] = q[f]
        if q["pending"]:
            due.append(q["due_ms"])
    tail = {"next_due_ms": min(due) if due else TCP_SENDER_NO_DUE, "connections_waiting": int((v.codes == 5).sum()),
            "connections_pending": len(due)}
    return TcpPacedSenderTickView(v.arena, v.descs, v.codes, v.tick, v.counters, v.entries, v.prefix, v.taken,
                                  q_out, np.nonzero(v.codes == 5)[0], tail, wanted)


# ---- Push, Pull, PushPull and Duplex on the device-resident path (include/cts_tcp_exchange.h) ----------------------
TCP_EXCHANGE_TICK_FIELDS = TCP_SENDER_TICK_FIELDS + ("bytes_dir",)


def tcp_exchange_sequence(pattern: int, transfer: int, B: int, P: int = 0, Q: int = 0):
    """A connection's buffers one step at a time, as the reference's patterns hand them out: a restatement of
    GetNextTaskFromPattern / CompleteTaskBackToPattern (ctsIOPattern.cpp:808-1099) with every task completed in full
    before the next is asked for, and for Duplex the two directions taking turns, direction 0 first. Yields (direction,
    stream position, length, m_intraSegmentTransfer before the buffer). Kept apart from the closed form
    (tcp_exchange_element): this one walks, that one jumps."""
    from .types import TCP_EXCHANGE_DUPLEX, TCP_EXCHANGE_PULL, TCP_EXCHANGE_PUSH, TCP_EXCHANGE_PUSHPULL

    sent = [0, 0]
    if pattern in (TCP_EXCHANGE_PUSH, TCP_EXCHANGE_PULL):
        d, remaining = (0 if pattern == TCP_EXCHANGE_PUSH else 1), transfer
        while remaining:
            n = min(B, remaining)  # CreateNewTask: min(remaining transfer, buffer size)
            yield d, sent[d], n, 0
            sent[d] += n
            remaining -= n
    elif pattern == TCP_EXCHANGE_PUSHPULL:
        sending, intra, remaining = True, 0, transfer  # the client's m_sending: clients start sending
        while remaining:
            segment = P if sending else Q
            assert intra < segment
            n = min(B, remaining, segment - intra)  # CreateTrackedTask(action, segmentSize - m_intraSegmentTransfer)
            d = 0 if sending else 1
            yield d, sent[d], n, intra
            sent[d] += n
            remaining -= n
            intra += n
            if intra == segment:
                sending, intra = not sending, 0
    elif pattern == TCP_EXCHANGE_DUPLEX:
        transfer += transfer % 2  # max transfer bytes must be even
        left = [transfer // 2, transfer // 2]  # m_remainingSendBytes of the two sides
        d = 0
        while left[0] or left[1]:
            if left[d]:
                n = min(B, left[d])
                yield d, sent[d], n, 0
                sent[d] += n
                left[d] -= n
            d ^= 1
    else:
        raise ValueError("pattern %d" % pattern)


def tcp_exchange_total_buffers(pattern: int, transfer: int, B: int, P: int = 0, Q: int = 0) -> int:
    """N of include/cts_tcp_exchange.h, in Python integers."""
    if pattern in (0, 1):
        return -(-transfer // B)
    if pattern == 3:
        return 2 * -(-((transfer + transfer % 2) // 2) // B)
    kp, kq, C = -(-P // B), -(-Q // B), P + Q
    rem = transfer % C
    return transfer // C * (kp + kq) + (-(-rem // B) if rem <= P else kp + -(-(rem - P) // B))


def tcp_exchange_element(pattern: int, transfer: int, B: int, P: int, Q: int, m: int):
    """Element m of the sequence by the closed form of include/cts_tcp_exchange.h, in Python integers: (direction,
    stream position, length, m_intraSegmentTransfer)."""
    if pattern in (0, 1):
        return pattern, m * B, min(B, transfer - m * B), 0
    if pattern == 3:
        H = (transfer + transfer % 2) // 2
        return m & 1, (m >> 1) * B, min(B, H - (m >> 1) * B), 0
    kp, kq, C = -(-P // B), -(-Q // B), P + Q
    y, r = divmod(m, kp + kq)
    if r < kp:
        s = r * B
        return 0, y * P + s, min(B, P - s, transfer - (y * C + s)), s
    s = (r - kp) * B
    return 1, y * Q + s, min(B, Q - s, transfer - (y * C + P + s)), s


def tcp_exchange_position(pattern: int, transfer: int, B: int, P: int, Q: int, m: int):
    """[bytes of direction 0, of direction 1] that the first m <= N buffers carry, by closed form."""
    if m >= tcp_exchange_total_buffers(pattern, transfer, B, P, Q):
        if pattern in (0, 1):
            return [transfer * (1 - pattern), transfer * pattern]
        if pattern == 3:
            return [(transfer + transfer % 2) // 2] * 2
        full, rem = divmod(transfer, P + Q)
        return [full * P + min(rem, P), full * Q + max(rem - P, 0)]
    d, pos, _, _ = tcp_exchange_element(pattern, transfer, B, P, Q, m)
    # buffer m is the next of direction d at pos; the other direction stands where its next buffer starts
    if pattern in (0, 1):
        other = 0
    elif pattern == 3:
        other = min((m + 1) // 2 * B, (transfer + transfer % 2) // 2) if d == 1 else pos
    else:
        y = m // (-(-P // B) + -(-Q // B))
        other = y * P + P if d == 1 else y * Q
    return [pos, other] if d == 0 else [other, pos]


def tcp_exchange_entries(settings, seek=None):
    """cts_tcp_exchange_init (and, with seek = a position per connection, cts_tcp_exchange_seek) as a model, for a list
    of (pattern, transfer_bytes, buffer_size[, push_bytes, pull_bytes]). Returns TCP_EXCHANGE_DTYPE[len(settings)];
    raises ValueError where the C functions return CTS_E_INVALID."""
    from .types import TCP_EXCHANGE_DTYPE

    e = np.zeros(len(settings), dtype=TCP_EXCHANGE_DTYPE)
    for c, s in enumerate(settings):
        pattern, transfer, B = s[:3]
        P, Q = (tuple(s[3:5]) + (0, 0))[:2]
        bad = (transfer <= 0 or B <= 0 or transfer >= 1 << 64 or B >= 1 << 32 or pattern not in (0, 1, 2, 3)
               or not 0 <= P < 1 << 32 or not 0 <= Q < 1 << 32 or (pattern == 2 and (P == 0 or Q == 0))
               or (pattern == 3 and transfer == (1 << 64) - 1))
        if bad:
            raise ValueError("connection %d: pattern %d, transfer %d, buffer size %d, segments %d and %d"
                             % (c, pattern, transfer, B, P, Q))
        if pattern == 3:
            transfer += transfer % 2
        N = tcp_exchange_total_buffers(pattern, transfer, B, P, Q)
        m = 0 if seek is None else int(seek[c])
        if not 0 <= m <= N:
            raise ValueError("connection %d: position %d of %d" % (c, m, N))
        e[c] = (transfer, N, m, tcp_exchange_position(pattern, transfer, B, P, Q, m), B, pattern, P, Q, int(m == N), 0)
    return e


def _exchange_elements(e, m):
    """tcp_exchange_element over arrays: e = TCP_EXCHANGE_DTYPE records (one per buffer), m = their indices (uint64).
    Returns (direction, stream position, length) as uint64 arrays."""
    u = np.uint64
    T, B = e["transfer_bytes"].astype(u), e["buffer_size"].astype(u)
    P, Q, pattern = e["push_bytes"].astype(u), e["pull_bytes"].astype(u), e["pattern"]
    one = u(1)
    sub = lambda a, b: np.where(a > b, a - b, u(0))  # noqa: E731
    # Push, Pull
    d = np.where(pattern == 1, one, u(0))
    pos = m * B
    length = np.minimum(B, sub(T, pos))
    # Duplex
    dup = pattern == 3
    H = T // u(2) + (T & one)
    pos_d = (m >> one) * B
    d = np.where(dup, m & one, d)
    pos = np.where(dup, pos_d, pos)
    length = np.where(dup, np.minimum(B, sub(H, pos_d)), length)
    # PushPull
    pp = pattern == 2
    Bs = np.where(B == 0, one, B)
    kp, kq = (P + Bs - one) // Bs, (Q + Bs - one) // Bs
    K = np.where(kp + kq == 0, one, kp + kq)
    y = m // K
    r = m - y * K
    push = r < kp
    s = np.where(push, r, r - np.minimum(kp, r)) * B
    seg = np.where(push, P, Q)
    G = y * (P + Q) + np.where(push, u(0), P) + s
    d = np.where(pp, np.where(push, u(0), one), d)
    pos = np.where(pp, y * seg + s, pos)
    length = np.where(pp, np.minimum(np.minimum(B, sub(seg, s)), sub(T, G)), length)
    return d, pos, length


@dataclass
class TcpExchangeTickView:
    """What one cts_tcp_exchange_send leaves behind (tcp_exchange_view)."""
    arena: np.ndarray     # the arena's bytes after the tick
    descs: np.ndarray     # DESC_DTYPE[capacity]: [0, total) the tick's, the rest as before
    codes: np.ndarray     # uint32 per listed id
    tick: dict            # TCP_EXCHANGE_TICK_FIELDS (bytes_dir a list of two)
    counters: dict        # SENT_FIELDS: the sent block after the tick
    entries: np.ndarray   # TCP_EXCHANGE_DTYPE after the tick
    prefix: np.ndarray    # uint64 per listed id: its first tick-local slot
    taken: np.ndarray     # uint64 per listed id: the slots it took
    direction: np.ndarray  # uint64 per written buffer


def tcp_exchange_view(entries: np.ndarray, stride: int, arena: np.ndarray, first_slot: int, capacity: int, ids,
                      max_buffers: int, descs: np.ndarray = None, counters: dict = None) -> TcpExchangeTickView:
    """One tick of cts_tcp_exchange_send as a model, in numpy closed forms over the listed connections and over the
    tick's buffers (the only Python loop runs over the distinct buffer lengths). arena, descs (what dev_descs held
    before, default zeros) and counters (the sent block before, default zeros) are not modified; the results are
    copies."""
    return _tcp_exchange_tick(entries, stride, arena, first_slot, capacity, ids, max_buffers, descs, counters, None)


def _tcp_exchange_tick(entries, stride, arena, first_slot, capacity, ids, max_buffers, descs, counters, cut):
    """tcp_exchange_view's tick. cut (None for the plain tick): cut(i, c, limit, entry) -> the slots that listed
    connection i (slot c, running, wanting `limit`, entry = its record) wants after pacing; a running connection cut
    to 0 gets code 5."""
    from .types import TCP_EXCHANGE_DTYPE

    u = np.uint64
    e = np.array(entries, dtype=TCP_EXCHANGE_DTYPE, copy=True)
    ids = np.array([int(x) for x in ids], dtype=u)
    n, n_conns = len(ids), len(e)
    table = e if n_conns else np.zeros(1, dtype=TCP_EXCHANGE_DTYPE)
    valid = ids < u(n_conns)
    c = np.where(valid, ids, u(0)).astype(np.int64)
    E = table[c]
    B, N, m0 = E["buffer_size"].astype(u), E["total_buffers"].astype(u), E["buffers_sent"].astype(u)
    malformed = (B == 0) | (E["pattern"] > 3) | ((E["pattern"] == 2) & ((E["push_bytes"] == 0) | (E["pull_bytes"] == 0)))
    skipped = ~valid | malformed | (B > u(stride))
    ended = ~skipped & ((E["finished"] != 0) | (m0 >= N))
    running = ~skipped & ~ended
    w = np.where(running, np.minimum(N - np.minimum(m0, N), u(max_buffers)), u(0))
    waiting = np.zeros(n, dtype=bool)
    if cut is not None:
        for i in np.nonzero(running)[0]:
            w[i] = cut(int(i), int(c[i]), int(w[i]), E[i])
        waiting = running & (w == 0)
    p = np.concatenate([np.zeros(1, dtype=u), np.cumsum(w, dtype=u)])[:n]
    cap = u(capacity)
    t = np.minimum(w, cap - np.minimum(p, cap))
    took = running & (t > 0)
    finished = took & (m0 + t == N)
    codes = np.zeros(n, dtype=np.uint32)
    codes[skipped], codes[ended], codes[running & (t == 0)], codes[finished] = 4, 2, 3, 1
    codes[waiting] = 5
    total = int(t.sum())
    # the buffers: listed connection `owner` of tick-local slot g, its buffer j, element m of its sequence
    owner = np.repeat(np.arange(n, dtype=np.int64), t.astype(np.int64))
    g = np.arange(total, dtype=u)
    m = m0[owner] + (g - p[owner])
    d, pos, length = _exchange_elements(E[owner], m)
    offset = pos & u(PATTERN_PERIOD - 1)
    by_dir = [int(length[d == u(k)].sum()) for k in (0, 1)]
    tick = {"bytes": sum(by_dir), "buffers": total, "connections_sent": int(took.sum()),
            "connections_finished": int(finished.sum()),
            "connections_no_room": int((running & (t == 0) & ~waiting).sum()),
            "connections_skipped": int((skipped | ended).sum()), "bytes_dir": by_dir}
    out_descs = np.zeros(capacity, dtype=DESC_DTYPE) if descs is None else np.array(descs, dtype=DESC_DTYPE, copy=True)
    dd = out_descs[:total]
    dd["byte_offset"] = (u(first_slot) + g) * u(stride)
    dd["length"], dd["expected_pattern_offset"], dd["skip_head"] = length, offset, 0
    dd["conn_index"] = ids[owner] + d * u(n_conns)
    out = np.array(arena, dtype=np.uint8, copy=True)
    rows = out[: len(out) // stride * stride].reshape(-1, stride)
    P = _pattern_prefix(PATTERN_PERIOD)
    for L in np.unique(length):
        L = int(L)
        mine = np.nonzero(length == u(L))[0]
        tiled = np.tile(P, (PATTERN_PERIOD + L - 1) // PATTERN_PERIOD + 1)[: PATTERN_PERIOD + L - 1]
        windows = np.lib.stride_tricks.sliding_window_view(tiled, L)
        rows[first_slot + mine, :L] = windows[offset[mine].astype(np.int64)]
    for k in (0, 1):
        np.add.at(e["bytes_sent"][:, k], c[owner][d == u(k)], length[d == u(k)])
    e["buffers_sent"][c[took]] = m0[took] + t[took]
    e["finished"][c[finished]] = 1
    after = dict.fromkeys(SENT_FIELDS, 0) if counters is None else dict(counters)
    after["bytes_sent"] += tick["bytes"]
    after["buffers_sent"] += total
    after["connections_finished"] += tick["connections_finished"]
    return TcpExchangeTickView(out, out_descs, codes, tick, after, e, p, t, d)


# ---- send pacing for every pattern (cts_tcp_exchange_send_paced) ----------------------------------------------------
def tcp_exchange_pace_entries(pace_settings, start_ms: int = 0):
    """The pace table of cts_tcp_exchange_send_paced as a model: pace_settings is, per connection slot, a pair (client,
    server) of tcp_sender_pace_entries' dicts. Returns TCP_SENDER_PACE_DTYPE[2 x n_conns], entry c + d x n_conns for
    the side that sends direction d."""
    n_conns = len(pace_settings)
    return tcp_sender_pace_entries([pace_settings[c][d] for d in (0, 1) for c in range(n_conns)], start_ms)


def _pace_unpaced(q: dict) -> bool:
    return q["bytes_per_quantum"] <= 0 and q["burst_count"] == 0 and not q["pending"]


def _pace_run_x(Q: dict, now: int, cap: int, elements) -> int:
    """run_x(cap) of include/cts_tcp_exchange.h: Q = {direction: pace entry as a dict} (moved in place), elements(k) =
    (direction, length) of the k-th buffer from the connection's position."""
    count = 0
    while count < cap:
        d, size = elements(count)
        q = Q[d]
        if q["pending"]:
            if now < q["due_ms"]:
                break
            q["pending"] = 0
        else:
            off = _pace_step(q, now, size)
            if off > 0:
                q["pending"], q["due_ms"] = 1, now + off
                break
        count += 1
    return count


@dataclass
class TcpPacedExchangeTickView(TcpExchangeTickView):
    """What one cts_tcp_exchange_send_paced leaves behind (tcp_paced_exchange_view): a TcpExchangeTickView (codes with
    5 = waiting), and"""
    pace: np.ndarray = None     # TCP_SENDER_PACE_DTYPE[2 x n_conns] after the tick
    waiting: np.ndarray = None  # the listed positions with code 5
    tail: dict = None           # TCP_SENDER_PACED_TAIL_FIELDS
    wanted: np.ndarray = None   # uint64 per listed id: w, the slots pacing lets it want


def tcp_paced_exchange_view(entries: np.ndarray, pace: np.ndarray, now_ms: int, stride: int, arena: np.ndarray,
                            first_slot: int, capacity: int, ids, max_buffers: int, descs: np.ndarray = None,
                            counters: dict = None) -> TcpPacedExchangeTickView:
    """One tick of cts_tcp_exchange_send_paced as a model: tcp_exchange_view with every running listed connection's
    wanted slots cut by run_x(limit) over its two pace entries (a plain Python loop per paced connection, in Python
    integers), the pace entries moved as the header states (run_x(limit), or run_x(t) from the stored entries for the
    one connection the capacity cuts; untouched with code 3), and the tick's tail. pace has 2 x len(entries) records,
    entry c + d x n_conns for direction d. Nothing passed in is modified."""
    from .types import TCP_SENDER_PACE_DTYPE

    q_out = np.array(pace, dtype=TCP_SENDER_PACE_DTYPE, copy=True)
    n_conns = len(entries)
    if len(q_out) != 2 * n_conns:
        raise ValueError("%d pace entries beside %d exchange entries" % (len(q_out), n_conns))
    moved, asked = {}, {}

    def stored(c, dirs):
        return {d: {f: int(q_out[c + d * n_conns][f]) for f in _PACE_SCALARS} for d in dirs}

    def cut(i, c, limit, E):
        pattern, T, B = int(E["pattern"]), int(E["transfer_bytes"]), int(E["buffer_size"])
        P, Q_, m = int(E["push_bytes"]), int(E["pull_bytes"]), int(E["buffers_sent"])
        dirs = {0: (0,), 1: (1,)}.get(pattern, (0, 1))

        def elements(k):
            d, _, length, _ = tcp_exchange_element(pattern, T, B, P, Q_, m + k)
            return d, length

        Q = stored(c, dirs)
        if all(_pace_unpaced(q) for q in Q.values()):
            w = limit  # unpaced: no step moves an entry or defers a send (a limit of 2^31 is no loop)
        else:
            w = _pace_run_x(Q, now_ms, limit, elements)
        moved[i], asked[i] = Q, (c, dirs, elements, w)
        return w

    v = _tcp_exchange_tick(entries, stride, arena, first_slot, capacity, ids, max_buffers, descs, counters, cut)
    wanted = np.zeros(len(v.codes), dtype=np.uint64)
    due = []
    for i, (c, dirs, elements, w) in asked.items():  # q_out still holds c's entries from before: the ids are distinct
        t, code = int(v.taken[i]), int(v.codes[i])
        wanted[i] = w
        if code == 3:       # no room: the stored entries stay
            Q = stored(c, dirs)
        elif 0 < t < w:     # cut by the capacity: t steps, and no task beyond the t-th
            Q = stored(c, dirs)
            if _pace_run_x(Q, now_ms, t, elements) != t:
                raise AssertionError("run_x(t) stopped before t")
        else:               # code 5 (w == 0), or everything it wanted
            Q = moved[i]
        for d, q in Q.items():
            for f in ("bytes_this_quantum", "quantum_start_ms", "due_ms", "burst_left", "pending"):
                q_out[c + d * n_conns][f] = q[f]
        pending = [q["due_ms"] for q in Q.values() if q["pending"]]
        if pending:         # a connection counts once
            due.append(min(pending))
    tail = {"next_due_ms": min(due) if due else TCP_SENDER_NO_DUE, "connections_waiting": int((v.codes == 5).sum()),
            "connections_pending": len(due)}
    return TcpPacedExchangeTickView(v.arena, v.descs, v.codes, v.tick, v.counters, v.entries, v.prefix, v.taken,
                                    v.direction, q_out, np.nonzero(v.codes == 5)[0], tail, wanted)
