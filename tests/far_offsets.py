"""Plans that put rings, descriptors and ticks across the 4 GiB byte offset -- pure numpy, never a 4 GiB host array.

Every kernel of the engine builds a byte address from a small index and a stride. A 32-bit intermediate in one of
these products leaves every small test green, so the plans here place live data just below, across and just above
byte 2^32 (the SEAM) of an arena that is otherwise a sentinel, and keep a model of what a kernel with such a fault
would do:

  a  the slot's (or descriptor's) byte offset is taken mod 2^32;
  b  a tick's ring base first_slot * stride is taken mod 2^32, with 64-bit slot offsets on top of it;
  c  the byte_offset a tick writes into a descriptor is truncated to 32 bits;
  d  the in-arena bound (offset + length > arena_bytes) is compared in 32 bits;
  e  the offset is truncated after the skip (or the 26-byte MediaStream header) was added.

``plan.outcome(None)`` is what a correct kernel leaves: for the verifies the oracle's rows over a compact copy of the
live spans, for the fills and ticks the bytes written, as a SparseRing. ``plan.outcome(defect)`` is the same under one
fault; tests/test_far_offsets_cpu.py shows that every fault changes a field or a byte that
tests/test_far_offsets_gpu.py compares. ``plan.windows()`` lists the byte ranges the GPU tests read back: every live
range with a guard of 128 bytes, its alias mod 2^32, and for ticks the slots a wrapped ring base would hit.

The low aliases hold the opposite of the far content: where a far slot is clean its alias is dirty and the reverse,
so a reader that wraps sees a different outcome in both directions.
"""
from __future__ import annotations

import struct

import numpy as np

import oracle
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import DESC_DTYPE, DGRAM_HEADER_DTYPE, DGRAM_STATUS_DTYPE

SEAM = 1 << 32
BACKGROUND = 0xA5
GUARD = 128
HEADER = 26
EMPTY = 0xFFFFFFFF
QPC, QPF = 0x0102030405060708, -0x1112131415161718

_S = None


def pattern(expected: int, n: int) -> np.ndarray:
    """P[(expected + j) mod 65536] for j < n, from the oracle's sender buffer."""
    global _S
    if _S is None:
        _S = oracle.sender_buffer(65536)[:65536].copy()
    return _S[(int(expected) + np.arange(int(n), dtype=np.int64)) % 65536]


def tcp_bytes(length: int, skip: int, expected: int) -> np.ndarray:
    """A received buffer: `skip` bytes that no verify may read (0x11), then the pattern from `expected` on."""
    out = np.full(length, 0x11, dtype=np.uint8)
    if length > skip:
        out[skip:] = pattern(expected, length - skip)
    return out


def datagram_bytes(length: int, seq: int, qpc: int = QPC, qpf: int = QPF) -> np.ndarray:
    """A MediaStream data datagram: {u16 0, i64 seq, i64 qpc, i64 qpf} and P[0 .. length - 26)."""
    assert length >= HEADER
    out = np.empty(length, dtype=np.uint8)
    out[:HEADER] = np.frombuffer(struct.pack("<Hqqq", 0, seq, qpc, qpf), dtype=np.uint8)
    out[HEADER:] = pattern(0, length - HEADER)
    return out


# ---- the sparse ring ----------------------------------------------------------------------------------------------
class SparseRing:
    """An arena of arena_bytes bytes that is `background` everywhere but in the ranges written; a later write wins."""

    def __init__(self, arena_bytes: int, background: int = BACKGROUND):
        self.arena_bytes, self.background = int(arena_bytes), int(background)
        self._writes = []

    def write(self, off: int, data) -> None:
        data = np.array(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data,
                        dtype=np.uint8, copy=True).reshape(-1)
        if off < 0:
            raise ValueError("a write at %d" % off)
        if len(data):
            self._writes.append((int(off), data))

    def read(self, off: int, n: int) -> np.ndarray:
        off, n = int(off), int(n)
        out = np.full(n, self.background, dtype=np.uint8)
        for o, d in self._writes:
            lo, hi = max(off, o), min(off + n, o + len(d))
            if lo < hi:
                out[lo - off:hi - off] = d[lo - o:hi - o]
        return out

    def flip(self, off: int, mask: int) -> None:
        self.write(off, self.read(off, 1) ^ np.uint8(mask))

    def touched(self) -> list:
        """The written ranges [(a, b)], merged and sorted."""
        return merge_ranges([(o, o + len(d)) for o, d in self._writes])

    def compact(self, descs: np.ndarray, align: int = 16):
        """The live spans of `descs` packed at an `align`-byte-aligned stride: (arena, descriptors rebased onto it).
        A descriptor that leaves this arena points past the compact one as well."""
        return compact_view(self, descs, self.arena_bytes, None, align=align)


def merge_ranges(ranges) -> list:
    out = []
    for a, b in sorted((int(a), int(b)) for a, b in ranges if b > a):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]


def in_ranges(ranges, a: int, b: int) -> bool:
    return any(lo <= a and b <= hi for lo, hi in ranges)


def leaves_arena(off: int, length: int, arena_bytes: int, defect=None, seam: int = SEAM) -> bool:
    """The in-arena part of the bad-descriptor rule; under defect d compared in 32 bits."""
    if defect == "d":
        return (off + length) % seam > arena_bytes % seam
    return off > arena_bytes or arena_bytes - off < length


def read_pieces(off: int, length: int, head: int, defect=None, seam: int = SEAM) -> list:
    """Where a kernel finds (or puts) the `length` bytes of a buffer at `off` whose first `head` bytes are its skip or
    header: [(arena offset, count)] in buffer order."""
    if defect == "a":
        return [(off % seam, length)]
    if defect == "e":
        h = min(head, length)
        return [(off, h), ((off + h) % seam, length - h)]
    return [(off, length)]


def compact_view(ring: SparseRing, descs: np.ndarray, arena_bytes: int, defect=None, seam: int = SEAM, head=None,
                 align: int = 16):
    """What a reader (with `defect`) sees of `descs` over `ring`, as a compact arena and descriptors rebased onto it
    for the oracle. head: the bytes in front of the verified region per descriptor (default its skip_head)."""
    descs = np.asarray(descs, dtype=DESC_DTYPE)
    head = descs["skip_head"] if head is None else np.broadcast_to(head, len(descs))
    out = np.array(descs, copy=True)
    spans, at = [], 0
    bad = np.zeros(len(descs), dtype=bool)
    for i, d in enumerate(descs):
        off, length = int(d["byte_offset"]), int(d["length"])
        bad[i] = leaves_arena(off, length, arena_bytes, defect, seam)
        if bad[i]:
            continue
        data = np.concatenate([ring.read(o, c) for o, c in read_pieces(off, length, int(head[i]), defect, seam)])
        spans.append((at, data))
        out["byte_offset"][i] = at
        at += (length + align - 1) // align * align
    arena = np.full(max(16, at), ring.background, dtype=np.uint8)
    for o, data in spans:
        arena[o:o + len(data)] = data
    out["byte_offset"][bad] = len(arena) + 1
    return arena, out


def status_of(recs: np.ndarray, res: np.ndarray) -> np.ndarray:
    """The compact statuses (cts_datagram_status) of the oracle's records and results."""
    st = np.zeros(len(recs), dtype=DGRAM_STATUS_DTYPE)
    for f in ("sequence_number", "completed_bytes", "flag", "kind"):
        st[f] = recs[f]
    st["pass"] = (recs["kind"] == 0) & (res["pass"] == 1)
    return st


def frame_sums(status: np.ndarray, index, window: dict, dead_status=None, n_dead: int = 0, first_dead: int = 0):
    """What cts_media_stream_verify_frames sums for datagrams `index` with `status` under `window` (head, final,
    frames, finished), plus n_dead datagrams of dead_status from index first_dead on: (totals dict, frame_bytes)."""
    t = dict(bits_received=0, error_frames=0, datagrams=0, first_exception=EMPTY, exceptions=0)
    fb = np.zeros(window["frames"], dtype=np.uint64)

    def one(d, i, count):
        if d["kind"] == W.DGRAM_DATA and d["pass"]:
            seq = int(d["sequence_number"])
            t["bits_received"] += 8 * int(d["completed_bytes"]) * count
            t["datagrams"] += count
            k = seq - window["head"]
            if seq > window["final"] or k < 0 or k >= window["frames"]:
                t["error_frames"] += count
            else:
                fb[k] += np.uint64(int(d["completed_bytes"]) * count)
        elif not (d["kind"] == W.DGRAM_ZERO and window["finished"]):
            t["exceptions"] += count
            t["first_exception"] = min(t["first_exception"], i)

    for d, i in zip(status, index):
        one(d, int(i), 1)
    if n_dead:
        one(dead_status, first_dead, n_dead)
    return t, fb


def _windows_of(ranges, arena_bytes: int, seam: int = SEAM) -> list:
    """[a - 128, b + 128) of every range and of its alias mod seam, clipped to the arena and merged."""
    out = []
    for a, b in ranges:
        out.append((a - GUARD, b + GUARD))
        if b > seam:
            out.append((a % seam - GUARD if a >= seam else -GUARD, (b - 1) % seam + 1 + GUARD))
    return merge_ranges([(max(0, a), min(arena_bytes, b)) for a, b in out])


def ring_differs(x: SparseRing, y: SparseRing, windows) -> bool:
    return any(not np.array_equal(x.read(a, b - a), y.read(a, b - a)) for a, b in windows)


# ---- ring plans: the strided forms --------------------------------------------------------------------------------
VERIFY_STRIDES = (1472, 3072, 64, 1 << 20)
RING_FILL_STRIDES = (1040, 64, 1 << 20)


class RingPlan:
    """A ring of n = seam // stride + 8 slots, nearly all of length 0. Live: slots 0, 1, 2 (the low aliases), one in
    the middle of the ring's last slots below the seam (the witness of a 32-bit bound), the last slot wholly below
    the seam, the slot that holds byte seam - 1 (where the seam is no slot boundary, the slot that holds the seam as
    well), the first three slots wholly above, and the ring's last slot, inside which arena_bytes ends.

    kind "tcp": cts_verify_strided's buffers (skip, expected, one connection); "ms": MediaStream datagrams with
    sequence number slot + 1; "fill": cts_media_stream_fill_strided's lengths and headers, no content."""

    def __init__(self, stride: int, kind: str = "tcp", skip: int = 0, expected: int = 0, seam: int = SEAM,
                 conn: int = 1, n_conns: int = 3, base_index: int = 0):
        s = self.stride = int(stride)
        self.kind, self.skip, self.expected, self.seam = kind, int(skip), int(expected), int(seam)
        self.conn, self.n_conns, self.base_index = conn, n_conns, base_index
        self.head = self.skip if kind == "tcp" else HEADER
        self.n = n = seam // s + 8
        self.below = (seam - 1) // s
        self.above = -(-seam // s)
        self.wholly_below = self.above - 1 if seam % s == 0 else self.above - 2
        self.mid = self.above - 6
        lo = self.head + 1
        lens = {0: s, 1: max(lo, s - 1), 2: max(lo, s // 2), self.mid: max(lo, min(s, 40)), self.wholly_below: s,
                self.below: s, self.above: s, self.above + 1: max(lo, s - 3), self.above + 2: s, n - 1: s}
        assert self.mid > 2 and all(0 <= i < n for i in lens)
        self.live = np.array(sorted(lens), dtype=np.int64)
        self.lens = np.array([lens[int(i)] for i in self.live], dtype=np.uint32)
        self.dead_slot = 3
        assert self.dead_slot not in lens
        self.arena_bytes = (n - 1) * s + s // 2
        self.ring = SparseRing(self.arena_bytes)
        self.flips = []
        if kind != "fill":
            self._write_content()

    def content(self, slot: int, length: int) -> np.ndarray:
        if self.kind == "tcp":
            return tcp_bytes(length, self.skip, self.expected)
        return datagram_bytes(length, slot + 1)

    def headers(self) -> np.ndarray:
        """The live slots' DGRAM_HEADER_DTYPE values (kind "ms" and "fill")."""
        h = np.zeros(len(self.live), dtype=DGRAM_HEADER_DTYPE)
        h["sequence_number"], h["qpc"], h["qpf"] = self.live + 1, QPC, QPF
        return h

    def _write_content(self) -> None:
        s, seam, ring = self.stride, self.seam, self.ring
        for slot, length in zip(self.live, self.lens):
            slot, length = int(slot), int(length)
            ring.write(slot * s, self.content(slot, length)[: max(0, self.arena_bytes - slot * s)])
        # the aliases of the slots wholly above: clean under the dirty one, dirty under the clean ones
        far = [self.above, self.above + 1, self.above + 2]
        lens = dict(zip(self.live.tolist(), self.lens.tolist()))
        for f in far:
            data = self.content(f, lens[f])
            if f != self.above:
                data[min(self.head + 5, lens[f] - 1)] ^= 0x10
            ring.write(f * s - seam, data)
        # one bit in the last byte below the seam and one in the first verified byte at or above it in another slot
        # (the first slot wholly above); where one slot holds both sides of the seam, byte `seam` itself as well
        flips = [(seam - 1, 0x01), (self.above * s + self.head, 0x80)]
        if seam % s != 0:
            flips.append((seam, 0x40))
        for off, mask in flips:
            ring.flip(off, mask)
            self.flips.append(off)

    def descs(self, slots=None, lens=None) -> np.ndarray:
        slots = self.live if slots is None else np.asarray(slots, dtype=np.int64)
        d = np.zeros(len(slots), dtype=DESC_DTYPE)
        d["byte_offset"] = slots.astype(np.uint64) * np.uint64(self.stride)
        d["length"] = self.lens if lens is None else lens
        if self.kind == "tcp":
            d["expected_pattern_offset"], d["conn_index"], d["skip_head"] = self.expected, self.conn, self.skip
        return d

    def seam_slots(self) -> dict:
        """The slots the plan exists for: {"crossing": a live slot that starts below the seam and ends above it, or
        None where the seam is a slot boundary; "at": a live slot that starts exactly at the seam, or None}."""
        s, seam = self.stride, self.seam
        cross = [int(i) for i, ln in zip(self.live, self.lens) if i * s < seam < i * s + int(ln)]
        at = [int(i) for i in self.live if i * s == seam]
        return {"crossing": cross[0] if cross else None, "at": at[0] if at else None}

    def outcome(self, defect=None) -> dict:
        """The verify's or the receive's outputs: the live rows, the row of a dead slot (slot 3 stands for them
        all), the counters over all n slots, and the first-failure slots (kind "tcp"); for kind "fill" the bytes
        written, {"ring": SparseRing}."""
        if self.kind == "fill":
            return {"ring": self._filled(defect)}
        live = self.descs()
        dead = self.descs([self.dead_slot], [0])
        arena, d = compact_view(self.ring, np.concatenate([live, dead]), self.arena_bytes, defect, self.seam,
                                head=self.head)
        n_dead = self.n - len(live)
        if self.kind == "tcp":
            res, _, cff = oracle.verify_batch(arena, d[:-1], n_conns=self.n_conns)
            _, lc, _ = oracle.verify_batch(arena, d[:-1])
            dres, dc, _ = oracle.verify_batch(arena, d[-1:])
            assert dres["pass"][0] == 1 or dres["flags"][0] != 0  # a dead slot claims no first failure
            slots = np.where(cff == EMPTY, EMPTY, self.base_index + self.live[np.minimum(cff, len(live) - 1)])
            return {"live": self.live, "results": res, "dead_result": dres[0],
                    "counters": {f: lc[f] + n_dead * dc[f] for f in lc}, "cff": slots.astype(np.uint32)}
        recs, res, lc = oracle.media_stream_verify(arena, d[:-1])
        drecs, dres, dc = oracle.media_stream_verify(arena, d[-1:])
        return {"live": self.live, "records": recs, "results": res, "status": status_of(recs, res),
                "dead_record": drecs[0], "dead_result": dres[0], "dead_status": status_of(drecs, dres)[0],
                "counters": {f: lc[f] + n_dead * dc[f] for f in lc}}

    def window(self, finished: bool = False) -> dict:
        """A jitter window of 16 frames whose head is the sequence number of the last slot wholly below the seam."""
        return {"head": self.wholly_below + 1, "final": self.n + 100, "frames": 16, "finished": int(finished)}

    def frames(self, out: dict, finished: bool = False):
        first_dead = next(i for i in range(self.n) if i not in set(self.live.tolist()))
        return frame_sums(out["status"], self.live, self.window(finished), out["dead_status"],
                          self.n - len(self.live), first_dead)

    def _filled(self, defect) -> SparseRing:
        out, s = SparseRing(self.arena_bytes), self.stride
        for slot, length in zip(self.live.tolist(), self.lens.tolist()):
            off = slot * s
            if length < HEADER or length > s or leaves_arena(off, length, self.arena_bytes, defect, self.seam):
                continue
            data, at = datagram_bytes(length, slot + 1), 0
            for o, c in read_pieces(off, length, HEADER, defect, self.seam):
                out.write(o, data[at:at + c])
                at += c
        return out

    def windows(self) -> list:
        s = self.stride
        return _windows_of([(int(i) * s, int(i) * s + int(ln)) for i, ln in zip(self.live, self.lens)],
                           self.arena_bytes, self.seam)

    def accounting(self, slots: np.ndarray, defect=None):
        """cts_refview_accumulate_strided and _conns_strided over the whole ring's lengths, the slots preset:
        (reference_view's sums, connection_view's table) over host-built descriptors for all n slots."""
        assert self.kind == "tcp"
        lens = np.zeros(self.n, dtype=np.uint32)
        lens[self.live] = self.lens
        d = self.descs(np.arange(self.n, dtype=np.int64), lens)
        bad = W.descs_bad(d, self.arena_bytes)
        if defect == "d":
            end = (d["byte_offset"] + d["length"].astype(np.uint64)) % np.uint64(self.seam)
            bad = (d["length"] < d["skip_head"]) | (end > np.uint64(self.arena_bytes % self.seam))
        g = self.base_index + np.arange(self.n, dtype=np.int64)
        sums, _ = W.reference_view(d, None, g, self.n_conns, bad=bad, slots=slots)
        table, _ = W.connection_view(d, None, g, self.n_conns, bad=bad, slots=slots)
        return sums, table


# ---- descriptor plans ----------------------------------------------------------------------------------------------
DESC_VARIANTS = ("at", "crossing", "minus1", "plus1", "big")


class DescPlan:
    """About twenty descriptors over the variants, with the lengths of test_buffer_edges (65536, 65531, 8193, 9000,
    1472, 33, 48). Each variant has its own spans at the seam (they would overlap in one arena):

      at        one ends exactly at the seam, the next starts exactly at it;
      crossing  starts below the seam at an odd address and ends above it;
      minus1    starts at seam - 1;
      plus1     one ends at the seam, byte `seam` stays a sentinel, the next starts at seam + 1;
      big       `crossing`, and one descriptor above 16 GiB in an arena of 16 GiB + 64 MiB.

    and the common ones: three low descriptors, one high below the seam (the witness of a 32-bit bound), one of
    length 0 ("tcp"), one that leaves the arena. kind "tcp": skip / expected / connection vary; "ms": datagrams."""

    def __init__(self, variant: str, kind: str = "tcp", seam: int = SEAM, n_conns: int = 5, corrupt: bool = True):
        assert variant in DESC_VARIANTS
        self.variant, self.kind, self.seam, self.n_conns = variant, kind, int(seam), n_conns
        self.arena_bytes = (4 * seam if variant == "big" else seam) + (1 << 26) + 1000
        rows = []  # (offset, length, expected, conn, skip)

        def add(off, length, expected=0, conn=0, skip=0):
            rows.append((off, length, expected if kind == "tcp" else 0, conn, skip if kind == "tcp" else 0))

        add((1 << 20) + 3, 1472, 777, 0, 26)
        add((1 << 21) + 16, 65536, 0, 1, 0)
        add((1 << 22) + 7, 48, 65535, 2, 3)
        add(seam - (1 << 20) - 5, 1472, 12345, 3, 0)
        if kind == "tcp":
            add((1 << 22) + 4096, 0, 5, 4, 0)
        if variant == "at":
            add(seam - 48, 48, 65500, 0, 0)
            add(seam, 65536, 0, 1, 0)
        elif variant in ("crossing", "big"):
            add(seam - 1000 - 7, 65531, 65535, 2, 3)
        elif variant == "minus1":
            add(seam - 1, 9000, 4321, 3, 0)
        elif variant == "plus1":
            add(seam - 1472, 1472, 0, 1, 26)
            add(seam + 1, 8193, 60000, 2, 0)
        add(seam + (1 << 24) + 33, 33 if kind == "tcp" else 48, 31, 4, 0)
        if variant == "big":
            add(4 * seam + 12345, 65531, 100, 0, 0)
        add(self.arena_bytes - 100, 1000, 9, 1, 0)
        rows.sort()
        self.descs = np.array(rows, dtype=DESC_DTYPE)
        self.heads = self.descs["skip_head"].copy() if kind == "tcp" else np.full(len(rows), HEADER, np.uint32)
        self.headers = np.zeros(len(rows), dtype=DGRAM_HEADER_DTYPE)
        self.headers["sequence_number"] = (1 << 40) + np.arange(len(rows))
        self.headers["qpc"], self.headers["qpf"] = QPC, QPF
        self.bad = np.array([leaves_arena(int(d["byte_offset"]), int(d["length"]), self.arena_bytes)
                             for d in self.descs])
        assert self.bad.sum() == 1
        ends = self.descs["byte_offset"] + self.descs["length"].astype(np.uint64)
        assert (self.descs["byte_offset"][1:] >= ends[:-1]).all(), "the spans overlap"
        self.ring = SparseRing(self.arena_bytes)
        self.flips = []
        if corrupt is not None:
            self._write_content(corrupt)

    def content(self, i: int) -> np.ndarray:
        d = self.descs[i]
        if self.kind == "tcp":
            return tcp_bytes(int(d["length"]), int(d["skip_head"]), int(d["expected_pattern_offset"]))
        return datagram_bytes(int(d["length"]), int(self.headers["sequence_number"][i]))

    def _verified(self, off: int):
        """The descriptor whose verified region holds arena byte `off`, or None."""
        for i, d in enumerate(self.descs):
            lo = int(d["byte_offset"]) + int(self.heads[i])
            if not self.bad[i] and lo <= off < int(d["byte_offset"]) + int(d["length"]):
                return i
        return None

    def _write_content(self, corrupt: bool) -> None:
        seam, ring = self.seam, self.ring
        for i in np.nonzero(~self.bad)[0]:
            ring.write(int(self.descs["byte_offset"][i]), self.content(int(i)))
        if not corrupt:
            return
        dirty = set()
        for off, mask in ((seam - 1, 0x01), (seam, 0x80)):
            i = self._verified(off)
            if i is not None:
                ring.flip(off, mask)
                self.flips.append(off)
                dirty.add(i)
        # the low aliases of the descriptors that start at or above the seam hold the opposite
        for i in np.nonzero(~self.bad & (self.descs["byte_offset"] >= seam))[0]:
            data = self.content(int(i))
            if int(i) not in dirty:
                data[min(int(self.heads[i]) + 5, len(data) - 1)] ^= 0x10
            ring.write(int(self.descs["byte_offset"][i]) % seam, data)

    def seam_spans(self) -> dict:
        seam, d = self.seam, self.descs
        end = d["byte_offset"].astype(np.int64) + d["length"].astype(np.int64)
        off = d["byte_offset"].astype(np.int64)
        return {"crossing": bool(((off < seam) & (end > seam) & (off % 16 != 0)).any()),
                "at": bool((off == seam).any()), "minus1": bool((off == seam - 1).any()),
                "plus1": bool((off == seam + 1).any()), "above_16g": bool((off > 4 * seam).any()),
                "leaves": bool(self.bad.any())}

    def outcome(self, defect=None, what: str = "verify") -> dict:
        """what "verify": the oracle's rows, counters and first-failure slots (kind "tcp") or records, results,
        statuses and counters (kind "ms"); what "fill": {"ring": the bytes cts_fill / cts_media_stream_fill write}."""
        if what == "fill":
            return {"ring": self._filled(defect)}
        arena, d = compact_view(self.ring, self.descs, self.arena_bytes, defect, self.seam, head=self.heads)
        if self.kind == "tcp":
            res, ctr, cff = oracle.verify_batch(arena, d, n_conns=self.n_conns)
            return {"results": res, "counters": ctr, "cff": cff}
        recs, res, ctr = oracle.media_stream_verify(arena, d)
        return {"records": recs, "results": res, "status": status_of(recs, res), "counters": ctr}

    def _filled(self, defect) -> SparseRing:
        out = SparseRing(self.arena_bytes)
        for i, d in enumerate(self.descs):
            off, length, head = int(d["byte_offset"]), int(d["length"]), int(self.heads[i])
            if length < head or leaves_arena(off, length, self.arena_bytes, defect, self.seam):
                continue
            data, at = self.content(i), 0
            for o, c in read_pieces(off, length, head, defect, self.seam):
                if self.kind == "ms" or at >= head:  # cts_fill leaves the skipped head alone
                    out.write(o, data[at:at + c])
                elif at + c > head:
                    out.write(o + head - at, data[head:at + c])
                at += c
        return out

    def windows(self) -> list:
        d = self.descs[~self.bad]
        spans = [(int(o), int(o) + int(n)) for o, n in zip(d["byte_offset"], d["length"])]
        return _windows_of(spans + [(self.arena_bytes - 100, self.arena_bytes)], self.arena_bytes, self.seam)


# ---- tick plans ----------------------------------------------------------------------------------------------------
SERVER_STRIDES = (1040, 65536, 1 << 20)
TCP_SHAPES = ((65536, 65531), (65552, 65531), (16384, 9000), (1488, 1472))
TICKS = 2


class TickPlan:
    """Two ticks of a device-resident sender whose slots lie below, across and above the seam: the first at
    first_slot = seam // stride - 3, the second at first_slot + what the first one wrote.

    kind "server": cts_media_stream_servers_send; "tcp": cts_tcp_senders_send; "paced": cts_tcp_senders_send_paced,
    with pace "cut" (a rate limit stops two connections in the tick) or "unpaced"; "exchange":
    cts_tcp_exchange_send over a Push, a Pull, two PushPull (one seeked far out, so that its push-to-pull turn falls
    inside the first tick), a Duplex connection and one that finds no room.

    The expected state comes from the models of ctstraffic_amd.workload, run at the rebased first slot 1 over a host
    arena that starts one slot below the first tick; rebase=False runs them at the true first slot over a host arena
    from byte 0 (only feasible for a scaled-down seam), which tests/test_far_offsets_cpu.py compares."""

    def __init__(self, kind: str, stride: int, B: int = 0, seam: int = SEAM, pace: str = "cut", rebase: bool = True):
        self.kind, self.stride, self.B, self.seam, self.pace_kind = kind, int(stride), int(B), int(seam), pace
        s = self.stride
        self.first_slot = seam // s - 3
        assert self.first_slot >= 1
        self.base_slot = self.first_slot - 1 if rebase else 0
        if kind == "server":
            big = min(s, 65536) if s <= 65536 else 1472
            self.settings = [(3 * big + 5, big, 9), (27, 53, 9), (2 * 60 + 30, 60, 9), (big, big, 9),
                             (4 * big, big, 9)]
            self.ids = [3, 1, 0, 2, 4]          # slot 3 of the first tick is a full datagram of connection 0
            self.capacity = 12                  # 1 + 1 + 4 + 3, connection 4 finds no room
            self.entries = W.media_stream_server_entries(self.settings)
        elif kind == "exchange":
            B = self.B
            Pb, Qb = 2 * B + B // 2, B + 1      # a cycle is the buffers B, B, B // 2 | B, 1
            self.settings = [(0, 8 * B, B), (1, 3 * B + 1, B), (2, 1 << 60, B, Pb, Qb), (2, 20 * B + 7, B, Pb, Qb),
                             (3, 5 * B + 3, B), (0, 6 * B, B)]
            self.seek = [0, 0, 5 * ((1 << 33) // 5 + 1) + 1, 0, 0, 0]   # buffers B, B // 2 | B of a cycle far out
            self.ids = [2, 0, 4, 1, 3, 5]
            self.max_buffers = 3
            self.capacity = 14                  # 3 + 3 + 3 + 3 + 2 of 3, connection 5 finds no room
            self.entries = W.tcp_exchange_entries(self.settings, seek=self.seek)
        else:
            B = self.B
            self.settings = [(3 * B + 1, B), (8 * B, B), (2 * B + B // 2 + 1, B), (1 << 40, B), (1, B), (6 * B, B)]
            self.ids = [3, 0, 4, 1, 2, 5]
            self.max_buffers = 3
            self.capacity = 12                  # 3 + 3 + 1 + 3 + 2 of 3, connection 5 finds no room
            self.entries = W.tcp_sender_entries(self.settings)
            self.entries["bytes_sent"][3] = 7 * 65536 - 2 * B + 1
            cut = dict(bytes_per_second=10 * B, period_ms=1000)   # 10 B a quantum: B, then nothing until the next
            self.pace_settings = ([{}, cut, {}, dict(burst_count=2, burst_delay_ms=50), {}, {}]
                                  if pace == "cut" else [{}] * 6)
            self.pace = W.tcp_sender_pace_entries(self.pace_settings, 1000)
            self.now = (1000, 1010)
        self.arena_slots = self.first_slot + TICKS * self.capacity + 2
        self.arena_bytes = self.arena_slots * s
        self.host_slots = self.arena_slots - self.base_slot
        self._ticks = None

    # -- the models
    def ticks(self) -> list:
        """Per tick a dict: first_slot, written, descs (DESC_DTYPE[capacity], byte_offset on the device), codes,
        tick, and the state after it (entries, counters / udp, lengths, pace, tail), and `host`, the host arena."""
        if self._ticks is not None:
            return self._ticks
        s, shift = self.stride, self.base_slot * self.stride
        host = np.full(self.host_slots * s, BACKGROUND, dtype=np.uint8)
        out, first = [], self.first_slot
        if self.kind == "server":
            view = W.media_stream_server_view(self.entries, s, host, self.capacity)
            for t in range(TICKS):
                codes, tick = view.send(self.ids, QPC + t, QPF, first_slot=first - self.base_slot)
                descs = view.descs.copy()
                n = tick["datagrams"]
                descs["byte_offset"][:n] += np.uint64(shift)
                out.append(dict(first_slot=first, written=n, descs=descs, codes=codes.copy(), tick=dict(tick),
                                entries=view.entries.copy(), udp=dict(view.udp), lengths=view.lengths.copy(),
                                host=view.ring.copy()))
                first += n
        else:
            entries, pace, counters = self.entries, getattr(self, "pace", None), None
            descs, left = np.zeros(self.capacity, DESC_DTYPE), np.zeros(self.capacity, DESC_DTYPE)
            for t in range(TICKS):
                if self.kind == "tcp":
                    v = W.tcp_sender_view(entries, s, host, first - self.base_slot, self.capacity, self.ids,
                                          self.max_buffers, descs=descs, counters=counters)
                elif self.kind == "exchange":
                    v = W.tcp_exchange_view(entries, s, host, first - self.base_slot, self.capacity, self.ids,
                                            self.max_buffers, descs=descs, counters=counters)
                else:
                    v = W.tcp_paced_sender_view(entries, pace, self.now[t], s, host, first - self.base_slot,
                                                self.capacity, self.ids, self.max_buffers, descs=descs,
                                                counters=counters)
                    pace = v.pace
                entries, host, counters, n, descs = v.entries, v.arena, v.counters, v.tick["buffers"], v.descs
                left[:n] = descs[:n]   # what the device's array holds: this tick's, then the older ticks' rest
                left["byte_offset"][:n] += np.uint64(shift)
                out.append(dict(first_slot=first, written=n, descs=left.copy(), codes=v.codes.copy(),
                                tick=dict(v.tick), entries=entries.copy(), counters=dict(counters), host=host,
                                pace=pace.copy() if self.kind == "paced" else None,
                                tail=dict(v.tail) if self.kind == "paced" else None))
                first += n
        self._ticks = out
        return out

    def seam_slots(self) -> dict:
        s, seam = self.stride, self.seam
        spans = [(int(d["byte_offset"]), int(d["byte_offset"]) + int(d["length"]))
                 for t in self.ticks() for d in t["descs"][: t["written"]]]
        return {"crossing": any(a < seam < b for a, b in spans), "at": any(a == seam for a, b in spans),
                "below": any(b <= seam for a, b in spans), "above": any(a > seam for a, b in spans)}

    def outcome(self, defect=None, n_ticks: int = TICKS) -> dict:
        """{"descs": the descriptors each of the first n_ticks ticks leaves, "ring": the bytes they write}."""
        s, seam, shift = self.stride, self.seam, self.base_slot * self.stride
        ring, all_descs = SparseRing(self.arena_bytes), []
        for t in self.ticks()[:n_ticks]:
            descs = t["descs"].copy()
            for g in range(t["written"]):
                off, length = int(descs["byte_offset"][g]), int(descs["length"][g])
                data = t["host"][off - shift:off - shift + length]
                if defect == "a":
                    off %= seam
                elif defect == "b":
                    off = (t["first_slot"] * s) % seam + g * s
                ring.write(off, data)
            if defect == "c":
                descs["byte_offset"][: t["written"]] %= np.uint64(seam)
            all_descs.append(descs)
        return {"descs": all_descs, "ring": ring}

    def windows(self) -> list:
        s, seam, spans = self.stride, self.seam, []
        for t in self.ticks():
            for g in range(t["written"]):
                off, length = int(t["descs"]["byte_offset"][g]), int(t["descs"]["length"][g])
                spans.append((off, off + length))
                wrapped = (t["first_slot"] * s) % seam + g * s
                spans.append((wrapped, wrapped + length))
        return _windows_of(spans, self.arena_bytes, seam)

    def seam_hit(self):
        """(tick, g, flip offset): the first datagram or buffer of the first tick with verified bytes at or above
        the seam, and the first such byte: where the receive half's dirty run flips a bit."""
        head = HEADER if self.kind == "server" else 0
        t = self.ticks()[0]
        for g in range(t["written"]):
            off, length = int(t["descs"]["byte_offset"][g]), int(t["descs"]["length"][g])
            if off + length > max(self.seam, off + head):
                return 0, g, max(self.seam, off + head)
        raise AssertionError("no slot above the seam")


# ---- one exchange tick that moves more than 4 GiB -------------------------------------------------------------------
BIG_STRIDE = 16 << 20  # the largest stride a tick takes


def big_exchange_tick() -> dict:
    """One cts_tcp_exchange_send whose bytes need more than 32 bits: stride 16 MiB, B = 16 MiB - 5, four PushPull
    connections of P = 3B, Q = B that take 86 buffers each (21 cycles and two more push buffers: 65 of direction 0,
    21 of direction 1) and a Duplex one that takes the 16 slots left of a capacity of 360. Direction 0 carries 268
    buffers, 2^32 bytes and more; the slot that starts at byte 2^32 of the arena is slot 256."""
    B = BIG_STRIDE - 5
    return {"stride": BIG_STRIDE, "B": B, "settings": [(2, 1 << 40, B, 3 * B, B)] * 4 + [(3, 1 << 40, B)],
            "ids": [0, 1, 2, 3, 4], "max_buffers": 86, "capacity": 360}
