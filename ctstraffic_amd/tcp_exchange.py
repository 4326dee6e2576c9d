"""Push, Pull, PushPull and Duplex connections on the device-resident path (include/cts_tcp_exchange.h): the entry
helpers, the tick, and a table that holds what a tick needs.

A connection is a 64-byte entry per slot (types.TCP_EXCHANGE_DTYPE) whose buffers, in both directions, form one fixed
sequence; one :func:`exchange_send` writes up to ``max_buffers`` of them for every listed connection into consecutive
arena slots, with their descriptors. The receiver of direction d of connection c is slot ``c + d * n_conns`` of
receiver tables of ``2 * n_conns`` slots, and the receive half (Engine.verify with a base_index, Engine.refview_conns,
Engine.conns_close) runs over the descriptors unchanged. The model of a tick is workload.tcp_exchange_view.

Send pacing for every pattern is :func:`exchange_send_paced` over a pace table of ``2 * n_conns`` 64-byte entries
(types.TCP_SENDER_PACE_DTYPE, made by tcp_senders.pace_init), entry ``c + d * n_conns`` for the side that sends
direction d; :class:`PacedExchangeTable` holds one. Its model is workload.tcp_paced_exchange_view.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import check, lib
from .types import (DESC_DTYPE, TCP_EXCHANGE_DTYPE, TCP_EXCHANGE_PACED_TICK_DTYPE, TCP_EXCHANGE_TICK_DTYPE,
                    TCP_SENDER_PACE_DTYPE)


def _one(entry) -> np.ndarray:
    return np.array([entry], dtype=TCP_EXCHANGE_DTYPE)


def exchange_init(pattern: int, transfer_bytes: int, buffer_size: int, push_bytes: int = 0,
                  pull_bytes: int = 0) -> np.ndarray:
    """cts_tcp_exchange_init: a fresh cts_tcp_exchange_state (one TCP_EXCHANGE_DTYPE record) with its total_buffers.
    Raises CtsError for a transfer or a buffer size of 0, an unknown pattern, or PushPull without both segment
    sizes."""
    out = np.zeros(1, dtype=TCP_EXCHANGE_DTYPE)
    check("cts_tcp_exchange_init",
          lib().cts_tcp_exchange_init(pattern, transfer_bytes, buffer_size, push_bytes, pull_bytes, out.ctypes.data))
    return out[0]


def exchange_seek(entry, m: int) -> np.ndarray:
    """cts_tcp_exchange_seek: a copy of entry in the state after its first m buffers."""
    out = _one(entry)
    check("cts_tcp_exchange_seek", lib().cts_tcp_exchange_seek(out.ctypes.data, m))
    return out[0]


def exchange_where(entry):
    """cts_tcp_exchange_where: (direction of the next buffer, m_intraSegmentTransfer) at the entry's position."""
    e = _one(entry)
    d, intra = ctypes.c_uint32(), ctypes.c_uint32()
    check("cts_tcp_exchange_where", lib().cts_tcp_exchange_where(e.ctypes.data, ctypes.byref(d), ctypes.byref(intra)))
    return int(d.value), int(intra.value)


def exchange_direction_bytes(entry, direction: int) -> int:
    """cts_tcp_exchange_direction_bytes: what direction 0 or 1 of the entry's connection carries in total."""
    e = _one(entry)
    return int(lib().cts_tcp_exchange_direction_bytes(e.ctypes.data, direction))


def exchange_scratch_bytes(n: int) -> int:
    """cts_tcp_exchange_scratch_bytes: the scratch a tick over n listed connections needs."""
    return int(lib().cts_tcp_exchange_scratch_bytes(n))


def exchange_send(engine, arena, stride: int, first_slot: int, capacity: int, conn_ids, max_buffers: int, entries,
                  n_conns: int, descs, scratch, codes=None, tick=None, sent_counters=None, stream=None, n: int = None,
                  arena_bytes: int = None, scratch_bytes: int = None) -> None:
    """cts_tcp_exchange_send: one tick of the connections conn_ids (uint32/int32 device tensor, distinct) into slots
    first_slot .. of arena. descs (24 bytes per slot of the capacity) is required; codes (4 bytes per id), tick (48
    bytes) and sent_counters are device tensors or None. Raises CtsError(CTS_E_INVALID) for a refused argument."""
    from .engine import _nbytes, _ptr, _stream

    n = _nbytes(conn_ids) // 4 if n is None else n
    check("cts_tcp_exchange_send",
          engine._L.cts_tcp_exchange_send(
              engine._h, _ptr(arena), _nbytes(arena) if arena_bytes is None else arena_bytes, stride, first_slot,
              capacity, _ptr(conn_ids), n, max_buffers, _ptr(entries), n_conns, _ptr(descs), _ptr(codes), _ptr(tick),
              _ptr(sent_counters), _ptr(scratch), _nbytes(scratch) if scratch_bytes is None else scratch_bytes,
              _stream(stream)))


def exchange_paced_scratch_bytes(n: int) -> int:
    """cts_tcp_exchange_paced_scratch_bytes: the scratch a paced tick over n listed connections needs."""
    return int(lib().cts_tcp_exchange_paced_scratch_bytes(n))


def exchange_send_paced(engine, arena, stride: int, first_slot: int, capacity: int, conn_ids, max_buffers: int,
                        entries, pace, n_conns: int, now_ms: int, descs, scratch, codes=None, tick=None,
                        sent_counters=None, stream=None, n: int = None, arena_bytes: int = None,
                        scratch_bytes: int = None) -> None:
    """cts_tcp_exchange_send_paced: :func:`exchange_send` at the time now_ms over the pace table `pace` (64 bytes per
    side: 2 x n_conns entries); tick is 64 bytes or None. Raises CtsError(CTS_E_INVALID) for a refused argument."""
    from .engine import _nbytes, _ptr, _stream

    n = _nbytes(conn_ids) // 4 if n is None else n
    check("cts_tcp_exchange_send_paced",
          engine._L.cts_tcp_exchange_send_paced(
              engine._h, _ptr(arena), _nbytes(arena) if arena_bytes is None else arena_bytes, stride, first_slot,
              capacity, _ptr(conn_ids), n, max_buffers, _ptr(entries), _ptr(pace), n_conns, now_ms, _ptr(descs),
              _ptr(codes), _ptr(tick), _ptr(sent_counters), _ptr(scratch),
              _nbytes(scratch) if scratch_bytes is None else scratch_bytes, _stream(stream)))


class ExchangeTable:
    """Many two-way TCP connections on one device: the entry table, a tick's scratch, the arena with its descriptors,
    the codes, the tick block and the sent block, with the tick as a method.

    settings: (pattern, transfer_bytes, buffer_size, push_bytes, pull_bytes) per connection slot (the last two may be
    left out). The arena holds arena_slots slots of stride bytes (pre-filled with `fill`), a tick writes at most
    capacity of them from first_slot on. ``descs_of(n)`` is the descriptor array of the tick's first n buffers for the
    receive half, whose tables have ``n_receivers`` = 2 x n_conns slots; ``expected_bytes()`` is their
    dev_expected_bytes."""

    def __init__(self, engine, settings, stride: int, capacity: int, arena_slots: int = None, device=None,
                 fill: int = 0, max_listed: int = None):
        import torch

        self.engine = engine
        self.device = device or "cuda:%d" % engine.device
        self.fresh = np.zeros(len(settings), dtype=TCP_EXCHANGE_DTYPE)
        for c, s in enumerate(settings):
            self.fresh[c] = exchange_init(*s)
        self.n_conns, self.stride, self.capacity = len(settings), stride, capacity
        self.n_receivers = 2 * self.n_conns
        self.arena_slots = capacity if arena_slots is None else arena_slots
        words = max(1, self.n_conns) * (TCP_EXCHANGE_DTYPE.itemsize // 8)
        self.entries = torch.zeros(words, dtype=torch.int64, device=self.device)
        self.load(self.fresh)
        self.max_listed = max(1, self.n_conns if max_listed is None else max_listed)
        self.scratch = torch.zeros((exchange_scratch_bytes(self.max_listed) + 7) // 8, dtype=torch.int64,
                                   device=self.device)
        self.arena = torch.full((max(16, self.arena_slots * stride),), fill, dtype=torch.uint8, device=self.device)
        self.descs = torch.zeros(max(1, capacity) * (DESC_DTYPE.itemsize // 8), dtype=torch.int64, device=self.device)
        self.codes = torch.zeros(self.max_listed, dtype=torch.int32, device=self.device)
        self.tick = torch.zeros(TCP_EXCHANGE_TICK_DTYPE.itemsize // 8, dtype=torch.int64, device=self.device)
        self.sent = engine.new_counters()

    def send(self, conn_ids, max_buffers: int, first_slot: int = 0, stream=None, capacity: int = None) -> None:
        """One tick of conn_ids (uint32/int32 device tensor, distinct, at most max_listed of them)."""
        from .engine import _nbytes

        n = _nbytes(conn_ids) // 4
        if n > self.codes.numel():
            raise ValueError("%d ids listed, the table's codes and scratch hold %d" % (n, self.codes.numel()))
        capacity = self.capacity if capacity is None else capacity
        if capacity > self.capacity:
            raise ValueError("capacity %d, the table's descriptors hold %d" % (capacity, self.capacity))
        exchange_send(self.engine, self.arena, self.stride, first_slot, capacity, conn_ids, max_buffers, self.entries,
                      self.n_conns, self.descs, self.scratch, codes=self.codes, tick=self.tick,
                      sent_counters=self.sent, stream=stream)

    def load(self, entries: np.ndarray) -> None:
        """Write entries (TCP_EXCHANGE_DTYPE[n_conns]) over the table: a transfer resumed, or a test's preset."""
        import torch

        e = np.ascontiguousarray(entries, dtype=TCP_EXCHANGE_DTYPE)
        if len(e) != self.n_conns:
            raise ValueError("%d entries for a table of %d" % (len(e), self.n_conns))
        if self.n_conns:
            self.entries.copy_(torch.from_numpy(e.view(np.int64).copy()))

    def expected_bytes(self) -> np.ndarray:
        """uint64[2 x n_conns]: what every receiver gets in total, direction-0 receivers first."""
        return np.array([exchange_direction_bytes(e, d) for d in (0, 1) for e in self.fresh], dtype=np.uint64)

    def descs_of(self, n: int):
        """The descriptors of the last tick's first n buffers (a view)."""
        return self.descs[: n * (DESC_DTYPE.itemsize // 8)]

    def read(self):
        """(entries TCP_EXCHANGE_DTYPE, codes uint32, tick: one TCP_EXCHANGE_TICK_DTYPE record) copied to the host."""
        return (self.entries.cpu().numpy().view(TCP_EXCHANGE_DTYPE)[: self.n_conns],
                self.codes.cpu().numpy().view(np.uint32), self.tick.cpu().numpy().view(TCP_EXCHANGE_TICK_DTYPE)[0])

    def read_arena(self):
        """(arena bytes, descriptors DESC_DTYPE[capacity]) copied to the host."""
        return self.arena.cpu().numpy(), self.descs.cpu().numpy().view(DESC_DTYPE)[: self.capacity]

    def read_sent(self, stream=None) -> dict:
        return self.engine.read_counters_sent(self.sent, stream=stream)


class PacedExchangeTable(ExchangeTable):
    """An ExchangeTable with a pace entry per side of every connection slot and the paced tick.

    pace_settings: per connection slot a pair (client, server) of dicts of tcp_senders.pace_init's keywords
    (bytes_per_second, period_ms, burst_count, burst_delay_ms; {} = unpaced): the client's pace direction 0, the
    server's direction 1. The pace table has 2 x n_conns entries, entry ``c + d * n_conns`` for direction d. Every
    first quantum starts at start_ms. ``send(conn_ids, max_buffers, now_ms)`` is one paced tick; the plain tick stays
    available as ``ExchangeTable.send(table, ...)`` over the same entries."""

    def __init__(self, engine, settings, pace_settings, stride: int, capacity: int, start_ms: int = 0, **kw):
        import torch

        from .tcp_senders import pace_init

        super().__init__(engine, settings, stride, capacity, **kw)
        if len(pace_settings) != self.n_conns:
            raise ValueError("%d pace settings for a table of %d" % (len(pace_settings), self.n_conns))
        self.fresh_pace = np.zeros(2 * self.n_conns, dtype=TCP_SENDER_PACE_DTYPE)
        for c, sides in enumerate(pace_settings):
            for d in (0, 1):
                self.fresh_pace[c + d * self.n_conns] = pace_init(start_ms=start_ms, **sides[d])
        words = max(1, 2 * self.n_conns) * (TCP_SENDER_PACE_DTYPE.itemsize // 8)
        self.pace = torch.zeros(words, dtype=torch.int64, device=self.device)
        self.load_pace(self.fresh_pace)
        self.scratch = torch.zeros((exchange_paced_scratch_bytes(self.max_listed) + 7) // 8, dtype=torch.int64,
                                   device=self.device)
        self.tick = torch.zeros(TCP_EXCHANGE_PACED_TICK_DTYPE.itemsize // 8, dtype=torch.int64, device=self.device)

    def send(self, conn_ids, max_buffers: int, now_ms: int, first_slot: int = 0, stream=None,
             capacity: int = None) -> None:
        """One paced tick of conn_ids (uint32/int32 device tensor, distinct, at most max_listed of them) at now_ms."""
        from .engine import _nbytes

        n = _nbytes(conn_ids) // 4
        if n > self.codes.numel():
            raise ValueError("%d ids listed, the table's codes and scratch hold %d" % (n, self.codes.numel()))
        capacity = self.capacity if capacity is None else capacity
        if capacity > self.capacity:
            raise ValueError("capacity %d, the table's descriptors hold %d" % (capacity, self.capacity))
        exchange_send_paced(self.engine, self.arena, self.stride, first_slot, capacity, conn_ids, max_buffers,
                            self.entries, self.pace, self.n_conns, now_ms, self.descs, self.scratch, codes=self.codes,
                            tick=self.tick, sent_counters=self.sent, stream=stream)

    def load_pace(self, pace: np.ndarray) -> None:
        """Write pace (TCP_SENDER_PACE_DTYPE[2 x n_conns]) over the pace table."""
        import torch

        q = np.ascontiguousarray(pace, dtype=TCP_SENDER_PACE_DTYPE)
        if len(q) != 2 * self.n_conns:
            raise ValueError("%d pace entries for a table of %d connections" % (len(q), self.n_conns))
        if self.n_conns:
            self.pace.copy_(torch.from_numpy(q.view(np.int64).copy()))

    def read(self):
        """(entries, codes uint32, tick: one TCP_EXCHANGE_PACED_TICK_DTYPE record) copied to the host."""
        return (self.entries.cpu().numpy().view(TCP_EXCHANGE_DTYPE)[: self.n_conns],
                self.codes.cpu().numpy().view(np.uint32),
                self.tick.cpu().numpy().view(TCP_EXCHANGE_PACED_TICK_DTYPE)[0])

    def read_pace(self) -> np.ndarray:
        """The pace table (TCP_SENDER_PACE_DTYPE[2 x n_conns]) copied to the host."""
        return self.pace.cpu().numpy().view(TCP_SENDER_PACE_DTYPE)[: 2 * self.n_conns]
