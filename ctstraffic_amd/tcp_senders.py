"""TCP senders on the device-resident path (include/cts_tcp_senders.h): the entry initialiser, the tick, and a table
that holds what a tick needs.

A sender is a 32-byte entry per connection slot (types.TCP_SENDER_DTYPE); one :func:`senders_send` writes up to
``max_buffers`` buffers of every listed connection into consecutive arena slots, with their descriptors, and the
receive half (Engine.verify with a base_index, Engine.refview_conns, Engine.conns_close) runs over those descriptors
unchanged. The model of a tick is workload.tcp_sender_view.

Send pacing (-RateLimit, -BurstCount / -BurstDelay) is a second table of 64-byte entries
(types.TCP_SENDER_PACE_DTYPE) and :func:`senders_send_paced`, which takes the time: every listed connection sends what
its pace entry lets out at ``now_ms``, and the 48-byte tick block ends with the time of the next deferred send.
:class:`PacedSenderTable` holds both tables; the model is workload.tcp_paced_sender_view.
"""
from __future__ import annotations

import numpy as np

from ._lib import check, lib
from .types import (DESC_DTYPE, TCP_SENDER_DTYPE, TCP_SENDER_PACE_DTYPE, TCP_SENDER_PACED_TICK_DTYPE,
                    TCP_SENDER_TICK_DTYPE)


def sender_init(transfer_bytes: int, buffer_size: int) -> np.ndarray:
    """cts_tcp_sender_init: a fresh cts_tcp_sender_state (one TCP_SENDER_DTYPE record). Raises CtsError for a
    transfer or a buffer size of 0."""
    out = np.zeros(1, dtype=TCP_SENDER_DTYPE)
    check("cts_tcp_sender_init", lib().cts_tcp_sender_init(transfer_bytes, buffer_size, out.ctypes.data))
    return out[0]


def senders_scratch_bytes(n: int) -> int:
    """cts_tcp_senders_scratch_bytes: the scratch a tick over n listed connections needs."""
    return int(lib().cts_tcp_senders_scratch_bytes(n))


def senders_send(engine, arena, stride: int, first_slot: int, capacity: int, conn_ids, max_buffers: int, senders,
                 n_conns: int, descs, scratch, codes=None, tick=None, sent_counters=None, stream=None, n: int = None,
                 arena_bytes: int = None, scratch_bytes: int = None) -> None:
    """cts_tcp_senders_send: one tick of the connections conn_ids (uint32/int32 device tensor, distinct) into slots
    first_slot .. of arena. descs (24 bytes per slot of the capacity) is required; codes (4 bytes per id), tick (32
    bytes) and sent_counters are device tensors or None. Raises CtsError(CTS_E_INVALID) for a refused argument."""
    from .engine import _nbytes, _ptr, _stream

    n = _nbytes(conn_ids) // 4 if n is None else n
    check("cts_tcp_senders_send",
          engine._L.cts_tcp_senders_send(
              engine._h, _ptr(arena), _nbytes(arena) if arena_bytes is None else arena_bytes, stride, first_slot,
              capacity, _ptr(conn_ids), n, max_buffers, _ptr(senders), n_conns, _ptr(descs), _ptr(codes), _ptr(tick),
              _ptr(sent_counters), _ptr(scratch), _nbytes(scratch) if scratch_bytes is None else scratch_bytes,
              _stream(stream)))


def pace_init(bytes_per_second: int = 0, period_ms: int = 0, burst_count: int = 0, burst_delay_ms: int = 0,
              start_ms: int = 0) -> np.ndarray:
    """cts_tcp_sender_pace_init: a fresh cts_tcp_sender_pace (one TCP_SENDER_PACE_DTYPE record) whose first quantum
    starts at start_ms. Raises CtsError for a negative start_ms or a rate x period beyond an int64."""
    out = np.zeros(1, dtype=TCP_SENDER_PACE_DTYPE)
    check("cts_tcp_sender_pace_init",
          lib().cts_tcp_sender_pace_init(bytes_per_second, period_ms, burst_count, burst_delay_ms, start_ms,
                                         out.ctypes.data))
    return out[0]


def senders_paced_scratch_bytes(n: int) -> int:
    """cts_tcp_senders_paced_scratch_bytes: the scratch a paced tick over n listed connections needs."""
    return int(lib().cts_tcp_senders_paced_scratch_bytes(n))


def senders_send_paced(engine, arena, stride: int, first_slot: int, capacity: int, conn_ids, max_buffers: int,
                       senders, pace, n_conns: int, now_ms: int, descs, scratch, codes=None, tick=None,
                       sent_counters=None, stream=None, n: int = None, arena_bytes: int = None,
                       scratch_bytes: int = None) -> None:
    """cts_tcp_senders_send_paced: :func:`senders_send` at the time now_ms over the pace table `pace` (64 bytes per
    connection slot); tick is 48 bytes or None. Raises CtsError(CTS_E_INVALID) for a refused argument."""
    from .engine import _nbytes, _ptr, _stream

    n = _nbytes(conn_ids) // 4 if n is None else n
    check("cts_tcp_senders_send_paced",
          engine._L.cts_tcp_senders_send_paced(
              engine._h, _ptr(arena), _nbytes(arena) if arena_bytes is None else arena_bytes, stride, first_slot,
              capacity, _ptr(conn_ids), n, max_buffers, _ptr(senders), _ptr(pace), n_conns, now_ms, _ptr(descs),
              _ptr(codes), _ptr(tick), _ptr(sent_counters), _ptr(scratch),
              _nbytes(scratch) if scratch_bytes is None else scratch_bytes, _stream(stream)))


class _TickTable:
    """What the four TCP tick tables share: the entry table on one device, a tick's scratch, the arena with its
    descriptors, the codes, the tick block and the sent block, the checks of a tick's arguments and the reads.

    A table class names its entry table (_TABLE, the attribute that holds it) and gives the entries' and the tick
    block's dtypes, the entry initialiser (_init, called with one connection slot's setting) and the scratch size
    (_scratch_bytes); its ``send`` passes its own tick function to :meth:`_tick`, so a base class's tick stays
    available on a derived table as ``Base.send(table, ...)``."""

    _TABLE = _ENTRY_DTYPE = _TICK_DTYPE = _init = _scratch_bytes = None

    def __init__(self, engine, settings, stride: int, capacity: int, arena_slots: int = None, device=None,
                 fill: int = 0, max_listed: int = None):
        import torch

        self.engine = engine
        self.device = device or "cuda:%d" % engine.device
        self.fresh = np.zeros(len(settings), dtype=self._ENTRY_DTYPE)
        for c, setting in enumerate(settings):
            self.fresh[c] = type(self)._init(setting)
        self.n_conns, self.stride, self.capacity = len(settings), stride, capacity
        self.arena_slots = capacity if arena_slots is None else arena_slots
        words = max(1, self.n_conns) * (self._ENTRY_DTYPE.itemsize // 8)
        setattr(self, self._TABLE, torch.zeros(words, dtype=torch.int64, device=self.device))
        self.load(self.fresh)
        self.max_listed = max(1, self.n_conns if max_listed is None else max_listed)
        self.scratch = torch.zeros((type(self)._scratch_bytes(self.max_listed) + 7) // 8, dtype=torch.int64,
                                   device=self.device)
        self.arena = torch.full((max(16, self.arena_slots * stride),), fill, dtype=torch.uint8, device=self.device)
        self.descs = torch.zeros(max(1, capacity) * (DESC_DTYPE.itemsize // 8), dtype=torch.int64, device=self.device)
        self.codes = torch.zeros(self.max_listed, dtype=torch.int32, device=self.device)
        self.tick = torch.zeros(self._TICK_DTYPE.itemsize // 8, dtype=torch.int64, device=self.device)
        self.sent = engine.new_counters()

    def _tick(self, send, conn_ids, max_buffers: int, first_slot: int, stream, capacity: int, now_ms: int = None):
        """One tick through `send` (one of the four *_send functions; a paced one takes now_ms)."""
        from .engine import _nbytes

        n = _nbytes(conn_ids) // 4
        if n > self.codes.numel():
            raise ValueError("%d ids listed, the table's codes and scratch hold %d" % (n, self.codes.numel()))
        capacity = self.capacity if capacity is None else capacity
        if capacity > self.capacity:
            raise ValueError("capacity %d, the table's descriptors hold %d" % (capacity, self.capacity))
        table = getattr(self, self._TABLE)
        tables = (table, self.n_conns) if now_ms is None else (table, self.pace, self.n_conns, now_ms)
        send(self.engine, self.arena, self.stride, first_slot, capacity, conn_ids, max_buffers, *tables, self.descs,
             self.scratch, codes=self.codes, tick=self.tick, sent_counters=self.sent, stream=stream)

    def load(self, entries: np.ndarray) -> None:
        """Write entries (the table's entry dtype, n_conns of them) over the table: a transfer resumed, or a test's
        preset."""
        import torch

        e = np.ascontiguousarray(entries, dtype=self._ENTRY_DTYPE)
        if len(e) != self.n_conns:
            raise ValueError("%d entries for a table of %d" % (len(e), self.n_conns))
        if self.n_conns:
            getattr(self, self._TABLE).copy_(torch.from_numpy(e.view(np.int64).copy()))

    def descs_of(self, n: int):
        """The descriptors of the last tick's first n buffers (a view)."""
        return self.descs[: n * (DESC_DTYPE.itemsize // 8)]

    def read(self):
        """(entries, codes uint32, tick: one record of the table's tick dtype) copied to the host."""
        return (getattr(self, self._TABLE).cpu().numpy().view(self._ENTRY_DTYPE)[: self.n_conns],
                self.codes.cpu().numpy().view(np.uint32), self.tick.cpu().numpy().view(self._TICK_DTYPE)[0])

    def read_arena(self):
        """(arena bytes, descriptors DESC_DTYPE[capacity]) copied to the host."""
        return self.arena.cpu().numpy(), self.descs.cpu().numpy().view(DESC_DTYPE)[: self.capacity]

    def read_sent(self, stream=None) -> dict:
        return self.engine.read_counters_sent(self.sent, stream=stream)


class _PaceTable:
    """The pace table of a paced tick table, beside a :class:`_TickTable`: _PACE_SIDES entries per connection slot
    (TCP_SENDER_PACE_DTYPE), entry ``c + d * n_conns`` for side d."""

    _PACE_SIDES = 1

    def _init_pace(self, pace_settings, start_ms: int) -> None:
        """pace_settings: per connection slot _PACE_SIDES dicts of :func:`pace_init`'s keywords."""
        import torch

        if len(pace_settings) != self.n_conns:
            raise ValueError("%d pace settings for a table of %d" % (len(pace_settings), self.n_conns))
        self.fresh_pace = np.zeros(self._PACE_SIDES * self.n_conns, dtype=TCP_SENDER_PACE_DTYPE)
        for c, sides in enumerate(pace_settings):
            for d in range(self._PACE_SIDES):
                self.fresh_pace[c + d * self.n_conns] = pace_init(start_ms=start_ms, **sides[d])
        words = max(1, len(self.fresh_pace)) * (TCP_SENDER_PACE_DTYPE.itemsize // 8)
        self.pace = torch.zeros(words, dtype=torch.int64, device=self.device)
        self.load_pace(self.fresh_pace)

    def load_pace(self, pace: np.ndarray) -> None:
        """Write pace (TCP_SENDER_PACE_DTYPE, _PACE_SIDES x n_conns of them) over the pace table."""
        import torch

        q = np.ascontiguousarray(pace, dtype=TCP_SENDER_PACE_DTYPE)
        if len(q) != self._PACE_SIDES * self.n_conns:
            raise ValueError("%d pace entries for a table of %d connections" % (len(q), self.n_conns))
        if self.n_conns:
            self.pace.copy_(torch.from_numpy(q.view(np.int64).copy()))

    def read_pace(self) -> np.ndarray:
        """The pace table (TCP_SENDER_PACE_DTYPE, _PACE_SIDES x n_conns of them) copied to the host."""
        return self.pace.cpu().numpy().view(TCP_SENDER_PACE_DTYPE)[: self._PACE_SIDES * self.n_conns]


class SenderTable(_TickTable):
    """Many TCP senders on one device: the entry table (``senders``), a tick's scratch, the arena with its
    descriptors, the codes, the tick block and the sent block, with the tick as a method.

    settings: (transfer_bytes, buffer_size) per connection slot. The arena holds arena_slots slots of stride bytes
    (pre-filled with `fill`), a tick writes at most capacity of them from first_slot on. ``descs_of(n)`` is the
    descriptor array of the tick's first n buffers for the receive half, with n computed from the settings: nothing is
    read back between the send and the receive pass."""

    _TABLE, _ENTRY_DTYPE, _TICK_DTYPE = "senders", TCP_SENDER_DTYPE, TCP_SENDER_TICK_DTYPE
    _init = staticmethod(lambda setting: sender_init(*setting))
    _scratch_bytes = staticmethod(senders_scratch_bytes)

    def send(self, conn_ids, max_buffers: int, first_slot: int = 0, stream=None, capacity: int = None) -> None:
        """One tick of conn_ids (uint32/int32 device tensor, distinct, at most max_listed of them)."""
        self._tick(senders_send, conn_ids, max_buffers, first_slot, stream, capacity)


class PacedSenderTable(SenderTable, _PaceTable):
    """A SenderTable with a pace entry per connection slot (``pace``) and the paced tick.

    settings: (transfer_bytes, buffer_size) per connection slot; pace_settings: per slot a dict of
    :func:`pace_init`'s keywords (bytes_per_second, period_ms, burst_count, burst_delay_ms; {} = unpaced). Every
    first quantum starts at start_ms. ``send(conn_ids, max_buffers, now_ms)`` is one paced tick; the plain tick
    stays available as ``SenderTable.send(table, ...)`` over the same entries."""

    _TICK_DTYPE = TCP_SENDER_PACED_TICK_DTYPE
    _scratch_bytes = staticmethod(senders_paced_scratch_bytes)

    def __init__(self, engine, settings, pace_settings, stride: int, capacity: int, start_ms: int = 0, **kw):
        super().__init__(engine, settings, stride, capacity, **kw)
        self._init_pace([(s,) for s in pace_settings], start_ms)

    def send(self, conn_ids, max_buffers: int, now_ms: int, first_slot: int = 0, stream=None,
             capacity: int = None) -> None:
        """One paced tick of conn_ids (uint32/int32 device tensor, distinct, at most max_listed of them) at now_ms."""
        self._tick(senders_send_paced, conn_ids, max_buffers, first_slot, stream, capacity, now_ms=now_ms)
