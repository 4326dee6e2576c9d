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
from .tcp_senders import _PaceTable, _TickTable
from .types import TCP_EXCHANGE_DTYPE, TCP_EXCHANGE_PACED_TICK_DTYPE, TCP_EXCHANGE_TICK_DTYPE


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


class ExchangeTable(_TickTable):
    """Many two-way TCP connections on one device: the entry table (``entries``), a tick's scratch, the arena with its
    descriptors, the codes, the tick block and the sent block, with the tick as a method.

    settings: (pattern, transfer_bytes, buffer_size, push_bytes, pull_bytes) per connection slot (the last two may be
    left out). The arena holds arena_slots slots of stride bytes (pre-filled with `fill`), a tick writes at most
    capacity of them from first_slot on. ``descs_of(n)`` is the descriptor array of the tick's first n buffers for the
    receive half, whose tables have ``n_receivers`` = 2 x n_conns slots; ``expected_bytes()`` is their
    dev_expected_bytes."""

    _TABLE, _ENTRY_DTYPE, _TICK_DTYPE = "entries", TCP_EXCHANGE_DTYPE, TCP_EXCHANGE_TICK_DTYPE
    _init = staticmethod(lambda setting: exchange_init(*setting))
    _scratch_bytes = staticmethod(exchange_scratch_bytes)

    def __init__(self, engine, settings, stride: int, capacity: int, **kw):
        super().__init__(engine, settings, stride, capacity, **kw)
        self.n_receivers = 2 * self.n_conns

    def send(self, conn_ids, max_buffers: int, first_slot: int = 0, stream=None, capacity: int = None) -> None:
        """One tick of conn_ids (uint32/int32 device tensor, distinct, at most max_listed of them)."""
        self._tick(exchange_send, conn_ids, max_buffers, first_slot, stream, capacity)

    def expected_bytes(self) -> np.ndarray:
        """uint64[2 x n_conns]: what every receiver gets in total, direction-0 receivers first."""
        return np.array([exchange_direction_bytes(e, d) for d in (0, 1) for e in self.fresh], dtype=np.uint64)


class PacedExchangeTable(ExchangeTable, _PaceTable):
    """An ExchangeTable with a pace entry per side of every connection slot (``pace``) and the paced tick.

    pace_settings: per connection slot a pair (client, server) of dicts of tcp_senders.pace_init's keywords
    (bytes_per_second, period_ms, burst_count, burst_delay_ms; {} = unpaced): the client's pace direction 0, the
    server's direction 1. The pace table has 2 x n_conns entries, entry ``c + d * n_conns`` for direction d. Every
    first quantum starts at start_ms. ``send(conn_ids, max_buffers, now_ms)`` is one paced tick; the plain tick stays
    available as ``ExchangeTable.send(table, ...)`` over the same entries."""

    _TICK_DTYPE, _PACE_SIDES = TCP_EXCHANGE_PACED_TICK_DTYPE, 2
    _scratch_bytes = staticmethod(exchange_paced_scratch_bytes)

    def __init__(self, engine, settings, pace_settings, stride: int, capacity: int, start_ms: int = 0, **kw):
        super().__init__(engine, settings, stride, capacity, **kw)
        self._init_pace(pace_settings, start_ms)

    def send(self, conn_ids, max_buffers: int, now_ms: int, first_slot: int = 0, stream=None,
             capacity: int = None) -> None:
        """One paced tick of conn_ids (uint32/int32 device tensor, distinct, at most max_listed of them) at now_ms."""
        self._tick(exchange_send_paced, conn_ids, max_buffers, first_slot, stream, capacity, now_ms=now_ms)
