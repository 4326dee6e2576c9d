"""MediaStream (UDP) framing around the verify path — Python handle over
include/cts_media_stream.h.

* :func:`split` — ctsMediaStreamSendRequests' datagram sizes for one frame
  (ctsMediaStreamProtocol.hpp:151-205);
* :func:`fill` / :func:`verify` — the gfx950 datagram kernels (sender
  materialisation; receiver header parse + validate + payload verify);
* :class:`MediaStreamClient` — ctsIoPatternMediaStreamClient's frame accounting
  (ctsIOPatternMediaStream.cpp), driven by explicit render ticks.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import CtsError, check, lib
from .types import DESC_DTYPE, DGRAM_HEADER_DTYPE, DGRAM_RECORD_DTYPE, DGRAM_STATUS_DTYPE, RESULT_DTYPE

DGRAM_DATA, DGRAM_ID, DGRAM_ZERO, DGRAM_SHORT, DGRAM_UNKNOWN, DGRAM_BAD_DESC = range(6)
FLAG_DATA, FLAG_ID = 0x0000, 0x1000
DATA_HEADER_LENGTH = 26
CONNECTION_ID_HEADER_LENGTH = 39


class Settings(ctypes.Structure):
    """ctsConfig::MediaStreamSettings (the fields the client reads)."""

    _fields_ = [("frame_size_bytes", ctypes.c_uint32), ("datagram_max_size", ctypes.c_uint32),
                ("frames_per_second", ctypes.c_uint32), ("buffered_frames", ctypes.c_uint32),
                ("stream_length_frames", ctypes.c_int64)]


class Stats(ctypes.Structure):
    _fields_ = [("bits_received", ctypes.c_int64), ("successful_frames", ctypes.c_int64),
                ("dropped_frames", ctypes.c_int64), ("duplicate_frames", ctypes.c_int64),
                ("error_frames", ctypes.c_int64), ("datagrams", ctypes.c_uint64), ("last_error", ctypes.c_uint32),
                ("finished", ctypes.c_uint32), ("head_sequence_number", ctypes.c_int64),
                ("fail_datagram", ctypes.c_uint32), ("has_failure", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


class FrameWindow(ctypes.Structure):
    """cts_frame_window: the client's jitter window a batch is summed for."""

    _fields_ = [("head_sequence_number", ctypes.c_int64), ("final_frame", ctypes.c_int64),
                ("frames", ctypes.c_uint32), ("finished", ctypes.c_uint32)]


class FrameTotals(ctypes.Structure):
    """cts_frame_totals: a batch's sums, folded from the device block."""

    _fields_ = [("bits_received", ctypes.c_uint64), ("error_frames", ctypes.c_uint64), ("datagrams", ctypes.c_uint64),
                ("first_exception", ctypes.c_uint32), ("exceptions", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


FRAMES_REPLAY = 16  # CTS_MS_FRAMES_REPLAY
NO_EXCEPTION = 0xFFFFFFFF


class UdpStatusDetails(ctypes.Structure):
    """cts_udp_status_details: the process-wide UdpStatusDetails (ctsConfig.h:417)."""

    _fields_ = [(f, ctypes.c_int64) for f in ("bits_received", "successful_frames", "dropped_frames",
                                               "duplicate_frames", "error_frames")]


def declare(L: ctypes.CDLL) -> None:
    P = ctypes.c_void_p
    u32, u64, i32, i64 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_int64
    sigs = {
        "cts_media_stream_split": ([u64, u32, P, u64], u64),
        "cts_media_stream_fill": ([P, P, u64, P, P, u32, P], i32),
        "cts_media_stream_fill_strided": ([P, P, u64, u32, P, P, u32, P], i32),
        "cts_media_stream_verify": ([P, P, u64, P, u32, P, P, P, P], i32),
        "cts_media_stream_verify_strided": ([P, P, u64, u32, P, u32, P, P, P, P], i32),
        "cts_media_stream_verify_status": ([P, P, u64, P, u32, P, P, P], i32),
        "cts_media_stream_verify_strided_status": ([P, P, u64, u32, P, u32, P, P, P], i32),
        "cts_media_stream_client_complete_status": ([P, P, u32, i64, i64, ctypes.POINTER(u32)], i32),
        "cts_media_stream_client_create": ([ctypes.POINTER(Settings), ctypes.POINTER(P)], i32),
        "cts_media_stream_client_destroy": ([P], i32),
        "cts_media_stream_client_complete": ([P, P, P, u32, i64, i64, ctypes.POINTER(u32)], i32),
        "cts_media_stream_client_set_connection_id": ([P, ctypes.c_char_p, u32], i32),
        "cts_media_stream_client_render": ([P], i32),
        "cts_media_stream_client_stats": ([P, ctypes.POINTER(Stats)], i32),
        "cts_media_stream_client_connection_id": ([P], ctypes.c_char_p),
        "cts_frame_totals_device_bytes": ([], ctypes.c_size_t),
        "cts_frame_totals_fold": ([P, ctypes.POINTER(FrameTotals)], i32),
        "cts_media_stream_verify_frames": ([P, P, u64, P, u32, ctypes.POINTER(FrameWindow), P, P, P, P], i32),
        "cts_media_stream_verify_strided_frames": ([P, P, u64, u32, P, u32, ctypes.POINTER(FrameWindow), P, P, P, P],
                                                   i32),
        "cts_media_stream_client_window": ([P, ctypes.POINTER(FrameWindow)], i32),
        "cts_media_stream_client_complete_frames": ([P, ctypes.POINTER(FrameWindow), ctypes.POINTER(FrameTotals), P,
                                                     u32, i64, i64], i32),
        "cts_udp_status_details_read": ([ctypes.POINTER(UdpStatusDetails)], i32),
        "cts_udp_status_details_reset": ([], None),
    }
    for name, (argtypes, restype) in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = argtypes
        fn.restype = restype


def udp_status_details() -> dict:
    """The process-wide UDP counters every MediaStreamClient feeds (cts_udp_status_details_read)."""
    s = UdpStatusDetails()
    check("cts_udp_status_details_read", lib().cts_udp_status_details_read(ctypes.byref(s)))
    return {f: int(getattr(s, f)) for f, _ in s._fields_}


def udp_status_details_reset() -> None:
    lib().cts_udp_status_details_reset()


def split(frame_bytes: int, max_datagram: int) -> np.ndarray:
    """Total lengths (26-byte header included) of the datagrams one frame is sent as."""
    n = int(lib().cts_media_stream_split(frame_bytes, max_datagram, None, 0))
    out = np.zeros(n, dtype=np.uint32)
    if n:
        lib().cts_media_stream_split(frame_bytes, max_datagram, out.ctypes.data, n)
    return out


def _ptr(x):
    from .engine import _ptr as p

    return p(x)


def fill(engine, arena, descs, headers, stream=None) -> None:
    """cts_media_stream_fill: descs (uint8 device tensor of DESC_DTYPE), headers (uint8 device tensor of
    DGRAM_HEADER_DTYPE)."""
    from .engine import _nbytes, _stream

    n = _nbytes(descs) // DESC_DTYPE.itemsize
    if _nbytes(headers) < n * DGRAM_HEADER_DTYPE.itemsize:
        raise ValueError("headers holds %d bytes, %d datagrams need %d" % (_nbytes(headers), n,
                                                                          n * DGRAM_HEADER_DTYPE.itemsize))
    check("cts_media_stream_fill", engine._L.cts_media_stream_fill(engine._h, _ptr(arena), _nbytes(arena), _ptr(descs),
                                                               _ptr(headers), n, _stream(stream)))


def fill_strided(engine, arena, stride: int, lengths, headers, stream=None) -> None:
    """cts_media_stream_fill_strided: datagram i at arena + i * stride, lengths (uint32 device tensor) its bytes,
    headers (uint8 device tensor of DGRAM_HEADER_DTYPE) its header values."""
    from .engine import _nbytes, _stream

    n = _nbytes(lengths) // 4
    if _nbytes(headers) < n * DGRAM_HEADER_DTYPE.itemsize:
        raise ValueError("headers holds %d bytes, %d datagrams need %d" % (_nbytes(headers), n,
                                                                          n * DGRAM_HEADER_DTYPE.itemsize))
    check("cts_media_stream_fill_strided",
          engine._L.cts_media_stream_fill_strided(engine._h, _ptr(arena), _nbytes(arena), stride, _ptr(lengths),
                                                  _ptr(headers), n, _stream(stream)))


def verify(engine, arena, descs, records=None, results=None, counters=None, stream=None) -> None:
    from .engine import _check_outputs, _nbytes, _stream

    n = _nbytes(descs) // DESC_DTYPE.itemsize
    _check_outputs(n, results, counters)
    if records is not None and _nbytes(records) < n * DGRAM_RECORD_DTYPE.itemsize:
        raise ValueError("records holds %d bytes, %d datagrams need %d" % (_nbytes(records), n,
                                                                          n * DGRAM_RECORD_DTYPE.itemsize))
    check("cts_media_stream_verify",
          engine._L.cts_media_stream_verify(engine._h, _ptr(arena), _nbytes(arena), _ptr(descs), n, _ptr(records),
                                        _ptr(results), _ptr(counters), _stream(stream)))


def verify_strided(engine, arena, stride: int, lengths, records=None, results=None, counters=None,
                   stream=None) -> None:
    """cts_media_stream_verify_strided: datagram i at arena + i * stride, lengths (uint32 device tensor) its
    completed bytes."""
    from .engine import _check_outputs, _nbytes, _stream

    n = _nbytes(lengths) // 4
    _check_outputs(n, results, counters)
    if records is not None and _nbytes(records) < n * DGRAM_RECORD_DTYPE.itemsize:
        raise ValueError("records holds %d bytes, %d datagrams need %d" % (_nbytes(records), n,
                                                                          n * DGRAM_RECORD_DTYPE.itemsize))
    check("cts_media_stream_verify_strided",
          engine._L.cts_media_stream_verify_strided(engine._h, _ptr(arena), _nbytes(arena), stride, _ptr(lengths), n,
                                                _ptr(records), _ptr(results), _ptr(counters), _stream(stream)))


def _check_status(n, status):
    from .engine import _nbytes

    if status is not None and _nbytes(status) < n * DGRAM_STATUS_DTYPE.itemsize:
        raise ValueError("status holds %d bytes, %d datagrams need %d" % (_nbytes(status), n,
                                                                         n * DGRAM_STATUS_DTYPE.itemsize))


def verify_status(engine, arena, descs, status=None, counters=None, stream=None) -> None:
    """cts_media_stream_verify_status: the receive pass writing one 16-byte cts_datagram_status per datagram."""
    from .engine import _check_outputs, _nbytes, _stream

    n = _nbytes(descs) // DESC_DTYPE.itemsize
    _check_outputs(n, None, counters)
    _check_status(n, status)
    check("cts_media_stream_verify_status",
          engine._L.cts_media_stream_verify_status(engine._h, _ptr(arena), _nbytes(arena), _ptr(descs), n, _ptr(status),
                                                   _ptr(counters), _stream(stream)))


def verify_strided_status(engine, arena, stride: int, lengths, status=None, counters=None, stream=None) -> None:
    """cts_media_stream_verify_strided_status: the strided receive ring, 16-byte statuses."""
    from .engine import _check_outputs, _nbytes, _stream

    n = _nbytes(lengths) // 4
    _check_outputs(n, None, counters)
    _check_status(n, status)
    check("cts_media_stream_verify_strided_status",
          engine._L.cts_media_stream_verify_strided_status(engine._h, _ptr(arena), _nbytes(arena), stride,
                                                           _ptr(lengths), n, _ptr(status), _ptr(counters),
                                                           _stream(stream)))


class FrameSums:
    """Device outputs of one cts_media_stream_verify_frames launch: the totals block and bytes per window slot."""

    def __init__(self, window_frames: int, device="cuda"):
        import torch

        self.totals = torch.zeros(int(lib().cts_frame_totals_device_bytes()), dtype=torch.uint8, device=device)
        self.frame_bytes = torch.zeros(max(1, window_frames), dtype=torch.int64, device=device)

    def read(self):
        """(FrameTotals folded on the host, frame_bytes as uint64 numpy)."""
        t = FrameTotals()
        host = np.ascontiguousarray(self.totals.cpu().numpy())
        check("cts_frame_totals_fold", lib().cts_frame_totals_fold(host.ctypes.data, ctypes.byref(t)))
        return t, self.frame_bytes.cpu().numpy().view(np.uint64)


def verify_frames(engine, arena, descs, window: FrameWindow, sums: FrameSums, counters=None, stream=None) -> None:
    """cts_media_stream_verify_frames: the receive pass summing the client's frame accounting for `window`."""
    from .engine import _check_outputs, _nbytes, _stream

    n = _nbytes(descs) // DESC_DTYPE.itemsize
    _check_outputs(n, None, counters)
    if sums.frame_bytes.numel() < window.frames:
        raise ValueError("frame_bytes holds %d slots, the window %d" % (sums.frame_bytes.numel(), window.frames))
    check("cts_media_stream_verify_frames",
          engine._L.cts_media_stream_verify_frames(engine._h, _ptr(arena), _nbytes(arena), _ptr(descs), n,
                                                   ctypes.byref(window), _ptr(sums.totals), _ptr(sums.frame_bytes),
                                                   _ptr(counters), _stream(stream)))


def verify_strided_frames(engine, arena, stride: int, lengths, window: FrameWindow, sums: FrameSums, counters=None,
                          stream=None) -> None:
    """cts_media_stream_verify_strided_frames: the same over a strided receive ring."""
    from .engine import _check_outputs, _nbytes, _stream

    n = _nbytes(lengths) // 4
    _check_outputs(n, None, counters)
    if sums.frame_bytes.numel() < window.frames:
        raise ValueError("frame_bytes holds %d slots, the window %d" % (sums.frame_bytes.numel(), window.frames))
    check("cts_media_stream_verify_strided_frames",
          engine._L.cts_media_stream_verify_strided_frames(engine._h, _ptr(arena), _nbytes(arena), stride,
                                                           _ptr(lengths), n, ctypes.byref(window), _ptr(sums.totals),
                                                           _ptr(sums.frame_bytes), _ptr(counters), _stream(stream)))


class MediaStreamClient:
    """ctsIoPatternMediaStreamClient's frame accounting (ctsIOPatternMediaStream.cpp:46-530)."""

    def __init__(self, frame_size_bytes: int, buffered_frames: int, stream_length_frames: int,
                 datagram_max_size: int = 1400, frames_per_second: int = 60):
        self._s = Settings(frame_size_bytes, datagram_max_size, frames_per_second, buffered_frames,
                           stream_length_frames)
        h = ctypes.c_void_p()
        check("cts_media_stream_client_create", lib().cts_media_stream_client_create(ctypes.byref(self._s),
                                                                                       ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().cts_media_stream_client_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def complete(self, records: np.ndarray, results: np.ndarray, receiver_qpc: int = 0, receiver_qpf: int = 0):
        """Returns (cts_io_status, consumed)."""
        records = np.ascontiguousarray(records, dtype=DGRAM_RECORD_DTYPE)
        results = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        if len(records) != len(results):
            raise ValueError("%d records but %d results" % (len(records), len(results)))
        consumed = ctypes.c_uint32()
        rc = lib().cts_media_stream_client_complete(self._h, records.ctypes.data, results.ctypes.data, len(records),
                                                    receiver_qpc, receiver_qpf, ctypes.byref(consumed))
        if rc < 0:
            raise CtsError("cts_media_stream_client_complete", rc)
        return rc, consumed.value

    def complete_status(self, status: np.ndarray, receiver_qpc: int = 0, receiver_qpf: int = 0):
        """CompleteIo over compact statuses (cts_media_stream_client_complete_status). Returns (cts_io_status,
        consumed)."""
        status = np.ascontiguousarray(status, dtype=DGRAM_STATUS_DTYPE)
        consumed = ctypes.c_uint32()
        rc = lib().cts_media_stream_client_complete_status(self._h, status.ctypes.data, len(status), receiver_qpc,
                                                           receiver_qpf, ctypes.byref(consumed))
        if rc < 0:
            raise CtsError("cts_media_stream_client_complete_status", rc)
        return rc, consumed.value

    def window(self) -> FrameWindow:
        w = FrameWindow()
        check("cts_media_stream_client_window", lib().cts_media_stream_client_window(self._h, ctypes.byref(w)))
        return w

    def complete_frames(self, window: FrameWindow, totals: FrameTotals, frame_bytes: np.ndarray, n: int,
                        receiver_qpc: int = 0, receiver_qpf: int = 0) -> int:
        """CompleteIo of a batch of n datagrams from its GPU sums. Returns a cts_io_status, or FRAMES_REPLAY when
        the batch holds an exception (nothing applied)."""
        fb = np.ascontiguousarray(frame_bytes, dtype=np.uint64)
        rc = lib().cts_media_stream_client_complete_frames(self._h, ctypes.byref(window), ctypes.byref(totals),
                                                           fb.ctypes.data, n, receiver_qpc, receiver_qpf)
        if rc < 0:
            raise CtsError("cts_media_stream_client_complete_frames", rc)
        return rc

    def complete_batch_on_gpu(self, engine, arena, descs, sums: "FrameSums" = None, status=None, receiver_qpc: int = 0,
                              receiver_qpf: int = 0):
        """One batch through the GPU sums, replayed datagram by datagram from compact statuses when it holds an
        exception. Returns (cts_io_status, replayed)."""
        import torch

        from .engine import _nbytes

        n = _nbytes(descs) // DESC_DTYPE.itemsize
        w = self.window()
        sums = sums or FrameSums(w.frames, device=arena.device)
        verify_frames(engine, arena, descs, w, sums)
        torch.cuda.synchronize(arena.device)
        t, fb = sums.read()
        rc = self.complete_frames(w, t, fb, n, receiver_qpc, receiver_qpf)
        if rc != FRAMES_REPLAY:
            return rc, False
        st = status if status is not None else torch.empty(n * DGRAM_STATUS_DTYPE.itemsize, dtype=torch.uint8,
                                                           device=arena.device)
        verify_status(engine, arena, descs, status=st)
        torch.cuda.synchronize(arena.device)
        rc, _ = self.complete_status(st[: n * DGRAM_STATUS_DTYPE.itemsize].cpu().numpy().view(DGRAM_STATUS_DTYPE),
                                     receiver_qpc, receiver_qpf)
        return rc, True

    def set_connection_id(self, datagram: bytes) -> None:
        check("cts_media_stream_client_set_connection_id",
              lib().cts_media_stream_client_set_connection_id(self._h, datagram, len(datagram)))

    def render(self) -> int:
        rc = lib().cts_media_stream_client_render(self._h)
        if rc < 0:
            raise CtsError("cts_media_stream_client_render", rc)
        return rc

    def stats(self) -> dict:
        s = Stats()
        check("cts_media_stream_client_stats", lib().cts_media_stream_client_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def connection_id(self) -> str:
        return lib().cts_media_stream_client_connection_id(self._h).decode()


# ---- MediaStream connections on the device-resident path (include/cts_media_stream_conns.h) ---------------------
def conn_init(frame_size_bytes: int, buffered_frames: int, stream_length_frames: int, frame_base: int = 0,
              datagram_max_size: int = 1400, frames_per_second: int = 60) -> np.ndarray:
    """cts_ms_conn_init: a fresh cts_ms_conn_state (one MS_CONN_STATE_DTYPE record) for a client with these settings,
    its ring at frame_base. Raises CtsError where cts_media_stream_client_create would refuse the settings."""
    from .types import MS_CONN_STATE_DTYPE

    s = Settings(frame_size_bytes, datagram_max_size, frames_per_second, buffered_frames, stream_length_frames)
    out = np.zeros(1, dtype=MS_CONN_STATE_DTYPE)
    check("cts_ms_conn_init", lib().cts_ms_conn_init(ctypes.addressof(s), frame_base, out.ctypes.data))
    return out[0]


class ConnectionTable:
    """Many MediaStream clients on one device: the entry table, the rings, the first-failure slots and the UDP block,
    with the per-batch passes, the render tick and the close as methods.

    settings: (frame_size_bytes, buffered_frames, stream_length_frames) per connection slot. Per batch call
    :meth:`verify` then :meth:`accumulate` with the batch's base_index (its first stream ordinal), :meth:`render` at a
    tick, :meth:`close` to report and recycle slots, :meth:`reinit` before a slot's next connection."""

    def __init__(self, engine, settings, device=None):
        import torch

        from .types import MS_CONN_STATE_DTYPE

        self.engine = engine
        self.device = device or "cuda:%d" % engine.device
        self.fresh = np.zeros(len(settings), dtype=MS_CONN_STATE_DTYPE)
        base = 0
        for c, (frame_size, buffered, length) in enumerate(settings):
            self.fresh[c] = conn_init(frame_size, buffered, length, frame_base=base)
            base += int(self.fresh[c]["frames"])
        self.n_conns, self.frame_elems = len(settings), base
        self.conns = torch.from_numpy(self.fresh.view(np.int64).copy()).to(self.device)
        self.frame_bytes = torch.zeros(max(1, base), dtype=torch.int64, device=self.device)
        self.slots = torch.full((max(1, self.n_conns),), -1, dtype=torch.int32, device=self.device)[: self.n_conns]
        self.udp = engine.new_counters()

    def verify(self, arena, descs, base_index: int = 0, status=None, counters=None, stream=None) -> None:
        """cts_media_stream_verify_status_at: the receive pass; lowers the slots of connections with an exception."""
        from .engine import _check_outputs, _nbytes, _stream

        n = _nbytes(descs) // DESC_DTYPE.itemsize
        _check_outputs(n, None, counters)
        _check_status(n, status)
        check("cts_media_stream_verify_status_at",
              self.engine._L.cts_media_stream_verify_status_at(
                  self.engine._h, _ptr(arena), _nbytes(arena), _ptr(descs), n, base_index, _ptr(status),
                  _ptr(counters), _ptr(self.slots), self.n_conns, _stream(stream)))

    def accumulate(self, arena_bytes: int, descs, status, base_index: int = 0, stream=None) -> None:
        """cts_media_stream_conns_accumulate: the accounting pass over the batch's descriptors and statuses."""
        from .engine import _nbytes, _stream

        n = _nbytes(descs) // DESC_DTYPE.itemsize
        if status is None:
            raise ValueError("the accounting pass reads the batch's statuses")
        _check_status(n, status)
        check("cts_media_stream_conns_accumulate",
              self.engine._L.cts_media_stream_conns_accumulate(
                  self.engine._h, arena_bytes, _ptr(descs), _ptr(status), n, base_index, _ptr(self.slots),
                  _ptr(self.conns), _ptr(self.frame_bytes), self.frame_elems, self.n_conns, _ptr(self.udp),
                  _stream(stream)))

    def render(self, conn_ids, codes=None, stream=None) -> None:
        """cts_media_stream_conns_render: one tick of conn_ids (uint32/int32 device tensor, distinct); codes: None or
        an int32 device tensor of as many elements."""
        from .engine import _nbytes, _stream

        n = _nbytes(conn_ids) // 4
        if codes is not None and _nbytes(codes) < 4 * n:
            raise ValueError("codes holds %d bytes, %d ids need %d" % (_nbytes(codes), n, 4 * n))
        check("cts_media_stream_conns_render",
              self.engine._L.cts_media_stream_conns_render(self.engine._h, _ptr(conn_ids), n, _ptr(self.conns),
                                                           _ptr(self.frame_bytes), self.n_conns, _ptr(self.udp),
                                                           _ptr(codes), _stream(stream)))

    def close(self, conn_ids, close_counters, results=None, stream=None) -> None:
        """cts_media_stream_conns_close: results None or 88 bytes per id (MS_CONN_RESULT_DTYPE)."""
        from .engine import _check_outputs, _nbytes, _stream
        from .types import MS_CONN_RESULT_DTYPE

        n = _nbytes(conn_ids) // 4
        _check_outputs(0, None, close_counters)
        if results is not None and _nbytes(results) < n * MS_CONN_RESULT_DTYPE.itemsize:
            raise ValueError("results holds %d bytes, %d ids need %d" % (_nbytes(results), n,
                                                                         n * MS_CONN_RESULT_DTYPE.itemsize))
        check("cts_media_stream_conns_close",
              self.engine._L.cts_media_stream_conns_close(self.engine._h, _ptr(conn_ids), n, _ptr(self.slots),
                                                          _ptr(self.conns), _ptr(self.frame_bytes), self.n_conns,
                                                          _ptr(results), _ptr(close_counters), _stream(stream)))

    def new_results(self, n: int):
        import torch

        from .types import MS_CONN_RESULT_DTYPE

        return torch.zeros(n * (MS_CONN_RESULT_DTYPE.itemsize // 8), dtype=torch.int64, device=self.device)

    def reinit(self, conn_ids) -> None:
        """Fresh entries over the listed slots (host ids): the slots' next connections, same settings."""
        import torch

        words = self.fresh.dtype.itemsize // 8
        view = self.conns.view(-1, words)
        ids = torch.as_tensor(list(conn_ids), dtype=torch.int64, device=self.device)
        view[ids] = torch.from_numpy(self.fresh.view(np.int64).reshape(-1, words).copy()).to(self.device)[ids]

    def read(self):
        """(entries MS_CONN_STATE_DTYPE, ring uint64, slots uint32) copied to the host."""
        return (self.conns.cpu().numpy().view(self.fresh.dtype), self.frame_bytes.cpu().numpy().view(np.uint64)
                [: self.frame_elems], self.slots.cpu().numpy().view(np.uint32))

    def read_udp(self, stream=None) -> dict:
        return self.engine.read_counters_udp(self.udp, stream=stream)


# ---- MediaStream servers on the device-resident path (include/cts_media_stream_servers.h) ------------------------
def server_init(frame_size_bytes: int, datagram_max_size: int, stream_length_frames: int,
                frames_per_second: int = 60) -> np.ndarray:
    """cts_ms_server_init: a fresh cts_ms_server_state (one MS_SERVER_STATE_DTYPE record) for a server with these
    settings. Raises CtsError where the settings are refused (a frame of at most 26 bytes, a datagram_max_size below
    53: the device's own rule)."""
    from .types import MS_SERVER_STATE_DTYPE

    s = Settings(frame_size_bytes, datagram_max_size, frames_per_second, 0, stream_length_frames)
    out = np.zeros(1, dtype=MS_SERVER_STATE_DTYPE)
    check("cts_ms_server_init", lib().cts_ms_server_init(ctypes.addressof(s), out.ctypes.data))
    return out[0]


def servers_scratch_bytes(n: int) -> int:
    """cts_media_stream_servers_scratch_bytes: the scratch a tick over n listed connections needs."""
    return int(lib().cts_media_stream_servers_scratch_bytes(n))


def servers_send(engine, arena, stride: int, first_slot: int, capacity: int, conn_ids, servers, n_conns: int, qpc: int,
                 qpf: int, scratch, descs=None, lengths=None, codes=None, tick=None, udp_counters=None, stream=None,
                 n: int = None, arena_bytes: int = None, scratch_bytes: int = None) -> None:
    """cts_media_stream_servers_send: one tick of the connections conn_ids (uint32/int32 device tensor, distinct) into
    slots first_slot .. of arena. descs (24 bytes per slot of the capacity), lengths, codes (4 bytes each), tick (32
    bytes) and udp_counters are device tensors or None. Raises CtsError(CTS_E_INVALID) for a refused argument."""
    from .engine import _nbytes, _stream

    n = _nbytes(conn_ids) // 4 if n is None else n
    check("cts_media_stream_servers_send",
          engine._L.cts_media_stream_servers_send(
              engine._h, _ptr(arena), _nbytes(arena) if arena_bytes is None else arena_bytes, stride, first_slot,
              capacity, _ptr(conn_ids), n, _ptr(servers), n_conns, qpc, qpf, _ptr(descs), _ptr(lengths), _ptr(codes),
              _ptr(tick), _ptr(udp_counters), _ptr(scratch),
              _nbytes(scratch) if scratch_bytes is None else scratch_bytes, _stream(stream)))


def server_schedule_init(frames_per_second: int, base_time_ms: int) -> np.ndarray:
    """cts_ms_server_schedule_init: a schedule entry (one MS_SERVER_SCHEDULE_DTYPE record) for a server of this frame
    rate whose frame 0 is due at base_time_ms. Raises CtsError for frames_per_second == 0 or a base outside
    [0, 2^62)."""
    from .types import MS_SERVER_SCHEDULE_DTYPE

    s = Settings(0, 0, frames_per_second, 0, 0)
    out = np.zeros(1, dtype=MS_SERVER_SCHEDULE_DTYPE)
    check("cts_ms_server_schedule_init",
          lib().cts_ms_server_schedule_init(ctypes.addressof(s), base_time_ms, out.ctypes.data))
    return out[0]


def server_frames_due(state, schedule, now_ms: int, max_frames: int):
    """cts_ms_server_frames_due: (frames, next_due_ms) of one entry and its schedule entry (records of
    MS_SERVER_STATE_DTYPE and MS_SERVER_SCHEDULE_DTYPE) at now_ms: the closed form on the host."""
    from .types import MS_SERVER_SCHEDULE_DTYPE, MS_SERVER_STATE_DTYPE

    e = np.array([state], dtype=MS_SERVER_STATE_DTYPE)
    q = np.array([schedule], dtype=MS_SERVER_SCHEDULE_DTYPE)
    frames, due = ctypes.c_uint32(0), ctypes.c_int64(0)
    check("cts_ms_server_frames_due",
          lib().cts_ms_server_frames_due(e.ctypes.data, q.ctypes.data, now_ms, max_frames, ctypes.byref(frames),
                                         ctypes.byref(due)))
    return int(frames.value), int(due.value)


def servers_timed_scratch_bytes(n: int) -> int:
    """cts_media_stream_servers_timed_scratch_bytes: the scratch a timed tick over n listed connections needs."""
    return int(lib().cts_media_stream_servers_timed_scratch_bytes(n))


def servers_send_at(engine, arena, stride: int, first_slot: int, capacity: int, conn_ids, servers, schedule,
                    n_conns: int, max_frames: int, now_ms: int, qpc: int, qpf: int, scratch, descs=None, lengths=None,
                    codes=None, tick=None, udp_counters=None, stream=None, n: int = None, arena_bytes: int = None,
                    scratch_bytes: int = None) -> None:
    """cts_media_stream_servers_send_at: one timed tick of the connections conn_ids at now_ms, at most max_frames
    frames of each. servers_send's arguments, and schedule (16 bytes per connection slot, a device tensor); tick is 48
    bytes. Raises CtsError(CTS_E_INVALID) for a refused argument."""
    from .engine import _nbytes, _stream

    n = _nbytes(conn_ids) // 4 if n is None else n
    check("cts_media_stream_servers_send_at",
          engine._L.cts_media_stream_servers_send_at(
              engine._h, _ptr(arena), _nbytes(arena) if arena_bytes is None else arena_bytes, stride, first_slot,
              capacity, _ptr(conn_ids), n, _ptr(servers), _ptr(schedule), n_conns, max_frames, now_ms, qpc, qpf,
              _ptr(descs), _ptr(lengths), _ptr(codes), _ptr(tick), _ptr(udp_counters), _ptr(scratch),
              _nbytes(scratch) if scratch_bytes is None else scratch_bytes, _stream(stream)))


class ServerTable:
    """Many MediaStream servers on one device: the entry table, a tick's scratch, the datagram ring with its
    descriptors and lengths, the codes, the tick block and the UDP block, with the tick as a method.

    settings: (frame_size_bytes, datagram_max_size, stream_length_frames) per connection slot. The ring holds
    ring_slots slots of stride bytes (pre-filled with `fill`), a tick writes at most capacity of them from first_slot
    on. :meth:`send` is one frame of the listed connections; ``descs_of(n)`` is the descriptor array of the tick's
    first n datagrams for :meth:`ConnectionTable.verify` and :meth:`ConnectionTable.accumulate`, with n computed from
    the settings (``datagrams_per_tick``): nothing is read back between the send and the receive pass.

    schedule: (frames_per_second, base_time_ms) per connection slot (see :meth:`set_schedule`). With it
    :meth:`send_at` is the tick by the clock: the frames of the listed connections that are due at now_ms."""

    def __init__(self, engine, settings, stride: int, capacity: int, ring_slots: int = None, device=None,
                 fill: int = 0, max_listed: int = None, schedule=None):
        import torch

        from .types import MS_SERVER_STATE_DTYPE, MS_SERVER_TICK_DTYPE

        self.engine = engine
        self.device = device or "cuda:%d" % engine.device
        self.fresh = np.zeros(len(settings), dtype=MS_SERVER_STATE_DTYPE)
        for c, (frame_size, datagram_max, length) in enumerate(settings):
            self.fresh[c] = server_init(frame_size, datagram_max, length)
        self.n_conns, self.stride, self.capacity = len(settings), stride, capacity
        self.ring_slots = capacity if ring_slots is None else ring_slots
        words = max(1, self.n_conns) * (MS_SERVER_STATE_DTYPE.itemsize // 8)
        self.servers = torch.zeros(words, dtype=torch.int64, device=self.device)
        if self.n_conns:
            self.servers.copy_(torch.from_numpy(self.fresh.view(np.int64).copy()))
        self.max_listed = max(1, self.n_conns if max_listed is None else max_listed)
        self.scratch = torch.zeros((servers_scratch_bytes(self.max_listed) + 7) // 8, dtype=torch.int64,
                                   device=self.device)
        self.ring = torch.full((max(16, self.ring_slots * stride),), fill, dtype=torch.uint8, device=self.device)
        self.descs = torch.zeros(max(1, capacity) * (DESC_DTYPE.itemsize // 8), dtype=torch.int64, device=self.device)
        self.lengths = torch.zeros(max(1, capacity), dtype=torch.int32, device=self.device)
        self.codes = torch.zeros(self.max_listed, dtype=torch.int32, device=self.device)
        self.tick = torch.zeros(MS_SERVER_TICK_DTYPE.itemsize // 8, dtype=torch.int64, device=self.device)
        self.udp = engine.new_counters()
        # the frame schedule (set_schedule) and what send_at needs beside it; the plain tick reads none of them
        self.schedule = self.timed_scratch = self.timed_tick = None
        if schedule is not None:
            self.set_schedule(schedule)

    def set_schedule(self, schedule) -> None:
        """The table's frame schedule: (frames_per_second, base_time_ms) per connection slot, or an
        MS_SERVER_SCHEDULE_DTYPE array of n_conns records written as it is (a test's preset). Needed before
        :meth:`send_at`; the host may write it again at any time between ticks, no tick writes it."""
        import torch

        from .types import MS_SERVER_SCHEDULE_DTYPE, MS_SERVER_TIMED_TICK_DTYPE

        if isinstance(schedule, np.ndarray) and schedule.dtype == MS_SERVER_SCHEDULE_DTYPE:
            q = np.ascontiguousarray(schedule)
        else:
            q = np.zeros(len(schedule), dtype=MS_SERVER_SCHEDULE_DTYPE)
            for c, (fps, base) in enumerate(schedule):
                q[c] = server_schedule_init(fps, base)
        if len(q) != self.n_conns:
            raise ValueError("%d schedule entries for a table of %d" % (len(q), self.n_conns))
        words = max(1, self.n_conns) * (MS_SERVER_SCHEDULE_DTYPE.itemsize // 8)
        self.schedule = torch.zeros(words, dtype=torch.int64, device=self.device)
        if self.n_conns:
            self.schedule.copy_(torch.from_numpy(q.view(np.int64).copy()))
        if self.timed_scratch is None:
            self.timed_scratch = torch.zeros((servers_timed_scratch_bytes(self.max_listed) + 7) // 8,
                                             dtype=torch.int64, device=self.device)
            self.timed_tick = torch.zeros(MS_SERVER_TIMED_TICK_DTYPE.itemsize // 8, dtype=torch.int64,
                                          device=self.device)

    def send_at(self, conn_ids, now_ms: int, max_frames: int, qpc: int, qpf: int, first_slot: int = 0,
                stream=None) -> None:
        """One timed tick of conn_ids (uint32/int32 device tensor, distinct, at most max_listed of them): the frames
        the schedule releases at now_ms, at most max_frames of each connection. :meth:`read_timed` has the tick block;
        the codes, ring, descriptors, lengths and UDP block are the plain tick's arrays."""
        from .engine import _nbytes

        if self.schedule is None:
            raise ValueError("send_at needs the table's schedule: set_schedule first")
        n = _nbytes(conn_ids) // 4
        if n > self.codes.numel():
            raise ValueError("%d ids listed, the table's codes and scratch hold %d" % (n, self.codes.numel()))
        servers_send_at(self.engine, self.ring, self.stride, first_slot, self.capacity, conn_ids, self.servers,
                        self.schedule, self.n_conns, max_frames, now_ms, qpc, qpf, self.timed_scratch,
                        descs=self.descs, lengths=self.lengths, codes=self.codes, tick=self.timed_tick,
                        udp_counters=self.udp, stream=stream)

    def read_timed(self):
        """(entries, codes uint32, tick: one MS_SERVER_TIMED_TICK_DTYPE record) copied to the host, after send_at."""
        from .types import MS_SERVER_TIMED_TICK_DTYPE

        return (self.servers.cpu().numpy().view(self.fresh.dtype)[: self.n_conns],
                self.codes.cpu().numpy().view(np.uint32),
                self.timed_tick.cpu().numpy().view(MS_SERVER_TIMED_TICK_DTYPE)[0])

    def datagrams_per_tick(self, conn_ids) -> int:
        """The datagrams one tick of these (host) ids writes while all of them run and fit: the receive pass's n."""
        return int(sum(int(self.fresh["datagrams_per_frame"][c]) for c in conn_ids))

    def send(self, conn_ids, qpc: int, qpf: int, first_slot: int = 0, stream=None) -> None:
        """One tick of conn_ids (uint32/int32 device tensor, distinct, at most max_listed of them)."""
        from .engine import _nbytes

        n = _nbytes(conn_ids) // 4
        if n > self.codes.numel():
            raise ValueError("%d ids listed, the table's codes and scratch hold %d" % (n, self.codes.numel()))
        servers_send(self.engine, self.ring, self.stride, first_slot, self.capacity, conn_ids, self.servers,
                     self.n_conns, qpc, qpf, self.scratch, descs=self.descs, lengths=self.lengths, codes=self.codes,
                     tick=self.tick, udp_counters=self.udp, stream=stream)

    def load(self, entries: np.ndarray) -> None:
        """Write entries (MS_SERVER_STATE_DTYPE[n_conns]) over the table: a stream resumed, or a test's preset."""
        import torch

        e = np.ascontiguousarray(entries, dtype=self.fresh.dtype)
        if len(e) != self.n_conns:
            raise ValueError("%d entries for a table of %d" % (len(e), self.n_conns))
        if self.n_conns:
            self.servers.copy_(torch.from_numpy(e.view(np.int64).copy()))

    def descs_of(self, n: int):
        """The descriptors of the last tick's first n datagrams (a view)."""
        return self.descs[: n * (DESC_DTYPE.itemsize // 8)]

    def read(self):
        """(entries MS_SERVER_STATE_DTYPE, codes uint32, tick: one MS_SERVER_TICK_DTYPE record) copied to the host."""
        from .types import MS_SERVER_TICK_DTYPE

        return (self.servers.cpu().numpy().view(self.fresh.dtype)[: self.n_conns],
                self.codes.cpu().numpy().view(np.uint32), self.tick.cpu().numpy().view(MS_SERVER_TICK_DTYPE)[0])

    def read_ring(self):
        """(ring bytes, descriptors DESC_DTYPE[capacity], lengths uint32[capacity]) copied to the host."""
        return (self.ring.cpu().numpy(), self.descs.cpu().numpy().view(DESC_DTYPE)[: self.capacity],
                self.lengths.cpu().numpy().view(np.uint32)[: self.capacity])

    def read_udp(self, stream=None) -> dict:
        return self.engine.read_counters_udp(self.udp, stream=stream)
