#!/usr/bin/env python3
"""ms_conn_probe.py — what the device-resident MediaStream connections cost on this GPU.

Config 3's datagrams (--n x 1472 B, default 16 Mi, one frame per datagram, 1 in 1024 corrupt) spread over 1, 1 024 and
65 536 connections, connection-major and interleaved (datagram i of connection i mod N). Every connection has a window
of 600 frames and its datagrams carry sequence numbers 1 + (k mod 600), so every clean datagram is booked to the ring:
the accounting pass's worst case, one ring add per datagram. HIP events around each launch, median / min / max over
--reps launches after --warmup, descriptors rotated over two copies. One JSON line per layout with

  rx_today      cts_media_stream_verify_status                 the receive pass as it was
  rx_ordinal    cts_media_stream_verify_status_at              the same with the slot claim of every exception
  refview_conns cts_refview_accumulate_conns                   the TCP per-connection pass over the same descriptors
  accounting    cts_media_stream_conns_accumulate              with empty slots (every datagram applied)
  accounting_stopped                                           with the slots the receive pass left (streams stopped at
                                                               their first exception: later datagrams only count)
  tick, close   cts_media_stream_conns_render / _close          of all N connections (the close net of the refill)
  today         N launches of cts_media_stream_verify_frames, each with its read-back, over the connection-major
                layout (at most --today-launches of them are run; the line says when the figure is extrapolated)

and the sum rx_ordinal + accounting + tick against `today`. Writes ms_conn_probe.jsonl under --out (default
profiles/ms_connections/) and prints the same lines.

  python tools/ms_conn_probe.py
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=16 * 1024 * 1024)
    ap.add_argument("--conns", default="1,1024,65536")
    ap.add_argument("--today-launches", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ms_connections"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from ctstraffic_amd import Engine
    from ctstraffic_amd import media_stream as M
    from ctstraffic_amd import workload as W
    from ctstraffic_amd.engine import descs_to_device
    from ctstraffic_amd.types import DGRAM_STATUS_DTYPE

    assert torch.cuda.is_available(), "ms_conn_probe needs a GPU"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    os.makedirs(args.out, exist_ok=True)
    sink = open(os.path.join(args.out, "ms_conn_probe.jsonl"), "w")

    def emit(**line):
        text = json.dumps(line)
        print(text, flush=True)
        sink.write(text + "\n")
        sink.flush()

    def timed(launch, reps=None):
        for i in range(args.warmup):
            launch(i)
        torch.cuda.synchronize()
        us = []
        for i in range(reps or args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(i)
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        return us

    def stats(us):
        return dict(us=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2))

    n, window = args.n, 600
    with Engine(0) as eng:
        w = W.udp_datagrams(n_datagrams=n)
        arena, _ = W.materialize(eng, w, device=dev)
        a2 = arena[: n * 1472].view(n, 1472)
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        for n_conns in (int(x) for x in args.conns.split(",")):
            per = n // n_conns
            table = M.ConnectionTable(eng, [(1472, window // 2, 1 << 30)] * n_conns)
            ids = torch.arange(n_conns, dtype=torch.int32, device=dev)
            fresh_conns, empty_slots = table.conns.clone(), table.slots.clone()
            for order in ("conn_major", "interleaved"):
                if n_conns == 1 and order == "interleaved":
                    continue
                conn = (np.arange(n) // per if order == "conn_major" else np.arange(n) % n_conns).astype(np.uint32)
                k = idx % per if order == "conn_major" else idx // n_conns
                a2[:, 2:10] = (1 + k % window).view(torch.uint8).view(n, 8)
                w.descs["conn_index"] = np.minimum(conn, n_conns - 1)
                dd = [descs_to_device(w.descs, dev) for _ in range(2)]
                sbuf = torch.zeros(n * DGRAM_STATUS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                ctr, ref = eng.new_counters(), eng.new_counters()
                state = eng.new_conn_state(n_conns)
                rx_today = timed(lambda i: M.verify_status(eng, arena, dd[i % 2], status=sbuf, counters=ctr))
                rx_ord = timed(lambda i: table.verify(arena, dd[i % 2], 1, status=sbuf, counters=ctr))
                stopped_slots = table.slots.clone()
                refc = timed(lambda i: eng.refview_conns(w.arena_bytes, dd[i % 2], ref, state, base_index=1,
                                                         conn_first_fail=stopped_slots))
                table.slots.copy_(empty_slots)
                table.conns.copy_(fresh_conns)
                table.frame_bytes.zero_()
                eng.reset_counters(table.udp)
                table.accumulate(w.arena_bytes, dd[0], sbuf, 1)
                torch.cuda.synchronize()
                entries, ring, _ = table.read()
                udp = table.read_udp()
                assert int(entries["datagrams"].sum()) == n == udp["datagrams"], udp
                assert int(ring.sum()) * 8 == udp["bits_received"] and udp["error_frames"] == 0, udp
                acc = timed(lambda i: table.accumulate(w.arena_bytes, dd[i % 2], sbuf, 1))
                table.slots.copy_(stopped_slots)
                acc_stopped = timed(lambda i: table.accumulate(w.arena_bytes, dd[i % 2], sbuf, 1))
                table.slots.copy_(empty_slots)
                tick = timed(lambda i: table.render(ids))
                blk, res = eng.new_counters(), table.new_results(n_conns)

                def close_refilled(i):
                    table.conns.copy_(fresh_conns)
                    table.close(ids, blk, results=res)

                both = timed(close_refilled)
                refill = timed(lambda i: table.conns.copy_(fresh_conns))
                line = dict(n=n, n_conns=n_conns, order=order, window_frames=window, rx_today=stats(rx_today),
                            rx_ordinal=stats(rx_ord), refview_conns=stats(refc), accounting=stats(acc),
                            accounting_stopped=stats(acc_stopped), tick=stats(tick),
                            close_us=round(statistics.median(both) - statistics.median(refill), 2),
                            rx_ordinal_over_today=round(statistics.median(rx_ord) / statistics.median(rx_today), 4),
                            accounting_over_refview_conns=round(statistics.median(acc) / statistics.median(refc), 3),
                            reps=args.reps)
                if order == "conn_major":
                    # today's path: one launch and one read-back per connection and batch
                    client = M.MediaStreamClient(1472, window // 2, 1 << 30)
                    win, sums = client.window(), M.FrameSums(window, device=dev)
                    launches = min(n_conns, args.today_launches)
                    step = per * DESC_BYTES

                    def today():
                        for c in range(launches):
                            M.verify_frames(eng, arena, dd[0][c * step:(c + 1) * step], win, sums, counters=ctr)
                            torch.cuda.synchronize()
                            sums.read()

                    today()
                    t0 = time.perf_counter()
                    today()
                    wall = (time.perf_counter() - t0) * 1e6 * (n_conns / launches)
                    ours = sum(statistics.median(x) for x in (rx_ord, acc, tick))
                    line.update(today_us=round(wall, 1), today_launches_run=launches,
                                today_extrapolated=bool(launches < n_conns), batch_us=round(ours, 1),
                                today_over_batch=round(wall / ours, 2))
                emit(**line)
                del dd, sbuf
            del table
    sink.close()


DESC_BYTES = 24

if __name__ == "__main__":
    main()
