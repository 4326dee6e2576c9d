#!/usr/bin/env python3
"""tcp_sender_probe.py — what a device-planned TCP sender tick costs beside the host-fed fill.

Four shapes (--cases):

  4096x1      4 096 x 64 KiB (config 2's buffers), 4 096 connections, max_buffers 1
  128x32      4 096 x 64 KiB, 128 connections, max_buffers 32
  small       4 Mi x 1 472 B at stride 1 488, 1 024 connections of 4 096 buffers each
  65536x1     65 536 x 64 KiB, 65 536 connections of one buffer each

For each shape, alternated in this one process (baseline, tick, planning; --rounds times), HIP events around each call,
the median of --reps calls after --warmup, the arenas rotated so that no call finds its lines in the 256 MB Infinity
Cache (at least 1 GiB of arenas, and at least two):

  baseline    cts_fill over the same buffers with the descriptors already in device memory and the stride as the
              length hint (the yardstick: the host-fed form)
  tick        cts_tcp_senders_send, whole: three planning launches, the descriptor launch and the fill
  planning    the same call at capacity 0: the three planning launches with no slot to take, so no entry moves and
              neither the descriptor pass nor the fill is launched
  fill        tick - planning (derived, not measured alone; it holds the descriptor launch)

The expectation (stated, not a gate): fill within the spread of the baseline's own medians, the whole tick above the
baseline by about the planning time. One JSON line per shape goes to tcp_sender_probe.jsonl under --out (default
profiles/tcp_senders/) and to stdout.

  python tools/tcp_sender_probe.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# case: (connections, max_buffers, buffer size, stride)
SHAPES = {"4096x1": (4096, 1, 65536, 65536), "128x32": (128, 32, 65536, 65536), "small": (1024, 4096, 1472, 1488),
          "65536x1": (65536, 1, 65536, 65536)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="4096x1,128x32,small,65536x1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcp_senders"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from ctstraffic_amd import Engine
    from ctstraffic_amd import tcp_senders as T
    from ctstraffic_amd.types import DESC_DTYPE, TCP_SENDER_DTYPE, TCP_SENDER_TICK_DTYPE

    assert torch.cuda.is_available(), "tcp_sender_probe needs a GPU"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    os.makedirs(args.out, exist_ok=True)
    sink = open(os.path.join(args.out, "tcp_sender_probe.jsonl"), "w")

    def timed(launch):
        for i in range(args.warmup):
            launch(i)
        torch.cuda.synchronize()
        us = []
        for i in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(i)
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        return statistics.median(us)

    with Engine(0) as eng:
        for case in args.cases.split(","):
            n_conns, max_buffers, B, stride = SHAPES[case]
            n = n_conns * max_buffers
            arena_bytes = n * stride
            rot = max(2, -(-(1 << 30) // arena_bytes))
            arenas = [torch.empty(arena_bytes, dtype=torch.uint8, device=dev) for _ in range(rot)]
            descs = torch.zeros(n * (DESC_DTYPE.itemsize // 8), dtype=torch.int64, device=dev)
            tick = torch.zeros(TCP_SENDER_TICK_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
            # a transfer no call of this probe ends: every tick sends max_buffers full buffers per connection
            entries = np.empty(n_conns, dtype=TCP_SENDER_DTYPE)
            entries[:] = T.sender_init(1 << 60, B)
            senders = torch.from_numpy(entries.view(np.int64).copy()).to(dev)
            ids = torch.arange(n_conns, dtype=torch.int32, device=dev)
            scratch = torch.zeros((T.senders_scratch_bytes(n_conns) + 7) // 8, dtype=torch.int64, device=dev)
            sent = eng.new_counters()

            def send(i, capacity=n):
                T.senders_send(eng, arenas[i % rot], stride, 0, capacity, ids, max_buffers, senders, n_conns, descs,
                               scratch, tick=tick, sent_counters=sent)

            # the two paths write the same bytes: the tick's own descriptors fed to cts_fill
            send(0)
            host_descs = descs.clone()
            eng.fill(arenas[1], host_descs, max_length_hint=stride)
            torch.cuda.synchronize()
            t = tick.cpu().numpy().view(TCP_SENDER_TICK_DTYPE)[0]
            assert int(t["buffers"]) == n and int(t["connections_sent"]) == n_conns and int(t["bytes"]) == n * B, t
            step = (1 << 28) // stride * stride  # whole slots; the bytes behind a buffer in its slot are nobody's
            for o in range(0, arena_bytes, step):
                assert torch.equal(arenas[0][o:o + step].view(-1, stride)[:, :B],
                                   arenas[1][o:o + step].view(-1, stride)[:, :B]), (case, o)
            base, whole, plan = [], [], []
            for _ in range(args.rounds):
                base.append(timed(lambda i: eng.fill(arenas[i % rot], host_descs, max_length_hint=stride)))
                whole.append(timed(send))
                plan.append(timed(lambda i: send(i, capacity=0)))
            b, w, p = (statistics.median(x) for x in (base, whole, plan))
            margin = max(base) - min(base)
            line = dict(case=case, buffers=n, n_conns=n_conns, max_buffers=max_buffers, buffer_size=B, stride=stride,
                        arenas=rot, bytes=n * B, baseline_us=[round(x, 2) for x in base],
                        tick_us=[round(x, 2) for x in whole], planning_us=[round(x, 2) for x in plan],
                        baseline_median_us=round(b, 2), tick_median_us=round(w, 2), planning_median_us=round(p, 2),
                        fill_derived_us=round(w - p, 2), baseline_spread_us=round(margin, 2),
                        tick_over_baseline=round(w / b, 4), fill_within_spread=bool(w - p <= b + margin),
                        baseline_tbps=round(n * B / b / 1e6, 3), reps=args.reps, rounds=args.rounds)
            text = json.dumps(line)
            print(text, flush=True)
            sink.write(text + "\n")
            sink.flush()
            del arenas, descs, senders, ids, scratch, host_descs
            torch.cuda.empty_cache()
    sink.close()


if __name__ == "__main__":
    main()
