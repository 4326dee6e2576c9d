#!/usr/bin/env python3
"""tcp_paced_sender_probe.py — what the paced TCP sender tick costs beside the plain one.

The four shapes of tools/tcp_sender_probe.py (--cases). For each, alternated in this one process (--rounds times), HIP
events around each call, the median of --reps calls after --warmup, the arenas rotated as there:

  plain          cts_tcp_senders_send, whole
  unpaced        cts_tcp_senders_send_paced over pace entries without a rate or a burst setting, whole
  half           cts_tcp_senders_send_paced with every connection rate-limited to half of max_buffers (at least one
                 buffer) per quantum, the clock one quantum further at every call: half the buffers, the pace loop run
                 by every lane
  plain_plan     the plain tick at capacity 0: its three planning launches alone
  unpaced_plan   the paced tick over unpaced entries at capacity 0

and, with --loop, the longest-lane loop: the planning alone (capacity 0) of 4 096 listed connections at max_buffers
700, unpaced (no loop), rate-limited with room for all 700 (700 steps without a division) and with a burst setting
above 700 (700 steps of the burst branch).

The expectation (stated, not a gate): unpaced_plan within plain_plan's spread plus the read of 64 B per listed
connection, and unpaced - unpaced_plan equal to plain - plain_plan. One JSON line per shape goes to
tcp_paced_sender_probe.jsonl under --out (default profiles/tcp_paced_senders/) and to stdout.

  python tools/tcp_paced_sender_probe.py --loop
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
PERIOD = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="4096x1,128x32,small,65536x1")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcp_paced_senders"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from ctstraffic_amd import Engine
    from ctstraffic_amd import tcp_senders as T
    from ctstraffic_amd.types import (DESC_DTYPE, TCP_SENDER_DTYPE, TCP_SENDER_PACE_DTYPE,
                                      TCP_SENDER_PACED_TICK_DTYPE)

    assert torch.cuda.is_available(), "tcp_paced_sender_probe needs a GPU"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    os.makedirs(args.out, exist_ok=True)
    sink = open(os.path.join(args.out, "tcp_paced_sender_probe.jsonl"), "w")
    clock = [0]

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

    def table(n_conns, B, **pace):
        entries = np.empty(n_conns, dtype=TCP_SENDER_DTYPE)
        entries[:] = T.sender_init(1 << 60, B)  # a transfer no call of this probe ends
        q = np.empty(n_conns, dtype=TCP_SENDER_PACE_DTYPE)
        q[:] = T.pace_init(**pace)
        return (torch.from_numpy(entries.view(np.int64).copy()).to(dev),
                torch.from_numpy(q.view(np.int64).copy()).to(dev))

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        sink.write(text + "\n")
        sink.flush()

    def med(x):
        return round(statistics.median(x), 2)

    with Engine(0) as eng:
        for case in args.cases.split(","):
            n_conns, max_buffers, B, stride = SHAPES[case]
            n = n_conns * max_buffers
            arena_bytes = n * stride
            rot = max(2, -(-(1 << 30) // arena_bytes))
            arenas = [torch.empty(arena_bytes, dtype=torch.uint8, device=dev) for _ in range(rot)]
            descs = torch.zeros(n * (DESC_DTYPE.itemsize // 8), dtype=torch.int64, device=dev)
            tick = torch.zeros(TCP_SENDER_PACED_TICK_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
            ids = torch.arange(n_conns, dtype=torch.int32, device=dev)
            scratch = torch.zeros((T.senders_paced_scratch_bytes(n_conns) + 7) // 8, dtype=torch.int64, device=dev)
            sent = eng.new_counters()
            half = max(1, max_buffers // 2)
            plain_senders, _ = table(n_conns, B)
            unpaced_senders, unpaced = table(n_conns, B)
            half_senders, halved = table(n_conns, B, bytes_per_second=half * B * 1000 // PERIOD, period_ms=PERIOD)

            def plain(i, capacity=n):
                T.senders_send(eng, arenas[i % rot], stride, 0, capacity, ids, max_buffers, plain_senders, n_conns,
                               descs, scratch, tick=tick[:4], sent_counters=sent)

            def paced(i, capacity=n, senders=unpaced_senders, pace=unpaced):
                clock[0] += PERIOD
                T.senders_send_paced(eng, arenas[i % rot], stride, 0, capacity, ids, max_buffers, senders, pace,
                                     n_conns, clock[0], descs, scratch, tick=tick, sent_counters=sent)

            def read_tick():
                torch.cuda.synchronize()
                return tick.cpu().numpy().view(TCP_SENDER_PACED_TICK_DTYPE)[0]

            paced(0)
            t = read_tick()
            assert int(t["buffers"]) == n and int(t["connections_pending"]) == 0, t
            paced(0, senders=half_senders, pace=halved)
            paced(0, senders=half_senders, pace=halved)
            t = read_tick()
            assert int(t["buffers"]) == n_conns * half, t
            half_pending = int(t["connections_pending"])
            r = {k: [] for k in ("plain", "unpaced", "half", "plain_plan", "unpaced_plan")}
            for _ in range(args.rounds):
                r["plain"].append(timed(plain))
                r["unpaced"].append(timed(paced))
                r["half"].append(timed(lambda i: paced(i, senders=half_senders, pace=halved)))
                r["plain_plan"].append(timed(lambda i: plain(i, capacity=0)))
                r["unpaced_plan"].append(timed(lambda i: paced(i, capacity=0)))
            line = dict(case=case, buffers=n, n_conns=n_conns, max_buffers=max_buffers, buffer_size=B, stride=stride,
                        arenas=rot, half_buffers=n_conns * half, half_pending=half_pending, reps=args.reps, rounds=args.rounds)
            for k, v in r.items():
                line[k + "_us"] = [round(x, 2) for x in v]
                line[k + "_median_us"] = med(v)
            line["plain_rest_us"] = round(line["plain_median_us"] - line["plain_plan_median_us"], 2)
            line["unpaced_rest_us"] = round(line["unpaced_median_us"] - line["unpaced_plan_median_us"], 2)
            line["plain_plan_spread_us"] = round(max(r["plain_plan"]) - min(r["plain_plan"]), 2)
            line["plain_spread_us"] = round(max(r["plain"]) - min(r["plain"]), 2)
            emit(line)
            del arenas, descs, ids, scratch, plain_senders, unpaced_senders, unpaced, half_senders, halved
            torch.cuda.empty_cache()

        if args.loop:
            n_conns, max_buffers, B, stride = 4096, 700, 48, 48
            arena = torch.empty(16 * stride, dtype=torch.uint8, device=dev)
            descs = torch.zeros(16 * (DESC_DTYPE.itemsize // 8), dtype=torch.int64, device=dev)
            tick = torch.zeros(TCP_SENDER_PACED_TICK_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
            ids = torch.arange(n_conns, dtype=torch.int32, device=dev)
            scratch = torch.zeros((T.senders_paced_scratch_bytes(n_conns) + 7) // 8, dtype=torch.int64, device=dev)
            tables = {"unpaced": table(n_conns, B),
                      "rate_700_steps": table(n_conns, B, bytes_per_second=10 * 1000 * B * 1000, period_ms=PERIOD),
                      "burst_700_steps": table(n_conns, B, burst_count=100000, burst_delay_ms=5)}
            # capacity 0 stores no pace entry of a connection that wants slots, so every call runs the same loop
            r = {k: [] for k in tables}
            for _ in range(args.rounds):
                for k, (senders, pace) in tables.items():
                    r[k].append(timed(lambda i: T.senders_send_paced(eng, arena, stride, 0, 0, ids, max_buffers,
                                                                     senders, pace, n_conns, 0, descs, scratch,
                                                                     tick=tick)))
            line = dict(case="loop700", n_conns=n_conns, max_buffers=max_buffers, reps=args.reps, rounds=args.rounds)
            for k, v in r.items():
                line[k + "_plan_us"] = [round(x, 2) for x in v]
                line[k + "_plan_median_us"] = med(v)
            emit(line)
    sink.close()


if __name__ == "__main__":
    main()
