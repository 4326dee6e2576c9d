#!/usr/bin/env python3
"""tcp_exchange_paced_probe.py — what the paced exchange tick costs beside the plain one.

PushPull connections (-PushBytes 2.5 buffers, -PullBytes 1.5 buffers, so a tick of max_buffers 8 crosses three segment
ends) whose transfers no call ends. For each shape (--cases), alternated in this one process (--rounds times), HIP
events around each call (both ticks through the bare C ABI), the median of --reps calls after --warmup, two arenas in
rotation:

  plain          cts_tcp_exchange_send, whole
  unpaced        cts_tcp_exchange_send_paced over pace entries without a rate or a burst setting, whole
  all            cts_tcp_exchange_send_paced with both sides rate-limited at a rate that lets every connection release
                 all max_buffers, the clock one quantum further at every call: the walk run to its end by every lane
  plain_plan     the plain tick at capacity 0: its three planning launches alone
  unpaced_plan   the paced tick over unpaced entries at capacity 0
  all_plan       the walk of `all` at capacity 0 (nothing is stored, so every call runs the same max_buffers steps)
  wait_plan      every connection's next send pending and not yet due, capacity 0: the walk stops at its first step

A shape whose max_buffers x connections slots would not fit --max-slots is run with that capacity: the planning still
covers every listed connection, the fill and the descriptors only the slots. The planning cost per step and planning
launch of a wave's longest lane (sums and apply both walk) is given two ways: step_us = (all_plan - unpaced_plan) /
(2 x max_buffers), the walk beside no walk over the same loads, and step_over_wait_us with wait_plan as the floor,
whose apply also stores every connection's two pace entries (code 5 saves them, capacity 0 saves nothing for `all`).

The expectation (stated, not a gate): unpaced within plain's own spread. One JSON line per shape goes to
tcp_exchange_paced_probe.jsonl under --out (default profiles/tcp_exchange_paced/) and to stdout.

  python tools/tcp_exchange_paced_probe.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# case: (connections, max_buffers, buffer size, stride)
SHAPES = {"1024x8_64k": (1024, 8, 65536, 65536), "65536x8_64k": (65536, 8, 65536, 65536),
          "1024x8_1472": (1024, 8, 1472, 1488), "65536x8_1472": (65536, 8, 1472, 1488)}
PERIOD = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default=",".join(SHAPES))
    ap.add_argument("--max-slots", type=int, default=65536, help="capacity cap for the 64 KiB shapes (4 GiB an arena)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcp_exchange_paced"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from ctstraffic_amd import Engine
    from ctstraffic_amd import tcp_exchange as X
    from ctstraffic_amd import tcp_senders as T
    from ctstraffic_amd.types import (DESC_DTYPE, TCP_EXCHANGE_DTYPE, TCP_EXCHANGE_PACED_TICK_DTYPE,
                                      TCP_EXCHANGE_PUSHPULL, TCP_SENDER_PACE_DTYPE)

    assert torch.cuda.is_available(), "tcp_exchange_paced_probe needs a GPU"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    os.makedirs(args.out, exist_ok=True)
    sink = open(os.path.join(args.out, "tcp_exchange_paced_probe.jsonl"), "w")
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

    def entries_of(n_conns, B):
        e = np.empty(n_conns, dtype=TCP_EXCHANGE_DTYPE)
        e[:] = X.exchange_init(TCP_EXCHANGE_PUSHPULL, 1 << 60, B, 2 * B + B // 2, B + B // 2)
        return torch.from_numpy(e.view(np.int64).copy()).to(dev)

    def pace_of(n_conns, pending=False, **pace):
        q = np.empty(2 * n_conns, dtype=TCP_SENDER_PACE_DTYPE)
        q[:] = T.pace_init(**pace)
        if pending:
            q["pending"], q["due_ms"] = 1, 1 << 61
        return torch.from_numpy(q.view(np.int64).copy()).to(dev)

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        sink.write(text + "\n")
        sink.flush()

    with Engine(0) as eng:
        for case in args.cases.split(","):
            n_conns, max_buffers, B, stride = SHAPES[case]
            wanted = n_conns * max_buffers
            n = wanted if stride < 65536 else min(wanted, args.max_slots)
            arena_bytes = n * stride
            arenas = [torch.empty(arena_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
            descs = torch.zeros(n * (DESC_DTYPE.itemsize // 8), dtype=torch.int64, device=dev)
            tick = torch.zeros(TCP_EXCHANGE_PACED_TICK_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
            ids = torch.arange(n_conns, dtype=torch.int32, device=dev)
            scratch = torch.zeros((X.exchange_paced_scratch_bytes(n_conns) + 7) // 8, dtype=torch.int64, device=dev)
            sent = eng.new_counters()
            plain_entries, unpaced_entries, all_entries = (entries_of(n_conns, B) for _ in range(3))
            unpaced = pace_of(n_conns)
            # a side sends at most 5 of a tick's 8 buffers and a quantum's count is taken back every other call (the
            # clock moves by exactly one period): 32 buffers a quantum are never reached
            roomy = pace_of(n_conns, bytes_per_second=32 * B * 1000 // PERIOD, period_ms=PERIOD)
            held = pace_of(n_conns, pending=True)

            # both ticks through the bare C ABI with the addresses taken once: at five small launches a call, a
            # Python wrapper's microseconds show in the events
            L, h, stream = eng._L, eng._h, torch.cuda.current_stream().cuda_stream
            where = [a.data_ptr() for a in arenas]
            p_ids, p_descs, p_tick, p_sent, p_scratch = (x.data_ptr() for x in (ids, descs, tick, sent, scratch))
            scratch_bytes = scratch.numel() * 8
            p_plain = plain_entries.data_ptr()

            def plain(i, capacity=n):
                rc = L.cts_tcp_exchange_send(h, where[i % 2], arena_bytes, stride, 0, capacity, p_ids, n_conns,
                                             max_buffers, p_plain, n_conns, p_descs, None, p_tick, p_sent, p_scratch,
                                             scratch_bytes, stream)
                assert rc == 0, rc

            def paced(i, capacity=n, entries=unpaced_entries, pace=unpaced):
                clock[0] += PERIOD
                rc = L.cts_tcp_exchange_send_paced(h, where[i % 2], arena_bytes, stride, 0, capacity, p_ids, n_conns,
                                                   max_buffers, entries.data_ptr(), pace.data_ptr(), n_conns, clock[0],
                                                   p_descs, None, p_tick, p_sent, p_scratch, scratch_bytes, stream)
                assert rc == 0, rc

            def read_tick():
                torch.cuda.synchronize()
                return tick.cpu().numpy().view(TCP_EXCHANGE_PACED_TICK_DTYPE)[0]

            paced(0)
            t = read_tick()
            assert int(t["buffers"]) == n and int(t["connections_pending"]) == 0, t
            paced(0, entries=all_entries, pace=roomy)
            paced(0, entries=all_entries, pace=roomy)
            t = read_tick()
            assert int(t["buffers"]) == n and int(t["connections_waiting"]) == 0, t
            paced(0, capacity=0, pace=held)
            t = read_tick()
            assert int(t["connections_waiting"]) == n_conns == int(t["connections_pending"]), t
            r = {k: [] for k in ("plain", "unpaced", "all", "plain_plan", "unpaced_plan", "all_plan", "wait_plan")}
            for _ in range(args.rounds):
                r["plain"].append(timed(plain))
                r["unpaced"].append(timed(paced))
                r["all"].append(timed(lambda i: paced(i, entries=all_entries, pace=roomy)))
                r["plain_plan"].append(timed(lambda i: plain(i, capacity=0)))
                r["unpaced_plan"].append(timed(lambda i: paced(i, capacity=0)))
                r["all_plan"].append(timed(lambda i: paced(i, capacity=0, entries=all_entries, pace=roomy)))
                r["wait_plan"].append(timed(lambda i: paced(i, capacity=0, pace=held)))
            line = dict(case=case, buffers=n, wanted=wanted, n_conns=n_conns, max_buffers=max_buffers, buffer_size=B,
                        stride=stride, reps=args.reps, rounds=args.rounds)
            for k, v in r.items():
                line[k + "_us"] = [round(x, 2) for x in v]
                line[k + "_median_us"] = round(statistics.median(v), 2)
            line["plain_spread_us"] = round(max(r["plain"]) - min(r["plain"]), 2)
            line["unpaced_minus_plain_us"] = round(line["unpaced_median_us"] - line["plain_median_us"], 2)
            line["plain_plan_spread_us"] = round(max(r["plain_plan"]) - min(r["plain_plan"]), 2)
            line["unpaced_plan_minus_plain_plan_us"] = round(line["unpaced_plan_median_us"] -
                                                             line["plain_plan_median_us"], 2)
            line["step_us"] = round((line["all_plan_median_us"] - line["unpaced_plan_median_us"]) /
                                    (2 * max_buffers), 3)
            line["step_over_wait_us"] = round((line["all_plan_median_us"] - line["wait_plan_median_us"]) /
                                              (2 * max_buffers), 3)
            emit(line)
            del arenas, descs, ids, scratch, plain_entries, unpaced_entries, all_entries, unpaced, roomy, held
            torch.cuda.empty_cache()
    sink.close()


if __name__ == "__main__":
    main()
