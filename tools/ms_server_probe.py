#!/usr/bin/env python3
"""ms_server_probe.py — what a device-planned MediaStream server tick costs beside the host-fed ring fill.

Config 3's shape: --n datagrams of 1472 B per tick (default 16 Mi) at stride 1472, as

  one         one connection; frame_size_bytes is a u32, so its frame holds at most 2 917 776 datagrams of 1472 B and
              this case runs over that many, not over --n
  1024        1 024 connections of n / 1 024 datagrams each
  65536       65 536 connections of n / 65 536 datagrams each
  65536x1     65 536 connections of one datagram each: the planning-bound case

For each case, alternated in this one process (baseline, tick, baseline, tick, ...; --rounds times), HIP events around
each call, the median of --reps calls after --warmup, rotated over two rings:

  baseline    cts_media_stream_fill_strided over the same datagrams, lengths and headers already in device memory
              (the yardstick: the parent's code)
  tick        cts_media_stream_servers_send, whole: the three planning launches and the fill
  planning    the same call at capacity 0: the three planning launches with nothing fitting, so no entry moves and the
              fill is not launched
  fill        tick - planning (derived, not measured alone)

The expectation is tick <= baseline + (the spread of the baseline's own medians). One JSON line per case goes to
ms_server_probe.jsonl under --out (default profiles/ms_servers/) and to stdout.

  python tools/ms_server_probe.py

With --timed the yardstick is the plain tick itself and the subject the timed tick
(cts_media_stream_servers_send_at) over the same four shapes with one frame of every connection out and max_frames 1,
so both write the same datagrams: baseline = cts_media_stream_servers_send, tick = cts_media_stream_servers_send_at,
planning = the timed tick at capacity 0. A fifth line, "catchup", is 1 024 connections x 16 frames of 4 datagrams in
one timed tick (max_frames 16) against 16 plain ticks of one frame each into the same slots: what the multi-frame
tick saves in launches. The lines go to ms_server_timed_probe.jsonl under --out.

  python tools/ms_server_probe.py --timed --out profiles/ms_server_schedule
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DATAGRAM = 1472


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=16 * 1024 * 1024)
    ap.add_argument("--cases", default="one,1024,65536,65536x1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ms_servers"))
    ap.add_argument("--timed", action="store_true", help="the timed tick against the plain tick (see above)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from ctstraffic_amd import Engine
    from ctstraffic_amd import media_stream as M
    from ctstraffic_amd.types import DESC_DTYPE, DGRAM_HEADER_DTYPE, MS_SERVER_STATE_DTYPE, MS_SERVER_TICK_DTYPE

    assert torch.cuda.is_available(), "ms_server_probe needs a GPU"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    os.makedirs(args.out, exist_ok=True)
    sink = open(os.path.join(args.out, "ms_server_timed_probe.jsonl" if args.timed else "ms_server_probe.jsonl"), "w")

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

    qpc, qpf = 123456789, 10_000_000
    shapes = {"one": (1, min(args.n, 0xFFFFFFFF // DATAGRAM)), "1024": (1024, args.n // 1024),
              "65536": (65536, args.n // 65536), "65536x1": (65536, 1)}
    if args.timed:
        timed_probe(args, timed, sink)
        sink.close()
        return
    with Engine(0) as eng:
        rings = [torch.empty(args.n * DATAGRAM, dtype=torch.uint8, device=dev) for _ in range(2)]
        descs = torch.zeros(args.n * (DESC_DTYPE.itemsize // 8), dtype=torch.int64, device=dev)
        lengths = torch.zeros(args.n, dtype=torch.int32, device=dev)
        tick = torch.zeros(MS_SERVER_TICK_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
        for case in args.cases.split(","):
            n_conns, per = shapes[case]
            n = n_conns * per
            entry = M.server_init(per * DATAGRAM, DATAGRAM, 0xFFFFFFFF)
            entries = np.empty(n_conns, dtype=MS_SERVER_STATE_DTYPE)
            entries[:] = entry
            servers = torch.from_numpy(entries.view(np.int64).copy()).to(dev)
            ids = torch.arange(n_conns, dtype=torch.int32, device=dev)
            scratch = torch.zeros((M.servers_scratch_bytes(n_conns) + 7) // 8, dtype=torch.int64, device=dev)
            udp = eng.new_counters()
            host_lengths = torch.full((n,), DATAGRAM, dtype=torch.int32, device=dev)
            h = np.zeros(n, dtype=DGRAM_HEADER_DTYPE)
            h["sequence_number"], h["qpc"], h["qpf"] = 1, qpc, qpf
            headers = torch.from_numpy(h.view(np.uint8)).to(dev)
            del h

            def send(i, capacity=n):
                M.servers_send(eng, rings[i % 2], DATAGRAM, 0, capacity, ids, servers, n_conns, qpc, qpf, scratch,
                               descs=descs, lengths=lengths, tick=tick, udp_counters=udp)

            # the two paths write the same bytes
            send(0)
            M.fill_strided(eng, rings[1][: n * DATAGRAM], DATAGRAM, host_lengths, headers)
            torch.cuda.synchronize()
            t = tick.cpu().numpy().view(MS_SERVER_TICK_DTYPE)[0]
            assert int(t["datagrams"]) == n and int(t["connections_sent"]) == n_conns, t
            step = 1 << 28
            for o in range(0, n * DATAGRAM, step):
                assert torch.equal(rings[0][o:o + step][: n * DATAGRAM - o], rings[1][o:o + step][: n * DATAGRAM - o])
            base, whole, plan = [], [], []
            for _ in range(args.rounds):
                base.append(timed(lambda i: M.fill_strided(eng, rings[i % 2][: n * DATAGRAM], DATAGRAM, host_lengths,
                                                           headers)))
                whole.append(timed(send))
                plan.append(timed(lambda i: send(i, capacity=0)))
            b, w, p = (statistics.median(x) for x in (base, whole, plan))
            margin = max(base) - min(base)
            line = dict(case=case, n=n, n_conns=n_conns, datagrams_per_frame=per, stride=DATAGRAM,
                        baseline_us=[round(x, 2) for x in base], tick_us=[round(x, 2) for x in whole],
                        planning_us=[round(x, 2) for x in plan], baseline_median_us=round(b, 2),
                        tick_median_us=round(w, 2), planning_median_us=round(p, 2), fill_derived_us=round(w - p, 2),
                        baseline_spread_us=round(margin, 2), tick_over_baseline=round(w / b, 4),
                        within_margin=bool(w <= b + margin), reps=args.reps, rounds=args.rounds)
            text = json.dumps(line)
            print(text, flush=True)
            sink.write(text + "\n")
            sink.flush()
            del servers, ids, scratch, host_lengths, headers
    sink.close()


def timed_probe(args, timed, sink):
    """--timed: cts_media_stream_servers_send_at beside cts_media_stream_servers_send, alternated in this process."""
    import numpy as np
    import torch

    from ctstraffic_amd import Engine
    from ctstraffic_amd import media_stream as M
    from ctstraffic_amd.types import (DESC_DTYPE, MS_SERVER_SCHEDULE_DTYPE, MS_SERVER_STATE_DTYPE,
                                      MS_SERVER_TIMED_TICK_DTYPE)

    dev = "cuda:0"
    qpc, qpf, now = 123456789, 10_000_000, 1 << 40  # every frame of a 1 000 fps stream from 0 is long out
    shapes = {"one": (1, min(args.n, 0xFFFFFFFF // DATAGRAM), 1), "1024": (1024, args.n // 1024, 1),
              "65536": (65536, args.n // 65536, 1), "65536x1": (65536, 1, 1), "catchup": (1024, 4, 16)}
    with Engine(0) as eng:
        rings = [torch.empty(args.n * DATAGRAM, dtype=torch.uint8, device=dev) for _ in range(2)]
        descs = torch.zeros(args.n * (DESC_DTYPE.itemsize // 8), dtype=torch.int64, device=dev)
        lengths = torch.zeros(args.n, dtype=torch.int32, device=dev)
        tick = torch.zeros(MS_SERVER_TIMED_TICK_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
        for case in args.cases.split(",") + ["catchup"]:
            n_conns, per, frames = shapes[case]
            n = n_conns * per * frames
            entries = np.empty(n_conns, dtype=MS_SERVER_STATE_DTYPE)
            entries[:] = M.server_init(per * DATAGRAM, DATAGRAM, 0xFFFFFFFF)
            sched = np.empty(n_conns, dtype=MS_SERVER_SCHEDULE_DTYPE)
            sched[:] = M.server_schedule_init(1000, 0)
            servers = torch.from_numpy(entries.view(np.int64).copy()).to(dev)
            fresh = servers.clone()
            schedule = torch.from_numpy(sched.view(np.int64).copy()).to(dev)
            ids = torch.arange(n_conns, dtype=torch.int32, device=dev)
            scratch = torch.zeros((M.servers_timed_scratch_bytes(n_conns) + 7) // 8, dtype=torch.int64, device=dev)
            udp = eng.new_counters()

            def plain(i):  # `frames` plain ticks of one frame each, into the slots the timed tick writes
                for f in range(frames):
                    M.servers_send(eng, rings[i % 2], DATAGRAM, f * n_conns * per, n_conns * per, ids, servers, n_conns,
                                   qpc, qpf, scratch, descs=descs, lengths=lengths, tick=tick[:4], udp_counters=udp,
                                   arena_bytes=n * DATAGRAM)

            def at(i, capacity=n):
                M.servers_send_at(eng, rings[i % 2], DATAGRAM, 0, capacity, ids, servers, schedule, n_conns, frames,
                                  now, qpc, qpf, scratch, descs=descs, lengths=lengths, tick=tick, udp_counters=udp,
                                  arena_bytes=n * DATAGRAM)

            if frames == 1:  # the two ticks write the same bytes from the same entries
                plain(0)
                servers.copy_(fresh)
                at(1)
                torch.cuda.synchronize()
                t = tick.cpu().numpy().view(MS_SERVER_TIMED_TICK_DTYPE)[0]
                assert int(t["datagrams"]) == n and int(t["frames"]) == n_conns, t
                step = 1 << 28
                for o in range(0, n * DATAGRAM, step):
                    assert torch.equal(rings[0][o:o + step][: n * DATAGRAM - o], rings[1][o:o + step][: n * DATAGRAM - o])
            else:
                at(0)
                torch.cuda.synchronize()
                t = tick.cpu().numpy().view(MS_SERVER_TIMED_TICK_DTYPE)[0]
                assert int(t["datagrams"]) == n and int(t["frames"]) == n_conns * frames, t
            base, whole, plan = [], [], []
            for _ in range(args.rounds):
                base.append(timed(plain))
                whole.append(timed(at))
                plan.append(timed(lambda i: at(i, capacity=0)))
            b, w, p = (statistics.median(x) for x in (base, whole, plan))
            margin = max(base) - min(base)
            line = dict(case=case, n=n, n_conns=n_conns, datagrams_per_frame=per, frames_per_tick=frames,
                        stride=DATAGRAM, baseline="cts_media_stream_servers_send x %d" % frames,
                        baseline_us=[round(x, 2) for x in base], tick_us=[round(x, 2) for x in whole],
                        planning_us=[round(x, 2) for x in plan], baseline_median_us=round(b, 2),
                        tick_median_us=round(w, 2), planning_median_us=round(p, 2), fill_derived_us=round(w - p, 2),
                        baseline_spread_us=round(margin, 2), tick_over_baseline=round(w / b, 4),
                        within_margin=bool(w <= b + margin), reps=args.reps, rounds=args.rounds)
            text = json.dumps(line)
            print(text, flush=True)
            sink.write(text + "\n")
            sink.flush()
            del servers, fresh, schedule, ids, scratch


if __name__ == "__main__":
    main()
