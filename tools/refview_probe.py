#!/usr/bin/env python3
"""refview_probe.py — what the reference-view pass (cts_refview_accumulate) costs on this GPU.

Times the pass with HIP events over three inputs and prints one JSON line each:

  dg16m      16 Mi datagram descriptors (config 3's batch: 384 MB of descriptors, one connection)
  strided    16 Mi strided-ring lengths (64 MB), rotated over eight arrays so the set exceeds the 256 MB MALL
  config5    the descriptor set of config 5's rank-0 shard (1024 connections x 1024 x 64 KiB over 8 GPUs)

For each: microseconds per pass (median, min, max over --reps timed launches after --warmup), bytes read per second
(descriptor or length bytes, the slot gathers not counted), the same launch over one descriptor (floor_us: what a
launch costs between two events whatever it reads), that rate against a same-box run of
tools/hbm_read_ceiling (run first, in a process of its own, unless --ceiling-jsonl names a file with its output),
and the time as a share of the verify of the same batch: config 3's recorded 3.55 ms (profiles/r06) for the two
datagram inputs, and for config5 the verify of the shard timed here (--no-verify skips it).

  make tools/hbm_read_ceiling && python tools/refview_probe.py > refview_probe.jsonl
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIG3_VERIFY_US = 3550.0  # 16 Mi x 1472 B datagram verify, profiles/r06


def ceiling_gbps(path):
    """The best plain streaming-read rate of tools/hbm_read_ceiling's quick sweep (a file of its JSON lines, or a
    run of it now)."""
    if path:
        text = open(path).read()
    else:
        exe = os.path.join(ROOT, "tools", "hbm_read_ceiling")
        if not os.path.exists(exe):
            raise SystemExit("tools/hbm_read_ceiling is not built (make tools/hbm_read_ceiling)")
        text = subprocess.run([exe, "16", "256", "1"], capture_output=True, text=True, check=True, timeout=300).stdout
    rates = [json.loads(l)["GBps"] for l in text.splitlines() if l.startswith("{")]
    return max(rates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=16 * 1024 * 1024, help="datagrams of the two datagram inputs")
    ap.add_argument("--ceiling-jsonl", default="")
    ap.add_argument("--no-verify", action="store_true")
    args = ap.parse_args()

    ceil = ceiling_gbps(args.ceiling_jsonl)  # before this process opens the GPU

    import numpy as np
    import torch

    from ctstraffic_amd import Engine
    from ctstraffic_amd import workload as W
    from ctstraffic_amd.engine import descs_to_device

    assert torch.cuda.is_available(), "refview_probe needs a GPU"
    torch.cuda.set_device(0)
    dev = "cuda:0"

    def timed(launch, reps):
        for i in range(args.warmup):
            launch(i)
        torch.cuda.synchronize()
        us = []
        for i in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(i)
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        return us

    floor = [0.0]

    def report(name, us, nbytes, verify_us, verify_src, extra):
        med = statistics.median(us)
        rate = nbytes / (med * 1e-6) / 1e9
        print(json.dumps(dict(input=name, us=round(med, 2), us_min=round(min(us), 2), us_max=round(max(us), 2),
                              floor_us=round(floor[0], 2),
                              bytes_read=nbytes, GBps=round(rate, 1), ceiling_GBps=ceil,
                              share_of_ceiling=round(rate / ceil, 3), verify_us=round(verify_us, 1),
                              verify_source=verify_src, share_of_verify=round(med / verify_us, 5), **extra)),
              flush=True)

    with Engine(0) as eng:
        n = args.n
        # ---- the floor: the pass over one descriptor ----
        one = descs_to_device(W.udp_datagrams(n_datagrams=1, corrupt_rate=0).descs, dev)
        ref0 = eng.new_counters()
        floor[0] = statistics.median(timed(lambda i: eng.refview(1472, one, ref0), args.reps))

        # ---- 16 Mi datagram descriptors, one connection failing half way ----
        w = W.udp_datagrams(n_datagrams=n, corrupt_rate=0)
        descs = descs_to_device(w.descs, dev)
        slot = torch.tensor([n // 2], dtype=torch.int32, device=dev)
        ref = eng.new_counters()
        us = timed(lambda i: eng.refview(w.arena_bytes, descs, ref, conn_first_fail=slot), args.reps)
        view = eng.read_counters_ref(ref)
        assert view["buffers_recv"] == (n // 2 + 1) * (args.reps + args.warmup), view
        report("dg16m", us, descs.numel(), CONFIG3_VERIFY_US * n / (16 * 1024 * 1024),
               "config 3, profiles/r06 (recorded)", dict(n=n))
        del descs

        # ---- 16 Mi strided lengths, eight arrays in rotation ----
        lens = [torch.full((n,), 1472, dtype=torch.int32, device=dev) for _ in range(8)]
        eng.reset_counters(ref)
        us = timed(lambda i: eng.refview_strided(n * 1472, 1472, lens[i % 8], ref, skip_head=26,
                                                 conn_first_fail=slot), args.reps)
        view = eng.read_counters_ref(ref)
        assert view["buffers_recv"] == (n // 2 + 1) * (args.reps + args.warmup), view
        report("strided", us, 4 * n, CONFIG3_VERIFY_US * n / (16 * 1024 * 1024), "config 3, profiles/r06 (recorded)",
               dict(n=n, arrays=8))
        del lens

        # ---- config 5's rank-0 shard: connection-major 64 KiB buffers, the plan's own first failures ----
        w = W.connection_streams(world=8, rank=0, name="config5")
        _, _, _, ecff = W.expected_results(w)
        slots = torch.from_numpy(ecff.view(np.int32).copy()).to(dev)
        descs = descs_to_device(w.descs, dev)
        eng.reset_counters(ref)
        us = timed(lambda i: eng.refview(w.arena_bytes, descs, ref, conn_first_fail=slots), args.reps)
        want, _ = W.reference_view(w.descs, np.zeros(w.n, bool), np.arange(w.n), w.n_conns, slots=ecff)
        view = eng.read_counters_ref(ref)
        assert view == {k: v * (args.reps + args.warmup) for k, v in want.items()}, (view, want)
        if args.no_verify:
            verify_us, src = w.verified_bytes() / 6.5e12 * 1e6, "bytes at 6.5 TB/s (not measured)"
        else:
            arena, _ = W.materialize(eng, w, device=dev)
            ctr = eng.new_counters()
            cff = torch.full((w.n_conns,), -1, dtype=torch.int32, device=dev)
            vus = timed(lambda i: eng.verify(arena, descs, max_length_hint=w.max_length, counters=ctr,
                                             conn_first_fail=cff), max(8, args.reps // 4))
            verify_us, src = statistics.median(vus), "timed here"
        report("config5", us, descs.numel(), verify_us, src, dict(n=w.n, verified_bytes=w.verified_bytes()))


if __name__ == "__main__":
    main()
