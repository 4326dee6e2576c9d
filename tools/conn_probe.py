#!/usr/bin/env python3
"""conn_probe.py — what the per-connection reference-view pass and the connection close cost on this GPU.

Times four things with HIP events (one pair per launch, median / min / max over --reps launches after --warmup, the
inputs rotated over several copies so no launch finds its descriptors in the Infinity Cache from the one before):

  a  cts_refview_accumulate          the node-wide pass alone
  b  cts_refview_accumulate_conns    the same pass keeping every connection's entry too, over the same descriptors
  c  the verify of the same batch    cts_verify_at / cts_verify_strided_at
  d  cts_conns_close                 of 1 024 and of 65 536 connections (one line of its own)

on four shapes, one JSON line each with the ratios b/a and b/c:

  config2    4 096 x 64 KiB buffers, one per connection
  config5    the descriptors of config 4/5's rank-0 shard (128 connections x 1 024 x 64 KiB, connection-major)
  ring       config 3's 16 Mi-datagram ring of one connection (4 bytes of lengths per buffer): the run-aggregation case,
             every wave's span one run
  no_runs    16 Mi datagram descriptors in buffer-major order over 1 024 connections: neighbouring descriptors always
             differ in connection, one set of atomic adds per buffer (the atomic-bound case)

b must stay below c on every shape: the pass keeps the books of that verify. --n shrinks the two 16 Mi shapes.

  python tools/conn_probe.py > conn_probe.jsonl
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--n", type=int, default=16 * 1024 * 1024, help="datagrams of the ring and of the no-runs shape")
    ap.add_argument("--shapes", default="config2,config5,ring,no_runs,close")
    args = ap.parse_args()
    shapes = args.shapes.split(",")

    import numpy as np
    import torch

    from ctstraffic_amd import Engine
    from ctstraffic_amd import workload as W
    from ctstraffic_amd.engine import descs_to_device
    from ctstraffic_amd.types import CONN_STATE_DTYPE

    assert torch.cuda.is_available(), "conn_probe needs a GPU"
    torch.cuda.set_device(0)
    dev = "cuda:0"

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

    def report(shape, a, b, c, **extra):
        ma, mb, mc = (statistics.median(x) for x in (a, b, c))
        print(json.dumps(dict(shape=shape, refview=stats(a), refview_conns=stats(b), verify=stats(c),
                              b_over_a=round(mb / ma, 3), b_over_c=round(mb / mc, 5), b_below_c=bool(mb < mc),
                              reps=args.reps, **extra)), flush=True)

    def slots_dev(slots):
        return torch.from_numpy(np.ascontiguousarray(slots, dtype=np.uint32).view(np.int32).copy()).to(dev)

    def descriptor_shape(eng, name, w, arenas, copies, **extra):
        """a, b, c over a descriptor batch; the model's table checks b once."""
        _, _, _, ecff = W.expected_results(w)
        dd = [descs_to_device(w.descs, dev) for _ in range(copies)]
        ref, ctr = eng.new_counters(), eng.new_counters()
        slots = slots_dev(ecff)
        state = eng.new_conn_state(w.n_conns)
        eng.refview_conns(w.arena_bytes, dd[0], ref, state, conn_first_fail=slots)
        torch.cuda.synchronize()
        want, _ = W.connection_view(w.descs, None, np.arange(w.n), w.n_conns, slots=ecff)
        assert np.array_equal(state.cpu().numpy().view(CONN_STATE_DTYPE), want), name
        a = timed(lambda i: eng.refview(w.arena_bytes, dd[i % copies], ref, conn_first_fail=slots))
        b = timed(lambda i: eng.refview_conns(w.arena_bytes, dd[i % copies], ref, state, conn_first_fail=slots))
        cff = torch.full((w.n_conns,), -1, dtype=torch.int32, device=dev)
        c = timed(lambda i: eng.verify(arenas[i % len(arenas)], dd[i % copies], max_length_hint=w.max_length,
                                       counters=ctr, conn_first_fail=cff, base_index=1), max(8, args.reps // 2))
        report(name, a, b, c, n=w.n, n_conns=w.n_conns, descriptor_bytes=24 * w.n, verified_bytes=w.verified_bytes(),
               descriptor_copies=copies, arenas=len(arenas), **extra)

    with Engine(0) as eng:
        if "config2" in shapes:
            w = W.tcp_resident()
            arenas = [W.materialize(eng, w, device=dev)[0] for _ in range(4)]  # 1 GiB in rotation
            descriptor_shape(eng, "config2", w, arenas, 8)
            del arenas
        if "config5" in shapes:
            w = W.connection_streams(world=8, rank=0, name="config5")
            arenas = [W.materialize(eng, w, device=dev)[0]]  # 8 GiB: far beyond the Infinity Cache
            descriptor_shape(eng, "config5", w, arenas, 16)  # 16 x 25 MB of descriptors
            del arenas
        if "ring" in shapes or "no_runs" in shapes:
            n = args.n
            w = W.udp_datagrams(n_datagrams=n, corrupt_rate=0)
            arena, _ = W.materialize(eng, w, device=dev)
        if "ring" in shapes:
            lens = [torch.full((n,), 1472, dtype=torch.int32, device=dev) for _ in range(8)]
            ref, ctr = eng.new_counters(), eng.new_counters()
            slot = slots_dev([n // 2])
            state = eng.new_conn_state(1)
            kw = dict(skip_head=26, conn_first_fail=slot)
            eng.refview_conns_strided(w.arena_bytes, 1472, lens[0], ref, state, **kw)
            torch.cuda.synchronize()
            got = state.cpu().numpy().view(CONN_STATE_DTYPE)[0]
            assert tuple(int(x) for x in got) == ((n // 2 + 1) * 1446, n // 2 + 1, (n - n // 2 - 1) * 1446,
                                                  n - n // 2 - 1), got
            a = timed(lambda i: eng.refview_strided(w.arena_bytes, 1472, lens[i % 8], ref, **kw))
            b = timed(lambda i: eng.refview_conns_strided(w.arena_bytes, 1472, lens[i % 8], ref, state, **kw))
            cff = torch.full((1,), -1, dtype=torch.int32, device=dev)
            c = timed(lambda i: eng.verify_strided(arena, 1472, lens[i % 8], skip_head=26, counters=ctr,
                                                   conn_first_fail=cff, base_index=1), max(8, args.reps // 2))
            report("ring", a, b, c, n=n, n_conns=1, descriptor_bytes=4 * n, verified_bytes=w.verified_bytes(),
                   descriptor_copies=8, arenas=1)
            del lens
        if "no_runs" in shapes:
            w.descs["conn_index"] = (np.arange(n) % 1024).astype(np.uint32)
            w.n_conns = 1024
            descriptor_shape(eng, "no_runs", w, [arena], 2)
        if "close" in shapes:
            for n_close in (1024, 65536):
                rng = np.random.default_rng(n_close)
                slots_h = np.where(rng.random(n_close) < 0.1, rng.integers(0, 1 << 20, n_close), 0xFFFFFFFF)
                table = np.zeros(n_close, dtype=CONN_STATE_DTYPE)
                table["bytes_recv"] = rng.integers(0, 1 << 30, n_close)
                table["buffers_recv"] = 1
                ids = torch.from_numpy(rng.permutation(n_close).astype(np.int32)).to(dev)
                expect = torch.from_numpy(table["bytes_recv"].astype(np.int64) + rng.integers(-1, 2, n_close)).to(dev)
                fresh_slots, fresh_state = slots_dev(slots_h), torch.from_numpy(table.view(np.int64).copy()).to(dev)
                slots, state = fresh_slots.clone(), fresh_state.clone()
                blk, out = eng.new_counters(), eng.new_conn_results(n_close)

                def launch(i):
                    slots.copy_(fresh_slots)  # a close empties what it closes: the refill is timed apart, below
                    state.copy_(fresh_state)
                    eng.conns_close(ids, expect, slots, state, blk, results=out)

                def refill(i):
                    slots.copy_(fresh_slots)
                    state.copy_(fresh_state)

                both, fill = timed(launch), timed(refill)
                empty = timed(lambda i: eng.conns_close(ids, expect, slots, state, blk, results=out))
                print(json.dumps(dict(shape="close", n=n_close, close_with_refill=stats(both), refill=stats(fill),
                                      close_of_emptied_slots=stats(empty),
                                      close_us=round(statistics.median(both) - statistics.median(fill), 2),
                                      reps=args.reps)), flush=True)


if __name__ == "__main__":
    main()
