#!/usr/bin/env python3
"""tcp_exchange_probe.py — what the exchange tick (cts_tcp_exchange_send) costs beside the TCP senders' tick.

The four shapes of tools/tcp_sender_probe.py (--cases):

  4096x1      4 096 x 64 KiB (config 2's buffers), 4 096 connections, max_buffers 1
  128x32      4 096 x 64 KiB, 128 connections, max_buffers 32
  small       4 Mi x 1 472 B at stride 1 488, 1 024 connections of 4 096 buffers each
  65536x1     65 536 x 64 KiB, 65 536 connections of one buffer each

For each shape, alternated in this one process (--rounds times), HIP events around each call, the median of --reps
calls after --warmup, the arenas rotated so that no call finds its lines in the 256 MB Infinity Cache (at least 1 GiB
of arenas, and at least two):

  senders         cts_tcp_senders_send, whole (the yardstick). With --parent-lib PATH it is that library's, through an
                  engine of its own on the same device and the same buffers: a build of the parent commit; without, it
                  is this build's
  push            cts_tcp_exchange_send over a table of Push entries, whole
  pushpull        cts_tcp_exchange_send over PushPull entries with P = Q = 1 MiB (the reference's default): the same
                  buffer count, and the same byte count where the buffer size divides 1 MiB (reported beside its own
                  byte count; no bar)
  *_plan          the same calls at capacity 0: the three planning launches alone

The expectation for a Push table (stated, and reported as met or missed, not a gate): the whole tick and the
capacity-0 planning within the yardstick's median plus its own max - min over the rounds. One JSON line per shape goes
to tcp_exchange_probe.jsonl under --out (default profiles/tcp_exchange/) and to stdout.

  python tools/tcp_exchange_probe.py [--parent-lib parent/ctstraffic_amd/libcts_engine.so]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# case: (connections, max_buffers, buffer size, stride)
SHAPES = {"4096x1": (4096, 1, 65536, 65536), "128x32": (128, 32, 65536, 65536), "small": (1024, 4096, 1472, 1488),
          "65536x1": (65536, 1, 65536, 65536)}
SEGMENT = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="4096x1,128x32,small,65536x1")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcp_exchange"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from ctstraffic_amd import Engine
    from ctstraffic_amd import tcp_exchange as X
    from ctstraffic_amd import tcp_senders as T
    from ctstraffic_amd.types import (DESC_DTYPE, TCP_EXCHANGE_DTYPE, TCP_EXCHANGE_PUSH, TCP_EXCHANGE_PUSHPULL,
                                      TCP_EXCHANGE_TICK_DTYPE, TCP_SENDER_DTYPE)

    assert torch.cuda.is_available(), "tcp_exchange_probe needs a GPU"
    torch.cuda.set_device(0)
    dev = "cuda:0"
    os.makedirs(args.out, exist_ok=True)
    sink = open(os.path.join(args.out, "tcp_exchange_probe.jsonl"), "w")

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
        yard_lib, yard_engine = eng._L, eng._h
        if args.parent_lib:
            # the parent's build beside this one (-Bsymbolic: its entry points bind inside it), with its own engine
            yard_lib = ctypes.CDLL(os.path.abspath(args.parent_lib), mode=ctypes.RTLD_LOCAL)
            yard_lib.cts_engine_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
            yard_lib.cts_tcp_senders_send.argtypes = eng._L.cts_tcp_senders_send.argtypes
            yard_lib.cts_engine_destroy.argtypes = [ctypes.c_void_p]
            h = ctypes.c_void_p()
            assert yard_lib.cts_engine_create(0, ctypes.byref(h)) == 0
            yard_engine = h
        for case in args.cases.split(","):
            n_conns, max_buffers, B, stride = SHAPES[case]
            n = n_conns * max_buffers
            arena_bytes = n * stride
            rot = max(2, -(-(1 << 30) // arena_bytes))
            arenas = [torch.empty(arena_bytes, dtype=torch.uint8, device=dev) for _ in range(rot)]
            descs = torch.zeros(n * (DESC_DTYPE.itemsize // 8), dtype=torch.int64, device=dev)
            descs_x = torch.zeros_like(descs)
            tick = torch.zeros(TCP_EXCHANGE_TICK_DTYPE.itemsize // 8, dtype=torch.int64, device=dev)
            # transfers no call of this probe ends: every tick sends max_buffers buffers per connection
            plain = np.empty(n_conns, dtype=TCP_SENDER_DTYPE)
            plain[:] = T.sender_init(1 << 60, B)
            push = np.empty(n_conns, dtype=TCP_EXCHANGE_DTYPE)
            push[:] = X.exchange_init(TCP_EXCHANGE_PUSH, 1 << 60, B)
            pp = np.empty(n_conns, dtype=TCP_EXCHANGE_DTYPE)
            pp[:] = X.exchange_init(TCP_EXCHANGE_PUSHPULL, 1 << 60, B, SEGMENT, SEGMENT)
            tables = {k: torch.from_numpy(v.view(np.int64).copy()).to(dev)
                      for k, v in (("senders", plain), ("push", push), ("pushpull", pp))}
            ids = torch.arange(n_conns, dtype=torch.int32, device=dev)
            scratch = torch.zeros((X.exchange_scratch_bytes(n_conns) + 7) // 8, dtype=torch.int64, device=dev)
            sent = eng.new_counters()

            def senders(i, capacity=n):
                rc = yard_lib.cts_tcp_senders_send(yard_engine, arenas[i % rot].data_ptr(), arena_bytes, stride, 0,
                                                   capacity, ids.data_ptr(), n_conns, max_buffers,
                                                   tables["senders"].data_ptr(), n_conns, descs.data_ptr(), None,
                                                   tick.data_ptr(), sent.data_ptr(), scratch.data_ptr(),
                                                   scratch.numel() * 8, None)
                assert rc == 0, rc

            # both ticks are called the same way, through the bare C ABI with the addresses taken once: at three
            # small launches a call, a wrapper's microseconds on the host show in the events
            def exchange(which):
                table = tables[which].data_ptr()

                def send(i, capacity=n):
                    rc = eng._L.cts_tcp_exchange_send(eng._h, arenas[i % rot].data_ptr(), arena_bytes, stride, 0,
                                                      capacity, ids.data_ptr(), n_conns, max_buffers, table, n_conns,
                                                      descs_x.data_ptr(), None, tick.data_ptr(), sent.data_ptr(),
                                                      scratch.data_ptr(), scratch.numel() * 8, None)
                    assert rc == 0, rc
                return send

            # the Push table writes what the senders write: arena and descriptors
            senders(0)
            exchange("push")(1)
            torch.cuda.synchronize()
            assert torch.equal(descs, descs_x), case
            step = (1 << 28) // stride * stride  # whole slots; the bytes behind a buffer in its slot are nobody's
            for o in range(0, arena_bytes, step):
                assert torch.equal(arenas[0][o:o + step].view(-1, stride)[:, :B],
                                   arenas[1][o:o + step].view(-1, stride)[:, :B]), (case, o)
            exchange("pushpull")(0)
            torch.cuda.synchronize()
            t = tick.cpu().numpy().view(TCP_EXCHANGE_TICK_DTYPE)[0]
            assert int(t["buffers"]) == n, t
            pp_bytes = int(t["bytes"])
            names = ("senders", "push", "pushpull", "senders_plan", "push_plan", "pushpull_plan")
            calls = {"senders": senders, "push": exchange("push"), "pushpull": exchange("pushpull")}
            us = {k: [] for k in names}
            for _ in range(args.rounds):
                for k in names:
                    f = calls[k.split("_")[0]]
                    us[k].append(timed(f if not k.endswith("_plan") else (lambda i, f=f: f(i, capacity=0))))
            med = {k: statistics.median(v) for k, v in us.items()}
            spread = max(us["senders"]) - min(us["senders"])
            spread_plan = max(us["senders_plan"]) - min(us["senders_plan"])
            line = dict(case=case, buffers=n, n_conns=n_conns, max_buffers=max_buffers, buffer_size=B, stride=stride,
                        arenas=rot, bytes=n * B, pushpull_bytes=pp_bytes,
                        yardstick="parent build" if args.parent_lib else "this build",
                        **{k + "_us": [round(x, 2) for x in v] for k, v in us.items()},
                        **{k + "_median_us": round(v, 2) for k, v in med.items()},
                        senders_spread_us=round(spread, 2), senders_plan_spread_us=round(spread_plan, 2),
                        push_tick_within=bool(med["push"] <= med["senders"] + spread),
                        push_plan_within=bool(med["push_plan"] <= med["senders_plan"] + spread_plan),
                        reps=args.reps, rounds=args.rounds)
            text = json.dumps(line)
            print(text, flush=True)
            sink.write(text + "\n")
            sink.flush()
            del arenas, descs, descs_x, tables, ids, scratch
            torch.cuda.empty_cache()
        if args.parent_lib:
            yard_lib.cts_engine_destroy(yard_engine)
    sink.close()


if __name__ == "__main__":
    main()
