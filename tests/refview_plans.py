"""The workloads of the reference-view tests (tests/test_refview_cpu.py, tests/test_refview_gpu.py) and what their
corruption plans hold, worked out once on the CPU from the plans alone."""
import numpy as np

from ctstraffic_amd import workload as W

EMPTY = 0xFFFFFFFF

# name -> (connection_streams arguments, launches, facts of the plan)
PLANS = {
    # the workgroup path: config-4/5 shaped streams, one buffer in 37 corrupt
    "wg": (dict(n_conns=96, buffers_per_conn=48, length=65536, corrupt_rate=37), 3,
           dict(failed=73, clean=23, first_by_launch=[34, 24, 15], multi=26, first_buffer=2,
                bytes_recv=167313408, bytes_after_failure=134676480, buffers_failed_verify=124)),
    # ragged completions at every alignment, still the workgroup path
    "ragged": (dict(n_conns=64, buffers_per_conn=24, length=65536, ragged=True, corrupt_rate=29, align=1), 3,
               dict(failed=39, clean=25, multi=7, last_buffer=1)),
    # datagram-sized ragged completions: the four-buffers-per-wave path
    "quad": (dict(n_conns=200, buffers_per_conn=64, length=1472, ragged=True, corrupt_rate=97, align=1), 2,
             dict(failed=93, clean=107, first_by_launch=[51, 42])),
}


def plan(name):
    """(workload, [(descs_k, base_k, index_k)], ordinals[n], facts)."""
    kw, parts, facts = PLANS[name]
    w = W.connection_streams(**kw)
    launches = W.stream_launches(w.descs, kw["buffers_per_conn"], parts)
    ordinals = np.zeros(w.n, dtype=np.int64)
    for d, base, idx in launches:
        ordinals[idx] = base + np.arange(len(idx))
    return w, launches, ordinals, facts


def plan_failed_mask(w):
    """The buffers the corruption plan fails (every injected byte differs: workload.py's module docstring)."""
    m = np.zeros(w.n, dtype=bool)
    m[w.corrupt_buf] = True
    return m


def check_facts(w, launches, ordinals, failed, facts, buffers_per_conn):
    """The facts the issue lists for a plan, from a failed mask; returns (sums, slots) of the model."""
    sums, slots = W.reference_view(w.descs, failed, ordinals, w.n_conns)
    assert int((slots != EMPTY).sum()) == facts["failed"]
    assert int((slots == EMPTY).sum()) == facts["clean"]
    assert sums["buffers_failed"] == facts["failed"]
    per_launch = np.zeros((len(launches), w.n_conns), dtype=bool)
    for k, (d, base, idx) in enumerate(launches):
        f = failed[idx]
        per_launch[k, d["conn_index"][f].astype(np.int64)] = True
    if "first_by_launch" in facts:
        bases = [b for _, b, _ in launches] + [w.n]
        got = [int(((slots >= bases[k]) & (slots < bases[k + 1])).sum()) for k in range(len(launches))]
        assert got == facts["first_by_launch"]
    if "multi" in facts:
        assert int((per_launch.sum(0) > 1).sum()) == facts["multi"]
    grid = failed.reshape(-1, buffers_per_conn)  # connection-major
    first_pos = np.where(grid.any(1), grid.argmax(1), -1)
    if "first_buffer" in facts:
        assert int((first_pos == 0).sum()) == facts["first_buffer"]
    if "last_buffer" in facts:
        assert int((first_pos == buffers_per_conn - 1).sum()) == facts["last_buffer"]
    for f in ("bytes_recv", "bytes_after_failure"):
        if f in facts:
            assert sums[f] == facts[f]
    if "buffers_failed_verify" in facts:
        assert int(failed.sum()) == facts["buffers_failed_verify"]
    vlen = w.descs["length"].astype(np.int64) - w.descs["skip_head"].astype(np.int64)
    assert sums["bytes_recv"] + sums["bytes_after_failure"] == int(vlen.sum())
    assert sums["buffers_recv"] + sums["buffers_after_failure"] == w.n
    assert sums["bytes_ok"] <= sums["bytes_recv"] and sums["buffers_recv"] - sums["buffers_failed"] >= 0
    return sums, slots
