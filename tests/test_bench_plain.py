"""bench.py's plain run and `--dump-outputs`.

CPU: the argument checks (no GPU call before them).
GPU: a plain run (no --full) times exactly --steps steps, carries none of the --full legs in its line, and
`--dump-outputs DIR` leaves the last step's outputs as float64 .npy files equal to the corruption plan's analytic outcome
(ctstraffic_amd.workload.expected_results), which depends on the seeds alone: two builds given the same arguments write
the same files.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
_RANK_ENV = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in _RANK_ENV}
    return subprocess.run([sys.executable, BENCH, *argv], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=300)


def test_argument_checks():
    for argv, msg in ((["--steps", "0"], "--steps must be at least 1"),
                      (["--stub-gpu", "--dump-outputs", "x"], "--dump-outputs writes the default leg's outputs"),
                      (["--engines", "1", "--dump-outputs", "x"], "--dump-outputs writes the default leg's outputs")):
        r = _bench(*argv)
        assert r.returncode == 2 and r.stdout == "" and msg in r.stderr, (argv, r.stderr)
    assert not os.path.exists(os.path.join(ROOT, "x"))


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path):
    from ctstraffic_amd import workload as W
    from ctstraffic_amd.types import COUNTER_FIELDS_EX, RESULT_DTYPE

    n, R, K = 2048, 2, 3  # 2048 buffers: two corrupt ones per batch (1/1024)
    out = tmp_path / "dump"
    r = _bench("--gpus", "1", "--steps", str(K), "--warmup", "1", "--arenas", str(R), "--buffers", str(n),
               "--dump-outputs", str(out))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    # the headline's keys, and none of the --full legs
    assert j["unit"] == "GiB/s" and j["higher_is_better"] is True and j["dtype"] == "u8" and j["n_gpus"] == 1
    assert j["full"] is False and j["parity"] is None and j["cpu_baseline"] is None and "extras" not in j
    assert j["roofline"]["timing"].startswith("HIP events around the headline leg's K*R pipelined launches")
    assert j["roofline"]["avg_kernel_us"] == j["roofline"]["pipelined"]["us_per_launch"]
    # --steps sets the timed steps: value and ms_per_step are the same clock over K steps of R launches
    assert j["steps"] == K and j["config"]["launches_per_step"] == R and j["ms_per_step"] > 0
    step_gib = j["config"]["verified_bytes_per_step_per_gpu"] / float(1 << 30)
    assert step_gib == R * n * 65536 / float(1 << 30)
    assert j["value"] * j["ms_per_step"] / 1e3 == pytest.approx(step_gib, rel=0.02)  # both rounded in the line

    names = ["records_%s" % f for f in RESULT_DTYPE.names] + ["conn_first_fail", "counters"]
    assert sorted(os.listdir(out)) == sorted(x + ".npy" for x in names)
    got = {x: np.load(out / (x + ".npy")) for x in names}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    w = W.tcp_resident(n_buffers=n)
    first, count, ctr, cff = W.expected_results(w)
    failed = first >= 0
    assert failed.sum() == 2
    for x in names[:-1]:
        assert got[x].shape == (R, n), x
    for a in range(R):
        assert np.array_equal(got["records_pass"][a], (~failed).astype(np.float64))
        assert np.array_equal(got["records_first_mismatch"][a], np.where(failed, first, 65536))
        assert np.array_equal(got["records_mismatch_bytes"][a], count)
        assert np.all(got["records_flags"][a] == 0)
        bad = np.nonzero(failed)[0]
        assert np.all(got["records_expected"][a][bad] != got["records_actual"][a][bad])
        assert np.array_equal(got["conn_first_fail"][a], cff.view(np.int32))  # an empty slot reads -1
    exp = {k: v * K * R for k, v in ctr.items()}
    exp["connections_failed"] = int(failed.sum()) * R  # each arena's first timed launch claims its failed connections
    assert dict(zip(COUNTER_FIELDS_EX, got["counters"].tolist())) == exp
