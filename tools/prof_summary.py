#!/usr/bin/env python3
"""Summarise a tools/gpu_round.sh run (rocprofv3 CSVs) into profiles/<tag>/.

* kernel_stats.csv            — rocprofv3 --kernel-trace --stats summary (copied)
* verify_kernel_trace.json    — per-kernel/grid duration statistics from the trace
* pmc_traffic.json            — HBM bytes per launch from the PMC passes, corrected
                                as /opt/skills/guides/MI355X_MICROARCH.md §HBM says:
                                FETCH_SIZE is reported in KiB and counts exactly 1/2
                                of the bytes of a 16-B/lane streaming read on gfx950
                                (so bytes = 2 x 1024 x FETCH_SIZE); WRITE_SIZE (KiB)
                                is exact for 16-B/lane streaming stores.
usage: python tools/prof_summary.py gpurun_out/r01 profiles/r01
"""
import csv
import json
import os
import shutil
import sys
from collections import defaultdict

import numpy as np

# kernel name -> workload tag, per bench.py's launches. Two profiled runs: prof_* is the config-2
# headline (bench.py --no-extras), prof_dg_* the config-3 datagram extras (--extras-only datagram);
# each kernel is summarised from the first run that launched it most, and reports its grid.
DG = 16 * 1024 * 1024
WORKLOADS = {
    "verify_wg_kernel": "config2 verify: 4096 x 64 KiB (268435456 B read)",
    "fill_kernel": "config2 fill: 4096 x 64 KiB (268435456 B written)",
    "fill_pieces_kernel": "config2 fill in piece order (round 6): 4096 x 64 KiB (268435456 B written)",
    "verify_quad_kernel": "config3 verify: 16M x 1472 B datagrams (%d B payload read)" % (DG * 1446),
    "media_stream_verify_quad_kernel": "config3 MediaStream receive: 16M x 1472 B datagrams (%d B payload read)" % (
        DG * 1446),
    "media_stream_verify_quad_kernel[strided]": "config3 MediaStream receive, strided ring (lengths only): 16M x "
                                                "1472 B datagrams (%d B payload read)" % (DG * 1446),
    "verify_quad_kernel[strided]": "config3 verify, strided ring (lengths only): 16M x 1472 B datagrams "
                                   "(%d B payload read)" % (DG * 1446),
    "media_stream_verify_quad_kernel[status]": "config3 MediaStream compact receive (16-B statuses): 16M x 1472 B "
                                               "datagrams (%d B payload read)" % (DG * 1446),
    "media_stream_verify_quad_kernel[strided][status]": "config3 MediaStream compact receive, strided ring: 16M x "
                                                        "1472 B datagrams (%d B payload read)" % (DG * 1446),
    "media_stream_verify_quad_kernel[frames]": "config3 MediaStream receive with the frame accounting summed on the "
                                               "GPU: 16M x 1472 B datagrams (%d B payload read)" % (DG * 1446),
    "media_stream_verify_quad_kernel[strided][frames]": "config3 MediaStream receive with GPU frame sums, strided "
                                                        "ring: 16M x 1472 B datagrams (%d B payload read)" % (DG * 1446),
    "fill_batched_kernel": "config3 MediaStream fill through descriptors (cts_media_stream_fill, LDS-batched): 16M x "
                           "1472 B datagrams (%d B written)" % (DG * 1472),
    "media_stream_fill_ring_kernel": "config3 MediaStream fill of a datagram ring (cts_media_stream_fill_strided): 16M "
                                     "x 1472 B datagrams (%d B written)" % (DG * 1472),
}
ALGO_BYTES = {"fill_batched_kernel": DG * 1472, "media_stream_fill_ring_kernel": DG * 1472,
              "verify_wg_kernel": 268435456, "fill_kernel": 268435456, "fill_pieces_kernel": 268435456,
              "verify_quad_kernel": DG * 1446,
              "media_stream_verify_quad_kernel": DG * 1446,
              "media_stream_verify_quad_kernel[strided]": DG * 1446, "verify_quad_kernel[strided]": DG * 1446,
              "media_stream_verify_quad_kernel[status]": DG * 1446,
              "media_stream_verify_quad_kernel[strided][status]": DG * 1446,
              "media_stream_verify_quad_kernel[frames]": DG * 1446,
              "media_stream_verify_quad_kernel[strided][frames]": DG * 1446}
RUNS = ("prof", "prof_dg")
# since round 6 the config-2 run launches fill_pieces_kernel; fill_kernel is then the datagram run's payload fill
# (cts_fill with a 1472-B hint: one wave per datagram, 26-B header skipped)
RUN_WORKLOADS = {("fill_kernel", "prof_dg"): ("config3 datagram payload fill (cts_fill, wave per datagram): 16M x 1472 B "
                                              "datagrams (%d B payload written)" % (DG * 1446), DG * 1446)}


def _label(k, run):
    return RUN_WORKLOADS.get((k, run), (WORKLOADS[k], ALGO_BYTES[k]))


def _kname(name):
    base = name.split("(")[0].split("<")[0].split("::")[-1].strip()
    if base in ("media_stream_verify_quad_kernel", "verify_quad_kernel") and "<" in name:
        targs = [t.strip() for t in name.split("(")[0].split("<", 1)[1].rsplit(">", 1)[0].split(",")]
        # template arguments <NT, STRIDED[, RING, STATUS, FRAMES]> (cts_verify.hip, cts_media_stream_recv.hip)
        tag = "[strided]" if len(targs) > 1 and targs[1] == "true" else ""
        if base == "media_stream_verify_quad_kernel" and len(targs) > 3 and targs[3] == "true":
            tag += "[status]"
        if base == "media_stream_verify_quad_kernel" and len(targs) > 4 and targs[4] == "true":
            tag += "[frames]"
        return base + tag
    return base


def _grid(r):
    return r.get("Grid_Size") or r.get("Grid_Size_X")


def _by_kernel(rows, value):
    """{kernel: (grid, [values])} keeping, per kernel, the grid launched most often."""
    by = defaultdict(list)
    for r in rows:
        k = _kname(r["Kernel_Name"])
        if k in WORKLOADS:
            by[(k, _grid(r))].append(value(r))
    best = {}
    for (k, g), v in by.items():
        if k not in best or len(v) > len(best[k][1]):
            best[k] = (g, v)
    return best


def _pipelined(tr):
    """Bursts of config-2 verify launches (gaps > 200 us split them) in a `bench.py --full` run: the
    serialized roofline leg and the pipelined headline leg. Per burst: launches, grids, wall span /
    launch (first start to last end), mean kernel duration, and how many launches start before the
    previous one ends (overlap)."""
    if not os.path.exists(tr):
        return None
    iv = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(_grid(r))) for r in csv.DictReader(open(tr))
                if _kname(r["Kernel_Name"]) == "verify_wg_kernel" and int(_grid(r)) >= 65536)
    bursts = []
    for a, b, g in iv:
        if not bursts or a - max(e for _, e, _ in bursts[-1]) > 200_000:
            bursts.append([])
        bursts[-1].append((a, b, g))
    res = []
    for bu in bursts:
        if len(bu) < 50:
            continue
        span = max(e for _, e, _ in bu) - bu[0][0]
        over = sum(1 for i in range(1, len(bu)) if bu[i][0] < max(e for _, e, _ in bu[:i]))
        res.append({"launches": len(bu), "grids": sorted({g for _, _, g in bu}),
                    "wall_us_per_launch": round(span / len(bu) / 1e3, 2),
                    "algorithmic_GBps_at_wall": round(ALGO_BYTES["verify_wg_kernel"] * len(bu) / span, 1),
                    "mean_kernel_us": round(float(np.mean([b - a for a, b, _ in bu])) / 1e3, 2),
                    "launches_overlapping_previous": over})
    return {"kernel": "verify_wg_kernel", "run": "prof_pipe", "bursts": res} if res else None


def main(src, dst):
    os.makedirs(dst, exist_ok=True)
    for run in RUNS:
        ks = os.path.join(src, run + "_kt", "run_kernel_stats.csv")
        if os.path.exists(ks):
            shutil.copy(ks, os.path.join(dst, "kernel_stats.csv" if run == "prof" else "kernel_stats_datagram.csv"))
    out = {}
    for run in RUNS:
        tr = os.path.join(src, run + "_kt", "run_kernel_trace.csv")
        if not os.path.exists(tr):
            continue
        best = _by_kernel(csv.DictReader(open(tr)), lambda r: int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        for k, (g, d) in best.items():
            label, algo = _label(k, run)
            if label in out:
                continue
            d = np.array(d)
            out[label] = {"kernel": k, "grid": int(g), "launches": int(d.size), "run": run,
                          "avg_us": round(float(d.mean()) / 1e3, 2), "median_us": round(float(np.median(d)) / 1e3, 2),
                          "min_us": round(float(d.min()) / 1e3, 2),
                          "algorithmic_GBps_at_avg": round(algo / float(d.mean()), 1)}
            if k in ("fill_kernel", "fill_pieces_kernel") and run == "prof":
                # the profiled runs (--no-extras) launch the fill only in workload.materialize, right after
                # torch.zeros wrote the same 256 MiB arena: the 256 MB Infinity Cache absorbs most of that re-write,
                # so this is not an HBM write rate; the bench's extras.fill_GBps (100 launches over 8 rotated
                # arenas, 2 GiB) is
                out[label]["note"] = ("MALL-resident re-write of an arena torch.zeros just wrote: not an HBM "
                                      "rate (see bench.py extras.fill_GBps, 8 rotated arenas)")
                out[label].pop("algorithmic_GBps_at_avg")
                out[label]["algorithmic_GBps_at_avg_mall_resident"] = round(algo / float(d.mean()), 1)
    pipe = _pipelined(os.path.join(src, "prof_pipe_kt", "run_kernel_trace.csv"))
    if pipe:
        out["config2 verify, pipelined headline leg (bench.py default, streams round-robin)"] = pipe
        shutil.copy(os.path.join(src, "prof_pipe_kt", "run_kernel_stats.csv"),
                    os.path.join(dst, "kernel_stats_pipelined.csv"))
    if out:
        json.dump(out, open(os.path.join(dst, "kernel_trace_summary.json"), "w"), indent=1)
    pmc = {}
    for run in RUNS:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE", "TCC_EA0_RDREQ_sum"):
            p = os.path.join(src, "%s_pmc_%s" % (run, ctr), "run_counter_collection.csv")
            if not os.path.exists(p):
                continue
            best = _by_kernel(csv.DictReader(open(p)), lambda r: float(r["Counter_Value"]))
            for k, (g, v) in best.items():
                label, algo = _label(k, run)
                e = pmc.setdefault(label, {"kernel": k, "grid": int(g), "run": run, "algorithmic_bytes": algo})
                if e["run"] != run or ctr + "_median" in e:
                    continue
                e[ctr + "_median"] = float(np.median(v))
                e["launches_" + ctr] = len(v)
    for name, e in pmc.items():
        if "FETCH_SIZE_median" in e:
            e["hbm_read_bytes_per_launch"] = int(2 * 1024 * e["FETCH_SIZE_median"])
        if "TCC_EA0_RDREQ_sum_median" in e:
            e["hbm_read_bytes_per_launch_from_rdreq"] = int(128 * e["TCC_EA0_RDREQ_sum_median"])
        if "WRITE_SIZE_median" in e:
            e["hbm_write_bytes_per_launch"] = int(1024 * e["WRITE_SIZE_median"])
        main_bytes = e.get("hbm_write_bytes_per_launch") if "fill" in e["kernel"] else e.get(
            "hbm_read_bytes_per_launch")
        if main_bytes:
            e["traffic_over_algorithmic"] = round(main_bytes / e["algorithmic_bytes"], 4)
    if pmc:
        v = pmc.get(WORKLOADS["verify_wg_kernel"], {})
        pmc_out = {"workload": "config2", "buffers": 4096, "hbm_bytes_per_launch": v.get("hbm_read_bytes_per_launch"),
                   "correction": "bytes = 2 x 1024 x FETCH_SIZE(KiB) (gfx950 streaming-read halving)",
                   "kernels": pmc}
        json.dump(pmc_out, open(os.path.join(dst, "pmc_traffic.json"), "w"), indent=1)
    print(json.dumps({"trace": out, "pmc": pmc}, indent=1))


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit("usage: python tools/prof_summary.py gpurun_out/<tag> profiles/<round>/<dir>")
    main(sys.argv[1], sys.argv[2])
