"""CPU: the reference view of the device counters (include/cts_engine.h, cts_counters_ref): the numpy model
workload.reference_view, the ABI's struct layout and argument checks, and the world-2 all-reduce of a reference-view
block over gloo.

ctsTraffic fails a connection on the completion whose VerifyBuffer failed (ctsIOPattern.cpp:486-489 -> FailedIo), so
its counters hold nothing of a connection after its first failing buffer; the reference view is that stop, applied to
the batched engine's counters. The kernels are checked against the same model in
tests/test_refview_gpu.py.
"""
import ctypes
import os
import socket
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import refview_plans as P
from ctstraffic_amd import _lib
from ctstraffic_amd import distributed as D
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import DESC_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = 0xFFFFFFFF


def _eight():
    d = np.zeros(8, dtype=DESC_DTYPE)
    d["conn_index"] = [0, 1, 0, 2, 0, 1, 2, 0]
    d["length"] = [100, 50, 200, 10, 300, 70, 20, 400]
    d["skip_head"] = [0, 26, 0, 0, 0, 26, 0, 0]
    d["byte_offset"] = np.cumsum(d["length"]) - d["length"]
    failed = np.array([0, 1, 1, 0, 1, 0, 0, 0], dtype=bool)
    return d, failed, np.arange(8)


def test_reference_view_hand_worked_example():
    """Eight buffers of three connections, in arrival order (ordinal = index):
         connection 0: 100 ok, 200 FAIL, 300 FAIL, 400 ok   -> stops at ordinal 2: received 300, clean 100, lost 700
         connection 1: 24 FAIL (50 - 26 header), 44 ok      -> stops at ordinal 1: received 24, clean 0, lost 44
         connection 2: 10 ok, 20 ok                         -> never fails: received 30, clean 30"""
    d, failed, g = _eight()
    sums, slots = W.reference_view(d, failed, g, 3)
    assert slots.tolist() == [2, 1, EMPTY]
    assert sums == {"bytes_recv": 354, "bytes_ok": 130, "buffers_recv": 5, "buffers_failed": 2,
                    "bytes_after_failure": 744, "buffers_after_failure": 3}
    assert tuple(sums) == W.REF_FIELDS == D.REF_FIELDS
    # connection 1 without a slot (n_conns = 1) counts as never failing: its 24 + 44 bytes are received and clean
    sums1, slots1 = W.reference_view(d, failed, g, 1)
    assert slots1.tolist() == [2]
    assert sums1 == {"bytes_recv": 398, "bytes_ok": 198, "buffers_recv": 6, "buffers_failed": 1,
                     "bytes_after_failure": 700, "buffers_after_failure": 2}
    # the ordinals need only increase along each connection: shifted by a base, and with given slots
    sums2, _ = W.reference_view(d, failed, g + 1000, 3)
    assert sums2 == sums
    sums3, _ = W.reference_view(d, np.zeros(8, bool), g, 3, slots=np.array([2, 1, EMPTY], dtype=np.uint32))
    assert sums3 == sums
    # a bad descriptor counts nowhere and fails nothing: buffer 2 refused, connection 0 stops at ordinal 4 instead
    bad = np.zeros(8, bool)
    bad[2] = True
    sums4, slots4 = W.reference_view(d, failed, g, 3, bad=bad)
    assert slots4.tolist() == [4, 1, EMPTY]
    assert sums4 == {"bytes_recv": 100 + 300 + 24 + 30, "bytes_ok": 130, "buffers_recv": 5, "buffers_failed": 2,
                     "bytes_after_failure": 400 + 44, "buffers_after_failure": 2}


@pytest.mark.parametrize("name", sorted(P.PLANS))
def test_reference_view_identities_on_the_gpu_plans(name):
    """The three connection-stream plans of tests/test_refview_gpu.py, failed mask from the corruption plan: the
    counts of failed / clean connections, where the first failures fall, and received + after == checked."""
    w, launches, ordinals, facts = P.plan(name)
    failed = P.plan_failed_mask(w)
    sums, slots = P.check_facts(w, launches, ordinals, failed, facts, P.PLANS[name][0]["buffers_per_conn"])
    # per-connection stream order: every connection's ordinals increase along its stream
    per_conn = ordinals.reshape(w.n_conns, -1)
    assert (np.diff(per_conn, axis=1) > 0).all()
    # launch-local first-failure indices are not ordinals: launch 1's own slots differ from the stream's
    _, _, _, ecff = W.expected_results(w)
    d1, base1, idx1 = launches[1]
    assert base1 > 0 and int((slots != EMPTY).sum()) == int((ecff != EMPTY).sum())
    assert sums["bytes_after_failure"] > 0


def test_descs_bad_is_the_verifys_rule():
    d = np.zeros(6, dtype=DESC_DTYPE)
    d["length"] = 100
    d["byte_offset"] = [0, 900, 901, 2000, 0, 0]
    d["expected_pattern_offset"] = [0, 65535, 0, 0, 65536, 0]
    d["skip_head"] = [0, 100, 0, 0, 0, 101]
    assert W.descs_bad(d, 1000).tolist() == [False, False, True, True, True, True]


def test_counters_ref_layout_matches_c():
    """cts_counters_ref: six u64 in the order of a counter shard's slots, 48 bytes, as cts_counters_ex."""
    assert ctypes.sizeof(_lib.CtsCountersRef) == 48 == ctypes.sizeof(_lib.CtsCountersEx)
    assert tuple(f for f, _ in _lib.CtsCountersRef._fields_) == W.REF_FIELDS
    probe = r"""
#include <stdio.h>
#include <stddef.h>
#include "cts_engine.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(cts_counters_ref), offsetof(cts_counters_ref, bytes_recv),
        offsetof(cts_counters_ref, bytes_ok), offsetof(cts_counters_ref, buffers_recv),
        offsetof(cts_counters_ref, buffers_failed), offsetof(cts_counters_ref, bytes_after_failure),
        offsetof(cts_counters_ref, buffers_after_failure));
 return 0; }
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        with open(c, "w") as f:
            f.write(probe)
        exe = os.path.join(d, "p")
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [48] + [getattr(_lib.CtsCountersRef, f).offset for f in W.REF_FIELDS] == [48, 0, 8, 16, 24, 32, 40]


def test_new_entry_points_refuse_a_null_engine():
    L = _lib.lib()
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.addressof(buf)
    assert L.cts_verify_at(None, p, 64, p, 1, 0, 0, None, None, None, 0, None) == _lib.CTS_E_INVALID
    assert L.cts_verify_strided_at(None, p, 64, 64, p, 1, 0, 0, 0, 0, None, None, None, 0, None) == _lib.CTS_E_INVALID
    assert L.cts_refview_accumulate(None, 64, p, 1, 0, None, 0, p, None) == _lib.CTS_E_INVALID
    assert L.cts_refview_accumulate_strided(None, 64, 64, p, 1, 0, 0, 0, None, 0, p, None) == _lib.CTS_E_INVALID
    out = _lib.CtsCountersRef()
    assert L.cts_counters_read_ref(None, p, ctypes.byref(out), None) == _lib.CTS_E_INVALID
    assert L.cts_counters_read_ref(None, p, None, None) == _lib.CTS_E_INVALID
    assert L.cts_counters_read_multi_ref(None, None, None, 1, ctypes.byref(out)) == _lib.CTS_E_INVALID
    assert L.cts_counters_allreduce_ref(None, None, None, 1, ctypes.byref(out)) == _lib.CTS_E_INVALID


def test_product_library_carries_the_ordinal_and_reference_view_kernels():
    """Next to the kernels tests/test_abi.py lists, the library holds the workgroup verify with a base_index argument
    and the reference-view pass over descriptors and over a strided ring, each for nontemporal and plain loads, and
    nothing else of theirs."""
    import re

    blob = open(_lib.LIB_PATH, "rb").read()
    got = sorted(set(m.decode() for m in re.findall(rb"_ZN3cts\d+(?:verify_wg_ordinal|refview_)[A-Za-z0-9_]*\.kd", blob)))
    want = sorted(["_ZN3cts17verify_wg_ordinalILb%dEEEvPKhmPK12cts_buf_descjP17cts_verify_resultPmPjjj.kd" % nt
                   for nt in (0, 1)] +
                  ["_ZN3cts18refview_accumulateILb%dELb%dEEEvmNS_7VSourceEjjPKjjPm.kd" % (nt, st)
                   for nt in (0, 1) for st in (0, 1)])
    assert got == want


def test_integration_verify_then_refview_fragment_compiles():
    """INTEGRATION.md's per-batch sequence (cts_verify_at, then cts_refview_accumulate on the same stream) compiles
    against the header, as tests/test_integration_snippets.py does for the document's other fragments."""
    import re

    text = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    found = [c for lang, c in re.findall(r"```(\w*)\n(.*?)```", text, re.S)
             if lang == "cpp" and c.startswith("// device-resident receive, per batch k")]
    assert len(found) == 1
    assert found[0].index("cts_verify_at(") < found[0].index("cts_refview_accumulate(")
    params = ("cts_engine* e, const void* arena, uint64_t arena_bytes, const cts_buf_desc* descs_k, uint32_t n_k, "
              "uint32_t& ordinal, cts_verify_result* results_k, void* ctr, uint32_t* conn_first_fail, uint32_t n_conns, "
              "void* refs, void* stream")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "f.cpp")
        with open(src, "w", encoding="utf-8") as f:
            f.write('#include "cts_engine.h"\nvoid snippet(' + params + ")\n{\n" + found[0] + "\n}\n")
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]


# ---- world 2 over gloo: a reference-view block folds and all-reduces like a counter block ----
KW = dict(n_conns=48, buffers_per_conn=6, length=4096, ragged=True, corrupt_rate=7, align=1)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_view(world, rank):
    w = W.connection_streams(world=world, rank=rank, **KW)
    failed = P.plan_failed_mask(w)
    sums, _ = W.reference_view(w.descs, failed, np.arange(w.n), w.n_conns)
    return w, sums


def _rank_main(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    try:
        D.init("gloo")
        _, sums = _rank_view(world, rank)
        # a device-shaped block: 64 shards x 8 u64, this rank's reference view spread over two shards
        block = torch.zeros(64 * 8, dtype=torch.int64)
        for k, f in enumerate(D.REF_FIELDS):
            block[8 * 3 + k] = sums[f] // 3
            block[8 * 63 + k] = sums[f] - sums[f] // 3
        c = D.fold_counters(block, D.REF_FIELDS)
        assert D.counters_dict(c, D.REF_FIELDS) == sums
        D.allreduce_counters(c)
        q.put((rank, "ok", D.counters_dict(c, D.REF_FIELDS), sums))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        q.put((rank, "error", repr(e), None))


def test_world2_reference_view_allreduce():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = {}
    for _ in range(world):
        r = q.get(timeout=240)
        out[r[0]] = r
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in range(world):
        assert out[r][1] == "ok", out[r][2]
    total = {f: sum(out[r][3][f] for r in range(world)) for f in D.REF_FIELDS}
    assert out[0][2] == out[1][2] == total
    # connections are rank-local, so the sum of the ranks' views is the view of the whole job's connections
    exp = {f: sum(_rank_view(world, r)[1][f] for r in range(world)) for f in D.REF_FIELDS}
    assert total == exp and total["buffers_failed"] > 0 and total["bytes_after_failure"] > 0
