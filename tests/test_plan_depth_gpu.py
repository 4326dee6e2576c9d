"""GPU: the tick planners of the three device-resident senders on long lists, idle runs and 64-bit slot sums.

The older sender tests stay within five tiles, prefixes of a few thousand and idle runs of two
(tests/test_plan_depths_cpu.py shows it). Here every case is built in tests/plan_depths.py for one path of the planning
-- 1 the scan's second pass, 2 prefixes above 2^32, 3 limb sums that carry, 4 ms_server_fill's search of prefix[]
beyond its staged window, 5 tcp_sender_descs' second grid-stride pass -- and plan_depths.facts, with the device's own
compute units and the engine's attributes, must show that the tick reaches it before anything is launched. Then the
device is compared with the numpy models of ctstraffic_amd/workload.py through the helpers of the three older files:
entries, codes, tick block, descriptors, lengths, counters and every byte of the arena or ring. The scratch's first
n + 1 words, prefix[0 .. n], are compared with the model's prefix as well. Every comparison is exact.

  path 1   test_long_list_tcp, test_long_list_tcp_paced, test_long_list_ms  (65 537 and 65 829 listed)
  path 2   test_wide_sums_tcp (plain and paced), test_wide_sums_ms
  path 3   test_wide_sums_tcp (plain and paced; ticks 1, 3 and 4)
  path 4   test_idle_runs_ms, test_idle_runs_ms_one_workgroup_per_cu
  path 5   test_descs_in_two_passes; the search over a long prefix[] also in test_idle_runs_tcp and the long lists

The exchange tick (tcp_exchange_sums / _scan / _apply, tcp_exchange_descs) takes paths 1, 2, 3 and the long search in
test_long_list_exchange, test_wide_sums_exchange and test_idle_runs_exchange, compared with the numpy model and with
plan_depths.exchange_tick (tests/test_tcp_exchange_gpu.py has its second grid-stride pass).
"""
import os

import numpy as np
import pytest
import torch

import plan_depths as P
from ctstraffic_amd import _lib
from ctstraffic_amd import workload as W
from test_media_stream_servers_gpu import QPC, _pair, _tick
from test_tcp_paced_senders_gpu import Pair as PacedPair
from test_tcp_senders_gpu import Pair as TcpPair

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ring_bpc():
    """The ring-fill blocks per CU of an engine created now (read from the environment at creation only)."""
    v = int(os.environ.get("CTS_RING_FILL_BLOCKS_PER_CU") or P.RING_BPC_DEFAULT)
    return v if v > 0 else P.RING_BPC_DEFAULT


def _tcp_facts(engine, w, capacity):
    return P.facts(w, capacity, "tcp", _cus(), blocks_per_cu=engine.get_attr(_lib.ATTR_BLOCKS_PER_CU))


def _same_prefix(table, prefix, wants, where):
    """The scratch's first n + 1 words (MsServerScratch / TcpTickScratch: prefix[0 .. n]) against the model's."""
    n = len(prefix)
    got = table.scratch[: n + 1].cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:n], np.asarray(prefix, dtype=np.uint64)), where
    assert int(got[n]) == sum(int(x) for x in wants) & P.M64, where


@pytest.fixture(scope="module")
def ring1_engine():
    """An engine whose ring-fill cap (read at creation only) is one workgroup per CU."""
    from ctstraffic_amd import Engine

    old = os.environ.get("CTS_RING_FILL_BLOCKS_PER_CU")
    os.environ["CTS_RING_FILL_BLOCKS_PER_CU"] = "1"
    try:
        eng = Engine(0)
    finally:
        if old is None:
            del os.environ["CTS_RING_FILL_BLOCKS_PER_CU"]
        else:
            os.environ["CTS_RING_FILL_BLOCKS_PER_CU"] = old
    yield eng
    eng.close()


# ---- A. long lists: the scan's second pass (path 1) ------------------------------------------------------------------
def _tcp_entries(case):
    entries = W.tcp_sender_entries(case["settings"])
    entries["finished"][list(case["finished"])] = 1
    return entries


@pytest.mark.parametrize("n_listed", P.LONG_LISTED)
def test_long_list_tcp(engine, n_listed):
    """256 full tiles, 256 tiles and one connection, 257 tiles and a ragged one; two ticks, the capacity 5 below the
    first tick's wants."""
    case = P.long_tcp(n_listed)
    f = _tcp_facts(engine, case["w"], case["capacity"])
    assert P.long_reaches(case, n_listed, f) == [] and f["search_steps_max"] >= 16, f
    p = TcpPair(engine, case["settings"], 16, case["capacity"], max_listed=n_listed, entries=_tcp_entries(case))
    state, seen = P.tcp_state(case["settings"], case["finished"]), set()
    for t in range(2):
        v = p.tick(case["ids"], 2, where="tick %d" % t)
        got = P.tcp_tick(state, case["ids"], 16, case["capacity"], 2)
        assert got["w"] == case["w"] or t
        _same_prefix(p.table, v.prefix, got["w"], "tick %d" % t)
        assert t or (3 in v.codes[-64:] and v.tick["buffers"] == case["capacity"])
        seen |= set(v.codes.tolist())
        assert n_listed == 65_536 or int(v.prefix[65_536]) > 0
    assert {0, 1, 2, 3, 4} <= seen


@pytest.mark.parametrize("n_listed", P.LONG_LISTED)
def test_long_list_tcp_paced(engine, n_listed):
    """The same through tcp_paced_sums / _scan / _apply: unpaced, rate-limited and burst entries by turns, ticks at
    the start and 4 ms on."""
    case = P.long_tcp(n_listed, paced=True)
    f = _tcp_facts(engine, case["w"], case["capacity"])
    assert P.long_reaches(case, n_listed, f) == [], f
    p = PacedPair(engine, case["settings"], case["pace"], 16, case["capacity"], start_ms=case["start"],
                  max_listed=n_listed, entries=_tcp_entries(case))
    seen = set()
    for t, now in enumerate(case["times"]):
        v = p.tick(case["ids"], 2, now, where="tick %d" % t)
        assert t or v.wanted.tolist() == case["w"]
        _same_prefix(p.table, v.prefix, v.wanted, "tick %d" % t)
        seen |= set(v.codes.tolist())
        # (4 ms on, all that still wants is the tail the capacity cut: the carry is the first tick's)
        assert t or n_listed == 65_536 or int(v.prefix[65_536]) > 0
    assert {0, 1, 2, 3, 4, 5} <= seen


@pytest.mark.parametrize("n_listed", P.LONG_LISTED)
def test_long_list_ms(engine, n_listed):
    """The servers' ms_server_sums / _scan / _apply and the ring fill over the same list lengths: frames of 1 or 2
    datagrams of at most 53 bytes, the capacity 3 below the first tick's wants."""
    case = P.long_ms(n_listed)
    f = P.facts(case["w"], case["capacity"], "ms", _cus(), ring_bpc=_ring_bpc())
    assert P.long_reaches(case, n_listed, f) == [], {k: v for k, v in f.items() if k != "prefixes"}
    entries = W.media_stream_server_entries(case["settings"])
    entries["finished"][list(case["finished"])] = 1
    table, view = _pair(engine, case["settings"], 64, case["capacity"], max_listed=n_listed, entries=entries)
    state = P.ms_state(case["settings"], case["finished"])
    for t in range(2):
        _tick(table, view, case["ids"], qpc=QPC + t, where="tick %d" % t)
        got = P.ms_tick(state, case["ids"], 64, case["capacity"])
        assert got["w"] == case["w"] or t
        _same_prefix(table, got["prefix"], got["w"], "tick %d" % t)
        assert t or (3 in view.codes[-64:] and 0 < view.tick["datagrams"] <= case["capacity"])


# ---- path 5: tcp_sender_descs past its first grid-stride pass --------------------------------------------------------
def test_descs_in_two_passes():
    """An engine of its own with blocks-per-CU 1: tcp_sender_descs' grid is at most one workgroup per CU, and the
    tick's buffers, sized from the CU count, are more than its lanes. The capacity lies above the total: descriptors
    past the total keep a marker."""
    from ctstraffic_amd import Engine

    cus = _cus()
    case = P.descs_two_passes(cus)
    f = P.facts(case["w"], case["capacity"], "tcp", cus, blocks_per_cu=1)
    assert P.descs_reaches(f) == [], f
    eng = Engine(0)
    try:
        eng.set_attr(_lib.ATTR_BLOCKS_PER_CU, 1)
        assert eng.get_attr(_lib.ATTR_BLOCKS_PER_CU) == case["blocks_per_cu"] == 1
        p = TcpPair(eng, case["settings"], 16, case["capacity"])
        p.descs["length"] = 0xA5A5A5A5
        p.table.descs.copy_(torch.from_numpy(p.descs.view(np.int64).copy()))
        v = p.tick(case["ids"], case["max_buffers"], where="two passes")
        _same_prefix(p.table, v.prefix, case["w"], "two passes")
        total = v.tick["buffers"]
        assert total == f["total"] > f["descs_grid"] * 256
        assert (p.descs["length"][total:] == 0xA5A5A5A5).all() and (p.descs["length"][:total] <= 16).all()
        # the slots of the second pass are other connections' than those of the first
        lanes = f["descs_grid"] * 256
        first, later = p.descs["conn_index"][:lanes], p.descs["conn_index"][lanes:total]
        assert len(set(later.tolist()) - set(first.tolist())) > 100
    finally:
        eng.close()


# ---- B. idle runs: the lookup beyond the staged window (path 4) ------------------------------------------------------
def _idle_ms(eng, ring_bpc, stride, full):
    cus = _cus()
    case = P.idle_runs_full("ms", stride, cus, ring_bpc) if full else P.idle_runs("ms", stride)
    f = P.facts(case["w"], case["capacity"], "ms", cus, ring_bpc=ring_bpc)
    assert P.idle_reaches(f, full) == [], {k: v for k, v in f.items() if k not in ("ring_batches", "prefixes")}
    entries = W.media_stream_server_entries(case["settings"])
    entries["finished"][case["finished"]] = 1
    table, view = _pair(eng, case["settings"], stride, case["capacity"], max_listed=len(case["ids"]), entries=entries)
    state = P.ms_state(case["settings"], case["finished"])
    for t in range(1 if full else 2):
        _tick(table, view, case["ids"], qpc=QPC - t, where="tick %d" % t)
        got = P.ms_tick(state, case["ids"], stride, case["capacity"])
        _same_prefix(table, got["prefix"], got["w"], "tick %d" % t)
        assert view.tick["datagrams"] == case["capacity"] and set(view.codes.tolist()) == {t, 2, 4}


@pytest.mark.parametrize("stride,full", [(64, False), (1040, False), (64, True)])
def test_idle_runs_ms(engine, stride, full):
    """[S, idle x 511, S, idle x 512, S, idle x 513, S, idle x 1500, S, S, idle x 700] and senders behind it, at the
    start of the list (two workgroups of one batch) and, `full`, at the start of the second workgroup of a tick in
    which every workgroup walks two batches (the session engine's ring: 512 x 4 x CUs + 77 slots of 64 bytes)."""
    _idle_ms(engine, _ring_bpc(), stride, full)


@pytest.mark.parametrize("stride", [64, 1040])
def test_idle_runs_ms_one_workgroup_per_cu(ring1_engine, stride):
    """The runs at the start of the second workgroup, on an engine with one ring-fill workgroup per CU; stride 1040 is
    the wave-uniform form of the store loop."""
    _idle_ms(ring1_engine, 1, stride, True)


@pytest.mark.parametrize("paced", [False, True])
def test_idle_runs_tcp(engine, paced):
    """The same list through tcp_sender_descs: one global search per slot over thousands of prefixes, the idle runs
    between two neighbouring slots' connections."""
    case = P.idle_runs("tcp", 64)
    w = case["w_paced"] if paced else case["w"]
    f = _tcp_facts(engine, w, case["capacity"])
    assert P.idle_descs_reaches(f) == [], f
    n = len(case["ids"])
    if paced:
        p = PacedPair(engine, case["settings"], case["pace"], 64, case["capacity"], start_ms=case["start"],
                      max_listed=n, entries=_tcp_entries(case))
        for t, now in enumerate((100, 104)):
            v = p.tick(case["ids"], 3, now, where="tick %d" % t)
            assert t or v.wanted.tolist() == w
            _same_prefix(p.table, v.prefix, v.wanted, "tick %d" % t)
    else:
        p = TcpPair(engine, case["settings"], 64, case["capacity"], max_listed=n, entries=_tcp_entries(case))
        state = P.tcp_state(case["settings"], case["finished"])
        for t in range(2):
            v = p.tick(case["ids"], 3, where="tick %d" % t)
            got = P.tcp_tick(state, case["ids"], 64, case["capacity"], 3)
            _same_prefix(p.table, v.prefix, got["w"], "tick %d" % t)
        assert v.tick["buffers"] == 0 and set(v.codes.tolist()) == {2, 4}


# ---- C. wide sums: prefixes above 2^32 and limb sums that carry (paths 2 and 3) --------------------------------------
@pytest.mark.parametrize("paced", [False, True])
def test_wide_sums_tcp(engine, paced):
    """[small, huge, huge, small, small, ...]: wants of 2 and 2^31 beside a capacity of 7, then wants of 0xFFFFFFFF
    beside a capacity of 0, one wave of 0xFFFFFFFF, and that wave in front of a second tile."""
    case = P.wide_tcp()
    n_max = max(len(t["ids"]) for t in case["ticks"])
    state = P.tcp_state(case["settings"])
    cut = P.pace_cut(case["pace"], 0, 0) if paced else None
    if paced:
        p = PacedPair(engine, case["settings"], case["pace"], 16, 7, start_ms=0, max_listed=n_max)
    else:
        p = TcpPair(engine, case["settings"], 16, 7, max_listed=n_max)
    for k, t in enumerate(case["ticks"]):
        got = P.tcp_tick(state, t["ids"], 16, t["capacity"], t["max_buffers"], cut)
        f = _tcp_facts(engine, got["w"], t["capacity"])
        assert P.wide_tcp_reaches(k, f) == [], (k, {x: y for x, y in f.items() if x != "prefixes"})
        args = (t["ids"], t["max_buffers"]) + ((0,) if paced else ())
        v = p.tick(*args, capacity=t["capacity"], where="tick %d" % k)
        assert [int(x) for x in v.prefix] == got["prefix"] and [int(x) for x in v.taken] == got["taken"], k
        _same_prefix(p.table, v.prefix, got["w"], "tick %d" % k)
        if k == 0:
            assert v.taken[:3].tolist() == [2, 5, 0] and set(v.codes[2:].tolist()) == {3}
            assert [int(x) for x in v.prefix[:4]] == [0, 2, 2 + (1 << 31), 2 + (1 << 32)]
            assert all((int(x) - 2) % (1 << 31) < 200 for x in v.prefix[1:])
        elif k == 1:
            assert v.tick["buffers"] == 0 and set(v.codes.tolist()) == {2, 3}
        else:
            assert v.taken[0] == 7 and set(v.codes[1:].tolist()) <= {2, 3} and int(v.prefix[1]) == 0xFFFFFFFF


def test_wide_sums_ms(engine):
    """60 frames of 0xFFFFFFFF bytes in datagrams of 53 between small ones: none fits, every small one behind the
    first gets code 3, and from the 53rd on the prefixes are above 2^32."""
    case = P.wide_ms()
    state = P.ms_state(case["settings"])
    entries = W.media_stream_server_entries(case["settings"])
    assert int(entries["datagrams_per_frame"][4]) == P.HUGE_DATAGRAMS and case["kinds"][4] == "h"
    n = len(case["ids"])
    table, view = _pair(engine, case["settings"], 64, case["capacity"], max_listed=n, entries=entries)
    for t in range(2):
        got = P.ms_tick(state, case["ids"], 64, case["capacity"])
        f = P.facts(got["w"], case["capacity"], "ms", _cus(), ring_bpc=_ring_bpc())
        assert P.wide_ms_reaches(case, f) == [], {k: v for k, v in f.items() if k != "prefixes"}
        _tick(table, view, case["ids"], qpc=QPC + t, where="tick %d" % t)
        _same_prefix(table, got["prefix"], got["w"], "tick %d" % t)
        assert view.codes.tolist() == [0] * 4 + [3] * (n - 4) and view.tick["datagrams"] == 8
        assert got["prefix"][-1] > 1 << 32


# ---- the exchange tick (tcp_exchange_sums / _scan / _apply, tcp_exchange_descs) on the same three cases --------------
def _exchange_pair(engine, case, capacity, n_listed):
    from test_tcp_exchange_gpu import Pair as ExchangePair

    entries = P.exchange_records(P.exchange_case_state(case))
    return ExchangePair(engine, case["settings"], case["stride"], capacity, max_listed=n_listed, entries=entries)


def _same_exchange_plan(p, v, got, where):
    """The model's tick v and the scratch's prefix[] against exchange_tick's result: the plan, the codes, the tick,
    the entries and, per written slot, receiver, length and pattern offset."""
    assert [int(x) for x in v.prefix] == got["prefix"] and [int(x) for x in v.taken] == got["taken"], where
    _same_prefix(p.table, v.prefix, got["w"], where)
    assert v.codes.tolist() == got["codes"] and v.tick == dict(got["tick"], bytes_dir=got["bytes_dir"]), where
    total = got["tick"]["buffers"]
    d = v.descs[:total]
    assert list(zip(d["conn_index"].tolist(), d["length"].tolist(),
                    d["expected_pattern_offset"].tolist())) == got["slots"], where
    assert np.array_equal(p.entries, P.exchange_records(got["entries"])), where


@pytest.mark.parametrize("n_listed", P.LONG_LISTED)
def test_long_list_exchange(engine, n_listed):
    """long_tcp's table with the patterns by turns, P and Q in 1..3B + 1, finished connections, two ids beyond the
    table, two with B above the stride, one entry with pattern 4, and a capacity 5 below the first tick's wants: a
    non-zero carry into the scan's second pass, a sender behind it, the tail cut; ticked to the end."""
    case = P.long_exchange(n_listed)
    f = _tcp_facts(engine, case["w"], case["capacity"])
    assert P.long_reaches(case, n_listed, f) == [] and f["search_steps_max"] >= 16, f
    p = _exchange_pair(engine, case, case["capacity"], n_listed)
    state, seen = P.exchange_case_state(case), set()
    for t in range(6):
        v = p.tick(case["ids"], 2, where="tick %d" % t)
        got = P.exchange_tick(state, case["ids"], 16, case["capacity"], 2, P.LONG_TABLE)
        assert got["w"] == case["w"] or t
        _same_exchange_plan(p, v, got, "tick %d" % t)
        assert t or (3 in v.codes[-64:] and v.tick["buffers"] == case["capacity"] and min(v.tick["bytes_dir"]) > 0)
        assert t or n_listed == 65_536 or int(v.prefix[65_536]) > 0
        seen |= set(v.codes.tolist())
        if v.tick["buffers"] == 0:
            break
    assert {0, 1, 2, 3, 4} <= seen and 2 <= t <= 4 and set(v.codes.tolist()) == {2, 4}


def test_idle_runs_exchange(engine):
    """The idle runs of 511, 512, 513 and 1500 through tcp_exchange_descs: finished connections, ids beyond the table,
    B above the stride and PushPull entries with push_bytes 0 between two slots' owners; every PushPull sender's three
    slots cross a turn. Two ticks."""
    case = P.idle_runs("exchange", 64)
    f = _tcp_facts(engine, case["w"], case["capacity"])
    assert P.idle_descs_reaches(f) == [], f
    n = len(case["ids"])
    p = _exchange_pair(engine, case, case["capacity"], n)
    state = P.exchange_case_state(case)
    for t in range(2):
        v = p.tick(case["ids"], 3, where="tick %d" % t)
        got = P.exchange_tick(state, case["ids"], 64, case["capacity"], 3, len(state))
        assert got["w"] == case["w"]
        _same_exchange_plan(p, v, got, "tick %d" % t)
        assert v.tick["buffers"] == case["capacity"] and set(v.codes.tolist()) == {t, 2, 4}
    assert (p.entries["finished"][[c for c, x in zip(case["ids"], case["w"]) if x]] == 1).all()


def test_wide_sums_exchange(engine):
    """wide_tcp's four ticks with 2^50-byte Push, Pull, PushPull and Duplex connections at B = 1: wants of 2^31 and
    0xFFFFFFFF from N - m beside capacities of 7 and 0."""
    case = P.wide_exchange()
    n_max = max(len(t["ids"]) for t in case["ticks"])
    state = P.exchange_case_state(case)
    p = _exchange_pair(engine, case, 7, n_max)
    n_conns = len(state)
    for k, t in enumerate(case["ticks"]):
        got = P.exchange_tick(state, t["ids"], 16, t["capacity"], t["max_buffers"], n_conns)
        f = _tcp_facts(engine, got["w"], t["capacity"])
        assert P.wide_tcp_reaches(k, f) == [], (k, {x: y for x, y in f.items() if x != "prefixes"})
        v = p.tick(t["ids"], t["max_buffers"], capacity=t["capacity"], where="tick %d" % k)
        _same_exchange_plan(p, v, got, "tick %d" % k)
        if k == 0:
            assert v.taken[:3].tolist() == [2, 5, 0] and set(v.codes[2:].tolist()) == {3}
            assert [int(x) for x in v.prefix[:4]] == [0, 2, 2 + (1 << 31), 2 + (1 << 32)]
        elif k == 1:
            assert v.tick["buffers"] == 0 and set(v.codes.tolist()) == {2, 3}
        else:  # seven buffers of one PushPull connection: both of its receivers
            assert v.taken[0] == 7 and int(v.prefix[1]) == 0xFFFFFFFF
            assert set(v.descs["conn_index"][:7].tolist()) == {t["ids"][0], t["ids"][0] + n_conns}
            assert min(v.tick["bytes_dir"]) >= 2
