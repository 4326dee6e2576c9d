"""GPU: the exchange tick at the top of 64 bits (tests/exchange_edges.py), against plan_depths.exchange_tick.

Every other exchange test takes its expectation from workload.tcp_exchange_view, whose closed form is the kernels' own
in numpy uint64. Here the expectation is Python integers one connection at a time, and the shapes are those where a
device build that keeps 32 bits of P + B - 1, of C = P + Q or of the division's K, 48 bits of before + j or 32 bits of
N - m gives another result (tests/test_exchange_edges_cpu.py shows that each does, and that the case list holds the
corners). Two tables of seeked entries, two ticks each over a shuffled list; the arena is pre-filled with 0xA5 and
every byte of it is compared, as are the entries, the codes, the 48-byte tick block, the sent block and every
descriptor. Every comparison is exact.
"""
import numpy as np
import pytest
import torch

import exchange_edges as E
import plan_depths as P
from ctstraffic_amd import workload as W
from ctstraffic_amd.types import DESC_DTYPE, TCP_EXCHANGE_DTYPE
from test_tcp_exchange_gpu import Pair, _ids

pytestmark = pytest.mark.gpu


def same_as_exchange_tick(table, ref, n_listed, first_slot, stride, arena, descs, sent, where):
    """The device's table after a tick against exchange_tick's result ref. arena, descs (numpy, updated in place) and
    sent (a dict, updated) are what the reference side has accumulated over the ticks so far."""
    torch.cuda.synchronize()
    total = ref["tick"]["buffers"]
    entries, codes, tick = table.read()
    want = P.exchange_records(ref["entries"])
    for f in TCP_EXCHANGE_DTYPE.names:
        assert np.array_equal(entries[f], want[f]), (where, f, np.nonzero(entries[f] != want[f])[0][:5].tolist())
    assert codes[:n_listed].tolist() == ref["codes"], where
    for f in W.TCP_SENDER_TICK_FIELDS:
        assert int(tick[f]) == ref["tick"][f], (where, f)
    assert tick["bytes_dir"].tolist() == ref["bytes_dir"] and int(tick["reserved"]) == 0, where
    sent["bytes_sent"] += ref["tick"]["bytes"]
    sent["buffers_sent"] += total
    sent["connections_finished"] += ref["tick"]["connections_finished"]
    assert table.read_sent() == sent, where
    d = descs[:total]
    d["byte_offset"] = (first_slot + np.arange(total, dtype=np.uint64)) * np.uint64(stride)
    d["conn_index"], d["length"], d["expected_pattern_offset"] = (np.array(x, dtype=np.uint32)
                                                                  for x in zip(*ref["slots"]))
    d["skip_head"] = 0
    got_arena, got_descs = table.read_arena()
    for f in DESC_DTYPE.names:
        bad = np.nonzero(got_descs[f] != descs[f])[0]
        assert bad.size == 0, (where, f, bad[:5].tolist(), got_descs[bad[:5]].tolist(), descs[bad[:5]].tolist())
    E.arena_after(arena, ref["slots"], first_slot, stride)
    assert np.array_equal(got_arena, arena), where


@pytest.mark.parametrize("table", [1, 2])
def test_edge_shapes(engine, table):
    """Table 1: stride 16, B in 1, 2, 3, 15, 16, about 2 000 entries. Table 2: stride 65536, B = 65531 and 65536,
    about 60. One tick of max_buffers 5 over a shuffled list, its capacity cutting the last few connections, and a
    second that runs the rest into the slots behind a gap of two."""
    stride = E.TABLES[table]["stride"]
    settings, seeks = E.settings_of(table), E.seeks_of(table)
    ids, capacities = E.ticks_of(table)
    n = len(settings)
    entries = W.tcp_exchange_entries(settings, seek=seeks)
    assert np.array_equal(entries, P.exchange_records(P.exchange_state(settings, seeks)))
    capacity = max(capacities)
    p = Pair(engine, settings, stride, capacity, arena_slots=capacity + 2, entries=entries)
    sent = dict.fromkeys(W.SENT_FIELDS, 0)
    dev_ids = _ids(ids)
    for t, ref in enumerate(E.reference(table)):
        first_slot = 2 * t
        p.table.send(dev_ids, E.MAX_BUFFERS, first_slot=first_slot, capacity=capacities[t])
        same_as_exchange_tick(p.table, ref, n, first_slot, stride, p.arena, p.descs, sent, "tick %d" % t)
    assert ref["tick"]["buffers"] == capacities[1] - 3 and 1 in ref["codes"] and 3 not in ref["codes"]
