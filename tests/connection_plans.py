"""What the connection tests (tests/test_connections_cpu.py, tests/test_connections_gpu.py) share: the close sizes the
issue sets and the reorderings of the reference-view plans (tests/refview_plans.py), worked out on the CPU."""
import numpy as np

EMPTY = 0xFFFFFFFF


def expected_bytes(table, slots):
    """Each connection's own total (received + after failure), except that among the clean connections every third
    gets its total + 1 and every fifth its total - 1 (a connection that is both keeps the + 1)."""
    want = table["bytes_recv"].astype(np.int64) + table["bytes_after_failure"].astype(np.int64)
    clean = np.nonzero(np.asarray(slots) == EMPTY)[0]
    third, fifth = clean[::3], clean[::5]
    want[third] += 1
    want[fifth[~np.isin(fifth, third)]] -= 1
    return want.astype(np.uint64)


def first_failed_buffers(slots, ordinals):
    """Per connection the index (into the plan's descriptors) of its first failing buffer, -1 for a clean one: the
    buffer whose ordinal its slot holds."""
    ordinals = np.asarray(ordinals, dtype=np.int64)
    where = np.full(int(ordinals.max()) + 1, -1, dtype=np.int64)
    where[ordinals] = np.arange(len(ordinals))
    slots = np.asarray(slots, dtype=np.int64)
    return np.where(slots == EMPTY, -1, where[np.minimum(slots, len(where) - 1)])


def slots_under(slots, ordinals, order):
    """The slots of the same failures when the plan's buffers are handed in as descs[order] with ordinals = positions
    (a reordering that keeps every connection's stream order keeps its first failing buffer)."""
    first = first_failed_buffers(slots, ordinals)
    pos = np.full(len(ordinals), -1, dtype=np.int64)
    pos[order] = np.arange(len(order))
    out = np.where(first < 0, EMPTY, pos[np.maximum(first, 0)])
    assert (out >= 0).all()
    return out.astype(np.uint32)


def buffer_major(n_conns, buffers_per_conn):
    """Buffer k of every connection, then buffer k + 1: neighbouring descriptors always differ in connection."""
    return np.arange(n_conns * buffers_per_conn, dtype=np.int64).reshape(n_conns, buffers_per_conn).T.reshape(-1)


def runs_of(n, n_conns, longest, rng):
    """conn_index[n] in runs of 1..longest buffers (lengths log-uniform, the first run the longest allowed, the second
    a single buffer); neighbouring runs differ in connection and the first n_conns runs visit every connection."""
    conn = np.zeros(n, dtype=np.uint32)
    first = rng.permutation(n_conns)
    at, last, k = 0, -1, 0
    while at < n:
        if k < n_conns:
            c = int(first[k])
        else:
            c = int(rng.integers(0, n_conns - 1))
            c += c >= last  # never the previous run's connection
        length = longest if k == 0 else 1 if k == 1 else int(np.exp(rng.uniform(0.0, np.log(longest))))
        conn[at:at + length] = c
        at, last, k = at + length, c, k + 1
    return conn
