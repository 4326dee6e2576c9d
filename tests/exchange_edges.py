"""Shared by tests/test_exchange_edges_cpu.py and tests/test_exchange_edges_gpu.py (CPU only, no device, no torch).

The exchange tick's closed forms (cts_tcp_exchange_math.hpp) at the top of 64 bits: shapes where P + B - 1, C = P + Q
and K = kp + kq pass 2^32, and positions where y * C, m * B, before + j and N - m lie above 2^63. Two tables of seeked
entries, one per stride, each ticked twice over a shuffled list; the reference is plan_depths.exchange_tick, plain
Python integers one connection at a time, never the numpy model. The cases are drawn with a fixed seed from the
product of the values below, behind hard-wired corners; tests/test_exchange_edges_cpu.py asserts what the list must
contain before the GPU file relies on it.
"""
import random

import numpy as np

import plan_depths as P

PUSH, PULL, PUSHPULL, DUPLEX = P.PUSH, P.PULL, P.PUSHPULL, P.DUPLEX
TOP = 1 << 64
MAX_BUFFERS = 5
TABLES = {1: dict(stride=16, sizes=(1, 2, 3, 15, 16), entries=2000),
          2: dict(stride=65536, sizes=(65531, 65536), entries=60)}
SEEK_KINDS = ("cycle_last", "cycle_far", "turn", "end_short", "end_exact", "zero", "random")
WALK_REACH = 4096  # buffers a CPU test walks one step at a time without thinking twice


def counts(B, Pb, Qb):
    """(kp, kq, K, C) in Python integers."""
    kp, kq = -(-Pb // B), -(-Qb // B)
    return kp, kq, kp + kq, Pb + Qb


def segment_values(B):
    return sorted(v for v in {1, B - 1, B, B + 1, 2 * B + 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 2, (1 << 32) - 1}
                  if 0 < v < 1 << 32)


def transfer_values(pattern, B, Pb, Qb):
    out = [TOP - 2, TOP - B, TOP - B - 1, 1 << 63, (1 << 63) + 1, (1 << 62) + 12345, 10 * (Pb + Qb) + Pb, 7 * B + 1]
    # (cts_tcp_exchange_init takes no Duplex transfer of 2^64 - 1: rounded up to even it has no 64-bit value)
    return [T for T in out if T != TOP - 1] if pattern == DUPLEX else [TOP - 1] + out


def total_buffers(pattern, T, B, Pb, Qb):
    from ctstraffic_amd import workload as W

    return W.tcp_exchange_total_buffers(pattern, T + (T % 2 if pattern == DUPLEX else 0), B, Pb, Qb)


def seek_of(kind, pattern, T, B, Pb, Qb, rng):
    """The position of seek kind `kind`, or None where the shape has no such position. A tick of MAX_BUFFERS from
    cycle_last / cycle_far (y * K - 2) crosses a cycle end, from turn (y * K + kp - 2) the push-to-pull turn;
    end_short (N - 3) ends short of MAX_BUFFERS, end_exact (N - 5) ends with them."""
    N = total_buffers(pattern, T, B, Pb, Qb)
    if kind == "zero":
        return 0
    if kind == "random":
        return rng.randrange(N)
    if kind in ("end_short", "end_exact"):
        back = 3 if kind == "end_short" else MAX_BUFFERS
        return N - back if N >= back else None
    if pattern != PUSHPULL:
        return None
    kp, _, K, _ = counts(B, Pb, Qb)
    if kind == "turn":
        if N < kp + 3 or kp < 2:
            return None
        y_max = (N - 3 - kp) // K
        return (y_max if rng.random() < 0.5 else rng.randrange(y_max + 1)) * K + kp - 2
    y_max = (N - 3) // K  # the largest y whose tick has room behind the cycle's end
    if kind == "cycle_last":
        return y_max * K - 2 if y_max >= 1 else None
    y_min = (1 << 40) // K + 1
    return rng.randrange(y_min, y_max + 1) * K - 2 if y_max >= y_min else None


def _corners(table):
    """The shapes and positions that must be there whatever the seed draws: (pattern, T, B, P, Q, seek kind or m)."""
    top32 = (1 << 32) - 1
    out = []
    if table == 1:
        for B in (1, 2, 16):
            out += [(DUPLEX, TOP - 2, B, 1, 1, kind) for kind in ("end_short", "end_exact", "zero", "random")]
        out += [(PUSH, TOP - 1, 1, 1, 1, "end_short"), (PULL, TOP - 1, 1, 1, 1, "end_exact"),
                (PUSH, TOP - 1, 3, 1, 1, "end_short"), (PULL, TOP - 2, 2, 1, 1, "end_short")]
        # K = 2^33 - 2, the widest divisor there is; K = 2^32 exactly; P + B - 1 above 2^32 beside a small Q
        shapes = [(TOP - 1, 1, top32, top32), (TOP - 2, 1, top32, top32), (TOP - 2, 2, top32, top32),
                  (TOP - 1, 2, top32, top32 - 1), (TOP - 1, 16, top32, 1), (TOP - 16, 16, top32 - 1, top32),
                  (TOP - 1, 3, top32, 1 << 31), (TOP - 16, 15, (1 << 31) + 1, top32), (1 << 63, 1, 1 << 31, 1 << 31),
                  ((1 << 63) + 1, 2, top32, 3)]
        for T, B, Pb, Qb in shapes:
            out += [(PUSHPULL, T, B, Pb, Qb, kind) for kind in SEEK_KINDS]
            # N - m a multiple of 2^32 and two more, and a multiple of 2^32 exactly: a want from 32 bits of N - m
            N = total_buffers(PUSHPULL, T, B, Pb, Qb)
            out += [(PUSHPULL, T, B, Pb, Qb, N - (3 << 32) - 2), (PUSHPULL, T, B, Pb, Qb, N - (1 << 32))]
        out += [(PUSH, TOP - 1, 1, 1, 1, TOP - 1 - (1 << 32) - 2), (DUPLEX, TOP - 2, 1, 1, 1, TOP - 2 - (1 << 33))]
    else:
        for T, B, Pb, Qb in [(TOP - 1, 65531, top32, top32 - 1), (TOP - 65536, 65536, top32, top32),
                             (TOP - 65537, 65536, top32 - 1, 65537), ((1 << 63) + 1, 65531, 1 << 31, top32)]:
            out += [(PUSHPULL, T, B, Pb, Qb, kind) for kind in ("cycle_last", "cycle_far", "turn", "end_short")]
        out += [(DUPLEX, TOP - 2, 65531, 1, 1, "end_short"), (PUSH, TOP - 1, 65531, 1, 1, "end_short"),
                (PULL, TOP - 65536, 65536, 1, 1, "end_exact"), (DUPLEX, TOP - 2, 65536, 1, 1, "random")]
    return out


_CASES = {}


def cases(table):
    """The entries of table 1 or 2: dicts with pattern, T, B, P, Q, m, kind (a seek kind, or "wired" for a hard-wired
    position), N, and for PushPull kp, K, C and the cycle y = m // K."""
    if table in _CASES:
        return _CASES[table]
    rng = random.Random(6400 + table)
    spec = TABLES[table]
    drawn = []
    for pattern, T, B, Pb, Qb, where in _corners(table):
        m = where if isinstance(where, int) else seek_of(where, pattern, T, B, Pb, Qb, rng)
        assert m is not None, (pattern, T, B, Pb, Qb, where)
        drawn.append((pattern, T, B, Pb, Qb, m, where if isinstance(where, str) else "wired"))
    while len(drawn) < spec["entries"]:
        B = rng.choice(spec["sizes"])
        pattern = rng.choice((PUSH, PULL, DUPLEX) + (PUSHPULL,) * 7)
        Pb, Qb = rng.choice(segment_values(B)), rng.choice(segment_values(B))
        T = rng.choice(transfer_values(pattern, B, Pb, Qb))
        kind = rng.choice(SEEK_KINDS)
        m = seek_of(kind, pattern, T, B, Pb, Qb, rng)
        if m is not None:
            drawn.append((pattern, T, B, Pb, Qb, m, kind))
    out = []
    for pattern, T, B, Pb, Qb, m, kind in drawn:
        case = dict(pattern=pattern, T=T, B=B, P=Pb, Q=Qb, m=m, kind=kind, N=total_buffers(pattern, T, B, Pb, Qb))
        if pattern == PUSHPULL:
            kp, _, K, C = counts(B, Pb, Qb)
            case.update(kp=kp, K=K, C=C, y=m // K)
        assert 0 <= m < case["N"] and B <= spec["stride"], case
        out.append(case)
    _CASES[table] = out
    return out


def all_cases():
    return cases(1) + cases(2)


def settings_of(table):
    return [(c["pattern"], c["T"], c["B"], c["P"], c["Q"]) for c in cases(table)]


def seeks_of(table):
    return [c["m"] for c in cases(table)]


def ticks_of(table):
    """The two ticks of a table: a shuffled list of every connection at MAX_BUFFERS; the first tick's capacity cuts
    the last few listed connections, the second runs them and five more buffers of everyone else."""
    n = len(cases(table))
    ids = list(range(n))
    random.Random(table).shuffle(ids)
    state = P.exchange_state(settings_of(table), seeks_of(table))
    stride = TABLES[table]["stride"]
    wants = sum(P.exchange_tick([list(e) for e in state], ids, stride, P.M32, MAX_BUFFERS, n)["w"])
    P.exchange_tick(state, ids, stride, wants - 12, MAX_BUFFERS, n)
    second = P.exchange_tick(state, ids, stride, P.M32, MAX_BUFFERS, n)
    return ids, (wants - 12, sum(second["w"]) + 3)  # (the second lies above its total: three descriptors stay)


_REFERENCE = {}


def reference(table, defect=None):
    """exchange_tick's results of the table's two ticks (with `defect`, what a build with that fault would leave)."""
    if (table, defect) in _REFERENCE:
        return _REFERENCE[(table, defect)]
    ids, capacities = ticks_of(table)
    state = P.exchange_state(settings_of(table), seeks_of(table))
    out = [P.exchange_tick(state, ids, TABLES[table]["stride"], capacity, MAX_BUFFERS, len(state), defect)
           for capacity in capacities]
    _REFERENCE[(table, defect)] = out
    return out


def compared(result):
    """What the GPU test compares of one tick's result, as one value: descriptor fields, codes, entry fields, the tick
    and its bytes by direction."""
    return (result["slots"], result["codes"], result["entries"], sorted(result["tick"].items()), result["bytes_dir"])


def arena_after(arena, slots, first_slot, stride):
    """arena (uint8, changed in place) with the buffers of exchange_tick's slots written from first_slot on: byte k of
    a buffer is the pattern's byte (offset + k) mod 65536."""
    from ctstraffic_amd import workload as W

    pattern = W._pattern_prefix(W.PATTERN_PERIOD)
    twice = np.concatenate([pattern, pattern])
    for g, (_, length, offset) in enumerate(slots):
        at = (first_slot + g) * stride
        arena[at:at + length] = twice[offset:offset + length]
    return arena


# ---- the walk from a position far out --------------------------------------------------------------------------------
def walk_from(pattern, T, B, Pb, Qb, m, count):
    """Up to `count` buffers (direction, stream position, length, intra) from buffer m on, by the step-by-step state
    machine workload.tcp_exchange_sequence started there: m is a whole number of buffers into its segment, so the
    machine at m is a fresh machine over what is left of the transfer whose first segment is what is left of the
    segment it stands in (its turn taken first), with every position moved up by what the directions have sent. Where
    it starts inside a segment the walk stops when that direction's turn comes again: the fresh machine's second
    segment of that kind would be the short one once more."""
    from ctstraffic_amd import workload as W

    out = []
    if pattern == DUPLEX:
        T += T % 2
    if pattern != PUSHPULL and m * B >= T:  # (nothing is left: m is N)
        return out, None
    if pattern in (PUSH, PULL):
        for d, pos, length, _ in W.tcp_exchange_sequence(pattern, T - m * B, B):
            out.append((d, pos + m * B, length, 0))
            if len(out) == count:
                break
        return out, [m * B * (1 - pattern), m * B * pattern]
    if pattern == DUPLEX:
        assert m % 2 == 0
        for d, pos, length, _ in W.tcp_exchange_sequence(pattern, T - m * B, B):
            out.append((d, pos + m // 2 * B, length, 0))
            if len(out) == count:
                break
        return out, [m // 2 * B] * 2
    kp, _, K, C = counts(B, Pb, Qb)
    y, r = divmod(m, K)
    if r < kp:  # in the push segment, r whole buffers in
        intra, flip = r * B, 0
        gone, base = y * C + intra, (y * Pb + intra, y * Qb)
        first, second = Pb - intra, Qb
    else:       # in the pull segment: the fresh machine's "push" is the pull
        intra, flip = (r - kp) * B, 1
        gone, base = y * C + Pb + intra, (y * Qb + intra, (y + 1) * Pb)
        first, second = Qb - intra, Pb
    if gone >= T:
        return out, None
    turns, last = 0, 0
    for d, pos, length, in_seg in W.tcp_exchange_sequence(PUSHPULL, T - gone, B, first, second):
        turns += d != last
        last = d
        if intra and turns == 2:
            break
        out.append((d ^ flip, pos + base[d], length, in_seg + (intra if turns == 0 else 0)))
        if len(out) == count:
            break
    return out, [base[flip], base[1 - flip]]


def walk_span(pattern, T, B, Pb, Qb, m, count):
    """walk_from, started again at every turn it stops at: (up to count buffers from m on, [bytes of direction 0, of
    direction 1] sent before buffer m)."""
    out, sent = [], None
    while len(out) < count:
        got, start = walk_from(pattern, T, B, Pb, Qb, m + len(out), count - len(out))
        sent = start if sent is None else sent
        if not got:
            break
        out += got
    return out, sent
