"""Inputs that pin the value arithmetic of the bounding kernels exactly.

Two kinds of table, shared by tests/test_value_edges_host.py (CPU) and
tests/test_gpu_value_edges.py (GPU):

dyadic table -- values k/8 with integer |k| <= 2^12 and bounds that are
    multiples of 1/8.  Every clipped and every normalised value then has 3
    fraction bits and every square 6, so an fp64 sum of them is exact as long
    as its sum of |terms| stays below 2^53 units of 2^-6 -- whatever the order,
    the atomics or an FMA contraction.  check_exact() does not take that on
    trust: it adds the |terms| of every partition in integers and raises when
    the largest reaches 2^53.  About a third of the values lie below min_value
    and a third above max_value; rows exactly at min_value, max_value and
    middle are planted.

edge table -- a few thousand dyadic filler rows plus the values at which a
    clip or a conversion can go wrong (non-finite values, the three NaN
    encodings, the bounds and their fp64 neighbours, a subnormal, int64
    extremes, integers above 2^53, pairs whose raw sum overflows or wraps).
    Each edge kind owns one partition that holds nothing but that kind's
    values, so every partition's sums stay independent of the order of
    addition (equal terms, or a result that any order makes non-finite) and
    the comparison with the oracle is an equality there too.

plain_group_by() is the expected result when nothing is sampled, from the
rows alone: fractions.Fraction / Python ints for a dyadic table, one Python
float operation per element with np.clip's rule (a NaN stays NaN) for an edge
table.  It shares no code with oracle/columnar.py.
"""
import dataclasses
from fractions import Fraction

import numpy as np

from oracle import columnar as O

K_MAX = 1 << 12  # |value| <= K_MAX / 8
FIELDS = ("sum", "normalized_sum", "normalized_sum_sq")


@dataclasses.dataclass(frozen=True)
class Bounds:
    lo: float
    hi: float
    mid: float
    min_sum: float
    max_sum: float


# all multiples of 1/8; values span [-512, 512], so a third lies on each side
# of [lo, hi], and pair sums of two rows land on both sides of [min_sum, max_sum].
# middle lies off centre on purpose: the fp64 normalised values then span
# 1,929/8 .. 4,663/8 (13 significant bits), so most of their squares need more
# than the 24 bits of an fp32 significand -- a square taken in fp32 shows.
F64_BOUNDS = Bounds(-170.5, 171.25, -411.625, -200.25, 300.5)
I64_BOUNDS = Bounds(-170.0, 171.0, -411.5, -200.0, 300.0)
LO_EQ_HI = Bounds(2.5, 2.5, 2.5, 2.5, 2.5)
I64_LO_EQ_HI = Bounds(3.0, 3.0, 3.0, 3.0, 3.0)  # SUM_INT takes int64 bounds only
UNBOUNDED = Bounds(-np.inf, np.inf, 0.0, -np.inf, np.inf)


def bounds_for(value_kind):
    return I64_BOUNDS if value_kind == O.VALUE_I64 else F64_BOUNDS


def dyadic_values(rng, n, value_kind, b=None):
    """n values k/8 (integers for VALUE_I64), |k| <= K_MAX, with planted rows
    exactly at lo, hi and middle (middle rounded down for integer values)."""
    b = b or bounds_for(value_kind)
    if value_kind == O.VALUE_NONE:
        return None
    if value_kind == O.VALUE_I64:
        val = rng.integers(-K_MAX // 8, K_MAX // 8 + 1, n, dtype=np.int64)
        plant = np.array([int(b.lo), int(b.hi), int(np.floor(b.mid))], dtype=np.int64)
    else:
        val = rng.integers(-K_MAX, K_MAX + 1, n).astype(np.float64) / 8.0
        plant = np.array([b.lo, b.hi, b.mid])
    where = rng.random(n) < 3.0 / 32.0
    val[where] = plant[rng.integers(0, 3, int(where.sum()))]
    return val


def check_exact(pk, val, P, b):
    """Raises unless every fp64 sum over a dyadic table is exact: the largest
    per-partition sum of |terms|, over all rows (a superset of the kept ones)
    and in units of 2^-6, must stay below 2^53.  Integer arithmetic only."""
    if val is None:
        return 0
    k8 = np.asarray(val, dtype=np.float64) * 8.0
    k = k8.astype(np.int64)
    if not np.array_equal(k.astype(np.float64), k8) or int(np.abs(k).max(initial=0)) > K_MAX:
        raise ValueError("not a dyadic table: values must be k/8 with |k| <= 2^12")
    ib = {}
    for name in ("lo", "hi", "mid", "min_sum", "max_sum"):
        f = Fraction(getattr(b, name)) * 8
        if f.denominator != 1:
            raise ValueError(f"{name} is no multiple of 1/8")
        ib[name] = int(f)
    n = len(k)
    worst_term = max(8 * (K_MAX + abs(ib["mid"])), (K_MAX + abs(ib["mid"])) ** 2)
    if n * worst_term >= 1 << 62:
        raise ValueError("too many rows for the int64 bookkeeping of check_exact")
    ck = np.clip(k, ib["lo"], ib["hi"])
    nk = ck - ib["mid"]
    largest = 0
    # units of 2^-6: a value k/8 is 8k of them, a square (k/8)^2 is k^2
    for terms in (8 * np.abs(k), 8 * np.abs(ck), 8 * np.abs(nk), nk * nk):
        s = np.zeros(P, dtype=np.int64)
        np.add.at(s, pk, terms)
        largest = max(largest, int(s.max(initial=0)))
    if largest >= 1 << 53:
        raise ValueError(f"sum of |terms| reaches {largest} >= 2^53 units of 2^-6: fp64 sums would round")
    return largest


def filler_bounds(value_kind, b):
    """The bounds that dyadic filler rows are drawn and checked against: b
    itself, or, where b is infinite (no clip: the raw values are summed), the
    kind's default bounds widened to the whole value range."""
    if np.isfinite(b.lo) and np.isfinite(b.hi):
        return b
    return dataclasses.replace(bounds_for(value_kind), lo=-K_MAX / 8, hi=K_MAX / 8, mid=0.0)


def dyadic_table(seed, n, U, P, value_kind, skew=False, b=None):
    """(pid, pk, val) with the key columns of tests.test_gpu_kernels._gen and
    dyadic values, checked by check_exact."""
    b = b or bounds_for(value_kind)
    rng = np.random.default_rng(seed)
    pid = rng.integers(0, U, n, dtype=np.int64)
    if skew:
        pk = np.minimum(rng.zipf(1.3, n) - 1, P - 1).astype(np.int64)
    else:
        pk = rng.integers(0, P, n, dtype=np.int64)
    val = dyadic_values(rng, n, value_kind, b)
    check_exact(pk, val, P, b)
    return pid, pk, val


# ------------------------------------------------------------ edge values --
def _f64_bits(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


NAN_KINDS = ("nan_quiet", "nan_signalling", "nan_all_ones")
# fp64 neighbours of lo / hi have 53 significant bits and SUM_PER_PARTITION adds
# them unclipped, so a sum of several would depend on the order: these kinds
# hold their one dedicated row and nothing else (0 + c = c in any order)
SINGLE_ROW_KINDS = ("under_lo", "over_hi")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def edge_kinds(value_kind, b):
    """[(name, values of one pair)]; fp64 values as bit patterns, so that the
    NaN encodings reach the device as written."""
    if value_kind == O.VALUE_I64:
        return [("minus_one_all_ones", [-1]), ("int64_min", [I64_MIN]), ("int64_max", [I64_MAX]),
                ("above_2^53", [(1 << 53) + 1]), ("below_-2^53", [-(1 << 53) - 1]), ("zero", [0]),
                ("lo", [int(b.lo)]), ("hi", [int(b.hi)]), ("under_lo", [int(b.lo) - 1]), ("over_hi", [int(b.hi) + 1]),
                ("wrap_up", [I64_MAX, I64_MAX]),  # raw int sum wraps to -2
                ("wrap_down", [I64_MIN, -1])]     # raw int sum wraps to INT64_MAX
    kinds = []
    if np.isfinite(b.lo) and np.isfinite(b.hi):
        kinds += [("lo", [b.lo]), ("hi", [b.hi]), ("under_lo", [np.nextafter(b.lo, -np.inf)]),
                  ("over_hi", [np.nextafter(b.hi, np.inf)]),
                  # (every pair sum of these stays outside [min_sum, max_sum]: clipped either way)
                  ("under_min_sum", [np.nextafter(min(b.min_sum, b.lo), -np.inf)]),
                  ("over_max_sum", [np.nextafter(max(b.max_sum, b.hi), np.inf)])]
    kinds += [("plus_zero", [0.0]), ("minus_zero", [-0.0]), ("plus_inf", [np.inf]), ("minus_inf", [-np.inf]),
              ("plus_1e308", [1e308]), ("minus_1e308", [-1e308]), ("subnormal", [5e-324])]
    out = [(name, [_f64_bits(v) for v in vals]) for name, vals in kinds]
    out += [("nan_quiet", [_f64_bits(np.nan)]), ("nan_signalling", [0x7FF0000000000001]),
            ("nan_all_ones", [0xFFFFFFFFFFFFFFFF]),  # the row sketches' empty sentinel
            ("inf_minus_inf", [_f64_bits(np.inf), _f64_bits(-np.inf)]),  # raw pair sum NaN
            ("overflow", [_f64_bits(1e308), _f64_bits(1e308)])]  # raw pair sum +inf
    return out


@dataclasses.dataclass
class EdgeTable:
    pid: np.ndarray
    pk: np.ndarray
    val: np.ndarray
    partition: dict   # kind name -> its partition
    dedicated: list   # (privacy id, partition, rows) of the pairs that are certainly kept
    first_edge_partition: int


def edge_table(seed, U, P, value_kind, b, l0, linf, n_fill=3000, fill_ids=200, fill_partitions=50):
    """Dyadic filler over `fill_ids` privacy ids (many rows each, so they are
    sampled) and the first `fill_partitions` partitions; kind j owns partition
    P - E + j.  Its values sit once in a privacy id of their own (the last E
    ids: one partition <= l0, <= linf rows per pair, so certainly kept) and six
    times in rows of the sampled ids (SINGLE_ROW_KINDS: the dedicated row only)."""
    rng = np.random.default_rng(seed)
    kinds = edge_kinds(value_kind, b)
    E = len(kinds)
    fill_ids = min(fill_ids, U - E)
    assert U - E >= fill_ids and P - E >= fill_partitions, (U, P, E)
    dt = np.int64 if value_kind == O.VALUE_I64 else np.uint64
    pid = [rng.integers(0, fill_ids, n_fill, dtype=np.int64)]
    pk = [rng.integers(0, fill_partitions, n_fill, dtype=np.int64)]
    fill = dyadic_values(rng, n_fill, value_kind)
    check_exact(pk[0], fill, P, filler_bounds(value_kind, b))
    val = [fill if value_kind == O.VALUE_I64 else fill.view(np.uint64)]
    partition, dedicated = {}, []
    for j, (name, vals) in enumerate(kinds):
        p, u = P - E + j, U - E + j
        partition[name] = p
        own = vals if (linf == 0 or linf >= len(vals)) else vals[:linf]
        dedicated.append((u, p, len(own)))
        pid.append(np.full(len(own), u, dtype=np.int64))
        pk.append(np.full(len(own), p, dtype=np.int64))
        val.append(np.array(own, dtype=dt))
        reps = 0 if name in SINGLE_ROW_KINDS and value_kind != O.VALUE_I64 else 6
        pid.append(rng.integers(0, fill_ids, reps, dtype=np.int64))
        pk.append(np.full(reps, p, dtype=np.int64))
        val.append(np.array([vals[i % len(vals)] for i in range(reps)], dtype=dt))
    pid, pk, val = np.concatenate(pid), np.concatenate(pk), np.concatenate(val)
    perm = rng.permutation(len(pid))
    val = val[perm]
    if value_kind != O.VALUE_I64:
        val = val.view(np.float64)
    return EdgeTable(pid[perm], pk[perm], val, partition, dedicated, P - E)


# ----------------------------------------------------- plain expectation --
def _clip(v, lo, hi):
    """np.clip on one number: a NaN stays NaN."""
    if v != v:
        return v
    return min(max(v, lo), hi)


def _wrap64(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def plain_group_by(pid, pk, val, P, value_kind, flags, b, exact):
    """The accumulators when nothing is sampled: every row of every (privacy
    id, partition) pair counts.  exact: Fractions (dyadic tables; the result
    is converted once, so it is the true sum); otherwise Python floats, one
    operation per element in row order.  Integer sums wrap modulo 2^64."""
    num = (lambda x: Fraction(x)) if exact else float
    lo, hi, mid = num(b.lo), num(b.hi), num(b.mid)
    pairs = {}
    for u, k, i in zip(pid.tolist(), pk.tolist(), range(len(pk))):
        pairs.setdefault((u, k), []).append(i)
    zero = num(0)
    pidc, cnt = [0] * P, [0] * P
    isum, fsum, nsum, nsum2 = [0] * P, [zero] * P, [zero] * P, [zero] * P
    ints = val.tolist() if value_kind == O.VALUE_I64 else None
    flts = None if val is None else [num(x) for x in np.asarray(val, dtype=np.float64).tolist()]
    for (u, k), rows in pairs.items():
        pidc[k] += 1
        cnt[k] += len(rows)
        if val is None:
            continue
        if flags & O.SUM_PER_PARTITION:
            if flags & O.SUM_INT:
                raw = 0
                for i in rows:
                    raw = _wrap64(raw + ints[i])
                isum[k] = _wrap64(isum[k] + _clip(raw, int(b.min_sum), int(b.max_sum)))
            else:
                raw = zero
                for i in rows:
                    raw = raw + flts[i]
                fsum[k] = fsum[k] + _clip(raw, num(b.min_sum), num(b.max_sum))
        for i in rows:
            c = _clip(flts[i], lo, hi)
            if not flags & O.SUM_PER_PARTITION:
                if flags & O.SUM_INT:
                    isum[k] = _wrap64(isum[k] + _clip(ints[i], int(b.lo), int(b.hi)))
                else:
                    fsum[k] = fsum[k] + c
            nc = c - mid
            nsum[k] = nsum[k] + nc
            nsum2[k] = nsum2[k] + nc * nc
    has_sum = flags & (O.ACC_SUM | O.SUM_PER_PARTITION)
    out = {"privacy_id_count": np.array(pidc, dtype=np.int64), "count": np.array(cnt, dtype=np.int64)}
    if flags & O.SUM_INT:
        out["sum"] = np.array(isum if has_sum else [0] * P, dtype=np.int64)
    else:
        out["sum"] = np.array([float(x) for x in fsum]) if has_sum else np.zeros(P)
    out["normalized_sum"] = np.array([float(x) for x in nsum]) if flags & O.ACC_NSUM else np.zeros(P)
    out["normalized_sum_sq"] = np.array([float(x) for x in nsum2]) if flags & O.ACC_NSUM2 else np.zeros(P)
    return out


def assert_exactly_equal(got, want):
    """Counts, int sums and fp64 fields by equality (NaN equals NaN, +0 equals
    -0: np.testing.assert_array_equal); a field the run does not carry (None)
    is skipped."""
    np.testing.assert_array_equal(got["privacy_id_count"], want["privacy_id_count"])
    np.testing.assert_array_equal(got["count"], want["count"])
    for k in FIELDS:
        if got.get(k) is None:
            continue
        assert got[k].dtype == want[k].dtype, (k, got[k].dtype, want[k].dtype)
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
