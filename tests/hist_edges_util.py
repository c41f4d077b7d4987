"""Inputs that pin the dataset histograms (csrc/pdp_hist.hip) at their edges.

Shared by tests/test_histogram_edges_host.py (CPU: the oracle against a plain
restatement) and tests/test_gpu_histogram_edges.py (GPU: every pairs phase and
the pre-aggregated path against the oracle).  Every builder returns
(pid, pk, val, U, P) as NumPy arrays and sizes, is deterministic, and asserts
on the CPU that the edge it aims at is really in the table: a table that
misses its target fails where it is built.

Exactness rule.  Every comparison made on these tables is an equality, so
every pair sum, every partition sum and every bin sum of the two float
histograms must be the same fp64 number in any summation order (the
reference adds in insertion order, NumPy pairwise, the kernels in the order
their atomics arrive).  check_exact() accepts a pair's or a partition's sum
only when it is a single term (one row per pair, one pair per partition) or
when all its terms are dyadic, k/8, with the |k| adding up to less than 2^53;
a bin's sum also when it has two terms (one rounded addition, which
commutes).  It adds the |k| in integers and raises otherwise.  Every builder
runs it.  The float-edge values are no k/8 (they are the lowers of a linspace
and their neighbours), so the values of one range are dealt out over as many
tables as it takes to leave at most two in any bin.

Three families:

float edges -- values on, one ulp below and one ulp above the lowers of
    np.linspace(min, max, 10001), which k_h_lowers / lin_lower / lin_bin
    restate with individually rounded operations; ranges narrower than 10,000
    ulps, where the lowers repeat and bisect_right must land on the last
    duplicate; min == max; the subnormal (STEP0) form.
logarithmic bins -- row counts and distinct counts at 999 / 1000 / 1009 /
    1010 / 9999 / 10000 / ... (log_bin_index and the host's index -> bounds),
    and waves of k_h_ids that hold several values of two wide bins
    (int_hist_add_wave).
structure -- row counts and partition counts on both sides of every boundary
    of the two-level partition, with a row that no other row shares a key
    with at every boundary index.
"""
import numpy as np

N_LOWERS = 10001  # NUMBER_OF_BUCKETS_SUM_HISTOGRAM + 1 (computing_histograms.py:25)
ULP1 = 2.0 ** -52  # the ulp of [1, 2)


# ------------------------------------------------------------ exactness --
def _dyadic(x):
    """(is k/8 with |k| < 2^53, k) per element"""
    k8 = x * 8.0  # a power of two: exact unless it overflows
    ok = np.isfinite(k8) & (np.abs(k8) < 2.0 ** 53) & (np.floor(k8) == k8)
    return ok, np.where(ok, k8, 0.0).astype(np.int64)


def _check_bins(name, sums):
    """the bins of one float histogram over `sums` (exact already): two terms
    at most, or k/8 terms whose |k| stay below 2^53"""
    mn, mx = sums.min(), sums.max()
    if mn == mx:
        idx = np.zeros(len(sums), dtype=np.int64)
    else:
        lowers = np.linspace(mn, mx, N_LOWERS)
        idx = np.searchsorted(lowers, sums, side="right") - 1
        idx[sums == mx] = N_LOWERS - 2
    ok, k = _dyadic(sums)
    rows = np.bincount(idx)
    multi = rows[idx] > 2
    if not ok[multi].all():
        raise ValueError(f"a bin of the {name} sums holds more than two values that are not all k/8")
    s = np.zeros(len(rows), dtype=np.float64)  # fp64: only its size matters here
    np.add.at(s, idx[multi], np.abs(k[multi]).astype(np.float64))
    if s.max(initial=0.0) >= 2.0 ** 52:
        raise ValueError(f"a bin of the {name} sums adds |k| up to 2^52 or more")


def check_exact(pid, pk, val):
    """Raises unless every pair sum and every partition sum of the table is
    exact in any order -- a group (the rows of one pair; the rows of one
    partition) has one row, or all its values are k/8 and their |k| add up to
    less than 2^53 -- and every bin of the two float histograms over those
    sums as well (_check_bins).  Returns the largest sum of |k| over the
    groups of more than one row."""
    pid = np.asarray(pid, dtype=np.int64)
    pk = np.asarray(pk, dtype=np.int64)
    val = np.asarray(val, dtype=np.float64)
    if not np.isfinite(val).all():
        raise ValueError("non-finite value: the reference defines no histogram for it")
    dyadic, k = _dyadic(val)
    largest = 0
    pair_key = pid * (int(pk.max(initial=0)) + 1) + pk
    for name, key in (("pair", pair_key), ("partition", pk)):
        _, inv, rows = np.unique(key, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        multi = rows[inv] > 1
        if not dyadic[multi].all():
            raise ValueError(f"a {name} sums several values that are not all k/8: its sum depends on the order")
        if len(k) * int(np.abs(k[multi]).max(initial=0)) >= 1 << 62:
            raise ValueError("too many rows for the int64 bookkeeping of check_exact")
        s = np.zeros(len(rows), dtype=np.int64)
        np.add.at(s, inv[multi], np.abs(k[multi]))
        if int(s.max(initial=0)) >= 1 << 53:
            raise ValueError(f"a {name}'s sum of |k| reaches 2^53: an fp64 sum would round")
        largest = max(largest, int(s.max(initial=0)))
        _check_bins(name, np.bincount(inv, weights=val))  # exact: single terms or k/8
    return largest


def weight_sums_clear_of_half(pre):
    """The pre-aggregated L0 / L1 bins round a sum of 1 / n_partitions
    weights per distinct value (computing_histograms.py:81-102).  True when
    every such sum of a pre-aggregated table (hist_util.preaggregate's
    columns) lies more than 1e-6 from x.5, so that the rounding does not
    depend on the order of the additions.  Exact: Fractions."""
    from fractions import Fraction
    _, _, _, npart, ncontr = pre
    for col in (npart, ncontr):
        sums = {}
        for v, m in zip(np.asarray(col).tolist(), np.asarray(npart).tolist()):
            sums[v] = sums.get(v, Fraction(0)) + Fraction(1, m)
        for s in sums.values():
            if abs((s % 1) - Fraction(1, 2)) <= Fraction(1, 10 ** 6):
                return False
    return True


# ---------------------------------------------------------- float edges --
EDGE_INDEX = (0, 1, 2, 3, 4999, 5000, 5001, 9997, 9998, 9999, 10000)

# L = linspace(mn, mx, 10001) has L[9999] == L[10000] == mx (65 ulps wide)
DUP_LAST = (float.fromhex("-0x1.6a7e06f3358e8p+0"), float.fromhex("-0x1.6a7e06f3358a7p+0"))

FLOAT_RANGES = {
    "unit": (0.0, 1.0),
    "third": (-1.0 / 3.0, 2.0 / 3.0),
    "tenth_milli": (0.1, 0.1 + 1e-3),
    "huge": (-1e300, 1e300),
    "1e15": (1e15, 1e15 + 1.0),
    "ulp37": (1.0, 1.0 + 37 * ULP1),
    "ulp9999": (1.0, 1.0 + 9999 * ULP1),
    "ulp10000": (1.0, 1.0 + 10000 * ULP1),
    "ulp10001": (1.0, 1.0 + 10001 * ULP1),
    "dup_last": DUP_LAST,
    "subnormal": (-3 * 5e-324, 7 * 5e-324),  # delta / 10,000 underflows to 0: the STEP0 form
}
# narrower than 10,000 ulps (1e15: 8 ulps of 1/8): np.linspace repeats lowers
NARROW = ("1e15", "ulp37", "ulp9999", "dup_last", "subnormal")
# the three ranges of the fixture recorded from the reference
FIXTURE_RANGES = ("third", "ulp37", "dup_last")


def float_edge_values(name, n_uniform=200, n_on_lower=40):
    """The values of one range: each lower L[i], i in EDGE_INDEX, with its two
    fp64 neighbours, clipped into [mn, mx]; mn and mx; n_uniform seeded
    uniform values and n_on_lower seeded lowers.  Asserts that the range is
    finite, that at least 30 values equal a lower, that every L[i] is present, and the property the
    range is there for (repeated lowers; L[9999] == mx; a zero step)."""
    mn, mx = FLOAT_RANGES[name]
    assert mn < mx and np.isfinite(mx - mn), name
    L = np.linspace(mn, mx, N_LOWERS)
    assert L[0] == mn and L[-1] == mx and (np.diff(L) >= 0).all(), name
    vals = [mn, mx]
    for i in EDGE_INDEX:
        vals += [L[i], np.nextafter(L[i], -np.inf), np.nextafter(L[i], np.inf)]
    rng = np.random.default_rng(sorted(FLOAT_RANGES).index(name) + 100)
    vals += (rng.random(n_uniform) * (mx - mn) + mn).tolist()
    vals += L[rng.integers(0, N_LOWERS, n_on_lower)].tolist()
    val = np.clip(np.asarray(vals, dtype=np.float64), mn, mx)
    val = val[rng.permutation(len(val))]
    assert int(np.isin(val, L).sum()) >= 30, name
    assert all((val == L[i]).any() for i in EDGE_INDEX), name
    assert val.min() == mn and val.max() == mx
    if name in NARROW:
        assert (np.diff(L) == 0).any(), f"{name}: no repeated lower"
    if name == "dup_last":
        assert L[9999] == L[10000] == mx
    if name == "subnormal":
        assert (mx - mn) / (N_LOWERS - 1) == 0.0
    return val


def _one_row_per_pair_and_partition(val, seed):
    n = len(val)
    pid = np.arange(n, dtype=np.int64)
    pk = np.random.default_rng(seed).permutation(n).astype(np.int64)
    check_exact(pid, pk, val)
    return pid, pk, val, n, n


def float_edge_parts(name):
    """The distinct values of float_edge_values(name) dealt out over tables
    that each hold mn and mx (so each has the range's lowers) and at most two
    values per bin, the bin taken by Python's bisect as the reference does:
    then every bin sum is one rounded addition, the same in any order."""
    import bisect
    mn, mx = FLOAT_RANGES[name]
    L = np.linspace(mn, mx, N_LOWERS).tolist()

    def bin_of(v):
        return len(L) - 2 if v == L[-1] else bisect.bisect_right(L, v) - 1

    parts = []  # [values, {bin: rows}]
    for v in dict.fromkeys(float_edge_values(name).tolist()):
        if v in (mn, mx):
            continue
        b = bin_of(v)
        for vals, used in parts:
            if used.get(b, 0) < 2:
                break
        else:
            vals, used = [mn, mx], {bin_of(mn): 1}
            used[bin_of(mx)] = used.get(bin_of(mx), 0) + 1
            parts.append([vals, used])
        vals.append(v)
        used[b] = used.get(b, 0) + 1
    assert len(parts) <= 4, (name, len(parts))
    return [np.asarray(vals) for vals, _ in parts]


def float_edges(name):
    """Aims at k_h_lowers, lin_lower and lin_bin (and k_hp_float in the
    pre-aggregated path): one row per pair and one pair per partition, so the
    Linf-sum and the sum-per-partition histograms bin the same values --
    those of float_edge_values(name).  A list of tables (float_edge_parts)
    that together hold every distinct value."""
    parts = float_edge_parts(name)
    want = set(float_edge_values(name).tolist())
    assert set(np.concatenate(parts).tolist()) == want
    return [_one_row_per_pair_and_partition(v, 7 + j) for j, v in enumerate(parts)]


def float_constant():
    """Every value 0.1: min == max, so the lowers are [0.1, 0.1] and the one
    bin has lower == upper (k_h_lowers' n_lowers = 2 branch).  Two rows: a
    third 0.1 in the bin would make its sum depend on the order."""
    return _one_row_per_pair_and_partition(np.full(2, 0.1), 8)


def float_signed_zeros():
    """+0.0 and -0.0 mixed: min == max although the bit patterns differ (the
    kernels take min and max from order-preserving integer images, in which
    -0.0 < +0.0)."""
    val = np.where(np.arange(100) % 3 == 0, -0.0, 0.0)
    assert np.signbit(val).any() and not np.signbit(val).all()
    return _one_row_per_pair_and_partition(val, 9)


def float_edges_two_pairs():
    """The second variant: two pairs in each partition, values k/8, so the
    sum-per-partition histogram bins sums that differ from the pair sums.
    Pair sums span [-1250, 1250] (step 1/4: lower i is -1250 + i/4 exactly)
    and partition sums [0, 1250] (step 1/8: lower i is i/8 exactly), so every
    multiple of 1/4 (pairs) and every partition sum sits exactly on a lower;
    the partition sums include the lowers of EDGE_INDEX."""
    rng = np.random.default_rng(17)
    s8 = np.concatenate([np.asarray(EDGE_INDEX), rng.integers(0, 10001, 200)])  # partition sums, in 1/8
    x8 = rng.integers(s8 - 10000, 10001)                                      # first pair, in 1/8
    x8[0], x8[len(EDGE_INDEX) - 1] = -10000, 10000      # sums 0 and 1250: the pair range's two ends
    y8 = s8 - x8
    assert (np.abs(x8) <= 10000).all() and (np.abs(y8) <= 10000).all()
    m = len(s8)
    pk = np.repeat(np.arange(m, dtype=np.int64), 2)
    pid = np.arange(2 * m, dtype=np.int64)
    val = np.stack([x8, y8], 1).reshape(-1) / 8.0
    order = rng.permutation(2 * m)
    pid, pk, val = pid[order], pk[order], val[order]
    check_exact(pid, pk, val)
    psum = np.bincount(pk, weights=val)
    assert val.min() == -1250.0 and val.max() == 1250.0 and psum.min() == 0.0 and psum.max() == 1250.0
    assert np.array_equal(np.linspace(0.0, 1250.0, N_LOWERS), np.arange(N_LOWERS) / 8.0)
    assert np.array_equal(np.linspace(-1250.0, 1250.0, N_LOWERS), np.arange(N_LOWERS) / 4.0 - 1250.0)
    assert all((psum == i / 8.0).any() for i in EDGE_INDEX)
    assert int((val * 4 == np.floor(val * 4)).sum()) >= 30    # pair sums on a lower
    assert len(set(psum.tolist()) - set(val.tolist())) >= 30  # partition sums that are no pair sum
    return pid, pk, val, 2 * m, m


# ----------------------------------------------------- logarithmic bins --
LOG_COUNTS = (1, 2, 999, 1000, 1001, 1009, 1010, 1011, 9989, 9990, 9999, 10000, 10001, 10009, 10010, 10099,
              10100, 99999, 100000, 100999, 101000)
LOG_DISTINCT = (999, 1000, 1001, 1009, 1010, 3628, 3629)
# the d-tables of the fixture recorded from the reference (and one GPU table)
LOG_DISTINCT_SMALL = tuple(d for d in LOG_DISTINCT if d <= 1010)


def _short_dyadic(rng, n):
    """k/2 with |k| <= 6: dyadic, and short in a JSON fixture"""
    return rng.integers(-6, 7, n).astype(np.float64) / 2.0


def log_counts():
    """Aims at log_bin_index and the host's index -> (lower, upper): one
    (privacy id, partition) pair with c rows for every c in LOG_COUNTS, each
    pair with a privacy id and a partition of its own, so Linf, L1 and
    count-per-partition all see exactly LOG_COUNTS."""
    rng = np.random.default_rng(23)
    c = np.asarray(LOG_COUNTS)
    key = np.repeat(rng.permutation(len(c)).astype(np.int64), c)
    key = key[rng.permutation(len(key))]
    val = rng.integers(-8, 9, len(key)).astype(np.float64) / 8.0
    check_exact(key, key, val)
    assert sorted(np.bincount(key).tolist()) == sorted(LOG_COUNTS)
    return key, key.copy(), val, len(c), len(c)


def log_distinct(ds):
    """Aims at the L0 and count_privacy_id_per_partition bins (distinct counts
    per key, counted in the LDS pair tables): for every d in ds a privacy id
    with d distinct partitions and a partition with d distinct privacy ids,
    one row per pair, the blocks of different d on disjoint keys.  d = 3,629
    is one pair more than a privacy-id bucket's LDS table holds (kHbPidFill =
    3,628): the default call overflows and starts again with pair buckets."""
    rng = np.random.default_rng(29)
    pid, pk, base = [], [], 0
    for d in ds:
        # key base: the hub privacy id and the hub partition; base + 1 .. base + d: the others
        pid += [np.full(d, base), base + 1 + np.arange(d)]
        pk += [base + 1 + np.arange(d), np.full(d, base)]
        base += d + 1
    pid = np.concatenate(pid).astype(np.int64)
    pk = np.concatenate(pk).astype(np.int64)
    order = rng.permutation(len(pid))
    pid, pk = pid[order], pk[order]
    val = _short_dyadic(rng, len(pid))
    check_exact(pid, pk, val)
    pairs = np.unique(np.stack([pid, pk], 1), axis=0)
    assert len(pairs) == len(pid)  # one row per pair
    l0 = np.bincount(pairs[:, 0])
    npid = np.bincount(pairs[:, 1])
    assert sorted(l0[l0 > 1].tolist()) == sorted(ds) and sorted(npid[npid > 1].tolist()) == sorted(ds)
    return pid, pk, val, base, base


def log_wave_bins(key="partition"):
    """Aims at int_hist_add_wave: 140 partitions, the even ones with 1000 ..
    1009 rows (seven of each: bin [1000, 1010)), the odd ones with 1010 ..
    1019 (bin [1010, 1020)), so a wave of k_h_ids holds several values of two
    wide bins, interleaved; each row of a partition from another privacy id,
    so count_privacy_id_per_partition sees the same counts.  key =
    "privacy_id": the twin with the two key columns swapped (L1 and L0)."""
    rng = np.random.default_rng(31)
    counts = np.asarray([(1000 if j % 2 == 0 else 1010) + (j // 2) % 10 for j in range(140)])
    a = np.repeat(np.arange(140, dtype=np.int64), counts)
    b = np.concatenate([rng.permutation(2000)[:c] for c in counts]).astype(np.int64)
    order = rng.permutation(len(a))
    a, b = a[order], b[order]
    val = rng.integers(-8, 9, len(a)).astype(np.float64) / 8.0
    got = np.bincount(a)
    assert all(int((got[0::2] == 1000 + j).sum()) == 7 and int((got[1::2] == 1010 + j).sum()) == 7 for j in range(10))
    pid, pk, U, P = (b, a, 2000, 140) if key == "partition" else (a, b, 140, 2000)
    check_exact(pid, pk, val)
    return pid, pk, val, U, P


# the two bins of log_wave_bins: (lower, upper, count, sum, max)
WAVE_BINS = [(1000, 1010, 70, 7 * sum(range(1000, 1010)), 1009), (1010, 1020, 70, 7 * sum(range(1010, 1020)), 1019)]


# ------------------------------------------------------------ structure --
# rows per bucket, level-1 stage / level-2 window, tile (pdp_hist.hip: kHbRowsPerBucket, kHbStage = kHbWin,
# kHbTileRows) and one wave
ROW_BOUNDARIES = (64, 1536, 8192, 65536)
STRUCTURE_N = (1, 63, 64, 65,
               1535, 1536, 1537,        # one bucket / two
               8191, 8192, 8193,        # one level-1 stage and level-2 window / two
               65535, 65536, 65537,     # one tile / two
               98304, 98305,            # 64 buckets (one wave of k_hb_prange's runs) / 65
               393216, 393217,          # 256 buckets (one super-bucket) / 257
               1572864, 1572865)        # 1,024 buckets (1,024 range workgroups, per = 1) / 1,025 (per = 2)
STRUCTURE_P = (2048, 2049,              # one partition range / two
               4096, 4097,              # one pair-table region / two
               131072, 131073,          # 64 ranges (one wave chunk of k_hb_pid_pairs' range scan) / 65
               262144, 262145)          # 128 ranges (kHbRangeMax) / 129: per-pair partition atomics
STRUCTURE_P_ROWS = 20000


def structure_rows(n):
    """the row indices that carry a key and a value of their own"""
    idx = {0, n - 1}
    for b in ROW_BOUNDARIES:
        if b < n:
            idx |= {b - 1, b}
    return sorted(idx)


def structure(n, P=2000):
    """Aims at the kernels' boundaries (k_hb_count .. k_hb_prange, the pair
    table's regions): n rows of seeded uniform keys over n / 8 privacy ids
    and P partitions, values k/8 with |k| <= 8.  Each row at index 0, n - 1,
    b - 1 and b (b in ROW_BOUNDARIES, b < n) has a privacy id and a partition
    that no other row uses (the highest codes, so partition P - 1 is present)
    and a value beyond +-n, alternating in sign and growing in size: above
    any sum of the other rows, so those rows are the strict minimum and
    maximum of both float histograms and each sits in a bin alone.  Losing or
    doubling one of them moves a lower or a count-1 bin."""
    rng = np.random.default_rng(1000 + n % 997 + P)
    special = structure_rows(n)
    S = len(special)
    U0, P0 = max(n // 8, 1), P - S
    assert P0 >= 1
    pid = rng.integers(0, U0, n, dtype=np.int64)
    pk = rng.integers(0, P0, n, dtype=np.int64)
    val = rng.integers(-8, 9, n).astype(np.float64) / 8.0
    for j, i in enumerate(special):
        pid[i], pk[i] = U0 + j, P0 + j
        val[i] = (n + 1 + j) * (1.0 if j % 2 else -1.0)
    check_exact(pid, pk, val)
    sp = np.asarray(special)
    rest = np.ones(n, dtype=bool)
    rest[sp] = False
    assert not np.isin(pid[rest], pid[sp]).any() and not np.isin(pk[rest], pk[sp]).any()
    assert len(set(pid[sp].tolist())) == S and len(set(pk[sp].tolist())) == S
    assert np.abs(val[rest]).sum() < n + 1 and (pk == P - 1).any()
    return pid, pk, val, U0 + S, P
