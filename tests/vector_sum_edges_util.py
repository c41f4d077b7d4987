"""Host side of the VECTOR_SUM edge tests: restatements and constructed inputs.

Shared by tests/test_vector_sum_edges_host.py (CPU: proves everything here)
and tests/test_gpu_vector_sum_edges.py (GPU: compares k_vs_* of pdp_pairs.hip
and k_vector_sum_metrics of pdp_select.hip with it by equality).

accumulate()       np.add.at of the kept rows' vectors.
clip_rows()        k_vector_sum_metrics' clip in fp64, in the kernel's order: a
                   lane's coordinates j = lane, lane + 64, ... one after the
                   other, then the xor butterfly over the 64 lanes.
clip_rows_exact()  the same quantity in fractions.Fraction; clip_bound() is
                   the derived distance between the two on non-dyadic input.
oracle_kept()      which rows oracle.columnar.bound_and_reduce keeps, decoded
                   from its own integer sums.
geometry()         the lane layout pairs_vector_sum chooses for (d, alignment).
The builders assert what their tables are for: a table that stops exercising
its edge fails on the CPU, it does not pass silently on the GPU.
"""
import fractions
import functools
import math

import numpy as np

from oracle import columnar as O

U53 = 2.0**-53
MAX_D = 4096          # PDP_MAX_VECTOR_SIZE
MAX_ENTRY = 1 << 20   # |entry| of every integer table
KINDS = ("l1", "l2")
NOISE_SEED = 0xC0FFEE1234567  # above 2^32: both key words of the Philox streams are non-zero


# ---------------------------------------------------------- restatements --
def accumulate(pk, vec, P, kept=None):
    """[P, d]: the sums of the kept rows' vectors per partition (kept: a bool
    mask over the rows; None: every row)."""
    pk, vec = np.asarray(pk, np.int64), np.asarray(vec, np.float64)
    if kept is not None:
        pk, vec = pk[kept], vec[kept]
    out = np.zeros((int(P), vec.shape[1]), np.float64)
    np.add.at(out, pk, vec)
    return out


def _wave_sum(terms):
    """The kernel's order over [rows, d] non-negative terms: lane l adds its
    coordinates l, l + 64, ... to 0.0 in turn, then `s += shfl_xor(s, o)` for
    o = 32 ... 1, after which every lane holds the same bits; lane 0's."""
    rows, d = terms.shape
    trips = (d + 63) // 64
    padded = np.zeros((rows, trips * 64), np.float64)
    padded[:, :d] = terms
    s = np.zeros((rows, 64), np.float64)
    for t in range(trips):
        s = s + padded[:, t * 64:(t + 1) * 64]
    lanes = np.arange(64)
    o = 32
    while o:
        s = s + s[:, lanes ^ o]
        o >>= 1
    assert (s.view(np.int64) == s[:, :1].view(np.int64)).all() or np.isnan(s).any()
    return s[:, 0]


def clip_rows(vacc, index, kind, max_norm):
    """out[i] = vacc[index[i]] clipped as k_vector_sum_metrics clips it: Linf by
    np.clip; L1 / L2 by x * coef, coef = fmin(1, max_norm / norm) with norm =
    sum |x| resp. sqrt(sum x * x).  fmin ignores a NaN, so coef is 1 when the
    quotient is inf or NaN: the zero vector (with or without max_norm == 0)
    and a vector with a NaN coordinate."""
    x = np.asarray(vacc, np.float64)
    index = np.asarray(index, np.int64)
    if kind == "linf":
        return np.clip(x, -max_norm, max_norm)[index]
    assert kind in KINDS, kind
    with np.errstate(all="ignore"):
        s = _wave_sum(np.abs(x) if kind == "l1" else x * x)
        norm = s if kind == "l1" else np.sqrt(s)
        coef = np.fmin(1.0, np.float64(max_norm) / norm)
        out = x * coef[:, None]
    return out[index]


def _sqrt_fraction(s, bits=160):
    """sqrt of the Fraction s >= 0, rounded down to a multiple of
    2^-bits / denominator: sqrt(a / b) = sqrt(a b) / b, and math.isqrt of
    a b 4^bits is exact to one unit, a relative error below 2^-bits for
    a b >= 1."""
    a, b = s.numerator, s.denominator
    return fractions.Fraction(math.isqrt(a * b << (2 * bits)), b << bits)


def clip_rows_exact(vacc, index, kind, max_norm):
    """clip_rows in exact arithmetic for finite input: norm and coef as
    Fractions (the L2 square root to 160 bits), every product rounded to fp64
    once, by float(Fraction), which rounds correctly."""
    x = np.asarray(vacc, np.float64)
    assert np.isfinite(x).all()
    index = np.asarray(index, np.int64)
    if kind == "linf":
        return np.clip(x, -max_norm, max_norm)[index]
    assert kind in KINDS, kind
    out = np.empty_like(x)
    m = fractions.Fraction(float(max_norm))
    for r, row in enumerate(x.tolist()):
        fr = [fractions.Fraction(v) for v in row]
        s = sum(abs(v) for v in fr) if kind == "l1" else sum(v * v for v in fr)
        norm = s if kind == "l1" else _sqrt_fraction(s)
        coef = min(fractions.Fraction(1), m / norm) if norm else fractions.Fraction(1)
        out[r] = [float(v * coef) for v in fr]
    return out[index]


def clip_bound(d):
    """Relative bound on |device - clip_rows_exact| per coordinate for finite
    non-dyadic input, u = 2^-53, valid while (2 d + 4) u < 1:

        clip_bound(d) = (d + 4) u / (1 - (2 d + 4) u)

    The device's s is a sum of d non-negative terms, each a product rounded
    once (|x| is exact) or fused into its addition; whatever the order, a term
    passes through at most d - 1 inexact additions (adding 0.0 is exact), so
    s^ = s (1 + t), |t| <= g = d u / (1 - d u) (Higham, Accuracy and Stability,
    lemma 3.1 and section 4.2).  Then
      L1: coef^ = (M / s^)(1 + e1), out^ = x coef^ (1 + e2), and the exact
          reference rounds once more (e3), |e_i| <= u.  min(1, .) is exact and
          keeps a relative error (it is monotone and 1 is exact).  So
          out^ / out <= (1 + u)^3 / (1 - g) <= (1 - d u) / ((1 - 2 d u)(1 - 3 u))
          <= 1 + (d + 3) u / (1 - (2 d + 3) u).
      L2: norm^ = sqrt(s^)(1 + e0); the square root halves t:
          (1 - g)^(-1/2) <= 1 + d u / (2 (1 - 2 d u)), and four roundings
          remain, so out^ / out <= 1 + (d / 2 + 4) u / (1 - (2 d + 4) u).
    The lower sides (1 - u)^3 / (1 + g) and (1 - u)^3 / ((1 + u) sqrt(1 + g))
    are closer to 1 than the upper ones.  (d + 4) u / (1 - (2 d + 4) u) is at
    least both; one expression serves both norms."""
    assert (2 * d + 4) * U53 < 1
    return (d + 4) * U53 / (1 - (2 * d + 4) * U53)


def same_bits(got, want):
    """Equality that pins the sign of a zero: NaN wherever `want` is NaN
    (payload and sign of a NaN are not compared: inf * 0 makes the
    platform's default NaN), the same bits everywhere else."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got.view(np.int64)[~nan] == want.view(np.int64)[~nan]).all())


def check_exact(mat):
    """Integer-valued, |entries| <= 2^20, d <= 4096: every L1 sum is below
    2^32 and every L2 sum of squares at most 2^52, so each is exact in any
    order, and so is every partial sum on the way."""
    mat = np.asarray(mat, np.float64)
    assert mat.ndim == 2 and 1 <= mat.shape[1] <= MAX_D
    assert np.array_equal(mat, np.rint(mat)) and np.abs(mat).max(initial=0) <= MAX_ENTRY
    assert mat.shape[1] * MAX_ENTRY**2 < 2**53
    return mat


def offset_view(t, n, d):
    """A contiguous [n, d] torch view with the contents of `t` ([n, d]
    float64, any device) whose data_ptr() % 16 == 8: n d + 1 doubles are
    allocated (torch aligns allocations to 64 bytes or more) and the first is
    dropped."""
    import torch
    assert t.dtype == torch.float64 and tuple(t.shape) == (n, d)
    buf = torch.empty(n * d + 1, dtype=torch.float64, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(n, d)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    return view


# ------------------------------------------------------- kept rows by oracle --
def oracle_kept(pid, pk, *, U, P, l0, linf, seed, row_offset=0, allowed=None, max_contributions=0):
    """(kept mask, count, privacy_id_count) of oracle.columnar.bound_and_reduce.
    The oracle returns sums only, so the mask is decoded from them: 62 rows at
    a time carry the int64 values 1, 2, 4, ... (the others 0), and the bits of
    the sums over all partitions are the kept rows of the batch (no carries:
    every bit has one row)."""
    pid, pk = np.asarray(pid, np.int64), np.asarray(pk, np.int64)
    n = len(pk)
    kw = dict(n_privacy_ids=U, n_partitions=P, l0=l0, linf=linf, seed=seed, row_offset=row_offset,
              allowed=allowed, max_contributions=max_contributions)
    kept = np.zeros(n, bool)
    for a in range(0, n, 62):
        b = min(n, a + 62)
        val = np.zeros(n, np.int64)
        val[a:b] = np.int64(1) << np.arange(b - a, dtype=np.int64)
        r = O.bound_and_reduce(pid, pk, val, value_kind=O.VALUE_I64, flags=O.ACC_SUM | O.SUM_INT,
                               min_value=0, max_value=1 << 62, **kw)
        bits = int(np.bitwise_or.reduce(r["sum"]))
        assert int(r["sum"].sum()) == bits
        kept[a:b] = [(bits >> k) & 1 for k in range(b - a)]
    r = O.bound_and_reduce(pid, pk, None, value_kind=O.VALUE_NONE, flags=0, **kw)
    assert (np.bincount(pk[kept], minlength=P) == r["count"]).all()
    return kept, r["count"], r["privacy_id_count"]


def oracle_columns(pid, pk, vec, *, U, P, l0, linf, seed, row_offset=0, allowed=None, max_contributions=0):
    """The [P, d] sums column by column, as tests/test_gpu_vector_sum.py's
    _expected builds them: the oracle is linear in the value."""
    cols = [O.bound_and_reduce(pid, pk, vec[:, j], n_privacy_ids=U, n_partitions=P, l0=l0, linf=linf,
                               value_kind=O.VALUE_F64, flags=O.ACC_SUM, min_value=-np.inf, max_value=np.inf,
                               seed=seed, row_offset=row_offset, allowed=allowed,
                               max_contributions=max_contributions)["sum"] for j in range(vec.shape[1])]
    return np.stack(cols, axis=1)


# ------------------------------------------------------------ lane layouts --
def geometry(d, vectors_off, acc_off):
    """pairs_vector_sum's choice: (bytes per lane, lane columns, lanes per row,
    row slots per wave, column chunks in blockIdx.y)."""
    wide = d % 2 == 0 and not vectors_off and not acc_off
    cols = d // 2 if wide else d
    log2_g = 0
    while log2_g < 6 and (1 << log2_g) < cols:
        log2_g += 1
    chunks = (cols + 63) // 64 if log2_g == 6 else 1
    return (16 if wide else 8, cols, 1 << log2_g, 64 >> log2_g, chunks)


# id: d, vectors +8, vector_acc +8, geometry()
LAYOUTS = {
    "d2_wide_1col_64slots": (2, False, False, (16, 1, 1, 64, 1)),
    "d2_vectors_off_2cols": (2, True, False, (8, 2, 2, 32, 1)),
    "d2_acc_off": (2, False, True, (8, 2, 2, 32, 1)),
    "d6_wide_3_of_4": (6, False, False, (16, 3, 4, 16, 1)),
    "d17_17_of_32_2slots": (17, False, False, (8, 17, 32, 2, 1)),
    "d33_31_idle": (33, False, False, (8, 33, 64, 1, 1)),
    "d64_vectors_off_full_chunk": (64, True, False, (8, 64, 64, 1, 1)),
    "d128_wide_64cols": (128, False, False, (16, 64, 64, 1, 1)),
    "d128_acc_off_2chunks": (128, False, True, (8, 128, 64, 1, 2)),
    "d129_3chunks_last_of_1": (129, False, False, (8, 129, 64, 1, 3)),
    "d4095_64chunks": (4095, False, False, (8, 4095, 64, 1, 64)),
    "d4096_wide_32chunks": (4096, False, False, (16, 2048, 64, 1, 32)),
    "d4096_vectors_off_64chunks": (4096, True, False, (8, 4096, 64, 1, 64)),
}
SPLIT_P = 40
SPLIT = ((3, 4, 30, 39), (1024, 1025, 1500, 3))  # tests/test_gpu_vector_sum.py test_segment_split_shapes
SPLIT_LARGE_D = ((4, 39), (1025, 3))             # d >= 4095: 1,028 rows, 34 MB
TILE = 1024                                      # kVsTile


def _integer_rows(rng, n, d, bound=MAX_ENTRY):
    return rng.integers(-bound, bound + 1, (n, d)).astype(np.float64)


@functools.lru_cache(maxsize=2)
def split_table(d):
    """(pid, pk, vec, P): integer rows in shuffled order over the partitions of
    SPLIT (d <= 129) or SPLIT_LARGE_D.  With NoOp bounding the kept-row list is
    the rows by partition."""
    codes, sizes = SPLIT if d <= 129 else SPLIT_LARGE_D
    rng = np.random.default_rng(7000 + d)
    pk = rng.permutation(np.repeat(codes, sizes)).astype(np.int64)
    pid = rng.integers(0, 500, len(pk)).astype(np.int64)
    vec = check_exact(_integer_rows(rng, len(pk), d))
    check_split(pk, d)
    return pid, pk, vec, SPLIT_P


def check_split(pk, d):
    cnt = np.bincount(pk, minlength=SPLIT_P)
    off = np.concatenate([[0], np.cumsum(cnt)])
    assert (cnt == 0).sum() == SPLIT_P - (4 if d <= 129 else 2)
    assert (cnt > TILE).any() and ((cnt > 0) & (cnt <= TILE)).any()  # k_vs_combine and the whole-piece store both run
    if d <= 129:
        assert cnt[3] == TILE and off[3] == 0             # a tile filled whole by a partition summed whole
        assert off[4] == TILE and cnt[4] == TILE + 1      # a partition starting on a tile edge
        assert off[30] // TILE == 2 and off[30] % TILE and off[31] // TILE == 3  # tile 2 writes both partial slots
    assert len(pk) * MAX_ENTRY < 2**53


@functools.lru_cache(maxsize=2)
def split_expected(d):
    _, pk, vec, P = split_table(d)
    return accumulate(pk, vec, P)


def prefill(P, d, live):
    """[P + 1, d]: a non-zero integer vector in every live partition, a quiet
    NaN in every coordinate of the others, and a guard row behind the last."""
    j = np.arange(d, dtype=np.float64)
    out = np.full((P + 1, d), np.nan)
    for p in np.flatnonzero(live):
        out[p] = (p + 1) * (1 - 2 * (j % 2)) * (j % 7 + 1)
    out[P] = -(j + 12345.0)
    assert (out[:P][live] != 0).all() and np.isnan(out[:P][~live]).all()
    check_exact(np.nan_to_num(out, nan=0.0))
    return out


# id: d, vectors +8, row slots
SLOT_LAYOUTS = {
    "d2_wide_64slots": (2, False, 64),
    "d8_wide_16slots": (8, False, 16),
    "d64_narrow_1slot": (64, True, 1),
}
SLOT_SIZES = tuple(range(10)) + tuple(s for R in (64, 16, 1)
                                      for s in (R * 3, R * 4, R * 4 + 1, R * 5 - 1, R * 6, R * 7))


@functools.lru_cache(maxsize=None)
def slot_table(d):
    """Partition p has SLOT_SIZES[p] rows: 0 ... 9, and R 3, R 4, R 4 + 1,
    R 5 - 1, R 6, R 7 for R = 64, 16, 1: at R row slots a slot gets 3, 4, 4 or
    5, 5 or 4, 6 and 7 entries, the `r + 3R < b` loop of vs_sum not entered,
    entered once with a tail of 0, 1, 2 and 3 (R 6 and R 7 give the tails of 2
    and 3 after a full trip, which the first four sizes give at R = 1 only)."""
    P = len(SLOT_SIZES)
    assert max(SLOT_SIZES) <= TILE  # every partition is one piece: one vs_sum over [off[p], off[p + 1])
    rng = np.random.default_rng(7100 + d)
    pk = rng.permutation(np.repeat(np.arange(P), SLOT_SIZES)).astype(np.int64)
    pid = rng.integers(0, 500, len(pk)).astype(np.int64)
    vec = check_exact(_integer_rows(rng, len(pk), d))
    return pid, pk, vec, P


def check_slots(R):
    """Entries per row slot that the sizes give at R row slots: none, one, 3
    (the loop not entered), and 4 ... 7 (one trip and every tail)."""
    per_slot = {(s + R - 1 - k) // R for s in SLOT_SIZES for k in range(R)}
    assert {0, 1, 3, 4, 5, 6, 7} <= per_slot, (R, per_slot)
    for s in (R * 3, R * 4, R * 4 + 1, R * 5 - 1):
        assert s in SLOT_SIZES


# ----------------------------------------------------------- sampled rows --
SAMPLED_SEED = 0x51A3_0000_0079
ROW_OFFSET = (1 << 32) + 5


def _with_ones(vec):
    vec[:, 1] = 1.0  # this column of the sums is the partitions' row count
    return vec


@functools.lru_cache(maxsize=None)
def per_id_table():
    """40 privacy ids with 1 ... 40 rows over 24 partitions, d = 3."""
    U, P, d = 40, 24, 3
    rng = np.random.default_rng(7200)
    pid = rng.permutation(np.repeat(np.arange(U), np.arange(1, U + 1))).astype(np.int64)
    pk = rng.integers(0, P, len(pid)).astype(np.int64)
    vec = check_exact(_with_ones(_integer_rows(rng, len(pid), d)))
    assert sorted(np.bincount(pid).tolist()) == list(range(1, U + 1)) and len(np.unique(pk)) == P
    return pid, pk, vec, U, P


@functools.lru_cache(maxsize=None)
def linf_table():
    """3,000 rows of 60 privacy ids over 24 partitions, d = 3: about two rows
    a pair, many pairs over linf = 2."""
    U, P, d, n = 60, 24, 3, 3000
    rng = np.random.default_rng(7201)
    pid = rng.integers(0, U, n).astype(np.int64)
    pk = rng.integers(0, P, n).astype(np.int64)
    vec = check_exact(_with_ones(_integer_rows(rng, n, d)))
    return pid, pk, vec, U, P


SAMPLED_CASES = {  # l0, linf, max_contributions, row_offset, allowed mask
    "max_contributions_3": (0, 0, 3, 0, False),
    "row_offset_above_2_32": (0, 2, 0, ROW_OFFSET, False),
    "allowed_mask": (2, 2, 0, 0, True),
}


@functools.lru_cache(maxsize=None)
def sampled_case(name):
    """(pid, pk, vec, kwargs of oracle_kept, kept, count, privacy_id_count)."""
    l0, linf, maxc, row_offset, masked = SAMPLED_CASES[name]
    pid, pk, vec, U, P = per_id_table() if maxc else linf_table()
    allowed = (np.arange(P) % 3 != 1).astype(np.uint8) if masked else None
    kw = dict(U=U, P=P, l0=l0, linf=linf, seed=SAMPLED_SEED, row_offset=row_offset, allowed=allowed,
              max_contributions=maxc)
    kept, count, pid_count = oracle_kept(pid, pk, **kw)
    return pid, pk, vec, kw, kept, count, pid_count


def check_sampled_case(name):
    pid, pk, vec, kw, kept, count, _ = sampled_case(name)
    l0, linf, maxc, row_offset, masked = SAMPLED_CASES[name]
    if maxc:  # the kept-row total is the sum of min(rows, 3)
        assert int(kept.sum()) == int(np.minimum(np.bincount(pid), maxc).sum()) < len(pid)
        assert (np.bincount(pid[kept], minlength=kw["U"]) == np.minimum(np.bincount(pid, minlength=kw["U"]), maxc)).all()
    if row_offset:
        pairs, rows = np.unique(pid * kw["P"] + pk, return_counts=True)
        assert (rows > linf).sum() > 100 and int(kept.sum()) == int(np.minimum(rows, linf).sum())
        kept0, count0, _ = oracle_kept(pid, pk, **dict(kw, row_offset=0))
        assert (count0 == count).all() and (kept0 != kept).any()  # other rows of the same pairs
        assert not np.array_equal(accumulate(pk, vec, kw["P"], kept0), accumulate(pk, vec, kw["P"], kept))
    if masked:
        assert not count[kw["allowed"] == 0].any() and count[kw["allowed"] == 1].all()
        assert int(kept.sum()) < int(kw["allowed"][pk].sum())
    assert (accumulate(pk, vec, kw["P"], kept)[:, 1] == count).all()


# ------------------------------------------------ accumulators for the clip --
CLIP_DS = (1, 2, 63, 64, 65, 128, 130, 4096)
MAX_NORM = 5.0 * 1024            # 5 * 2^10: the 3-4-5 row scaled by 2^10
CLIP_ROWS = ("below", "above", "equal", "zero", "high_coordinates", "last_coordinate")
CLIP_INDEX = (5, 2, 0, 3, 2, 1, 4)   # a permutation of the rows that repeats row 2
NOISE_INDEX = (5, 2, 0, 3, 1, 4, 6)  # no repeat: every stream index once


@functools.lru_cache(maxsize=None)
def clip_acc(d, kind):
    """[7, d] integer accumulator, rows in the order of CLIP_ROWS (row 6: one
    more row above max_norm), for max_norm = MAX_NORM:
      below            entries in {-1, 0, 1}: norm <= d < MAX_NORM, coef 1
      above            entries up to 2^20, the first 2^20 - 1
      equal            norm == MAX_NORM exactly.  L1: |entries| summing to
                       5,120; L2: (3, ..., -4) * 2^10 in the first and the last
                       coordinate (d = 1: -5,120)
      zero
      high_coordinates d > 64: zero in coordinates 0 ... 63, entries up to
                       2^20 from 64 on; a norm over one trip of 64 lanes is 0
                       and gives coef 1.  d <= 64: the upper half instead
      last_coordinate  -(2^20 - 3) in coordinate d - 1 alone"""
    rng = np.random.default_rng(7300 + d + (0 if kind == "l1" else 10000))
    acc = np.zeros((7, d))
    acc[0] = rng.integers(-1, 2, d)
    acc[0, d - 1] = 1.0
    acc[1] = _integer_rows(rng, 1, d)[0]
    acc[1, 0] = MAX_ENTRY - 1
    m = int(MAX_NORM)
    if kind == "l1":
        base, rem = divmod(m, d)
        acc[2] = base * rng.choice([-1.0, 1.0], d)
        acc[2, 0] = -(base + rem)
    elif d == 1:
        acc[2, 0] = -m
    else:
        acc[2, 0], acc[2, d - 1] = 3 * m // 5, -4 * m // 5
    lo = 64 if d > 64 else d // 2
    acc[4, lo:] = _integer_rows(rng, 1, d - lo)[0]
    acc[4, lo] = -(MAX_ENTRY - 5)
    acc[5, d - 1] = -(MAX_ENTRY - 3)
    acc[6] = _integer_rows(rng, 1, d)[0]
    acc[6, d - 1] = MAX_ENTRY - 7
    check_clip_acc(acc, kind)
    return acc


def exact_norm_sq(row, kind):
    """Python ints: (sum |x|)^2 for L1, sum x^2 for L2."""
    ints = [int(v) for v in row]
    return sum(abs(v) for v in ints)**2 if kind == "l1" else sum(v * v for v in ints)


def check_clip_acc(acc, kind):
    check_exact(acc)
    d = acc.shape[1]
    m2 = int(MAX_NORM)**2
    n2 = [exact_norm_sq(r, kind) for r in acc]
    assert 0 < n2[0] < m2 and n2[1] > m2 and n2[2] == m2 and n2[3] == 0 and n2[4] > m2 and n2[5] > m2 and n2[6] > m2
    if d > 64:
        assert not acc[4, :64].any() and acc[4, 64:].any()
    assert not acc[5, :d - 1].any()
    assert sorted(set(CLIP_INDEX)) == list(range(6)) and len(CLIP_INDEX) == 7
    assert sorted(NOISE_INDEX) == list(range(7))


NONFINITE_D = 130
NONFINITE = tuple((v, j) for v in (np.inf, -np.inf, np.nan) for j in (5, 100))


@functools.lru_cache(maxsize=None)
def nonfinite_acc():
    """[6, 130]: an integer row above MAX_NORM with one coordinate replaced by
    +inf, -inf or NaN, once below and once above coordinate 64."""
    rng = np.random.default_rng(7400)
    acc = check_exact(_integer_rows(rng, len(NONFINITE), NONFINITE_D))
    acc[acc == 0] = 1.0  # so every finite coordinate shows its sign as a zero
    acc = acc.copy()
    for r, (v, j) in enumerate(NONFINITE):
        acc[r, j] = v
    return acc


@functools.lru_cache(maxsize=None)
def normal_acc():
    """[8, 130] normal-valued rows, half of them below MAX_NORM."""
    rng = np.random.default_rng(7401)
    acc = rng.normal(0.0, 1.0, (8, NONFINITE_D))
    acc[::2] *= 700.0  # L1 norm about 72,000, L2 about 8,000
    return acc


# ------------------------------------------------------------------ noise --
NOISE_D = 130
# (NOISE_OFFSET + 3) * 130 = 2^32 - 126: row 3 crosses 2^32 at coordinate 126
NOISE_OFFSET = (1 << 32) // NOISE_D - 3


def noise_gidx(index, partition_offset, d):
    """Philox stream of out[i][j]: (partition_offset + index[i]) * d + j."""
    return ((partition_offset + np.asarray(index, np.int64))[:, None] * d + np.arange(d)[None, :]).ravel()


def noise(kind, d):
    import pipelinedp_amd as pdp
    from pipelinedp_amd import dp_computations as dpc
    nk = pdp.NoiseKind.LAPLACE if kind == "laplace" else pdp.NoiseKind.GAUSSIAN
    return dpc.noise_params(nk, 1.0 / d, 1e-6 / d, 2, 2)


# ------------------------------------------------------- metrics loop bounds --
LOOP_P, LOOP_D = 500, 3
LOOP_N = (8193, 16385)  # 2,048 blocks of 4 waves: trips 2 and 3 start at 8,192 and 16,384
SENTINEL = -777.25


@functools.lru_cache(maxsize=None)
def loop_acc():
    rng = np.random.default_rng(7500)
    acc = check_exact(_integer_rows(rng, LOOP_P, LOOP_D))
    acc[7] = 0.0
    return acc


@functools.lru_cache(maxsize=None)
def loop_index(n):
    """n entries over P = 500: every partition, most of them many times, in
    no order."""
    rng = np.random.default_rng(7501 + n)
    index = np.concatenate([np.arange(LOOP_P), rng.integers(0, LOOP_P, n - LOOP_P)])
    index = rng.permutation(index).astype(np.int64)
    assert len(index) == n and len(np.unique(index)) == LOOP_P and (np.diff(index) < 0).any()
    return index


# -------------------------------------------------------------------- API --
API = dict(d=130, P=20, empty=11, max_norm=24000.0, eps=1e6, delta=1e-6, seed=7600)


@functools.lru_cache(maxsize=None)
def api_table():
    """(pid, pk, vec): one row per privacy id, 5 ... 23 rows in each of the 19
    live partitions of 20; partition API['empty'] has none.  |entries| <= 1,024,
    so the squares of the partitions' sums add exactly (check_exact_sums)."""
    rng = np.random.default_rng(API["seed"])
    live = [p for p in range(API["P"]) if p != API["empty"]]
    pk = rng.permutation(np.repeat(live, np.arange(5, 5 + len(live)))).astype(np.int64)
    pid = np.arange(len(pk), dtype=np.int64)
    vec = check_exact(_integer_rows(rng, len(pk), API["d"], 1024))
    return pid, pk, vec


def check_api_table():
    pid, pk, vec = api_table()
    assert len(np.unique(pid)) == len(pid) and API["empty"] not in pk
    acc = check_exact_sums(accumulate(pk, vec, API["P"]))
    norms = np.sqrt((acc * acc).sum(axis=1))
    live = np.arange(API["P"]) != API["empty"]
    assert (norms[live] < API["max_norm"]).any() and (norms[live] > API["max_norm"]).any()  # both branches of min
    return acc


def check_exact_sums(acc):
    """A [P, d] accumulator of integer sums whose squares still add exactly."""
    assert np.array_equal(acc, np.rint(acc)) and float((acc * acc).sum(axis=1).max()) < 2.0**53
    assert max(exact_norm_sq(r, "l2") for r in acc) < 2**53
    return acc
