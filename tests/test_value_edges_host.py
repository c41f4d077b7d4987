"""The oracle's value semantics, pinned without the oracle's own arithmetic (CPU).

With bounds that sample nothing (l0 >= the partitions of every privacy id,
linf >= the rows of every pair) the accumulators are a plain group-by of the
rows.  tests/value_edges_util.plain_group_by computes it from the rows with
fractions.Fraction and Python ints, clipping per row (or the pair sum with
SUM_PER_PARTITION); oracle/columnar.py bound_and_reduce must equal it
exactly on a dyadic table (whose fp64 sums are exact in any order).

On the edge table the rule is np.clip's, element by element: a finite value
goes to the nearer bound, +-inf to a bound, and a NaN stays NaN -- the
reference's SumCombiner.create_accumulator is np.clip(values, lo, hi).sum()
(combiners.py:411), MeanCombiner and VarianceCombiner normalise the same
np.clip'ed values (combiners.py:477, 554), and with per-partition bounds the
pair's raw sum is clipped, np.clip(sum(values), min_sum, max_sum)
(combiners.py:409).  So a NaN row makes NaN the fp64 fields of its own
partition and of no other; int64 sums wrap modulo 2^64 before the clip.
"""
import numpy as np
import pytest

from oracle import columnar as O
from tests import value_edges_util as VU

U, P, N_ROWS = 300, 120, 2000
NO_SAMPLING = 256  # >= the partitions of any id and the rows of any pair at this size

VARIANTS = {
    "f64": (O.VALUE_F64, O.ACC_SUM | O.ACC_NSUM | O.ACC_NSUM2),
    "f64_per_partition": (O.VALUE_F64, O.SUM_PER_PARTITION | O.ACC_NSUM | O.ACC_NSUM2),
    "i64": (O.VALUE_I64, O.ACC_SUM | O.SUM_INT | O.ACC_NSUM | O.ACC_NSUM2),
    "i64_per_partition": (O.VALUE_I64, O.SUM_PER_PARTITION | O.SUM_INT | O.ACC_NSUM | O.ACC_NSUM2),
}


def _oracle(pid, pk, val, vk, flags, b, linf=NO_SAMPLING):
    with np.errstate(all="ignore"):  # inf - inf and 1e308 + 1e308 are inputs here
        return O.bound_and_reduce(pid, pk, val, n_privacy_ids=U, n_partitions=P, l0=NO_SAMPLING, linf=linf,
                                  value_kind=vk, flags=flags, min_value=b.lo, max_value=b.hi, middle=b.mid,
                                  min_sum=b.min_sum, max_sum=b.max_sum, seed=7)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("linf", [NO_SAMPLING, 0], ids=["rows-sampled-form", "keep-every-row"])
def test_oracle_equals_exact_group_by_on_a_dyadic_table(variant, linf):
    vk, flags = VARIANTS[variant]
    b = VU.bounds_for(vk)
    pid, pk, val = VU.dyadic_table(3, N_ROWS, U, P, vk)
    # the clip must have work on both sides, and the planted rows are there
    f = val.astype(np.float64)
    assert (f < b.lo).mean() > 0.25 and (f > b.hi).mean() > 0.25
    assert (f == b.lo).any() and (f == b.hi).any() and (f == np.floor(b.mid) if vk == O.VALUE_I64 else f == b.mid).any()
    want = VU.plain_group_by(pid, pk, val, P, vk, flags, b, exact=True)
    VU.assert_exactly_equal(_oracle(pid, pk, val, vk, flags, b, linf), want)


def test_check_exact_refuses_what_could_round():
    pid, pk, val = VU.dyadic_table(1, 500, U, P, O.VALUE_F64)
    with pytest.raises(ValueError, match="dyadic"):
        VU.check_exact(pk, val + 1.0 / 16.0, P, VU.F64_BOUNDS)
    with pytest.raises(ValueError, match="multiple of 1/8"):
        VU.check_exact(pk, val, P, VU.Bounds(0.1, 1.0, 0.5, 0.0, 1.0))
    import dataclasses
    huge = dataclasses.replace(VU.F64_BOUNDS, mid=float(1 << 23))  # squares of 2^52 units each, ~4 rows per partition
    with pytest.raises(ValueError, match="2\\^53"):
        VU.check_exact(pk, val, P, huge)


EDGE_BOUNDS = {"bounded": None, "lo_eq_hi": VU.LO_EQ_HI, "unbounded": VU.UNBOUNDED}


# (SUM_INT takes int64 bounds only: no unbounded int case)
EDGE_CASES = [(v, k) for v in sorted(VARIANTS) for k in sorted(EDGE_BOUNDS)
              if not (v.startswith("i64") and k == "unbounded")]


@pytest.mark.parametrize("variant,bounds", EDGE_CASES)
def test_oracle_follows_np_clip_on_the_edge_table(variant, bounds):
    vk, flags = VARIANTS[variant]
    b = EDGE_BOUNDS[bounds] or VU.bounds_for(vk)
    if bounds == "lo_eq_hi" and vk == O.VALUE_I64:
        b = VU.I64_LO_EQ_HI
    t = VU.edge_table(11, U, P, vk, b, l0=NO_SAMPLING, linf=NO_SAMPLING)
    want = VU.plain_group_by(t.pid, t.pk, t.val, P, vk, flags, b, exact=False)
    got = _oracle(t.pid, t.pk, t.val, vk, flags, b)
    VU.assert_exactly_equal(got, want)
    # every dedicated pair is there
    for u, p, rows in t.dedicated:
        assert got["privacy_id_count"][p] >= 1 and got["count"][p] >= rows
    if vk == O.VALUE_F64:
        # a NaN row makes NaN the fp64 fields of its own partition, and only those
        nan_parts = [t.partition[k] for k in VU.NAN_KINDS]
        for k in VU.FIELDS:
            assert np.isnan(got[k][nan_parts]).all(), k
            assert np.isfinite(got[k][:t.first_edge_partition]).all(), k
        per_partition = bool(flags & O.SUM_PER_PARTITION)
        mixed = t.partition["inf_minus_inf"]  # a pair holding +inf and -inf
        if per_partition:
            assert np.isnan(got["sum"][mixed])  # raw sum NaN, and the clip keeps it
            if np.isfinite(b.max_sum):  # a pair of 1e308 + 1e308 = +inf is clipped to max_sum
                n_pairs = got["privacy_id_count"][t.partition["overflow"]]
                assert got["sum"][t.partition["overflow"]] == n_pairs * b.max_sum
        not_nan = sorted(set(range(P)) - set(nan_parts) - ({mixed} if per_partition or bounds == "unbounded" else set()))
        assert not np.isnan(got["sum"][not_nan]).any()
    else:
        # 2^53 + 1 read as fp64 is clipped like any large value
        assert got["normalized_sum"][t.partition["above_2^53"]] == \
            got["count"][t.partition["above_2^53"]] * (b.hi - b.mid)


def test_int_pair_sum_wraps_before_the_clip():
    """INT64_MAX + INT64_MAX = -2 and INT64_MIN + -1 = INT64_MAX modulo 2^64:
    the per-partition clip sees the wrapped sum."""
    vk, flags = VARIANTS["i64_per_partition"]
    b = VU.I64_BOUNDS
    pid = np.array([0, 0, 1, 1])
    pk = np.array([0, 0, 1, 1])
    val = np.array([VU.I64_MAX, VU.I64_MAX, VU.I64_MIN, -1], dtype=np.int64)
    got = _oracle(pid, pk, val, vk, flags, b)
    assert got["sum"][0] == -2 and got["sum"][1] == int(b.max_sum)
