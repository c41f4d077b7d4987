"""PERCENTILE on the GPU: pdp_reduce_quantile_leaves and pdp_quantile_metrics
(through executor.reduce_quantile_leaves / quantile_metrics) and
DPEngine.aggregate on ColumnarBackend, against the NumPy restatement of the
quantile tree (tests/quantile_tree_util.py).

With the noise off the kernel must EQUAL the restatement run on the rows the
restatement's bounder keeps: l0 and linf are chosen so large that nothing is
sampled away (the bounder asserts it), so no random choice enters, and the
walk performs the restatement's fp64 operations in the restatement's order
(the device code is compiled without floating-point contraction).
"""
import functools
import math

import numpy as np
import pytest

import pipelinedp_amd as pdp
from pipelinedp_amd import columnar_backend as CB
from pipelinedp_amd import dp_computations as dpc
from pipelinedp_amd import executor as X
from pipelinedp_amd import _native as N
from tests import quantile_tree_util as Q

pytestmark = pytest.mark.gpu

BIG = 1 << 20  # l0 / linf no table below reaches
RANKS5 = [0.0, 0.37, 0.5, 0.5, 1.0]


def _run(device, pid, pk, values, *, P, lo, hi, ranks, l0=BIG, linf=BIG, noise=None, seed=11, allowed=None,
         U=None, noise_seed=None):
    """(out [P, len(ranks)], leaves uint16, offsets uint32) for all P partitions, empty ones included."""
    import torch
    pid, pk = np.asarray(pid, np.int64), np.asarray(pk, np.int64)
    values = np.asarray(values)
    U = int(pid.max(initial=0)) + 1 if U is None else U
    spec = X.BoundingSpec(l0=l0, linf=linf, value_kind=N.VALUE_NONE, flags=0)
    t = functools.partial(torch.as_tensor, device=device)
    mask = None if allowed is None else t(np.asarray(allowed, np.uint8))
    acc, leaves, offsets = X.reduce_quantile_leaves(t(pid), t(pk), t(values), n_privacy_ids=U, n_partitions=P,
                                                    bounding=spec, min_value=lo, max_value=hi, seed=seed,
                                                    allowed=mask)
    index = torch.arange(P, dtype=torch.int64, device=device)
    out = X.quantile_metrics(leaves, offsets, index, min_value=lo, max_value=hi, ranks=ranks, noise=noise,
                             seed=seed if noise_seed is None else noise_seed)
    off = offsets.cpu().numpy().view(np.uint32)
    return out.cpu().numpy(), leaves.cpu().numpy().view(np.uint16)[:off[-1]], off


def _check_equal(device, pid, pk, values, *, P, lo, hi, ranks, allowed=None):
    got, leaves, off = _run(device, pid, pk, values, P=P, lo=lo, hi=hi, ranks=ranks, allowed=allowed)
    rows = Q.kept_rows_by_partition(pid, pk, values, P, BIG, BIG, allowed)
    want_leaves = [np.sort(Q.leaf_index(rows[p], lo, hi)) for p in range(P)]
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in want_leaves])]).tolist()
    assert leaves.tolist() == np.concatenate(want_leaves).tolist() if len(leaves) else off[-1] == 0
    want = Q.expected(pid, pk, values, P, lo, hi, ranks, BIG, BIG, allowed)
    assert got.shape == want.shape
    assert got.tolist() == want.tolist()  # equality, NaN-free
    return got


# ------------------------------------------------------------ one partition --
@pytest.mark.parametrize("case", ["one_row", "two_rows", "seventeen_in_one_leaf", "known_answers_1001"])
def test_one_partition_equals_restatement(device, case):
    lo, hi = 0.0, 1000.0
    values = {"one_row": [123.456], "two_rows": [10.0, 990.0],
              "seventeen_in_one_leaf": [500.001 + 1e-4 * i for i in range(17)],
              "known_answers_1001": np.arange(1001.0)}[case]
    n = len(values)
    if case == "seventeen_in_one_leaf":
        assert len(set(Q.leaf_index(values, lo, hi).tolist())) == 1
    ranks = [0.1, 0.5, 0.9, 0.0, 1.0]
    got = _check_equal(device, np.arange(n), np.zeros(n, np.int64), values, P=1, lo=lo, hi=hi, ranks=ranks)
    if case == "known_answers_1001":  # the reference's QuantileCombinerTest
        assert np.all(np.abs(got[0, :3] - [100.0, 500.0, 900.0]) <= 0.1)


@pytest.mark.parametrize("lo,hi", [(0.0, 1000.0), (-5.0, 3.0), (0.0, 1e-3), (-1e9, 1e9)])
def test_edge_values_ranges_and_nan(device, lo, hi):
    """Values at lo, at hi, outside the range, on leaf boundaries and NaN, over
    a negative min_value and ranges of 1e-3 and 1e9; partition 2 holds only NaN
    (an empty tree), partition 3 nothing."""
    w = hi - lo
    p0 = [lo, hi, lo - w, hi + w, -math.inf, math.inf, math.nan, lo + w / 3]
    p1 = [lo + w * (leaf / Q.L) for leaf in (1, 2, 4096, 32768, 65535)] + [math.nan, lo + w * 0.75]
    p2 = [math.nan, math.nan]
    values = np.array(p0 + p1 + p2)
    pk = np.array([0] * len(p0) + [1] * len(p1) + [2] * len(p2))
    got = _check_equal(device, np.arange(len(values)), pk, values, P=4, lo=lo, hi=hi, ranks=RANKS5)
    assert got[2].tolist() == got[3].tolist() == [Q.empty_answer(lo, hi, r) for r in RANKS5]


def test_integer_value_column(device):
    rng = np.random.default_rng(3)
    values = rng.integers(-50, 1100, 700)  # int64: some outside [0, 1000]
    pk = rng.integers(0, 3, 700)
    _check_equal(device, np.arange(700), pk, values, P=3, lo=0.0, hi=1000.0, ranks=RANKS5)


# -------------------------------------------------------- many partitions --
@functools.lru_cache(maxsize=None)
def _uneven_table():
    """70 partitions of uneven sizes: 0 (several), 1, 63, 64, 65, 2,500 (more
    than the sort's 2,048-record tile) and random sizes below 300; the rows are
    shuffled, so segments cross wave, tile and workgroup boundaries."""
    rng = np.random.default_rng(70)
    sizes = rng.integers(2, 300, 70)
    sizes[[0, 7, 33, 69]] = 0
    sizes[[1, 2, 3, 4, 40]] = [1, 63, 64, 65, 2500]
    pk = np.repeat(np.arange(70), sizes)
    values = rng.normal(40.0, 30.0, len(pk))
    values[rng.random(len(pk)) < 0.02] = math.nan
    order = rng.permutation(len(pk))
    pk, values = pk[order], values[order]
    pid = rng.integers(0, 500, len(pk))  # ids span partitions and repeat within them
    return pid, pk, values


def test_seventy_uneven_partitions_equal_restatement(device):
    pid, pk, values = _uneven_table()
    allowed = np.ones(70, np.uint8)  # public partitions: the empty ones are answered too
    got = _check_equal(device, pid, pk, values, P=70, lo=-20.0, hi=120.0, ranks=RANKS5, allowed=allowed)
    assert got[0].tolist() == [Q.empty_answer(-20.0, 120.0, r) for r in RANKS5]


def test_non_public_partitions_rows_are_dropped(device):
    pid, pk, values = _uneven_table()
    allowed = (np.arange(70) % 3 != 1).astype(np.uint8)
    _check_equal(device, pid, pk, values, P=70, lo=-20.0, hi=120.0, ranks=[0.25, 0.75], allowed=allowed)


@pytest.mark.parametrize("n_ranks", [1, 3, 4, 5, 64])
def test_rank_counts_partial_lane_groups_and_rounds(device, n_ranks):
    """1, 3 and 5 ranks leave lane groups without a rank (they must not sway
    the others' ballots), 5 and 64 take more than one round of four; ranks 0,
    1 and duplicates are among them."""
    rng = np.random.default_rng(n_ranks)
    base = [0.5, 0.0, 1.0, 0.5, 0.999999, 1e-7, 0.25]
    ranks = (base + rng.uniform(0, 1, 64).tolist())[:n_ranks]
    sizes = [0, 1, 17, 300, 64]
    pk = np.repeat(np.arange(5), sizes)
    values = rng.uniform(-1.0, 11.0, len(pk))
    _check_equal(device, np.arange(len(pk)), pk, values, P=5, lo=0.0, hi=10.0, ranks=ranks)


# ----------------------------------------------------------------- bounding --
def test_bounding_is_applied(device):
    """linf = 1 and an id with three rows in the partition: the tree holds
    exactly one of them, whichever the sampling picks."""
    values = [100.0, 500.0, 900.0]
    got, leaves, off = _run(device, [0, 0, 0], [0, 0, 0], values, P=1, lo=0.0, hi=1000.0, ranks=[0.5], l0=1, linf=1)
    assert off.tolist() == [0, 1]
    singles = [Q.Tree(0.0, 1000.0, [v]).quantiles([0.5])[0] for v in values]
    assert got[0, 0] in singles
    assert leaves.tolist() in [Q.leaf_index([v], 0.0, 1000.0).tolist() for v in values]


def test_out_of_range_keys_set_the_error_word(device):
    with pytest.raises(ValueError, match="outside the dense key range"):
        _run(device, [0, 1], [0, 5], [1.0, 2.0], P=2, lo=0.0, hi=10.0, ranks=[0.5])


def test_other_plans_are_unsupported(device):
    import torch
    t = functools.partial(torch.as_tensor, device=device)
    spec = X.BoundingSpec(l0=2, linf=2, value_kind=N.VALUE_NONE, flags=0)
    with pytest.raises(N.NativeLibraryError, match="PDP_ALGO_PAIR_TABLE"):
        X.reduce_quantile_leaves(t(np.zeros(4, np.int64)), t(np.zeros(4, np.int64)), t(np.zeros(4)),
                                 n_privacy_ids=1, n_partitions=1, bounding=spec, min_value=0.0, max_value=1.0,
                                 seed=1, algorithm=N.ALGO_BUCKETED)


# -------------------------------------------------------------- with noise --
def _noise(kind, eps, delta=1e-6, l0=1, linf=1):
    nk = pdp.NoiseKind.LAPLACE if kind == "laplace" else pdp.NoiseKind.GAUSSIAN
    return dpc.noise_params(nk, eps, delta, l0 * Q.H, linf)


@pytest.mark.parametrize("kind", ["laplace", "gaussian"])
def test_same_seed_same_bits_other_seed_other_noise(device, kind):
    rng = np.random.default_rng(8)
    pk = rng.integers(0, 12, 1500)
    values = rng.uniform(0, 1, 1500)
    args = dict(P=12, lo=0.0, hi=1.0, ranks=[0.1, 0.5, 0.9], l0=1, linf=1, noise=_noise(kind, 0.5))
    a = _run(device, np.arange(1500), pk, values, **args, noise_seed=5)[0]
    b = _run(device, np.arange(1500), pk, values, **args, noise_seed=5)[0]
    c = _run(device, np.arange(1500), pk, values, **args, noise_seed=6)[0]
    assert a.tobytes() == b.tobytes()
    assert np.any(a != c)
    assert np.all((a >= 0.0) & (a <= 1.0))


def test_one_noisy_tree_per_partition(device):
    """64 ascending ranks of one partition read ONE noisy tree, so they come
    out non-decreasing in every partition.  Budget eps = 1.0 (Laplace scale
    l0 H linf / eps = 4 per node count, 200 values per partition): with
    independent noise per rank the restatement puts the 64 outputs out of order
    in 32 of 32 such partitions (tools/percentile_test_bands.py,
    monotone_violations(1.0) = 1.0), so sharing is what this shows."""
    rng = np.random.default_rng(2)
    P, per = 32, 200
    pk = np.repeat(np.arange(P), per)
    values = rng.uniform(0, 1, P * per)
    ranks = np.linspace(0.0, 1.0, 64).tolist()
    out = _run(device, np.arange(P * per), pk, values, P=P, lo=0.0, hi=1.0, ranks=ranks, l0=1, linf=1,
               noise=_noise("laplace", 1.0), noise_seed=21)[0]
    assert out.shape == (P, 64)
    assert np.all(np.diff(out, axis=1) >= 0.0)


# eps = 0.2, delta = 1e-6, l0 = linf = 1: Laplace b = 4 / 0.2 = 20, Gaussian sigma = compute_sigma(0.2, 1e-6, 2)
SCALE_BANDS = {"laplace": (0.017746, 0.026393), "gaussian": (0.022924, 0.038598)}


@pytest.mark.parametrize("kind", ["laplace", "gaussian"])
def test_noise_scale_is_right(device, kind):
    """Mean absolute error of the median over 256 partitions holding the same
    2,000 uniform values (np.random.default_rng(7)), against the noise-free
    median of the restatement.

    The accepted band was computed on the CPU by tools/percentile_test_bands.py
    (median_mae_band): the restatement with NumPy noise of the specified scale
    (Laplace b = l0 H linf / eps = 20; Gaussian sigma for L2 = sqrt(l0 H) linf
    = 2) gives one such figure per seed; over 24 seeds they span
    [0.020459, 0.023680] (Laplace, std 0.000904) and [0.027640, 0.033882]
    (Gaussian, std 0.001572).  The band is that span widened by three of those
    standard deviations on either side: a figure of the same distribution
    falls outside with probability well below 1e-3, while a scale wrong by a
    factor of sqrt(H) = 2 or H = 4 (the tree height left out of, or doubled
    in, a sensitivity) moves the figure by about that factor.  Nothing here
    was tuned against GPU output."""
    P, per = 256, 2000
    one = np.random.default_rng(7).uniform(0.0, 1.0, per)
    values = np.tile(one, P)
    pk = np.repeat(np.arange(P), per)
    truth = Q.Tree(0.0, 1.0, one).quantiles([0.5])[0]
    out = _run(device, np.arange(P * per), pk, values, P=P, lo=0.0, hi=1.0, ranks=[0.5], l0=1, linf=1,
               noise=_noise(kind, 0.2), noise_seed=99)[0]
    mae = float(np.mean(np.abs(out[:, 0] - truth)))
    print(f"median MAE ({kind}): {mae:.6f}, band {SCALE_BANDS[kind]}")
    lo, hi = SCALE_BANDS[kind]
    assert lo <= mae <= hi


# -------------------------------------------------------------- end to end --
_EXT = dict(privacy_id_extractor=lambda r: r[0], partition_extractor=lambda r: r[1], value_extractor=lambda r: r[2])


def _aggregate(device, rows, metrics, public=None, seed=31, total_epsilon=2.0**30):
    params = pdp.AggregateParams(metrics=metrics, noise_kind=pdp.NoiseKind.LAPLACE, max_partitions_contributed=1,
                                 max_contributions_per_partition=1, min_value=0.0, max_value=100.0)
    acc = pdp.NaiveBudgetAccountant(total_epsilon=total_epsilon, total_delta=1e-6)
    engine = pdp.DPEngine(acc, CB.ColumnarBackend(device=device, seed=seed))
    sink = engine.aggregate(rows, params, pdp.DataExtractors(**_EXT), public_partitions=public)
    acc.compute_budgets()
    return dict(sink), acc


@pytest.mark.parametrize("public", [True, False])
def test_aggregate_count_and_percentiles(device, public):
    """[COUNT, PERCENTILE(50), PERCENTILE(90)] with public partitions and with
    private selection, at a huge budget (every mechanism gets eps = 2^30, so its
    noise is of the order 1e-9).  The run without percentiles gets one
    mechanism's share less in total, so that COUNT has the same eps, hence the
    same sampler, in both runs; with the same seed it then draws the same noise
    and the two COUNT columns are equal bit for bit."""
    rng = np.random.default_rng(12)
    per = {p: rng.uniform(0.0, 100.0, 150 + 40 * p) for p in range(5)}
    rows = [(1000 * p + i, p, float(v)) for p, vs in per.items() for i, v in enumerate(vs)]
    keys = list(range(5)) + ([5] if public else [])  # public: one partition without rows
    pub = keys if public else None
    n_mech = 2 if public else 3  # COUNT, the percentiles' one budget, [private selection]
    metrics = [pdp.Metrics.COUNT, pdp.Metrics.PERCENTILE(50), pdp.Metrics.PERCENTILE(90)]
    out, acc = _aggregate(device, rows, metrics, pub, total_epsilon=n_mech * 2.0**30)
    plain, acc_plain = _aggregate(device, rows, [pdp.Metrics.COUNT], pub, total_epsilon=(n_mech - 1) * 2.0**30)
    assert sorted(out) == sorted(plain) == keys
    assert len(acc._mechanisms) == n_mech
    assert [m.mechanism_spec.eps for m in acc._mechanisms] == [2.0**30] * n_mech
    assert [m.mechanism_spec.eps for m in acc_plain._mechanisms] == [2.0**30] * (n_mech - 1)
    for p in keys:
        m = out[p]
        assert m._fields == ("count", "percentile_50", "percentile_90")
        assert m.count == plain[p].count
        if p == 5:  # no rows: the walk runs on noise alone
            assert abs(m.count) < 1e-6 and 0.0 <= m.percentile_50 <= 100.0 and 0.0 <= m.percentile_90 <= 100.0
            continue
        n = len(per[p])
        assert abs(m.count - n) < 1e-6
        srt = np.sort(per[p])
        for got, q in ((m.percentile_50, 50), (m.percentile_90, 90)):
            true = srt[-(-q * n // 100) - 1]  # the ceil(q n / 100)-th smallest value
            assert abs(got - true) <= 0.1


def test_aggregate_percentile_alone_and_with_privacy_id_count(device):
    rows = [(i, i % 3, float(i % 50)) for i in range(600)]
    out, _ = _aggregate(device, rows, [pdp.Metrics.PERCENTILE(99.5)], [0, 1, 2])
    assert all(m._fields == ("percentile_99_5",) and 48.0 <= m.percentile_99_5 <= 50.0 for m in out.values())
    out, _ = _aggregate(device, rows, [pdp.Metrics.PRIVACY_ID_COUNT, pdp.Metrics.PERCENTILE(10)], [0, 1, 2])
    assert all(m._fields == ("privacy_id_count", "percentile_10") and abs(m.privacy_id_count - 200) < 1e-6
               for m in out.values())  # (the huge budget leaves noise of the order 1e-9)


def test_raw_accumulators_hold_the_leaf_codes(device):
    rows = [(i, i % 2, float(i)) for i in range(40)]
    params = pdp.AggregateParams(metrics=[pdp.Metrics.COUNT, pdp.Metrics.PERCENTILE(50)],
                                 max_partitions_contributed=1, max_contributions_per_partition=1, min_value=0.0,
                                 max_value=40.0)
    acc = pdp.NaiveBudgetAccountant(total_epsilon=1.0, total_delta=1e-6)
    backend = CB.ColumnarBackend(device=device, seed=4)
    sink = pdp.DPEngine(acc, backend).aggregate(rows, params, pdp.DataExtractors(**_EXT))
    acc.compute_budgets()
    raw = backend.accumulators(sink)
    for p in (0, 1):
        row_count, (count, leaves) = raw[p]
        assert (row_count, count) == (20, 20)
        assert leaves.tolist() == Q.leaf_index([float(i) for i in range(p, 40, 2)], 0.0, 40.0).tolist()
