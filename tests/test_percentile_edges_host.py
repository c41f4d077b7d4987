"""tests/percentile_edges_util.py proven on the CPU, before a GPU sees it.

kept_rows (dicts, sorted(), Python ints) against oracle.columnar.bound_and_reduce
on random tables and on the GPU tests' own table: counts, distinct ids and,
through an int64 column of distinct weights, the kept set itself.
noised_expected against quantile_tree_util.expected without noise and, with
noise, against the product's own host tree (pipelinedp_amd.quantile_tree
.compute_quantiles), the second, independently written walk.  And every
builder's preconditions: a table that stops exercising its edge fails here.
"""
import numpy as np
import pytest

from oracle import columnar as O
from pipelinedp_amd import _native as N
from pipelinedp_amd import quantile_tree as QT
from tests import percentile_edges_util as PU
from tests import quantile_tree_util as Q


# -------------------------------------------------------------- kept rows --
def _oracle(pid, pk, P, U, l0, linf, seed, row_offset, allowed):
    n = len(pid)
    weights = (1 << 20) + np.arange(n, dtype=np.int64) ** 2  # distinct subset sums for all practical purposes
    acc = O.bound_and_reduce(pid, pk, weights, n_privacy_ids=U, n_partitions=P, l0=l0, linf=linf,
                             value_kind=O.VALUE_I64, flags=O.ACC_SUM | O.SUM_INT, min_value=0, max_value=1 << 62,
                             seed=seed, row_offset=row_offset, allowed=allowed,
                             rand_shift=PU.pair_table_rand_shift(n, U, P, l0, linf))
    return acc, weights


def _same_as_oracle(pid, pk, P, U, l0, linf, seed, row_offset=0, allowed=None, kept=None):
    if kept is None:
        kept = PU.kept_rows(pid, pk, P=P, U=U, l0=l0, linf=linf, seed=seed, row_offset=row_offset, allowed=allowed)
    acc, weights = _oracle(pid, pk, P, U, l0, linf, seed, row_offset, allowed)
    assert acc["count"].tolist() == np.bincount(pk[kept], minlength=P).tolist()
    pairs = np.unique(np.stack([pid[kept], pk[kept]], axis=1), axis=0)
    assert acc["privacy_id_count"].tolist() == np.bincount(pairs[:, 1], minlength=P).tolist()
    assert acc["sum"].tolist() == np.bincount(pk[kept], weights=weights[kept].astype(np.float64),
                                              minlength=P).astype(np.int64).tolist()
    return kept


def test_pair_table_rand_shift_is_the_partition_bits():
    for P in (1, 2, 40, 255, 256, 257, 70_000):
        assert PU.pair_table_rand_shift(6000, 300, P, 3, 2) == O.pk_bits(P)


@pytest.mark.parametrize("case", range(12))
def test_kept_rows_equal_the_oracle_on_random_tables(case):
    rng = np.random.default_rng(case)
    U, P = int(rng.integers(1, 60)), int(rng.choice([1, 3, 17, 64, 300]))
    n = int(rng.integers(1, 1500))
    pid, pk = rng.integers(0, U, n), np.minimum(rng.zipf(1.3, n) - 1, P - 1).astype(np.int64)
    l0, linf = int(rng.choice([1, 2, 5, PU.BIG])), int(rng.choice([1, 3, PU.BIG]))
    allowed = None if case % 3 else (rng.random(P) < 0.7).astype(np.uint8)
    row_offset = 0 if case % 4 else int(rng.integers(1, 1 << 40))
    kept = _same_as_oracle(pid, pk, P, U, l0, linf, seed=1000 + case, row_offset=row_offset, allowed=allowed)
    assert len(kept) == len(set(kept.tolist())) and (np.diff(kept) > 0).all()


def test_the_weights_identify_the_set():
    """Two different kept sets of equal size give different sums: the sum
    column is not a second count."""
    w = (1 << 20) + np.arange(6000, dtype=np.int64) ** 2
    rng = np.random.default_rng(0)
    sums = {int(w[rng.choice(6000, 50, replace=False)].sum()) for _ in range(2000)}
    assert len(sums) == 2000 and int(w.sum()) < 1 << 62


@pytest.mark.parametrize("case", sorted(PU.SAMPLED_CASES))
def test_sampled_table_cases_equal_the_oracle_and_sample_what_they_are_for(case):
    pid, pk, values, allowed = PU.sampled_table()
    l0, linf, row_offset, masked = PU.SAMPLED_CASES[case]
    _same_as_oracle(pid, pk, PU.SAMPLED["P"], PU.SAMPLED["U"], l0, linf, PU.SAMPLED_SEED, row_offset,
                    allowed if masked else None, kept=PU.sampled_kept(case))
    PU.check_sampled_case(case)


def test_sampled_table_nan_rows_cost_the_tree_a_value():
    """A NaN row that wins a slot stays in COUNT and leaves the tree: with
    linf = 1 some partition's tree is shorter than its count."""
    pid, pk, values, _ = PU.sampled_table()
    kept = PU.sampled_kept("l0_1_linf_1")
    leaves, off = PU.leaves_of_rows(values, pk, kept, PU.SAMPLED["P"], 0.0, 1.0)
    count = np.bincount(pk[kept], minlength=PU.SAMPLED["P"])
    assert (np.diff(off) <= count).all() and (np.diff(off) < count).any() and len(leaves) == off[-1]
    # dropping NaN *before* sampling would keep another row of that pair instead: the sets differ
    ok = ~np.isnan(values)
    pre = PU.kept_rows(pid[ok], pk[ok], P=PU.SAMPLED["P"], U=PU.SAMPLED["U"], l0=1, linf=1, seed=PU.SAMPLED_SEED)
    assert len(pre) > int(ok[kept].sum())


# ------------------------------------------------------------ noised walk --
def test_batched_draws_equal_single_draws():
    nd = PU.noise("laplace").as_dict()
    gidx = np.array([5, (1 << 32) - 1, 1 << 32, (1 << 32) + 7, 61_447 * Q.NODES], dtype=np.int64)
    raw = np.array([0.0, 1.0, 2.0, 300.0, 0.0])
    both = O.secure_add_noise(nd, raw, PU.NOISE_SEED, gidx, N.QUANTILE_SLOT)
    for i in range(len(gidx)):
        one = O.secure_add_noise(nd, raw[i:i + 1], PU.NOISE_SEED, gidx[i:i + 1], N.QUANTILE_SLOT)
        assert one[0] == both[i]
    # the counter's high word takes part: streams 2^32 apart differ
    lo = O.secure_add_noise(nd, np.zeros(64), PU.NOISE_SEED, np.arange(64), N.QUANTILE_SLOT)
    hi = O.secure_add_noise(nd, np.zeros(64), PU.NOISE_SEED, np.arange(64) + (1 << 32), N.QUANTILE_SLOT)
    assert (lo != hi).sum() > 32


def test_without_noise_it_is_the_restatement():
    trees = PU.walk_trees()
    got, counters = PU.walk_expected(None)
    rng = np.random.default_rng(41)  # walk_trees' values again, through Q.expected's own path
    values = [rng.uniform(0.0, 1.0, m) for m in PU.WALK_SIZES]
    pk = np.repeat(np.arange(8), PU.WALK_SIZES)
    want = Q.expected(np.arange(len(pk)), pk, np.concatenate(values), 8, 0.0, 1.0, PU.RANKS7, PU.BIG, PU.BIG)
    assert got.tolist() == want.tolist()
    assert counters == {"clamped": 0, "entered_raw0": 0, "picked_zero": 0}
    assert got[0].tolist() == [Q.empty_answer(0.0, 1.0, r) for r in PU.RANKS7]
    leaves, off = PU.pack_trees(trees)
    assert off.view(np.uint32).tolist() == np.concatenate([[0], np.cumsum(PU.WALK_SIZES)]).tolist()
    assert leaves.view(np.uint16)[off[7]:off[8]].tolist() == trees[7].tolist()


@pytest.mark.parametrize("kind", ["laplace", "gaussian"])
def test_with_noise_it_is_the_products_host_tree(kind):
    """quantile_tree.compute_quantiles shares nothing with the restatement but
    the specification; both read the same memoised draws."""
    trees = PU.walk_trees()
    got, counters = PU.walk_expected(kind)
    assert all(v > 0 for v in counters.values()), counters
    if kind == "laplace":
        assert counters["clamped"] > 1000, counters
    plain, _ = PU.walk_expected(None)
    for p in range(8):
        fn = PU.node_noise(PU.tree_of_leaves(trees[p], 0.0, 1.0), PU.noise(kind), PU.NOISE_SEED, 0, p)
        assert QT.compute_quantiles(trees[p], 0.0, 1.0, PU.RANKS7, add_noise=fn) == got[p].tolist()
        assert ((got[p] >= 0.0) & (got[p] <= 1.0)).all()
        if p > 0:
            assert (got[p] != plain[p]).any()
    assert got[:, 3].tolist() == got[:, 4].tolist()  # the repeated rank reads the same noisy tree


def test_stream_index_enters_as_specified():
    """The offset moves every partition's answers; equal trees under different
    stream indices differ; a walk keyed by (level, position) or without the
    offset would be another function."""
    base, _ = PU.walk_expected("laplace", 0, duplicate=True)
    assert base[:8].tolist() == PU.walk_expected("laplace")[0].tolist()
    for off in PU.OFFSETS:
        got, counters = PU.walk_expected("laplace", off, duplicate=True)
        assert all(v > 0 for v in counters.values())
        assert all((got[p] != base[p]).any() for p in range(9))
        assert (got[6] != got[8]).any()
    # index: a row per entry, NaN where the entry is no partition
    got, _ = PU.walk_expected("laplace", 0, partitions=tuple(PU.INDEX7))
    assert got[1].tolist() == got[2].tolist() == base[2].tolist() and got[0].tolist() == base[5].tolist()
    assert np.isnan(got[3]).all() and np.isnan(got[4]).all() and got[6].tolist() == base[7].tolist()


def test_sixty_four_ranks_on_the_smallest_trees():
    got, counters = PU.walk_expected("laplace", 0, tuple(PU.RANKS64), (0, 1, 2))
    assert got.shape == (3, 64) and all(v > 0 for v in counters.values())
    assert (np.diff(got, axis=1) >= 0.0).all()  # one noisy tree: ascending ranks, ascending answers
    trees = PU.walk_trees()
    for i, p in enumerate((0, 1, 2)):
        fn = PU.node_noise(PU.tree_of_leaves(trees[p], 0.0, 1.0), PU.noise("laplace"), PU.NOISE_SEED, 0, p)
        assert QT.compute_quantiles(trees[p], 0.0, 1.0, PU.RANKS64, add_noise=fn) == got[i].tolist()


# ------------------------------------------------- wide sorts and integers --
@pytest.mark.parametrize("P", PU.SORT_P)
def test_sort_tables_vary_every_key_byte(P):
    pid, pk, values = PU.sort_table(P)  # (the builder asserts; this runs it)
    assert len(pk) == 6000 and PU.partition_passes(P) == {255: 1, 256: 2, 257: 2, 65_535: 2, 65_536: 3, 70_000: 3}[P]
    idx = PU.sort_walk_index(P, pk, values)
    assert len(idx) == len(set(idx.tolist())) == len(set(pk[~np.isnan(values)].tolist())) + 3
    leaves, off = PU.leaves_of_rows(values, pk, np.arange(len(pk)), P, PU.SORT_LO, PU.SORT_HI)
    assert len(off) == P + 1 and off[-1] == len(leaves) == int((~np.isnan(values)).sum())
    p = P - 1
    assert leaves[off[p]:off[p + 1]].tolist() == np.sort(Q.leaf_index(values[pk == p], PU.SORT_LO, PU.SORT_HI)).tolist()


@pytest.mark.parametrize("n", PU.TILE_EDGE_N)
def test_tile_edge_tables(n):
    pid, pk, values = PU.sort_table(PU.TILE_EDGE_P, n)
    assert len(pk) == n and -(-n // PU.SORT_TILE) == (1 if n <= 2048 else 2)


@pytest.mark.parametrize("lo,hi", PU.INT_RANGES)
def test_integer_table_reaches_the_conversions_edges(lo, hi):
    pid, pk, values = PU.int_table(lo, hi)
    assert values.dtype == np.int64 and {values.min(), values.max()} == {np.iinfo(np.int64).min, np.iinfo(np.int64).max}
    leaves, off = PU.leaves_of_rows(values, pk, np.arange(len(pk)), 2, lo, hi)
    assert off[-1] == len(values) and leaves.min() == 0 and leaves.max() == Q.L - 1
