"""DPEngine.calculate_private_contribution_bounds on the GPU: the row filter
(`pdp_filter_rows`) against NumPy, the score kernel (`pdp_l0_impact_dropped`)
against its definition in Python integers, and the whole call on
ColumnarBackend against the fixture recorded from the reference
(tests/golden/private_bounds, tools/gen_golden_private_bounds.py)."""
import numpy as np
import pytest
import torch

import pipelinedp_amd as pdp
from pipelinedp_amd import _native as N
from pipelinedp_amd import executor as X
from pipelinedp_amd.dataset_histograms.computing_histograms import log_bin_bounds
from tests import private_bounds_util as U

pytestmark = pytest.mark.gpu

MASKS = ("all", "none", "alternating", "single")


def _mask(kind, P):
    m = np.zeros(P, dtype=np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "alternating":
        m[::2] = 1
    elif kind == "single":
        m[P // 2] = 1
    return m


def _pairs(pid, pk):
    """The multiset of (pid, pk) rows as a sorted [n, 2] array."""
    a = np.stack([np.asarray(pid), np.asarray(pk)], axis=1) if len(pid) else np.zeros((0, 2), np.int64)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def _check_filter(device, pid, pk, mask, P):
    got_pid, got_pk = X.filter_rows(torch.as_tensor(pid).to(device), torch.as_tensor(pk).to(device),
                                    torch.as_tensor(mask).to(device), n_partitions=P)
    keep = mask[pk] != 0
    assert got_pid.numel() == got_pk.numel() == int(keep.sum())
    np.testing.assert_array_equal(_pairs(got_pid.cpu().numpy(), got_pk.cpu().numpy()), _pairs(pid[keep], pk[keep]))


# ------------------------------------------------------------ filter kernel --
@pytest.mark.parametrize("P", [1, 100_003])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025, 70_001])
def test_filter_rows_against_numpy(device, n, P):
    rng = np.random.default_rng(n * 7 + P)
    pid = rng.integers(0, 1 << 40, n).astype(np.int64)
    pk = rng.integers(0, P, n).astype(np.int64)
    if n:
        pk[-1] = P - 1  # the last partition, in the ragged tail
    for kind in MASKS:
        _check_filter(device, pid, pk, _mask(kind, P), P)


def test_filter_rows_unaligned_columns(device):
    """Columns 8 bytes off a 16-byte boundary take the scalar-load kernel."""
    n, P = 5000, 37
    rng = np.random.default_rng(5)
    pid = torch.as_tensor(rng.integers(0, 1000, n + 1)).to(device)[1:]
    pk = torch.as_tensor(rng.integers(0, P, n + 1)).to(device)[1:]
    assert pid.data_ptr() % 16 == 8 and pk.data_ptr() % 16 == 8
    mask = _mask("alternating", P)
    got_pid, got_pk = X.filter_rows(pid, pk, torch.as_tensor(mask).to(device), n_partitions=P)
    keep = mask[pk.cpu().numpy()] != 0
    np.testing.assert_array_equal(_pairs(got_pid.cpu().numpy(), got_pk.cpu().numpy()),
                                  _pairs(pid.cpu().numpy()[keep], pk.cpu().numpy()[keep]))


@pytest.mark.parametrize("bad", [-1, 50, 1 << 40])
def test_filter_rows_out_of_range_partition(device, bad):
    """A partition code outside [0, P) sets the error word; the mask is not
    read for it (the kernel guards the read)."""
    n, P = 3000, 50
    rng = np.random.default_rng(9)
    pid = rng.integers(0, 100, n).astype(np.int64)
    pk = rng.integers(0, P, n).astype(np.int64)
    pk[n // 2] = bad
    with pytest.raises(ValueError, match="dense key range"):
        X.filter_rows(torch.as_tensor(pid).to(device), torch.as_tensor(pk).to(device),
                      torch.as_tensor(_mask("all", P)).to(device), n_partitions=P)
    # unchecked, the row is dropped and the others pass
    got_pid, got_pk = X.filter_rows(torch.as_tensor(pid).to(device), torch.as_tensor(pk).to(device),
                                    torch.as_tensor(_mask("all", P)).to(device), n_partitions=P, check_keys=False)
    ok = np.arange(n) != n // 2
    np.testing.assert_array_equal(_pairs(got_pid.cpu().numpy(), got_pk.cpu().numpy()), _pairs(pid[ok], pk[ok]))


# ------------------------------------------------------------- score kernel --
def _dropped(device, bins, B, candidates):
    row = U.dense_l0_counts(bins)
    got = X.l0_impact_dropped(torch.as_tensor(row).to(device), B,
                              torch.as_tensor(np.asarray(candidates, dtype=np.int64)).to(device))
    want = U.impact_dropped(row, B, candidates)
    assert all(w < 2**63 for w in want)
    assert got.dtype == torch.int64
    assert got.cpu().tolist() == want
    return want


def test_score_kernel_bin_lowers_match_log_bin_bounds():
    assert [log_bin_bounds(b)[0] for b in (0, 999, 1000, 1001, 1900, 2800)] == [0, 999, 1000, 1010, 10000, 100000]


@pytest.mark.parametrize("m", [1, 64, 65, 2800])
def test_score_kernel_candidate_counts(device, m):
    bins = [(1, 500), (2, 300), (7, 11), (999, 3), (1000, 2), (1010, 1), (12300, 4)]
    cands = list(range(1, m + 1)) if m < 2800 else \
        list(range(1, 1000)) + list(range(1000, 10000, 10)) + list(range(10000, 100000, 100)) + [100000]
    assert len(cands) == m
    want = _dropped(device, bins, 20000, cands)
    assert want[0] > 0


def test_score_kernel_empty_histogram(device):
    assert set(_dropped(device, [], 100, list(range(1, 101)))) == {0}


def test_score_kernel_small_bins_only(device):
    _dropped(device, [(1, 10), (3, 7), (500, 2), (999, 1)], 1000, [1, 2, 3, 499, 500, 998, 999, 1000])


def test_score_kernel_wide_bins(device):
    """Bins at dense indices >= 1000: lowers 1,000 and 1,010, one in the 10,000 decade."""
    want = _dropped(device, [(5, 3), (1000, 2), (1010, 5), (45600, 1)], 100000, [1, 999, 1000, 1005, 1010, 45600, 45700])
    assert want[3] == 5 * 5 + (45600 - 1005)


def test_score_kernel_upper_bound_clamps_lowers(device):
    want = _dropped(device, [(2, 4), (50, 3), (1010, 2), (20000, 1)], 40, [1, 10, 39, 40, 41])
    assert want[1] == (40 - 10) * (3 + 2 + 1)


def test_score_kernel_all_candidates_above_every_lower(device):
    assert set(_dropped(device, [(1, 9), (17, 4), (1020, 1)], 5000, [1020, 1030, 4000, 5000])) == {0}


def test_score_kernel_products_beyond_32_bits(device):
    """Counts near 2^31 with the bound near 1e6: products above 2^32, sums below 2^63."""
    want = _dropped(device, [(3, 2**31 - 5), (999000, 2**31 - 1), (2000000, 7)], 1_000_000, [1, 2, 1000, 999000])
    assert want[0] > 2**50


def test_score_kernel_rejects_bounds_that_could_overflow(device):
    row = torch.zeros(N.HIST_LOG_BINS, dtype=torch.int64, device=device)
    cand = torch.ones(1, dtype=torch.int64, device=device)
    assert X.l0_impact_dropped(row, 1 << 32, cand).cpu().tolist() == [0]
    with pytest.raises(N.NativeLibraryError, match="code -4"):
        X.l0_impact_dropped(row, (1 << 32) + 1, cand)


# ------------------------------------------------------------- end to end --
def _engine():
    return pdp.DPEngine(pdp.NaiveBudgetAccountant(total_epsilon=1.0, total_delta=1e-6), pdp.ColumnarBackend())


def _table(rows):
    pks = [r[1] for r in rows]
    pk_col = np.asarray(pks, dtype=np.int64) if isinstance(pks[0], int) else np.asarray(pks, dtype=object)
    return pdp.ColumnTable({"user": np.asarray([r[0] for r in rows], dtype=np.int64), "part": pk_col})


def _check_against_fixture(engine, fx):
    calc = engine._last_private_l0_calculator
    (raw,) = calc._histograms
    host = {k: raw[k][0].cpu().numpy() for k in ("int_count", "int_sum", "int_max")}
    present = np.flatnonzero(host["int_count"]).tolist()
    got_bins = [[*log_bin_bounds(b), int(host["int_count"][b]), int(host["int_sum"][b]), int(host["int_max"][b])]
                for b in present]
    assert got_bins == fx["l0_bins"]
    sf = calc.scoring_function()
    assert sf._number_of_partitions == fx["number_of_partitions"]
    assert sf.global_sensitivity == fx["upper_bound"] == fx["global_sensitivity"]
    cands, scores, probs = calc.probabilities()
    assert cands == fx["candidates"]
    np.testing.assert_allclose(scores, fx["scores"], rtol=U.RTOL, atol=0)
    np.testing.assert_allclose(probs, fx["probabilities"], rtol=U.RTOL, atol=0)


@pytest.mark.parametrize("as_table", [False, True], ids=["rows", "table"])
@pytest.mark.parametrize("fx", U.cases(), ids=U.case_ids())
def test_calculate_private_contribution_bounds_matches_reference(device, fx, as_table):
    engine = _engine()
    if as_table:
        col = _table(U.rows(fx))
        ex = pdp.DataExtractors(privacy_id_extractor=pdp.ColumnExtractor("user"),
                                partition_extractor=pdp.ColumnExtractor("part"))
    else:
        col, ex = U.rows(fx), U.extractors()
    out = engine.calculate_private_contribution_bounds(col, U.params(fx), ex, fx["partitions"])
    assert len(out) == 1 and isinstance(out[0], pdp.PrivateContributionBounds)
    assert out[0].max_partitions_contributed in fx["candidates"]
    _check_against_fixture(engine, fx)


def test_partitions_already_filtered(device):
    fx = next(c for c in U.cases() if c["name"] == "laplace_partitions_drop_rows")
    kept = set(fx["partitions"])
    rows = [r for r in U.rows(fx) if r[1] in kept]
    assert len(rows) == fx["rows_kept"] < len(fx["rows"])
    engine = _engine()
    out = engine.calculate_private_contribution_bounds(rows, U.params(fx), U.extractors(), fx["partitions"],
                                                       partitions_already_filtered=True)
    assert out[0].max_partitions_contributed in fx["candidates"]
    _check_against_fixture(engine, fx)


def test_one_bound_has_much_higher_score_returns_it(device):
    """The reference's test_calculate_one_bound_has_much_higher_score_returns_it
    from rows: one user in 1 partition, 10,000 users in 2, 200 partitions, upper
    bound 2.  With a very large calculation_eps the draw is the argmax: 2."""
    users = np.concatenate([[0], np.repeat(np.arange(1, 10001), 2)]).astype(np.int64)
    parts = np.ones(20001, dtype=np.int64)                  # user 0: partition 1
    parts[1::2] = 1 + (np.arange(10000) % 100) * 2          # two distinct partitions of 1..200 per user
    parts[2::2] = 2 + (np.arange(10000) % 100) * 2
    table = pdp.ColumnTable({"user": users, "part": parts})
    ex = pdp.DataExtractors(privacy_id_extractor=pdp.ColumnExtractor("user"),
                            partition_extractor=pdp.ColumnExtractor("part"))
    params = pdp.CalculatePrivateContributionBoundsParams(
        aggregation_noise_kind=pdp.NoiseKind.LAPLACE, aggregation_eps=0.9, aggregation_delta=0,
        calculation_eps=1e4, max_partitions_contributed_upper_bound=2)
    engine = _engine()
    out = engine.calculate_private_contribution_bounds(table, params, ex, list(range(1, 201)))
    assert out == [pdp.PrivateContributionBounds(max_partitions_contributed=2)]
    cands, scores, probs = engine._last_private_l0_calculator.probabilities()
    assert cands == [1, 2]
    # score(1) = -0.5 * 200 * 1 / 0.9 * sqrt(2) - 0.5 * 10000, score(2) = -0.5 * 200 * 2 / 0.9 * sqrt(2)
    np.testing.assert_allclose(scores, [-100 / 0.9 * np.sqrt(2) - 5000, -200 / 0.9 * np.sqrt(2)], rtol=U.RTOL)
    assert probs.tolist() == [0.0, 1.0]


def test_every_row_filtered_out(device):
    """No row is in `partitions`: empty histograms, the noise term alone decides."""
    fx = U.cases()[0]
    engine = _engine()
    out = engine.calculate_private_contribution_bounds(U.rows(fx), U.params(fx), U.extractors(), [10**6, 10**6 + 1])
    assert out[0].max_partitions_contributed in (1, 2)
    cands, scores, _ = engine._last_private_l0_calculator.probabilities()
    assert cands == [1, 2]
    np.testing.assert_allclose(scores, [-0.5 * 2 * k / fx["case"]["eps"] * np.sqrt(2) for k in cands], rtol=U.RTOL)
