"""Private contribution bounds on the host (CPU): candidate generation, the L0
score's known answers from the reference's own tests
(tests/private_contribution_bounds_test.py), parity of the host score and
exponential-mechanism probabilities with the fixture recorded from the
reference, the stable softmax, the draw's distribution, and parameter
validation."""
import math

import numpy as np
import pytest

import pipelinedp_amd as pdp
from pipelinedp_amd import dp_computations
from pipelinedp_amd import private_contribution_bounds as pcb
from pipelinedp_amd.dataset_histograms import histograms as hist
from tests import private_bounds_util as U


def _params(**kw):
    """construct_params of the reference's test (private_contribution_bounds_test.py:8-17)."""
    base = dict(aggregation_noise_kind=pdp.NoiseKind.GAUSSIAN, aggregation_eps=0.9, aggregation_delta=0.1,
                calculation_eps=0.1, max_partitions_contributed_upper_bound=3)
    base.update(kw)
    return pdp.CalculatePrivateContributionBoundsParams(**base)


def _known_histogram():
    return hist.Histogram(hist.HistogramType.L0_CONTRIBUTIONS, [
        hist.FrequencyBin(lower=1, upper=2, count=100, sum=100, max=1),
        hist.FrequencyBin(lower=2, upper=6, count=10, sum=10, max=5),
        hist.FrequencyBin(lower=6, upper=100, count=20, sum=20, max=60)])


# ----------------------------------------------------------- candidates --
def test_generate_possible_contribution_bounds():
    expected = (list(range(1, 1000, 1)) + list(range(1000, 10000, 10)) + list(range(10000, 100000, 100)) +
                list(range(100000, 1000000, 1000)))
    assert pcb.generate_possible_contribution_bounds(999999) == expected


@pytest.mark.parametrize("upper,expected", [(0, []), (1, [1]), (2, [1, 2]), (1000, list(range(1, 1001))),
                                            (1009, list(range(1, 1001))), (1010, list(range(1, 1001)) + [1010])])
def test_generate_possible_contribution_bounds_edges(upper, expected):
    assert pcb.generate_possible_contribution_bounds(upper) == expected


# -------------------------------------------------------- scoring function --
def test_scoring_function_properties():
    assert pcb.L0ScoringFunction(None, 0, None).is_monotonic is True
    sf = pcb.L0ScoringFunction(_params(max_partitions_contributed_upper_bound=3), 100, None)
    assert sf.global_sensitivity == 3
    sf = pcb.L0ScoringFunction(_params(max_partitions_contributed_upper_bound=100), 10, None)
    assert sf.global_sensitivity == 10
    assert isinstance(sf, dp_computations.ExponentialMechanism.ScoringFunction)


@pytest.mark.parametrize("k,expected,places", [(1, -212.135, 3), (2, -354.270, 3), (5, -795.674, 3),
                                               (6, -942.809, 3), (60, -9428.09, 2), (61, -9585.23, 2),
                                               (101, -15870.6, 1), (200, -31427.0, 1)])
def test_score_laplace_known_answers(k, expected, places):
    params = _params(aggregation_noise_kind=pdp.NoiseKind.LAPLACE, aggregation_eps=0.9,
                     max_partitions_contributed_upper_bound=100)
    sf = pcb.L0ScoringFunction(params, 200, _known_histogram())
    # unittest's assertAlmostEqual(places): round(diff, places) == 0
    assert round(abs(sf.score(k) - expected), places) == 0


@pytest.mark.parametrize("k,expected", [(1, -336), (2, -437), (5, -638), (6, -688), (60, -2178), (61, -2196),
                                        (101, -2826), (200, -3977)])
def test_score_gaussian_known_answers(k, expected):
    params = _params(aggregation_noise_kind=pdp.NoiseKind.GAUSSIAN, aggregation_eps=0.9, aggregation_delta=0.001,
                     max_partitions_contributed_upper_bound=100)
    sf = pcb.L0ScoringFunction(params, 200, _known_histogram())
    assert abs(sf.score(k) - expected) <= 10


def test_count_noise_std():
    def std(kind, eps, delta, l0, linf):
        return dp_computations.compute_dp_count_noise_std(dp_computations.ScalarNoiseParams(
            eps=eps, delta=delta, min_value=None, max_value=None, min_sum_per_partition=None,
            max_sum_per_partition=None, max_partitions_contributed=l0, max_contributions_per_partition=linf,
            noise_kind=kind))

    assert std(pdp.NoiseKind.LAPLACE, 0.5, 0, 3, 2) == 3 * 2 / 0.5 * np.sqrt(2)
    assert std(pdp.NoiseKind.GAUSSIAN, 0.9, 1e-3, 4, 2) == dp_computations.compute_sigma(0.9, 1e-3, np.sqrt(4) * 2)


# ---------------------------------------------------------- fixture parity --
@pytest.mark.parametrize("fx", U.cases(), ids=U.case_ids())
def test_host_score_and_probabilities_match_reference(fx):
    sf = pcb.L0ScoringFunction(U.params(fx), fx["number_of_partitions"], U.l0_histogram(fx))
    assert sf._max_partitions_contributed_best_upper_bound() == fx["upper_bound"]
    assert sf.global_sensitivity == fx["global_sensitivity"]
    cands = pcb.generate_possible_contribution_bounds(fx["upper_bound"])
    assert cands == fx["candidates"]
    scores = [sf.score(k) for k in cands]
    np.testing.assert_allclose(scores, fx["scores"], rtol=U.RTOL, atol=0)
    probs = dp_computations.ExponentialMechanism(sf)._calculate_probabilities(fx["case"]["calc_eps"], cands)
    np.testing.assert_allclose(probs, fx["probabilities"], rtol=U.RTOL, atol=0)
    # the noise standard deviation (the Gaussian sigma) bit for bit
    std = [sf._l0_impact_noise(k) / fx["number_of_partitions"] for k in cands]
    assert std == fx["noise_std"]


@pytest.mark.parametrize("fx", U.cases(), ids=U.case_ids())
def test_calculator_on_host_histograms(fx):
    """PrivateL0Calculator with a host DatasetHistograms, as the reference's
    test builds it: the probabilities hook and a draw from the candidates."""
    dh = hist.DatasetHistograms(U.l0_histogram(fx), None, None, None, None, None, None)
    calc = pcb.PrivateL0Calculator(U.params(fx), fx["partitions"], [dh], None)
    cands, scores, probs = calc.probabilities()
    assert cands == fx["candidates"]
    np.testing.assert_allclose(scores, fx["scores"], rtol=U.RTOL, atol=0)
    np.testing.assert_allclose(probs, fx["probabilities"], rtol=U.RTOL, atol=0)
    out = calc.calculate()
    assert len(out) == 1 and out[0] in fx["candidates"]
    assert calc.calculate() is out  # computed once


def test_calculate_one_bound_has_much_higher_score_returns_it():
    params = _params(aggregation_eps=0.9, aggregation_delta=0, calculation_eps=0.1,
                     aggregation_noise_kind=pdp.NoiseKind.LAPLACE, max_partitions_contributed_upper_bound=2)
    l0 = hist.Histogram(hist.HistogramType.L0_CONTRIBUTIONS, [
        hist.FrequencyBin(lower=1, upper=2, count=1, sum=1, max=1),
        hist.FrequencyBin(lower=2, upper=3, count=10000, sum=10000, max=2)])
    dh = hist.DatasetHistograms(l0, None, None, None, None, None, None)
    calc = pcb.PrivateL0Calculator(params, list(range(1, 201)), [dh], None)
    assert list(calc.calculate())[0] == 2


# ----------------------------------------------------------- the mechanism --
class _Scores(dp_computations.ExponentialMechanism.ScoringFunction):

    def __init__(self, scores, sensitivity=1.0, monotonic=True):
        self._scores, self._sensitivity, self._monotonic = scores, sensitivity, monotonic

    def score(self, k):
        return self._scores[k]

    @property
    def global_sensitivity(self):
        return self._sensitivity

    @property
    def is_monotonic(self):
        return self._monotonic


def test_stable_softmax_where_the_naive_form_underflows():
    scores = {0: -5000.0, 1: -5001.0, 2: -5003.0}
    eps = 1.0
    with np.errstate(invalid="ignore"):
        naive = np.exp(np.array(list(scores.values())) * eps)
        assert not np.isfinite(naive / naive.sum()).any()  # 0 / 0
    probs = dp_computations.ExponentialMechanism(_Scores(scores))._calculate_probabilities(eps, [0, 1, 2])
    assert np.isfinite(probs).all() and abs(probs.sum() - 1) < 1e-15
    w = np.array([1.0, math.exp(-1), math.exp(-3)])
    np.testing.assert_allclose(probs, w / w.sum(), rtol=1e-15)


def test_non_monotonic_score_doubles_the_denominator():
    scores = {0: -1.0, 1: -3.0}
    mono = dp_computations.ExponentialMechanism(_Scores(scores, 2.0, True))._calculate_probabilities(1.0, [0, 1])
    non = dp_computations.ExponentialMechanism(_Scores(scores, 2.0, False))._calculate_probabilities(1.0, [0, 1])
    np.testing.assert_allclose(mono[1] / mono[0], math.exp(-1.0), rtol=1e-15)
    np.testing.assert_allclose(non[1] / non[0], math.exp(-0.5), rtol=1e-15)


def test_draw_distribution():
    """20,000 draws of ExponentialMechanism.apply over 4 candidates against
    its own probabilities: chi-square, p > 1e-4 (the reference's significance
    level for statistical tests)."""
    from scipy.stats import chisquare
    params = _params(aggregation_noise_kind=pdp.NoiseKind.LAPLACE, aggregation_eps=2.0, aggregation_delta=0,
                     calculation_eps=1.0, max_partitions_contributed_upper_bound=4)
    l0 = hist.Histogram(hist.HistogramType.L0_CONTRIBUTIONS, [
        hist.FrequencyBin(lower=1, upper=2, count=5, sum=5, max=1),
        hist.FrequencyBin(lower=3, upper=4, count=4, sum=12, max=3),
        hist.FrequencyBin(lower=4, upper=5, count=3, sum=12, max=4)])
    sf = pcb.L0ScoringFunction(params, 6, l0)
    mech = dp_computations.ExponentialMechanism(sf)
    cands = pcb.generate_possible_contribution_bounds(4)
    assert cands == [1, 2, 3, 4]
    probs = mech._calculate_probabilities(params.calculation_eps, cands)
    assert probs.min() > 0.02  # every candidate is drawn often enough for the test to see it
    n = 20000
    draws = np.array([mech.apply(params.calculation_eps, cands) for _ in range(n)])
    observed = np.array([(draws == k).sum() for k in cands])
    assert observed.sum() == n
    assert chisquare(observed, probs * n).pvalue > 1e-4


# -------------------------------------------------------------- validation --
@pytest.mark.parametrize("kw,error", [
    (dict(aggregation_eps=0), ValueError), (dict(aggregation_eps=-1), ValueError),
    (dict(aggregation_delta=-0.1), ValueError), (dict(aggregation_delta=1), ValueError),
    (dict(aggregation_noise_kind=None), ValueError),
    (dict(aggregation_noise_kind=pdp.NoiseKind.GAUSSIAN, aggregation_delta=0), ValueError),
    (dict(calculation_eps=0), ValueError), (dict(calculation_eps=-2), ValueError),
    (dict(max_partitions_contributed_upper_bound=0), ValueError),
    (dict(max_partitions_contributed_upper_bound=-3), ValueError),
    (dict(max_partitions_contributed_upper_bound=2.5), ValueError),
])
def test_params_validation(kw, error):
    with pytest.raises(error):
        _params(**kw)


def test_params_and_result_types():
    p = _params(aggregation_noise_kind=pdp.NoiseKind.LAPLACE, aggregation_delta=0)
    assert p.max_partitions_contributed_upper_bound == 3
    assert pdp.PrivateContributionBounds(max_partitions_contributed=7).max_partitions_contributed == 7


def test_engine_checks():
    ex = U.extractors()
    accountant = pdp.NaiveBudgetAccountant(total_epsilon=1.0, total_delta=1e-6)
    engine = pdp.DPEngine(accountant, pdp.ColumnarBackend())
    p = _params()
    with pytest.raises(ValueError, match="col must be non-empty"):
        engine.calculate_private_contribution_bounds([], p, ex, [1])
    with pytest.raises(ValueError, match="params must be set"):
        engine.calculate_private_contribution_bounds([(0, 1)], None, ex, [1])
    with pytest.raises(TypeError, match="params must be set"):
        engine.calculate_private_contribution_bounds([(0, 1)], pdp.SelectPartitionsParams(1), ex, [1])
    with pytest.raises(ValueError, match="data_extractors"):
        engine.calculate_private_contribution_bounds([(0, 1)], p, None, [1])
    with pytest.raises(TypeError, match="data_extractors"):
        engine.calculate_private_contribution_bounds([(0, 1)], p, object(), [1])


def test_other_backends_are_not_implemented():
    engine = pdp.DPEngine(pdp.NaiveBudgetAccountant(1.0, 1e-6), object())  # any backend but ColumnarBackend
    with pytest.raises(NotImplementedError, match="ColumnarBackend"):
        engine.calculate_private_contribution_bounds([(0, 1)], _params(), U.extractors(), [1])
