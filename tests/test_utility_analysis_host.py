"""Utility analysis on the host (no GPU): the NumPy restatement against the
fixture the reference produced (tests/golden/utility_analysis), the product's
configuration planning (budgets, std_noise, keep tables), the API dataclasses
and every NotImplementedError of UtilityAnalysisEngine.analyze."""
import math

import numpy as np
import pytest

import pipelinedp_amd as pdp
from pipelinedp_amd import _native as N
from pipelinedp_amd import analysis
from pipelinedp_amd.analysis import utility_analysis_engine as E
from tests import utility_analysis_util as U

FIXTURE = U.load_fixture()
IDS = [c["name"] for c in FIXTURE]


def test_fixture_is_complete():
    assert sorted(IDS) == sorted(c["name"] for c in U.fixture_cases())
    strategies = {s for c in FIXTURE for s in (c["multi"] or {}).get("partition_selection_strategy", [])}
    assert strategies == {"LAPLACE_THRESHOLDING", "GAUSSIAN_THRESHOLDING", "TRUNCATED_GEOMETRIC"}


@pytest.mark.parametrize("case", FIXTURE, ids=IDS)
def test_restatement_equals_fixture(case):
    """Every recorded value of the reference is within the derived bound of the
    restatement (equal, for the dyadic cases), with the product's keep tables."""
    plans = U.product_plans(case)
    pairs = U.case_pairs(case)
    cfgs = U.case_configurations(case)
    assert len(case["expected"]) == len(pairs) * len(cfgs)
    for e in case["expected"]:
        k = e["configuration"]
        got = dict(raw=e["raw"], keep=e["keep"], metrics=e["metrics"])
        U.check_against_restatement((case["name"], e["partition"], k), pairs[e["partition"]], cfgs[k],
                                    [m["aggregation"] for m in e["metrics"]], plans[k].keep_table, got,
                                    U.is_dyadic(case))


def test_fixture_covers_both_selection_paths_and_the_public_quirk():
    by_name = {c["name"]: c for c in FIXTURE}
    sizes = sorted(len(v[0]) for v in U.case_pairs(by_name["pre_private_each_strategy"]).values())
    assert sizes == [1, 7, 100, 101, 150]
    pub = by_name["raw_public_with_empty"]
    empty = [e for e in pub["expected"] if e["partition"] == 9]
    assert empty and all(e["raw"] == [1, 0] and e["keep"] is None for e in empty)
    # the (0, 0, 0) pair is clipped like any other: min_sum = 0.5 > 0 shows as a clipping error
    assert empty[0]["metrics"][0]["aggregation"] == "SUM" and empty[0]["metrics"][0]["clipping_to_min_error"] == 0.5
    # ... and every public partition has it, not only the empty one
    n_pairs = {pk: len(v[0]) for pk, v in U.case_pairs(dict(pub, public_partitions=None)).items()}
    assert [e["raw"][0] for e in pub["expected"] if e["partition"] == 0][0] == n_pairs[0] + 1


@pytest.mark.parametrize("case", FIXTURE, ids=IDS)
def test_budget_split_and_std_noise(case):
    """std_noise is host arithmetic: equal to the fixture, per configuration
    and metric; the budget is split over selection (private partitions only)
    and the metrics of one configuration, never across configurations."""
    plans = U.product_plans(case)
    public = case["public_partitions"] is not None
    n_mech = len(case["metrics"]) + (0 if public else 1)
    for k, plan in enumerate(plans):
        assert (plan.selection_spec is None) == public
        specs = ([] if public else [plan.selection_spec]) + plan.metric_specs
        assert len(specs) == n_mech
        assert math.isclose(sum(s.eps for s in specs), case["epsilon"], rel_tol=1e-12)
        recorded = next(e for e in case["expected"] if e["configuration"] == k)
        order = [m for m in U.METRIC_ORDER if m in case["metrics"]]
        assert [m["aggregation"] for m in recorded["metrics"]] == order
        assert [m["std_noise"] for m in recorded["metrics"]] == plan.std_noise
        assert {m["noise_kind"] for m in recorded["metrics"]} <= {plan.params.noise_kind.name}


def test_keep_table_ends_at_one_and_is_capped():
    case = next(c for c in FIXTURE if c["name"] == "pre_private_each_strategy")
    for plan in U.product_plans(case):
        t = plan.keep_table
        assert t[-1] == 1.0 and (t[:-1] < 1.0).all() and (np.diff(t) >= 0).all() and t[0] >= 0.0

    class Never:
        def probability_of_keep(self, n):
            return 0.5
    with pytest.raises(NotImplementedError, match="PDP_UA_MAX_KEEP_TABLE"):
        E.keep_probability_table(Never(), cap=1000)


def test_pre_threshold_shifts_the_keep_table():
    case = next(c for c in FIXTURE if c["name"] == "pre_private_pre_threshold")
    t = U.product_plans(case)[0].keep_table
    assert (t[:3] == 0.0).all() and t[3] > 0.0


def _params(**kw):
    base = dict(metrics=[pdp.Metrics.COUNT], noise_kind=pdp.NoiseKind.LAPLACE, max_partitions_contributed=2,
                max_contributions_per_partition=3)
    base.update(kw)
    return pdp.AggregateParams(**base)


def test_multi_parameter_configuration_validation_and_expansion():
    with pytest.raises(ValueError, match="at least 1"):
        analysis.MultiParameterConfiguration()
    with pytest.raises(ValueError, match="same length"):
        analysis.MultiParameterConfiguration(max_partitions_contributed=[1, 2], max_contributions_per_partition=[1])
    with pytest.raises(ValueError, match="both set or both None"):
        analysis.MultiParameterConfiguration(min_sum_per_partition=[1.0])
    multi = analysis.MultiParameterConfiguration(max_partitions_contributed=[1, 5], noise_kind=[
        pdp.NoiseKind.GAUSSIAN, pdp.NoiseKind.LAPLACE])
    assert multi.size == 2
    options = analysis.UtilityAnalysisOptions(1.0, 1e-5, _params(), multi)
    assert options.n_configurations == 2
    got = list(analysis.get_aggregate_params(options))
    assert [p.max_partitions_contributed for p in got] == [1, 5]
    assert [p.noise_kind for p in got] == [pdp.NoiseKind.GAUSSIAN, pdp.NoiseKind.LAPLACE]
    assert all(p.max_contributions_per_partition == 3 for p in got)
    assert options.aggregate_params.max_partitions_contributed == 2  # the blueprint is not modified
    single = analysis.UtilityAnalysisOptions(1.0, 1e-5, _params())
    assert single.n_configurations == 1 and list(analysis.get_aggregate_params(single)) == [single.aggregate_params]


def test_options_validation():
    for eps, delta in ((0.0, 1e-5), (-1.0, 1e-5), (1.0, -0.1), (1.0, 1.0)):
        with pytest.raises(ValueError):
            analysis.UtilityAnalysisOptions(eps, delta, _params())
    for prob in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="partitions_sampling_prob"):
            analysis.UtilityAnalysisOptions(1.0, 1e-5, _params(), partitions_sampling_prob=prob)


def _engine(backend=None):
    return analysis.UtilityAnalysisEngine(pdp.NaiveBudgetAccountant(1.0, 1e-5), backend or pdp.ColumnarBackend())


RAW = pdp.DataExtractors(privacy_id_extractor=lambda r: r[0], partition_extractor=lambda r: r[1],
                         value_extractor=lambda r: r[2])
PRE = pdp.PreAggregateExtractors(partition_extractor=lambda r: r[0], preaggregate_extractor=lambda r: r[1:])


def test_check_utility_analysis_params():
    eng = _engine()
    rows = [(0, 0, 1.0)]
    with pytest.raises(ValueError, match="PreAggregateExtractors"):
        eng.analyze(rows, analysis.UtilityAnalysisOptions(1.0, 1e-5, _params(), pre_aggregated_data=True), RAW)
    with pytest.raises(ValueError, match="DataExtractors should be specified"):
        eng.analyze(rows, analysis.UtilityAnalysisOptions(1.0, 1e-5, _params()), PRE)
    with pytest.raises(NotImplementedError, match="unsupported metric"):
        eng.analyze(rows, analysis.UtilityAnalysisOptions(1.0, 1e-5, _params(
            metrics=[pdp.Metrics.MEAN], min_value=0.0, max_value=1.0)), RAW)
    with pytest.raises(NotImplementedError, match="post_aggregation_thresholding"):
        eng.analyze(rows, analysis.UtilityAnalysisOptions(1.0, 1e-5, _params(
            metrics=[pdp.Metrics.PRIVACY_ID_COUNT], post_aggregation_thresholding=True)), RAW)
    with pytest.raises(NotImplementedError, match="already enforced"):
        eng.analyze(rows, analysis.UtilityAnalysisOptions(1.0, 1e-5, _params(
            contribution_bounds_already_enforced=True)), RAW)
    with pytest.raises(ValueError, match="can't be called"):
        eng.aggregate(rows, _params(), RAW)


def test_not_implemented_paths(monkeypatch):
    rows = [(0, 0, 1.0)]
    options = analysis.UtilityAnalysisOptions(1.0, 1e-5, _params())
    with pytest.raises(NotImplementedError, match="ColumnarBackend"):
        _engine(backend=object()).analyze(rows, options, RAW)
    with pytest.raises(NotImplementedError, match="partitions_sampling_prob"):
        _engine().analyze(rows, analysis.UtilityAnalysisOptions(1.0, 1e-5, _params(), partitions_sampling_prob=0.5),
                          RAW)
    too_many = analysis.MultiParameterConfiguration(max_partitions_contributed=[1] * (N.MAX_CONFIGURATIONS + 1))
    with pytest.raises(NotImplementedError, match="PDP_MAX_CONFIGURATIONS"):
        _engine().analyze(rows, analysis.UtilityAnalysisOptions(1.0, 1e-5, _params(), too_many), RAW)
    from pipelinedp_amd import parallel
    monkeypatch.setattr(parallel, "world_info", lambda group=None: (2, 0))
    with pytest.raises(NotImplementedError, match="one rank"):
        _engine().analyze(rows, options, RAW)


def test_preaggregate_matches_the_contribution_bounder():
    rows = [(1, "a", 2.0), (1, "a", 3.0), (1, "b", 1.0), (2, "a", 4.0)]
    got = sorted(analysis.preaggregate(rows, None, RAW))
    assert got == [("a", (1, 4.0, 1, 1)), ("a", (2, 5.0, 2, 3)), ("b", (1, 1.0, 2, 3))]
    with pytest.raises(NotImplementedError):
        analysis.preaggregate(rows, None, RAW, partitions_sampling_prob=0.5)


def test_c_abi_rejects_bad_arguments():
    import ctypes
    import os
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = N.lib()
    need = ctypes.c_uint64(0)
    assert lib.pdp_utility_analysis_workspace_bytes(1000, 10, 64, N.UA_COUNT, ctypes.byref(need)) == 0
    assert need.value >= 1000 * 40 + 3 * 10 * 64 * 8
    assert lib.pdp_utility_analysis_workspace_bytes(1000, 10, 64, N.UA_COUNT, None) == -1
    assert lib.pdp_utility_analysis_workspace_bytes(-1, 10, 64, N.UA_COUNT, ctypes.byref(need)) == -1
    assert lib.pdp_utility_analysis_workspace_bytes(1 << 31, 10, 64, N.UA_COUNT, ctypes.byref(need)) == -4
    assert lib.pdp_utility_analysis_workspace_bytes(10, 0, 64, N.UA_COUNT, ctypes.byref(need)) == -1
    assert lib.pdp_utility_analysis_workspace_bytes(10, 10, 0, N.UA_COUNT, ctypes.byref(need)) == -1
    assert lib.pdp_utility_analysis_workspace_bytes(10, 10, N.MAX_CONFIGURATIONS + 1, N.UA_COUNT,
                                                    ctypes.byref(need)) == -4
    assert b"PDP_MAX_CONFIGURATIONS" in lib.pdp_last_error()
    assert lib.pdp_utility_analysis_workspace_bytes(10, 10, 1, 0x100, ctypes.byref(need)) == -1
    assert lib.pdp_utility_analysis_workspace_bytes(10, 10, 1, N.UA_PUBLIC, ctypes.byref(need)) == -1

    buf = ctypes.create_string_buffer(4096 + 256)
    host = (ctypes.addressof(buf) + 255) & ~255  # never dereferenced: every call below is refused first
    params = (N.UaConfigParams * 1)(N.UaConfigParams(2, 3, 0.0, 1.0))
    offsets = (ctypes.c_int64 * 2)(0, 4)
    out = N.UaOutputs(host, host, host)

    def call(params=params, offsets=offsets, out=out, flags=N.UA_COUNT, tables=host, ws=host, ws_bytes=1 << 40,
             partition=host):
        return lib.pdp_utility_analysis(partition, host, host, host, 10, 10, params, 1, tables, offsets, flags,
                                        None if out is None else ctypes.byref(out), ws, ws_bytes, None)
    assert call(params=None) == -1 and b"params" in lib.pdp_last_error()
    assert call(out=None) == -1 and b"raw_statistics" in lib.pdp_last_error()
    assert call(out=N.UaOutputs(host, None, host)) == -1 and b"keep_probability" in lib.pdp_last_error()
    assert call(out=N.UaOutputs(host, host, None)) == -1 and b"metrics" in lib.pdp_last_error()
    assert call(partition=None) == -1 and b"pair columns" in lib.pdp_last_error()
    assert call(params=(N.UaConfigParams * 1)(N.UaConfigParams(0, 3, 0.0, 1.0))) == -1 and b"l0" in lib.pdp_last_error()
    assert call(params=(N.UaConfigParams * 1)(N.UaConfigParams(1, -1, 0.0, 1.0))) == -1
    nan = (N.UaConfigParams * 1)(N.UaConfigParams(1, 1, float("nan"), 1.0))
    assert call(params=nan, flags=N.UA_SUM) == -1 and b"NaN" in lib.pdp_last_error()
    assert call(offsets=None) == -1 and b"keep_offsets" in lib.pdp_last_error()
    assert call(offsets=(ctypes.c_int64 * 2)(1, 4)) == -1
    assert call(offsets=(ctypes.c_int64 * 2)(0, -1)) == -1
    assert call(offsets=(ctypes.c_int64 * 2)(0, N.UA_MAX_KEEP_TABLE + 1)) == -4
    assert b"PDP_UA_MAX_KEEP_TABLE" in lib.pdp_last_error()
    assert call(tables=None) == -1 and b"keep_tables" in lib.pdp_last_error()
    assert call(ws=None) == -3
    assert call(ws_bytes=16) == -3 and b"workspace too small" in lib.pdp_last_error()
    assert call(ws=host + 8) == -1 and b"aligned" in lib.pdp_last_error()
