"""Utility analysis on the GPU (pdp_utility_analysis, csrc/pdp_analysis.hip):
fixture parity through UtilityAnalysisEngine.analyze, the kernels' edge shapes
against the NumPy restatement under the derived tolerances
(tests/utility_analysis_util.py), and bitwise reproducibility."""
import functools

import numpy as np
import pytest

import pipelinedp_amd as pdp
from pipelinedp_amd import _native as N
from pipelinedp_amd import analysis
from pipelinedp_amd import partition_selection
from pipelinedp_amd.analysis import utility_analysis_engine as E
from tests import utility_analysis_util as U

pytestmark = pytest.mark.gpu

FIXTURE = U.load_fixture()


@pytest.mark.parametrize("case", FIXTURE, ids=[c["name"] for c in FIXTURE])
def test_fixture_parity(case):
    """Raw and pre-aggregated rows, public partitions (one of them empty) and
    private ones with each selection strategy, both noise kinds."""
    lib = U.product_lib()
    options, ext, col, public = U.build_options(case, lib)
    engine = lib.UtilityAnalysisEngine(lib.NaiveBudgetAccountant(case["epsilon"], case["delta"]),
                                       pdp.ColumnarBackend(seed=1))
    result = engine.analyze(col, options, ext, public)
    assert result.n_configurations == options.n_configurations
    got = dict(result.rows())
    recorded = {(e["partition"], e["configuration"]): e for e in case["expected"]}
    assert sorted(got) == sorted(recorded)
    plans, pairs, cfgs = U.product_plans(case), U.case_pairs(case), U.case_configurations(case)
    for (pk, k), m in got.items():
        e = recorded[(pk, k)]
        names = [x["aggregation"] for x in e["metrics"]]
        assert [str(x.aggregation) for x in m.metric_errors] == names
        assert [x.std_noise for x in m.metric_errors] == [x["std_noise"] for x in e["metrics"]]
        assert [x.noise_kind.name for x in m.metric_errors] == [x["noise_kind"] for x in e["metrics"]]
        mine = dict(raw=[m.raw_statistics.privacy_id_count, m.raw_statistics.count],
                    keep=m.partition_selection_probability_to_keep,
                    metrics=[{f: getattr(x, f) for f in U.FIELDS} for x in m.metric_errors])
        assert mine["raw"] == e["raw"]
        U.check_against_restatement((case["name"], pk, k), pairs[pk], cfgs[k], names, plans[k].keep_table, mine,
                                    U.is_dyadic(case), recorded=e)


# ------------------------------------------------------------ edge shapes --
# Dyadic pairs (integer counts and sums, n_partitions and l0 powers of two):
# every term and moment is exact.  Partition sizes 1, 100 and 101 straddle the
# exact / approximate selection paths, 5,000 > the 4,096-pair chunk runs the
# segment split and combine, partition 4 has q = 1 for every pair of its 101
# (sigma == 0), partition 5 has pairs with n_partitions == 0; partition 6 is empty.
SIZES = (1, 100, 101, 5000, 101, 3)
N_PARTITIONS = 7
BOUNDS = ((0.0, 5.0), (2.0, 2.0), (-3.0, 11.0), (-8.0, -1.0), (4.0, 64.0))  # sums span [-3, 11]


def _edge_pairs():
    rng = np.random.default_rng(7)
    pk, cnt, sm, npart = [], [], [], []
    for p, size in enumerate(SIZES):
        pk += [p] * size
        cnt += [int(v) for v in rng.integers(0, 6, size)]
        sm += [float(v) for v in rng.integers(-3, 12, size)]
        if p == 4:
            npart += [1] * size
        elif p == 5:
            npart += [0, 0, 2]
        else:
            npart += [int(2 ** v) for v in rng.integers(0, 5, size)]
    order = rng.permutation(len(pk))
    return tuple(np.asarray(a)[order] for a in (pk, cnt, sm, npart))


def _edge_configurations(k):
    return [dict(l0=(1, 2, 4, 8)[i % 4], linf=(1, 2, 4)[i % 3], min_sum=BOUNDS[i % 5][0], max_sum=BOUNDS[i % 5][1])
            for i in range(k)]


@functools.lru_cache(maxsize=None)
def _keep_tables():
    return {l0: E.keep_probability_table(partition_selection.create_partition_selection_strategy(
        pdp.PartitionSelectionStrategy.TRUNCATED_GEOMETRIC, 1.0, 1e-4, l0)) for l0 in (1, 2, 4, 8)}


@pytest.fixture(scope="module")
def edge():
    import torch
    pk, cnt, sm, npart = _edge_pairs()
    dev = torch.device("cuda:0")
    tensors = (torch.as_tensor(pk, dtype=torch.int64, device=dev), torch.as_tensor(cnt, dtype=torch.int64, device=dev),
               torch.as_tensor(sm, dtype=torch.float64, device=dev),
               torch.as_tensor(npart, dtype=torch.int64, device=dev))
    by_partition = {p: (cnt[pk == p], sm[pk == p], npart[pk == p]) for p in range(N_PARTITIONS)}
    return dict(tensors=tensors, pairs=by_partition, tables=_keep_tables(), restated={})


def _run(edge, k, flags=N.UA_SUM | N.UA_COUNT | N.UA_PRIVACY_ID_COUNT, public=False):
    cfgs = _edge_configurations(k)
    tables = None if public else [edge["tables"][c["l0"]] for c in cfgs]
    out = E.run_utility_analysis(*edge["tensors"], N_PARTITIONS,
                                 [(c["l0"], c["linf"], c["min_sum"], c["max_sum"]) for c in cfgs], tables, flags)
    return cfgs, out


@pytest.mark.parametrize("k", [1, 64, 65])
def test_edge_shapes_against_restatement(edge, k):
    cfgs, out = _run(edge, k)
    raw = out["raw_statistics"].cpu().numpy()
    keep = out["keep_probability"].cpu().numpy()
    metrics = out["metrics"].cpu().numpy()
    assert metrics.shape == (3, 5, N_PARTITIONS, k) and keep.shape == (N_PARTITIONS, k)
    paths = set()
    for p in range(N_PARTITIONS):
        cnt, sm, npart = edge["pairs"][p]
        assert list(raw[p]) == [len(cnt), int(cnt.sum())]
        for c, cfg in enumerate(cfgs):
            key = (p, c % 60)  # the configurations repeat with period lcm(4, 3, 5)
            if key not in edge["restated"]:
                vals = [U.restate_metric(m, cnt, sm, npart, cfg)[0] for m in U.METRIC_ORDER]
                edge["restated"][key] = (vals, U.restate_keep(npart, cfg["l0"],
                                                              U.keep_fn_of_table(edge["tables"][cfg["l0"]])))
            vals, (kv, path, m) = edge["restated"][key]
            paths.add(path)
            for mi in range(3):
                for fi, f in enumerate(U.FIELDS):  # dyadic inputs: equality
                    assert metrics[mi, fi, p, c] == vals[mi][f], (p, c, U.METRIC_ORDER[mi], f)
            bound = U.keep_bound(kv, path, len(npart), m)
            assert abs(keep[p, c] - kv) <= bound, (p, c, path, keep[p, c], kv, abs(keep[p, c] - kv), bound)
    assert paths == {"exact", "approx"}
    # sigma == 0 (q = 1 for all 101 pairs): the PMF is one point at 101
    for c, cfg in enumerate(cfgs):
        assert keep[4, c] == U.keep_fn_of_table(edge["tables"][cfg["l0"]])(101)
    # the empty partition: no pairs, keep table entry 0
    assert (raw[6] == 0).all() and (metrics[:, :, 6, :] == 0).all() and (keep[6] == 0).all()


def test_metric_subsets_and_public_flag(edge):
    """Each metric alone, in its own output slot; PDP_UA_PUBLIC writes no selection probability."""
    _, full = _run(edge, 5)
    for slot, flag in enumerate((N.UA_SUM, N.UA_COUNT, N.UA_PRIVACY_ID_COUNT)):
        _, one = _run(edge, 5, flags=flag, public=True)
        assert one["keep_probability"] is None
        assert one["metrics"].shape[0] == 1
        assert (one["metrics"][0] == full["metrics"][slot]).all()
        assert (one["raw_statistics"] == full["raw_statistics"]).all()
    _, select_only = _run(edge, 5, flags=0)
    assert (select_only["keep_probability"] == full["keep_probability"]).all()


def test_two_runs_are_bitwise_equal(edge):
    import torch
    _, a = _run(edge, 65)
    _, b = _run(edge, 65)
    for name in ("raw_statistics", "keep_probability", "metrics"):
        assert torch.equal(a[name].view(torch.int64), b[name].view(torch.int64)), name


# ---------------------------------------------------- segment split shapes --
# 300 partitions: 9-bit sort keys, so the radix sort runs two passes.  In sorted
# order partition 3 (4,096 pairs, one chunk, reduced whole) fills tile 0;
# partition 4 (4,097 > a chunk) starts exactly on the tile boundary 4,096 and
# leaves one pair in tile 2; partition 260 (5,000) starts inside that same tile
# at 8,193, so tile 2 writes both of its partial slots, and ends inside tile 3;
# partition 299 has 3 pairs.  The other 296 partitions, those between the two
# long ones included, are empty.
SPLIT_CODES = (3, 4, 260, 299)
SPLIT_SIZES = (4096, 4097, 5000, 3)
SPLIT_PARTITIONS = 300
SPLIT_K = 65


def _split_pairs():
    rng = np.random.default_rng(11)
    pk, cnt, sm, npart = [], [], [], []
    for p, size in zip(SPLIT_CODES, SPLIT_SIZES):
        pk += [p] * size
        cnt += [int(v) for v in rng.integers(0, 6, size)]
        sm += [float(v) for v in rng.integers(-3, 12, size)]
        npart += [int(2 ** v) for v in rng.integers(0, 5, size)]
    order = rng.permutation(len(pk))
    return tuple(np.asarray(a)[order] for a in (pk, cnt, sm, npart))


@pytest.fixture(scope="module")
def split():
    import torch
    pk, cnt, sm, npart = _split_pairs()
    dev = torch.device("cuda:0")
    tensors = (torch.as_tensor(pk, dtype=torch.int64, device=dev), torch.as_tensor(cnt, dtype=torch.int64, device=dev),
               torch.as_tensor(sm, dtype=torch.float64, device=dev),
               torch.as_tensor(npart, dtype=torch.int64, device=dev))
    by_partition = {p: (cnt[pk == p], sm[pk == p], npart[pk == p]) for p in SPLIT_CODES}
    return dict(tensors=tensors, pairs=by_partition, tables=_keep_tables(), restated={})


def _run_split(split):
    cfgs = _edge_configurations(SPLIT_K)
    out = E.run_utility_analysis(*split["tensors"], SPLIT_PARTITIONS,
                                 [(c["l0"], c["linf"], c["min_sum"], c["max_sum"]) for c in cfgs],
                                 [split["tables"][c["l0"]] for c in cfgs],
                                 N.UA_SUM | N.UA_COUNT | N.UA_PRIVACY_ID_COUNT)
    return cfgs, out


def test_segment_split_shapes_against_restatement(split):
    import torch
    cfgs, out = _run_split(split)
    raw = out["raw_statistics"].cpu().numpy()
    keep = out["keep_probability"].cpu().numpy()
    metrics = out["metrics"].cpu().numpy()
    assert metrics.shape == (3, 5, SPLIT_PARTITIONS, SPLIT_K) and keep.shape == (SPLIT_PARTITIONS, SPLIT_K)
    for p, size in zip(SPLIT_CODES, SPLIT_SIZES):
        cnt, sm, npart = split["pairs"][p]
        assert len(cnt) == size and list(raw[p]) == [size, int(cnt.sum())]
        for c, cfg in enumerate(cfgs):
            key = (p, c % 60)  # the configurations repeat with period lcm(4, 3, 5)
            if key not in split["restated"]:
                vals = [U.restate_metric(m, cnt, sm, npart, cfg)[0] for m in U.METRIC_ORDER]
                split["restated"][key] = (vals, U.restate_keep(npart, cfg["l0"],
                                                               U.keep_fn_of_table(split["tables"][cfg["l0"]])))
            vals, (kv, path, m) = split["restated"][key]
            for mi in range(3):
                for fi, f in enumerate(U.FIELDS):  # dyadic inputs: equality
                    assert metrics[mi, fi, p, c] == vals[mi][f], (p, c, U.METRIC_ORDER[mi], f)
            bound = U.keep_bound(kv, path, len(npart), m)
            assert abs(keep[p, c] - kv) <= bound, (p, c, path, keep[p, c], kv, abs(keep[p, c] - kv), bound)
    empty = np.setdiff1d(np.arange(SPLIT_PARTITIONS), SPLIT_CODES)
    assert len(empty) == 296
    assert (raw[empty] == 0).all() and (metrics[:, :, empty, :] == 0).all() and (keep[empty] == 0).all()
    _, again = _run_split(split)
    for name in ("raw_statistics", "keep_probability", "metrics"):
        assert torch.equal(out[name].view(torch.int64), again[name].view(torch.int64)), name


def test_out_of_range_partition_is_reported(edge):
    import torch
    pk, cnt, sm, npart = edge["tensors"]
    bad = pk.clone()
    bad[0] = N_PARTITIONS
    with pytest.raises(ValueError, match="outside the declared range"):
        E.run_utility_analysis(bad, cnt, sm, npart, N_PARTITIONS, [(1, 1, 0.0, 1.0)], None, N.UA_COUNT)
    assert torch.equal(pk, edge["tensors"][0])


def test_too_many_configurations():
    import torch
    z = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    with pytest.raises(NotImplementedError, match="PDP_MAX_CONFIGURATIONS"):
        E.run_utility_analysis(z, z, z.double(), z, 1, [(1, 1, 0.0, 1.0)] * (N.MAX_CONFIGURATIONS + 1), None,
                               N.UA_COUNT)


def test_columnar_result_shapes():
    case = next(c for c in FIXTURE if c["name"] == "raw_private_truncated_geometric")
    lib = U.product_lib()
    options, ext, col, public = U.build_options(case, lib)
    result = analysis.UtilityAnalysisEngine(lib.NaiveBudgetAccountant(2.0, 1e-5), pdp.ColumnarBackend()).analyze(
        col, options, ext, public)
    p, k = len(result), result.n_configurations
    assert (p, k) == (5, 3) and tuple(result.keep_probability.shape) == (p, k)
    assert result.keep_probability.is_cuda and [str(m) for m in result.metric_names] == list(U.METRIC_ORDER)
    assert all(tuple(result.metrics[m][f].shape) == (p, k) for m in range(3) for f in U.FIELDS)
    host = result.numpy()
    assert isinstance(host.keep_probability, np.ndarray) and host.raw_statistics.shape == (p, 2)
