"""PERCENTILE and VECTOR_SUM under a process group: two ranks (gloo, sharing
the one GPU), rows sharded by privacy id, give the single-process result by
EQUALITY.  The rows are ordered by owner rank, so a row's global index is the
same in both runs and the bounder keeps the same rows; a partition's merged
leaf array (parallel.exchange_quantile_leaves + executor.merge_quantile_leaves)
is then the single process's, its noise stream is keyed by the global partition
index, and the integer-valued vectors sum exactly in any order."""
import os
import socket

import numpy as np
import pytest

import pipelinedp_amd as pdp
from pipelinedp_amd import columnar_backend as CB

pytestmark = pytest.mark.gpu

P_ROWS, P_ALL, D = 12, 13, 3  # partition 12 is public and has no rows; 13 pads to 14 over two ranks


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_data():
    rng = np.random.default_rng(77)
    n, U = 6_000, 2_000  # ~460 privacy ids a partition: private selection keeps them at eps = 1
    pid = rng.integers(0, U, n)
    pk = rng.integers(0, P_ROWS, n)
    v = rng.normal(40.0, 25.0, n)  # some values beyond [0, 100]: clamped into the end leaves
    vec = rng.integers(-4, 5, (n, D)).astype(np.float64)
    owner = pid % 2  # privacy ids never span ranks
    order = np.argsort(owner, kind="stable")  # rank 0's rows first, then rank 1's
    return pid[order], pk[order], v[order], vec[order], owner[order], U


def _ext():
    return pdp.DataExtractors(privacy_id_extractor=pdp.ColumnExtractor("pid"),
                              partition_extractor=pdp.ColumnExtractor("pk"),
                              value_extractor=pdp.ColumnExtractor("v"))


def _table(pid, pk, v, U):
    return pdp.ColumnTable({"pid": pid, "pk": pk, "v": v}, n_privacy_ids=U, n_partitions=P_ALL)


def _aggregate(table, params, *, public=None, seed, sharding="verify"):
    backend = CB.ColumnarBackend(seed=seed, privacy_id_sharding=sharding)
    acc = pdp.NaiveBudgetAccountant(total_epsilon=1.0, total_delta=1e-6)
    sink = pdp.DPEngine(acc, backend).aggregate(table, params, _ext(), public_partitions=public)
    acc.compute_budgets()
    return [(int(k), [np.asarray(x, np.float64).tolist() for x in m]) for k, m in sink]


def _percentile_params():
    return pdp.AggregateParams(metrics=[pdp.Metrics.COUNT, pdp.Metrics.PRIVACY_ID_COUNT, pdp.Metrics.PERCENTILE(10),
                                        pdp.Metrics.PERCENTILE(50), pdp.Metrics.PERCENTILE(99.5)],
                               noise_kind=pdp.NoiseKind.LAPLACE, max_partitions_contributed=3,
                               max_contributions_per_partition=2, min_value=0.0, max_value=100.0)


PUBLIC = [p for p in range(P_ALL) if p != 5]  # partition 5's rows are dropped; 12 has none


def _vector_params(l0, linf):
    return pdp.AggregateParams(metrics=[pdp.Metrics.VECTOR_SUM, pdp.Metrics.COUNT],
                               noise_kind=pdp.NoiseKind.LAPLACE, max_partitions_contributed=l0,
                               max_contributions_per_partition=linf, vector_size=D, vector_max_norm=40.0,
                               vector_norm_kind=pdp.NormKind.L2)


NO_SAMPLING = (P_ROWS, 64)  # l0, linf no privacy id of _rank_data reaches (checked below)


def _runs(kind, pid, pk, v, vec, U, rank=None, owner=None):
    """The aggregations of one test, on the whole data (rank None) or on one
    rank's rows: {label: [(key, [metric values])]}."""
    mine = slice(None) if rank is None else owner == rank
    if kind == "percentile":
        table = _table(pid[mine], pk[mine], v[mine], U)
        return {"public": _aggregate(table, _percentile_params(), public=PUBLIC, seed=41),
                "private": _aggregate(table, _percentile_params(), seed=42)}
    out = {"verify": _aggregate(_table(pid[mine], pk[mine], vec[mine], U), _vector_params(3, 2), seed=43)}
    # "shuffle": the rows split by ROW index (privacy ids span ranks); with nothing
    # sampled away the kept rows do not depend on where a row sits
    half = len(pid) // 2
    rows = slice(None) if rank is None else (slice(0, half) if rank == 0 else slice(half, None))
    out["shuffle"] = _aggregate(_table(pid[rows], pk[rows], vec[rows], U), _vector_params(*NO_SAMPLING),
                                public=PUBLIC, seed=44, sharding="shuffle")
    return out


def _worker(rank, port, kind, results):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        pid, pk, v, vec, owner, U = _rank_data()
        results[rank] = _runs(kind, pid, pk, v, vec, U, rank, owner)
    except Exception as e:
        import traceback
        results[rank] = repr(e) + "\n" + traceback.format_exc()
    finally:
        dist.destroy_process_group()


def _two_ranks(kind):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    manager = ctx.Manager()
    results = manager.dict()
    mp.spawn(_worker, args=(_free_port(), kind, results), nprocs=2, join=True)
    res = dict(results)
    assert all(isinstance(res.get(r), dict) for r in (0, 1)), res
    return res


def _union(res, label):
    merged = {}
    for r in (0, 1):
        for k, m in res[r][label]:
            assert k not in merged, f"partition {k} came from both ranks"
            merged[k] = m
    return merged


def test_percentiles_on_two_ranks_equal_single_process(device):
    pid, pk, v, vec, owner, U = _rank_data()
    # sampling fires: some privacy id has more than 3 partitions and some pair more than 2 rows
    pairs, per_pair = np.unique(np.stack([pid, pk]), axis=1, return_counts=True)
    assert per_pair.max() > 2 and np.bincount(pairs[0]).max() > 3
    single = {label: dict(rows) for label, rows in _runs("percentile", pid, pk, v, vec, U).items()}
    res = _two_ranks("percentile")
    assert sorted(single["public"]) == PUBLIC
    assert len(single["private"]) >= 8
    for label in ("public", "private"):
        merged = _union(res, label)
        assert sorted(merged) == sorted(single[label])
        for k, want in single[label].items():
            got = merged[k]
            assert len(got) == 5
            print(label, k, got, want)
            # count, privacy_id_count, percentile_10, percentile_50, percentile_99_5: bit for bit
            assert got == want, (label, k)
    # the partition without rows walks on noise alone, inside the value range
    assert all(0.0 <= q <= 100.0 for q in single["public"][12][2:])


def test_vector_sums_on_two_ranks_equal_single_process(device):
    pid, pk, v, vec, owner, U = _rank_data()
    pairs, per_pair = np.unique(np.stack([pid, pk]), axis=1, return_counts=True)
    assert per_pair.max() <= NO_SAMPLING[1] and np.bincount(pairs[0]).max() <= NO_SAMPLING[0]
    single = {label: dict(rows) for label, rows in _runs("vector", pid, pk, v, vec, U).items()}
    res = _two_ranks("vector")
    for label in ("verify", "shuffle"):
        merged = _union(res, label)
        assert len(single[label]) >= 8
        assert sorted(merged) == sorted(single[label])
        for k, want in single[label].items():
            got = merged[k]
            print(label, k, got, want)
            assert len(got[-1]) == D  # vector_sum comes last in the MetricsTuple
            assert got == want, (label, k)
