"""The dataset histograms (csrc/pdp_hist.hip) on the edge tables of
tests/hist_edges_util.py: every pairs phase (privacy-id buckets, pair
buckets, the HBM pair table) and the pre-aggregated path against the oracle
(oracle/histograms.py, which tests/test_histogram_edges_host.py pins on the
same tables against the reference's recorded bins and a plain restatement).

Every comparison is an equality -- bounds, counts, sums and maxima: the
tables' pair, partition and bin sums are exact in any order
(hist_edges_util.check_exact).  The raw lowers are compared with np.linspace
bit for bit."""
import functools

import numpy as np
import pytest

from oracle import histograms as OH
from pipelinedp_amd import executor as X
from pipelinedp_amd.dataset_histograms import computing_histograms as CH
from tests import hist_edges_util as E
from tests import hist_util as HU

pytestmark = pytest.mark.gpu

MODES = ("auto", "pair_hash", "pair_table")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _raw(table, mode="auto", workspace=None):
    import torch
    pid, pk, val, U, P = table
    d = _dev()
    return X.dataset_histograms(torch.as_tensor(pid, device=d), torch.as_tensor(pk, device=d),
                                torch.as_tensor(val, device=d), n_privacy_ids=U, n_partitions=P,
                                force_pair_table=mode == "pair_table", force_pair_hash=mode == "pair_hash",
                                workspace=workspace)


def _raw_pre(table, workspace=None):
    import torch
    pid, pk, val, U, P = table
    d = _dev()
    cols = [torch.as_tensor(np.ascontiguousarray(c), device=d) for c in HU.preaggregate(pid, pk, val)]
    return X.dataset_histograms_preaggregated(*cols, n_partitions=P, workspace=workspace)


def _bins(raw):
    h = CH.histograms_from_device(raw)
    return {f: HU.as_tuples(getattr(h, f).bins) for f in OH.HIST_FIELDS}


def _assert_equal(got, want, what):
    for f in OH.HIST_FIELDS:
        HU.assert_bins_equal(got[f], want[f], f"{what}/{f}", exact=True)


def _assert_lowers(raw, table, what):
    """float_lowers / float_n_lowers against np.linspace over the exact pair
    and partition sums, as bit patterns ([mn, mn] when min == max, where +0.0
    and -0.0 count as equal: which of the two a minimum is depends on the
    order)"""
    pid, pk, val, _, P = table
    pair = np.unique(pid * P + pk, return_inverse=True)[1].reshape(-1)
    part = np.unique(pk, return_inverse=True)[1].reshape(-1)
    lowers = raw["float_lowers"].cpu().numpy()
    n_lowers = raw["float_n_lowers"].cpu().numpy()
    for f, inv in enumerate((pair, part)):
        sums = np.bincount(inv, weights=val)
        mn, mx = sums.min(), sums.max()
        if mn == mx:
            assert n_lowers[f] == 2 and (lowers[f, :2] == mn).all(), what
        else:
            assert n_lowers[f] == E.N_LOWERS, what
            want = np.linspace(mn, mx, E.N_LOWERS)
            diff = np.flatnonzero(lowers[f].view(np.int64) != want.view(np.int64))
            assert diff.size == 0, f"{what}: histogram {f}, lowers {diff[:5].tolist()} differ"


@functools.lru_cache(maxsize=None)
def _table(name):
    """(table, the oracle's bins), built once and shared"""
    kind, _, arg = name.partition("/")
    if kind == "float":
        rng, part = arg.rsplit(".", 1)
        t = E.float_edges(rng)[int(part)]
    elif kind == "n":
        t = E.structure(int(arg))
    elif kind == "P":
        t = E.structure(E.STRUCTURE_P_ROWS, int(arg))
    else:
        t = {"constant": E.float_constant, "signed_zeros": E.float_signed_zeros, "two_pairs": E.float_edges_two_pairs,
             "log_counts": E.log_counts, "distinct_small": lambda: E.log_distinct(E.LOG_DISTINCT_SMALL),
             "distinct_3628": lambda: E.log_distinct((3628,)), "distinct_3629": lambda: E.log_distinct((3629,)),
             "wave_partition": lambda: E.log_wave_bins("partition"),
             "wave_privacy_id": lambda: E.log_wave_bins("privacy_id")}[name]()
    return t, OH.dataset_histograms(*t[:3])


EDGE_TABLES = [f"float/{r}.{j}" for r in E.FLOAT_RANGES for j in range(len(E.float_edge_parts(r)))]
EDGE_TABLES += ["constant", "signed_zeros", "two_pairs", "log_counts", "distinct_small", "distinct_3628",
                "distinct_3629", "wave_partition", "wave_privacy_id"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", EDGE_TABLES)
def test_edge_tables_raw(name, mode):
    """float bins on, one ulp below and one ulp above a lower, repeated
    lowers, min == max, the subnormal form; logarithmic bins at the decades;
    through each pairs phase (distinct_3629 overflows a privacy-id bucket's
    LDS table: `auto` starts again with pair buckets)"""
    table, want = _table(name)
    raw = _raw(table, mode)
    _assert_lowers(raw, table, f"{name}/{mode}")
    _assert_equal(_bins(raw), want, f"{name}/{mode}")


@pytest.mark.parametrize("name", EDGE_TABLES)
def test_edge_tables_preaggregated(name):
    """the same bins from preaggregate()'s rows (k_hp_*); the L0 / L1 weights
    are k x (1 / k) per privacy id, and no weight sum lies near x.5"""
    table, want = _table(name)
    assert E.weight_sums_clear_of_half(HU.preaggregate(*table[:3])), name
    raw = _raw_pre(table)
    _assert_lowers(raw, table, f"pre/{name}")
    _assert_equal(_bins(raw), want, f"pre/{name}")


def test_wave_tables_known_bins():
    """int_hist_add_wave's count, sum and max of the two wide bins, as numbers"""
    for name, fields in (("wave_partition", ("count_per_partition_histogram", "count_privacy_id_per_partition")),
                         ("wave_privacy_id", ("l1_contributions_histogram", "l0_contributions_histogram"))):
        got = _bins(_raw(_table(name)[0]))
        for f in fields:
            assert got[f] == E.WAVE_BINS, (name, f)


def _structure_modes(n):
    return MODES if n <= 393217 else ("auto", "pair_table")


@pytest.mark.parametrize("n,mode", [(n, m) for n in E.STRUCTURE_N for m in _structure_modes(n)])
def test_row_count_boundaries(n, mode):
    """one wave, one bucket (1,536 rows), one level-1 stage / level-2 window
    (8,192), one tile (65,536), 64 buckets (k_hb_prange's wave), one
    super-bucket (256 buckets), 1,024 range workgroups: the size on each side"""
    table, want = _table(f"n/{n}")
    raw = _raw(table, mode)
    _assert_lowers(raw, table, f"n{n}/{mode}")
    _assert_equal(_bins(raw), want, f"n{n}/{mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", E.STRUCTURE_P)
def test_partition_count_boundaries(P, mode):
    """one partition range (2,048 partitions), one pair-table region (4,096),
    128 ranges (above: per-pair partition atomics): the size on each side"""
    table, want = _table(f"P/{P}")
    raw = _raw(table, mode)
    _assert_lowers(raw, table, f"P{P}/{mode}")
    _assert_equal(_bins(raw), want, f"P{P}/{mode}")


def _all_equal(a, b, what):
    import torch
    for k in a:
        if k != "workspace":
            assert torch.equal(a[k], b[k]), f"{what}: {k} differs between a used and a fresh workspace"


def test_reused_workspace_carries_no_state():
    """one workspace through a large call, a small one, a call whose
    privacy-id bucket overflows (it re-zeroes a list of buffers and starts
    again), the small one again, a call on per-pair partition atomics and one
    on partition ranges: every raw output equals the same call's on a fresh
    workspace, and the bins the oracle's"""
    ws = X.BoundWorkspace()
    for name in ("n/393217", "n/1537", "distinct_3629", "n/1537", "P/262145", "P/2049"):
        table, want = _table(name)
        used, fresh = _raw(table, workspace=ws), _raw(table)
        assert used["workspace"].data_ptr() == ws.buf.data_ptr()
        _all_equal(used, fresh, name)
        _assert_equal(_bins(used), want, f"reused/{name}")


def test_preaggregated_after_raw_on_one_workspace():
    ws = X.BoundWorkspace()
    big, _ = _table("n/65537")
    _raw(big, workspace=ws)
    for name in ("float/third.0", "distinct_small"):
        table, want = _table(name)
        used, fresh = _raw_pre(table, workspace=ws), _raw_pre(table)
        assert used["workspace"].data_ptr() == ws.buf.data_ptr()
        _all_equal(used, fresh, f"pre/{name}")
        _assert_equal(_bins(used), want, f"pre-reused/{name}")
        _raw(big, workspace=ws)
