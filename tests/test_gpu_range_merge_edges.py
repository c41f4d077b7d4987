"""The range merge (csrc/pdp_bound_merge.hip) on constructed tables, by equality (GPU).

The other GPU files reach k_range_plan, k_range_reduce, k_split_count,
k_split_scatter[_staged], k_fine_plan and k_fine_reduce with random keys, which
put the kernels' decision points wherever chance puts them.  The tables of
tests/range_merge_edges_util.py fix the record count of every (bucket, range)
cell (l0 = 4 >= the partitions of every id, linf = 0: nothing is sampled, one
record per distinct pair), so each shape sits on one edge:

  S1  one item per range at D - 1, D and D + 1 records (the direct / LDS switch
      at kRangeDirect), an empty range, the last range of 5 partitions with
      records on P - 5 and P - 1
  S2  range totals C, 2C, C + 1 and C - 1 (kRangeChunk): the sentinel written
      by the cut loop and by the explicit store, cuts on a bucket's last
      record, a one-record tail item
  S3  runs of 2,047: position C inside a bucket, an item above C, and a range
      whose last item is empty
  S4  3C records on one partition: the LDS counters of one slot take whole items
  S5  1,026 buckets with runs in 0, 511, 512, 1023, 1024 and the last only:
      k_range_plan's carry into its second batch of 1,024 buckets, an item over
      three batches of 512 buckets of k_range_reduce
  T1  two levels (P = 2,097,153, 8 fine ranges per coarse range, the staged
      scatter): fine ranges 0 and 7 only, and the last coarse range -- one fine
      range of one partition, P - 1 -- behind the n_fine_ranges guards
  T2  fine totals D - 1, D, C, C + 1, 2C: k_fine_plan's chunks, k_fine_reduce's switch
  T3  coarse items of 2,048 and 2,049 records (kSplitStageRows), in one fine
      range and over all eight
  U1, U2  T1 (fine ranges 0, 255, 256, 511) and T2 at P = 2^27 + 1: 512 fine
      ranges per coarse range, over kSplitStageFan, so the plain k_split_scatter runs

tests/test_range_merge_edges_host.py proves on the CPU, through a model of the
work-item rules, that each table is what this list says, and pins the plans.
Expected: NumPy bincount / add.at over the pair list and the rows (dyadic
values: exact in any order), compared with assert_array_equal -- torch.equal
on the device at P = 2^27 + 1, where an accumulator is 1 GiB.  No tolerance and
no skip anywhere in this file.
"""
import numpy as np
import pytest

from oracle import columnar as O
from tests import range_merge_edges_util as RU
from tests import value_edges_util as VU

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0000_0004
ROW_OFFSET = 77


@pytest.fixture(scope="module", autouse=True)
def _forget_tables():
    yield
    RU.drop_tables()


def _columns(device, t):
    import torch
    to = lambda a: None if a is None else torch.as_tensor(a).to(device)  # noqa: E731
    return to(t.pid), to(t.pk), to(t.val)


def _run(device, shape, variant, cols, ws):
    """One bound_and_reduce on the shape's pinned plan -> the device accumulators."""
    import torch
    from pipelinedp_amd import executor as X
    t, plan = RU.shape_table(shape, variant)
    RU.assert_plan(shape, t, plan)  # not the plan the table was laid out for: fail, do not skip
    U, P, _ = RU.SHAPES[shape]
    acc = X.bound_and_reduce(*cols, n_privacy_ids=U, n_partitions=P, bounding=RU.spec_for(variant), seed=SEED,
                             row_offset=ROW_OFFSET, workspace=ws, algorithm=2, merge=2)
    torch.cuda.synchronize()
    st = ws.stats()
    assert st["error_flags"] == 0 and st["sieve"] == 0, st
    assert st["rows_partitioned"] == len(t.pid), st
    return acc


@pytest.mark.parametrize("variant", sorted(RU.VARIANTS))
@pytest.mark.parametrize("shape", RU.SINGLE + RU.STAGED)
def test_range_merge_equals_the_table(device, shape, variant):
    from pipelinedp_amd import executor as X
    t, _ = RU.shape_table(shape, variant)
    want = t.expected()
    assert want["count"].sum() == len(t.pid) and want["privacy_id_count"].sum() == len(t.pair_pid)
    cols = _columns(device, t)
    ws = X.BoundWorkspace()
    runs = []
    for _ in range(2):  # the second on the first's workspace: exact sums, so equal despite the atomics
        acc = _run(device, shape, variant, cols, ws)
        runs.append({k: (None if v is None else v.cpu().numpy()) for k, v in acc.items()})
    got = runs[0]
    VU.assert_exactly_equal(got, want)
    VU.assert_exactly_equal(runs[1], got)
    if variant == "none":
        assert all(got[k] is None for k in VU.FIELDS)
    else:
        assert all(got[k] is not None for k in VU.FIELDS)
        assert got["sum"].dtype == (np.int64 if t.flags & O.SUM_INT else np.float64)
    # partitions outside the populated cells are exactly zero
    empty = np.ones(t.geom.P, dtype=bool)
    empty[t.pair_pk] = False
    assert empty.sum() == t.geom.P - len(np.unique(t.pair_pk))
    for k, v in got.items():
        assert v is None or not v[empty].any(), k


def _device_expected(device, t):
    """Table.expected() with torch on the device, from the same pair list and row terms."""
    import torch
    P = t.geom.P
    pk = torch.as_tensor(t.pk).to(device)
    want = {"privacy_id_count": torch.bincount(torch.as_tensor(t.pair_pk).to(device), minlength=P),
            "count": torch.bincount(pk, minlength=P)}
    for k, term in t.row_terms().items():
        if term is not None:
            want[k] = torch.zeros(P, dtype=torch.float64, device=device)
            want[k].index_add_(0, pk, torch.as_tensor(term).to(device))
    return want


@pytest.mark.parametrize("variant", ["f64", "none"])
@pytest.mark.parametrize("shape", RU.UNSTAGED)
def test_unstaged_scatter_equals_the_table(device, shape, variant):
    """P = 2^27 + 1: every P-sized array stays on the device; only a mismatch report comes back."""
    import torch
    from pipelinedp_amd import executor as X
    t, _ = RU.shape_table(shape, variant)
    assert t.geom.fine_per_coarse == 512 > RU.STAGE_FAN
    got = _run(device, shape, variant, _columns(device, t), X.BoundWorkspace())
    want = _device_expected(device, t)
    assert int(want["count"].sum()) == len(t.pid) and int(want["privacy_id_count"].sum()) == len(t.pair_pid)
    assert set(want) == {k for k, v in got.items() if v is not None}
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and g.shape == w.shape, k
        if not torch.equal(g, w):
            at = torch.nonzero(g != w).flatten()
            head = at[:8]
            pytest.fail(f"{k}: {at.numel()} partitions differ, first {head.tolist()}: got {g[head].tolist()}, "
                        f"want {w[head].tolist()}")
    # partitions outside the populated cells are exactly zero
    assert int(torch.count_nonzero(got["privacy_id_count"])) == len(np.unique(t.pair_pk))
    # (the one partition of the last fine range: U1 holds records there)
    assert int(got["privacy_id_count"][t.geom.P - 1]) == int((t.pair_pk == t.geom.P - 1).sum())
    del got, want
    torch.cuda.empty_cache()  # 10 GiB back to the driver
