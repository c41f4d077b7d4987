"""PERCENTILE on the GPU where tests/test_gpu_percentile.py does not look: the
noised walk and its Philox stream index, `index` / `n_kept_dev` /
`partition_offset` of pdp_quantile_metrics, partition sorts of one, two and
three passes, rows sampled away by l0 and linf, and the int64 column's edges.

Every comparison is an equality with tests/percentile_edges_util.py, which
tests/test_percentile_edges_host.py proves on the CPU: the walk performs the
restatement's fp64 operations in its order (no contraction in the device code)
and the secure samplers are restated bit for bit (oracle.columnar
.secure_add_noise; its caveat holds: a last-ulp difference of expm1 can flip
one Bernoulli with probability about 1e-16 per draw, and the seeds are fixed).
"""
import functools

import numpy as np
import pytest

from pipelinedp_amd import _native as N
from pipelinedp_amd import executor as X
from tests import percentile_edges_util as PU
from tests import quantile_tree_util as Q

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _walk(device, trees, index, *, ranks=PU.RANKS7, kind=None, partition_offset=0, n_kept=None, n_kept_dev=None,
          lo=0.0, hi=1.0):
    """pdp_quantile_metrics on host-built trees; returns the WHOLE output
    buffer [len(index), len(ranks)], prefilled with SENTINEL, of which the call
    is given the first n_kept rows."""
    import torch
    leaves, off = PU.pack_trees(trees)
    t = functools.partial(torch.as_tensor, device=device)
    idx = t(np.asarray(index, dtype=np.int64))
    buf = torch.full((len(index), len(ranks)), SENTINEL, dtype=torch.float64, device=device)
    n_kept = len(index) if n_kept is None else n_kept
    dev = None if n_kept_dev is None else t(np.array([n_kept_dev], dtype=np.int64))
    X.quantile_metrics(t(leaves), t(off), idx, min_value=lo, max_value=hi, ranks=ranks,
                       noise=None if kind is None else PU.noise(kind), seed=PU.NOISE_SEED, n_kept=n_kept,
                       n_kept_dev=dev, partition_offset=partition_offset, out=buf[:n_kept])
    return buf.cpu().numpy()


# ------------------------------------------- A. noised walk, built trees --
@pytest.mark.parametrize("kind", ["laplace", "gaussian"])
def test_noised_walk_equals_restatement(device, kind):
    """Eight trees of 0 ... 2,000 values, seven ranks (two rounds, the second
    partial).  The restatement met clamped counts, subtrees that exist only by
    noise and picked children without a count (asserted on the host)."""
    want, counters = PU.walk_expected(kind)
    assert all(v > 0 for v in counters.values()), counters
    got = _walk(device, PU.walk_trees(), range(8), kind=kind)
    assert got.tolist() == want.tolist()
    plain = _walk(device, PU.walk_trees(), range(8))
    assert plain.tolist() == PU.walk_expected(None)[0].tolist()
    assert all((got[p] != plain[p]).any() for p in range(1, 8))


def test_noised_walk_sixteen_rounds(device):
    """64 ranks on the trees of 0, 1 and 2 values: every round reads the first
    round's noisy tree."""
    want, counters = PU.walk_expected("laplace", 0, tuple(PU.RANKS64), (0, 1, 2))
    assert all(v > 0 for v in counters.values()), counters
    got = _walk(device, PU.walk_trees(), [0, 1, 2], ranks=PU.RANKS64, kind="laplace")
    assert got.tolist() == want.tolist()


# --------------------------------------------------------- B. stream index --
@pytest.mark.parametrize("offset", PU.OFFSETS)
def test_partition_offset_enters_the_stream_index(device, offset):
    """At 61,440 the stream indices of one launch straddle 2^32.  Partition 8
    holds partition 6's leaves."""
    trees = PU.walk_trees(duplicate=True)
    want, _ = PU.walk_expected("laplace", offset, duplicate=True)
    got = _walk(device, trees, range(9), kind="laplace", partition_offset=offset)
    assert got.tolist() == want.tolist()
    base = _walk(device, trees, range(9), kind="laplace")
    assert base.tolist() == PU.walk_expected("laplace", 0, duplicate=True)[0].tolist()
    assert all((got[p] != base[p]).any() for p in range(9))
    assert (got[6] != got[8]).any() and (base[6] != base[8]).any()


# ---------------------------------------------- C. index and n_kept_dev --
@pytest.mark.parametrize("kind", [None, "laplace"])
def test_index_and_n_kept_dev(device, kind):
    trees = PU.walk_trees()
    want, _ = PU.walk_expected(kind, 0, partitions=tuple(PU.INDEX7))
    valid = [i for i, p in enumerate(PU.INDEX7) if 0 <= p < 8]
    assert [i for i in range(7) if i not in valid] == [3, 4]

    def check(got, rows_written):
        for i in range(7):
            if i in valid and i < rows_written:
                assert got[i].tolist() == want[i].tolist(), i
            else:
                assert got[i].tolist() == [SENTINEL] * len(PU.RANKS7), i

    full = _walk(device, trees, PU.INDEX7, kind=kind)
    check(full, 7)
    assert full[1].tolist() == full[2].tolist()
    check(_walk(device, trees, PU.INDEX7, kind=kind, n_kept_dev=4), 4)
    check(_walk(device, trees, PU.INDEX7, kind=kind, n_kept_dev=100), 7)
    check(_walk(device, trees, PU.INDEX7, kind=kind, n_kept_dev=0), 0)
    check(_walk(device, trees, PU.INDEX7, kind=kind, n_kept=4, n_kept_dev=100), 4)
    check(_walk(device, trees, PU.INDEX7, kind=kind, n_kept=0), 0)


# ------------------------------------------------- D. wide partition sorts --
def _reduce(device, pid, pk, values, *, P, U, lo, hi, l0=PU.BIG, linf=PU.BIG, seed=7, row_offset=0, allowed=None):
    """(acc, leaves uint16 [off[-1]], offsets) of reduce_quantile_leaves, and the device tensors for a walk."""
    import torch
    t = functools.partial(torch.as_tensor, device=device)
    spec = X.BoundingSpec(l0=l0, linf=linf, value_kind=N.VALUE_NONE, flags=0)
    acc, leaves, offsets = X.reduce_quantile_leaves(
        t(pid), t(pk), t(values), n_privacy_ids=U, n_partitions=P, bounding=spec, min_value=lo, max_value=hi,
        seed=seed, row_offset=row_offset, allowed=None if allowed is None else t(np.asarray(allowed, np.uint8)))
    off = offsets.cpu().numpy().view(np.uint32)
    acc = {k: v.cpu().numpy() for k, v in acc.items() if v is not None}
    return acc, leaves.cpu().numpy().view(np.uint16)[:off[-1]], off, (leaves, offsets)


def _walk_leaves(device, dev, index, lo, hi, ranks=PU.RANKS7):
    import torch
    idx = torch.as_tensor(np.asarray(index, dtype=np.int64), device=device)
    return X.quantile_metrics(dev[0], dev[1], idx, min_value=lo, max_value=hi, ranks=ranks, noise=None,
                              seed=1).cpu().numpy()


def _check_sort(device, P, n):
    pid, pk, values = PU.sort_table(P, n)
    lo, hi = PU.SORT_LO, PU.SORT_HI
    acc, leaves, off, dev = _reduce(device, pid, pk, values, P=P, U=n, lo=lo, hi=hi)
    want_leaves, want_off = PU.leaves_of_rows(values, pk, np.arange(n), P, lo, hi)
    assert np.array_equal(off, want_off)
    assert np.array_equal(leaves, want_leaves)
    assert np.array_equal(acc["count"], np.bincount(pk, minlength=P))  # NaN rows are counted rows
    index = PU.sort_walk_index(P, pk, values)
    trees = PU.trees_of_rows(values, pk, np.arange(n), index.tolist(), lo, hi)
    want = np.array([trees[p].quantiles(PU.RANKS7) for p in index.tolist()])
    assert _walk_leaves(device, dev, index, lo, hi).tolist() == want.tolist()


@pytest.mark.parametrize("P", PU.SORT_P)
def test_partition_sort_passes(device, P):
    """P = 255 / 256: the not-kept key P moves from 8 to 9 bits (one pass to
    two); 65,535 / 65,536: two passes to three.  6,000 rows are three tiles,
    2,500 of them in one partition."""
    _check_sort(device, P, 6000)


@pytest.mark.parametrize("n", PU.TILE_EDGE_N)
def test_partition_sort_tile_edge(device, n):
    _check_sort(device, PU.TILE_EDGE_P, n)


# ----------------------------------------------------------- E. sampled rows --
@pytest.mark.parametrize("case", sorted(PU.SAMPLED_CASES))
def test_sampled_rows_build_the_trees(device, case):
    """The leaves' reader of the pair table keeps the rows the restatement
    keeps (every row has a leaf of its own), disallowed partitions take no l0
    slot, row_offset enters, and a NaN row is dropped after sampling: it is in
    COUNT and not in the tree."""
    pid, pk, values, allowed = PU.sampled_table()
    l0, linf, row_offset, masked = PU.SAMPLED_CASES[case]
    U, P = PU.SAMPLED["U"], PU.SAMPLED["P"]
    kept = PU.sampled_kept(case)
    acc, leaves, off, dev = _reduce(device, pid, pk, values, P=P, U=U, lo=0.0, hi=1.0, l0=l0, linf=linf,
                                    seed=PU.SAMPLED_SEED, row_offset=row_offset, allowed=allowed if masked else None)
    want_leaves, want_off = PU.leaves_of_rows(values, pk, kept, P, 0.0, 1.0)
    assert np.array_equal(off, want_off)
    assert np.array_equal(leaves, want_leaves)
    assert np.array_equal(acc["count"], np.bincount(pk[kept], minlength=P))
    pairs = np.unique(np.stack([pid[kept], pk[kept]], axis=1), axis=0)
    assert np.array_equal(acc["privacy_id_count"], np.bincount(pairs[:, 1], minlength=P))
    assert int(acc["count"].sum()) > int(off[-1])  # kept NaN rows
    trees = PU.trees_of_rows(values, pk, kept, range(P), 0.0, 1.0)
    want = np.array([trees[p].quantiles(PU.RANKS7) for p in range(P)])
    assert _walk_leaves(device, dev, np.arange(P), 0.0, 1.0).tolist() == want.tolist()


# --------------------------------------------------- F. integer column edges --
@pytest.mark.parametrize("lo,hi", PU.INT_RANGES)
def test_integer_column_edges(device, lo, hi):
    """INT64_MIN / MAX, +-(2^53 + 1), the range's ends and their outer
    neighbours: the device's int64 -> fp64 conversion rounds as astype does."""
    pid, pk, values = PU.int_table(lo, hi)
    n = len(values)
    acc, leaves, off, dev = _reduce(device, pid, pk, values, P=2, U=n, lo=lo, hi=hi)
    want_leaves, want_off = PU.leaves_of_rows(values, pk, np.arange(n), 2, lo, hi)
    assert np.array_equal(off, want_off) and off[-1] == n
    assert np.array_equal(leaves, want_leaves)
    want = np.array([Q.Tree(lo, hi, values[pk == p].astype(np.float64)).quantiles(PU.RANKS7) for p in (0, 1)])
    assert _walk_leaves(device, dev, [0, 1], lo, hi).tolist() == want.tolist()
