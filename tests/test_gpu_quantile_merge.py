"""pdp_merge_quantile_leaves on the GPU (through
executor.merge_quantile_leaves): the merged arrays EQUAL np.sort of each
partition's concatenated runs and the offsets the NumPy cumulative sum --
nothing in the contract is approximate.  The inputs are those of
tests/quantile_merge_util.py, whose placement rule the CPU tests check."""
import ctypes

import numpy as np
import pytest

from pipelinedp_amd import _native as N
from pipelinedp_amd import executor as X
from tests import quantile_merge_util as M

pytestmark = pytest.mark.gpu

CASES = M.all_cases()


def _device_inputs(device, case):
    import torch
    runs, counts = M.flatten(case)
    return (torch.as_tensor(runs.view(np.int16), device=device),
            torch.as_tensor(counts.view(np.int32), device=device), len(runs))


def _host(leaves, offsets, n):
    return leaves.cpu().numpy().view(np.uint16)[:n], offsets.cpu().numpy().view(np.uint32).astype(np.int64)


@pytest.fixture(scope="module")
def wanted():
    """np.sort per partition, once for every test of the module."""
    return {name: M.merge_by_sort(case) for name, case in CASES}


@pytest.mark.parametrize("name,case", CASES, ids=[c[0] for c in CASES])
def test_merge_equals_sort_per_partition(device, wanted, name, case):
    runs, counts, n = _device_inputs(device, case)
    leaves, offsets = X.merge_quantile_leaves(runs, counts, n)
    assert leaves.dtype == runs.dtype and leaves.shape[0] == max(n, 1)
    got, got_off = _host(leaves, offsets, n)
    want, want_off = wanted[name]
    assert got_off.tolist() == want_off.tolist()
    assert got.tolist() == want.tolist()
    # a second call, into fresh buffers: the same bytes
    again, again_off = X.merge_quantile_leaves(runs, counts, n)
    assert _host(again, again_off, n)[0].tobytes() == got.tobytes()
    assert again_off.cpu().numpy().tobytes() == offsets.cpu().numpy().tobytes()


def test_merged_tree_feeds_quantile_metrics(device, wanted):
    """The output has reduce_quantile_leaves' layout: the exact (no noise)
    quantiles of the merged arrays are those of the sorted ones."""
    import torch
    name, case = next(c for c in CASES if c[0] == "uneven70-r3")
    runs, counts, n = _device_inputs(device, case)
    leaves, offsets = X.merge_quantile_leaves(runs, counts, n)
    want, want_off = wanted[name]
    P = len(want_off) - 1
    ref_leaves = torch.as_tensor(want.view(np.int16), device=device)
    ref_off = torch.as_tensor(want_off.astype(np.int32), device=device)
    index = torch.arange(P, dtype=torch.int64, device=device)
    kw = dict(min_value=0.0, max_value=1.0, ranks=[0.1, 0.5, 0.995], noise=None, seed=5)
    got = X.quantile_metrics(leaves, offsets, index, **kw).cpu().numpy()
    ref = X.quantile_metrics(ref_leaves, ref_off, index, **kw).cpu().numpy()
    assert got.tolist() == ref.tolist()


def test_reused_workspace_and_partial_prefix(device, wanted):
    """A caller's workspace of exactly the advertised size; `runs` longer than
    n_leaves (only the prefix is read)."""
    import torch
    name, case = next(c for c in CASES if c[0] == "long_run")
    runs, counts, n = _device_inputs(device, case)
    need = ctypes.c_uint64(0)
    N.check(N.lib().pdp_quantile_merge_workspace_bytes(2, 3, ctypes.byref(need)), "workspace_bytes")
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=device)
    padded = torch.cat([runs, torch.full((100,), -1, dtype=torch.int16, device=device)])
    for _ in range(2):
        leaves, offsets = X.merge_quantile_leaves(padded, counts, n, workspace=ws)
        got, got_off = _host(leaves, offsets, n)
        assert got.tolist() == wanted[name][0].tolist() and got_off.tolist() == wanted[name][1].tolist()


def test_refusals_launch_nothing(device):
    import torch
    runs, counts, n = _device_inputs(device, M.uneven_case(2, seed=1, n_partitions=6))
    with pytest.raises(N.NativeLibraryError, match=r"code -4.*n_runs"):
        X.merge_quantile_leaves(runs, counts[:0], 0)  # n_runs = 0
    many = torch.zeros((N.MAX_QUANTILE_RUNS + 1, 6), dtype=torch.int32, device=device)
    with pytest.raises(N.NativeLibraryError, match=r"code -4.*n_runs"):
        X.merge_quantile_leaves(runs, many, 0)  # n_runs = 65
    small = torch.empty(16, dtype=torch.uint8, device=device)
    with pytest.raises(N.NativeLibraryError, match=r"code -3.*workspace too small"):
        X.merge_quantile_leaves(runs, counts, n, workspace=small)
    with pytest.raises(TypeError):
        X.merge_quantile_leaves(runs, counts.to(torch.int64), n)
    with pytest.raises(TypeError):
        X.merge_quantile_leaves(runs.to(torch.int32), counts, n)
    with pytest.raises(ValueError):
        X.merge_quantile_leaves(runs, counts, n + 1)
    with pytest.raises(ValueError):
        X.merge_quantile_leaves(runs.cpu(), counts, n)
    # the largest supported number of runs passes the checks
    full = torch.ones((N.MAX_QUANTILE_RUNS, 1), dtype=torch.int32, device=device)
    codes = torch.arange(N.MAX_QUANTILE_RUNS, 0, -1, dtype=torch.int16, device=device)
    leaves, offsets = X.merge_quantile_leaves(codes, full, N.MAX_QUANTILE_RUNS)
    assert leaves.cpu().tolist() == list(range(1, N.MAX_QUANTILE_RUNS + 1))
    assert offsets.cpu().tolist() == [0, N.MAX_QUANTILE_RUNS]


def test_counts_that_disagree_with_n_leaves_stay_in_bounds(device):
    """Counts that sum to more than n_leaves: every store is bounded by
    n_leaves, so the guard words behind the output keep their value.  (The
    merged prefix is then unspecified; only the bound is pinned.)"""
    import torch
    case = M.uneven_case(3, seed=2, n_partitions=10)
    runs, counts, n = _device_inputs(device, case)
    short = n - 37
    need = ctypes.c_uint64(0)
    N.check(N.lib().pdp_quantile_merge_workspace_bytes(3, 10, ctypes.byref(need)), "workspace_bytes")
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=device)
    out = torch.full((short + 64,), 0x5A5A, dtype=torch.int16, device=device)
    offsets = torch.empty(11, dtype=torch.int32, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    N.check(N.lib().pdp_merge_quantile_leaves(runs.data_ptr(), short, counts.data_ptr(), 3, 10, ws.data_ptr(),
                                              ws.numel(), out.data_ptr(), offsets.data_ptr(), st),
            "pdp_merge_quantile_leaves")
    assert out[short:].cpu().tolist() == [0x5A5A] * 64
    assert offsets.cpu().numpy().view(np.uint32).tolist() == M.merged_offsets(M.flatten(case)[1]).tolist()
