"""The merge of the ranks' quantile trees, on the CPU: the NumPy statement of
pdp_merge_quantile_leaves' placement rule (tests/quantile_merge_util.py) is a
permutation and sorts; the entry points refuse bad shapes before any device
work; parallel.exchange_quantile_leaves / exchange_vector_accumulator are
identities on one rank and deliver hand-cut slices on two (gloo)."""
import ctypes
import os
import socket

import numpy as np
import pytest

from pipelinedp_amd import _native as N
from pipelinedp_amd import parallel
from tests import quantile_merge_util as M

CASES = M.all_cases()


# ------------------------------------------------------- two ranks, gloo --
WORLD, P_PAD, D = 2, 8, 3  # rank r owns partitions [4 r, 4 r + 4)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_tree(rank):
    """(leaves uint16, offsets) of one rank's 8 partitions.  Rank 1 holds
    nothing in rank 0's partitions: it sends rank 0 zero leaves."""
    rng = np.random.default_rng(50 + rank)
    sizes = [3, 0, 7, 2, 0, 5, 1, 4] if rank == 0 else [0, 0, 0, 0, 6, 0, 2, 9]
    segs = [np.sort(rng.integers(0, 65536, n).astype(np.uint16)) for n in sizes]
    return np.concatenate(segs).astype(np.uint16), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _rank_vectors(rank):
    return np.random.default_rng(60 + rank).integers(-50, 50, (P_PAD, D)).astype(np.float64)


def _gloo_worker(rank, port, results):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        S = P_PAD // WORLD
        trees = [_rank_tree(r) for r in range(WORLD)]
        leaves, off = trees[rank]
        runs, counts, n = parallel.exchange_quantile_leaves(torch.as_tensor(leaves.view(np.int16)),
                                                            torch.as_tensor(off.astype(np.int32)))
        # by hand: source s's span and counts of this rank's partitions, in source order
        want_runs = np.concatenate([lv[o[rank * S]:o[(rank + 1) * S]] for lv, o in trees])
        want_counts = np.stack([np.diff(o)[rank * S:(rank + 1) * S] for _, o in trees])
        assert runs.dtype == torch.int16 and counts.dtype == torch.int32 and counts.shape == (WORLD, S)
        assert n == len(want_runs) == int(runs.shape[0])
        assert runs.numpy().view(np.uint16).tolist() == want_runs.tolist()
        assert counts.numpy().tolist() == want_counts.tolist()
        if rank == 0:
            assert want_counts[1].sum() == 0  # the empty span arrived as an empty span
        # the received runs merge into the two ranks' trees of the slice
        got, got_off = M.merge_by_positions(runs.numpy().view(np.uint16), counts.numpy().astype(np.uint32))
        case = [[lv[o[p]:o[p + 1]] for p in range(rank * S, (rank + 1) * S)] for lv, o in trees]
        want, want_off = M.merge_by_sort(case)
        assert got.tolist() == want.tolist() and got_off.tolist() == want_off.tolist()

        vecs = [_rank_vectors(r) for r in range(WORLD)]
        mine = torch.as_tensor(vecs[rank])
        part, first = parallel.exchange_vector_accumulator(mine)
        assert first == rank * S and part.shape == (S, D)
        assert part.numpy().tolist() == (vecs[0] + vecs[1])[first:first + S].tolist()
        assert mine.numpy().tolist() == vecs[rank].tolist()  # the caller's accumulator is not overwritten

        # "shuffle" carries a 2-D column: whole rows move with their privacy id
        ident = torch.arange(40, dtype=torch.int64) * 2 + rank
        rows = torch.stack([ident.to(torch.float64), -ident.to(torch.float64), ident.to(torch.float64) * 0.5], dim=1)
        pk = ident % 5
        got_id, (got_pk, got_rows, none) = parallel.shuffle_by_privacy_id(ident, [pk, rows, None])
        assert none is None and got_rows.shape == (got_id.numel(), 3)
        assert bool((parallel.owner_of(got_id, WORLD) == rank).all())
        assert got_rows[:, 0].tolist() == got_id.to(torch.float64).tolist()
        assert got_rows[:, 1].tolist() == (-got_id.to(torch.float64)).tolist()
        assert got_pk.tolist() == (got_id % 5).tolist()
        results[rank] = ("ok", int(got_id.numel()))
    except Exception as e:  # reported to the parent
        import traceback
        results[rank] = repr(e) + traceback.format_exc()
    finally:
        dist.destroy_process_group()


def test_two_ranks_receive_hand_cut_slices():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")  # no fork of the test process; the manager ends with the test
    with ctx.Manager() as manager:
        results = manager.dict()
        mp.spawn(_gloo_worker, args=(_free_port(), results), nprocs=WORLD, join=True)
        res = dict(results)
    assert [res[r][0] for r in range(WORLD)] == ["ok", "ok"], res
    assert res[0][1] + res[1][1] == 80  # every shuffled row arrived on one rank


# ------------------------------------------------------ the placement rule --
@pytest.mark.parametrize("name,case", CASES, ids=[c[0] for c in CASES])
def test_positions_are_a_permutation_and_sort(name, case):
    runs, counts = M.flatten(case)
    pos = M.merge_positions(runs, counts)
    assert sorted(pos.tolist()) == list(range(len(runs)))
    leaves, off = M.merge_by_positions(runs, counts)
    want, want_off = M.merge_by_sort(case)
    assert off.tolist() == want_off.tolist()
    assert leaves.tolist() == want.tolist()
    # every element stays inside its partition's slots
    n_runs, P = counts.shape
    part = np.concatenate([np.repeat(np.arange(P), counts[s]) for s in range(n_runs)]) if len(runs) else pos
    assert np.all((off[part] <= pos) & (pos < off[part + 1])) if len(runs) else True


def test_ties_go_by_run_then_index():
    runs, counts = M.flatten(M.ties_case())
    pos = M.merge_positions(runs, counts)
    # partition 0: run s's 17 equal codes take the slots 17 s .. 17 s + 16, in order
    run_off = np.concatenate([[0], np.cumsum(counts.ravel().astype(np.int64))])
    for s in range(3):
        at = pos[run_off[s * 2]:run_off[s * 2] + 17]
        assert at.tolist() == list(range(17 * s, 17 * s + 17))


# ------------------------------------------------- argument checks (host) --
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return N.lib()


_DUMMY = ctypes.create_string_buffer(4096 + 16)
_HOST = (ctypes.addressof(_DUMMY) + 15) & ~15  # never dereferenced: every call below is refused first


def test_merge_entry_points_refuse_before_device_work(lib):
    need = ctypes.c_uint64(0)
    for n_runs in (0, -1, N.MAX_QUANTILE_RUNS + 1):
        assert lib.pdp_quantile_merge_workspace_bytes(n_runs, 10, ctypes.byref(need)) == -4
        assert b"n_runs" in lib.pdp_last_error()
        assert lib.pdp_merge_quantile_leaves(_HOST, 4, _HOST, n_runs, 10, _HOST, 1 << 20, _HOST + 2048, _HOST, None) == -4
    assert lib.pdp_quantile_merge_workspace_bytes(2, 0, ctypes.byref(need)) == -1
    assert lib.pdp_quantile_merge_workspace_bytes(2, 10, None) == -1
    assert lib.pdp_quantile_merge_workspace_bytes(N.MAX_QUANTILE_RUNS, 1 << 26, ctypes.byref(need)) == -4
    assert lib.pdp_quantile_merge_workspace_bytes(N.MAX_QUANTILE_RUNS, 10, ctypes.byref(need)) == 0
    assert lib.pdp_quantile_merge_workspace_bytes(3, 70, ctypes.byref(need)) == 0
    assert need.value >= (3 * 70 + 1) * 4
    call = lib.pdp_merge_quantile_leaves
    assert call(_HOST, 4, _HOST, 3, 70, _HOST, need.value - 1, _HOST + 2048, _HOST, None) == -3
    assert b"workspace too small" in lib.pdp_last_error()
    assert call(_HOST, 4, _HOST, 3, 70, None, need.value, _HOST + 2048, _HOST, None) == -3
    assert call(_HOST, -1, _HOST, 3, 70, _HOST, need.value, _HOST + 2048, _HOST, None) == -1
    assert call(_HOST, 1 << 31, _HOST, 3, 70, _HOST, need.value, _HOST + 2048, _HOST, None) == -4
    assert call(_HOST, 4, None, 3, 70, _HOST, need.value, _HOST + 2048, _HOST, None) == -1
    assert call(None, 4, _HOST, 3, 70, _HOST, need.value, _HOST + 2048, _HOST, None) == -1
    assert call(_HOST, 4, _HOST, 3, 70, _HOST, need.value, _HOST, _HOST, None) == -1  # runs == leaves
    assert b"alias" in lib.pdp_last_error()
    assert call(_HOST + 1, 4, _HOST, 3, 70, _HOST, need.value, _HOST + 2048, _HOST, None) == -1
    assert b"aligned" in lib.pdp_last_error()


# ------------------------------------------------------------- one rank --
def test_exchanges_are_identities_on_one_rank(monkeypatch):
    import torch
    import torch.distributed as dist

    def boom(*a, **k):
        raise AssertionError("a collective ran on one rank")
    for name in ("all_to_all_single", "all_reduce", "all_gather", "reduce_scatter_tensor", "broadcast"):
        monkeypatch.setattr(dist, name, boom)
    runs, counts = M.flatten(M.uneven_case(1, seed=3, n_partitions=11))
    off = M.merged_offsets(counts)
    leaves = torch.as_tensor(runs.view(np.int16))
    offsets = torch.as_tensor(off.astype(np.int32))
    got_runs, got_counts, n = parallel.exchange_quantile_leaves(leaves, offsets)
    assert got_runs is leaves and n == len(runs)
    assert got_counts.dtype == torch.int32 and got_counts.shape == (1, 11)
    assert got_counts.numpy().tolist() == counts.astype(np.int64).tolist()
    vacc = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    part, first = parallel.exchange_vector_accumulator(vacc)
    assert part is vacc and first == 0
