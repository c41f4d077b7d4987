"""GPU parity of the sieve's per-id fix-up (pdp_bound.hip, Plan.fix_ids).

Where a wave's sketches fit its LDS slice (l0 * (1 + linf) <= 32, linf > 0)
the unresolved privacy ids are finished by k_fix_id_count -> k_fix_id_alloc ->
k_fix_id_scatter -> k_fix_ids (one wave per id; ids over the 4,096-row cap by a listed bucket
launch), and their kept pairs reach the partitions through the reduce
kernels' flat list.  Kept pairs and rows must equal the oracle's (no sieve:
oracle/columnar.py) and the unsieved GPU path's: counts and privacy-id counts
exactly, fp64 sums to test_gpu_sieve.py's tolerance.

Shapes: 8,192 privacy ids in 128 buckets of 64 (the PIPELINEDP_AMD_BUCKET_BITS
test hook: more than 64 buckets is the sieve's precondition), ~2e5 rows (four
tiles, a ragged last one).  Every case first derives from the pair hashes
alone which ids have fewer than l0 distinct pairs below t and below 2t, and
the run's statistics must report exactly those counts, so no case can pass
without entering the path it is about.
"""
import numpy as np
import pytest

from oracle import columnar as O
from tests.test_gpu_kernels import _abs_scale, _compare
from tests.test_gpu_sieve import _run, _want

pytestmark = pytest.mark.gpu

U, P = 8192, 3001
ROW_CAP = 4096  # kFixIdsRowCap


@pytest.fixture(autouse=True)
def _small_buckets(monkeypatch):
    monkeypatch.setenv("PIPELINEDP_AMD_TEST_HOOKS", "1")
    monkeypatch.setenv("PIPELINEDP_AMD_BUCKET_BITS", "6")


def _spec(l0, linf, vk=O.VALUE_F64, flags=O.ACC_SUM | O.ACC_NSUM, lo=0.0, hi=10.0):
    from pipelinedp_amd import executor as X
    mid = lo + (hi - lo) / 2 if vk != O.VALUE_NONE else 0.0
    return X.BoundingSpec(l0=l0, linf=linf, value_kind=vk, flags=flags, min_value=lo, max_value=hi, middle=mid,
                          min_sum=0.0, max_sum=0.0)


def _values(rng, n, vk):
    if vk == O.VALUE_NONE:
        return None
    if vk == O.VALUE_I64:
        return rng.integers(-3, 12, n)
    return rng.random(n) * 12.0 - 1.0


def _base(seed, n=200_000 + 321, vk=O.VALUE_F64):
    rng = np.random.default_rng(seed)
    return rng.integers(0, U, n), rng.integers(0, P, n), _values(rng, n, vk)


def _short_ids(pid, pk, seed, l0, sieve):
    """(ids with < l0 distinct pairs below t, those with < l0 below 2t) from
    the pair hashes alone; ids without rows count (they are unresolved too)."""
    h = O.pair_hash(seed, pid, pk).astype(np.uint64)
    pairs = np.unique(np.stack([pid, pk, h.astype(np.int64)]), axis=1)
    out = []
    for t in (sieve, min(2 * sieve, 32768)):
        below = pairs[2] < (t << 16)
        out.append(np.flatnonzero(np.bincount(pairs[0][below], minlength=U) < l0))
    return out


def _check(device, pid, pk, val, spec, seed, sieve, row_offset=0, want_fix_ids=1):
    from pipelinedp_amd import executor as X
    plan = X.bound_plan(len(pid), U, P, spec, sieve=sieve)
    # (the band is planned up to t = 1/4)
    assert plan.sieve == sieve and plan.band == (2 * sieve if sieve <= 16384 else 0), (plan.sieve, plan.band)
    assert plan.bucket_bits == 6 and plan.fix_ids == want_fix_ids, (plan.bucket_bits, plan.fix_ids)
    short1, short2 = _short_ids(pid, pk, seed, spec.l0, sieve)
    want = _want(pid, pk, val, U, P, spec, seed, row_offset=row_offset)
    scale = _abs_scale(pid, pk, val, P, spec.min_value, spec.max_value, spec.middle)
    ws = X.BoundWorkspace()
    got = _run(device, pid, pk, val, U, P, spec, seed, sieve, row_offset=row_offset, workspace=ws)
    st = ws.stats()
    print("stats", st, "expected", len(short1), len(short2))
    assert st["unresolved_ids"] == len(short1), st
    if plan.band:
        assert st["unresolved2_ids"] == len(short2), st
    _compare(got, want, scale)
    off = _run(device, pid, pk, val, U, P, spec, seed, -1, row_offset=row_offset)
    np.testing.assert_array_equal(got["privacy_id_count"], off["privacy_id_count"])
    np.testing.assert_array_equal(got["count"], off["count"])
    _compare(off, want, scale)
    return st, short1, short2


CASES = [
    (1, 1, O.VALUE_F64, O.ACC_SUM | O.ACC_NSUM, 3000),
    (2, 1, O.VALUE_F64, O.ACC_SUM | O.ACC_NSUM, 6000),
    (4, 2, O.VALUE_F64, O.ACC_SUM | O.ACC_NSUM | O.ACC_NSUM2, 9000),
    (8, 2, O.VALUE_F64, O.ACC_SUM | O.ACC_NSUM, 14000),
    (2, 1, O.VALUE_NONE, 0, 6000),
    (4, 2, O.VALUE_I64, O.ACC_SUM | O.SUM_INT, 9000),
]


@pytest.mark.parametrize("case", CASES, ids=[f"l0={c[0]}-linf={c[1]}-vk={c[2]}" for c in CASES])
def test_per_id_fixup_matches_oracle(device, case):
    """Both rounds (band, then rescan) at a threshold that leaves a few
    thousand ids unresolved; two seeds and a row offset, which the sampling
    depends on."""
    l0, linf, vk, flags, sieve = case
    lo, hi = (0, 7) if vk == O.VALUE_I64 else (0.0, 10.0)
    spec = _spec(l0, linf, vk, flags, lo, hi)
    pid, pk, val = _base(11 + l0, vk=vk)
    for seed, off in ((0xA5A5_0000_1111 + l0, 0), (424242, 987_654_321)):
        st, short1, short2 = _check(device, pid, pk, val, spec, seed, sieve, row_offset=off)
        assert 100 < len(short2) <= len(short1) < U, (len(short1), len(short2))


def test_id_one_pair_short_goes_through_the_rescan(device):
    """An id with exactly l0 - 1 distinct partitions and 3,000 rows (under the
    row cap): short of l0 pairs at any threshold, so it is listed a second
    time and finished from the rescan by its own wave."""
    spec = _spec(4, 2)
    pid, pk, val = _base(5)
    rng = np.random.default_rng(6)
    target = 4099
    keep = pid != target
    pid, pk, val = pid[keep], pk[keep], val[keep]
    extra = 3000
    pid = np.concatenate([pid, np.full(extra, target)])
    pk = np.concatenate([pk, rng.choice(np.array([17, 1234, 2999]), extra)])
    val = np.concatenate([val, rng.random(extra) * 10.0])
    perm = rng.permutation(len(pid))
    pid, pk, val = pid[perm], pk[perm], val[perm]
    st, short1, short2 = _check(device, pid, pk, val, spec, 777, 9000)
    assert target in short1 and target in short2 and st["unresolved2_ids"] > 0
    assert st["fixup2_rows"] >= extra


def test_ids_over_the_row_cap_take_the_bucket_launch(device):
    """Two ids with l0 - 1 distinct partitions and more rows than the per-wave
    cap -- one whose pairs hash below t (over the cap in the first round
    already: the main launch sends all its rows), one whose pairs hash above
    2t (over the cap in the rescan's round only) -- next to thousands of ids
    finished by their own waves in the same call."""
    spec = _spec(2, 1)
    seed, sieve = 31337, 6000
    pid, pk, val = _base(9)
    rng = np.random.default_rng(10)
    heavy = {70: None, 5001: None}
    hashes = {u: O.pair_hash(seed, np.full(P, u), np.arange(P)) for u in heavy}
    heavy[70] = int(np.flatnonzero(hashes[70] < np.uint32(sieve << 16))[0])
    heavy[5001] = int(np.flatnonzero(hashes[5001] >= np.uint32(2 * sieve << 16))[0])
    keep = ~np.isin(pid, list(heavy))
    pid, pk, val = pid[keep], pk[keep], val[keep]
    extra = ROW_CAP + 1500
    for u, k in heavy.items():
        pid = np.concatenate([pid, np.full(extra, u)])
        pk = np.concatenate([pk, np.full(extra, k)])
        val = np.concatenate([val, rng.random(extra) * 10.0])
    perm = rng.permutation(len(pid))
    pid, pk, val = pid[perm], pk[perm], val[perm]
    st, short1, short2 = _check(device, pid, pk, val, spec, seed, sieve)
    assert set(heavy) <= set(short2.tolist()) and len(short1) > 1000
    assert st["fixup_rows"] > extra and st["fixup2_rows"] >= 2 * extra


def test_no_unresolved_id_launches_and_does_nothing(device):
    """Every id has 24 distinct pairs and t = 1/2 (no band: the rescan chain): none is short of l0 = 1
    pair, the fix-up launches run over empty lists."""
    spec = _spec(1, 1)
    rng = np.random.default_rng(3)
    pid = np.tile(np.arange(U), 24)
    pk = (np.repeat(np.arange(24), U) * 97 + pid * 31) % P  # 24 distinct partitions per id
    val = rng.random(len(pid)) * 10.0
    seed = next(s for s in range(100, 200) if len(_short_ids(pid, pk, s, 1, 32768)[0]) == 0)
    st, short1, short2 = _check(device, pid, pk, val, spec, seed, 32768)
    assert st["unresolved_ids"] == 0 and st["fixup_rows"] == 0 and st["unresolved2_ids"] == 0


def test_almost_every_id_unresolved(device):
    """t = 2^-16: nearly every id is unresolved after the band as well, so the
    rescan lists nearly every row and each id has a wave."""
    spec = _spec(2, 1)
    pid, pk, val = _base(21)
    st, short1, short2 = _check(device, pid, pk, val, spec, 99, 1)
    assert len(short2) > 0.99 * U and st["fixup2_rows"] > 0.99 * len(pid)


def test_out_of_range_partition_of_an_unresolved_id(device):
    """A partition key >= P among an unresolved id's rows: the error word is
    set as on the unsieved path and nothing is dereferenced -- the device
    stays healthy and the clean table then equals the oracle."""
    spec = _spec(2, 1)
    seed, sieve = 1212, 6000
    pid, pk, val = _base(33)
    short1, short2 = _short_ids(pid, pk, seed, 2, sieve)
    u = int(short2[len(short2) // 2])
    rows = np.flatnonzero(pid == u)
    assert len(rows) > 0
    bad = pk.copy()
    bad[rows[0]] = P + 5
    for s in (sieve, -1):
        with pytest.raises(ValueError, match="outside the dense key range"):
            _run(device, pid, bad, val, U, P, spec, seed, s)
    _check(device, pid, pk, val, spec, seed, sieve)


def test_bounds_over_the_lds_budget_keep_the_bucket_launches(device):
    """l0 * (1 + linf) = 48 > 32: the plan reports the bucket path and the
    result still equals the oracle."""
    spec = _spec(16, 2)
    pid, pk, val = _base(44)
    _check(device, pid, pk, val, spec, 5, 14000, want_fix_ids=0)


def test_fix_list_capacity_guard(device, monkeypatch):
    """The guard on the fix-up row list and its test hook, on the per-id path."""
    from pipelinedp_amd import _native as N
    spec = _spec(2, 1)
    pid, pk, val = _base(55)
    monkeypatch.setenv("PIPELINEDP_AMD_FIX_CAP", "64")
    with pytest.raises(N.NativeLibraryError, match="outgrew its workspace region"):
        _run(device, pid, pk, val, U, P, spec, 8, 6000)
    monkeypatch.delenv("PIPELINEDP_AMD_FIX_CAP")
    _check(device, pid, pk, val, spec, 8, 6000)
