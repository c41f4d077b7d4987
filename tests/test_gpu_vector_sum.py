"""VECTOR_SUM on the GPU: pdp_reduce_vector_sum and pdp_vector_sum_metrics at
the ABI level (through executor.reduce_vector_sum / vector_sum_metrics), and
DPEngine.aggregate on ColumnarBackend against the reference's fixture
(tests/golden/vector_sum/vector_sum.json).

The expected accumulator is the CPU oracle's: oracle.columnar.bound_and_reduce
is linear in the values, so with value = V[:, j], flags = ACC_SUM and infinite
clipping bounds its `sum` is column j of the expected [P, d] accumulator.
Integer-valued vectors (|entries| <= 2^20) must match exactly; the one
normal-valued case within rtol = 8 * (rows of the largest partition) * 2^-53
(two summations of positive terms in different orders)."""
import ctypes
import functools

import numpy as np
import pytest

import pipelinedp_amd as pdp
from oracle import columnar as O
from pipelinedp_amd import _native as N
from pipelinedp_amd import columnar_backend as CB
from pipelinedp_amd import dp_computations as dpc
from pipelinedp_amd import executor as X
from tests import vector_sum_util as V

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ data --
@functools.lru_cache(maxsize=None)
def _table(n, U, P, d, seed, hot=0.0, integer=True, empty=True):
    """Rows over U privacy ids and P partitions (a third of the partitions
    empty when P > 1; `hot` = share of the rows in one partition)."""
    rng = np.random.default_rng(seed)
    live = np.arange(P) if P == 1 or not empty else np.setdiff1d(np.arange(P), np.arange(1, P, 3))
    pid = rng.integers(0, U, n)
    pk = live[rng.integers(0, len(live), n)]
    if hot:
        pk = np.where(rng.random(n) < hot, live[len(live) // 2], pk)
    if integer:
        vec = rng.integers(-(1 << 20), (1 << 20) + 1, (n, d)).astype(np.float64)
    else:
        vec = rng.normal(5.0, 1.0, (n, d))
    return pid.astype(np.int64), pk.astype(np.int64), vec


def _expected(pid, pk, vec, *, U, P, l0, linf, seed, allowed=None, max_contributions=0, rows_are_units=False):
    cols, counts = [], None
    for j in range(vec.shape[1]):
        r = O.bound_and_reduce(pid, pk, vec[:, j], n_privacy_ids=U, n_partitions=P, l0=l0, linf=linf,
                               value_kind=O.VALUE_F64, flags=O.ACC_SUM, min_value=-np.inf, max_value=np.inf,
                               seed=seed, allowed=allowed, max_contributions=max_contributions,
                               rows_are_units=rows_are_units)
        cols.append(r["sum"])
        counts = r
    return np.stack(cols, axis=1), counts["count"], counts["privacy_id_count"]


def _run(device, pid, pk, vec, *, U, P, l0, linf, seed, allowed=None, max_contributions=0,
         rows_are_units=False, vector_acc=None, acc=None, check_keys=True, workspace=None, **kw):
    import torch
    spec = X.BoundingSpec(l0=l0, linf=linf, value_kind=N.VALUE_NONE, flags=0,
                          max_contributions=max_contributions, rows_are_units=rows_are_units)
    acc, vacc = X.reduce_vector_sum(
        None if rows_are_units else torch.as_tensor(pid, device=device), torch.as_tensor(pk, device=device),
        torch.as_tensor(vec, device=device), n_privacy_ids=U, n_partitions=P, bounding=spec, seed=seed,
        allowed=None if allowed is None else torch.as_tensor(allowed, device=device), vector_acc=vector_acc,
        acc=acc, check_keys=check_keys, workspace=workspace, **kw)
    return acc, vacc


def _check(device, pid, pk, vec, *, integer=True, **kw):
    acc, vacc = _run(device, pid, pk, vec, **kw)
    want, count, pid_count = _expected(pid, pk, vec, **kw)
    got = vacc.cpu().numpy()
    assert (acc["count"].cpu().numpy() == count).all()
    assert (acc["privacy_id_count"].cpu().numpy() == pid_count).all()
    if integer:
        assert np.array_equal(got, want)
    else:
        rtol = 8 * max(int(count.max()), 1) * 2.0**-53
        print("largest partition", int(count.max()), "rtol", rtol, "max rel err",
              float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))))
        np.testing.assert_allclose(got, want, rtol=rtol, atol=0)
    return count


# --------------------------------------------------- accumulator shapes --
@pytest.mark.parametrize("P", [1, 37])
@pytest.mark.parametrize("d", [1, 3, 64, 65, 130])
def test_accumulator_shapes(device, d, P):
    """Lane layouts: one lane per row (d = 1), padded groups (3), 16 B lanes
    (64, 130), a second column chunk (65: 8 B lanes, 130: 16 B lanes); P = 37
    has empty partitions and one holding more than half of the rows, split
    over several waves."""
    n, U = (20000, 4000) if d <= 3 else (6000, 1200)
    pid, pk, vec = _table(n, U, P, d, seed=100 + d, hot=0.6 if P > 1 else 0.0)
    count = _check(device, pid, pk, vec, U=U, P=P, l0=2, linf=2, seed=7 * d + P)
    assert count.max() > 1024  # the long-partition path ran
    if P > 1:
        assert np.bincount(pk, minlength=P).max() > n // 2 and (count == 0).any()


def test_hot_partition_every_row_kept(device):
    """NoOp bounding (every row kept): 30,000 rows, over half of them in one
    partition, whose segment starts inside a tile of the kept-row list."""
    n, U, P, d = 30000, 5000, 37, 16
    pid, pk, vec = _table(n, U, P, d, seed=5, hot=0.55)
    count = _check(device, pid, pk, vec, U=U, P=P, l0=0, linf=0, seed=3)
    assert count.max() > n // 2 and int(count.sum()) == n


@pytest.mark.parametrize("d", [3, 16])
def test_segment_split_shapes(device, d):
    """NoOp bounding, so the kept-row list is the rows by partition: partition
    3 (1,024 rows, one tile, summed whole) fills tile 0; partition 4 (1,025)
    starts exactly on the tile boundary and leaves one row in tile 2; partition
    30 (1,500) starts inside that same tile, which so writes both of its
    partial slots, and ends inside tile 3; partition 39 has 3 rows.  d = 3: 8 B
    lanes in a padded group; d = 16: 16 B lanes."""
    U, P = 500, 40
    codes, sizes = (3, 4, 30, 39), (1024, 1025, 1500, 3)
    rng = np.random.default_rng(40 + d)
    pk = rng.permutation(np.repeat(codes, sizes)).astype(np.int64)
    n = len(pk)
    pid = rng.integers(0, U, n).astype(np.int64)
    vec = rng.integers(-(1 << 20), (1 << 20) + 1, (n, d)).astype(np.float64)
    count = _check(device, pid, pk, vec, U=U, P=P, l0=0, linf=0, seed=5)
    want = np.zeros(P, np.int64)
    want[list(codes)] = sizes
    assert (count == want).all()


def test_normal_values_within_summation_order(device):
    n, U, P, d = 20000, 3000, 37, 16
    pid, pk, vec = _table(n, U, P, d, seed=6, hot=0.6, integer=False)
    _check(device, pid, pk, vec, integer=False, U=U, P=P, l0=3, linf=4, seed=4)


# ---------------------------------------------------- sampling that fires --
def test_l0_and_linf_sampling_sketch_mode(device):
    """40 privacy ids over 24 live partitions: every id has more than l0 = 2
    partitions and its pairs more than linf = 2 rows."""
    n, U, P, d = 12000, 40, 37, 3
    pid, pk, vec = _table(n, U, P, d, seed=8)
    count = _check(device, pid, pk, vec, U=U, P=P, l0=2, linf=2, seed=21)
    assert int(count.sum()) == U * 2 * 2


def test_linf_select_mode(device):
    """linf = 300 (radix select): one pair of 400 rows keeps 300 of them."""
    n, U, P, d = 4000, 300, 37, 5
    pid, pk, vec = _table(n, U, P, d, seed=9)
    pid, pk = pid.copy(), pk.copy()
    pid[pid == 299] = 298  # privacy id 299 holds that pair alone, so L0 keeps it
    pid[:400], pk[:400] = 299, 0
    count = _check(device, pid, pk, vec, U=U, P=P, l0=2, linf=300, seed=22)
    assert count[0] >= 300


# --------------------------------------------------- other bounding modes --
@pytest.mark.parametrize("linf", [2, 0], ids=["linf_sampler", "noop"])
def test_no_cross_partition_bounding(device, linf):
    n, U, P, d = 9000, 300, 37, 3
    pid, pk, vec = _table(n, U, P, d, seed=10)
    _check(device, pid, pk, vec, U=U, P=P, l0=0, linf=linf, seed=23)


def test_rows_are_units(device):
    n, U, P, d = 9000, 1, 37, 6
    pid, pk, vec = _table(n, U, P, d, seed=11)
    count = _check(device, pid, pk, vec, U=U, P=P, l0=0, linf=0, seed=24, rows_are_units=True)
    assert int(count.sum()) == n


def test_pk_allowed_mask(device):
    n, U, P, d = 9000, 700, 37, 4
    pid, pk, vec = _table(n, U, P, d, seed=12, empty=False)
    allowed = (np.arange(P) % 2 == 0).astype(np.uint8)
    acc, vacc = _run(device, pid, pk, vec, U=U, P=P, l0=2, linf=2, seed=25, allowed=allowed)
    want, count, _ = _expected(pid, pk, vec, U=U, P=P, l0=2, linf=2, seed=25, allowed=allowed)
    got = vacc.cpu().numpy()
    assert np.array_equal(got, want)
    assert not got[1::2].any() and got[0::2].any()


# ------------------------------------------------ chaining, edges, errors --
def test_two_calls_add_into_one_accumulator(device):
    U, P, d = 500, 37, 7
    a = _table(5000, U, P, d, seed=13)
    b = _table(3000, U, P, d, seed=14, hot=0.7)
    ws = X.BoundWorkspace()
    acc, vacc = _run(device, *a, U=U, P=P, l0=2, linf=2, seed=30, workspace=ws)
    acc, vacc = _run(device, *b, U=U, P=P, l0=2, linf=2, seed=31, workspace=ws, acc=acc, vector_acc=vacc)
    wa, ca, _ = _expected(*a, U=U, P=P, l0=2, linf=2, seed=30)
    wb, cb, _ = _expected(*b, U=U, P=P, l0=2, linf=2, seed=31)
    assert np.array_equal(vacc.cpu().numpy(), wa + wb)
    assert (acc["count"].cpu().numpy() == ca + cb).all()


def test_zero_rows(device):
    import torch
    P, d = 5, 4
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, d)))
    before = torch.full((P, d), 2.5, dtype=torch.float64, device=device)
    acc, vacc = _run(device, *empty, U=1, P=P, l0=2, linf=1, seed=1, vector_acc=before)
    assert (vacc.cpu().numpy() == 2.5).all() and not acc["count"].cpu().numpy().any()


def test_out_of_range_keys_set_the_error_bit_and_are_skipped(device):
    n, U, P, d = 3000, 200, 37, 3
    pid, pk, vec = _table(n, U, P, d, seed=15)
    pid, pk = pid.copy(), pk.copy()
    pid[17], pk[1234] = U, P  # one privacy id and one partition past the dense range
    ws = X.BoundWorkspace()
    acc, vacc = _run(device, pid, pk, vec, U=U, P=P, l0=2, linf=2, seed=32, check_keys=False, workspace=ws)
    flags = ctypes.c_uint32(0)
    N.check(N.lib().pdp_bound_error_flags(X._ptr(ws.buf), ctypes.byref(flags), X._stream()), "flags")
    assert flags.value == 1
    want, count, _ = _expected(pid, pk, vec, U=U, P=P, l0=2, linf=2, seed=32)  # the oracle drops them
    assert np.array_equal(vacc.cpu().numpy(), want)
    assert (acc["count"].cpu().numpy() == count).all()
    with pytest.raises(ValueError, match="dense key range"):
        _run(device, pid, pk, vec, U=U, P=P, l0=2, linf=2, seed=32)


def test_invalid_arguments(device):
    import torch
    n, U, P = 64, 8, 5
    pid, pk, vec = _table(n, U, P, 4, seed=16)
    with pytest.raises(N.NativeLibraryError, match=r"code -4.*PAIR_TABLE"):
        _run(device, pid, pk, vec, U=U, P=P, l0=2, linf=2, seed=1, algorithm=N.ALGO_BUCKETED)
    with pytest.raises(N.NativeLibraryError, match=r"code -4.*PAIR_TABLE"):  # AUTO resolves to BUCKETED here
        _run(device, pid, pk, vec, U=U, P=P, l0=2, linf=2, seed=1, algorithm=N.ALGO_AUTO)
    for d in (0, N.MAX_VECTOR_SIZE + 1):
        with pytest.raises(N.NativeLibraryError, match=r"code -4.*vector_size"):
            _run(device, pid, pk, np.zeros((n, d)), U=U, P=P, l0=2, linf=2, seed=1)
    # a workspace sized for bounding alone is too small for the vector reduction
    lib = N.lib()
    spec = X.BoundingSpec(l0=2, linf=2, value_kind=N.VALUE_NONE, flags=0)
    cfg = X.bound_config(n, U, P, spec, 1, 0, N.ALGO_PAIR_TABLE)
    small, full = ctypes.c_uint64(0), ctypes.c_uint64(0)
    N.check(lib.pdp_bound_workspace_bytes(ctypes.byref(cfg), ctypes.byref(small)), "bytes")
    N.check(lib.pdp_vector_sum_workspace_bytes(ctypes.byref(cfg), 4, ctypes.byref(full)), "bytes")
    assert full.value > small.value
    t = [torch.as_tensor(x, device=device) for x in (pid, pk, vec)]
    ws = torch.empty(full.value, dtype=torch.uint8, device=device)
    out = torch.zeros((P, 4), dtype=torch.float64, device=device)
    rc = lib.pdp_reduce_vector_sum(ctypes.byref(cfg), X._ptr(t[0]), X._ptr(t[1]), None, X._ptr(t[2]), 4,
                                   X._ptr(ws), small.value, X._ptr(out), X._stream())
    assert rc == -3 and b"workspace" in lib.pdp_last_error()
    # the metrics entry point
    index = torch.arange(P, device=device)
    for d in (0, N.MAX_VECTOR_SIZE + 1):
        with pytest.raises(N.NativeLibraryError, match="code -4"):
            X.vector_sum_metrics(torch.zeros((P, d), dtype=torch.float64, device=device), index,
                                 norm_kind=N.NORM_L1, max_norm=1.0, noise=dpc.NO_NOISE, seed=1)
    with pytest.raises(N.NativeLibraryError, match="code -1"):
        X.vector_sum_metrics(out, index, norm_kind=7, max_norm=1.0, noise=dpc.NO_NOISE, seed=1)


# --------------------------------------------------- pdp_vector_sum_metrics --
def _fixture_acc(fx, device):
    """The fixture's accumulators as a [P + 1, d] device matrix, the last row
    all zero, and the partitions in fixture order."""
    import torch
    vectors = V.accumulator_vectors(fx)
    pks = sorted(vectors)
    d = V.FIXTURE["vector_size"]
    mat = np.zeros((max(pks) + 2, d))
    for pk in pks:
        mat[pk] = vectors[pk]
    return torch.as_tensor(mat, device=device), pks


@pytest.mark.parametrize("fx", V.cases(), ids=V.case_ids())
@pytest.mark.parametrize("kind", ["linf", "l1", "l2"])
def test_metrics_clip_only_matches_reference(device, fx, kind):
    import torch
    vacc, pks = _fixture_acc(fx, device)
    clip = V.clip_of(fx, kind)
    zero_row = vacc.shape[0] - 1
    index = torch.as_tensor(pks + [zero_row], device=device)
    out = X.vector_sum_metrics(vacc, index, norm_kind=CB._NORM_CODES[kind], max_norm=clip["max_norm"],
                               noise=dpc.NO_NOISE, seed=1).cpu().numpy()
    want = {pk: v for pk, v in clip["clipped"]}
    d = V.FIXTURE["vector_size"]
    exact = fx["case"]["integer"] and kind in ("linf", "l1")
    for i, pk in enumerate(pks):
        if exact:
            assert out[i].tolist() == [float(x) for x in want[pk]], (pk, kind)
        else:
            np.testing.assert_allclose(out[i], want[pk], rtol=1e-12 if kind == "l2" else 1e-15 * d, atol=0)
    assert not np.isnan(out).any()
    assert out[-1].tolist() == [float(x) for x in clip["zero_clipped"]]


@pytest.mark.parametrize("noise_kind", [pdp.NoiseKind.LAPLACE, pdp.NoiseKind.GAUSSIAN], ids=["laplace", "gaussian"])
@pytest.mark.parametrize("kind", ["linf", "l1"])
def test_metrics_noise_is_bit_equal_to_the_oracle(device, kind, noise_kind):
    """Integer accumulators, so the clipped values are exact; stream index of
    out[i][j] = (partition_offset + p) * d + j on slot PDP_VECTOR_SUM_SLOT;
    n_kept_dev below n_kept leaves the rows past it untouched."""
    import torch
    fx = V.cases()[0]
    assert fx["case"]["integer"]
    vacc, pks = _fixture_acc(fx, device)
    clip = V.clip_of(fx, kind)
    d = V.FIXTURE["vector_size"]
    noise = dpc.noise_params(noise_kind, 1.0 / d, 1e-6 / d, 2, 2)
    seed, offset, n_dev = 0xC0FFEE1234567, 1000, len(pks) - 7
    index = torch.as_tensor(pks, device=device)
    out = torch.full((len(pks), d), -777.0, dtype=torch.float64, device=device)
    X.vector_sum_metrics(vacc, index, norm_kind=CB._NORM_CODES[kind], max_norm=clip["max_norm"], noise=noise,
                         seed=seed, partition_offset=offset, out=out,
                         n_kept_dev=torch.as_tensor([n_dev], device=device))
    got = out.cpu().numpy()
    vectors = V.accumulator_vectors(fx)
    clipped = np.stack([np.asarray(dpc.clip_vector(vectors[pk], clip["max_norm"], pdp.NormKind(kind)), np.float64)
                        for pk in pks[:n_dev]])
    gidx = ((offset + np.asarray(pks[:n_dev], np.int64))[:, None] * d + np.arange(d)[None, :]).ravel()
    want = O.secure_add_noise(noise.as_dict(), clipped.ravel(), seed, gidx, N.VECTOR_SUM_SLOT).reshape(n_dev, d)
    assert np.array_equal(got[:n_dev], want)
    assert (got[n_dev:] == -777.0).all()
    assert (got[:n_dev] != clipped).any()


def test_metrics_laplace_noise_distribution(device):
    """KS test of the released noise against Laplace(b), b = l0 linf / (eps / d)."""
    import torch
    from scipy.stats import kstest, laplace
    P, d = 3000, 4
    vacc = torch.full((P, d), 3.0, dtype=torch.float64, device=device)
    noise = dpc.noise_params(pdp.NoiseKind.LAPLACE, 1.0 / d, 0.0, 2, 1)
    out = X.vector_sum_metrics(vacc, torch.arange(P, device=device), norm_kind=N.NORM_LINF, max_norm=10.0,
                               noise=noise, seed=99).cpu().numpy()
    assert abs(noise.scale - 2 * d) < 1e-12
    assert kstest(out.ravel() - 3.0, laplace(scale=noise.scale).cdf).pvalue > 1e-4
    # coordinates draw independently: no two columns share their noise
    assert not np.array_equal(out[:, 0], out[:, 1])


# ------------------------------------------------------------- API level --
_EXT = dict(privacy_id_extractor=pdp.ColumnExtractor("pid"), partition_extractor=pdp.ColumnExtractor("pk"),
            value_extractor=pdp.ColumnExtractor("v"))


def _source(fx, how, device):
    import torch
    rows = fx["rows"]
    if how == "rows":
        ext = pdp.DataExtractors(privacy_id_extractor=lambda r: r[0], partition_extractor=lambda r: r[1],
                                 value_extractor=lambda r: r[2])
        return [tuple(r) for r in rows], ext
    pid = np.asarray([r[0] for r in rows], np.int64)
    pk = np.asarray([r[1] for r in rows], np.int64)
    v = np.asarray([r[2] for r in rows], np.float64)
    if how == "device":
        cols = {"pid": torch.as_tensor(pid, device=device), "pk": torch.as_tensor(pk, device=device),
                "v": torch.as_tensor(v, device=device)}
        return pdp.ColumnTable(cols, n_privacy_ids=int(pid.max()) + 1, n_partitions=int(pk.max()) + 1), \
            pdp.DataExtractors(**_EXT)
    return pdp.ColumnTable({"pid": pid, "pk": pk, "v": v}), pdp.DataExtractors(**_EXT)


def _noise_tolerance(fx, eps, delta, n_requests):
    """40 scales of the per-coordinate noise plus its grid: P(|Laplace| > 40 b)
    = e^-40, a Gaussian's 40 sigma is rarer still."""
    d, case = V.FIXTURE["vector_size"], fx["case"]
    p = dpc.noise_params(getattr(pdp.NoiseKind, case["noise"]), eps / n_requests / d, delta / n_requests / d,
                         case["l0"], case["linf"])
    return 40 * p.scale + p.granularity


@pytest.mark.parametrize("how", ["rows", "table", "device"])
@pytest.mark.parametrize("kind", ["linf", "l1", "l2"])
@pytest.mark.parametrize("fx", V.cases(), ids=V.case_ids())
def test_aggregate_public_partitions_huge_eps(device, fx, kind, how):
    clip = V.clip_of(fx, kind)
    src, ext = _source(fx, how, device)
    eps, delta = 1e6, 1e-6
    acc = pdp.NaiveBudgetAccountant(total_epsilon=eps, total_delta=delta)
    engine = pdp.DPEngine(acc, CB.ColumnarBackend(device=device, seed=17))
    public = sorted(pk for pk, _ in fx["expected"])
    sink = engine.aggregate(src, V.params(fx, norm_kind=kind, max_norm=clip["max_norm"]), ext,
                            public_partitions=public)
    acc.compute_budgets()
    out = dict(sink)
    assert sorted(out) == public
    want_vec = {pk: np.asarray(v, np.float64) for pk, v in clip["clipped"]}
    want_acc = {pk: a for pk, a in fx["expected"]}
    tol = _noise_tolerance(fx, eps, delta, 3)
    assert tol < 1e-2
    # + the accumulator's summation order against the reference's: m rows of |v| <= vmax
    # summed in any order err by at most m u sum|v| <= m^2 u vmax each (u = 2^-53); clipping shrinks
    m = max(a[1][0] for _, a in fx["expected"])
    vmax = max(abs(x) for r in fx["rows"] for x in r[2])
    tol += 2 * m * m * 2.0**-53 * vmax
    rel = 1e-12 if kind == "l2" else 0.0
    for pk, m in out.items():
        assert m._fields == ("count", "privacy_id_count", "vector_sum")
        assert isinstance(m.vector_sum, np.ndarray) and m.vector_sum.shape == (V.FIXTURE["vector_size"],)
        np.testing.assert_allclose(m.vector_sum, want_vec[pk], rtol=rel, atol=tol)
        assert abs(m.count - want_acc[pk][1][0]) <= 1 and abs(m.privacy_id_count - want_acc[pk][1][1]) <= 1


@pytest.mark.parametrize("fx", V.cases(), ids=V.case_ids())
def test_aggregate_private_selection_budgets_and_fields(device, fx):
    """The fixture's own budget (eps = 1, delta = 1e-6) with private
    selection: the budget split equals the reference's."""
    src, ext = _source(fx, "table", device)
    acc = pdp.NaiveBudgetAccountant(total_epsilon=1.0, total_delta=1e-6)
    engine = pdp.DPEngine(acc, CB.ColumnarBackend(device=device, seed=18))
    sink = engine.aggregate(src, V.params(fx, norm_kind="l2", max_norm=10.0), ext)
    acc.compute_budgets()
    got = [[m.mechanism_spec.mechanism_type.value, m.mechanism_spec.eps, m.mechanism_spec.delta]
           for m in acc._mechanisms]
    assert got == fx["budgets"]
    out = list(sink)
    assert sink.collect().fields == ("count", "privacy_id_count", "vector_sum")
    assert sink.collect().columns["vector_sum"].shape == (len(out), V.FIXTURE["vector_size"])
    for _, m in out:
        assert m.vector_sum.shape == (V.FIXTURE["vector_size"],) and np.isfinite(m.vector_sum).all()


def test_aggregate_private_selection_vectors_line_up_with_keys(device):
    """Half of the partitions hold one privacy id (dropped at delta = 1e-6),
    the others sixty (kept at a huge eps): every kept partition's vector is its
    own key's."""
    d, P, big = 3, 40, 60
    pid, pk, vec = [], [], []
    for p in range(P):
        for u in range(big if p % 2 else 1):
            pid.append(len(pid))
            pk.append(p)
            vec.append([p + 1.0, -2.0 * p, 0.5])
    table = pdp.ColumnTable({"pid": np.asarray(pid, np.int64), "pk": np.asarray(pk, np.int64),
                             "v": np.asarray(vec, np.float64)})
    params = pdp.AggregateParams(metrics=[pdp.Metrics.VECTOR_SUM, pdp.Metrics.COUNT],
                                 noise_kind=pdp.NoiseKind.LAPLACE, max_partitions_contributed=1,
                                 max_contributions_per_partition=1, vector_size=d, vector_max_norm=1e9,
                                 vector_norm_kind=pdp.NormKind.Linf)
    acc = pdp.NaiveBudgetAccountant(total_epsilon=1e6, total_delta=1e-6)
    engine = pdp.DPEngine(acc, CB.ColumnarBackend(device=device, seed=19))
    sink = engine.aggregate(table, params, pdp.DataExtractors(**_EXT))
    acc.compute_budgets()
    out = dict(sink)
    assert sorted(out) == [p for p in range(P) if p % 2]
    for p, m in out.items():
        np.testing.assert_allclose(m.vector_sum, big * np.asarray([p + 1.0, -2.0 * p, 0.5]), rtol=0, atol=1e-2)
        assert abs(m.count - big) <= 1


def test_wrong_vector_shape_raises_type_error(device):
    fx = V.cases()[0]
    rows = [tuple(r) for r in fx["rows"][:20]] + [(0, 0, [1.0, 2.0])]
    ext = pdp.DataExtractors(privacy_id_extractor=lambda r: r[0], partition_extractor=lambda r: r[1],
                             value_extractor=lambda r: r[2])
    acc = pdp.NaiveBudgetAccountant(total_epsilon=1.0, total_delta=1e-6)
    engine = pdp.DPEngine(acc, CB.ColumnarBackend(device=device, seed=20))
    sink = engine.aggregate(rows, V.params(fx), ext)
    acc.compute_budgets()
    with pytest.raises(TypeError, match=r"Shape mismatch: \(2,\) != \(5,\)"):
        list(sink)
