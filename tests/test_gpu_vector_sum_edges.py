"""VECTOR_SUM at the kernels' own edges, by equality: the lane layouts of
k_vs_reduce / k_vs_combine (pdp_pairs.hip) at both alignments, the entries per
row slot of vs_sum, the sampling modes of the kept-row marking, and the L1 / L2
clip, the noise streams and the loop bounds of k_vector_sum_metrics
(pdp_select.hip).  Inputs and expectations come from
tests/vector_sum_edges_util.py, which tests/test_vector_sum_edges_host.py
proves on the CPU.  Every accumulator is integer-valued with sums that are
exact in any order, so every comparison is of bits; the two exceptions are the
normal-valued clip (clip_bound, derived in the util) and the API case (the
noise at eps = 1e6)."""
import numpy as np
import pytest

import pipelinedp_amd as pdp
from oracle import columnar as O
from pipelinedp_amd import _native as N
from pipelinedp_amd import columnar_backend as CB
from pipelinedp_amd import dp_computations as dpc
from pipelinedp_amd import executor as X
from tests import vector_sum_edges_util as E

pytestmark = pytest.mark.gpu


def _placed(device, mat, off):
    """`mat` on the device, 16-byte aligned or 8 bytes off; the test states which."""
    import torch
    t = torch.as_tensor(np.ascontiguousarray(mat), device=device)
    if off:
        t = E.offset_view(t, *mat.shape)
        assert t.data_ptr() % 16 == 8
    else:
        assert t.data_ptr() % 16 == 0
    return t


def _reduce(device, pid, pk, vectors, *, U, P, l0=0, linf=0, seed=5, vector_acc=None, row_offset=0,
            allowed=None, max_contributions=0):
    import torch
    spec = X.BoundingSpec(l0=l0, linf=linf, value_kind=N.VALUE_NONE, flags=0, max_contributions=max_contributions)
    return X.reduce_vector_sum(torch.as_tensor(pid, device=device), torch.as_tensor(pk, device=device), vectors,
                               n_privacy_ids=U, n_partitions=P, bounding=spec, seed=seed, row_offset=row_offset,
                               allowed=None if allowed is None else torch.as_tensor(allowed, device=device),
                               vector_acc=vector_acc)


def _reduce_into_prefill(device, pid, pk, vec, P, want_sums, vectors_off, acc_off):
    """NoOp bounding into an accumulator of P rows that is a view of P + 1:
    live partitions hold an integer vector before the call and prefill + sum
    after it, the empty ones stay NaN in every coordinate, and the guard row
    keeps its bits."""
    live = np.bincount(pk, minlength=P) > 0
    before = E.prefill(P, vec.shape[1], live)
    full = _placed(device, before, acc_off)
    acc, vacc = _reduce(device, pid, pk, _placed(device, vec, vectors_off), U=500, P=P, vector_acc=full[:P])
    assert vacc.data_ptr() == full.data_ptr()
    got = full.cpu().numpy()
    want = before.copy()
    want[:P][live] += want_sums[live]
    assert not want_sums[~live].any() and (acc["count"].cpu().numpy() == np.bincount(pk, minlength=P)).all()
    assert np.isnan(got[:P][~live]).all()
    assert (got[P].view(np.int64) == before[P].view(np.int64)).all()
    assert E.same_bits(got[:P][live], want[:P][live])
    assert (got.view(np.int64) == want.view(np.int64)).all()  # the untouched NaNs bit for bit as well


# ------------------------------------------------------- (a) lane layouts --
@pytest.mark.parametrize("name", list(E.LAYOUTS))
def test_lane_layouts(device, name):
    d, vectors_off, acc_off, _ = E.LAYOUTS[name]
    pid, pk, vec, P = E.split_table(d)
    _reduce_into_prefill(device, pid, pk, vec, P, E.split_expected(d), vectors_off, acc_off)


# ------------------------------------------------ (b) entries per row slot --
@pytest.mark.parametrize("name", list(E.SLOT_LAYOUTS))
def test_entries_per_row_slot(device, name):
    d, vectors_off, R = E.SLOT_LAYOUTS[name]
    assert E.geometry(d, vectors_off, False)[3] == R
    pid, pk, vec, P = E.slot_table(d)
    _reduce_into_prefill(device, pid, pk, vec, P, E.accumulate(pk, vec, P), vectors_off, False)


# ----------------------------------------------------------- (c) sampling --
@pytest.mark.parametrize("name", list(E.SAMPLED_CASES))
def test_sampled_rows(device, name):
    """max_contributions = 3 (pid_keeps with maxc), row_offset = 2^32 + 5 in
    row_key for pairs over linf = 2, and an allowed mask under l0 = linf = 2:
    counts and sums equal the oracle's, and the all-ones column is the count."""
    pid, pk, vec, kw, kept, count, pid_count = E.sampled_case(name)
    E.check_sampled_case(name)
    acc, vacc = _reduce(device, pid, pk, _placed(device, vec, False), U=kw["U"], P=kw["P"], l0=kw["l0"],
                        linf=kw["linf"], seed=kw["seed"], row_offset=kw["row_offset"], allowed=kw["allowed"],
                        max_contributions=kw["max_contributions"])
    got = vacc.cpu().numpy()
    got_count = acc["count"].cpu().numpy()
    assert (got_count == count).all() and (acc["privacy_id_count"].cpu().numpy() == pid_count).all()
    assert int(got_count.sum()) == int(kept.sum())
    assert E.same_bits(got, E.accumulate(pk, vec, kw["P"], kept))
    assert (got[:, 1] == got_count).all()


# --------------------------------------------- (d) L1 / L2 clip, integers --
def _metrics(device, acc, index, kind, max_norm, noise=dpc.NO_NOISE, **kw):
    import torch
    index = torch.as_tensor(np.ascontiguousarray(index, dtype=np.int64), device=device)
    return X.vector_sum_metrics(torch.as_tensor(acc, device=device), index, norm_kind=CB._NORM_CODES[kind],
                                max_norm=max_norm, noise=noise, seed=E.NOISE_SEED, **kw).cpu().numpy()


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("d", E.CLIP_DS)
def test_clip_integer_rows(device, d, kind):
    """norm below, above and equal to max_norm, the zero row, mass beyond
    coordinate 64 only, the last coordinate only; through a permuted index with
    a repeat.  Equality under L2 rests on fp64 sqrt and division being
    correctly rounded on the device."""
    acc = E.clip_acc(d, kind)
    got = _metrics(device, acc, E.CLIP_INDEX, kind, E.MAX_NORM)
    assert E.same_bits(got, E.clip_rows(acc, E.CLIP_INDEX, kind, E.MAX_NORM))
    for i, r in enumerate(E.CLIP_INDEX):
        if E.CLIP_ROWS[r] in ("below", "equal", "zero"):
            assert E.same_bits(got[i], acc[r])  # coef = 1: the input's bits
    assert E.same_bits(got[1], got[4])  # the repeated partition


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("d", E.CLIP_DS)
def test_clip_to_max_norm_zero(device, d, kind):
    """The zero row stays zero (0 / 0 = NaN, coef 1); every other coordinate
    becomes a zero of its own sign."""
    acc = E.clip_acc(d, kind)
    got = _metrics(device, acc, E.CLIP_INDEX, kind, 0.0)
    assert E.same_bits(got, E.clip_rows(acc, E.CLIP_INDEX, kind, 0.0))
    assert not got.any() and (np.signbit(got) == np.signbit(acc[list(E.CLIP_INDEX)])).all()


# ------------------------------ (e) L1 / L2 clip, non-dyadic and non-finite --
@pytest.mark.parametrize("kind", E.KINDS)
def test_clip_normal_values_within_the_derived_bound(device, kind):
    acc = E.normal_acc()
    index = np.arange(len(acc))[::-1]
    got = _metrics(device, acc, index, kind, E.MAX_NORM)
    want = E.clip_rows_exact(acc, index, kind, E.MAX_NORM)
    bound = E.clip_bound(acc.shape[1])
    err = np.abs(got - want) / np.abs(want)
    print(kind, "clip_bound", bound, "largest relative error", float(err.max()))
    assert (np.abs(got - want) <= bound * np.abs(want)).all()
    assert E.same_bits(got[(want == acc[index]).all(axis=1)], acc[index][(want == acc[index]).all(axis=1)])


@pytest.mark.parametrize("kind", E.KINDS)
def test_clip_non_finite_coordinates(device, kind):
    """As the reference's _clip_vector: an infinite coordinate makes the norm
    infinite and coef 0, so the finite coordinates become zeros of their sign
    and the infinite one NaN; a NaN coordinate makes the quotient NaN, and
    min(1, NaN) is 1 there (Python's min) as fmin(1, NaN) is here, so the
    finite coordinates pass through unscaled."""
    acc = E.nonfinite_acc()
    index = np.arange(len(acc))
    got = _metrics(device, acc, index, kind, E.MAX_NORM)
    assert E.same_bits(got, E.clip_rows(acc, index, kind, E.MAX_NORM))
    for r, (v, j) in enumerate(E.NONFINITE):
        others = np.arange(E.NONFINITE_D) != j
        assert np.isnan(got[r, j])
        assert E.same_bits(got[r, others], acc[r, others] if np.isnan(v) else acc[r, others] * 0.0)


# --------------------------------------------------- (f) noise, L1 and L2 --
@pytest.mark.parametrize("noise_kind", ["laplace", "gaussian"])
@pytest.mark.parametrize("kind", E.KINDS)
def test_noise_under_l1_l2_is_bit_equal_to_the_oracle(device, kind, noise_kind):
    """Stream (partition_offset + p) * d + j of slot PDP_VECTOR_SUM_SLOT, with
    2^32 crossed inside row 3."""
    d = E.NOISE_D
    acc = E.clip_acc(d, kind)
    noise = E.noise(noise_kind, d)
    got = _metrics(device, acc, E.NOISE_INDEX, kind, E.MAX_NORM, noise=noise, partition_offset=E.NOISE_OFFSET)
    clipped = E.clip_rows(acc, E.NOISE_INDEX, kind, E.MAX_NORM)
    gidx = E.noise_gidx(E.NOISE_INDEX, E.NOISE_OFFSET, d)
    assert gidx.min() < 2**32 <= gidx.max()
    want = O.secure_add_noise(noise.as_dict(), clipped.ravel(), E.NOISE_SEED, gidx, N.VECTOR_SUM_SLOT).reshape(-1, d)
    assert E.same_bits(got, want)
    drawn = got - O.round_to_multiple(clipped, noise.granularity)
    for r in range(len(drawn)):
        assert (drawn[r, :d - 64] != drawn[r, 64:]).any()  # columns j and j + 64 draw on their own


# ----------------------------------------------------- (g) loop bounds --
def _loop_run(device, n_kept, *, index_len=None, n_kept_dev=None):
    """out is a view of n_kept rows of a sentinel-filled buffer one row
    longer (more when the index is longer); returns the whole buffer."""
    import torch
    index = E.loop_index(index_len or n_kept)
    acc = E.loop_acc()
    buf = torch.full((len(index) + 1, E.LOOP_D), E.SENTINEL, dtype=torch.float64, device=device)
    X.vector_sum_metrics(torch.as_tensor(acc, device=device), torch.as_tensor(index, device=device),
                         norm_kind=N.NORM_L2, max_norm=E.MAX_NORM, noise=dpc.NO_NOISE, seed=1, n_kept=n_kept,
                         n_kept_dev=None if n_kept_dev is None else torch.as_tensor([n_kept_dev], device=device),
                         out=buf[:n_kept])
    return buf.cpu().numpy(), E.clip_rows(acc, index, "l2", E.MAX_NORM)


@pytest.mark.parametrize("n_kept", E.LOOP_N)
def test_metrics_second_and_third_grid_stride_trip(device, n_kept):
    got, want = _loop_run(device, n_kept)
    assert E.same_bits(got[:n_kept], want) and (got[n_kept:] == E.SENTINEL).all()


def test_metrics_device_count_above_n_kept(device):
    n = E.LOOP_N[0]
    got, want = _loop_run(device, n, n_kept_dev=n + 7)
    assert E.same_bits(got[:n], want) and (got[n:] == E.SENTINEL).all()


def test_metrics_device_count_zero(device):
    got, _ = _loop_run(device, E.LOOP_N[0], n_kept_dev=0)
    assert (got == E.SENTINEL).all()


def test_metrics_n_kept_below_the_index_length(device):
    n = E.LOOP_N[0]
    got, want = _loop_run(device, n - 100, index_len=n)
    assert E.same_bits(got[:n - 100], want[:n - 100]) and (got[n - 100:] == E.SENTINEL).all()


# ---------------------------------------------------------------- (h) API --
def test_aggregate_vector_size_130_l2(device):
    """DPEngine.aggregate at a vector size above one wave: one row per privacy
    id, l0 = linf = 1 (no sampling), public partitions with an empty one.  The
    clip of the integer sums is exact, so the tolerance is the noise alone: the
    formula of tests/test_gpu_vector_sum.py's _noise_tolerance (40 scales plus
    the grid) at this case's eps / 2 / d."""
    pid, pk, vec = E.api_table()
    d, P, eps, delta = E.API["d"], E.API["P"], E.API["eps"], E.API["delta"]
    want = E.clip_rows(E.check_api_table(), np.arange(P), "l2", E.API["max_norm"])
    count = np.bincount(pk, minlength=P)
    table = pdp.ColumnTable({"pid": pid, "pk": pk, "v": vec})
    ext = pdp.DataExtractors(privacy_id_extractor=pdp.ColumnExtractor("pid"),
                             partition_extractor=pdp.ColumnExtractor("pk"), value_extractor=pdp.ColumnExtractor("v"))
    params = pdp.AggregateParams(metrics=[pdp.Metrics.VECTOR_SUM, pdp.Metrics.COUNT],
                                 noise_kind=pdp.NoiseKind.LAPLACE, max_partitions_contributed=1,
                                 max_contributions_per_partition=1, vector_size=d,
                                 vector_max_norm=E.API["max_norm"], vector_norm_kind=pdp.NormKind.L2)
    accountant = pdp.NaiveBudgetAccountant(total_epsilon=eps, total_delta=delta)
    engine = pdp.DPEngine(accountant, CB.ColumnarBackend(device=device, seed=21))
    sink = engine.aggregate(table, params, ext, public_partitions=list(range(P)))
    accountant.compute_budgets()
    out = dict(sink)
    assert sorted(out) == list(range(P))
    p = dpc.noise_params(pdp.NoiseKind.LAPLACE, eps / 2 / d, delta / 2 / d, 1, 1)
    tol = 40 * p.scale + p.granularity
    assert tol < 2e-2
    assert not want[E.API["empty"]].any() and count[E.API["empty"]] == 0
    for k, m in out.items():
        assert m.vector_sum.shape == (d,)
        err = float(np.abs(m.vector_sum - want[k]).max())
        assert err <= tol, (k, err, tol)
        assert abs(m.count - count[k]) <= 1
