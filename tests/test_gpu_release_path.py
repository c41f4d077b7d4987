"""The release path (pdp_select.hip) at the sizes where its code paths begin.

Selection, compaction and the noisy metrics decide which partitions leave the
library and with what noise.  Accumulators are made directly (no rows are
bounded), the reference is oracle/columnar.py on the CPU in fp64 / int64 and,
for compaction, np.flatnonzero.  Every comparison is an equality, NaN matching
NaN, except VARIANCE's column 0 (tests/release_path_util.compare_metrics).

Where each path begins:
* k_select_gauss hands a lane a second partition once a wave's chunk
  ceil(P / n_waves) exceeds 64: P >= 524,289 (2,048 workgroups of 4 waves).
* k_compact_scan reads a nonzero carry from its second tile of 256 block
  counts: n >= 256 * 4,096 + 1 = 1,048,577.
* k_noise_metrics pads an op list's draws to G = 1, 2, 4, 8, 16, 32 lanes and
  takes a second grid-stride trip once n_kept * G > 524,288.
* philox_for / noise_block put the global index's high word into the counter:
  offsets of 2^32 and more.
"""
import numpy as np
import pytest

from oracle import columnar as O
from pipelinedp_amd import dp_computations as dpc
from pipelinedp_amd import executor as X
from tests import release_path_util as RU

pytestmark = pytest.mark.gpu

lap, gau = dpc.laplace_noise_params, dpc.gaussian_noise_params


# ----------------------------------------------------------------- selection --
def _row_counts(P, seed, empty, mr, pre):
    """Row counts 1..40, a fraction `empty` of them 0; from 257 partitions up,
    the counts whose privacy-unit count ceil(rc / mr) is exactly
    pre_threshold - 1, pre_threshold and pre_threshold + 1 are planted."""
    rng = np.random.default_rng(seed)
    rc = rng.integers(1, 41, P).astype(np.int64)
    rc[rng.random(P) < empty] = 0
    if pre > 0 and P >= 257:
        edge = sorted({r for n in (pre - 1, pre, pre + 1) for r in (n * mr, (n - 1) * mr + 1) if r > 0})
        rc[3:3 + 7 * len(edge):7] = edge
    return rc


def _units(rc, mr, pre):
    """(passes the pre-threshold, privacy units minus the pre-threshold shift)."""
    n = (rc + mr - 1) // mr
    ok = (rc > 0) & (n >= pre)
    return ok, n - max(pre - 1, 0)


def _median_threshold(rc, mr, pre):
    ok, n = _units(rc, mr, pre)
    return float(np.median(n[ok])) + 0.25 if ok.any() else 0.0


def _check_selection(device, rc, sel, seed, offset, want_noised=True, fraction=True):
    """keep, noised count, compacted index and n_kept against the oracle."""
    keep_t, noised_t = RU.select(device, rc, sel, seed=seed, partition_offset=offset, want_noised=want_noised)
    want_keep, want_nz = RU.oracle_select(rc, sel, seed=seed, partition_offset=offset)
    live = int((rc > 0).sum())
    if fraction and live >= 40:  # the threshold must leave the decision to the noise
        assert 0.2 * live <= want_keep.sum() <= 0.8 * live, (int(want_keep.sum()), live)
    np.testing.assert_array_equal(keep_t.cpu().numpy(), want_keep.astype(np.uint8))
    if want_noised:
        np.testing.assert_array_equal(noised_t.cpu().numpy(), want_nz)
        thresholding = sel.strategy in (O.SELECT_LAPLACE, O.SELECT_GAUSSIAN)  # the others release no count
        assert np.isnan(want_nz[~want_keep]).all() and np.isnan(want_nz[want_keep]).any() != thresholding
    index, count = RU.compact(device, keep_t)
    RU.check_compaction(index, count, want_keep)
    return want_keep


GAUSS_SIZES = [1, 63, 64, 65, 257, 524_288, 524_289, 700_001]


@pytest.mark.parametrize("mr,pre", [(1, 0), (3, 0), (1, 2), (3, 2)])
@pytest.mark.parametrize("P", GAUSS_SIZES)
def test_select_gauss_matches_oracle(device, P, mr, pre):
    """k_select_gauss: chunks of at most 64 (no hand-off) up to P = 524,288,
    hand-offs from 524,289 on; at 700,001 the chunk is 86, the last wave with
    work is partial and empty waves follow it.  About 85 % of the partitions
    of the large tables are empty, so lanes finish on the first trip and dead
    partitions arrive after a hand-off.  Both strategies that reach the kernel,
    one of them at a partition offset above 2^32."""
    rc = _row_counts(P, P + 10 * mr + pre, 0.85 if P >= 524_288 else 0.2, mr, pre)
    if P == 1:
        rc[0] = 7
    for strategy, offset in ((O.SELECT_GAUSSIAN, 0), (O.SELECT_LAPLACE, RU.BIG_OFFSET)):
        sel = X.SelectionSpec(strategy=strategy, max_rows_per_privacy_id=mr, pre_threshold=pre, noise=gau(2.5),
                              threshold=_median_threshold(rc, mr, pre), want_noised_count=True)
        _check_selection(device, rc, sel, 42 + P, offset)


def test_select_gauss_coarse_grid(device):
    """A noise grid above 1 (sigma = 2^28: g = 2) takes round_to_multiple in the
    set-up of a fresh partition, not the integer shortcut; odd unit counts sit
    exactly half a step off the grid (ties go toward zero)."""
    mr, pre = 3, 2
    rc = _row_counts(5_000, 5, 0.2, mr, pre)
    noise = gau(2.0 ** 28)
    assert noise.granularity == 2.0
    sel = X.SelectionSpec(strategy=O.SELECT_GAUSSIAN, max_rows_per_privacy_id=mr, pre_threshold=pre, noise=noise,
                          threshold=_median_threshold(rc, mr, pre), want_noised_count=True)
    _check_selection(device, rc, sel, 77, RU.BIG_OFFSET)


@pytest.mark.parametrize("mr,pre", [(1, 0), (3, 0), (1, 2), (3, 2)])
@pytest.mark.parametrize("strategy", [O.SELECT_LAPLACE, O.SELECT_GAUSSIAN], ids=["laplace", "gaussian"])
def test_select_laplace_noise_matches_oracle(device, strategy, mr, pre):
    """k_select's thresholding branch (Laplace noise) with both strategies."""
    rc = _row_counts(5_000, 100 + mr + pre, 0.2, mr, pre)
    for offset in (0, RU.BIG_OFFSET):
        sel = X.SelectionSpec(strategy=strategy, max_rows_per_privacy_id=mr, pre_threshold=pre, noise=lap(0.4, 1.0),
                              threshold=_median_threshold(rc, mr, pre), want_noised_count=True)
        _check_selection(device, rc, sel, 4242, offset)


@pytest.mark.parametrize("mr,pre", [(1, 0), (3, 0), (1, 2), (3, 2)])
@pytest.mark.parametrize("table_len", [12, 1])
def test_select_truncated_geometric_clamps_to_the_table(device, table_len, mr, pre):
    """A keep table shorter than the largest unit count: k_select reads its
    last entry for every count past it (a table of one entry: always that)."""
    rc = _row_counts(5_000, 200 + mr + pre, 0.2, mr, pre)
    ok, n = _units(rc, mr, pre)
    assert (n[ok] >= table_len).any() and (table_len == 1 or (n[ok] < table_len - 1).any())
    table = np.array([0.37]) if table_len == 1 else np.linspace(0.0, 0.7, table_len)
    sel = X.SelectionSpec(strategy=O.SELECT_TRUNCATED_GEOMETRIC, max_rows_per_privacy_id=mr, pre_threshold=pre,
                          keep_prob=table)
    for offset in (0, RU.BIG_OFFSET):
        keep = _check_selection(device, rc, sel, 9, offset, fraction=False)
        past = ok & (n >= table_len)  # clamped partitions: kept at the last entry's rate
        assert abs(keep[past].mean() - table[-1]) < 0.1


@pytest.mark.parametrize("kernel", ["k_select", "k_select_gauss"])
def test_select_without_noised_count(device, kernel):
    """noised == nullptr on both kernels (the large table hands lanes on)."""
    P, noise = (5_000, lap(0.4, 1.0)) if kernel == "k_select" else (524_289, gau(2.5))
    rc = _row_counts(P, 31, 0.85 if P > 5_000 else 0.2, 3, 2)
    sel = X.SelectionSpec(strategy=O.SELECT_GAUSSIAN, max_rows_per_privacy_id=3, pre_threshold=2, noise=noise,
                          threshold=_median_threshold(rc, 3, 2))
    _check_selection(device, rc, sel, 8, 1000, want_noised=False)


def test_select_gauss_lane_independence(device):
    """A partition's decision depends on (seed, global index) alone: a table of
    700,001 partitions selected whole and as two shards at their offsets gives
    the same keep and noised columns.  A hand-off that carried k, base or
    shift over from the lane's previous partition would not."""
    P, cut, mr, pre = 700_001, 300_007, 3, 2
    rc = _row_counts(P, 17, 0.4, mr, pre)
    sel = X.SelectionSpec(strategy=O.SELECT_GAUSSIAN, max_rows_per_privacy_id=mr, pre_threshold=pre, noise=gau(2.5),
                          threshold=_median_threshold(rc, mr, pre), want_noised_count=True)
    for offset in (0, RU.BIG_OFFSET):
        whole = RU.select(device, rc, sel, seed=5, partition_offset=offset)
        a = RU.select(device, rc[:cut], sel, seed=5, partition_offset=offset)
        b = RU.select(device, rc[cut:], sel, seed=5, partition_offset=offset + cut)
        keep = whole[0].cpu().numpy()
        assert 0.2 * (rc > 0).sum() <= keep.sum() <= 0.8 * (rc > 0).sum()
        np.testing.assert_array_equal(keep, np.concatenate([a[0].cpu().numpy(), b[0].cpu().numpy()]))
        np.testing.assert_array_equal(whole[1].cpu().numpy(),
                                      np.concatenate([a[1].cpu().numpy(), b[1].cpu().numpy()]))


# ---------------------------------------------------------------- compaction --
SCAN_TILE = 4096 * 256  # elements per tile of k_compact_scan (256 block counts of 4,096 elements)


def _masks(n, rng):
    """name -> uint8 mask; kept bytes take the values 1, 2, 128 and 255."""
    z = np.zeros(n, dtype=np.uint8)
    out = {"all": np.resize(np.array([1, 2, 128, 255], dtype=np.uint8), n), "none": z}
    if n:
        out["first"] = z.copy()
        out["first"][0] = 2
        out["last"] = z.copy()
        out["last"][-1] = 128
        for density in (0.5, 0.001):
            kept = rng.random(n) < density
            out[f"random-{density}"] = np.where(kept, rng.choice([1, 2, 128, 255], n), 0).astype(np.uint8)
    if n > SCAN_TILE:
        out["second-tile-first"] = z.copy()
        out["second-tile-first"][SCAN_TILE] = 255
    return out


@pytest.mark.parametrize("n", [0, 1, 4_095, 4_096, 4_097, 1_048_576, 1_048_577, 2_097_153])
def test_compact_matches_flatnonzero(device, n):
    """pdp_compact around one block (4,096 elements), around one scan tile
    (1,048,576) and with three scan tiles; the carry between tiles is nonzero
    from n = 1,048,577 on."""
    for name, mask in _masks(n, np.random.default_rng(n)).items():
        index, count = RU.compact(device, mask)
        RU.check_compaction(index, count, mask, what=(n, name))


def test_public_selection_compacts_the_mask(device):
    """PUBLIC through executor.select_and_noise with no ops: any nonzero mask
    byte keeps its partition; two scan tiles."""
    n = SCAN_TILE + 1
    mask = _masks(n, np.random.default_rng(3))["random-0.5"]
    index, n_kept = RU.public_select(device, mask)
    want = np.flatnonzero(mask)
    assert n_kept == len(want)
    np.testing.assert_array_equal(index, want)


# ------------------------------------------------------------- noisy metrics --
NOISES = [lap(2.0, 3.0), gau(3.0), lap(1.0, 1.0), gau(1.0), gau(2.0), lap(0.5, 1.0), gau(0.7), gau(5.0),
          lap(0.3, 2.0), gau(0.4), gau(1.5)]
KINDS = {"C": O.OP_COUNT, "S": O.OP_SUM, "P": O.OP_PRIVACY_ID_COUNT, "M": O.OP_MEAN, "V": O.OP_VARIANCE,
         "D": O.OP_VARIANCE, "T": O.OP_THRESHOLDED_PID}
N_COLS = {"C": 1, "S": 1, "P": 1, "M": 3, "V": 4, "D": 4, "T": 1}
N_MECH = {"C": 1, "S": 1, "P": 1, "M": 2, "V": 3, "D": 3, "T": 0}


def _ops(spec, drop=(), noises=NOISES):
    """One op per letter (D: a degenerate VARIANCE), consecutive output
    columns, a different mechanism for every draw; drop: (op, j) pairs whose
    out_col[j] is -1 (their columns stay reserved and must stay untouched)."""
    ops, col, mech = [], 0, 0
    for i, c in enumerate(spec):
        cols = [-1 if (i, j) in drop else col + j for j in range(N_COLS[c])]
        col += N_COLS[c]
        noise = tuple(noises[(mech + m) % len(noises)] for m in range(N_MECH[c]))
        mech += N_MECH[c]
        ops.append(X.MetricOpSpec(kind=KINDS[c], out_col=tuple(cols), noise=noise, middle=5.0 + i,
                                  min_value=1.5 if c == "D" else 0.0, sq_min_value=2.25 if c == "D" else 0.0,
                                  degenerate=int(c == "D")))
    return ops, col


def _draws(spec):
    return sum(max(N_MECH[c], 1) for c in spec)


def _accumulators(P, seed, sum_int):
    rng = np.random.default_rng(seed)
    return {
        "privacy_id_count": rng.integers(1, 40, P).astype(np.int64),
        "count": rng.integers(1, 80, P).astype(np.int64),
        "sum": rng.integers(-500, 500, P).astype(np.int64) if sum_int else rng.normal(0, 10, P),
        "normalized_sum": rng.normal(0, 10, P),
        "normalized_sum_sq": np.abs(rng.normal(0, 10, P)),
    }


# draws -> (op list, P): every G = 1 .. 32, lists with and without padding
# lanes, lists ending in MEAN and in VARIANCE, eight VARIANCE ops; P is the
# smallest round size past 524,288 / G, so the second grid-stride trip runs
DRAW_CASES = {1: ("C", 600_000), 2: ("M", 263_001), 3: ("V", 132_001), 4: ("SV", 132_001), 5: ("VM", 66_001),
              8: ("VVM", 66_001), 9: ("VVV", 33_001), 16: ("VVVVMSP", 33_001), 17: ("VVVVVSC", 20_000),
              24: ("VVVVVVVV", 20_000)}
# the large cases draw Gaussian noise (the oracle's cheaper sampler) but for one Laplace mechanism
BIG_NOISES = [gau(3.0), gau(1.0), lap(1.0, 1.0), gau(2.0), gau(0.7), gau(5.0), gau(0.4), gau(1.5)]


@pytest.mark.parametrize("draws", list(DRAW_CASES))
def test_noise_metrics_group_shapes(device, draws):
    """Every group size on both grid-stride trips, against the oracle."""
    spec, P = DRAW_CASES[draws]
    assert _draws(spec) == draws
    log2_g = int(np.ceil(np.log2(draws)))
    assert (P << log2_g) > 524_288 and len(spec) <= 8
    ops, n_cols = _ops(spec, noises=BIG_NOISES)
    acc = _accumulators(P, draws, sum_int=draws in (4, 17))
    offset = RU.BIG_OFFSET if draws in (1, 3, 5, 9, 17) else 0
    index = np.arange(P, dtype=np.int64)
    got = RU.noise_metrics(device, ops, index, P, P if draws % 2 else None, acc, seed=1000 + draws,
                           partition_offset=offset, n_cols=n_cols)
    want, terms = RU.oracle_metrics(ops, index, acc, None, seed=1000 + draws, partition_offset=offset, n_cols=n_cols)
    RU.compare_metrics(got, want, ops, terms, what=spec)


@pytest.mark.parametrize("offset", [0, RU.BIG_OFFSET], ids=["offset-0", "offset-2^33+5"])
@pytest.mark.parametrize("sum_int", [False, True], ids=["f64-sum", "i64-sum"])
@pytest.mark.parametrize("spec,drop", [("DVMSTC", ((1, 3), (2, 1), (5, 0))), ("VDTPM", ((0, 0), (1, 2), (3, 0)))],
                         ids=["degenerate-first", "degenerate-second-ends-in-mean"])
def test_noise_metrics_after_a_selective_selection(device, spec, drop, sum_int, offset):
    """Thresholding selection, compaction, then the metrics with n_kept = P and
    the real count on the device: a degenerate VARIANCE next to a normal one,
    THRESHOLDED_PID, out_col = -1 (those columns and every column past the
    device count keep their fill), fp64 and int64 sums."""
    P, mr, pre = 4_000, 3, 2
    acc = _accumulators(P, 7 + sum_int, sum_int)
    rc = acc["privacy_id_count"]
    sel = X.SelectionSpec(strategy=O.SELECT_LAPLACE, max_rows_per_privacy_id=mr, pre_threshold=pre,
                          noise=lap(0.4, 1.0), threshold=_median_threshold(rc, mr, pre), want_noised_count=True)
    keep_t, noised_t = RU.select(device, rc, sel, seed=11, partition_offset=offset)
    want_keep, want_nz = RU.oracle_select(rc, sel, seed=11, partition_offset=offset)
    index, count = RU.compact(device, keep_t)
    RU.check_compaction(index, count, want_keep)
    assert 0.2 * P <= count <= 0.8 * P
    index = np.where(index == RU.INDEX_FILL, 0, index)  # the tail is never read; keep it in range all the same
    ops, n_cols = _ops(spec, drop)
    got = RU.noise_metrics(device, ops, index, P, count, acc, seed=12, partition_offset=offset, noised=noised_t,
                           n_cols=n_cols)
    want, terms = RU.oracle_metrics(ops, index[:count], acc, want_nz, seed=12, partition_offset=offset, n_cols=n_cols)
    RU.compare_metrics(got[:, :count], want, ops, terms, what=spec)
    assert (got[:, count:] == RU.FILL).all()


@pytest.mark.parametrize("sum_int", [False, True], ids=["f64-sum", "i64-sum"])
def test_noise_metrics_accumulator_edges(device, sum_int):
    """Accumulators that stress round_to_multiple and the int -> double
    conversions, on a fine grid (Gaussian sigma 3: g = 2^-25) and on a coarse
    one (Laplace b = 2^41: g = 2): zeros, negative sums, counts of 0 and 1,
    magnitudes of 2^52, values exactly half a step off the grid (the tie rule:
    toward zero) and int64 sums above 2^53."""
    P = 256
    fine, coarse = gau(3.0), lap(1.0, 2.0 ** 41)
    assert fine.granularity == 2.0 ** -25 and coarse.granularity == 2.0
    acc = _accumulators(P, 3, sum_int)
    acc["count"][:8] = [0, 1, 1, 3, 5, 7, 2, 9]  # odd counts: half a step off the coarse grid
    acc["privacy_id_count"][:4] = [1, 1, 3, 0]
    if sum_int:
        edges = [0, -7, 1, 3, -1, -3, 5, 2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53) - 1, 2 ** 60 + 1, 2 ** 62 + 513,
                 -(2 ** 62) - 1, 2 ** 63 - 1, -(2 ** 63)]
        acc["sum"][:len(edges)] = edges
    else:
        half = [(k + 0.5) * fine.granularity for k in (-3, -2, -1, 0, 1, 2, 12345)]
        edges = [0.0, -0.0, -3.5, 2.0 ** 52, -(2.0 ** 52), 2.0 ** 52 + 1, 1.0, 3.0, -1.0, -3.0] + half
        acc["sum"][:len(edges)] = edges
    halves = [(k + 0.5) * fine.granularity for k in (-2, -1, 0, 1, 7)] + [0.0, -1.0, 3.0, 2.0 ** 52]
    acc["normalized_sum"][:len(halves)] = halves
    acc["normalized_sum_sq"][:len(halves)] = [abs(h) for h in halves]
    # COUNT, the first SUM, PRIVACY_ID_COUNT and MEAN's count on the coarse grid, the rest on the fine one
    noises = [coarse, coarse, fine, coarse, coarse, fine, fine, fine, fine, fine]
    ops, n_cols = _ops("CSSPMCV", noises=noises)
    assert _draws("CSSPMCV") == len(noises)
    index = np.arange(P, dtype=np.int64)
    got = RU.noise_metrics(device, ops, index, P, None, acc, seed=99, partition_offset=RU.BIG_OFFSET, n_cols=n_cols)
    want, terms = RU.oracle_metrics(ops, index, acc, None, seed=99, partition_offset=RU.BIG_OFFSET, n_cols=n_cols)
    RU.compare_metrics(got, want, ops, terms, what="edges")


# ------------------------------------------------- add_noise and vector sums --
@pytest.mark.parametrize("noise", [lap(0.5, 2.0), gau(3.0)], ids=["laplace", "gaussian"])
@pytest.mark.parametrize("kind", ["f64", "i64"])
def test_add_noise_sizes_and_offsets(device, kind, noise):
    """k_add_noise's pair loop and odd tail at every parity of n and of the
    index offset, below and above 2^32; int64 inputs above 2^53."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 511, 512, 513):
        if kind == "i64":
            x = rng.integers(-1000, 1000, n).astype(np.int64)
            x[::5] = (2 ** 53 + 1 + 2 * rng.integers(0, 1 << 20, len(x[::5]))) * rng.choice([-1, 1], len(x[::5]))
        else:
            x = rng.normal(0, 100, n)
            x[::7] = (rng.integers(-50, 50, len(x[::7])) + 0.5) * noise.granularity
        for offset in (0, 1, 2 ** 32 - 1, 2 ** 33 + 1):
            got = RU.add_noise(device, x, noise, seed=0xABCDEF0123, index_offset=offset)
            want = O.add_noise(x, noise.as_dict(), 0xABCDEF0123, offset)
            np.testing.assert_array_equal(got, want, err_msg=f"n={n} offset={offset}")


def test_vector_sum_metrics_above_2_32(device):
    """partition_offset = 2^33 and d = 65: the stream index (offset + p) * d + j
    has a high word and a row takes a second trip over the 64 lanes."""
    from pipelinedp_amd import _native as N
    P, d, offset, seed = 40, 65, 1 << 33, 0x5EED
    rng = np.random.default_rng(1)
    vacc = rng.integers(-50, 51, (P, d)).astype(np.float64)
    index = np.array([0, 3, 4, 17, 38, 39], dtype=np.int64)
    for noise in (lap(0.5, 2.0), gau(3.0)):
        got = RU.vector_sum_metrics(device, vacc, index, norm_kind=N.NORM_LINF, max_norm=20.0, noise=noise,
                                    seed=seed, partition_offset=offset)
        gidx = ((offset + index)[:, None] * d + np.arange(d)[None, :]).ravel()
        assert gidx.min() >= 1 << 32
        clipped = np.clip(vacc[index], -20.0, 20.0).ravel()
        want = O.secure_add_noise(noise.as_dict(), clipped, seed, gidx, N.VECTOR_SUM_SLOT).reshape(len(index), d)
        np.testing.assert_array_equal(got, want)
