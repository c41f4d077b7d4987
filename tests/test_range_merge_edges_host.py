"""The range-merge edge tables, proven on the CPU (tests/range_merge_edges_util.py).

tests/test_gpu_range_merge_edges.py runs these tables through
csrc/pdp_bound_merge.hip and compares by equality; the device does not say
which work items it made.  So this file shows, without a GPU, that every shape
is what its name says: the plan it runs on (pinned field by field), the record
count of every (bucket, range) cell, and -- through plan_items() / fine_items(),
the work-item rules restated from the comments of the source -- how many items
a range gets, how large they are, where they are cut and on which side of the
direct threshold each falls.  The builder's expected accumulators are held to
oracle/columnar.py on the single-level shapes, so the two check each other.
"""
import numpy as np
import pytest

from oracle import columnar as O
from tests import range_merge_edges_util as RU
from tests import value_edges_util as VU

C, D, R = RU.C, RU.D, RU.R
SLOTS_MAX = RU.LDS_BUDGET // 20  # 6,348: the most pair records one bucket emits (below)


@pytest.fixture(scope="module", autouse=True)
def _forget_tables():
    yield
    RU.drop_tables()


def _plan(n, U, P, variant="f64", **kw):
    from pipelinedp_amd import executor as X
    return X.bound_plan(n, U, P, RU.spec_for(variant), **kw)


def test_constants_are_the_sources():
    k = RU.header_constants()
    assert (k["kRangeChunk"], k["kRangeDirect"], k["kSplitStageRows"]) == (C, D, R) == (8192, 256, 2048)
    assert k["kRangeBits"] == RU.RANGE_BITS and k["kSplitStageFan"] == RU.STAGE_FAN
    assert k["kCoarseRanges"] == RU.COARSE_RANGES and k["kMaxRanges"] == RU.MAX_RANGES
    assert k["kLdsBudget"] == RU.LDS_BUDGET
    assert k["kRangeThreads"] == RU.RANGE_THREADS
    assert k["kReduceThreads"] == k["kSplitThreads"] == RU.REDUCE_THREADS
    assert k["kSplitStageRows"] == 4 * k["kSplitThreads"]


def test_a_buckets_run_fits_one_item():
    """A bucket emits at most l0 * 2^bucket_bits records, and the planner keeps
    2^bucket_bits * per_pid_lds <= kLdsBudget with per_pid_lds = l0 * (8 + 4 +
    (linf > 0 ? 8 * linf : 24)) >= 20 * l0: so l0 * 2^bucket_bits <= kLdsBudget
    / 20 = 6,348 < kRangeChunk, and no bucket's run holds two cut positions."""
    assert SLOTS_MAX == 6348 < C
    from pipelinedp_amd import _native as N
    from pipelinedp_amd import executor as X
    seen = 0
    for l0 in (1, 2, 3, 4, 5, 8, 16, 64, 256):
        for linf in (0, 1, 2, 4):
            spec = X.BoundingSpec(l0=l0, linf=linf, value_kind=O.VALUE_F64, flags=RU.F_ALL, min_value=0.0,
                                  max_value=1.0, middle=0.5)
            for bt in (0, 512):
                try:
                    plan = X.bound_plan(1_000_000, 5_000_000, RU.P_SINGLE, spec, 2, 2, bucket_threads=bt)
                except N.NativeLibraryError:
                    continue  # no bucketed plan for these bounds
                assert l0 << plan.bucket_bits <= SLOTS_MAX, (l0, linf, bt, plan.bucket_bits)
                seen += 1
    assert seen >= 40
    # the pair the shapes use; (1, 1) is the case that comes closest: 4,096 <= 6,348
    assert RU.L0 << _plan(50_000, 1 << 20, RU.P_SINGLE).bucket_bits == 2048 == R


@pytest.mark.parametrize("variant", sorted(RU.VARIANTS))
@pytest.mark.parametrize("shape", list(RU.SHAPES))
def test_plan_of_every_shape(shape, variant):
    assert set(RU.PLANS) == set(RU.SHAPES)
    t, plan = RU.shape_table(shape, variant)
    g = t.geom
    U, P, _ = RU.SHAPES[shape]
    n_buckets, n_ranges, two_level, per_coarse = RU.PLANS[shape]
    RU.assert_plan(shape, t, plan)
    assert n_buckets == -(-U // 512)
    n_fine = -(-P // 2048)
    assert two_level == (n_fine > RU.MAX_RANGES) and g.n_fine == n_fine
    assert plan.range_group == C
    # the plan AUTO resolves to is the same one
    auto = _plan(len(t.pid), U, P, variant)
    assert (auto.algorithm, auto.merge, auto.bucket_bits, auto.n_buckets, auto.n_ranges, auto.key_format) == \
        (2, 2, plan.bucket_bits, plan.n_buckets, plan.n_ranges, plan.key_format)
    if shape[0] == "T":
        assert n_ranges <= RU.COARSE_RANGES and per_coarse <= RU.STAGE_FAN   # k_split_scatter_staged
    if shape[0] == "U":
        assert P < 1 << 32 and per_coarse > RU.STAGE_FAN                      # the plain k_split_scatter
    if two_level:  # the last coarse range: one fine range of one partition
        assert g.range_span(n_ranges - 1) == (P - 1, P) and g.n_fine - 1 == (P - 1) >> RU.RANGE_BITS


@pytest.mark.parametrize("variant", sorted(RU.VARIANTS))
@pytest.mark.parametrize("shape", list(RU.SHAPES))
def test_builder_keeps_its_word(shape, variant):
    t, _ = RU.shape_table(shape, variant)
    g = t.geom
    U, P, cells_of = RU.SHAPES[shape]
    cells = cells_of(g)
    # record count of every (bucket, range) cell
    want_runs = np.zeros((g.n_ranges, g.n_buckets), dtype=np.int64)
    for c in cells:
        want_runs[c.range, c.bucket] += c.n_pairs
    np.testing.assert_array_equal(t.run_lengths(), want_runs)
    assert t.run_lengths().sum(axis=0).max() <= g.pair_slots
    # pairs are distinct, an id holds at most l0 of them: nothing is sampled at l0, linf = 0
    code = t.pair_pid * P + t.pair_pk
    assert len(np.unique(code)) == len(code) == sum(c.n_pairs for c in cells)
    assert np.bincount(t.pair_pid).max() <= g.l0 == RU.L0
    assert t.pair_pid.min() >= 0 and t.pair_pid.max() < U and t.pair_pk.min() >= 0 and t.pair_pk.max() < P
    # rows: 1 to 3 per pair, every pair present, shuffled
    row_code, rows = np.unique(t.pid * P + t.pk, return_counts=True)
    np.testing.assert_array_equal(row_code, np.sort(code))
    assert rows.min() == 1 and rows.max() == 3 and len(set(rows.tolist())) == 3
    assert (np.diff(t.pid * P + t.pk) < 0).any()
    # exact in any order, and the clip has work on both sides
    if t.val is None:
        assert variant == "none"
    else:
        _, dense = np.unique(t.pk, return_inverse=True)
        assert VU.check_exact(dense, t.val, int(dense.max()) + 1, t.bounds) < 1 << 53
        f = t.val.astype(np.float64)
        assert (f < t.bounds.lo).any() and (f > t.bounds.hi).any()
    # a spread cell holds its span's first and last partition
    for c in cells:
        if c.placement[0] == "spread" and c.n_pairs >= 61:  # all of the cell's candidate partitions are dealt
            in_cell = t.pair_pk[(t.pair_pid >> g.bucket_bits == c.bucket) & (t.pair_pk >= c.placement[1]) &
                                (t.pair_pk < c.placement[2])]
            assert in_cell.min() == c.placement[1] and in_cell.max() == c.placement[2] - 1, c


@pytest.mark.parametrize("variant", sorted(RU.VARIANTS))
@pytest.mark.parametrize("shape", RU.SINGLE)
def test_expected_equals_the_oracle(shape, variant):
    t, plan = RU.shape_table(shape, variant)
    b = t.bounds
    U, P, _ = RU.SHAPES[shape]
    got = O.bound_and_reduce(t.pid, t.pk, t.val, n_privacy_ids=U, n_partitions=P, l0=RU.L0, linf=RU.LINF,
                             value_kind=t.value_kind, flags=t.flags, min_value=b.lo, max_value=b.hi, middle=b.mid,
                             min_sum=b.min_sum, max_sum=b.max_sum, seed=0x5EED + 4, row_offset=77,
                             rand_shift=plan.rand_shift)
    want = t.expected()
    VU.assert_exactly_equal(got, want)
    assert want["count"].sum() == len(t.pid) and want["privacy_id_count"].sum() == len(t.pair_pid)


# ---------------------------------------------------------------- the edges --
def _items(shape):
    t, _ = RU.shape_table(shape, "f64")
    by_range = {}
    for r, b0, b1, n in RU.plan_items(t.run_lengths()):
        by_range.setdefault(r, []).append((b0, b1, n))
    return t, by_range


def test_s1_sits_on_the_direct_switch():
    t, items = _items("S1-direct-switch")
    nb = t.geom.n_buckets
    assert items == {0: [(0, nb, D - 1)], 1: [(0, nb, D)], 3: [(0, nb, D + 1)]}  # range 2: no item
    # (255 goes to the device atomics, 256 and 257 through LDS)
    P = t.geom.P
    assert t.geom.range_span(3) == (P - 5, P) and {P - 5, P - 1} <= set(t.pair_pk.tolist())


def test_s2_totals_are_exact_multiples():
    t, items = _items("S2-exact-multiples")
    nb = t.geom.n_buckets
    totals = t.run_lengths().sum(axis=1)
    assert totals.tolist() == [C, 2 * C, C + 1, C - 1]
    assert [int(x) % C for x in totals] == [0, 0, 1, C - 1]
    # a multiple of C: the last cut is the sentinel, at the last populated bucket's end, not at n_buckets
    assert items[0] == [(0, 4, C)]
    assert items[1] == [(0, 8, C), (8, 12, C)]
    # C + 1: the cut lands on a bucket's last record (k * C == e); the tail item holds one record
    assert items[2] == [(0, 16, C), (16, nb, 1)]
    assert items[3] == [(0, nb, C - 1)]
    runs = t.run_lengths()
    assert runs[:, 21:].sum() == 0 and nb == 24  # trailing empty buckets
    assert set(runs[0, :4].tolist()) == {2048} and runs[2, 16] == 1


def test_s3_items_overshoot_the_chunk():
    t, items = _items("S3-overshoot")
    nb = t.geom.n_buckets
    assert set(t.run_lengths()[0, :10].tolist()) == {2047}
    assert C % 2047 != 0 and 4 * 2047 < C < 5 * 2047  # position C falls inside the fifth bucket
    assert items[0] == [(0, 5, 5 * 2047), (5, 9, 4 * 2047), (9, nb, 2047)]
    assert items[0][0][2] > C
    # range 1, nine such buckets: position 2C lies in the last, the third item is empty
    assert items[1] == [(0, 15, 5 * 2047), (15, 19, 4 * 2047), (19, nb, 0)]
    assert items[3] == [(0, nb, 3)]


def test_s4_is_one_hot_partition():
    t, items = _items("S4-hot-partition")
    hot = t.geom.range_span(1)[0] + 777
    assert (t.pair_pk == hot).sum() == 3 * C and ((t.pair_pk >> 11) == 1).sum() == 3 * C
    assert items[1] == [(0, 16, C), (16, 32, C), (32, 48, C)]  # every cut on a bucket's last record
    assert items[0] == [(0, t.geom.n_buckets, 10)]
    # the LDS counters of one partition take a whole item: pairs and rows fit a u32 by far
    assert np.bincount(t.pk)[hot] < 1 << 20


def test_s5_crosses_the_bucket_batches():
    t, items = _items("S5-batch-edges")
    g = t.geom
    runs = t.run_lengths()
    last = g.n_buckets - 1
    assert g.n_buckets == 1026 > RU.RANGE_THREADS + 1
    assert sorted(np.flatnonzero(runs.sum(axis=0)).tolist()) == [0, 511, 512, 1023, 1024, last]
    # k_range_plan: the second batch of 1,024 buckets starts with a carry, and the cut lies in it
    carry = int(runs[0, :RU.RANGE_THREADS].sum())
    assert 0 < carry < C <= carry + runs[0, 1024] and carry + runs[0, 1024] != C
    assert items[0] == [(0, 1025, carry + 2048), (1025, 1026, 2)]
    assert items[0][0][2] > C and items[0][1][2] < D
    # k_range_reduce: the first item takes three batches of 512 buckets, with records in each
    for lo in (0, 512, 1024):
        assert runs[0, lo:min(lo + RU.REDUCE_THREADS, 1025)].sum() > 0
    # one item whose records sit in buckets 511 | 512, on the LDS path
    assert items[1] == [(0, 1026, 2 * (2048 - 1500))] and items[1][0][2] >= D
    assert runs[1, 511] == runs[1, 512] == 548
    assert items[3] == [(0, 1026, 2)] and runs[3, last] == 2


def _fine_by_range(t):
    out = {}
    for f, a, n in RU.fine_items(t.fine_totals()):
        out.setdefault(f, []).append((a, n))
    return out


@pytest.mark.parametrize("shape,fines", [("T1-staged-fine-0-7-last", (0, 7)),
                                         ("U1-unstaged-fine-edges", (0, 255, 256, 511))])
def test_t1_fine_ranges(shape, fines):
    t, items = _items(shape)
    g = t.geom
    F = g.fine_per_coarse
    assert F - 1 == fines[-1]
    populated = np.flatnonzero(t.fine_totals()).tolist()
    assert populated == [5 * F + f for f in fines] + [g.n_fine - 1]
    assert g.n_fine - 1 == (g.n_ranges - 1) * F  # the last coarse range has one fine range; f0 + t < n_fine cuts F - 1
    assert g.fine_span(g.n_ranges - 1, 0) == (g.P - 1, g.P)
    assert sorted(items) == [5, g.n_ranges - 1] and all(len(v) == 1 for v in items.values())
    last = t.pair_pk == g.P - 1
    assert last.sum() == 305 and items[g.n_ranges - 1][0][2] == 305 >= D  # LDS path with plen = 1
    fine = _fine_by_range(t)
    assert all(len(v) == 1 and v[0][1] >= D for v in fine.values())


@pytest.mark.parametrize("shape", ["T2-staged-fine-totals", "U2-unstaged-fine-totals"])
def test_t2_fine_totals(shape):
    t, items = _items(shape)
    fine = _fine_by_range(t)
    assert [v for _, v in sorted(fine.items())] == [[(0, D - 1)], [(0, D)], [(0, C)], [(0, C), (C, 1)],
                                                     [(0, C), (C, C)]]
    assert len({f // t.geom.fine_per_coarse for f in fine}) == 1  # all in coarse range 3
    sizes = [n for _, _, n in items[3]]
    assert sizes == [C, C, C, C, D - 1 + D + 1] and list(items) == [3]
    # the coarse items hold 3, 2, 2, 1 and 1 fine ranges: rounds of the scatter with mixed and with single runs
    g = t.geom
    for k, (b0, b1, _) in enumerate(items[3]):
        sel = (t.pair_pid >> g.bucket_bits >= b0) & (t.pair_pid >> g.bucket_bits < b1)
        assert len(set((t.pair_pk[sel] >> RU.RANGE_BITS).tolist())) == (3, 2, 2, 1, 1)[k]


def test_t3_rounds_of_the_staged_scatter():
    t, items = _items("T3-staged-rounds")
    g = t.geom
    nb = g.n_buckets
    assert items == {10: [(0, nb, R)], 11: [(0, nb, R)], 12: [(0, nb, R + 1)], 13: [(0, nb, R + 1)]}
    fines = {r: set(((t.pair_pk[t.pair_pk >> g.range_bits == r] >> RU.RANGE_BITS) % g.fine_per_coarse).tolist())
             for r in items}
    assert fines == {10: {4}, 11: set(range(8)), 12: {7}, 13: set(range(8))}
    # an item's buckets are one batch, so a round is the item's first R records: R, then one more
    assert nb <= RU.REDUCE_THREADS and g.pair_slots == R


# --------------------------------------------------------- model invariants --
def _brute_items(runs, chunk):
    """plan_items from the records themselves: one list entry per record."""
    out = []
    for r, row in enumerate(runs):
        owner = [b for b, n in enumerate(row) for _ in range(int(n))]
        if not owner:
            continue
        K = -(-len(owner) // chunk)
        first, done = 0, 0
        for k in range(1, K + 1):
            if k * chunk <= len(owner):
                end_bucket = owner[k * chunk - 1] + 1
                upto = max(i for i, b in enumerate(owner) if b < end_bucket) + 1
            else:
                end_bucket, upto = len(row), len(owner)
            out.append((r, first, end_bucket, upto - done))
            first, done = end_bucket, upto
    return out


def test_model_invariants_on_random_run_tables():
    rng = np.random.default_rng(5)
    for trial in range(300):
        chunk = int(rng.choice([64, 100, 8192])) if trial % 3 else C
        slots = min(SLOTS_MAX, chunk - 1)  # a bucket's run fits one item
        n_ranges, n_buckets = int(rng.integers(1, 6)), int(rng.integers(1, 40))
        runs = rng.integers(0, slots + 1, (n_ranges, n_buckets))
        runs[rng.random(runs.shape) < 0.4] = 0
        if trial % 5 == 0:
            runs[0] = 0
            runs[0, : min(n_buckets, 4)] = chunk // 4  # exact multiples now and then
        items = RU.plan_items(runs, chunk)
        if chunk <= 100:
            assert items == _brute_items(runs, chunk)
        recs = int(runs.sum())
        live = int((runs.sum(axis=1) > 0).sum())
        assert len(items) + live <= recs // chunk + 2 * n_ranges + 1  # the planner's n_groups (sentinels included)
        for r in range(n_ranges):
            mine = [it for it in items if it[0] == r]
            total = int(runs[r].sum())
            assert len(mine) == -(-total // chunk)
            if not mine:
                continue
            assert mine[0][1] == 0 and sum(it[3] for it in mine) == total
            done = 0
            for k, (_, b0, b1, n) in enumerate(mine):
                assert n == runs[r, b0:b1].sum() and (k == 0 or b0 == mine[k - 1][2])
                done += n
                if k < len(mine) - 1:  # cut after the bucket holding position (k + 1) * chunk
                    assert (k + 1) * chunk <= done < (k + 1) * chunk + slots and n > 0
            assert runs[r, mine[-1][2]:].sum() == 0
        fine_totals = rng.integers(0, 3 * chunk, 17) * (rng.random(17) < 0.6)
        fine_totals[0] = chunk * int(rng.integers(0, 3))
        fitems = RU.fine_items(fine_totals, chunk)
        assert len(fitems) <= int(fine_totals.sum()) // chunk + len(fine_totals) + 1  # the planner's fine_items
        for f, total in enumerate(fine_totals):
            mine = [it for it in fitems if it[0] == f]
            assert [a for _, a, _ in mine] == list(range(0, int(total), chunk))
            assert sum(n for _, _, n in mine) == total and all(0 < n <= chunk for _, _, n in mine)
            assert all(n == chunk for _, _, n in mine[:-1])


@pytest.mark.parametrize("shape", list(RU.SHAPES))
def test_items_fit_the_planners_bounds(shape):
    t, plan = RU.shape_table(shape, "f64")
    g = t.geom
    runs = t.run_lengths()
    recs = g.n_buckets * g.pair_slots  # what plan_derived counts with: every slot of every bucket
    assert runs.sum() <= recs
    entries = len(RU.plan_items(runs)) + int((runs.sum(axis=1) > 0).sum())
    assert entries <= recs // C + 2 * g.n_ranges + 1
    if g.two_level:
        assert len(RU.fine_items(t.fine_totals())) <= recs // C + g.n_fine + 1
