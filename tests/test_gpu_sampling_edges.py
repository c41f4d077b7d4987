"""The sampling path of every plan on constructed tables, by equality with the oracle (GPU).

Which pairs and rows survive bounding is decided by comparisons that random
tables never bring to their edge.  tests/sampling_edges_util.py constructs the
inputs that do (pair hashes exactly at the sieve's and the band's edges, keys
whose random part is all ones, pairs of one id tied in their retained hash
bits at rank l0, rows tied in their 32 hash bits at rank linf or
max_contributions) and every plan that samples runs them: GLOBAL, BUCKETED
with either merge and record width (key formats 1 and 2, tile-local where the
shape has more than 64 buckets), the tile-local level 1 in key formats 3-5,
the automatic plan (two-level merge where P > 2,097,152), half-size buckets,
and the sieve at each threshold with the band on and off, both level-1
workgroup shapes and both bucket sizes; the per-id fix-up, the bucket-launch
fix-up and an id over the per-wave row cap on the 8,192-id shape of
test_gpu_fixup_ids.py; the pair table with linf, max_contributions and the
radix select.  A plan that bound_plan reports infeasible for a shape is left
out for that shape; which plans remain is a constant of the shape, and every
test asserts the whole set (PLANS_*, _all_ran) and that each granted plan is
the algorithm, merge, record format and bucket size that was asked for.

Values are the local row indices (int64, SUM_INT, bounds [0, 2^40]), so a
partition's sum says which rows were kept.  Expected: the oracle's
accumulators at the plan's rand_shift, compared with
value_edges_util.assert_exactly_equal; the sieve's statistics must equal the
counts of ids short of l0 pairs below t and below the band's edge, derived
from the pair hashes alone.  No tolerance anywhere in this file.
"""
import numpy as np
import pytest

from oracle import columnar as O
from tests import sampling_edges_util as SU
from tests import value_edges_util as VU

pytestmark = pytest.mark.gpu

ROW_CAP = 4096  # kFixIdsRowCap
# name -> (algorithm, merge, key_format, bucket_threads)
KERNEL_PLANS = {"global": (1, 0, 0, 0), "bucketed-atomic-wide": (2, 1, 1, 0), "bucketed-ranges-wide": (2, 2, 1, 0),
                "bucketed-atomic-compact": (2, 1, 2, 0), "bucketed-ranges-compact": (2, 2, 2, 0),
                "tile-local-keys3": (2, 2, 3, 0), "tile-local-keys4": (2, 2, 4, 0), "tile-local-keys5": (2, 2, 5, 0),
                "auto": (0, 0, 0, 0), "half-size-buckets": (0, 0, 0, 512)}
# (tile-local-keys1 and -keys2 are the bucketed-ranges-wide and -compact entries: the plan goes tile-local by shape)
# The plans that bound_plan grants, constants of the shapes: u32 COMPACT records need super + bucket + partition
# bits <= 31 (the P = 5,000 and the 64-id-bucket shapes), PACKED bucket + partition bits <= 31
PLANS_ALL = frozenset(KERNEL_PLANS)
PLANS_PACKED = PLANS_ALL - {"bucketed-atomic-compact", "bucketed-ranges-compact"}
PLANS_WIDE = PLANS_PACKED - {"tile-local-keys3"}

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _spec(l0, linf, maxc=0):
    from pipelinedp_amd import executor as X
    return X.BoundingSpec(l0=l0, linf=linf, value_kind=O.VALUE_I64, flags=SU.FLAGS, min_value=0, max_value=SU.VALUE_HI,
                          middle=0.0, max_contributions=maxc)


def _want(key, t, l0, linf, rand_shift, maxc=0):
    return _cached(("want", key, l0, linf, rand_shift, maxc),
                   lambda: SU.oracle_bound(t, l0=l0, linf=linf, rand_shift=rand_shift, max_contributions=maxc))


def _equal(got, want, what):
    try:
        VU.assert_exactly_equal(got, want)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


def feasible_kernel_plans(n, U, P, l0, linf, names=KERNEL_PLANS):
    """{name: plan} of the plans that bound_plan grants for this shape, each
    checked to be the algorithm, merge, record format and bucket size asked for."""
    from pipelinedp_amd import _native as N
    from pipelinedp_amd import executor as X
    out = {}
    for name in names:
        algorithm, merge, keys, bt = KERNEL_PLANS[name]
        try:
            plan = X.bound_plan(n, U, P, _spec(l0, linf), algorithm, merge, keys, bucket_threads=bt)
        except N.NativeLibraryError:
            continue  # infeasible for this shape (the tests pin the set of names that remain)
        if bt and plan.bucket_threads != bt:
            continue
        assert plan.algorithm == (algorithm or 2) and (merge == 0 or plan.merge == merge), (name, plan.algorithm)
        assert keys == 0 or plan.key_format == keys, (name, plan.key_format)
        out[name] = plan
    return out


def feasible_sieve_shapes(n, U, P, l0, linf, sieves, shapes, key_format=0):
    """[((sieve, band asked, threads, bucket threads), plan)] that bound_plan grants."""
    from pipelinedp_amd import executor as X
    out = []
    for sieve in sieves:
        for band, threads, bt in shapes:
            plan = X.bound_plan(n, U, P, _spec(l0, linf), key_format=key_format, sieve=sieve, sieve_band=band,
                                sieve_threads=threads, bucket_threads=bt)
            if plan.sieve != sieve or plan.sieve_threads != threads or (bt and plan.bucket_threads != bt):
                continue  # infeasible for this shape
            assert key_format == 0 or plan.key_format == key_format, plan.key_format
            out.append(((sieve, band, threads, bt), plan))
    return out


def _kernel_plans(device, key, t, l0, linf, expect):
    """Runs the table through every feasible plan, which must be exactly
    `expect` (a constant of the shape); returns {name: plan}."""
    from tests.test_gpu_kernels import _run_gpu
    plans = feasible_kernel_plans(len(t.pid), t.U, t.P, l0, linf)
    assert set(plans) == set(expect), (sorted(plans), sorted(expect))
    spec = _spec(l0, linf)
    for name, plan in plans.items():
        algorithm, merge, keys, bt = KERNEL_PLANS[name]
        got = _run_gpu(device, t.pid, t.pk, t.val, t.U, t.P, spec, t.seed, allowed=t.allowed, row_offset=t.row_offset,
                       algorithm=algorithm, merge=merge, key_format=keys, bucket_threads=bt)
        _equal(got, _want(key, t, l0, linf, plan.rand_shift), name)
    return plans


ALL_SHAPES = ((0, 1024, 0), (-1, 1024, 0), (0, 512, 0), (-1, 512, 0), (0, 1024, 512), (-1, 512, 512))


def _all_ran(sieves, shapes, band_fits=True):
    """What _sieve_plans returns when every shape is granted (the band up to t = 1/4)."""
    return sorted((s, 2 * s if band == 0 and s <= 16384 and band_fits else 0, th, bt or 1024)
                  for s in sieves for band, th, bt in shapes)


def _sieve_plans(device, key, t, l0, linf, sieves, fix_ids=None, shapes=ALL_SHAPES, key_format=0):
    """The sieve at every threshold x (band, level-1 threads, bucket threads);
    the statistics must name exactly the ids that the hashes say are short of
    l0 pairs.  Returns the (sieve, planned band, threads, planned bucket threads) that ran."""
    from pipelinedp_amd import executor as X
    from tests.test_gpu_sieve import _run
    spec, n, ran = _spec(l0, linf), len(t.pid), []
    for (sieve, band, threads, bt), plan in feasible_sieve_shapes(n, t.U, t.P, l0, linf, sieves, shapes, key_format):
        short1, short2 = _cached(("short", key, l0, sieve), lambda: SU.short_ids(t, l0, sieve))
        # (the band is planned up to t = 1/4, where its queues fit the level-1 LDS)
        assert plan.band in (0, 2 * sieve) and (plan.band == 0 or (band == 0 and sieve <= 16384)), plan.band
        assert (plan.sieve << 16) % SU.grain(plan.rand_shift) == 0 and (plan.band << 16) % SU.grain(
            plan.rand_shift) == 0
        assert fix_ids is None or plan.fix_ids == fix_ids, plan.fix_ids
        ws = X.BoundWorkspace()
        got = _run(device, t.pid, t.pk, t.val, t.U, t.P, spec, t.seed, sieve, allowed=t.allowed, key_format=key_format,
                   row_offset=t.row_offset, band=band, workspace=ws, threads=threads, bucket_threads=bt)
        st = ws.stats()
        what = f"sieve={sieve} band={band} threads={threads} bucket_threads={bt} keys={key_format}"
        print(what, "stats", st, "expected", len(short1), len(short2))
        assert st["unresolved_ids"] == len(short1), (what, st, len(short1))
        if plan.band:
            assert st["unresolved2_ids"] == len(short2), (what, st, len(short2))
        _equal(got, _want(key, t, l0, linf, plan.rand_shift), what)
        ran.append((sieve, plan.band, threads, plan.bucket_threads))
    # and the unsieved run of the same shape
    plan = X.bound_plan(n, t.U, t.P, spec, key_format=key_format, sieve=-1)
    assert plan.sieve == 0
    got = _run(device, t.pid, t.pk, t.val, t.U, t.P, spec, t.seed, -1, allowed=t.allowed, key_format=key_format,
               row_offset=t.row_offset)
    _equal(got, _want(key, t, l0, linf, plan.rand_shift), "unsieved")
    return ran


# ------------------------------------------------------ 1. threshold table --
def _threshold_large():
    return _cached("threshold-large", lambda: SU.threshold_table(SU.SEED, **SU.THRESHOLD_LARGE))


@pytest.mark.parametrize("l0", SU.THRESHOLD_L0S)
def test_hashes_at_the_sieve_and_band_edges(device, l0):
    """>= 32 ids per edge hash and l0 whose l0-th smallest pair hashes to
    exactly t32 - 1, t32, band_t32 - 1 or band_t32 (U = 299,008, P = 2^22,
    two-level merge)."""
    t = _threshold_large()
    n = {}
    for r in t.planted:
        n[(r["T"], r["l0"])] = n.get((r["T"], r["l0"]), 0) + 1
    assert min(n[(T, l0)] for s in SU.SIEVES for T in SU.edge_hashes(s)) >= 32
    ran = _sieve_plans(device, "threshold-large", t, l0, 2, SU.SIEVES)
    # every sieve x band on and off x both level-1 workgroups x both bucket sizes ran
    assert sorted(ran) == _all_ran(SU.SIEVES, ALL_SHAPES), ran
    plans = _kernel_plans(device, "threshold-large", t, l0, 2, PLANS_WIDE)
    assert plans["auto"].merge == 2 and plans["auto"].n_ranges <= 256 and plans["half-size-buckets"].bucket_threads == 512


@pytest.fixture
def _small_buckets(monkeypatch):
    monkeypatch.setenv("PIPELINEDP_AMD_TEST_HOOKS", "1")
    monkeypatch.setenv("PIPELINEDP_AMD_BUCKET_BITS", "6")


@pytest.mark.parametrize("fixup", ["per-id", "bucket-launch", "over-row-cap"])
@pytest.mark.parametrize("l0", SU.THRESHOLD_L0S)
def test_edge_hashes_through_the_fixups(device, _small_buckets, l0, fixup):
    """The same edges on 8,192 ids in 128 buckets of 64 (>= 3 ids per edge
    hash): an id whose l0-th pair sits at t32 is finished from the band, one
    at band_t32 from the rescan -- by its own wave (linf = 1), by the bucket
    launches (linf = 0), and with two planted ids over the per-wave row cap."""
    key = ("threshold-hooked", l0)
    t = _cached(key, lambda: SU.threshold_table(SU.SEED + l0, l0s=(l0,), **SU.THRESHOLD_HOOKED))
    for T in {T for s in SU.SIEVES for T in SU.edge_hashes(s)}:
        assert sum(r["T"] == T for r in t.planted) >= 3, T
    linf = 0 if fixup == "bucket-launch" else 1
    shapes = ((0, 1024, 0), (-1, 1024, 0), (0, 512, 0), (0, 1024, 512))
    if fixup == "over-row-cap":
        key = ("threshold-hooked-heavy", l0)
        heavy = [next(r["pid"] for r in t.planted if r["T"] == T) for T in (6000 << 16, 12000 << 16)]
        t = _cached(key, lambda: SU.with_heavy_ids(t, heavy, ROW_CAP + 1500))
        SU.check_threshold(t)
        shapes = shapes[:2]
    ran = _sieve_plans(device, key, t, l0, linf, SU.SIEVES, fix_ids=0 if fixup == "bucket-launch" else 1,
                       shapes=shapes)
    assert sorted(ran) == _all_ran(SU.SIEVES, shapes), ran  # the band on (12000, 32768) and off, every sieve


# ------------------------------------------------------- 2. all-ones table --
@pytest.mark.parametrize("shape", sorted(SU.ALL_ONES))
def test_keys_whose_random_part_is_all_ones(device, shape):
    """Pair hashes 0xFFFFFFFF and 0xFFFFFFFE (rand_shift > 32: the two top
    grains) as the last kept, the first dropped and a non-public pair; the
    tie after the cleared bit; rand_shift below, at and above 32."""
    from pipelinedp_amd import executor as X
    a = SU.ALL_ONES[shape]
    key = ("all-ones", shape)
    t = _cached(key, lambda: SU.all_ones_table(SU.SEED, a["U"], a["P"], a["rand_shift"], a["l0"], both=a["both"]))
    plan = X.bound_plan(len(t.pid), t.U, t.P, _spec(a["l0"], a["linf"]))
    assert plan.algorithm == 2 and plan.rand_shift == a["rand_shift"], plan.rand_shift
    plans = _kernel_plans(device, key, t, a["l0"], a["linf"], PLANS_PACKED if a["rand_shift"] < 32 else PLANS_WIDE)
    if a["rand_shift"] < 32:  # PACKED: u32 records from level 2 on, whose expand_key has no guard
        assert plans["auto"].key_format == 3, plans["auto"].key_format
    ran = _sieve_plans(device, key, t, a["l0"], a["linf"], (6000, 32768))
    if shape == "at32":  # 8,192 buckets: the level-1 LDS has room for neither the band nor the 512-thread shapes
        assert sorted(ran) == _all_ran((6000, 32768), ALL_SHAPES[:2], band_fits=False), ran
    else:
        assert sorted(ran) == _all_ran((6000, 32768), ALL_SHAPES), ran
    # (on the oracle's result, which every run above equalled: the planted non-public pairs are out)
    want = _want(key, t, a["l0"], a["linf"], a["rand_shift"])
    assert (want["privacy_id_count"][~t.allowed] == 0).all()


# ------------------------------------------------------- 3. pair-tie table --
@pytest.mark.parametrize("l0", SU.PAIR_TIE_L0S)
def test_pairs_tied_in_their_retained_hash_bits(device, l0):
    """rand_shift > 32 (P = 1e7): >= 32 ids with a tie group straddling rank
    l0, below the threshold, inside the band and above it; key formats 4, 5."""
    from pipelinedp_amd import executor as X
    a = SU.PAIR_TIE
    spec = _spec(l0, 2)
    auto = X.bound_plan(a["n_fill"], a["U"], a["P"], spec)
    assert auto.rand_shift > 32 and auto.key_format in (4, 5)
    key = ("pair-tie", l0)
    t = _cached(key, lambda: SU.pair_tie_table(SU.SEED, rand_shift=auto.rand_shift, l0=l0, **a))
    assert len(t.planted) >= 32 and X.bound_plan(len(t.pid), t.U, t.P, spec).rand_shift == auto.rand_shift
    assert (auto.sieve << 16) % SU.grain(auto.rand_shift) == 0 and (auto.band << 16) % SU.grain(auto.rand_shift) == 0
    plans = _kernel_plans(device, key, t, l0, 2, PLANS_WIDE)
    assert plans["tile-local-keys4"].rand_shift == plans["tile-local-keys5"].rand_shift == auto.rand_shift
    shapes = ((0, 1024, 0), (-1, 1024, 0), (0, 512, 0))
    for keys in (4, 5):  # the sieve on and off in both record formats
        ran = _sieve_plans(device, key, t, l0, 2, SU.PAIR_TIE_SIEVES, shapes=shapes, key_format=keys)
        assert sorted(ran) == _all_ran(SU.PAIR_TIE_SIEVES, shapes), (keys, ran)


# -------------------------------------------------------- 4. row-tie table --
def _row_table(cap, offset, per_pid):
    a = SU.ROW_TIE
    return _cached(("row-tie", cap, offset, per_pid),
                   lambda: SU.row_tie_table(SU.SEED, a["U"], a["P"], a["n"], cap, offset, per_pid=per_pid,
                                            min_ties=a["min_ties"]))


@pytest.mark.parametrize("offset", [0, SU.BIG_OFFSET])
@pytest.mark.parametrize("linf", [1, 2, 4])
def test_rows_tied_in_their_hash_bits(device, linf, offset):
    """Every pair of rows equal in their 32 hash bits among 2^19 consecutive
    rows, straddling rank linf of a pair: the lower row index is kept (the
    partition's sum says which)."""
    t = _row_table(linf, offset, False)
    key = ("row-tie", linf, offset)
    assert len(t.planted) >= 4
    plans = _kernel_plans(device, key, t, 1, linf, PLANS_ALL)
    shapes = ((0, 1024, 0), (-1, 512, 0), (0, 1024, 512))
    ran = _sieve_plans(device, key, t, 1, linf, (6000,), shapes=shapes)
    assert sorted(ran) == _all_ran((6000,), shapes), ran
    want = _want(key, t, 1, linf, plans["auto"].rand_shift)
    # (on the oracle's result, which every run above equalled)
    for r in t.planted:  # the kept row's index is in the sum
        others = sum(r["smaller"])
        assert want["sum"][r["pk"]] >= r["keep"] + others and want["count"][r["pk"]] >= linf


@pytest.mark.parametrize("mode,cap,offset", [("linf", 1, 0), ("linf", 2, SU.BIG_OFFSET), ("linf", 4, 0),
                                             ("linf", 300, SU.BIG_OFFSET), ("maxc", 1, 0), ("maxc", 3, SU.BIG_OFFSET),
                                             ("maxc", 300, 0)])
def test_rows_tied_in_the_pair_table(device, mode, cap, offset):
    """The same through pdp_pairs.hip: LinfSampler (l0 = 0) and
    SamplingPerPrivacyIdContributionBounder, by sketch (caps <= 256) and by
    radix select (300)."""
    from pipelinedp_amd import executor as X
    from tests.test_gpu_pairs import _gpu
    per_pid = mode == "maxc"
    t = _row_table(cap, offset, per_pid)
    assert len(t.planted) >= 4
    spec = _spec(0, 0 if per_pid else cap, cap if per_pid else 0)
    assert X.bound_plan(len(t.pid), t.U, t.P, spec).algorithm == 3  # PDP_ALGO_PAIR_TABLE
    got = _gpu(device, t.pid, t.pk, t.val, t.U, t.P, spec, seed=t.seed, row_offset=offset)
    want = _want(("row-tie-pairs", cap, offset, per_pid), t, 0, spec.linf, O.pk_bits(t.P), spec.max_contributions)
    VU.assert_exactly_equal(got, want)


# ------------------------------------------ the plan at the workgroup's LDS --
@pytest.mark.parametrize("l0,linf", [(3, 1), (1, 2), (1, 6)])
@pytest.mark.parametrize("plan", ["bucketed-atomic-wide", "bucketed-ranges-wide", "auto", "half-size-buckets"])
def test_bucket_kernel_launches_at_the_lds_limit(device, plan, l0, linf):
    """Bounds whose sketches fill kLdsBudget with many small ids: with the
    pid hashes, the wave queues and the kernel's static LDS the bucket kernel
    came to 163,844 bytes (l0 = 3, linf = 1, atomic merge) and more of a
    163,840-byte workgroup.  The plan must fit, launch and equal the oracle."""
    key = ("lds-limit", l0, linf)
    U, P, n = 8192, 257, 60_000
    rng = np.random.default_rng(l0 * 10 + linf)

    def make():
        pid, pk = rng.integers(0, U, n, dtype=np.int64), rng.integers(0, P, n, dtype=np.int64)
        return SU.Table(pid, pk, np.arange(n, dtype=np.int64), U, P, SU.SEED, [])
    t = _cached(key, make)
    plans = feasible_kernel_plans(n, U, P, l0, linf, names=[plan])
    assert plan in plans and plans[plan].lds_bytes + 64 <= 160 * 1024, plans
    assert plans[plan].bucket_bits >= 9  # (the sketches alone would allow up to 11)
    from tests.test_gpu_kernels import _run_gpu
    algorithm, merge, keys, bt = KERNEL_PLANS[plan]
    got = _run_gpu(device, t.pid, t.pk, t.val, U, P, _spec(l0, linf), t.seed, algorithm=algorithm, merge=merge,
                   key_format=keys, bucket_threads=bt)
    _equal(got, _want(key, t, l0, linf, plans[plan].rand_shift), plan)
