"""The constructors of tests/sampling_edges_util.py and the oracle's sampling, on the CPU.

The inverses round-trip; every builder's planted records hold under the
oracle's hashes (the builders assert it themselves and raise when they find
fewer cases than their minimum: nothing here skips); and
oracle.columnar.bound_and_reduce equals plain_bound -- dicts, sorted() over
(masked hash, partition) and (row hash, row) tuples, Python ints -- on all four
kinds of table.  The wrong row tie-break (the higher row index wins) differs
from the oracle at every planted collision, so a kernel that took it could not
equal the oracle on these tables.
"""
import numpy as np
import pytest

from oracle import columnar as O
from tests import sampling_edges_util as SU

FIELDS = ("privacy_id_count", "count", "sum")


def _same(t, l0, linf, rand_shift, maxc=0):
    want = SU.plain_bound(t.pid, t.pk, t.val, P=t.P, l0=l0, linf=linf, seed=t.seed, rand_shift=rand_shift,
                          row_offset=t.row_offset, allowed=t.allowed, max_contributions=maxc)
    got = SU.oracle_bound(t, l0=l0, linf=linf, rand_shift=rand_shift, max_contributions=maxc)
    for k in FIELDS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    return got


def test_inverses_round_trip():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.integers(0, 1 << 32, 100_000, dtype=np.uint64),
                        np.array([0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 6000 << 16, 1 << 31], dtype=np.uint64)])
    np.testing.assert_array_equal(O.fmix32(SU.unfmix32(x)), x.astype(np.uint32))
    np.testing.assert_array_equal(SU.unfmix32(O.fmix32(x.astype(np.uint32))), x.astype(np.uint32))
    ids = rng.integers(0, 1 << 40, 1000)  # the high half of an id takes part in its hash word
    for T in (0xFFFFFFFF, 0xFFFFFFFE, 6000 << 16, (6000 << 16) - 1, 12000 << 16, 0):
        for seed in (SU.SEED, 0, (1 << 64) - 1):
            pk = SU.solve_pk(seed, ids, T)
            assert ((0 <= pk) & (pk < 1 << 32)).all()
            assert (O.pair_hash(seed, ids, pk) == np.uint32(T)).all()
            # the solution is the only one: its neighbours give other hashes
            assert (O.pair_hash(seed, ids, (pk + 1) % (1 << 32)) != np.uint32(T)).all()


def test_solutions_below_P_are_as_many_as_expected():
    """U P / 2^32 = 293 ids per target hash at U = 300,000, P = 2^22."""
    ids = np.arange(300_000)
    for T in (0xFFFFFFFF, 0xFFFFFFFE, 6000 << 16, (6000 << 16) - 1, 12000 << 16):
        assert 220 <= int((SU.solve_pk(SU.SEED, ids, T) < 1 << 22).sum()) <= 370


def test_no_two_hashes_of_one_id_tie_without_truncation():
    """pair_hash is a bijection of the partition's low word: no tie groups at
    32 retained bits, ordinary ones at 29 and 24."""
    assert SU.tie_groups(SU.SEED, 5, 1 << 20, 32) == []
    n29, n24 = (len(SU.tie_groups(SU.SEED, 5, 1 << 20, b)) for b in (29, 24))
    assert 600 < n29 < 1200 and 25_000 < n24 < 40_000, (n29, n24)
    for rs in (20, 31, 32):  # rand_shift <= 32: distinct priorities among one id's pairs
        pr = O.pair_priority(SU.SEED, np.full(1 << 18, 5), np.arange(1 << 18), rs) >> np.uint64(rs)
        if rs < 32:
            assert len(np.unique(pr)) == 1 << 18
        else:  # only the all-ones hash may meet its neighbour
            assert len(np.unique(pr)) >= (1 << 18) - 1


@pytest.mark.parametrize("rand_shift", [20, 31, 32, 33, 36, 40])
def test_pair_priority_applies_the_all_ones_rule_exactly_there(rand_shift):
    g = SU.grain(rand_shift)
    ids = np.arange(40_000)
    T = np.array([0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF - g + 1, 0xFFFFFFFF - g, 0xFFFFFFFF - 2 * g + 1, 0x7FFFFFFF, 12345],
                 dtype=np.int64)
    low = np.uint64((1 << rand_shift) - 1)
    for t in T.tolist():
        sol = SU.solve_pk(SU.SEED, ids, t)
        fits = sol < 1 << min(rand_shift, 31)  # partitions that fit below rand_shift
        u, pk = ids[fits], sol[fits]
        assert len(pk)
        x = O.pair_priority(SU.SEED, u, pk, rand_shift)
        raw = ((np.uint64(t) << np.uint64(32)) & ~low) | pk.astype(np.uint64)
        fires = (raw | low) == O.EMPTY
        assert fires.all() == fires.any() == (rand_shift >= 32 and t > 0xFFFFFFFF - g)
        np.testing.assert_array_equal(x, np.where(fires, raw & ~np.uint64(1 << rand_shift), raw))
        assert ((x | low) != O.EMPTY).all()  # never a dead or an empty key
        assert [int(v) >> rand_shift for v in x.tolist()] == [SU.masked_hash(t, rand_shift)] * len(pk)


def test_threshold_tables_and_plain_bound():
    t = SU.threshold_table(SU.SEED, **SU.THRESHOLD_LARGE)
    by_edge = {}
    for r in t.planted:
        by_edge[(r["T"], r["l0"])] = by_edge.get((r["T"], r["l0"]), 0) + 1
    edges = {T for s in SU.SIEVES for T in SU.edge_hashes(s)}
    assert set(by_edge) == {(T, l0) for T in edges for l0 in SU.THRESHOLD_L0S} and min(by_edge.values()) >= 32
    for l0, rs in ((1, 22), (2, 33), (4, 32)):
        _same(t, l0, 2, rs)
    for l0 in SU.THRESHOLD_L0S:
        h = SU.threshold_table(SU.SEED + l0, l0s=(l0,), **SU.THRESHOLD_HOOKED)
        n = {T: sum(r["T"] == T for r in h.planted) for T in edges}
        assert min(n.values()) >= 3, n
        _same(h, l0, 1, 28)
        # the planted ids are short of l0 pairs exactly where their edge says
        for sieve in SU.SIEVES:
            s1, s2 = (set(x.tolist()) for x in SU.short_ids(h, l0, sieve))
            t32, b32 = sieve << 16, min(2 * sieve, 32768) << 16
            for r in h.planted:
                assert (r["pid"] in s1) == (r["T"] >= t32) and (r["pid"] in s2) == (r["T"] >= b32), (r, sieve)


@pytest.mark.parametrize("shape", sorted(SU.ALL_ONES))
def test_all_ones_tables_and_plain_bound(shape):
    a = SU.ALL_ONES[shape]
    t = SU.all_ones_table(SU.SEED, a["U"], a["P"], a["rand_shift"], a["l0"], both=a["both"])
    kinds = {r["kind"] for r in t.planted}
    assert {"exact", "over", "dead"} <= kinds and ("short" in kinds) == (a["l0"] > 1)
    assert ("tie" in kinds) == (a["rand_shift"] > 32) and ("both" in kinds) == (a["rand_shift"] == 32)
    got = _same(t, a["l0"], a["linf"], a["rand_shift"])
    _same(t, a["l0"], a["linf"], SU.O.pk_bits(a["P"]))  # the GLOBAL plan's keys: no all-ones part
    for r in t.planted:  # dead pairs stay out; a tie's loser is dropped
        if r["kind"] == "dead":
            assert got["privacy_id_count"][r["pk"]] == 0
    assert (got["privacy_id_count"][~t.allowed] == 0).all()


@pytest.mark.parametrize("l0,rand_shift", [(1, 36), (3, 34), (4, 34)])
def test_pair_tie_tables_and_plain_bound(l0, rand_shift):
    t = SU.pair_tie_table(SU.SEED, rand_shift=rand_shift, l0=l0, **SU.PAIR_TIE)
    assert len(t.planted) >= 32 and {r["zone"] for r in t.planted} == {"candidate", "band", "above"}
    assert l0 == 1 or any(r["winners"] == 2 for r in t.planted)
    for s in SU.PAIR_TIE_SIEVES + (32768,):
        assert (s << 16) % SU.grain(rand_shift) == 0 and (min(2 * s, 32768) << 16) % SU.grain(rand_shift) == 0
    _same(t, l0, 2, rand_shift)
    _same(t, l0, 2, 24)  # the GLOBAL plan's keys: 32 retained bits, no ties


@pytest.mark.parametrize("cap,offset,per_pid", [(1, 0, False), (2, SU.BIG_OFFSET, False), (4, 0, False),
                                                (1, SU.BIG_OFFSET, True), (3, 0, True)])
def test_row_tie_tables_and_plain_bound(cap, offset, per_pid):
    a = dict(SU.ROW_TIE, n=1 << 18, min_ties=4)  # (2^18 rows hold ~8 collisions)
    t = SU.row_tie_table(SU.SEED, a["U"], a["P"], a["n"], cap, offset, per_pid=per_pid, min_ties=a["min_ties"])
    assert len(t.planted) >= 4
    kw = dict(l0=0, linf=0, maxc=cap) if per_pid else dict(l0=1, linf=cap)
    got = _same(t, kw["l0"], kw["linf"], 24, kw.get("maxc", 0))
    wrong = SU.plain_bound(t.pid, t.pk, t.val, P=t.P, l0=kw["l0"], linf=kw["linf"], seed=t.seed, rand_shift=24,
                           row_offset=offset, max_contributions=kw.get("maxc", 0), higher_row_wins=True)
    assert wrong["count"].sum() == got["count"].sum()
    if not per_pid:  # (a per-id collision's two rows lie in different partitions)
        np.testing.assert_array_equal(wrong["count"], got["count"])
    assert int((wrong["sum"] - got["sum"]).sum()) == sum(r["drop"] - r["keep"] for r in t.planted)
    if not per_pid:  # each planted pair's partition says which row was kept
        for r in t.planted:
            assert wrong["sum"][r["pk"]] - got["sum"][r["pk"]] >= r["drop"] - r["keep"] > 0


def test_bucket_plan_fits_a_workgroups_lds():
    """The bucket kernel's whole LDS -- the dynamic request (sketches, pid
    hashes, wave queues, range scratch) plus its static LDS (kBucketStaticLds
    = 64 bytes) -- fits the 163,840 bytes a workgroup can have, for every small
    bound, both merges, every record format and both bucket sizes: 4,096 ids
    of 28 bytes (l0 = 1, linf = 2) and 2,048 of 60 (l0 = 3, linf = 1: exactly
    163,840 dynamic bytes under the atomic merge) were planned over it and
    failed at launch (test_gpu_sampling_edges.py::
    test_hashes_at_the_sieve_and_band_edges[1])."""
    from pipelinedp_amd import _native as N
    from pipelinedp_amd import executor as X
    seen = 0
    for U, P in ((300_000, 5000), (300_000, 1 << 22), (300_000, 10_000_000), (2048, 257), (8192, 257)):
        for l0 in range(1, 9):
            for linf in range(0, 9):
                spec = X.BoundingSpec(l0=l0, linf=linf, value_kind=O.VALUE_I64, flags=SU.FLAGS, min_value=0,
                                      max_value=SU.VALUE_HI, middle=0.0)
                for merge in (0, 1, 2):
                    for keys in range(6):
                        for bt in (0, 512):
                            try:
                                plan = X.bound_plan(200_000, U, P, spec, 2, merge, keys, bucket_threads=bt)
                            except N.NativeLibraryError:
                                continue  # this record format does not fit the shape
                            seen += 1
                            assert plan.algorithm == 2 and plan.lds_bytes + 64 <= 160 * 1024, \
                                (U, P, l0, linf, merge, keys, bt, plan.lds_bytes)
    assert seen > 5000
    spec = X.BoundingSpec(l0=3, linf=1, value_kind=O.VALUE_I64, flags=SU.FLAGS, min_value=0, max_value=SU.VALUE_HI)
    assert X.bound_plan(200_000, 8192, 257, spec, 2, 1, 1).bucket_bits == 10  # 2,048 ids came to the limit + 4 bytes
    spec = X.BoundingSpec(l0=2, linf=1, value_kind=O.VALUE_I64, flags=SU.FLAGS, min_value=0, max_value=SU.VALUE_HI)
    assert X.bound_plan(200_000, 300_000, 5000, spec).bucket_bits == 11  # plans that fitted keep their buckets
