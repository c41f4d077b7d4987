"""Constructed inputs that pin which pairs and rows survive contribution bounding.

Random tables cannot reach the places where the comparisons of the sampling
path (pdp_bound.hip, pdp_bound_merge.hip, pdp_pairs.hip, the key helpers of
pdp_internal.h) can be off by one: a pair hash exactly at the sieve's or the
band's edge, a pair key whose random part is all ones (the sketches' empty and
the bucket kernel's dead marker), two pairs of one privacy id equal in their
retained hash bits at the l0-th rank, two rows equal in their 32 hash bits at
the linf-th (or max_contributions-th) rank.  All of them can be constructed:
fmix32 and the odd multipliers of pair_hash are invertible, so for a seed, a
privacy id and a wanted hash T exactly one partition low word gives T
(solve_pk); ties are found by enumeration (tie_groups, row_ties).

Shared by tests/test_sampling_edges_host.py (CPU) and
tests/test_gpu_sampling_edges.py (GPU).  Every builder returns a Table whose
`planted` records say which id holds which constructed pair or row at which
rank, and asserts with the oracle's hashes that they do (check_*): a builder
that finds fewer cases than its minimum raises, it never skips.  Values are
int64, equal to the local row index, with bounds [0, 2^40] and SUM_INT: every
sum is exact and says *which* rows were kept.

plain_bound() restates bounding in dicts, sorted() over tuples and Python
ints; it shares nothing with oracle.columnar.bound_and_reduce but the hash
functions.
"""
import dataclasses

import numpy as np

from oracle import columnar as O

SEED = 0xA5A5_0000_1111
TILE_ROWS = 65536
VALUE_HI = 1 << 40
FLAGS = O.ACC_SUM | O.SUM_INT
_M32 = 1 << 32
_C1, _C2, _MPK, _MPID = 0x85EBCA6B, 0xC2B2AE35, 0xC2B2AE3D, 0x9E3779B1
_I1, _I2, _IPK, _IPID = (pow(c, -1, _M32) for c in (_C1, _C2, _MPK, _MPID))
_ROW_MUL = 0xD6E8FEB86659FD93

# shapes (constants: the counts in DESIGN.md section 4 are of these)
THRESHOLD_LARGE = dict(U=299_008, P=1 << 22, n_fill=150_000, per_edge=32)   # 73 * 4,096 ids, ~2.5 tiles
THRESHOLD_HOOKED = dict(U=8192, P=1 << 22, n_fill=190_000, per_edge=3)      # bucket-bits hook: 128 buckets of 64
SIEVES = (6000, 16384, 32768)
THRESHOLD_L0S = (1, 2, 4)
PAIR_TIE = dict(U=300_000, P=10_000_000, n_fill=140_000, n_ids=32, scan=1 << 18)
PAIR_TIE_L0S = (1, 3, 4)
PAIR_TIE_SIEVES = (6000, 16384)
# all-ones shapes: rand_shift of the bucketed plan below, at and above 32 (asserted against bound_plan)
ALL_ONES = {"below32": dict(U=300_000, P=1 << 20, l0=2, linf=2, rand_shift=31, both=False),
            "at32": dict(U=1 << 24, P=1 << 22, l0=4, linf=2, rand_shift=32, both=True),
            "above32": dict(U=300_000, P=10_000_000, l0=2, linf=2, rand_shift=35, both=False)}
ROW_TIE = dict(U=300_000, P=5000, n=1 << 19, min_ties=4)
BIG_OFFSET = 3_000_000_007


# ---------------------------------------------------------------- inverses --
def _u32(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def unfmix32(t):
    """The inverse of oracle.columnar.fmix32 (uint32 arrays)."""
    h = _u32(t)
    with np.errstate(over="ignore"):
        h = h ^ (h >> np.uint32(16))
        h = h * np.uint32(_I2)
        h = h ^ (h >> np.uint32(13)) ^ (h >> np.uint32(26))
        h = h * np.uint32(_I1)
        return h ^ (h >> np.uint32(16))


def _pid_word(seed, pid):
    pid = np.atleast_1d(np.asarray(pid)).astype(np.uint64)
    lo, hi = _u32(pid), _u32(pid >> np.uint64(32))
    with np.errstate(over="ignore"):
        rot = (hi << np.uint32(16)) | (hi >> np.uint32(16))
        return (lo ^ rot ^ np.uint32(int(seed) & 0xFFFFFFFF)) * np.uint32(_MPID)


def solve_pk(seed, pid, T):
    """The partition low word (int64 in [0, 2^32)) with pair_hash(seed, pid, pk) == T;
    pid and T broadcast.  Each result is checked with the oracle's pair_hash."""
    w, a = np.broadcast_arrays(_pid_word(seed, pid), unfmix32(T))
    with np.errstate(over="ignore"):
        pk = (((a ^ w) - np.uint32((int(seed) >> 32) & 0xFFFFFFFF)) * np.uint32(_IPK)).astype(np.int64)
    u = np.broadcast_to(np.atleast_1d(np.asarray(pid, dtype=np.int64)), pk.shape)
    assert np.array_equal(O.pair_hash(seed, u, pk), np.broadcast_to(_u32(T), pk.shape)), "solve_pk"
    return pk


def both_ids(seed, U, P, T1=0xFFFFFFFF, T2=0xFFFFFFFE):
    """[(pid, pk1, pk2)]: the ids below U that hold pair hash T1 at a
    partition pk1 < P and T2 at pk2 < P (about U (P / 2^32)^2 of them)."""
    ids = np.arange(U, dtype=np.int64)
    k1, k2 = solve_pk(seed, ids, T1), solve_pk(seed, ids, T2)
    return [(int(u), int(k1[u]), int(k2[u])) for u in np.flatnonzero((k1 < P) & (k2 < P))]


# ------------------------------------------------------------- priorities --
def grain(rand_shift):
    """Pair hashes equal above this many low bits share their retained bits."""
    return 1 << max(0, rand_shift - 32)


def masked_hash(h, rand_shift):
    """The random part of a pair key, as a Python int: the 32-bit pair hash
    from key bit 32 up, cut below rand_shift; a part that is all ones has its
    lowest bit cleared (all ones marks empty sketch slots and dead records)."""
    h = int(h)
    bits = 64 - rand_shift
    m = (h << (32 - rand_shift)) if rand_shift <= 32 else (h >> (rand_shift - 32))
    if m == (1 << bits) - 1:
        m -= 1
    return m


def row_hash32(row_seed, global_row):
    """The 32 hash bits of a row key (uint64 array of values < 2^32)."""
    g = np.asarray(global_row).astype(np.uint64)
    with np.errstate(over="ignore"):
        return O.mix64(np.uint64(row_seed) ^ (g * np.uint64(_ROW_MUL))) >> np.uint64(32)


def tie_groups(seed, pid, n_partitions_scanned, random_bits):
    """[(masked hash, [partitions, ascending])] for the groups of two or more
    of the id's first n partitions that are equal in the retained hash bits
    (with the all-ones rule), ascending by masked hash."""
    pk = np.arange(n_partitions_scanned, dtype=np.int64)
    h = O.pair_hash(seed, np.full(len(pk), pid, dtype=np.int64), pk).astype(np.int64)
    m = h >> (32 - random_bits) if random_bits <= 32 else h << (random_bits - 32)
    m = np.where(m == (1 << random_bits) - 1, m - 1, m)
    order = np.lexsort((pk, m))
    ms, ks = m[order], pk[order]
    start = np.flatnonzero(np.r_[True, ms[1:] != ms[:-1]])
    size = np.diff(np.r_[start, len(ms)])
    return [(int(ms[s]), ks[s:s + z].tolist()) for s, z in zip(start[size > 1], size[size > 1])]


def row_ties(seed, row_offset, n, per_pid=False):
    """[(i, j, hash)] with i < j < n: local rows whose keys under
    derive_row_seed (per_pid: derive_pid_row_seed) have equal high 32 bits."""
    rs = O.derive_pid_row_seed(seed) if per_pid else O.derive_row_seed(seed)
    h = row_hash32(rs, row_offset + np.arange(n, dtype=np.int64)).astype(np.int64)
    order = np.argsort(h, kind="stable")
    hs = h[order]
    eq = np.flatnonzero(hs[1:] == hs[:-1])
    return [(int(order[e]), int(order[e + 1]), int(hs[e])) for e in eq]


# ------------------------------------------------------------------ tables --
@dataclasses.dataclass
class Table:
    pid: np.ndarray
    pk: np.ndarray
    val: np.ndarray
    U: int
    P: int
    seed: int
    planted: list          # dicts: what was planted where (see each builder)
    allowed: np.ndarray = None
    row_offset: int = 0


def _assemble(rng, U, P, seed, planted_rows, n_fill, planted, reserved, allowed=None, fill_pk=None):
    """Random filler rows over the ids outside `reserved`, the planted rows
    (list of (pid, pk, copies)), shuffled; value = local row index."""
    fu = rng.integers(0, U, n_fill, dtype=np.int64)
    fk = rng.integers(0, P, n_fill, dtype=np.int64) if fill_pk is None else fill_pk(rng, n_fill)
    keep = ~np.isin(fu, np.fromiter(reserved, dtype=np.int64, count=len(reserved)))
    pu = np.array([u for u, k, c in planted_rows for _ in range(c)], dtype=np.int64)
    pk_ = np.array([k for u, k, c in planted_rows for _ in range(c)], dtype=np.int64)
    pid, pk = np.concatenate([fu[keep], pu]), np.concatenate([fk[keep], pk_])
    perm = rng.permutation(len(pid))
    pid, pk = pid[perm], pk[perm]
    return Table(pid, pk, np.arange(len(pid), dtype=np.int64), U, P, seed, planted, allowed)


def _near(seed, u, T, P, below, window=1 << 15):
    """Partitions < P of id u whose hash lies in [T - window, T) (below) or in
    (T, T + window], nearest first, as [(pk, hash)]."""
    ts = (T - 1 - np.arange(window, dtype=np.int64)) if below else (T + 1 + np.arange(window, dtype=np.int64))
    ts = ts[(ts >= 0) & (ts < _M32)]
    pk = solve_pk(seed, u, ts)
    ok = pk < P
    return list(zip(pk[ok].tolist(), ts[ok].tolist()))


def edge_hashes(sieve):
    """The four hashes at the candidate and band edges of one sieve value
    (two where the plan has no band: t = 1/2)."""
    t32 = sieve << 16
    out = [t32 - 1, t32]
    if sieve <= 16384:  # the band is planned up to t = 1/4 and reaches 2t
        out += [(2 * sieve << 16) - 1, 2 * sieve << 16]
    return out


def threshold_table(seed, U, P, n_fill, per_edge, l0s=THRESHOLD_L0S, sieves=SIEVES, rng_seed=1):
    """For every edge hash T of every sieve value and every l0: per_edge ids
    whose l0-th smallest pair has hash exactly T, their l0 - 1 other kept
    pairs solved strictly below T and two more strictly above.  planted:
    {"T", "l0", "pid", "pk", "below": [pk], "above": [pk]}."""
    rng = np.random.default_rng(rng_seed)
    ids = np.arange(U, dtype=np.int64)
    used, planted, rows = set(), [], []
    for T in sorted({T for s in sieves for T in edge_hashes(s)}):
        sol = solve_pk(seed, ids, T)
        cand = [int(u) for u in np.flatnonzero(sol < P)]
        for l0 in l0s:
            got = 0
            for u in cand:
                if got == per_edge:
                    break
                if u in used:
                    continue
                lo, hi = _near(seed, u, T, P, True), _near(seed, u, T, P, False)
                if len(lo) < l0 - 1 or len(hi) < 2:
                    continue  # (fewer solved neighbours below P than the id needs)
                used.add(u)
                got += 1
                rec = {"T": T, "l0": l0, "pid": u, "pk": int(sol[u]), "below": [k for k, _ in lo[:l0 - 1]],
                       "above": [k for k, _ in hi[:2]]}
                planted.append(rec)
                rows += [(u, k, 2) for k in [rec["pk"]] + rec["below"] + rec["above"]]
            assert got >= per_edge, f"threshold table: {got} ids for T={T:#x}, l0={l0}; need {per_edge}"
    t = _assemble(rng, U, P, seed, rows, n_fill, planted, used)
    check_threshold(t)
    return t


def with_heavy_ids(t, ids, extra, rng_seed=9):
    """t with `extra` more rows for each of `ids`, spread over the id's own
    partitions (no new pair: every hash-derived expectation stays)."""
    rng = np.random.default_rng(rng_seed)
    pu, pk = [t.pid], [t.pk]
    for u in ids:
        own = np.unique(t.pk[t.pid == u])
        pu.append(np.full(extra, u, dtype=np.int64))
        pk.append(rng.choice(own, extra))
    pid, pk = np.concatenate(pu), np.concatenate(pk)
    perm = rng.permutation(len(pid))
    return dataclasses.replace(t, pid=pid[perm], pk=pk[perm], val=np.arange(len(pid), dtype=np.int64))


def _pairs_of(t, ids):
    """{id: [(hash, pk)] ascending} over the table's distinct public pairs of `ids`."""
    m = np.isin(t.pid, np.fromiter(ids, dtype=np.int64, count=len(ids)))
    if t.allowed is not None:
        m &= t.allowed[t.pk]
    pairs = np.unique(np.stack([t.pid[m], t.pk[m]]), axis=1)
    h = O.pair_hash(t.seed, pairs[0], pairs[1])
    out = {}
    for u, k, x in zip(pairs[0].tolist(), pairs[1].tolist(), h.tolist()):
        out.setdefault(u, []).append((x, k))
    return {u: sorted(v) for u, v in out.items()}


def check_threshold(t):
    per = _pairs_of(t, {r["pid"] for r in t.planted})
    for r in t.planted:
        ps = per[r["pid"]]
        assert len(ps) == r["l0"] + 2 and ps[r["l0"] - 1] == (r["T"], r["pk"]), r
        assert all(x < r["T"] for x, _ in ps[:r["l0"] - 1]) and all(x > r["T"] for x, _ in ps[r["l0"]:]), r


def short_ids(t, l0, sieve):
    """(ids with fewer than l0 distinct public pairs below t, those with fewer
    than l0 below the band's edge min(2t, 1/2)), from the pair hashes alone;
    ids without rows count."""
    m = np.ones(len(t.pid), dtype=bool) if t.allowed is None else t.allowed[t.pk]
    pairs = np.unique(np.stack([t.pid[m], t.pk[m]]), axis=1)
    h = O.pair_hash(t.seed, pairs[0], pairs[1]).astype(np.int64)
    out = []
    for edge in (sieve, min(2 * sieve, 32768)):
        below = h < (edge << 16)
        out.append(np.flatnonzero(np.bincount(pairs[0][below], minlength=t.U) < l0))
    return out


def all_ones_table(seed, U, P, rand_shift, l0, per_kind=4, n_fill=100_000, both=False, rng_seed=2):
    """Pairs whose key's random part is all ones (and its neighbour below),
    as the largest pair of ids with l0 - 1 pairs ("short", l0 > 1), l0 pairs
    ("exact"), l0 + 1 pairs ("over": the planted pair is rank l0 + 1 and
    dropped), and of ids whose planted partition is not public ("dead": an
    `allowed` mask; the id's other l0 pairs are all kept).  With rand_shift >
    32 the planted hashes cover the whole all-ones grain and the one below;
    "tie": ids with two pairs in those two grains (equal after the cleared
    bit: the partition decides) at ranks l0, l0 + 1.  both (rand_shift == 32):
    every id that holds 0xFFFFFFFF and 0xFFFFFFFE (both_ids; at least one is
    required): they tie in the same way, "both".  planted: {"kind", "pid", "pk", "T",
    "others": [pk], "kept": bool}."""
    rng = np.random.default_rng(rng_seed)
    g = grain(rand_shift)
    tops = [_M32 - 1 - i for i in range(2 * g)] if g > 1 else [_M32 - 1, _M32 - 2]
    ids = np.arange(U, dtype=np.int64)
    sols = {T: solve_pk(seed, ids, T) for T in tops}
    used, planted, rows, dead_pk = set(), [], [], set()
    kinds = [("short", l0 - 2), ("exact", l0 - 1), ("over", l0), ("dead", l0)]
    want_both, both = both, (both_ids(seed, U, P) if both else [])
    assert not want_both or both, "all-ones table: no id holds both 0xFFFFFFFF and 0xFFFFFFFE below P"
    used.update(u for u, _, _ in both)
    for T in tops:
        cand = iter(int(u) for u in np.flatnonzero(sols[T] < P))
        for kind, n_other in kinds:
            if n_other < 0:
                continue
            got = 0
            quota = per_kind if T >= _M32 - 2 else 1  # every hash of the two grains at least once per kind
            while got < quota:
                u = next(cand, None)
                assert u is not None, f"all-ones table: {got} ids of kind {kind} for T={T:#x}; need {quota}"
                if u in used or int(sols[T][u]) in dead_pk:
                    continue
                lo = _near(seed, u, _M32 - 2 * g, P, True, window=1 << 17)
                if len(lo) < n_other:
                    continue
                used.add(u)
                got += 1
                rec = {"kind": kind, "pid": u, "pk": int(sols[T][u]), "T": T, "others": [k for k, _ in lo[:n_other]],
                       "kept": kind in ("short", "exact")}
                if kind == "dead":
                    dead_pk.add(rec["pk"])
                planted.append(rec)
                rows += [(u, k, 2) for k in [rec["pk"]] + rec["others"]]
    if g > 1:  # two pairs of one id in the top two grains
        hit = np.stack([sols[T] < P for T in tops])
        got = 0
        for u in np.flatnonzero(hit.sum(axis=0) >= 2).tolist():
            ks = sorted(int(sols[T][u]) for T, h in zip(tops, hit[:, u]) if h)[:2]
            lo = _near(seed, u, _M32 - 2 * g, P, True, window=1 << 17)
            if u in used or len(lo) < l0 - 1 or dead_pk & set(ks):
                continue
            used.add(u)
            got += 1
            planted.append({"kind": "tie", "pid": u, "pk": ks[0], "loser": ks[1], "T": None,
                            "others": [k for k, _ in lo[:l0 - 1]], "kept": True})
            rows += [(u, k, 2) for k in ks + planted[-1]["others"]]
            if got == 4 * per_kind:
                break
        assert got >= per_kind, f"all-ones table: {got} ids with two pairs in the top grains"
    for u, k1, k2 in both:
        lo = _near(seed, u, _M32 - 2, P, True, window=1 << 17)
        assert len(lo) >= l0 - 1 and not dead_pk & {k1, k2}
        planted.append({"kind": "both", "pid": u, "pk": min(k1, k2), "loser": max(k1, k2), "T": None,
                        "others": [k for k, _ in lo[:l0 - 1]], "kept": True})
        rows += [(u, k, 2) for k in [k1, k2] + planted[-1]["others"]]
    live_pk = {k for r in planted for k in [r["pk"]] + r["others"] + [r.get("loser", r["pk"])]} - dead_pk
    allowed = rng.random(P) < 0.9
    allowed[list(live_pk)] = True
    allowed[list(dead_pk)] = False
    t = _assemble(rng, U, P, seed, rows, n_fill, planted, used, allowed)
    check_all_ones(t, rand_shift, l0)
    return t


def check_all_ones(t, rand_shift, l0):
    ones = (1 << (64 - rand_shift)) - 1
    raw = lambda x: (x << (32 - rand_shift)) if rand_shift <= 32 else (x >> (rand_shift - 32))
    per = _pairs_of(t, {r["pid"] for r in t.planted})
    n_ones = 0
    for r in t.planted:
        ps = sorted((masked_hash(x, rand_shift), k) for x, k in per[r["pid"]])
        hashes = {k: x for x, k in per[r["pid"]]}
        if r["kind"] == "dead":
            assert not t.allowed[r["pk"]] and r["pk"] not in hashes and len(ps) == l0, r
            continue
        rank = ps.index((masked_hash(hashes[r["pk"]], rand_shift), r["pk"]))
        assert (rank < l0) == r["kept"], (r, rank)
        if r["kind"] in ("tie", "both"):  # equal random parts at ranks l0 - 1, l0: the partition decides
            assert rank == l0 - 1 and ps[l0][1] == r["loser"] and ps[l0][0] == ps[rank][0] and r["pk"] < r["loser"], r
            n_ones += 1
        else:
            assert hashes[r["pk"]] == r["T"] and rank == len(ps) - 1 == {"short": l0 - 2, "exact": l0 - 1,
                                                                        "over": l0}[r["kind"]], (r, rank)
            n_ones += raw(r["T"]) == ones
    # rand_shift < 32: no random part is all ones (the 32-bit expand_key has no guard)
    assert (n_ones > 0) == (rand_shift >= 32), (n_ones, rand_shift)


def _masked_scan(seed, u, scan, rand_shift):
    pk = np.arange(scan, dtype=np.int64)
    return O.pair_hash(seed, np.full(scan, u, dtype=np.int64), pk).astype(np.int64) >> (rand_shift - 32)


def pair_tie_table(seed, U, P, rand_shift, l0, n_fill, n_ids, scan, triples=2, sieves=PAIR_TIE_SIEVES, rng_seed=3):
    """n_ids ids holding a tie group (2 partitions equal in the retained
    hash bits; 3 for `triples` of them when l0 >= 2, found in a 16 times
    longer scan) that straddles rank l0: the lower partitions win.  The
    groups alternate between three zones of the smallest sieve value: wholly
    below its threshold, wholly inside its band, above the band.  planted:
    {"l0", "pid", "group": [pk], "winners": n, "zone", "below": [pk],
    "above": [pk]}."""
    assert rand_shift > 32
    rng = np.random.default_rng(rng_seed)
    bits, sh = 64 - rand_shift, rand_shift - 32
    t32 = min(sieves) << 16
    zones = {"candidate": (0, t32 >> sh), "band": (t32 >> sh, 2 * t32 >> sh), "above": (2 * t32 >> sh, (1 << bits) - 2)}
    planted, rows, used = [], [], set()
    u = U
    for j in range(n_ids):
        size = 3 if (j < triples and l0 >= 2) else 2
        n_scan = min(P, 16 * scan if size == 3 else scan)
        n_below = l0 - (size - 1)  # the group then holds ranks l0 - size + 2 .. l0 + 1
        while True:
            u -= 1
            assert u >= 0, "pair-tie table: ran out of ids"
            mh = _masked_scan(seed, u, n_scan, rand_shift)
            pick = None
            for m, ks in tie_groups(seed, u, n_scan, bits):
                zone = next(z for z, (lo, hi) in zones.items() if lo <= m < hi or (z == "above" and m >= lo))
                if len(ks) == size and m < zones["above"][1] and (size == 3 or zone == list(zones)[j % 3]) and \
                        (mh < m).sum() >= n_below:
                    pick = (m, ks, zone)
                    break
            if pick is not None:
                break
        m, ks, zone = pick
        below = rng.choice(np.flatnonzero(mh < m), n_below, replace=False).tolist()
        above = rng.choice(np.flatnonzero((mh > m) & (mh < (1 << bits) - 2)), 2, replace=False).tolist()
        used.add(u)
        planted.append({"l0": l0, "pid": u, "group": ks, "winners": size - 1, "zone": zone, "below": below,
                        "above": above})
        rows += [(u, k, 2) for k in ks + below + above]
    # filler partitions as test_sieve_packed_wide's: Zipf(1.1) folded into P
    t = _assemble(rng, U, P, seed, rows, n_fill, planted, used,
                  fill_pk=lambda r, n: np.minimum(r.zipf(1.1, n) - 1, P - 1).astype(np.int64))
    check_pair_ties(t, rand_shift)
    return t


def check_pair_ties(t, rand_shift):
    per = _pairs_of(t, {r["pid"] for r in t.planted})
    for r in t.planted:
        ps = sorted((masked_hash(x, rand_shift), k) for x, k in per[r["pid"]])
        first = r["l0"] - r["winners"]
        group = ps[first:first + len(r["group"])]
        assert [k for _, k in group] == r["group"] and len({m for m, _ in group}) == 1, r
        assert first + len(r["group"]) == r["l0"] + 1 and len(ps) == r["l0"] + 3, r  # straddles rank l0
        full = {x >> (rand_shift - 32) << (rand_shift - 32) for x, k in per[r["pid"]] if k in r["group"]}
        t32 = min(PAIR_TIE_SIEVES) << 16
        lo, hi = {"candidate": (0, t32), "band": (t32, 2 * t32), "above": (2 * t32, _M32)}[r["zone"]]
        assert len(full) == 1 and lo <= min(full) and max(full) + grain(rand_shift) <= hi, r


def row_tie_table(seed, U, P, n, cap, row_offset, per_pid=False, min_ties=4, rng_seed=4):
    """n rows whose local indices hold every pair (i, j) of rows equal in
    their 32 hash bits.  Both rows of a collision sit in one (pid, pk) pair of
    an id of their own (per_pid: in one id, in two partitions) together with
    cap - 1 rows of smaller hash and two of larger, so the collision straddles
    rank cap and the lower row index wins.  Half of the planted pairs have
    the smallest pair hash of their id's partitions (a sieve candidate), half
    the largest (beyond the band: the rescan).  planted: {"pid", "pk", "keep":
    i, "drop": j, "smaller": [rows], "larger": [rows]}."""
    rng = np.random.default_rng(rng_seed)
    rs = O.derive_pid_row_seed(seed) if per_pid else O.derive_row_seed(seed)
    h = row_hash32(rs, row_offset + np.arange(n, dtype=np.int64)).astype(np.int64)
    ties = row_ties(seed, row_offset, n, per_pid)
    n_ids = len(ties)
    pid = rng.integers(0, U - n_ids, n, dtype=np.int64)  # the last n_ids ids are the planted ones
    pk = rng.integers(0, P, n, dtype=np.int64)
    taken = {r for i, j, _ in ties for r in (i, j)}
    planted = []
    all_pk = np.arange(P, dtype=np.int64)
    for c, (i, j, x) in enumerate(ties):
        u = U - n_ids + c
        free = np.array([r for r in rng.permutation(n)[:20 * (cap + 2)].tolist() if r not in taken], dtype=np.int64)
        smaller, larger = free[h[free] < x][:cap - 1].tolist(), free[h[free] > x][:2].tolist()
        if len(smaller) < cap - 1 or len(larger) < 2:
            continue  # (a collision at a hash too small to have cap - 1 rows below it)
        taken.update(smaller + larger)
        ph = O.pair_hash(seed, np.full(P, u, dtype=np.int64), all_pk)
        k = int(np.argmin(ph) if c % 2 == 0 else np.argmax(ph))
        rows = [i, j] + smaller + larger
        pid[rows] = u
        pk[rows] = rng.integers(0, P, len(rows)) if per_pid else k
        planted.append({"pid": u, "pk": k, "keep": i, "drop": j, "smaller": smaller, "larger": larger})
    assert len(planted) >= min_ties, f"row-tie table: {len(planted)} collisions planted; need {min_ties}"
    t = Table(pid, pk, np.arange(n, dtype=np.int64), U, P, seed, planted, None, row_offset)
    check_row_ties(t, cap, per_pid)
    return t


def check_row_ties(t, cap, per_pid):
    rs = O.derive_pid_row_seed(t.seed) if per_pid else O.derive_row_seed(t.seed)
    for r in t.planted:
        rows = np.flatnonzero(t.pid == r["pid"])
        assert len(rows) == cap + 3 and (per_pid or (t.pk[rows] == r["pk"]).all()), r
        keys = sorted(zip(row_hash32(rs, t.row_offset + rows).tolist(), rows.tolist()))
        assert keys[cap - 1][1] == r["keep"] and keys[cap][1] == r["drop"] and r["keep"] < r["drop"], r
        assert keys[cap - 1][0] == keys[cap][0] and (cap == 1 or keys[cap - 2][0] < keys[cap - 1][0]), r
        assert keys[cap + 1][0] > keys[cap][0], r


# ----------------------------------------------------- plain restatement --
def plain_bound(pid, pk, val, *, P, l0, linf, seed, rand_shift, row_offset=0, allowed=None, max_contributions=0,
                lo=0, hi=VALUE_HI, higher_row_wins=False):
    """Bounding with the hash priorities in dicts, sorted() and Python ints:
    per id the max_contributions rows of smallest (row hash, row); per id the
    l0 pairs of smallest (masked hash with the all-ones rule, partition); per
    kept pair the linf rows of smallest (row hash, row); 0 = no bound.
    higher_row_wins: the wrong tie-break (a mutant the tables must tell apart).
    Returns privacy_id_count, count and the int64 sum of the clipped values."""
    pid, pk = np.asarray(pid, dtype=np.int64), np.asarray(pk, dtype=np.int64)
    n = len(pid)
    g = row_offset + np.arange(n, dtype=np.int64)
    rh = row_hash32(O.derive_row_seed(seed), g).tolist()
    sign = -1 if higher_row_wins else 1
    live = range(n) if allowed is None else [i for i in range(n) if allowed[pk[i]]]
    pl, kl, vl = pid.tolist(), pk.tolist(), np.asarray(val).tolist()
    if max_contributions:
        ph = row_hash32(O.derive_pid_row_seed(seed), g).tolist()
        by_id = {}
        for i in live:
            by_id.setdefault(pl[i], []).append((ph[i], sign * i))
        live = sorted(sign * si for rows in by_id.values() for _, si in sorted(rows)[:max_contributions])
    pairs = {}
    for i in live:
        pairs.setdefault(pl[i], {}).setdefault(kl[i], []).append((rh[i], sign * i))
    ids = list(pairs)
    flat_u = [u for u in ids for _ in pairs[u]]
    flat_k = [k for u in ids for k in pairs[u]]
    hashes = O.pair_hash(seed, np.array(flat_u, dtype=np.int64), np.array(flat_k, dtype=np.int64)).tolist()
    pidc, cnt, tot = [0] * P, [0] * P, [0] * P
    at = 0
    for u in ids:
        ks = list(pairs[u])
        order = sorted((masked_hash(hashes[at + j], rand_shift), k) for j, k in enumerate(ks))
        at += len(ks)
        for _, k in (order[:l0] if l0 else order):
            rows = sorted(pairs[u][k])
            rows = rows[:linf] if linf else rows
            pidc[k] += 1
            cnt[k] += len(rows)
            tot[k] += sum(min(max(vl[sign * si], lo), hi) for _, si in rows)
    return {"privacy_id_count": np.array(pidc, dtype=np.int64), "count": np.array(cnt, dtype=np.int64),
            "sum": np.array(tot, dtype=np.int64)}


def oracle_bound(t, *, l0, linf, rand_shift, max_contributions=0):
    return O.bound_and_reduce(t.pid, t.pk, t.val, n_privacy_ids=t.U, n_partitions=t.P, l0=l0, linf=linf,
                              value_kind=O.VALUE_I64, flags=FLAGS, min_value=0, max_value=VALUE_HI, seed=t.seed,
                              row_offset=t.row_offset, allowed=t.allowed, rand_shift=rand_shift,
                              max_contributions=max_contributions)
