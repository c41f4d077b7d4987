"""Host side of the PERCENTILE edge tests: restatements and constructed inputs.

Shared by tests/test_percentile_edges_host.py (CPU: proves everything here)
and tests/test_gpu_percentile_edges.py (GPU: compares the kernels with it by
equality).

noised_expected()  the restatement's walk (quantile_tree_util.Tree.quantiles)
                   over the bit-exact host form of the secure samplers
                   (oracle.columnar.secure_add_noise), node n of partition p on
                   the Philox stream (partition_offset + p) * 69904 + n - 1 of
                   slot N.QUANTILE_SLOT; it also counts the edges the walk met.
kept_rows()        which rows the pair table keeps, in dicts, sorted() and
                   Python ints over the oracle's hash functions; it shares
                   nothing else with oracle.columnar.bound_and_reduce.
walk_trees() ...   the inputs of the GPU tests.  Every builder asserts what its
                   table is for (check_*): a table that stops exercising its
                   edge fails on the CPU, it does not pass silently on the GPU.
"""
import functools
import math

import numpy as np

from oracle import columnar as O
from pipelinedp_amd import _native as N
from pipelinedp_amd import executor as X
from tests import quantile_tree_util as Q

BIG = 1 << 20  # l0 / linf no table below reaches
NOISE_SEED = 0x5EED_0001_0203  # above 2^32: both key words of the Philox streams are non-zero
RANKS7 = [0.0, 0.1, 0.37, 0.5, 0.5, 0.9, 1.0]  # two rounds of four, the second partial
RANKS64 = np.linspace(0.0, 1.0, 64).tolist()    # 16 full rounds
EPS, DELTA = 0.5, 1e-6
WALK_SIZES = (0, 1, 2, 5, 17, 64, 300, 2000)
OFFSETS = (1000, 61_440)  # 61,441 * 69,904 is the first product above 2^32
INDEX7 = [5, 2, 2, -1, 8, 0, 7]  # over P = 8: a repeat, a negative entry and P itself


def noise(kind):
    """The mechanism of the walk tests: eps = 0.5, delta = 1e-6, L0 = H (one
    partition per id, every level counts the row once), Linf = 1."""
    import pipelinedp_amd as pdp
    from pipelinedp_amd import dp_computations as dpc
    nk = pdp.NoiseKind.LAPLACE if kind == "laplace" else pdp.NoiseKind.GAUSSIAN
    return dpc.noise_params(nk, EPS, DELTA, Q.H, 1)


# ------------------------------------------------------------ noised walk --
def tree_of_leaves(leaves, lo, hi):
    """quantile_tree_util.Tree holding the given leaf codes."""
    t = Q.Tree(lo, hi)
    t.leaves += np.bincount(np.asarray(leaves, dtype=np.int64), minlength=Q.L)
    return t


def node_noise(tree, noise_params, seed, partition_offset, p, counters=None):
    """noise(node, raw) for partition p's tree.  The 16 children of one node
    are drawn in one call of the vectorised sampler (every element has its own
    stream and block counter, so that equals 16 single draws) and kept.
    counters, a dict, gains what the walk met; a node is seen once, when the
    walk first asks for it, whatever the number of ranks that pass it:
      clamped      noised counts below 0 (the walk reads them as 0)
      entered_raw0 nodes of levels 1 ... 3 the walk descended into whose raw
                   count is 0: every child below exists only by noise
      picked_zero  nodes of levels 1 ... 3 the walk descended into whose own
                   noised count is 0 (the step's rank became 0 or 1 from a
                   NaN or an infinity)"""
    nd = noise_params.as_dict()
    cum = np.concatenate([[0], np.cumsum(tree.leaves)])
    memo = {}

    def draw(level, group):
        span = Q.B**(Q.H - level)
        pos = group * Q.B + np.arange(Q.B)
        raw = (cum[(pos + 1) * span] - cum[pos * span]).astype(np.float64)
        nodes = Q.FIRST[level] + pos
        gidx = np.array([(partition_offset + p) * Q.NODES + int(n) - 1 for n in nodes], dtype=np.int64)
        out = O.secure_add_noise(nd, raw, seed, gidx, N.QUANTILE_SLOT)
        if counters is not None:
            counters["clamped"] += int((out < 0.0).sum())
            if level > 1:
                parent = Q.FIRST[level - 1] + group
                counters["entered_raw0"] += int(raw.sum() == 0.0)
                counters["picked_zero"] += int(not memo[parent][0] > 0.0)
        for n, x, r in zip(nodes.tolist(), out.tolist(), raw.tolist()):
            memo[n] = (x, r)

    def fn(node, raw):
        if node not in memo:
            level = max(lv for lv in range(1, Q.H + 1) if Q.FIRST[lv] <= node)
            draw(level, (node - Q.FIRST[level]) // Q.B)
        x, r = memo[node]
        assert r == raw, (node, raw, r)
        return x

    return fn


def noised_expected(leaves_by_partition, lo, hi, ranks, noise, seed, partition_offset, index):
    """(out, counters): out[i] = the restatement's answers at `ranks` for
    partition index[i], every node count noised by `noise` (a NoiseParams;
    None: the exact tree) on its own Philox stream.  Rows of entries outside
    [0, P) are NaN: the kernel leaves them alone."""
    P = len(leaves_by_partition)
    counters = {"clamped": 0, "entered_raw0": 0, "picked_zero": 0}
    rows = {}
    for p in sorted({int(i) for i in index if 0 <= int(i) < P}):
        tree = tree_of_leaves(leaves_by_partition[p], lo, hi)
        fn = None if noise is None else node_noise(tree, noise, seed, partition_offset, p, counters)
        rows[p] = tree.quantiles(ranks, noise=fn)
    nan_row = [math.nan] * len(ranks)
    out = np.array([rows.get(int(i), nan_row) for i in index], dtype=np.float64).reshape(len(index), len(ranks))
    return out, counters


def pack_trees(leaves_by_partition):
    """(leaves int16 holding uint16 bits, offsets int32 holding uint32 bits) as
    pdp_reduce_quantile_leaves lays them out."""
    sizes = [len(x) for x in leaves_by_partition]
    flat = np.concatenate([np.sort(np.asarray(x, dtype=np.uint16)) for x in leaves_by_partition] +
                          [np.zeros(0, np.uint16)])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    return flat.view(np.int16), off.view(np.int32)


@functools.lru_cache(maxsize=None)
def walk_trees(duplicate=False):
    """Eight partitions of 0, 1, 2, 5, 17, 64, 300 and 2,000 uniform values over
    [0, 1], as ascending leaf codes.  duplicate: a ninth partition with the
    leaves of partition 6 (the same tree under another stream index)."""
    rng = np.random.default_rng(41)
    trees = [np.sort(Q.leaf_index(rng.uniform(0.0, 1.0, m), 0.0, 1.0)).astype(np.uint16) for m in WALK_SIZES]
    if duplicate:
        trees.append(trees[6].copy())
    check_walk_trees(trees)
    return trees


def check_walk_trees(trees):
    assert [len(t) for t in trees[:8]] == list(WALK_SIZES)
    assert all(np.all(np.diff(t.astype(np.int64)) >= 0) for t in trees)
    if len(trees) > 8:
        assert np.array_equal(trees[8], trees[6]) and len(trees[8]) > 0
    # the stream indices of one launch straddle 2^32 at the larger offset
    first = (OFFSETS[1] + 0) * Q.NODES
    last = (OFFSETS[1] + len(trees) - 1) * Q.NODES + Q.NODES - 1
    assert first < 1 << 32 < last and (OFFSETS[1] + 1) * Q.NODES > 1 << 32 > OFFSETS[1] * Q.NODES


@functools.lru_cache(maxsize=None)
def walk_expected(kind, partition_offset=0, ranks=tuple(RANKS7), partitions=None, duplicate=False):
    """noised_expected of walk_trees, computed once per argument set.
    kind: "laplace", "gaussian" or None (no noise)."""
    trees = walk_trees(duplicate)
    index = list(range(len(trees))) if partitions is None else list(partitions)
    return noised_expected(trees, 0.0, 1.0, list(ranks), None if kind is None else noise(kind), NOISE_SEED,
                           partition_offset, index)


# -------------------------------------------------------------- kept rows --
def pair_table_rand_shift(n, U, P, l0, linf):
    """The lowest random bit of the pair table's sampling key.  The table ranks
    an id's pairs by the unbucketed pair key, whose random part starts above
    the partition bits of the configuration's n_partitions (pdp_pairs.hip:
    pk_bits = bits_for(n_partitions); the plan's rand_shift field describes
    the bucketed plans' keys and stays 0 here).  Read off the configuration
    executor.bound_config builds for reduce_quantile_leaves, after the library
    has confirmed that it resolves to the pair table (no device work)."""
    spec = X.BoundingSpec(l0=l0, linf=linf, value_kind=N.VALUE_NONE, flags=0)
    cfg = X.bound_config(n, U, P, spec, 0, 0, N.ALGO_PAIR_TABLE)
    assert X.bound_plan_info(cfg).algorithm == N.ALGO_PAIR_TABLE
    return O.pk_bits(int(cfg.n_partitions))


def kept_rows(pid, pk, *, P, U, l0, linf, seed, row_offset=0, allowed=None):
    """Ascending indices of the rows the pair table keeps: the rows of keys in
    range and of allowed partitions; per id the l0 pairs of smallest pair
    priority; per kept pair the linf rows of smallest row priority."""
    pid, pk = np.asarray(pid, dtype=np.int64), np.asarray(pk, dtype=np.int64)
    n = len(pid)
    rand_shift = pair_table_rand_shift(n, U, P, l0, linf)
    rows = np.arange(n, dtype=np.int64)
    rprio = O.row_priority(O.derive_row_seed(seed), row_offset + rows, rows).tolist()
    pl, kl = pid.tolist(), pk.tolist()
    pairs = {}
    for i in range(n):
        if not (0 <= pl[i] < U and 0 <= kl[i] < P):
            continue
        if allowed is not None and not allowed[kl[i]]:
            continue
        pairs.setdefault(pl[i], {}).setdefault(kl[i], []).append((rprio[i], i))
    kept = []
    for u, by_pk in pairs.items():
        ks = list(by_pk)
        pprio = O.pair_priority(seed, np.full(len(ks), u, dtype=np.int64), np.array(ks, dtype=np.int64),
                                rand_shift).tolist()
        for _, k in sorted(zip(pprio, ks))[:l0]:
            kept += [i for _, i in sorted(by_pk[k])[:linf]]
    return np.array(sorted(kept), dtype=np.int64)


def kept_partitions(pid, pk, rows):
    """{id: set of partitions} of the given rows."""
    out = {}
    for u, k in zip(np.asarray(pid)[rows].tolist(), np.asarray(pk)[rows].tolist()):
        out.setdefault(u, set()).add(k)
    return out


def leaves_of_rows(values, pk, rows, P, lo, hi):
    """(leaves uint16 in (partition, leaf) order, offsets) of values[rows], NaN
    removed; an integer column is converted as astype(float64) rounds."""
    v = np.asarray(values)[rows].astype(np.float64)
    k = np.asarray(pk, dtype=np.int64)[rows]
    ok = ~np.isnan(v)
    v, k = v[ok], k[ok]
    leaf = Q.leaf_index(v, lo, hi)
    order = np.lexsort((leaf, k))
    off = np.concatenate([[0], np.cumsum(np.bincount(k, minlength=P))])
    return leaf[order].astype(np.uint16), off


def trees_of_rows(values, pk, rows, partitions, lo, hi):
    """{p: Tree} of values[rows] for the given partitions."""
    v = np.asarray(values)[rows].astype(np.float64)
    k = np.asarray(pk, dtype=np.int64)[rows]
    return {p: Q.Tree(lo, hi, v[k == p]) for p in partitions}


# ------------------------------------------------------------- wide sorts --
SORT_KEYS = (0, 1, 254, 255, 256, 257, 511, 512, 65_534, 65_535, 65_536, 65_537)
SORT_P = (255, 256, 257, 65_535, 65_536, 70_000)
SORT_TILE = 2048
SORT_SEED = 23
SORT_LO, SORT_HI = -3.0, 9.0
TILE_EDGE_P, TILE_EDGE_N = 300, (2_047, 2_048, 2_049)


def partition_passes(P):
    """8-bit passes over the partition key, whose largest value is P (not kept)."""
    return -(-max(1, int(P).bit_length()) // 8)


@functools.lru_cache(maxsize=None)
def sort_table(P, n=6000):
    """(pid, pk, values): n shuffled rows, every row an id of its own, over the
    partitions of SORT_KEYS below P and P - 1; one of them (P - 1) holds 2,500
    rows (a third of a smaller table), more than a tile; about 3 % of the
    values are NaN, the rest spread a little beyond [SORT_LO, SORT_HI]."""
    rng = np.random.default_rng(1000 + P + n)
    keys = np.array(sorted({k for k in SORT_KEYS + (P - 1,) if k < P}), dtype=np.int64)
    heavy = 2500 if n >= 6000 else n // 3
    pk = np.concatenate([np.full(heavy, P - 1, dtype=np.int64), rng.choice(keys, n - heavy)])
    values = rng.uniform(SORT_LO - 0.5, SORT_HI + 0.5, n)
    values[rng.random(n) < 0.03] = math.nan
    perm = rng.permutation(n)
    pk, values = pk[perm], values[perm]
    check_sort_table(P, pk, values)
    return np.arange(n, dtype=np.int64), pk, values


def check_sort_table(P, pk, values):
    n = len(pk)
    assert n > SORT_TILE - 2 and ((pk >= 0) & (pk < P)).all()
    kept = pk[~np.isnan(values)]
    assert np.isnan(values).any()  # the not-kept key P is among the sort's keys
    all_keys = np.concatenate([kept, [P]])
    for byte in range(partition_passes(P)):
        assert len(set(((all_keys >> (8 * byte)) & 0xFF).tolist())) > 1, f"byte {byte} is constant"
    for byte in range(3):  # the kept keys alone, in every byte the largest of them (P - 1) reaches
        if (P - 1) >> (8 * byte):
            assert len(set(((kept >> (8 * byte)) & 0xFF).tolist())) > 1, f"kept keys: byte {byte} is constant"
    if n >= 6000:  # a partition longer than a tile, spread over every tile
        where = np.flatnonzero(pk == P - 1)
        assert len(where) >= 2500 > SORT_TILE and len(set((where // SORT_TILE).tolist())) == -(-n // SORT_TILE) == 3
    # equal (partition, leaf) records exist, so a pass that is not stable cannot be told by them; what stability
    # protects is the leaf order inside a partition, and that is what the comparison reads
    leaf = Q.leaf_index(values[~np.isnan(values)], SORT_LO, SORT_HI)
    assert len(set(leaf[kept == P - 1].tolist())) > 100


def sort_walk_index(P, pk, values):
    """Occupied partitions and three empty ones (a low, a middle and a high
    free key), shuffled: what the wide-sort test walks."""
    occ = sorted(set(pk[~np.isnan(values)].tolist()))
    free = [p for p in (2, P // 2, P - 2, P - 3, 3) if p not in occ and 0 <= p < P][:3]
    assert len(free) == 3, free
    idx = np.array(occ + free, dtype=np.int64)
    return idx[np.random.default_rng(P).permutation(len(idx))]


# ----------------------------------------------------------- sampled rows --
SAMPLED = dict(U=300, P=40)
SAMPLED_SEED = 0x51A3_0000_0077
SAMPLED_CASES = {  # name: l0, linf, row_offset, masked
    "l0_1_linf_1": (1, 1, 0, False),
    "l0_3_linf_2": (3, 2, 0, False),
    "l0_12_linf_5": (12, 5, 0, False),
    "l0_3_linf_none": (3, BIG, 0, False),
    "row_offset_1e9": (3, 2, 10**9, False),
    "masked": (3, 2, 0, True),
}


@functools.lru_cache(maxsize=None)
def sampled_table():
    """(pid, pk, values, allowed): 300 ids with 1 ... 12 partitions of 40 each
    and 1 ... 40 rows per pair (a geometric law, and ten pairs of exactly 40),
    about 6,000 shuffled rows.  Row i's value lies in a leaf no other row
    shares, so a tree says *which* rows it holds; 2 % are NaN.  allowed hides
    a third of the partitions."""
    rng = np.random.default_rng(300)
    U, P = SAMPLED["U"], SAMPLED["P"]
    pid, pk = [], []
    for u in range(U):
        for j, k in enumerate(rng.choice(P, int(rng.integers(1, 13)), replace=False).tolist()):
            rows = 40 if (u < 10 and j == 0) else min(40, int(rng.geometric(0.32)))
            pid += [u] * rows
            pk += [k] * rows
    pid, pk = np.array(pid, dtype=np.int64), np.array(pk, dtype=np.int64)
    n = len(pid)
    perm = rng.permutation(n)
    pid, pk = pid[perm], pk[perm]
    values = (rng.permutation(Q.L)[:n] + 0.5) / Q.L
    values[rng.random(n) < 0.02] = math.nan
    allowed = (np.arange(P) % 3 != 1).astype(np.uint8)
    check_sampled_table(pid, pk, values, allowed)
    return pid, pk, values, allowed


def check_sampled_table(pid, pk, values, allowed):
    U, P = SAMPLED["U"], SAMPLED["P"]
    n = len(pid)
    assert 5000 <= n <= 7000, n
    ok = ~np.isnan(values)
    leaf = Q.leaf_index(values[ok], 0.0, 1.0)
    assert len(set(leaf.tolist())) == int(ok.sum())  # every row in a leaf of its own
    pairs, per_pair = np.unique(np.stack([pid, pk], axis=1), axis=0, return_counts=True)
    per_id = np.bincount(pairs[:, 0], minlength=U)
    assert per_id.min() >= 1 and per_id.max() == 12 and per_pair.max() == 40
    assert int((~allowed.astype(bool)).sum()) == (P + 1) // 3


@functools.lru_cache(maxsize=None)
def sampled_kept(case):
    """kept_rows of sampled_table under SAMPLED_CASES[case], computed once."""
    pid, pk, values, allowed = sampled_table()
    l0, linf, row_offset, masked = SAMPLED_CASES[case]
    return kept_rows(pid, pk, P=SAMPLED["P"], U=SAMPLED["U"], l0=l0, linf=linf, seed=SAMPLED_SEED,
                     row_offset=row_offset, allowed=allowed if masked else None)


def check_sampled_case(case):
    """The case samples what it is there for: at least 100 pairs truncated by
    linf, at least 50 ids that lose a partition to l0 (none at l0 = 12, the
    linf-only case), a kept NaN row, under the mask at least 10 ids keeping a
    partition they lose without it, and another kept set under the other
    row_offset."""
    pid, pk, values, allowed = sampled_table()
    l0, linf, row_offset, masked = SAMPLED_CASES[case]
    kept = sampled_kept(case)
    live = np.ones(len(pid), dtype=bool) if not masked else allowed.astype(bool)[pk]
    assert np.isnan(values[kept]).any()
    kp = kept_partitions(pid, pk, kept)
    before = kept_partitions(pid, pk, np.flatnonzero(live))
    lose = sum(1 for u in before if len(kp[u]) < len(before[u]))
    assert all(len(kp[u]) == min(l0, len(before[u])) for u in before)
    assert lose >= 50 if l0 < 12 else lose == 0, lose
    if linf < BIG:
        full = {}
        for u, k in zip(pid[live].tolist(), pk[live].tolist()):
            full[(u, k)] = full.get((u, k), 0) + 1
        got = {}
        for u, k in zip(pid[kept].tolist(), pk[kept].tolist()):
            got[(u, k)] = got.get((u, k), 0) + 1
        assert all(c == min(linf, full[key]) for key, c in got.items())
        assert sum(1 for key in got if full[key] > linf) >= 100
    else:
        assert len(kept) == sum(int(((pid == u) & (pk == k)).sum()) for u, ks in kp.items() for k in ks)
    if masked:  # hidden partitions take no l0 slot: ids keep partitions they lose without the mask
        plain = kept_partitions(pid, pk, sampled_kept("l0_3_linf_2"))
        assert not any(k for ks in kp.values() for k in ks if not allowed[k])
        assert sum(1 for u in kp if not kp[u] <= plain[u]) >= 10
    if row_offset:
        other = sampled_kept("l0_3_linf_2")
        assert len(other) == len(kept) and not np.array_equal(other, kept)
        assert kept_partitions(pid, pk, other) == kp  # the pairs' sampling does not read the row offset


# --------------------------------------------------------- integer column --
INT_RANGES = ((-5.0, 3.0), (-1e18, 1e18))


def int_table(lo, hi):
    """(pid, pk, values int64): two partitions holding the int64 extremes, the
    neighbours of 2^53 (not representable in fp64), the range's ends and
    their outer neighbours, and 200 random integers around the range."""
    rng = np.random.default_rng(53)
    i64 = np.iinfo(np.int64)
    ilo, ihi = int(lo), int(hi)
    edge = [i64.min, i64.max, 2**53 + 1, -(2**53 + 1), ilo, ihi, ilo - 1, ihi + 1]
    span = ihi - ilo
    rnd = [ilo - span // 4 + int(x * (span + span // 2)) for x in rng.random(200)]
    values = np.array(edge + edge + rnd, dtype=np.int64)
    pk = np.array([0] * len(edge) + [1] * len(edge) + rng.integers(0, 2, len(rnd)).tolist(), dtype=np.int64)
    f = values.astype(np.float64)
    assert (f < lo).any() and (f > hi).any() and ((f > lo) & (f < hi)).any() and (f == lo).any() and (f == hi).any()
    assert int(f[2]) != 2**53 + 1  # the conversion rounds
    return np.arange(len(values), dtype=np.int64), pk, values
