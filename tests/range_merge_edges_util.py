"""Tables that put the range merge (csrc/pdp_bound_merge.hip) on its edges.

Shared by tests/test_range_merge_edges_host.py (CPU) and
tests/test_gpu_range_merge_edges.py (GPU).

With l0 >= the partitions of every privacy id and linf = 0 nothing is sampled:
the bucket kernel emits one record per distinct (privacy id, partition) pair,
into the run of (bucket, range) = (id >> bucket_bits, partition >> range_bits).
build_table() takes the record count of every such cell and deals the pairs out
over the bucket's ids, so a table decides where k_range_plan cuts, which items
k_range_reduce / k_fine_reduce add directly, how long a round of the staged
scatter is and what each fine range holds.  Values are dyadic
(tests/value_edges_util.py), so every fp64 sum is exact in any order and the
expected accumulators -- plain NumPy over the pair list and the rows -- are
compared by equality.

plan_items() and fine_items() restate the work-item rules from the comments
of pdp_bound_merge.hip (not from the kernel bodies); the device does not expose
its items, so the host test proves with these that a shape reaches its edge.
"""
import dataclasses
import os
import re

import numpy as np

from oracle import columnar as O
from tests import value_edges_util as VU

# mirrors of csrc/pdp_bound_plan.h and csrc/pdp_bound_merge.hip
# (header_constants() reads the sources; the host test holds these to them)
C = 8192            # kRangeChunk: records per work item
D = 256             # kRangeDirect: an item below it adds straight to the accumulators
R = 2048            # kSplitStageRows: records per round of item_rounds (4 per thread)
RANGE_BITS = 11     # kRangeBits: partitions per (fine) merge range = 2048
STAGE_FAN = 256     # kSplitStageFan: more fine ranges per coarse range -> the unstaged scatter
COARSE_RANGES = 256  # kCoarseRanges
MAX_RANGES = 1024   # kMaxRanges: more fine ranges -> two levels
LDS_BUDGET = 124 * 1024  # kLdsBudget: the per-id state of one bucket
RANGE_THREADS = 1024     # kRangeThreads: buckets per batch of k_range_plan
REDUCE_THREADS = 512     # kReduceThreads = kSplitThreads: buckets per batch of the reduce / split kernels

L0, LINF = 4, 0
F_ALL = O.ACC_SUM | O.ACC_NSUM | O.ACC_NSUM2
VARIANTS = {"f64": (O.VALUE_F64, F_ALL), "i64": (O.VALUE_I64, F_ALL | O.SUM_INT), "none": (O.VALUE_NONE, 0)}

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pipelinedp_amd", "csrc")


def header_constants():
    """The constexpr integers of pdp_bound_plan.h and pdp_bound_merge.hip by name."""
    text = ""
    for name in ("pdp_bound_plan.h", "pdp_bound_merge.hip"):
        with open(os.path.join(_CSRC, name)) as f:
            text += f.read()
    raw = dict(re.findall(r"constexpr\s+(?:unsigned|int64_t|int|size_t)\s+(k\w+)\s*=\s*([^;]+);", text))
    out = {}

    def value(name, depth=0):
        if name not in out:
            expr = re.sub(r"\((?:unsigned|int64_t|int|size_t)\)", "", raw[name])
            expr = re.sub(r"k\w+", lambda m: str(value(m.group(0), depth + 1)), expr)
            if depth > 8 or not re.fullmatch(r"[0-9 ()*+\-<]+", expr):
                raise ValueError(f"{name} = {raw[name]!r} is no integer expression")
            out[name] = int(eval(expr, {"__builtins__": {}}))  # digits, + - * << and parentheses only
        return out[name]

    for name in ("kRangeChunk", "kRangeDirect", "kSplitStageRows", "kRangeBits", "kSplitStageFan", "kCoarseRanges",
                 "kMaxRanges", "kLdsBudget", "kRangeThreads", "kReduceThreads", "kSplitThreads"):
        value(name)
    return out


# ---------------------------------------------------------------- geometry --
@dataclasses.dataclass(frozen=True)
class Geometry:
    """What a table needs of a plan (pdp_bound_plan) and its configuration."""
    U: int
    P: int
    l0: int
    bucket_bits: int
    n_buckets: int
    n_ranges: int
    range_bits: int       # partitions per range of the bucket kernel's runs
    n_fine: int           # ceil(P / 2^RANGE_BITS)
    two_level: bool       # n_ranges < n_fine: coarse ranges, then fine ranges
    fine_per_coarse: int  # 2^(range_bits - RANGE_BITS)

    @property
    def pair_slots(self):
        return self.l0 << self.bucket_bits

    def range_span(self, r):
        """[lo, hi): the partitions of range r."""
        lo = r << self.range_bits
        return lo, min(self.P, lo + (1 << self.range_bits))

    def fine_span(self, r, f):
        """[lo, hi): the partitions of fine range f of coarse range r."""
        lo = (r << self.range_bits) + (f << RANGE_BITS)
        return lo, min(self.P, lo + (1 << RANGE_BITS))


def geometry(plan, U, P, l0=L0):
    n_fine = -(-P // (1 << RANGE_BITS))
    rb = RANGE_BITS
    while -(-P // (1 << rb)) > plan.n_ranges:
        rb += 1
    if -(-P // (1 << rb)) != plan.n_ranges:
        raise ValueError(f"n_ranges = {plan.n_ranges} is no ceil(P / 2^k) for P = {P}")
    if plan.n_buckets != -(-U // (1 << plan.bucket_bits)):
        raise ValueError("n_buckets is not ceil(U / 2^bucket_bits)")
    return Geometry(U, P, l0, int(plan.bucket_bits), int(plan.n_buckets), int(plan.n_ranges), rb, n_fine,
                    plan.n_ranges < n_fine, 1 << (rb - RANGE_BITS))


# ------------------------------------------------------------------- cells --
@dataclasses.dataclass(frozen=True)
class Cell:
    bucket: int
    range: int
    n_pairs: int
    placement: tuple  # ("spread", lo, hi): over partitions [lo, hi), its first and last included; ("hot", p)


def spread(geom, r):
    return ("spread",) + geom.range_span(r)


def fine(geom, r, f):
    return ("spread",) + geom.fine_span(r, f)


def hot(p):
    return ("hot", int(p))


def _candidates(geom, r, placement):
    """The partitions a cell deals out, in order; all inside range r."""
    if placement[0] == "hot":
        cand = np.array([placement[1]], dtype=np.int64)
    else:
        lo, hi = placement[1], placement[2]
        if hi <= lo:
            raise ValueError(f"empty span {placement}")
        # evenly spaced, the span's first and last partition among them
        cand = lo + np.unique(np.round(np.linspace(0, hi - lo - 1, min(hi - lo, 61))).astype(np.int64))
    if (cand >> geom.range_bits != r).any() or cand.max() >= geom.P:
        raise ValueError(f"{placement} leaves range {r}")
    return cand


def pour(geom, free, r, total, placement, bucket, per_bucket=None):
    """Cells that put `total` pairs of range r into buckets `bucket`, bucket +
    1, ...: per_bucket in each (default: the pair slots the bucket has left;
    `free` maps bucket -> free slots and is updated).  Returns (cells, the
    first bucket not filled up)."""
    cells = []
    while total > 0:
        room = free.setdefault(bucket, geom.pair_slots)
        n = min(total, room if per_bucket is None else min(per_bucket, room))
        if n > 0:
            cells.append(Cell(bucket, r, n, placement))
            free[bucket] = room - n
            total -= n
        if total > 0 or free[bucket] == 0:
            bucket += 1
    return cells, bucket


@dataclasses.dataclass
class Table:
    geom: Geometry
    value_kind: int
    flags: int
    bounds: VU.Bounds
    pid: np.ndarray       # rows, shuffled
    pk: np.ndarray
    val: np.ndarray       # None for VALUE_NONE
    pair_pid: np.ndarray  # the distinct (privacy id, partition) pairs = the bucket kernel's records
    pair_pk: np.ndarray

    def run_lengths(self):
        """[range][bucket] -> records, the run table k_range_plan reads."""
        g = self.geom
        runs = np.zeros((g.n_ranges, g.n_buckets), dtype=np.int64)
        np.add.at(runs, (self.pair_pk >> g.range_bits, self.pair_pid >> g.bucket_bits), 1)
        return runs

    def fine_totals(self):
        return np.bincount(self.pair_pk >> RANGE_BITS, minlength=self.geom.n_fine)

    def row_terms(self):
        """Per row, what it adds to sum / normalized_sum / normalized_sum_sq
        (None: the field is off); every term a multiple of 2^-6."""
        b, flags = self.bounds, self.flags
        terms = dict.fromkeys(VU.FIELDS)
        if self.val is None:
            return terms
        clipped = np.clip(self.val.astype(np.float64), b.lo, b.hi)
        if flags & O.ACC_SUM:
            terms["sum"] = np.clip(self.val, int(b.lo), int(b.hi)) if flags & O.SUM_INT else clipped
        if flags & O.ACC_NSUM:
            terms["normalized_sum"] = clipped - b.mid
        if flags & O.ACC_NSUM2:
            terms["normalized_sum_sq"] = (clipped - b.mid) ** 2
        return terms

    def expected(self):
        """The accumulators, dense over P (host arrays: small P only)."""
        P = self.geom.P
        want = {"privacy_id_count": np.bincount(self.pair_pk, minlength=P).astype(np.int64),
                "count": np.bincount(self.pk, minlength=P).astype(np.int64)}
        for k, t in self.row_terms().items():
            want[k] = np.zeros(P, dtype=np.int64 if k == "sum" and self.flags & O.SUM_INT else np.float64)
            if t is not None:
                np.add.at(want[k], self.pk, t)
        return want


def build_table(geom, cells, value_kind, flags, seed=1, b=None):
    """Deals each cell's pairs out over its bucket's ids -- at most l0
    partitions per id over all cells of the bucket, distinct per id -- gives
    every pair 1 to 3 rows with dyadic values and shuffles the rows."""
    b = b or VU.bounds_for(value_kind)
    rng = np.random.default_rng(seed)
    held = {}   # bucket -> partitions per id so far
    taken = {}  # privacy id -> its partitions
    pair_pid, pair_pk = [], []
    for cell in cells:
        first = cell.bucket << geom.bucket_bits
        n_ids = min(1 << geom.bucket_bits, geom.U - first)
        if not (0 <= cell.bucket < geom.n_buckets and 0 <= cell.range < geom.n_ranges and n_ids > 0):
            raise ValueError(f"{cell} is outside the plan")
        cnt = held.setdefault(cell.bucket, [0] * n_ids)
        cand = _candidates(geom, cell.range, cell.placement)
        t, left = 0, cell.n_pairs
        for j in range(n_ids):
            m = min(geom.l0 - cnt[j], len(cand), left)
            if m <= 0:
                continue
            ps = [int(cand[(t + q) % len(cand)]) for q in range(m)]
            mine = taken.setdefault(first + j, set())
            if mine.intersection(ps):
                raise ValueError(f"{cell}: cells of one bucket and range must not share partitions")
            mine.update(ps)
            pair_pid += [first + j] * m
            pair_pk += ps
            cnt[j] += m
            t += m
            left -= m
            if left == 0:
                break
        if left:
            raise ValueError(f"{cell}: the bucket's ids hold {left} pairs fewer")
    pair_pid = np.array(pair_pid, dtype=np.int64)
    pair_pk = np.array(pair_pk, dtype=np.int64)
    rows = rng.integers(1, 4, len(pair_pid))
    perm = rng.permutation(int(rows.sum()))
    pid, pk = np.repeat(pair_pid, rows)[perm], np.repeat(pair_pk, rows)[perm]
    val = VU.dyadic_values(rng, len(pid), value_kind, b)
    # exactness over the populated partitions only (P may be 2^27)
    _, dense = np.unique(pk, return_inverse=True)
    VU.check_exact(dense, val, int(dense.max(initial=0)) + 1, b)
    return Table(geom, value_kind, flags, b, pid, pk, val, pair_pid, pair_pk)


# ------------------------------------------------------------------ models --
def plan_items(run_lengths, chunk=C):
    """k_range_plan's work items from run_lengths[range][bucket], as the comment
    above it states them: range r's records, taken bucket-major, are cut at
    bucket boundaries -- a new item starts after the bucket that holds record
    position k * chunk (k >= 1, positions counted from 1) -- into K_r =
    ceil(total_r / chunk) items, the last of which ends with the range.
    -> [(range, first bucket, end bucket, records)], empty items included (a
    position in the range's last populated bucket leaves the item after it
    empty; the reduce kernels return on those)."""
    items = []
    for r, runs in enumerate(run_lengths):
        runs = [int(x) for x in runs]
        total = sum(runs)
        if total == 0:
            continue
        K = -(-total // chunk)
        ends, e = [], 0
        for x in runs:
            e += x
            ends.append(e)
        entry = [(0, 0)]  # (first bucket, records before it)
        for k in range(1, K + 1):
            if k * chunk <= total:
                holder = next(i for i, e in enumerate(ends) if e >= k * chunk)
                entry.append((holder + 1, ends[holder]))
            else:  # k == K, total no multiple of chunk: the range's end
                entry.append((len(runs), total))
        for k in range(K):
            items.append((r, entry[k][0], entry[k + 1][0], entry[k + 1][1] - entry[k][1]))
    return items


def fine_items(fine_totals, chunk=C):
    """k_fine_plan's work items: fine range f's records in chunks of `chunk`.
    -> [(fine range, first record within the range, records)]"""
    items = []
    for f, total in enumerate(fine_totals):
        total = int(total)
        items += [(f, a, min(chunk, total - a)) for a in range(0, total, chunk)]
    return items


# ------------------------------------------------------------------ shapes --
P_SINGLE = 3 * 2048 + 5      # 4 ranges, the last of 5 partitions
P_STAGED = 2_097_153         # the smallest two-level P: 1,025 fine ranges, the last of one partition
P_UNSTAGED = (1 << 27) + 1   # 512 fine ranges per coarse range: over kSplitStageFan


def _s1(g):
    # one item per range: D - 1 (direct), D (LDS), none, D + 1 in the 5-partition range
    return [Cell(0, 0, D - 1, spread(g, 0)), Cell(0, 1, D, spread(g, 1)), Cell(1, 3, D + 1, spread(g, 3))]


def _s2(g):
    # totals C (4 full buckets), 2C, C + 1, C - 1; buckets 21.. stay empty
    free, cells, b = {}, [], 0
    for r, total in enumerate((C, 2 * C, C + 1, C - 1)):
        got, b = pour(g, free, r, total, spread(g, r), b)
        cells += got
        b += 1 if free.get(b, g.pair_slots) < g.pair_slots else 0  # the next range starts a bucket of its own
    return cells


def _s3(g):
    # runs of 2,047: position C falls inside the fifth bucket.  Range 0: ten
    # buckets, items of 5, 4 and 1 buckets; range 1: nine, the third item empty
    free = {}
    cells, b = pour(g, free, 0, 10 * (g.pair_slots - 1), spread(g, 0), 0, per_bucket=g.pair_slots - 1)
    more, b = pour(g, free, 1, 9 * (g.pair_slots - 1), spread(g, 1), b + 1, per_bucket=g.pair_slots - 1)
    return cells + more + [Cell(b + 1, 3, 3, spread(g, 3))]


def _s4(g):
    # 3C records on one partition (every id of 48 buckets once) beside a cold range
    ids = 1 << g.bucket_bits
    cells, b = pour(g, {}, 1, 3 * C, hot(g.range_span(1)[0] + 777), 0, per_bucket=ids)
    return cells + [Cell(b + 1, 0, 10, spread(g, 0))]


def _s5(g):
    # runs only in buckets 0, 511, 512, 1023, 1024 and the last (one id).
    # Range 0: 7,096 records before bucket 1024 (k_range_plan's carry into its
    # second batch), position C inside it; its first item spans three reduce
    # batches.  Range 1: one item over buckets 511 | 512
    last = g.n_buckets - 1
    s = g.pair_slots
    return [Cell(0, 0, s, spread(g, 0)), Cell(511, 0, 1500, spread(g, 0)), Cell(512, 0, 1500, spread(g, 0)),
            Cell(1023, 0, s, spread(g, 0)), Cell(1024, 0, s, spread(g, 0)), Cell(last, 0, 2, spread(g, 0)),
            Cell(511, 1, s - 1500, spread(g, 1)), Cell(512, 1, s - 1500, spread(g, 1)),
            Cell(last, 3, 2, spread(g, 3))]


def _t1(fines):
    def cells(g):
        # one coarse range with records in the given fine ranges only; the last
        # coarse range: the single fine range of one partition, P - 1
        out, r = [], 5
        for i, f in enumerate(fines):
            out += [Cell(0, r, 150 + 37 * i, fine(g, r, f)), Cell(1, r, 200 + 11 * i, fine(g, r, f))]
        last = g.n_ranges - 1
        assert g.range_span(last) == (g.P - 1, g.P)
        return out + [Cell(2, last, 300, hot(g.P - 1)), Cell(3, last, 5, hot(g.P - 1))]
    return cells


def _t2(fines):
    def cells(g):
        # fine totals D - 1, D, C, C + 1, 2C in one coarse range, bucket after bucket
        free, out, b = {}, [], 0
        for f, total in zip(fines, (D - 1, D, C, C + 1, 2 * C)):
            got, b = pour(g, free, 3, total, fine(g, 3, f), b)
            out += got
        return out
    return cells


def _t3(g):
    # coarse items of R and R + 1 records: in one fine range, and over all of them
    s = g.pair_slots
    assert s == R
    return [Cell(0, 10, R, fine(g, 10, 4)), Cell(1, 11, R, spread(g, 11)),
            Cell(2, 12, R, fine(g, 12, 7)), Cell(3, 12, 1, fine(g, 12, 7)),
            Cell(4, 13, R, spread(g, 13)), Cell(5, 13, 1, spread(g, 13))]


# name -> (U, P, cells(geometry))
SHAPES = {
    "S1-direct-switch": (3 * 512, P_SINGLE, _s1),
    "S2-exact-multiples": (24 * 512, P_SINGLE, _s2),
    "S3-overshoot": (22 * 512, P_SINGLE, _s3),
    "S4-hot-partition": (49 * 512 + 100, P_SINGLE, _s4),
    "S5-batch-edges": (1025 * 512 + 1, P_SINGLE, _s5),
    "T1-staged-fine-0-7-last": (4 * 512, P_STAGED, _t1((0, 7))),
    "T2-staged-fine-totals": (18 * 512, P_STAGED, _t2((1, 2, 3, 4, 5))),
    "T3-staged-rounds": (6 * 512, P_STAGED, _t3),
    "U1-unstaged-fine-edges": (4 * 512, P_UNSTAGED, _t1((0, 255, 256, 511))),
    "U2-unstaged-fine-totals": (18 * 512, P_UNSTAGED, _t2((1, 255, 256, 300, 511))),
}
SINGLE = [s for s in SHAPES if s[0] == "S"]
STAGED = [s for s in SHAPES if s[0] == "T"]
UNSTAGED = [s for s in SHAPES if s[0] == "U"]


# what pdp_bound_plan says of every shape: (n_buckets, n_ranges, two_level, fine ranges per coarse range)
PLANS = {
    "S1-direct-switch": (3, 4, False, 1), "S2-exact-multiples": (24, 4, False, 1), "S3-overshoot": (22, 4, False, 1),
    "S4-hot-partition": (50, 4, False, 1), "S5-batch-edges": (1026, 4, False, 1),
    "T1-staged-fine-0-7-last": (4, 129, True, 8), "T2-staged-fine-totals": (18, 129, True, 8),
    "T3-staged-rounds": (6, 129, True, 8),
    "U1-unstaged-fine-edges": (4, 129, True, 512), "U2-unstaged-fine-totals": (18, 129, True, 512),
}


def assert_plan(shape, t, plan):
    """The plan a shape was laid out for (the host test pins it; the GPU test
    refuses to run on another)."""
    g = t.geom
    n_buckets, n_ranges, two_level, per_coarse = PLANS[shape]
    assert (plan.algorithm, plan.merge) == (2, 2)  # BUCKETED, PDP_MERGE_RANGES
    assert plan.sieve == 0 and plan.band == 0 and plan.fix_ids == 0  # one record segment, no flat pair list
    assert plan.bucket_bits == 9 and g.pair_slots == R
    assert (plan.n_buckets, plan.n_ranges) == (n_buckets, n_ranges)
    assert g.two_level == two_level == (plan.n_ranges < -(-g.P // (1 << RANGE_BITS)))
    assert g.fine_per_coarse == per_coarse


def spec_for(variant, b=None):
    from pipelinedp_amd import executor as X
    vk, flags = VARIANTS[variant]
    b = b or VU.bounds_for(vk)
    return X.BoundingSpec(l0=L0, linf=LINF, value_kind=vk, flags=flags, min_value=b.lo, max_value=b.hi,
                          middle=b.mid, min_sum=b.min_sum, max_sum=b.max_sum)


_tables = {}


def shape_table(shape, variant):
    """(table, plan) of a shape, built once and never written to (drop_tables()
    forgets them: the test files call it when they are done, so nothing large
    stays behind for the rest of a run).  The cells are laid out on the
    geometry of the plan for a guessed row count; the plan for the table's own
    row count must have the same geometry."""
    from pipelinedp_amd import executor as X
    key = (shape, variant)
    if key not in _tables:
        U, P, cells = SHAPES[shape]
        spec = spec_for(variant)
        g = geometry(X.bound_plan(50_000, U, P, spec, 2, 2), U, P)
        vk, flags = VARIANTS[variant]
        t = build_table(g, cells(g), vk, flags, seed=sorted(SHAPES).index(shape) + 11)
        plan = X.bound_plan(len(t.pid), U, P, spec, 2, 2)
        if geometry(plan, U, P) != g:
            raise ValueError(f"{shape}: the plan's geometry depends on the row count")
        _tables[key] = (t, plan)
    return _tables[key]


def drop_tables():
    _tables.clear()
