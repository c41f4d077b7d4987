"""A NumPy restatement of the PERCENTILE quantile tree (DESIGN.md §3,
"PERCENTILE"), independent of pipelinedp_amd/quantile_tree.py: the tree is a
dense histogram of the 65,536 leaves folded level by level, not a sorted leaf
array.  Shared by tests/test_percentile_host.py and tests/test_gpu_percentile.py.

Every operation of the walk is a NumPy float64 operation, written in the order
the specification gives, so that the GPU kernel (compiled without
floating-point contraction) can be compared with it by equality.
"""
import math

import numpy as np

H = 4
B = 16
L = B**H                                   # 65,536 leaves
FIRST = [(B**lv - 1) // (B - 1) for lv in range(H + 2)]  # first node index of level lv
FIRST_LEAF = FIRST[H]                      # 4,369
NODES = FIRST[H + 1] - 1                   # 69,904 counted nodes
TOL = 1e-6

f64 = np.float64


def leaf_index(values, lo, hi):
    """Leaves of the values that are not NaN, in input order (int64)."""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    v = np.where(v < lo, f64(lo), np.where(v > hi, f64(hi), v))
    x = (v - f64(lo)) / (f64(hi) - f64(lo)) * f64(L)
    return np.minimum(np.floor(x), L - 1).astype(np.int64)


class Tree:
    """Raw counts of every level: level[lv][pos], lv = 1 ... H."""

    def __init__(self, lo, hi, values=()):
        self.lo, self.hi = f64(lo), f64(hi)
        self.leaves = np.zeros(L, dtype=np.int64)
        self.insert(values)

    def insert(self, values):
        self.leaves += np.bincount(leaf_index(values, self.lo, self.hi), minlength=L)
        return self

    def merge(self, other):
        assert (self.lo, self.hi) == (other.lo, other.hi)
        self.leaves += other.leaves
        return self

    def raw(self, level, pos):
        span = B**(H - level)
        cum = np.concatenate([[0], np.cumsum(self.leaves)])  # cum[x] = values in leaves below x
        return int(cum[(pos + 1) * span] - cum[pos * span])

    def node_count(self, node):
        """Raw count of node index `node` (1 ... NODES)."""
        level = max(lv for lv in range(1, H + 1) if FIRST[lv] <= node)
        return self.raw(level, node - FIRST[level])

    def quantiles(self, ranks, noise=None, shared=True):
        """Values at `ranks`.  noise(node, raw) -> noised count (None: none).
        shared: one noised count per node for all ranks (the specification);
        not shared: every rank draws its own (used only to show what the
        specification rules out)."""
        memo = {}
        cum = np.concatenate([[0], np.cumsum(self.leaves)])

        def noised(level, pos):
            node = FIRST[level] + pos
            if shared and node in memo:
                return memo[node]
            span = B**(H - level)
            raw = float(cum[(pos + 1) * span] - cum[pos * span])
            x = f64(raw if noise is None else noise(node, raw))
            x = x if x > 0.0 else f64(0.0)
            memo[node] = x
            return x

        with np.errstate(all="ignore"):
            return [self._walk(f64(r), noised) for r in ranks]

    def _walk(self, r, noised):
        a, b = self.lo, self.hi
        pos = 0
        for level in range(1, H + 1):
            cnt = [noised(level, pos * B + k) for k in range(B)]
            total = f64(0.0)
            for c in cnt:
                total = total + c
            if total <= 0.0:
                break
            partial = f64(0.0)
            chosen = None
            for k in range(B):
                partial = partial + cnt[k]
                if partial / total >= r - TOL:
                    chosen = k
                    break
            if chosen is None:
                chosen = max(k for k in range(B) if cnt[k] > 0.0)
                partial = f64(0.0)
                for k in range(chosen + 1):
                    partial = partial + cnt[k]
            c = cnt[chosen]
            r = (r - (partial - c) / total) / (c / total)
            r = r if 0.0 < r else f64(0.0)   # clamp as min(max(0, r), 1): a NaN becomes 0
            r = f64(1.0) if 1.0 < r else r
            a, b = a + f64(chosen) * (b - a) / f64(16.0), a + f64(chosen + 1) * (b - a) / f64(16.0)
            pos = pos * B + chosen
        return float((f64(1.0) - r) * a + r * b)


def empty_answer(lo, hi, r):
    return float((f64(1.0) - f64(r)) * f64(lo) + f64(r) * f64(hi))


# ------------------------------------------------------------------ noise --
def noise_scale(kind, eps, delta, l0, linf):
    """Laplace b = L1 / eps with L1 = (l0 H) linf; Gaussian sigma for
    L2 = sqrt(l0 H) linf (the project's calibration, dp_computations.compute_sigma)."""
    from pipelinedp_amd import dp_computations as dpc
    if kind == "laplace":
        return (l0 * H) * linf / eps
    return dpc.compute_sigma(eps, delta, math.sqrt(l0 * H) * linf)


def numpy_noise(rng, kind, scale):
    """noise(node, raw) drawing NumPy Laplace / Gaussian noise of `scale`."""
    if kind == "laplace":
        return lambda node, raw: raw + rng.laplace(0.0, scale)
    return lambda node, raw: raw + rng.normal(0.0, scale)


# ---------------------------------------------------------------- bounder --
def kept_rows_by_partition(pid, pk, values, n_partitions, l0, linf, allowed=None):
    """The restatement's contribution bounder for bounds that nothing reaches:
    asserts that no privacy id has more than l0 partitions nor a pair more than
    linf rows, so that every row of an allowed partition is kept whatever the
    sampling seed, and returns {partition: values}."""
    pid, pk, values = np.asarray(pid), np.asarray(pk), np.asarray(values, dtype=np.float64)
    if allowed is not None:
        m = np.asarray(allowed, dtype=bool)[pk]
        pid, pk, values = pid[m], pk[m], values[m]
    pairs, per_pair = np.unique(np.stack([pid, pk], axis=1), axis=0, return_counts=True) if len(pid) else \
        (np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert per_pair.max(initial=0) <= linf, "a pair exceeds linf: the comparison would depend on sampling"
    assert np.bincount(pairs[:, 0]).max(initial=0) <= l0, "an id exceeds l0: the comparison would depend on sampling"
    return {p: values[pk == p] for p in range(n_partitions)}


def expected(pid, pk, values, n_partitions, lo, hi, ranks, l0, linf, allowed=None):
    """[n_partitions, len(ranks)] noise-free answers of the restatement."""
    rows = kept_rows_by_partition(pid, pk, values, n_partitions, l0, linf, allowed)
    return np.array([Tree(lo, hi, rows[p]).quantiles(ranks) for p in range(n_partitions)], dtype=np.float64)
