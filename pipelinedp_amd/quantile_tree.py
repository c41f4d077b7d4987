"""The DP quantile tree of PERCENTILE on the host, in NumPy.

The reference's QuantileCombiner (pipeline_dp/combiners.py:590-669) delegates
the tree to PyDP's C++ QuantileTree.  This module restates that algorithm
("PERCENTILE"; not compared against PyDP output) for the
row-wise QuantileCombiner; the ColumnarBackend runs the same arithmetic, in the
same order, in csrc/pdp_quantiles.hip.

A tree over [lo, hi] of height 4 and branching factor 16: node 0 is the root
(never counted), the children of node i are 16 i + 1 ... 16 i + 16, level l has
16^l nodes and the 65,536 leaves are level 4.  A node's raw count is the
number of inserted values whose leaf lies below it, so the tree is held as
the array of the values' leaf codes.
"""
from typing import Callable, Iterable, List

import numpy as np

HEIGHT = 4
BRANCH = 16
N_LEAVES = BRANCH**HEIGHT
NUMERICAL_TOLERANCE = 1e-6


def level_first(level: int) -> int:
    """Index of the first node of `level` (0 = the root)."""
    return (BRANCH**level - 1) // (BRANCH - 1)


FIRST_LEAF = level_first(HEIGHT)
N_NODES = level_first(HEIGHT + 1) - 1  # counted nodes: every node but the root


def leaf_codes(values: Iterable[float], lo: float, hi: float) -> np.ndarray:
    """uint16 leaf of every value that is not NaN:
    min(L - 1, floor((clamp(v) - lo) / (hi - lo) * L)) in fp64, in this order."""
    v = np.asarray(list(values) if not isinstance(values, np.ndarray) else values, dtype=np.float64).ravel()
    v = v[~np.isnan(v)]
    v = np.minimum(np.maximum(v, np.float64(lo)), np.float64(hi))
    leaf = np.floor((v - np.float64(lo)) / (np.float64(hi) - np.float64(lo)) * np.float64(N_LEAVES))
    return np.minimum(leaf, N_LEAVES - 1).astype(np.uint16)


def compute_quantiles(leaves: np.ndarray, lo: float, hi: float, ranks: Iterable[float],
                      add_noise: Callable[[int, float], float] = None) -> List[float]:
    """The values at `ranks` (each in [0, 1]) of the tree holding `leaves`.

    add_noise(node, raw_count) -> noised count (None: no noise); a node's
    noised count max(0, add_noise(...)) is drawn once and shared by all ranks."""
    srt = np.sort(np.asarray(leaves, dtype=np.int64))
    memo = {}

    def noised(level, pos):
        node = level_first(level) + pos
        if node not in memo:
            span = BRANCH**(HEIGHT - level)
            raw = float(np.searchsorted(srt, (pos + 1) * span, side="left") -
                        np.searchsorted(srt, pos * span, side="left"))
            x = raw if add_noise is None else float(add_noise(node, raw))
            memo[node] = np.float64(x if x > 0.0 else 0.0)
        return memo[node]

    out = []
    with np.errstate(all="ignore"):
        for rank in ranks:
            r = np.float64(rank)
            a, b = np.float64(lo), np.float64(hi)
            pos = 0
            for level in range(1, HEIGHT + 1):
                counts = [noised(level, pos * BRANCH + k) for k in range(BRANCH)]
                total = np.float64(0.0)
                upto = []
                for c in counts:  # left to right
                    total = total + c
                    upto.append(total)
                if not total > 0.0:
                    break
                pick = next((k for k in range(BRANCH) if upto[k] / total >= r - NUMERICAL_TOLERANCE), None)
                if pick is None:  # rounding: the last child with a count
                    pick = max(k for k in range(BRANCH) if counts[k] > 0.0)
                t = (r - (upto[pick] - counts[pick]) / total) / (counts[pick] / total)
                t = t if 0.0 < t else np.float64(0.0)  # a NaN (a child without a count) becomes 0
                r = np.float64(1.0) if 1.0 < t else t
                w = b - a
                a, b = a + np.float64(pick) * w / 16.0, a + np.float64(pick + 1) * w / 16.0
                pos = pos * BRANCH + pick
            out.append(float((1.0 - r) * a + r * b))
    return out
