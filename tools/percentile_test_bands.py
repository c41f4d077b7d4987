"""Recomputes, on the CPU, the constants recorded in tests/test_gpu_percentile.py:
the budget of the one-noisy-tree test and the accepted bands of the noise-scale
test.  Uses only the NumPy restatement (tests/quantile_tree_util.py) with NumPy
noise; nothing here touches a GPU.

    python tools/percentile_test_bands.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import quantile_tree_util as Q  # noqa: E402


def monotone_violations(eps, n_partitions=32, n_values=200, seed=1):
    """Fraction of partitions whose 64 ascending ranks come out of order when
    every rank draws its own noise (what the specification rules out)."""
    rng = np.random.default_rng(seed)
    scale = Q.noise_scale("laplace", eps, 0.0, 1, 1)
    ranks = np.linspace(0.0, 1.0, 64)
    bad = 0
    for _ in range(n_partitions):
        t = Q.Tree(0.0, 1.0, rng.uniform(0, 1, n_values))
        out = t.quantiles(ranks, Q.numpy_noise(rng, "laplace", scale), shared=False)
        bad += any(x > y for x, y in zip(out, out[1:]))
    return bad / n_partitions


def median_mae_band(kind, eps, delta, n_partitions=256, n_values=2000, seeds=24, data_seed=7):
    """Per-seed mean absolute error of the median over n_partitions noisy trees
    of the same values; the band is [min - m, max + m], m = 3 sample standard
    deviations of the per-seed figures."""
    values = np.random.default_rng(data_seed).uniform(0.0, 1.0, n_values)
    tree = Q.Tree(0.0, 1.0, values)
    truth = tree.quantiles([0.5])[0]
    scale = Q.noise_scale(kind, eps, delta, 1, 1)
    maes = []
    for s in range(seeds):
        rng = np.random.default_rng(1000 + s)
        noise = Q.numpy_noise(rng, kind, scale)
        maes.append(np.mean([abs(tree.quantiles([0.5], noise)[0] - truth) for _ in range(n_partitions)]))
    maes = np.array(maes)
    m = 3.0 * maes.std(ddof=1)
    return dict(kind=kind, eps=eps, delta=delta, scale=scale, seeds=seeds, min=maes.min(), max=maes.max(),
                mean=maes.mean(), std=maes.std(ddof=1), band=(maes.min() - m, maes.max() + m))


if __name__ == "__main__":
    for eps in (2.0, 1.0, 0.5, 0.25):
        print("monotone: eps", eps, "violating fraction", monotone_violations(eps))
    print(median_mae_band("laplace", 0.2, 0.0))
    print(median_mae_band("gaussian", 0.2, 1e-6))
