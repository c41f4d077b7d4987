"""TEST INFRASTRUCTURE — regenerate tests/golden/vector_sum/vector_sum.json from the reference.

Runs only where the reference checkout is present (REFERENCE below, or the
PIPELINEDP_REFERENCE environment variable); the fixture it writes is data only
and is what the tests read.  The reference imports with the python-dp stand-in
of oracle/pydp_standin on the path, as oracle/gen_golden.py does.

For each case the reference's DPEngine.aggregate runs on LocalBackend for
[VECTOR_SUM, COUNT, PRIVACY_ID_COUNT] with CompoundCombiner.compute_metrics
patched to return the raw accumulator and private partition selection patched
to keep every partition, on rows where no contribution sampling fires (every
privacy id has <= L0 partitions, every pair <= Linf rows), so the expected
(row_count, (count, privacy_id_count, vector)) per partition is deterministic.
The reference's DPEngine runs VECTOR_SUM end to end under the stand-in; nothing
is driven by hand.  The clipped vectors are the reference's own
dp_computations._clip_vector on those accumulators, for Linf / L1 / L2 with a
max_norm (the median of the partitions' norms) that clips some partitions and
not others, plus one all-zero vector.

Usage: python tools/gen_golden_vector_sum.py   (from the repository root)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("PIPELINEDP_REFERENCE", "/root/reference")
# a directory of its own: tests/golden_util.py reads every tests/golden/*.json as a scalar aggregate case
OUT = os.path.join(ROOT, "tests", "golden", "vector_sum", "vector_sum.json")

VECTOR_SIZE = 5
CASES = [
    dict(name="int_laplace", integer=True, noise="LAPLACE", l0=2, linf=2, n_pids=300, n_partitions=40, seed=11),
    dict(name="float_gaussian", integer=False, noise="GAUSSIAN", l0=3, linf=1, n_pids=300, n_partitions=40,
         seed=12),
]


def _import_reference():
    for p in (os.path.join(ROOT, "oracle", "pydp_standin"), ROOT, REFERENCE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import pipeline_dp
    return pipeline_dp


def _py(x):
    if isinstance(x, np.ndarray):
        return [_py(v) for v in x.tolist()]
    if isinstance(x, (tuple, list)):
        return [_py(v) for v in x]
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    return x


def _rows(rng, case):
    """Every privacy id: 1..l0 distinct partitions, 1..linf rows per pair."""
    rows = []
    for u in range(case["n_pids"]):
        for k in rng.choice(case["n_partitions"], size=int(rng.integers(1, case["l0"] + 1)), replace=False):
            for _ in range(int(rng.integers(1, case["linf"] + 1))):
                if case["integer"]:
                    v = [int(x) for x in rng.integers(-9, 10, VECTOR_SIZE)]
                else:
                    v = [round(float(x), 3) for x in rng.normal(0.5, 2.0, VECTOR_SIZE)]
                rows.append([u, int(k), v])
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


def params_of(pdp, case, norm_kind="linf", max_norm=1.0):
    return pdp.AggregateParams(
        metrics=[pdp.Metrics.VECTOR_SUM, pdp.Metrics.COUNT, pdp.Metrics.PRIVACY_ID_COUNT],
        noise_kind=getattr(pdp.NoiseKind, case["noise"]), max_partitions_contributed=case["l0"],
        max_contributions_per_partition=case["linf"], vector_size=VECTOR_SIZE, vector_max_norm=max_norm,
        vector_norm_kind=pdp.NormKind(norm_kind))


def run_case(pdp, case):
    from pipeline_dp import combiners, dp_computations, partition_selection
    rows = _rows(np.random.default_rng(case["seed"]), case)
    params = params_of(pdp, case)
    accountant = pdp.NaiveBudgetAccountant(total_epsilon=1.0, total_delta=1e-6)
    engine = pdp.DPEngine(accountant, pdp.LocalBackend())
    extractors = pdp.DataExtractors(privacy_id_extractor=lambda r: r[0], partition_extractor=lambda r: r[1],
                                    value_extractor=lambda r: np.array(r[2]))

    class KeepAll:

        def should_keep(self, n):
            return True

    saved_cm = combiners.CompoundCombiner.compute_metrics
    saved_ps = partition_selection.create_partition_selection_strategy
    combiners.CompoundCombiner.compute_metrics = lambda self, acc: acc
    partition_selection.create_partition_selection_strategy = lambda *a, **k: KeepAll()
    try:
        out = engine.aggregate(rows, params, extractors)
        accountant.compute_budgets()
        raw = sorted(((int(pk), acc) for pk, acc in out), key=lambda t: t[0])
    finally:
        combiners.CompoundCombiner.compute_metrics = saved_cm
        partition_selection.create_partition_selection_strategy = saved_ps
    budgets = [[m.mechanism_spec.mechanism_type.value, m.mechanism_spec.eps, m.mechanism_spec.delta]
               for m in accountant._mechanisms]
    comb = combiners.create_compound_combiner(params, pdp.NaiveBudgetAccountant(1.0, 1e-6))
    probe = pdp.DPEngine(pdp.NaiveBudgetAccountant(1.0, 1e-6), pdp.LocalBackend())
    bounder = type(probe._create_contribution_bounder(params, comb.expects_per_partition_sampling())).__name__
    vectors = {pk: np.asarray(acc[1][2]) for pk, acc in raw}
    clips = []
    for kind, order in (("linf", np.inf), ("l1", 1), ("l2", 2)):
        norms = [float(np.linalg.norm(v, ord=order)) for v in vectors.values()]
        max_norm = float(np.median(norms))
        if case["integer"]:
            max_norm = float(round(max_norm))
        nk = pdp.NormKind(kind)
        clipped = [[pk, _py(dp_computations._clip_vector(v, max_norm, nk))] for pk, v in vectors.items()]
        n_clipped = sum(1 for n in norms if n > max_norm)
        assert 0 < n_clipped < len(norms), (kind, n_clipped)
        zero = np.zeros(VECTOR_SIZE, dtype=np.int64 if case["integer"] else np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            zero_clipped = _py(dp_computations._clip_vector(zero, max_norm, nk))
        clips.append({"norm_kind": kind, "max_norm": max_norm, "clipped": clipped, "n_clipped": n_clipped,
                      "zero_clipped": zero_clipped})
    return {"name": case["name"], "case": case, "rows": rows,
            "combiners": [type(c).__name__ for c in comb._combiners], "metrics_names": list(comb.metrics_names()),
            "expected": [[pk, _py(acc)] for pk, acc in raw], "budgets": budgets, "reference_bounder": bounder,
            "clips": clips}


def main():
    pdp = _import_reference()
    data = {"vector_size": VECTOR_SIZE, "cases": [run_case(pdp, c) for c in CASES]}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(data, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
