"""TEST INFRASTRUCTURE — regenerate tests/golden/private_bounds/private_bounds.json from the reference.

Runs only where the reference checkout is present (the PIPELINEDP_REFERENCE
environment variable, or a `reference` directory beside the repository); the
fixture it writes is data only
and is what the tests read.  The reference imports with the python-dp stand-in
of oracle/pydp_standin on the path, as oracle/gen_golden.py does.

For each case the reference's DPEngine.calculate_private_contribution_bounds
runs end to end on LocalBackend with ExponentialMechanism.apply patched to
record what it is given instead of drawing: the scoring function (whose L0
histogram, number of partitions and upper bound are the reference's own), the
candidate list, every candidate's score and _calculate_probabilities.  Nothing
is driven by hand, so the partition filter, the histograms and the candidate
generation recorded are those of the reference's call.

Usage: python tools/gen_golden_private_bounds.py   (from the repository root)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("PIPELINEDP_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
# a directory of its own: tests/golden_util.py reads every tests/golden/*.json as a scalar aggregate case
OUT = os.path.join(ROOT, "tests", "golden", "private_bounds", "private_bounds.json")

CASES = [
    # upper bound below the number of partitions
    dict(name="laplace_small", noise="LAPLACE", eps=1.0, delta=0.0, calc_eps=1.0, upper=10, n_pids=200,
         n_partitions=30, max_per_pid=8, keys="int", keep="all", seed=21),
    # upper bound above the number of partitions: B = P
    dict(name="gaussian_upper_above_partitions", noise="GAUSSIAN", eps=0.8, delta=1e-6, calc_eps=2.0, upper=100,
         n_pids=150, n_partitions=12, max_per_pid=12, keys="int", keep="all", seed=22),
    # `partitions` drops rows (string keys; three of its keys never occur in the data)
    dict(name="laplace_partitions_drop_rows", noise="LAPLACE", eps=2.0, delta=0.0, calc_eps=0.5, upper=15,
         n_pids=180, n_partitions=40, max_per_pid=10, keys="str", keep="half", seed=23),
    # two users in more than 1,000 partitions: bins with lower 1000 and 1010, candidates with step 10
    dict(name="gaussian_heavy_users", noise="GAUSSIAN", eps=1.0, delta=1e-6, calc_eps=1.0, upper=2000, n_pids=120,
         n_partitions=1200, max_per_pid=5, keys="int", keep="all", heavy=[1003, 1015], seed=24),
]


def _import_reference():
    for p in (os.path.join(ROOT, "oracle", "pydp_standin"), ROOT, REFERENCE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import pipeline_dp
    return pipeline_dp


def _key(case, k):
    return f"p{k}" if case["keys"] == "str" else int(k)


def make_rows(case):
    """(rows [privacy id, partition key], partitions) of a case."""
    rng = np.random.default_rng(case["seed"])
    rows = []
    for u in range(case["n_pids"]):
        for k in rng.choice(case["n_partitions"], size=int(rng.integers(1, case["max_per_pid"] + 1)), replace=False):
            for _ in range(int(rng.integers(1, 3))):
                rows.append([u, _key(case, k)])
    for j, n in enumerate(case.get("heavy", [])):
        for k in rng.choice(case["n_partitions"], size=n, replace=False):
            rows.append([case["n_pids"] + j, _key(case, k)])
    rows = [rows[i] for i in rng.permutation(len(rows))]
    if case["keep"] == "all":
        partitions = [_key(case, k) for k in range(case["n_partitions"])]
    else:
        partitions = [_key(case, k) for k in range(0, case["n_partitions"], 2)]
        partitions += [_key(case, case["n_partitions"] + j) for j in range(3)]  # never in the data
    return rows, partitions


def run_case(pdp, case):
    from pipeline_dp import dp_computations
    rows, partitions = make_rows(case)
    params = pdp.CalculatePrivateContributionBoundsParams(
        aggregation_noise_kind=getattr(pdp.NoiseKind, case["noise"]), aggregation_eps=case["eps"],
        aggregation_delta=case["delta"], calculation_eps=case["calc_eps"],
        max_partitions_contributed_upper_bound=case["upper"])
    engine = pdp.DPEngine(pdp.NaiveBudgetAccountant(total_epsilon=1.0, total_delta=1e-6), pdp.LocalBackend())
    extractors = pdp.DataExtractors(privacy_id_extractor=lambda r: r[0], partition_extractor=lambda r: r[1],
                                    value_extractor=lambda r: 0)
    seen = {}

    def record(self, eps, inputs):
        sf = self._scoring_function
        seen.update(
            eps=eps, candidates=[int(k) for k in inputs], scores=[float(sf.score(k)) for k in inputs],
            probabilities=[float(p) for p in self._calculate_probabilities(eps, inputs)],
            number_of_partitions=int(sf._number_of_partitions),
            upper_bound=int(sf._max_partitions_contributed_best_upper_bound()),
            global_sensitivity=int(sf.global_sensitivity),
            l0_bins=[[int(b.lower), int(b.upper), int(b.count), int(b.sum), int(b.max)]
                     for b in sf._l0_histogram.bins],
            noise_std=[float(sf._l0_impact_noise(k) / sf._number_of_partitions) for k in inputs])
        return inputs[0]

    saved = dp_computations.ExponentialMechanism.apply
    dp_computations.ExponentialMechanism.apply = record
    try:
        out = list(engine.calculate_private_contribution_bounds(rows, params, extractors, partitions))
    finally:
        dp_computations.ExponentialMechanism.apply = saved
    assert len(out) == 1 and out[0].max_partitions_contributed == seen["candidates"][0]
    assert seen["eps"] == case["calc_eps"]
    kept = set(partitions)
    seen["rows_kept"] = sum(1 for r in rows if r[1] in kept)
    del seen["eps"]
    return {"name": case["name"], "case": case, "rows": rows, "partitions": partitions, **seen}


def main():
    pdp = _import_reference()
    cases = [run_case(pdp, c) for c in CASES]
    by = {c["name"]: c for c in cases}
    assert by["gaussian_upper_above_partitions"]["upper_bound"] == 12
    assert by["laplace_partitions_drop_rows"]["rows_kept"] < len(by["laplace_partitions_drop_rows"]["rows"])
    heavy = by["gaussian_heavy_users"]
    assert {1000, 1010} <= {b[0] for b in heavy["l0_bins"]} and 1010 in heavy["candidates"]
    assert 1001 not in heavy["candidates"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
