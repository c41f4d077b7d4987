"""The VECTOR_SUM golden fixture (tests/golden/vector_sum/vector_sum.json, made
by tools/gen_golden_vector_sum.py from the reference) and helpers shared by
the host and GPU tests."""
import json
import os

import numpy as np

import pipelinedp_amd as pdp

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vector_sum", "vector_sum.json")
with open(PATH) as _f:
    FIXTURE = json.load(_f)


def cases():
    return FIXTURE["cases"]


def case_ids():
    return [c["name"] for c in FIXTURE["cases"]]


def params(fx, norm_kind="linf", max_norm=1.0, metrics=("VECTOR_SUM", "COUNT", "PRIVACY_ID_COUNT")):
    """AggregateParams as the generator built them for the reference."""
    case = fx["case"]
    return pdp.AggregateParams(metrics=[getattr(pdp.Metrics, m) for m in metrics],
                               noise_kind=getattr(pdp.NoiseKind, case["noise"]),
                               max_partitions_contributed=case["l0"],
                               max_contributions_per_partition=case["linf"], vector_size=FIXTURE["vector_size"],
                               vector_max_norm=max_norm, vector_norm_kind=pdp.NormKind(norm_kind))


def clip_of(fx, kind):
    return next(c for c in fx["clips"] if c["norm_kind"] == kind)


def accumulator_vectors(fx):
    """{partition: expected raw vector} (int64 for the integer case)."""
    dtype = np.int64 if fx["case"]["integer"] else np.float64
    return {pk: np.asarray(acc[1][2], dtype=dtype) for pk, acc in fx["expected"]}
