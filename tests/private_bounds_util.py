"""The private-contribution-bounds golden fixture
(tests/golden/private_bounds/private_bounds.json, made by
tools/gen_golden_private_bounds.py from the reference) and helpers shared by
the host and GPU tests."""
import json
import os

import numpy as np

import pipelinedp_amd as pdp
from pipelinedp_amd.dataset_histograms import histograms as hist
from pipelinedp_amd.dataset_histograms.computing_histograms import log_bin_bounds

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "private_bounds", "private_bounds.json")
with open(PATH) as _f:
    FIXTURE = json.load(_f)

RTOL = 1e-9  # the project's fp64 parity tolerance


def cases():
    return FIXTURE["cases"]


def case_ids():
    return [c["name"] for c in FIXTURE["cases"]]


def params(fx, **overrides):
    """CalculatePrivateContributionBoundsParams as the generator built them."""
    case = fx["case"]
    kw = dict(aggregation_noise_kind=getattr(pdp.NoiseKind, case["noise"]), aggregation_eps=case["eps"],
              aggregation_delta=case["delta"], calculation_eps=case["calc_eps"],
              max_partitions_contributed_upper_bound=case["upper"])
    kw.update(overrides)
    return pdp.CalculatePrivateContributionBoundsParams(**kw)


def rows(fx):
    """The fixture's rows as (privacy id, partition key) tuples."""
    return [(r[0], r[1]) for r in fx["rows"]]


def extractors():
    return pdp.DataExtractors(privacy_id_extractor=lambda r: r[0], partition_extractor=lambda r: r[1],
                              value_extractor=lambda r: 0)


def l0_histogram(fx) -> hist.Histogram:
    """The reference's L0 histogram of the case as a host Histogram."""
    return hist.Histogram(hist.HistogramType.L0_CONTRIBUTIONS,
                          [hist.FrequencyBin(lower=b[0], upper=b[1], count=b[2], sum=b[3], max=b[4])
                           for b in fx["l0_bins"]])


def dense_l0_counts(bins) -> np.ndarray:
    """[(lower, count), ...] -> the dense count row (int64[HIST_LOG_BINS]) of
    the device histograms; every lower must be a bin lower."""
    from pipelinedp_amd import _native as N
    lowers = {log_bin_bounds(b)[0]: b for b in range(N.HIST_LOG_BINS) if log_bin_bounds(b)[0] < 2**62}
    row = np.zeros(N.HIST_LOG_BINS, dtype=np.int64)
    for lower, count in bins:
        row[lowers[lower]] += count
    return row


def impact_dropped(count_row, upper_bound, candidates):
    """The definition of pdp_l0_impact_dropped in Python integers (exact)."""
    nz = [(log_bin_bounds(int(b))[0], int(count_row[b])) for b in np.flatnonzero(count_row)]
    return [sum(max(min(lower, upper_bound) - k, 0) * c for lower, c in nz) for k in candidates]
