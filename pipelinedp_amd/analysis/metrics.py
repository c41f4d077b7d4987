"""Per-partition utility analysis result types (reference analysis/metrics.py:23-72)."""
from dataclasses import dataclass
from typing import List, Optional

from pipelinedp_amd import aggregate_params as agg


@dataclass
class SumMetrics:
    """Per-partition metrics of a SUM, COUNT or PRIVACY_ID_COUNT analysis, s.t.
    E(sum after contribution bounding) = sum + clipping_to_min_error +
    clipping_to_max_error + expected_l0_bounding_error."""
    aggregation: agg.Metric
    sum: float
    clipping_to_min_error: float
    clipping_to_max_error: float
    expected_l0_bounding_error: float
    std_l0_bounding_error: float
    std_noise: float
    noise_kind: agg.NoiseKind


@dataclass
class RawStatistics:
    privacy_id_count: int
    count: int


@dataclass
class PerPartitionMetrics:
    partition_selection_probability_to_keep: float
    raw_statistics: RawStatistics
    metric_errors: Optional[List[SumMetrics]] = None
