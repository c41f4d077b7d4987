"""Utility analysis result types (reference analysis/metrics.py): per partition
(:23-72) and, further down, across partitions (:75-282)."""
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


# ------------------------------------------------------------------------
# Cross-partition result types (reference analysis/metrics.py:75-282): what
# perform_utility_analysis reports per parameter configuration.
@dataclass
class MeanVariance:
    mean: float
    var: float


@dataclass
class ContributionBoundingErrors:
    """Error by kind of contribution bounding: l0 (cross-partition bounding, a
    random variable per partition) and linf_min / linf_max (clipping to the
    lower / upper bound, deterministic per partition)."""
    l0: MeanVariance
    linf_min: float
    linf_max: float

    def to_relative(self, value: float) -> 'ContributionBoundingErrors':
        """The errors relative to the actual `value` (the variance by its square)."""
        return ContributionBoundingErrors(l0=MeanVariance(self.l0.mean / value, self.l0.var / value**2),
                                          linf_min=self.linf_min / value, linf_max=self.linf_max / value)


@dataclass
class ValueErrors:
    """Errors of (dp_value - actual_value), computed per partition and averaged
    across partitions: `mean` is the bias, `rmse` the mean of
    sqrt(E(dp_value - actual_value)^2); the *_with_dropped_partitions fields
    count a partition dropped by private selection (probability 1 - p) as an
    error of |actual_value|: p * rmse + (1 - p) * |actual_value|.  l1 and
    l1_with_dropped_partitions are 0, as in the reference."""
    bounding_errors: ContributionBoundingErrors
    mean: float
    variance: float
    rmse: float
    l1: float
    rmse_with_dropped_partitions: float
    l1_with_dropped_partitions: float

    def to_relative(self, value: float):
        """The errors relative to the actual `value`; all 0 when it is 0, so that
        such a partition does not move an averaged relative error."""
        if value == 0:
            return ValueErrors(bounding_errors=ContributionBoundingErrors(l0=MeanVariance(0, 0), linf_min=0,
                                                                         linf_max=0),
                               mean=0, variance=0, rmse=0, l1=0, rmse_with_dropped_partitions=0,
                               l1_with_dropped_partitions=0)
        return ValueErrors(self.bounding_errors.to_relative(value), mean=self.mean / value,
                           variance=self.variance / value**2, rmse=self.rmse / value, l1=self.l1 / value,
                           rmse_with_dropped_partitions=self.rmse_with_dropped_partitions / value,
                           l1_with_dropped_partitions=self.l1_with_dropped_partitions / value)


@dataclass
class DataDropInfo:
    """Ratio of the data dropped by l0 bounding, by linf bounding and by
    partition selection (of what survived bounding)."""
    l0: float
    linf: float
    partition_selection: float


@dataclass
class MetricUtility:
    """Cross-partition utility of one DP metric (COUNT, SUM, ...)."""
    metric: agg.Metric
    noise_std: float
    noise_kind: agg.NoiseKind
    ratio_data_dropped: Optional[DataDropInfo]
    absolute_error: ValueErrors
    relative_error: ValueErrors


@dataclass
class PartitionsInfo:
    """Partitions and partition selection: num_non_public_partitions and
    num_empty_partitions with public partitions, strategy and kept_partitions
    (mean and variance of the number of kept partitions) with private ones."""
    public_partitions: bool
    num_dataset_partitions: int
    num_non_public_partitions: Optional[int] = None
    num_empty_partitions: Optional[int] = None
    strategy: Optional[agg.PartitionSelectionStrategy] = None
    kept_partitions: Optional[MeanVariance] = None


@dataclass
class UtilityReport:
    """The utility analysis of the parameter configuration `configuration_index`."""
    configuration_index: int
    partitions_info: PartitionsInfo
    metric_errors: Optional[List[MetricUtility]] = None
    utility_report_histogram: Optional[List['UtilityReportBin']] = None


@dataclass
class UtilityReportBin:
    """The report over the partitions whose size (the non-DP value of the first
    analysed metric) lies in [partition_size_from, partition_size_to)."""
    partition_size_from: int
    partition_size_to: int
    report: UtilityReport
