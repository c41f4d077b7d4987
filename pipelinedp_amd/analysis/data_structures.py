"""API dataclasses of utility analysis (reference analysis/data_structures.py:24-151)."""
import copy
import dataclasses
from typing import Iterable, Optional, Sequence

from pipelinedp_amd import aggregate_params as agg


@dataclasses.dataclass
class MultiParameterConfiguration:
    """Parameter values to analyse at once: every set attribute is a sequence
    of values of the AggregateParams attribute of the same name, all of one
    length; configuration i takes the i-th value of each."""
    max_partitions_contributed: Sequence[int] = None
    max_contributions_per_partition: Sequence[int] = None
    min_sum_per_partition: Sequence[float] = None
    max_sum_per_partition: Sequence[float] = None
    noise_kind: Sequence[agg.NoiseKind] = None
    partition_selection_strategy: Sequence[agg.PartitionSelectionStrategy] = None

    def __post_init__(self):
        attributes = dataclasses.asdict(self)
        sizes = [len(value) for value in attributes.values() if value]
        if not sizes:
            raise ValueError("MultiParameterConfiguration must have at least 1 non-empty attribute.")
        if min(sizes) != max(sizes):
            raise ValueError("All set attributes in MultiParameterConfiguration must have the same length.")
        if (self.min_sum_per_partition is None) != (self.max_sum_per_partition is None):
            raise ValueError("MultiParameterConfiguration: min_sum_per_partition and "
                             "max_sum_per_partition must be both set or both None.")
        self._size = sizes[0]

    @property
    def size(self):
        return self._size

    def get_aggregate_params(self, params: agg.AggregateParams, index: int) -> agg.AggregateParams:
        """AggregateParams with the index-th parameters."""
        params = copy.copy(params)
        for name in ("max_partitions_contributed", "max_contributions_per_partition", "min_sum_per_partition",
                     "max_sum_per_partition", "noise_kind", "partition_selection_strategy"):
            values = getattr(self, name)
            if values:
                setattr(params, name, values[index])
        return params


@dataclasses.dataclass
class UtilityAnalysisOptions:
    """Options for the utility analysis."""
    epsilon: float
    delta: float
    aggregate_params: agg.AggregateParams
    multi_param_configuration: Optional[MultiParameterConfiguration] = None
    partitions_sampling_prob: float = 1
    pre_aggregated_data: bool = False

    def __post_init__(self):
        agg.validate_epsilon_delta(self.epsilon, self.delta, "UtilityAnalysisOptions")
        if self.partitions_sampling_prob <= 0 or self.partitions_sampling_prob > 1:
            raise ValueError(f"partitions_sampling_prob must be in the interval"
                             f" (0, 1], but {self.partitions_sampling_prob} given.")

    @property
    def n_configurations(self):
        if self.multi_param_configuration is None:
            return 1
        return self.multi_param_configuration.size


def get_aggregate_params(options: UtilityAnalysisOptions) -> Iterable[agg.AggregateParams]:
    """The AggregateParams of every configuration of `options`."""
    multi_param_configuration = options.multi_param_configuration
    if multi_param_configuration is None:
        yield options.aggregate_params
    else:
        for i in range(multi_param_configuration.size):
            yield multi_param_configuration.get_aggregate_params(options.aggregate_params, i)


def get_partition_selection_strategy(options: UtilityAnalysisOptions) -> Sequence[agg.PartitionSelectionStrategy]:
    """The partition selection strategy of every configuration."""
    multi_configuration = options.multi_param_configuration
    n_configurations = 1
    if multi_configuration is not None:
        if multi_configuration.partition_selection_strategy is not None:
            return multi_configuration.partition_selection_strategy
        n_configurations = multi_configuration.size
    return [options.aggregate_params.partition_selection_strategy] * n_configurations
