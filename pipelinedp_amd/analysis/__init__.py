"""Utility analysis (mirror of the reference's analysis/ package): the
per-partition stage on the GPU.  The cross-partition UtilityReport reduction,
parameter_tuning and dp_strategy_selector are not implemented; the [P, K]
arrays of UtilityAnalysisResult are their input."""
from pipelinedp_amd.analysis import metrics
from pipelinedp_amd.analysis.data_structures import MultiParameterConfiguration
from pipelinedp_amd.analysis.data_structures import UtilityAnalysisOptions
from pipelinedp_amd.analysis.data_structures import get_aggregate_params
from pipelinedp_amd.analysis.metrics import PerPartitionMetrics
from pipelinedp_amd.analysis.metrics import RawStatistics
from pipelinedp_amd.analysis.metrics import SumMetrics
from pipelinedp_amd.analysis.pre_aggregation import preaggregate
from pipelinedp_amd.analysis.utility_analysis_engine import UtilityAnalysisEngine
from pipelinedp_amd.analysis.utility_analysis_engine import UtilityAnalysisResult
