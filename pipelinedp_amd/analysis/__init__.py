"""Utility analysis (mirror of the reference's analysis/ package) on the GPU:
the per-partition stage (UtilityAnalysisEngine.analyze) and the cross-partition
UtilityReport reduction on top of it (perform_utility_analysis).
parameter_tuning and dp_strategy_selector are not implemented; the list of
UtilityReport that perform_utility_analysis returns is their input."""
from pipelinedp_amd.analysis import metrics
from pipelinedp_amd.analysis.data_structures import MultiParameterConfiguration
from pipelinedp_amd.analysis.data_structures import UtilityAnalysisOptions
from pipelinedp_amd.analysis.data_structures import get_aggregate_params
from pipelinedp_amd.analysis.metrics import ContributionBoundingErrors
from pipelinedp_amd.analysis.metrics import DataDropInfo
from pipelinedp_amd.analysis.metrics import MeanVariance
from pipelinedp_amd.analysis.metrics import MetricUtility
from pipelinedp_amd.analysis.metrics import PartitionsInfo
from pipelinedp_amd.analysis.metrics import PerPartitionMetrics
from pipelinedp_amd.analysis.metrics import RawStatistics
from pipelinedp_amd.analysis.metrics import SumMetrics
from pipelinedp_amd.analysis.metrics import UtilityReport
from pipelinedp_amd.analysis.metrics import UtilityReportBin
from pipelinedp_amd.analysis.metrics import ValueErrors
from pipelinedp_amd.analysis.pre_aggregation import preaggregate
from pipelinedp_amd.analysis.utility_analysis import BUCKET_BOUNDS
from pipelinedp_amd.analysis.utility_analysis import perform_utility_analysis
from pipelinedp_amd.analysis.utility_analysis import run_utility_report
from pipelinedp_amd.analysis.utility_analysis_engine import UtilityAnalysisEngine
from pipelinedp_amd.analysis.utility_analysis_engine import UtilityAnalysisResult
