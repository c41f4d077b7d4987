"""perform_utility_analysis: the public entry point of utility analysis
(reference analysis/utility_analysis.py), on one GPU.

UtilityAnalysisEngine.analyze leaves [P, K] arrays on the device (per partition
and parameter configuration).  `pdp_utility_report`
(csrc/pdp_analysis_report.hip) folds them, where they lie, into one report per
configuration over all partitions and one per bucket of partition size
(`run_utility_report`); only those sums, at most 39 x 63 x K doubles, are
copied to the host, where `assemble_reports` builds the reference's
UtilityReport dataclasses from them.
"""
import bisect
import ctypes
from typing import List, Optional, Sequence

import numpy as np

from pipelinedp_amd import _native as N
from pipelinedp_amd import budget_accounting
from pipelinedp_amd.analysis import data_structures
from pipelinedp_amd.analysis import metrics as metrics_lib
from pipelinedp_amd.analysis import utility_analysis_engine


def _generate_bucket_bounds():
    result = [0, 1]
    for i in range(1, 13):
        result += [10**i, 2 * 10**i, 5 * 10**i]
    return tuple(result)


# Lower bounds of the UtilityReport histogram's buckets by partition size:
# [0, 1] + [1, 2, 5] * 10**i, i = 1..12 (PDP_UA_REPORT_BUCKETS of them).
BUCKET_BOUNDS = _generate_bucket_bounds()
assert len(BUCKET_BOUNDS) == N.UA_REPORT_BUCKETS

N_SELECTION_FIELDS = 3   # total weight, kept_partitions mean and variance
N_METRIC_FIELDS = 20     # sum_actual, 3 dropped, 8 absolute, 8 relative


def bucket_index(size) -> int:
    """Index of the largest bound <= size; 0 for a negative size."""
    if size < 0:
        return 0
    return bisect.bisect_right(BUCKET_BOUNDS, size) - 1


def bucket_upper_bound(index: int) -> int:
    """The next bound, or -1 for the last bucket."""
    return BUCKET_BOUNDS[index + 1] if index + 1 < len(BUCKET_BOUNDS) else -1


def run_utility_report(raw_outputs, std_noise, flags: int):
    """pdp_utility_report on the device outputs of run_utility_analysis
    (`raw_outputs`: its dict, over all partition codes), the host-side
    std_noise[m][k] and the same flags.  Returns device tensors (report float64
    [39, 3 + 20 M, K], counts int64 [39, 2]); layout in pipelinedp_amd.h."""
    import torch
    from pipelinedp_amd import executor as X
    lib = N.lib()
    raw = raw_outputs["raw_statistics"]
    keep, metrics = raw_outputs["keep_probability"], raw_outputs["metrics"]
    n_metrics = bin(flags & 7).count("1")
    P = int(raw.shape[0])
    K = int(metrics.shape[3]) if n_metrics else int(keep.shape[1])
    if n_metrics:
        sn = np.ascontiguousarray(np.asarray(std_noise, dtype=np.float64).reshape(n_metrics, K))
        sn_ptr = sn.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    else:
        sn_ptr = None
    need = ctypes.c_uint64(0)
    N.check(lib.pdp_utility_report_workspace_bytes(P, K, flags, ctypes.byref(need)),
            "pdp_utility_report_workspace_bytes")
    device = raw.device
    workspace = torch.empty(need.value + 256, dtype=torch.uint8, device=device)
    shift = (-workspace.data_ptr()) % 256
    n_fields = N_SELECTION_FIELDS + N_METRIC_FIELDS * n_metrics
    report = torch.empty((N.UA_REPORT_BUCKETS + 1, n_fields, K), dtype=torch.float64, device=device)
    counts = torch.empty((N.UA_REPORT_BUCKETS + 1, 2), dtype=torch.int64, device=device)
    N.check(lib.pdp_utility_report(X._ptr(raw), X._ptr(keep) if not flags & N.UA_PUBLIC else None,
                                   X._ptr(metrics) if n_metrics else None, P, K, flags, sn_ptr, X._ptr(report),
                                   X._ptr(counts), workspace.data_ptr() + shift, need.value, X._stream()),
            "pdp_utility_report")
    if n_metrics:
        torch.cuda.current_stream(device).synchronize()  # the enqueued copy reads `sn`
    return report, counts


def _value_errors(v) -> metrics_lib.ValueErrors:
    """ValueErrors of the eight sums l0 mean, l0 var, linf_min, linf_max, mean,
    variance, rmse, rmse_with_dropped_partitions (l1 fields: 0, as in the reference)."""
    v = [float(x) for x in v]
    return metrics_lib.ValueErrors(
        bounding_errors=metrics_lib.ContributionBoundingErrors(l0=metrics_lib.MeanVariance(v[0], v[1]),
                                                               linf_min=v[2], linf_max=v[3]),
        mean=v[4], variance=v[5], rmse=v[6], l1=0.0, rmse_with_dropped_partitions=v[7],
        l1_with_dropped_partitions=0.0)


def _one_report(entry, count, k, metric_names, std_noise, noise_kind, strategy, is_public):
    """UtilityReport of configuration k from one [F, K] entry of `report` and its counts."""
    if is_public:
        info = metrics_lib.PartitionsInfo(public_partitions=True, num_dataset_partitions=int(count[0]),
                                          num_non_public_partitions=0, num_empty_partitions=int(count[1]))
    else:
        info = metrics_lib.PartitionsInfo(
            public_partitions=False, num_dataset_partitions=int(count[0]), strategy=strategy,
            kept_partitions=metrics_lib.MeanVariance(float(entry[1, k]), float(entry[2, k])))
    metric_errors = None
    if metric_names:
        metric_errors = []
        for m, name in enumerate(metric_names):
            f = entry[N_SELECTION_FIELDS + N_METRIC_FIELDS * m:N_SELECTION_FIELDS + N_METRIC_FIELDS * (m + 1), k]
            metric_errors.append(metrics_lib.MetricUtility(
                metric=name, noise_std=std_noise[m][k], noise_kind=noise_kind[k],
                ratio_data_dropped=metrics_lib.DataDropInfo(l0=float(f[1]), linf=float(f[2]),
                                                            partition_selection=float(f[3])),
                absolute_error=_value_errors(f[4:12]), relative_error=_value_errors(f[12:20])))
    return metrics_lib.UtilityReport(configuration_index=k, partitions_info=info, metric_errors=metric_errors)


def assemble_reports(report: np.ndarray, counts: np.ndarray, metric_names: Sequence, std_noise, noise_kind,
                     strategies: Optional[Sequence]) -> List[metrics_lib.UtilityReport]:
    """The K UtilityReports of host copies of pdp_utility_report's outputs:
    entry 38 is the report over all partitions, every non-empty bucket a
    UtilityReportBin of its histogram, in ascending order.  `strategies`: the
    partition selection strategy per configuration, None with public partitions.
    A MetricUtility's `metric` is the metric its numbers were computed for
    (SUM, COUNT, PRIVACY_ID_COUNT order)."""
    is_public = strategies is None
    K = report.shape[2]
    nonempty = [b for b in range(N.UA_REPORT_BUCKETS) if counts[b, 0] + counts[b, 1] > 0]
    out = []
    for k in range(K):
        strategy = None if is_public else strategies[k]
        args = (k, metric_names, std_noise, noise_kind, strategy, is_public)
        total = _one_report(report[N.UA_REPORT_BUCKETS], counts[N.UA_REPORT_BUCKETS], *args)
        total.utility_report_histogram = [
            metrics_lib.UtilityReportBin(BUCKET_BOUNDS[b], bucket_upper_bound(b),
                                         _one_report(report[b], counts[b], *args)) for b in nonempty]
        out.append(total)
    return out


def perform_utility_analysis(col, backend, options: data_structures.UtilityAnalysisOptions, data_extractors,
                             public_partitions=None):
    """Utility analysis of DP aggregations for every configuration of `options`.

    Args:
      col: collection where all elements are of the same type.
      backend: ColumnarBackend.
      options: options for utility analysis.
      data_extractors: DataExtractors for raw rows, PreAggregateExtractors when
        options.pre_aggregated_data.
      public_partitions: partition keys that will be present in the result; if
        None, private partition selection is analysed.
    Returns:
      (reports, per_partition_result): a list with one metrics.UtilityReport
      per configuration, and the UtilityAnalysisResult of
      UtilityAnalysisEngine.analyze.
    """
    budget_accountant = budget_accounting.NaiveBudgetAccountant(total_epsilon=options.epsilon,
                                                                total_delta=options.delta)
    engine = utility_analysis_engine.UtilityAnalysisEngine(budget_accountant=budget_accountant, backend=backend)
    result = engine.analyze(col, options=options, data_extractors=data_extractors,
                            public_partitions=public_partitions)
    report, counts = run_utility_report(result._raw_outputs, result.std_noise, result._flags)
    strategies = None
    if public_partitions is None:
        strategies = data_structures.get_partition_selection_strategy(options)
    reports = assemble_reports(report.cpu().numpy(), counts.cpu().numpy(), result.metric_names, result.std_noise,
                               result.noise_kind, strategies)
    return reports, result
