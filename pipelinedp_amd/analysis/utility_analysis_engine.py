"""UtilityAnalysisEngine: the per-partition stage of the reference's
analysis/utility_analysis_engine.py on one GPU.

The reference builds DPEngine._aggregate's graph with analysis combiners: per
(privacy id, partition) pair (count, sum, n_partitions), merged per partition
by per_partition_combiners.CompoundCombiner for every parameter configuration.
Here the host plans the configurations (budgets, noise standard deviations,
keep tables: `plan_configurations`), and `pdp_utility_analysis`
(csrc/pdp_analysis.hip) computes every partition x configuration in one pass
(`run_utility_analysis`).  Raw rows are reduced to pair rows with torch (sort,
unique_consecutive, segment sums); pre-aggregated rows go straight to the
kernels.
"""
import copy
import ctypes
import dataclasses
from typing import List, Optional, Sequence

import numpy as np

from pipelinedp_amd import _native as N
from pipelinedp_amd import aggregate_params as agg
from pipelinedp_amd import dp_computations
from pipelinedp_amd import partition_selection
from pipelinedp_amd.analysis import data_structures
from pipelinedp_amd.analysis import metrics as metrics_lib
from pipelinedp_amd.data_extractors import DataExtractors, PreAggregateExtractors

# the reference's combiner order (utility_analysis_engine.py:125-139)
METRIC_ORDER = ((agg.Metrics.SUM, N.UA_SUM), (agg.Metrics.COUNT, N.UA_COUNT),
                (agg.Metrics.PRIVACY_ID_COUNT, N.UA_PRIVACY_ID_COUNT))
FIELDS = ("sum", "clipping_to_min_error", "clipping_to_max_error", "expected_l0_bounding_error",
          "std_l0_bounding_error")


@dataclasses.dataclass
class ConfigurationPlan:
    """Host-side plan of one parameter configuration."""
    params: agg.AggregateParams
    selection_spec: Optional[object]  # MechanismSpec of partition selection (private partitions)
    metric_specs: List[object]        # MechanismSpec per analysed metric, METRIC_ORDER
    std_noise: List[float]            # noise standard deviation per analysed metric
    keep_table: Optional[np.ndarray]  # probability_of_keep(i), i = 0.. until it is 1.0


def analysed_metrics(params: agg.AggregateParams):
    return [m for m, _ in METRIC_ORDER if m in (params.metrics or [])]


def _sensitivities(metric, params):
    if metric == agg.Metrics.SUM:
        return dp_computations.compute_sensitivities_for_sum(params)
    if metric == agg.Metrics.COUNT:
        return dp_computations.compute_sensitivities_for_count(params)
    return dp_computations.compute_sensitivities_for_privacy_id_count(params)


def keep_probability_table(strategy, cap: int = N.UA_MAX_KEEP_TABLE) -> np.ndarray:
    """strategy.probability_of_keep(i) for i = 0, 1, ... up to and including
    the first value that is exactly 1.0 (every later one is 1.0: the kernel
    counts entries past the end as 1.0)."""
    table = []
    while True:
        p = float(strategy.probability_of_keep(len(table)))
        table.append(p)
        if p == 1.0:
            return np.asarray(table, dtype=np.float64)
        if len(table) >= cap:
            raise NotImplementedError(
                f"the keep probability does not reach 1.0 within {cap} privacy ids "
                "(PDP_UA_MAX_KEEP_TABLE): this partition selection configuration is not supported")


def plan_configurations(budget_accountant, options: data_structures.UtilityAnalysisOptions,
                        is_public_partitions: bool) -> List[ConfigurationPlan]:
    """Budgets and host-side quantities per configuration
    (utility_analysis_engine.py:99-143): a deep copy of the accountant per
    configuration, GENERIC for partition selection when partitions are private,
    then one request per metric in SUM, COUNT, PRIVACY_ID_COUNT order."""
    plans = []
    for params in data_structures.get_aggregate_params(options):
        accountant = copy.deepcopy(budget_accountant)
        metrics = analysed_metrics(params)
        mechanism_type = None
        if params.noise_kind is None:
            assert not metrics, f"Noise kind should be given when {metrics[0]} is analyzed"
        else:
            mechanism_type = params.noise_kind.convert_to_mechanism_type()
        selection_spec = None
        if not is_public_partitions:
            selection_spec = accountant.request_budget(agg.MechanismType.GENERIC)
        metric_specs = [accountant.request_budget(mechanism_type) for _ in metrics]
        accountant.compute_budgets()
        std_noise = [dp_computations.create_additive_mechanism(spec, _sensitivities(metric, params)).std
                     for metric, spec in zip(metrics, metric_specs)]
        keep_table = None
        if selection_spec is not None:
            strategy = partition_selection.create_partition_selection_strategy(
                params.partition_selection_strategy, selection_spec.eps, selection_spec.delta,
                params.max_partitions_contributed, params.pre_threshold)
            keep_table = keep_probability_table(strategy)
        plans.append(ConfigurationPlan(params, selection_spec, metric_specs, std_noise, keep_table))
    return plans


def run_utility_analysis(partition, count, pair_sum, n_partitions_of_pid, n_partitions: int,
                         configurations: Sequence[tuple], keep_tables: Optional[Sequence[np.ndarray]],
                         metric_flags: int):
    """pdp_utility_analysis on device pair columns.  configurations: (l0, linf,
    min_sum, max_sum) per configuration; keep_tables: one float64 array per
    configuration, or None for public partitions.  Returns a dict of device
    tensors: raw_statistics int64 [P, 2], keep_probability float64 [P, K] (or
    None), metrics float64 [M, 5, P, K]."""
    import torch
    from pipelinedp_amd import executor as X
    K = len(configurations)
    if K > N.MAX_CONFIGURATIONS:
        raise NotImplementedError(f"{K} configurations: more than PDP_MAX_CONFIGURATIONS = {N.MAX_CONFIGURATIONS}")
    lib = N.lib()
    device = partition.device
    n, P = int(partition.numel()), int(n_partitions)
    flags = int(metric_flags) | (N.UA_PUBLIC if keep_tables is None else 0)
    n_metrics = bin(metric_flags & 7).count("1")
    params = (N.UaConfigParams * K)()
    for k, (l0, linf, lo, hi) in enumerate(configurations):
        params[k].l0, params[k].linf = int(l0), int(linf or 0)
        params[k].min_sum, params[k].max_sum = float(lo or 0.0), float(hi or 0.0)
    offsets = (ctypes.c_int64 * (K + 1))()
    tables_t = None
    if keep_tables is not None:
        for k, t in enumerate(keep_tables):
            offsets[k + 1] = offsets[k] + len(t)
        flat = np.concatenate([np.asarray(t, dtype=np.float64) for t in keep_tables])
        tables_t = torch.from_numpy(flat).to(device)
    need = ctypes.c_uint64(0)
    N.check(lib.pdp_utility_analysis_workspace_bytes(n, P, K, flags, ctypes.byref(need)),
            "pdp_utility_analysis_workspace_bytes")
    workspace = torch.empty(need.value + 256, dtype=torch.uint8, device=device)
    shift = (-workspace.data_ptr()) % 256
    out = {
        "raw_statistics": torch.empty((P, 2), dtype=torch.int64, device=device),
        "keep_probability": None if keep_tables is None else torch.empty((P, K), dtype=torch.float64, device=device),
        "metrics": torch.empty((n_metrics, 5, P, K), dtype=torch.float64, device=device),
    }
    c_out = N.UaOutputs(X._ptr(out["raw_statistics"]), X._ptr(out["keep_probability"]),
                        X._ptr(out["metrics"]) if n_metrics else None)
    N.check(lib.pdp_utility_analysis(X._ptr(partition), X._ptr(count), X._ptr(pair_sum), X._ptr(n_partitions_of_pid),
                                     n, P, params, K, X._ptr(tables_t), offsets, flags, ctypes.byref(c_out),
                                     workspace.data_ptr() + shift, need.value, X._stream()),
            "pdp_utility_analysis")
    err = ctypes.c_uint32()
    N.check(lib.pdp_bound_error_flags(workspace.data_ptr() + shift, ctypes.byref(err), X._stream()),
            "pdp_bound_error_flags")
    if err.value & 1:
        raise ValueError("partition code outside the declared range")
    return out


class UtilityAnalysisResult:
    """The per-partition output of UtilityAnalysisEngine.analyze (the second
    output of the reference's perform_utility_analysis), held as columns:
    `partition_keys` (NumPy array, length P), `raw_statistics` (int64 [P, 2]:
    privacy_id_count, count), `keep_probability` (float64 [P, K]; None with
    public partitions), `metrics[m][field]` (float64 [P, K]) for each analysed
    metric m in SUM, COUNT, PRIVACY_ID_COUNT order and each field of FIELDS,
    and the host-side `std_noise[m][k]` / `noise_kind[k]`.  Arrays are device
    tensors; numpy() copies them to the host."""

    def __init__(self, partition_keys, raw_statistics, keep_probability, metric_names, metric_arrays, std_noise,
                 noise_kind):
        self.partition_keys = partition_keys
        self.raw_statistics = raw_statistics
        self.keep_probability = keep_probability
        self.metric_names = list(metric_names)
        self.metrics = metric_arrays   # list (per metric) of {field: [P, K]}
        self.std_noise = std_noise     # [M][K]
        self.noise_kind = noise_kind   # [K]
        self._raw_outputs = None       # run_utility_analysis's dict, [P]-indexed by partition code (analyze)
        self._flags = 0

    @property
    def n_configurations(self):
        return len(self.noise_kind)

    def __len__(self):
        return len(self.partition_keys)

    def numpy(self) -> "UtilityAnalysisResult":
        def host(t):
            return None if t is None else (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t))
        return UtilityAnalysisResult(self.partition_keys, host(self.raw_statistics), host(self.keep_probability),
                                     self.metric_names, [{f: host(a) for f, a in m.items()} for m in self.metrics],
                                     self.std_noise, self.noise_kind)

    def rows(self):
        """((partition_key, configuration_index), PerPartitionMetrics), partition-major."""
        h = self.numpy()
        for i, key in enumerate(h.partition_keys):
            raw = metrics_lib.RawStatistics(int(h.raw_statistics[i, 0]), int(h.raw_statistics[i, 1]))
            for k in range(self.n_configurations):
                errors = [metrics_lib.SumMetrics(aggregation=name, std_noise=h.std_noise[m][k],
                                                 noise_kind=h.noise_kind[k],
                                                 **{f: float(h.metrics[m][f][i, k]) for f in FIELDS})
                          for m, name in enumerate(h.metric_names)]
                keep = 1.0 if h.keep_probability is None else float(h.keep_probability[i, k])
                yield (_py(key), k), metrics_lib.PerPartitionMetrics(keep, raw, errors)


def _py(k):
    return k.item() if isinstance(k, np.generic) else k


class UtilityAnalysisEngine:
    """Utility analysis of DP aggregations per partition, for every
    configuration of options.multi_param_configuration at once."""

    def __init__(self, budget_accountant, backend):
        self._budget_accountant = budget_accountant
        self._backend = backend

    def aggregate(self, col, params, data_extractors, public_partitions=None):
        raise ValueError("UtilityAnalysisEngine.aggregate can't be called.\n"
                         "If you like to perform utility analysis use UtilityAnalysisEngine.analyze.\n"
                         "If you like to perform DP computations use DPEngine.aggregate.")

    def analyze(self, col, options: data_structures.UtilityAnalysisOptions, data_extractors,
                public_partitions=None) -> UtilityAnalysisResult:
        """Per partition and configuration what the reference's
        UtilityAnalysisEngine.analyze yields (PerPartitionMetrics), as a
        columnar UtilityAnalysisResult.  `data_extractors`: DataExtractors for
        raw rows, PreAggregateExtractors when options.pre_aggregated_data."""
        from pipelinedp_amd import parallel
        from pipelinedp_amd.columnar_backend import ColumnarBackend
        _check_utility_analysis_params(options, data_extractors)
        if col is None:
            raise ValueError("col must be non-empty")
        if not isinstance(self._backend, ColumnarBackend):
            raise NotImplementedError("UtilityAnalysisEngine.analyze runs on ColumnarBackend only")
        if parallel.world_info()[0] > 1:
            raise NotImplementedError("UtilityAnalysisEngine.analyze runs on one rank")
        if options.partitions_sampling_prob < 1:
            raise NotImplementedError("partitions_sampling_prob < 1 is not implemented")
        if options.n_configurations > N.MAX_CONFIGURATIONS:
            raise NotImplementedError(f"{options.n_configurations} configurations: more than "
                                      f"PDP_MAX_CONFIGURATIONS = {N.MAX_CONFIGURATIONS}")
        is_public = public_partitions is not None
        plans = plan_configurations(self._budget_accountant, options, is_public)
        names = analysed_metrics(options.aggregate_params)
        if is_public and not names:
            raise ValueError("public partitions without a metric: nothing to analyse")
        flags = 0
        for metric, bit in METRIC_ORDER:
            if metric in names:
                flags |= bit
        device = self._backend._torch_device()
        pk_enc, pairs, out_codes = _pair_columns(col, options, data_extractors, public_partitions, device)
        cfgs = [(p.params.max_partitions_contributed, p.params.max_contributions_per_partition,
                 p.params.min_sum_per_partition, p.params.max_sum_per_partition) for p in plans]
        raw = run_utility_analysis(*pairs, pk_enc.n, cfgs, None if is_public else [p.keep_table for p in plans],
                                   flags)
        import torch
        if out_codes is None:  # private partitions: the ones that have a pair
            out_codes = torch.nonzero(raw["raw_statistics"][:, 0] > 0).flatten()
        else:
            out_codes = torch.as_tensor(out_codes, device=device)
        keys = pk_enc.keys_of(out_codes.cpu().numpy())
        metric_arrays = [{f: raw["metrics"][m, j].index_select(0, out_codes) for j, f in enumerate(FIELDS)}
                         for m in range(len(names))]
        keep = None if is_public else raw["keep_probability"].index_select(0, out_codes)
        result = UtilityAnalysisResult(keys, raw["raw_statistics"].index_select(0, out_codes), keep, names,
                                       metric_arrays, [[p.std_noise[m] for p in plans] for m in range(len(names))],
                                       [p.params.noise_kind for p in plans])
        # the kernel outputs over all partition codes, for utility_analysis.run_utility_report
        result._raw_outputs, result._flags = raw, flags | (N.UA_PUBLIC if is_public else 0)
        return result


def _pair_columns(col, options, data_extractors, public_partitions, device):
    """Device pair columns (partition code, count, sum, n_partitions_of_pid),
    the partition dictionary and, with public partitions, their codes.  With
    public partitions the rows of other partitions are dropped first
    (dp_engine.py:125-129) and one (0, 0, 0) pair is appended to every public
    partition (:298-313: the reference adds an empty accumulator to each, which
    CompoundCombiner.create_accumulator turns into that pair)."""
    import torch
    from pipelinedp_amd import columnar as C
    from pipelinedp_amd.columnar_backend import _h2d, _host_or_device, _value_tensor
    from pipelinedp_amd.dataset_histograms import computing_histograms
    if options.pre_aggregated_data:
        rows = list(col)
        pk_raw = [data_extractors.partition_extractor(r) for r in rows]
        pre = [data_extractors.preaggregate_extractor(r) for r in rows]
        pk_enc = C.encode_keys(_host_or_device(pk_raw), None)
        cnt = torch.as_tensor(np.asarray([p[0] for p in pre], dtype=np.int64)).to(device)
        sm = torch.as_tensor(np.asarray([p[1] for p in pre], dtype=np.float64)).to(device)
        npart = torch.as_tensor(np.asarray([p[2] for p in pre], dtype=np.int64)).to(device)
        pid_t = None
    else:
        pid_raw, pk_raw, val_raw, n_pid, n_pk = computing_histograms._columns(col, data_extractors)
        pid_enc = C.encode_keys(_host_or_device(pid_raw), n_pid)
        pk_enc = C.encode_keys(_host_or_device(pk_raw), n_pk)
        pid_t = _h2d(pid_enc.codes, device, torch.int64)
        val_t = _value_tensor(val_raw, device).to(torch.float64) if val_raw is not None else None
    codes = None
    if public_partitions is not None:
        pk_enc, codes = C.extend_with_keys(pk_enc, public_partitions)
        codes = np.unique(codes)
    pk_t = _h2d(pk_enc.codes, device, torch.int64)
    mask = None
    if codes is not None:
        allowed = torch.zeros(pk_enc.n, dtype=torch.bool, device=device)
        allowed[torch.as_tensor(codes, device=device)] = True
        mask = allowed[pk_t]
    if options.pre_aggregated_data:
        if mask is not None:
            pk_t, cnt, sm, npart = pk_t[mask], cnt[mask], sm[mask], npart[mask]
    else:
        if mask is not None:
            pid_t, pk_t = pid_t[mask], pk_t[mask]
            val_t = val_t[mask] if val_t is not None else None
        pk_t, cnt, sm, npart = _pairs_from_rows(pid_t, pk_t, val_t, pid_enc.n, pk_enc.n)
    if codes is not None:
        extra = torch.as_tensor(codes, device=device)
        zeros = torch.zeros(len(codes), dtype=torch.int64, device=device)
        pk_t = torch.cat([pk_t, extra])
        cnt = torch.cat([cnt, zeros])
        sm = torch.cat([sm, zeros.to(torch.float64)])
        npart = torch.cat([npart, zeros])
    return pk_enc, (pk_t.contiguous(), cnt.contiguous(), sm.contiguous(), npart.contiguous()), codes


def _pairs_from_rows(pid_t, pk_t, val_t, n_pid: int, n_pk: int):
    """AnalysisContributionBounder (analysis/contribution_bounders.py:37-77)
    with torch: rows -> one row per (privacy id, partition) with the pair's row
    count and value sum (in row order: a stable sort, then a sequential
    segment sum) and the privacy id's number of distinct partitions."""
    import torch
    if n_pid * n_pk >= 2 ** 63:
        raise NotImplementedError("privacy id x partition codes do not fit 63 bits")
    key = pid_t * n_pk + pk_t
    key_sorted, order = torch.sort(key, stable=True)
    pairs, counts = torch.unique_consecutive(key_sorted, return_counts=True)
    if val_t is None:
        sums = torch.zeros(pairs.numel(), dtype=torch.float64, device=key.device)
    else:
        sums = torch.segment_reduce(val_t[order], "sum", lengths=counts, unsafe=True)
    pair_pid = torch.div(pairs, n_pk, rounding_mode="floor")
    _, per_pid = torch.unique_consecutive(pair_pid, return_counts=True)
    npart = torch.repeat_interleave(per_pid, per_pid)
    return pairs - pair_pid * n_pk, counts.to(torch.int64), sums, npart.to(torch.int64)


def _check_utility_analysis_params(options: data_structures.UtilityAnalysisOptions, data_extractors):
    """The reference's checks (utility_analysis_engine.py:188-225)."""
    if options.pre_aggregated_data:
        if not isinstance(data_extractors, PreAggregateExtractors):
            raise ValueError("options.pre_aggregated_data is set to true but PreAggregateExtractors aren't "
                             "provided. PreAggregateExtractors should be specified for pre-aggregated data.")
    elif not isinstance(data_extractors, DataExtractors):
        raise ValueError("pipeline_dp.DataExtractors should be specified for raw data.")
    params = options.aggregate_params
    if params.custom_combiners is not None:
        raise NotImplementedError("custom combiners are not supported")
    supported = {agg.Metrics.COUNT, agg.Metrics.SUM, agg.Metrics.PRIVACY_ID_COUNT}
    if not set(params.metrics or []).issubset(supported):
        not_supported_metrics = list(set(params.metrics).difference(supported))
        raise NotImplementedError(f"unsupported metric in metrics={not_supported_metrics}")
    if params.contribution_bounds_already_enforced:
        raise NotImplementedError("utility analysis when contribution bounds are already enforced is not supported")
    if params.post_aggregation_thresholding:
        raise NotImplementedError("Analysis with post_aggregation_thresholding are not yet implemented")
