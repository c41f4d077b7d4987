"""Differentially private choice of contribution bounds (mirror of
pipeline_dp/private_contribution_bounds.py).

PrivateL0Calculator chooses max_partitions_contributed with the exponential
mechanism over generate_possible_contribution_bounds(B), B = min(upper bound,
number of partitions), scoring each candidate k by

    score(k) = -0.5 * P * count_noise_std(k)
               - 0.5 * sum over L0 bins of max(min(bin.lower, B) - k, 0) * bin.count

L0ScoringFunction is the reference's row-wise form on a host Histogram
(:90-176).  DeviceL0ScoringFunction takes the L0 histogram as the dense device
count row of executor.dataset_histograms and computes the data-dependent sum
for every candidate in one kernel (`pdp_l0_impact_dropped`), so the bins never
travel to the host; the noise term, the softmax and the draw stay on the host.
"""
import dataclasses
from typing import List, Optional

import numpy as np

from pipelinedp_amd import aggregate_params as agg
from pipelinedp_amd import dp_computations
from pipelinedp_amd.dataset_histograms import histograms as hist


def generate_possible_contribution_bounds(upper_bound: int) -> List[int]:
    """The bounds with at most 3 leading non-zero digits up to upper_bound:
    1, 2, ..., 1000, 1010, ..., 10000, 10100, ... (:179-196; the lowers of the
    logarithmic histogram bins)."""
    bounds = []
    current, power = 1, 10
    while current <= upper_bound:
        bounds.append(current)
        if current >= power:
            power *= 10
        current += max(1, power // 1000)
    return bounds


class L0ScoringFunction(dp_computations.ExponentialMechanism.ScoringFunction):
    """Score of a max_partitions_contributed bound, for COUNT and
    PRIVACY_ID_COUNT aggregations (:90-176)."""

    def __init__(self, params: agg.CalculatePrivateContributionBoundsParams, number_of_partitions: int,
                 l0_histogram: Optional[hist.Histogram]):
        super().__init__()
        self._params = params
        self._number_of_partitions = number_of_partitions
        self._l0_histogram = l0_histogram

    def score(self, k: int) -> float:
        impact_noise_weight = 0.5
        return -(impact_noise_weight * self._l0_impact_noise(k) +
                 (1 - impact_noise_weight) * self._l0_impact_dropped(k))

    def _max_partitions_contributed_best_upper_bound(self) -> int:
        return min(self._params.max_partitions_contributed_upper_bound, self._number_of_partitions)

    @property
    def global_sensitivity(self) -> float:
        return self._max_partitions_contributed_best_upper_bound()

    @property
    def is_monotonic(self) -> bool:
        return True

    def _l0_impact_noise(self, k: int):
        noise_params = dp_computations.ScalarNoiseParams(
            eps=self._params.aggregation_eps, delta=self._params.aggregation_delta,
            max_partitions_contributed=k, max_contributions_per_partition=1,
            noise_kind=self._params.aggregation_noise_kind, min_value=None, max_value=None,
            min_sum_per_partition=None, max_sum_per_partition=None)
        return self._number_of_partitions * dp_computations.compute_dp_count_noise_std(noise_params)

    def _l0_impact_dropped(self, k: int):
        bound = self._max_partitions_contributed_best_upper_bound()
        return sum(max(min(b.lower, bound) - k, 0) * b.count for b in self._l0_histogram.bins)


class DeviceL0ScoringFunction(L0ScoringFunction):
    """L0ScoringFunction on the device L0 histogram: `l0_count` is the L0 row
    of executor.dataset_histograms(...)["int_count"] (int64[HIST_LOG_BINS] on
    the GPU).  The dropped-contributions sum of every candidate bound is
    computed at construction by one `pdp_l0_impact_dropped` launch; only those
    m integers come to the host."""

    def __init__(self, params: agg.CalculatePrivateContributionBoundsParams, number_of_partitions: int, l0_count):
        super().__init__(params, number_of_partitions, None)
        from pipelinedp_amd import executor as X
        import torch
        self.l0_count = l0_count
        self.candidates = generate_possible_contribution_bounds(self._max_partitions_contributed_best_upper_bound())
        cand = torch.as_tensor(np.asarray(self.candidates, dtype=np.int64)).to(l0_count.device)
        dropped = X.l0_impact_dropped(l0_count, self._max_partitions_contributed_best_upper_bound(), cand)
        self._dropped = dict(zip(self.candidates, dropped.cpu().tolist()))

    def _l0_impact_dropped(self, k: int):
        return self._dropped[int(k)]


def device_l0_inputs(backend, col, data_extractors, partitions, partitions_already_filtered: bool = False):
    """The device steps of DPEngine.calculate_private_contribution_bounds
    before the score (dp_engine.py:489-494): encodes the key columns, drops the
    rows outside `partitions` (`pdp_filter_rows`) unless already filtered, and
    computes the dataset histograms of the rest.  Returns (the raw device bins
    of executor.dataset_histograms, P = number of distinct keys in
    `partitions`); keys of `partitions` the data never has count towards P."""
    import ctypes

    import torch

    from pipelinedp_amd import _native as N
    from pipelinedp_amd import columnar as C
    from pipelinedp_amd import executor as X
    from pipelinedp_amd import parallel
    from pipelinedp_amd.columnar_backend import _h2d, _host_or_device
    from pipelinedp_amd.dataset_histograms import computing_histograms
    if parallel.world_info()[0] > 1:
        raise NotImplementedError("calculate_private_contribution_bounds runs on one rank: every rank would "
                                  "have to make the same draw, and that broadcast is not implemented")
    device = backend._torch_device()
    pid_raw, pk_raw, _, n_pid, n_pk = computing_histograms._columns(col, data_extractors)
    pid_enc = C.encode_keys(_host_or_device(pid_raw), n_pid)
    pk_enc = C.encode_keys(_host_or_device(pk_raw), n_pk)
    pk_enc, codes = C.extend_with_keys(pk_enc, partitions)
    n_partitions = int(np.unique(codes).size)
    pid_t = _h2d(pid_enc.codes, device, torch.int64)
    pk_t = _h2d(pk_enc.codes, device, torch.int64)
    if not partitions_already_filtered:
        mask = np.zeros(pk_enc.n, dtype=np.uint8)
        mask[codes] = 1
        pid_t, pk_t = X.filter_rows(pid_t, pk_t, torch.as_tensor(mask).to(device), n_partitions=pk_enc.n)
    if pk_t.numel() == 0:  # nothing left: every histogram is empty
        raw = {k: v.zero_() for k, v in X._histogram_outputs(device).items()}
        return raw, n_partitions
    raw = X.dataset_histograms(pid_t, pk_t, None, n_privacy_ids=pid_enc.n, n_partitions=pk_enc.n)
    flags = ctypes.c_uint32()
    N.check(N.lib().pdp_bound_error_flags(X._ptr(raw["workspace"]), ctypes.byref(flags), X._stream()),
            "pdp_bound_error_flags")
    if flags.value & 1:
        raise ValueError("privacy id or partition code outside the declared range")
    return raw, n_partitions


class PrivateL0Calculator:
    """Chooses the l0 bound (max_partitions_contributed) differentially
    privately (:27-87).  `histograms` is a one-element collection holding a
    DatasetHistograms, or the raw device bins of executor.dataset_histograms;
    `partitions` the partition keys the bound will be used with."""

    @dataclasses.dataclass
    class Inputs:
        l0_histogram: object
        number_of_partitions: int

    def __init__(self, params: agg.CalculatePrivateContributionBoundsParams, partitions, histograms,
                 backend=None, number_of_partitions: Optional[int] = None) -> None:
        self._params = params
        self._backend = backend
        self._partitions = partitions
        self._histograms = histograms
        self._number_of_partitions = number_of_partitions
        self._scoring_function = None
        self._result = None

    def calculate(self):
        """A one-element list holding the chosen bound (computed once)."""
        if self._result is None:
            sf = self.scoring_function()
            bound = dp_computations.ExponentialMechanism(sf).apply(self._params.calculation_eps, self.candidates())
            self._result = [int(bound)]
        return self._result

    def scoring_function(self) -> L0ScoringFunction:
        if self._scoring_function is None:
            (h,) = list(self._histograms)
            n = self._calculate_number_of_partitions()
            if isinstance(h, dict):  # device bins
                self._scoring_function = DeviceL0ScoringFunction(self._params, n, h["int_count"][0])
            else:
                self._scoring_function = L0ScoringFunction(self._params, n, h.l0_contributions_histogram)
        return self._scoring_function

    def candidates(self) -> List[int]:
        return generate_possible_contribution_bounds(
            self.scoring_function()._max_partitions_contributed_best_upper_bound())

    def probabilities(self):
        """(candidates, scores, probabilities) of the exponential mechanism:
        what calculate() draws from, without drawing (tests, diagnostics)."""
        sf = self.scoring_function()
        cands = self.candidates()
        probs = dp_computations.ExponentialMechanism(sf)._calculate_probabilities(self._params.calculation_eps, cands)
        return cands, [sf.score(k) for k in cands], probs

    def _calculate_number_of_partitions(self) -> int:
        if self._number_of_partitions is None:
            self._number_of_partitions = len(set(self._partitions))
        return self._number_of_partitions
