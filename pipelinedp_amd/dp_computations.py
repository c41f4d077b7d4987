"""Host-side DP arithmetic: sensitivities, noise calibration, selection thresholds.

Mirrors pipeline_dp/dp_computations.py (reference) for the functions on the
aggregate path, and restates the arithmetic the reference delegates to
python-dp (PyDP ~=1.1.5rc4, Google differential-privacy C++):

* Gaussian sigma calibration (PyDP GaussianMechanism(eps, delta, l2).std,
  called at dp_computations.py:116, 489-491): analytic-Gaussian delta(sigma),
  doubling then bisection until hi - lo <= 1e-3 * lo, returning hi.
* Laplace diversity b = l1 / eps (PyDP LaplaceMechanism.diversity,
  dp_computations.py:439-440, 461).
* Partition selection (partition_selection.py:29-44 -> PyDP
  create_partition_strategy): truncated-geometric keep probability,
  Laplace / Gaussian thresholding thresholds.
* The secure noise of those mechanisms (PyDP add_noise, dp_computations.py:
  456-457, 508-509): Google's granularity-snapped samplers.  NoiseParams
  holds one mechanism's grid and sampler constants (pdp_noise_params); the
  kernels draw with them, SecureSampler draws single host values.

These are scalars computed once per aggregation on the host; the per-partition
work (noise draws, keep decisions) runs in the HIP kernels.
"""
import abc
import dataclasses
import functools
import math
from typing import Any, List, Optional, Tuple

import numpy as np

from pipelinedp_amd import aggregate_params as agg


@dataclasses.dataclass
class ScalarNoiseParams:
    """dp_computations.py:28-60."""
    eps: float
    delta: float
    min_value: Optional[float]
    max_value: Optional[float]
    min_sum_per_partition: Optional[float]
    max_sum_per_partition: Optional[float]
    max_partitions_contributed: int
    max_contributions_per_partition: Optional[int]
    noise_kind: agg.NoiseKind

    def __post_init__(self):
        assert (self.min_value is None) == (self.max_value is None), \
            "min_value and max_value should be or both set or both None."
        assert (self.min_sum_per_partition is None) == (self.max_sum_per_partition is None), \
            "min_sum_per_partition and max_sum_per_partition should be or both set or both None."

    def l0_sensitivity(self) -> int:
        return self.max_partitions_contributed

    @property
    def bounds_per_contribution_are_set(self) -> bool:
        return self.min_value is not None and self.max_value is not None

    @property
    def bounds_per_partition_are_set(self) -> bool:
        return self.min_sum_per_partition is not None and self.max_sum_per_partition is not None


def compute_squares_interval(min_value: float, max_value: float) -> Tuple[float, float]:
    """dp_computations.py:63-68."""
    if min_value < 0 < max_value:
        return 0, max(min_value**2, max_value**2)
    return min_value**2, max_value**2


def compute_middle(min_value: float, max_value: float) -> float:
    """dp_computations.py:71-75 (overflow-safe midpoint)."""
    return min_value + (max_value - min_value) / 2


def compute_l1_sensitivity(l0_sensitivity: float, linf_sensitivity: float) -> float:
    return l0_sensitivity * linf_sensitivity


def compute_l2_sensitivity(l0_sensitivity: float, linf_sensitivity: float) -> float:
    return np.sqrt(l0_sensitivity) * linf_sensitivity


# ----------------------------------------------------- Gaussian calibration --
_SIGMA_RELATIVE_ACCURACY = 1e-3


def _std_normal_cdf(x: float) -> float:
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def gaussian_delta(sigma: float, eps: float, l2_sensitivity: float) -> float:
    """delta of the Gaussian mechanism with std sigma (analytic Gaussian,
    Balle & Wang 2018): Phi(l2/(2s) - eps s/l2) - e^eps Phi(-l2/(2s) - eps s/l2)."""
    a = l2_sensitivity / (2.0 * sigma)
    b = eps * sigma / l2_sensitivity
    if eps < 700.0:
        return _std_normal_cdf(a - b) - math.exp(eps) * _std_normal_cdf(-a - b)
    # IEEE double semantics of the C++ restated here: e^eps overflows to inf,
    # inf * 0 = NaN, and a NaN delta never exceeds the target, so huge budgets
    # calibrate sigma down to 0 (the reference's "no noise" test budgets).
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float64(_std_normal_cdf(a - b)) -
                     np.exp(np.float64(eps)) * np.float64(_std_normal_cdf(-a - b)))


def compute_sigma(eps: float, delta: float, l2_sensitivity: float) -> float:
    """Smallest sigma (to 1e-3 relative, rounded up) with gaussian_delta <= delta.

    Restates PyDP GaussianMechanism(eps, delta, l2).std (reference
    dp_computations.py:106-116); reproduces the reference's known answers
    114.375, 88.06640625, 17.1826171875, 16.9125, 277.34375, 18.662109375,
    37.53742639189524 exactly."""
    if eps <= 0:
        raise ValueError(f"epsilon must be positive, but {eps} given")
    if not 0 < delta < 1:
        raise ValueError(f"delta must be in (0, 1) for the Gaussian mechanism, but {delta} given")
    if l2_sensitivity <= 0:
        raise ValueError(f"l2 sensitivity must be positive, but {l2_sensitivity} given")
    lo, hi = 0.0, float(l2_sensitivity)
    while gaussian_delta(hi, eps, l2_sensitivity) > delta:
        lo = hi
        hi *= 2.0
    while hi - lo > _SIGMA_RELATIVE_ACCURACY * lo:
        mid = lo * 0.5 + hi * 0.5
        if gaussian_delta(mid, eps, l2_sensitivity) > delta:
            lo = mid
        else:
            hi = mid
    return hi


def laplace_diversity(eps: float, l1_sensitivity: float) -> float:
    if eps <= 0:
        raise ValueError(f"epsilon must be positive, but {eps} given")
    return l1_sensitivity / eps


# --------------------------------------------------------------- secure noise --
_GRANULARITY_PARAM = float(1 << 40)  # Laplace: b / 2^40 -> the grid
_BINOMIAL_BOUND = float(1 << 57)     # Gaussian: about 2^57 binomial trials


def _next_power_of_two(x: float) -> float:
    return math.pow(2.0, math.ceil(math.log2(x))) if x > 0 else 0.0


@dataclasses.dataclass(frozen=True)
class NoiseParams:
    """One additive mechanism's secure sampler (pdp_noise_params).

    Laplace(eps, l1): granularity g = 2^ceil(log2(b / 2^40)), b = l1 / eps;
    noise = g * k with P(k) ~ exp(-lambda |k|), lambda = g eps / (l1 + g).
    Gaussian(sigma): g = 2^ceil(log2(2 sigma / 2^28.5)), sqrt_n = 2 sigma / g;
    noise = g * (Binomial(sqrt_n^2, 1/2) - sqrt_n^2 / 2) by rejection.
    add_noise(x) = round_to_multiple(x, g) + noise; g = 0: no noise."""
    kind: int                 # 0 Laplace, 1 Gaussian (N.NOISE_*)
    scale: float              # b or sigma
    granularity: float
    lam: float = 0.0
    step: int = 0
    n: float = 0.0
    bound: float = 0.0
    coef: float = 0.0
    corr: float = 0.0

    def to_c(self):
        from pipelinedp_amd import _native as N
        c = N.NoiseParams()
        c.kind, c.scale, c.granularity, c.lambda_ = self.kind, self.scale, self.granularity, self.lam
        c.step, c.n, c.bound, c.coef, c.corr = self.step, self.n, self.bound, self.coef, self.corr
        return c

    def as_dict(self) -> dict:
        return {"kind": self.kind, "scale": self.scale, "granularity": self.granularity,
                "lambda": self.lam, "step": self.step, "n": self.n, "bound": self.bound,
                "coef": self.coef, "corr": self.corr}


NO_NOISE = NoiseParams(kind=0, scale=0.0, granularity=0.0)


def laplace_noise_params(eps: float, l1_sensitivity: float) -> NoiseParams:
    """Google LaplaceDistribution(epsilon, sensitivity) constants."""
    b = laplace_diversity(eps, l1_sensitivity)
    # fail closed: granularity 0 means "no noise", which only a scale of
    # exactly 0 (zero sensitivity) may produce
    if not math.isfinite(b) or b < 0:
        raise ValueError(f"Laplace scale l1/eps = {l1_sensitivity}/{eps} must be finite and >= 0")
    if b == 0:
        return NoiseParams(kind=0, scale=0.0, granularity=0.0)
    g = _next_power_of_two(b / _GRANULARITY_PARAM)
    lam = g * eps / (l1_sensitivity + g) if g > 0 else 0.0
    if not (g > 0 and math.isfinite(g) and lam > 0 and math.isfinite(lam)):
        raise ValueError(f"Laplace scale {b} has no representable noise grid")
    return NoiseParams(kind=0, scale=b, granularity=g, lam=lam)


def gaussian_noise_params(sigma: float) -> NoiseParams:
    """Google GaussianDistribution(stddev) constants (binomial sampler)."""
    if not math.isfinite(sigma) or sigma < 0:
        raise ValueError(f"Gaussian sigma {sigma} must be finite and >= 0")
    if sigma == 0:
        return NoiseParams(kind=1, scale=0.0, granularity=0.0)
    g = _next_power_of_two(2.0 * sigma / math.sqrt(_BINOMIAL_BOUND))
    if g == 0.0 or not math.isfinite(g):
        raise ValueError(f"Gaussian sigma {sigma} has no representable noise grid")
    sqrt_n = 2.0 * sigma / g
    n = sqrt_n * sqrt_n
    return NoiseParams(kind=1, scale=sigma, granularity=g,
                       step=int(math.floor(math.sqrt(2.0) * sqrt_n + 1.0 + 0.5)), n=n,
                       bound=sqrt_n * math.sqrt(math.log(n) / 2), coef=math.sqrt(2 / math.pi) / sqrt_n,
                       corr=1 - 0.4 * math.pow(2 * math.log(n), 1.5) / sqrt_n)


def round_to_multiple(x: float, base: float) -> float:
    """RoundToNearestDoubleMultiple (ties toward zero)."""
    if base == 0.0:
        return x
    r = math.fmod(x, base)
    if abs(r) > base / 2:
        return x - r + math.copysign(base, r)
    return x - r


class SecureSampler:
    """Host draw of the same samplers for single values (API parity: the
    reference's mechanism.add_noise outside a pipeline).  Randomness comes
    from the OS CSPRNG; the pipelines' noise is drawn on the GPU."""

    def __init__(self):
        import secrets
        self._bits = secrets.randbits

    def _u01(self) -> float:
        return ((self._bits(53)) + 0.5) / 9007199254740992.0

    def _geometric(self, lam: float) -> int:
        lo, hi = 0, (1 << 63) - 1
        while lo + 1 < hi:
            mid = lo + ((hi - lo) >> 1)
            q = math.expm1(lam * float(lo - mid)) / math.expm1(lam * float(lo - hi))
            if q >= 1.0 or self._u01() <= q:
                hi = mid
            else:
                lo = mid
        return hi - 1

    def sample(self, p: NoiseParams) -> float:
        if p.granularity == 0.0:
            return 0.0
        if p.kind == 0:
            while True:
                positive = self._bits(1) == 1
                s = self._geometric(p.lam)
                if s == 0 and not positive:
                    continue
                return (float(s) if positive else -float(s)) * p.granularity
        while True:
            geom = 0
            while self._bits(1) == 1 and geom < 64:
                geom += 1
            two_sided = geom if self._bits(1) == 1 else -geom - 1
            m = p.step * two_sided + ((self._bits(64) * p.step) >> 64)
            u = self._u01()
            md = float(m)
            if abs(md) > p.bound:
                continue
            prob = p.coef * math.exp(-2.0 * md * md / p.n) * p.corr
            if prob > 0.0 and u < prob * float(p.step) * math.ldexp(1.0, geom) / 4.0:
                return md * p.granularity

    def add_noise(self, p: NoiseParams, x: float) -> float:
        if p.granularity == 0.0:
            return float(x)
        return round_to_multiple(float(x), p.granularity) + self.sample(p)


_SAMPLER = None


def secure_sampler() -> SecureSampler:
    global _SAMPLER
    if _SAMPLER is None:
        _SAMPLER = SecureSampler()
    return _SAMPLER


def equally_split_budget(eps: float, delta: float, no_mechanisms: int):
    """dp_computations.py:232-260: equal shares, the last one takes the remainder."""
    if no_mechanisms <= 0:
        raise ValueError("The number of mechanisms must be a positive integer.")
    eps_used = delta_used = 0
    budgets = []
    for _ in range(no_mechanisms - 1):
        budget = (eps / no_mechanisms, delta / no_mechanisms)
        eps_used += budget[0]
        delta_used += budget[1]
        budgets.append(budget)
    budgets.append((eps - eps_used, delta - delta_used))
    return budgets


# -------------------------------------------------------------- sensitivities --
@dataclasses.dataclass
class Sensitivities:
    """dp_computations.py:578-618."""
    l0: Optional[int] = None
    linf: Optional[float] = None
    l1: Optional[float] = None
    l2: Optional[float] = None

    def __post_init__(self):
        def check_is_positive(num: Any, name: str):
            if num is not None and num <= 0:
                raise ValueError(f"{name} must be positive, but {num} given.")

        check_is_positive(self.l0, "L0")
        check_is_positive(self.linf, "Linf")
        check_is_positive(self.l1, "L1")
        check_is_positive(self.l2, "L2")
        if (self.l0 is None) != (self.linf is None):
            raise ValueError("l0 and linf sensitivities must be either both set or both unset.")
        if self.l0 is not None and self.linf is not None:
            l1 = compute_l1_sensitivity(self.l0, self.linf)
            if self.l1 is None:
                self.l1 = l1
            elif abs(l1 - self.l1) > 1e-12:
                raise ValueError(f"L1={self.l1} != L0*Linf={l1}")
            l2 = compute_l2_sensitivity(self.l0, self.linf)
            if self.l2 is None:
                self.l2 = l2
            elif abs(l2 - self.l2) > 1e-12:
                raise ValueError(f"L2={self.l2} != sqrt(L0)*Linf={l2}")


def compute_sensitivities_for_count(params) -> Sensitivities:
    """dp_computations.py:718-724."""
    if params.max_contributions is not None:
        return Sensitivities(l1=params.max_contributions, l2=params.max_contributions)
    return Sensitivities(l0=params.max_partitions_contributed,
                         linf=params.max_contributions_per_partition)


def compute_sensitivities_for_privacy_id_count(params) -> Sensitivities:
    """dp_computations.py:727-732."""
    if params.max_contributions is not None:
        return Sensitivities(l1=params.max_contributions, l2=math.sqrt(params.max_contributions))
    return Sensitivities(l0=params.max_partitions_contributed, linf=1)


def compute_sensitivities_for_sum(params) -> Sensitivities:
    """dp_computations.py:735-748."""
    l0_sensitivity = params.max_partitions_contributed
    max_abs = lambda x, y: max(abs(x), abs(y))
    if params.bounds_per_contribution_are_set:
        max_abs_val = max_abs(params.min_value, params.max_value)
        if params.max_contributions:
            s = max_abs_val * params.max_contributions
            return Sensitivities(l1=s, l2=s)
        linf_sensitivity = max_abs_val * params.max_contributions_per_partition
    else:
        linf_sensitivity = max_abs(params.min_sum_per_partition, params.max_sum_per_partition)
    return Sensitivities(l0=l0_sensitivity, linf=linf_sensitivity)


def compute_sensitivities_for_normalized_sum(params) -> Sensitivities:
    """dp_computations.py:762-771."""
    max_abs_value = (params.max_value - params.min_value) / 2
    if params.max_contributions:
        s = max_abs_value * params.max_contributions
        return Sensitivities(l1=s, l2=s)
    return Sensitivities(l0=params.max_partitions_contributed,
                         linf=max_abs_value * params.max_contributions_per_partition)


# -------------------------------------------------------------- mechanisms --
class AdditiveMechanism:
    """Noise parameters of an additive mechanism (dp_computations.py:397-537).

    add_noise() draws on the host for single values (API parity, e.g.
    explain reports and tests); the per-partition noise of aggregate() is
    drawn on the GPU with the same parameters."""

    noise_kind: agg.NoiseKind

    @property
    def noise_parameter(self) -> float:
        raise NotImplementedError

    @property
    def std(self) -> float:
        raise NotImplementedError


class LaplaceMechanism(AdditiveMechanism):

    def __init__(self, epsilon: float, l1_sensitivity: float):
        self._epsilon = epsilon
        self._sensitivity = l1_sensitivity
        self._diversity = laplace_diversity(epsilon, l1_sensitivity)

    @classmethod
    def create_from_epsilon(cls, epsilon: float, l1_sensitivity: float) -> "LaplaceMechanism":
        return LaplaceMechanism(epsilon, l1_sensitivity)

    @classmethod
    def create_from_std_deviation(cls, normalized_stddev: float, l1_sensitivity: float):
        b = normalized_stddev / math.sqrt(2)
        return LaplaceMechanism(1 / b, l1_sensitivity)

    def secure_params(self) -> NoiseParams:
        return laplace_noise_params(self._epsilon, self._sensitivity)

    def add_noise(self, value) -> float:
        return secure_sampler().add_noise(self.secure_params(), value)

    @property
    def noise_kind(self) -> agg.NoiseKind:
        return agg.NoiseKind.LAPLACE

    @property
    def noise_parameter(self) -> float:
        return self._diversity

    @property
    def std(self) -> float:
        return self._diversity * math.sqrt(2)

    @property
    def sensitivity(self) -> float:
        return self._sensitivity

    def describe(self) -> str:
        return (f"Laplace mechanism:  parameter={self.noise_parameter}  eps="
                f"{self._epsilon}  l1_sensitivity={self.sensitivity}")


class GaussianMechanism(AdditiveMechanism):

    def __init__(self, sigma: float, l2_sensitivity: float, epsilon: float = 0.0,
                 delta: float = 0.0):
        self._sigma = sigma
        self._l2_sensitivity = l2_sensitivity
        self._epsilon = epsilon
        self._delta = delta

    @classmethod
    def create_from_epsilon_delta(cls, epsilon: float, delta: float, l2_sensitivity: float):
        return GaussianMechanism(compute_sigma(epsilon, delta, l2_sensitivity), l2_sensitivity,
                                 epsilon, delta)

    @classmethod
    def create_from_std_deviation(cls, normalized_stddev: float, l2_sensitivity: float):
        return GaussianMechanism(normalized_stddev * l2_sensitivity, l2_sensitivity)

    def secure_params(self) -> NoiseParams:
        return gaussian_noise_params(self._sigma)

    def add_noise(self, value) -> float:
        return secure_sampler().add_noise(self.secure_params(), value)

    @property
    def noise_kind(self) -> agg.NoiseKind:
        return agg.NoiseKind.GAUSSIAN

    @property
    def noise_parameter(self) -> float:
        return self._sigma

    @property
    def std(self) -> float:
        return self._sigma

    @property
    def sensitivity(self) -> float:
        return self._l2_sensitivity

    def describe(self) -> str:
        if self._epsilon > 0:
            eps_delta_str = f"eps={self._epsilon}  delta={self._delta}  "
        else:
            eps_delta_str = ""
        return (f"Gaussian mechanism:  parameter={self.noise_parameter}"
                f"  {eps_delta_str}l2_sensitivity={self.sensitivity}")


def create_additive_mechanism(mechanism_spec, sensitivities: Sensitivities) -> AdditiveMechanism:
    """dp_computations.py:621-646."""
    # by value, so the reference's own MechanismSpec / enums work too
    noise_kind = agg.NoiseKind(getattr(mechanism_spec.mechanism_type.to_noise_kind(), "value", None))
    if noise_kind == agg.NoiseKind.LAPLACE:
        if sensitivities.l1 is None:
            raise ValueError("L1 or (L0 and Linf) sensitivities must be set for Laplace mechanism.")
        if mechanism_spec.standard_deviation_is_set:
            return LaplaceMechanism.create_from_std_deviation(mechanism_spec.noise_standard_deviation,
                                                              sensitivities.l1)
        return LaplaceMechanism.create_from_epsilon(mechanism_spec.eps, sensitivities.l1)
    if noise_kind == agg.NoiseKind.GAUSSIAN:
        if sensitivities.l2 is None:
            raise ValueError("L2 or (L0 and Linf) sensitivities must be set for Gaussian mechanism.")
        if mechanism_spec.standard_deviation_is_set:
            return GaussianMechanism.create_from_std_deviation(
                mechanism_spec.noise_standard_deviation, sensitivities.l2)
        return GaussianMechanism.create_from_epsilon_delta(mechanism_spec.eps, mechanism_spec.delta,
                                                           sensitivities.l2)
    raise AssertionError(f"{noise_kind} not supported.")


class MeanMechanism:
    """dp_computations.py:540-575 (noise drawn on the GPU, see PDP_OP_MEAN)."""

    def __init__(self, range_middle: float, count_mechanism: AdditiveMechanism,
                 sum_mechanism: AdditiveMechanism):
        self._range_middle = range_middle
        self._count_mechanism = count_mechanism
        self._sum_mechanism = sum_mechanism

    @property
    def range_middle(self):
        return self._range_middle

    @property
    def count_mechanism(self):
        return self._count_mechanism

    @property
    def sum_mechanism(self):
        return self._sum_mechanism

    def compute_mean(self, count: int, normalized_sum: float):
        dp_count = self._count_mechanism.add_noise(count)
        denominator = max(1.0, dp_count)
        dp_normalized_sum = self._sum_mechanism.add_noise(normalized_sum)
        dp_mean = self._range_middle + dp_normalized_sum / denominator
        return dp_count, dp_mean * dp_count, dp_mean

    def describe(self) -> str:
        return (f"    a. Computed 'normalized_sum' = sum of (value - {self._range_middle})\n"
                f"    b. Applied to 'count' {self._count_mechanism.describe()}\n"
                f"    c. Applied to 'normalized_sum' {self._sum_mechanism.describe()}")


def create_mean_mechanism(range_middle, count_spec, count_sensitivities, normalized_sum_spec,
                          normalized_sum_sensitivities) -> MeanMechanism:
    return MeanMechanism(range_middle, create_additive_mechanism(count_spec, count_sensitivities),
                         create_additive_mechanism(normalized_sum_spec, normalized_sum_sensitivities))


def noise_params(noise_kind: agg.NoiseKind, eps: float, delta: float, l0: float, linf: float) -> NoiseParams:
    """Secure sampler of _add_random_noise (dp_computations.py:154-183) for
    (eps, delta, l0, linf)."""
    if noise_kind == agg.NoiseKind.LAPLACE:
        return laplace_noise_params(eps, compute_l1_sensitivity(l0, linf))
    if noise_kind == agg.NoiseKind.GAUSSIAN:
        return gaussian_noise_params(compute_sigma(eps, delta, compute_l2_sensitivity(l0, linf)))
    raise ValueError("Noise kind must be either Laplace or Gaussian.")


def noise_scale(noise_kind: agg.NoiseKind, eps: float, delta: float, l0: float, linf: float) -> float:
    """Scale (Laplace b or Gaussian sigma) of _add_random_noise
    (dp_computations.py:154-183) for (eps, delta, l0, linf)."""
    if noise_kind == agg.NoiseKind.LAPLACE:
        return laplace_diversity(eps, compute_l1_sensitivity(l0, linf))
    if noise_kind == agg.NoiseKind.GAUSSIAN:
        return compute_sigma(eps, delta, compute_l2_sensitivity(l0, linf))
    raise ValueError("Noise kind must be either Laplace or Gaussian.")


@functools.lru_cache(maxsize=8192)
def _cached_sigma(eps: float, delta: float, l0: int, linf: float) -> float:
    """compute_sigma per (eps, delta, l0, linf): the private-bounds score asks
    for one sigma per candidate bound (a few thousand bisections), again on
    every call with the same budget.  Bounded by entries (least recently used
    out first)."""
    return compute_sigma(eps, delta, compute_l2_sensitivity(l0, linf))


def _compute_noise_std(linf_sensitivity: float, dp_params: ScalarNoiseParams) -> float:
    """dp_computations.py:368-381."""
    if dp_params.noise_kind == agg.NoiseKind.LAPLACE:
        l1 = compute_l1_sensitivity(dp_params.l0_sensitivity(), linf_sensitivity)
        return laplace_diversity(dp_params.eps, l1) * np.sqrt(2)
    if dp_params.noise_kind == agg.NoiseKind.GAUSSIAN:
        return _cached_sigma(dp_params.eps, dp_params.delta, dp_params.l0_sensitivity(), linf_sensitivity)
    raise ValueError("Only Laplace and Gaussian noise is supported.")


def compute_dp_count_noise_std(dp_params: ScalarNoiseParams) -> float:
    """Noise standard deviation of a DP count (dp_computations.py:384-387):
    Laplace l0 * linf / eps * sqrt(2), Gaussian compute_sigma's."""
    return _compute_noise_std(dp_params.max_contributions_per_partition, dp_params)


# ---------------------------------------------------------- exponential mechanism --
class ExponentialMechanism:
    """Chooses one of a list of parameters differentially privately
    (dp_computations.py:661-715): P(k) proportional to
    exp(score(k) * eps / global_sensitivity), the denominator doubled for a
    non-monotonic score.  All in memory.

    One deviation from the reference: the exponents are shifted by their
    maximum before np.exp.  The reference's np.exp(scores * eps / sensitivity)
    underflows to all zeros (0 / 0 = NaN probabilities) once every exponent is
    below about -745; the shifted form is the same softmax, equal to the
    reference's wherever that one is finite."""

    class ScoringFunction(abc.ABC):
        """The score of a parameter: the higher, the likelier it is chosen."""

        @abc.abstractmethod
        def score(self, k) -> float:
            """Score of parameter k."""

        @property
        @abc.abstractmethod
        def global_sensitivity(self) -> float:
            """Global sensitivity of the score."""

        @property
        @abc.abstractmethod
        def is_monotonic(self) -> bool:
            """Whether, for neighbouring datasets D and D', score(D, k) >=
            score(D', k) for every k or <= for every k."""

    def __init__(self, scoring_function: "ExponentialMechanism.ScoringFunction") -> None:
        self._scoring_function = scoring_function

    def apply(self, eps: float, inputs_to_score_col: List[Any]) -> Any:
        probs = self._calculate_probabilities(eps, inputs_to_score_col)
        return np.random.default_rng().choice(inputs_to_score_col, p=probs)

    def _calculate_probabilities(self, eps: float, inputs_to_score_col: List[Any]):
        scores = np.array(list(map(self._scoring_function.score, inputs_to_score_col)))
        denominator = self._scoring_function.global_sensitivity
        if not self._scoring_function.is_monotonic:
            denominator *= 2
        exponents = scores * eps / denominator
        weights = np.exp(exponents - exponents.max())
        return weights / weights.sum()


# ------------------------------------------------------------------ vector sums --
@dataclasses.dataclass
class AdditiveVectorNoiseParams:
    """dp_computations.py:186-194."""
    eps_per_coordinate: float
    delta_per_coordinate: float
    max_norm: float
    l0_sensitivity: float
    linf_sensitivity: float
    norm_kind: agg.NormKind
    noise_kind: agg.NoiseKind


def clip_vector(vec: np.ndarray, max_norm: float, norm_kind: agg.NormKind) -> np.ndarray:
    """_clip_vector (dp_computations.py:197-209): Linf clips every coordinate
    to [-max_norm, max_norm]; L1 / L2 scale the vector by
    min(1, max_norm / norm), which is 1 for the zero vector."""
    vec = np.asarray(vec)
    kind = norm_kind.value
    if kind == "linf":
        return np.clip(vec, -max_norm, max_norm)
    if kind in ("l1", "l2"):
        norm = float(np.linalg.norm(vec, ord=int(kind[-1])))
        ratio = max_norm / norm if norm != 0 else math.inf
        return vec * min(1, ratio)
    raise NotImplementedError(f"Vector Norm of kind '{kind}' is not supported.")


def vector_noise_params(p: AdditiveVectorNoiseParams) -> NoiseParams:
    """The per-coordinate secure sampler of add_noise_vector: the sensitivities
    are the L0 / Linf contribution bounds, as the reference passes them."""
    return noise_params(p.noise_kind, p.eps_per_coordinate, p.delta_per_coordinate, p.l0_sensitivity,
                        p.linf_sensitivity)


def add_noise_vector(vec: np.ndarray, noise_params_: AdditiveVectorNoiseParams) -> np.ndarray:
    """add_noise_vector (dp_computations.py:212-229) on the host secure sampler:
    clip, then independent noise on every coordinate."""
    vec = clip_vector(vec, noise_params_.max_norm, noise_params_.norm_kind)
    np_ = vector_noise_params(noise_params_)
    smp = secure_sampler()
    return np.array([smp.add_noise(np_, s) for s in vec])


# ---------------------------------------------------------- partition selection --
def adjusted_delta(delta: float, max_partitions_contributed: int) -> float:
    """Per-partition delta: 1 - (1 - delta)^(1/l0), computed stably.

    Parity note: for l0 = 1 this is delta exactly; for l0 > 1 the reference's
    tests cannot distinguish it from delta / l0 (SURVEY §8(c) "parity unpinned")."""
    return -math.expm1(math.log1p(-delta) / max_partitions_contributed)


def truncated_geometric_keep_table(eps: float, delta: float, max_partitions_contributed: int,
                                   max_len: int = 1 << 22) -> np.ndarray:
    """The table below, computed once per parameter set (an aggregation
    recomputes it per call otherwise: a Python loop over the table's length).
    The returned array is read-only (it is shared)."""
    return _keep_table(float(eps), float(delta), int(max_partitions_contributed), int(max_len))


@functools.lru_cache(maxsize=256)
def _keep_table(eps: float, delta: float, max_partitions_contributed: int, max_len: int) -> np.ndarray:
    """pi[n] = probability that truncated-geometric selection keeps a partition
    with n privacy units (PyDP "truncated_geometric", the optimal (eps, delta)
    partition selection of Desfontaines et al.), n = 0..len-1; pi[len-1]
    applies to every larger n.  eps' = eps / l0, delta' = adjusted_delta.
    Recurrence: pi[0] = 0, pi[n] = min(e^eps' pi[n-1] + delta',
    1 - e^-eps' (1 - pi[n-1] - delta'), 1)."""
    if eps <= 0:
        raise ValueError(f"epsilon must be positive, but {eps} given")
    if not 0 <= delta < 1:
        raise ValueError(f"delta must be in [0, 1), but {delta} given")
    e = eps / max_partitions_contributed
    d = adjusted_delta(delta, max_partitions_contributed)
    ee, eme = math.exp(min(e, 700.0)), math.exp(-e)  # e^700 already saturates pi
    table = [0.0]
    p = 0.0
    while len(table) < max_len:
        p = min(ee * p + d, 1.0 - eme * (1.0 - p - d), 1.0)
        table.append(p)
        if p >= 1.0:
            break
        if d == 0.0 and len(table) > 1:  # delta = 0: never keep
            break
    out = np.asarray(table, dtype=np.float64)
    out.flags.writeable = False
    return out


def truncated_geometric_keep_probability(n: int, eps: float, delta: float,
                                         max_partitions_contributed: int,
                                         pre_threshold: Optional[int] = None) -> float:
    """PyDP partition_selection strategy .probability_of_keep(n)."""
    if pre_threshold:
        if n < pre_threshold:
            return 0.0
        n = n - (pre_threshold - 1)
    table = truncated_geometric_keep_table(eps, delta, max_partitions_contributed)
    return float(table[min(n, len(table) - 1)])


def laplace_thresholding_params(eps: float, delta: float, max_partitions_contributed: int):
    """(b, threshold) of PyDP "laplace" partition selection:
    b = l0 / eps, T = 1 - b ln(2 delta') (delta' <= 1/2), 1 + b ln(2 (1 - delta')) otherwise."""
    b = max_partitions_contributed / eps
    d = adjusted_delta(delta, max_partitions_contributed)
    if d > 0.5:
        return b, 1.0 + b * math.log(2.0 * (1.0 - d))
    return b, 1.0 - b * math.log(2.0 * d)


def _upper_std_normal_quantile(q: float) -> float:
    """Phi^-1(1 - q), computed as -Phi^-1(q) to keep precision for tiny q."""
    from scipy.special import ndtri
    return -float(ndtri(q))


def gaussian_thresholding_params(eps: float, delta: float, max_partitions_contributed: int):
    """(sigma, threshold) of PyDP "gaussian" partition selection: delta split
    half for the noise, half for the threshold; sigma calibrated with
    l2 = sqrt(l0); T = 1 + sigma * Phi^-1(1 - delta_threshold')."""
    noise_delta = delta / 2
    threshold_delta = delta - noise_delta
    sigma = compute_sigma(eps, noise_delta, math.sqrt(max_partitions_contributed))
    d = adjusted_delta(threshold_delta, max_partitions_contributed)
    return sigma, 1.0 + sigma * _upper_std_normal_quantile(d)
