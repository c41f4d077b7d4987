"""Utility analysis, cross-partition stage: a NumPy restatement of what
pdp_utility_report computes (pipelinedp_amd.h; the reference's
analysis/cross_partition_combiners.py and the bucketing of
analysis/utility_analysis.py), the derived tolerances, and the fixture.

Restatement.  From per-partition arrays it forms every per-partition term with
the kernel's operation order (one NumPy operation per rounded step, x * x for
squares; NumPy's /, sqrt and * are correctly rounded, as the device's are), so
a device term equals a restated term bit for bit; it then sums each field with
math.fsum (the exact sum, rounded once).  Only the order of the sums differs.

Tolerances, U = 2^-52.
  * A sum S of n terms t: any two fp64 orders of summation differ by at most
    B_S = n U sum|t| (the rule of 3f; the exact sum lies between them).
  * Scaled fields S * (1 / W), W = sum keep > 0 (non-negative terms, so W = 0
    only when every term is 0, on both sides): with |S' - S| <= B_S and
    |W' - W| <= B_W < W,
      |S'/W' - S/W| <= (B_S + |S| B_W / W) / (W - B_W),
    plus three roundings (1 / W, the product, and one for the other side's
    pair): 3 U (|S| + B_S) / (W - B_W).  The dropped sums scale by
    1 / sum_actual in the same way with |sum_actual|; there B_a >= |a| (the
    actual values cancel) leaves no bound (inf) unless the caller states that
    the actual values add exactly in every order (`exact_actual`: integers, or
    dyadic values of one scale), which makes B_a = 0.
  * Against the recorded fixture (`fixture=True`): the reference squares with
    `**` (libm pow), which may differ from the rounded product by one ulp.  A
    quantity with relative slack a U keeps a U through a product or quotient
    with an exact operand and through a sum of non-negative terms (the larger
    a), halves it through sqrt, and gains U at every later rounding (the two
    sides may round apart).  l0_var: 1; var = l0_var + sn^2: 2;
    rmse = sqrt(bias^2 + var): 3; keep * rmse: 4; rmse_drop: 5; times the
    weight +1; divided by s +1, by s^2 (itself 1) +2.  So the terms of the
    eight absolute sums carry (0, 2, 0, 0, 0, 3, 4, 6) U and of the relative
    ones (0, 4, 0, 0, 0, 5, 5, 7) U: B_S grows to (n + c) U sum|t|.
  * Inputs that are themselves only known to a bound (`slack`: the device's
    per-partition arrays against the reference's, bounds of 3f) move a term by
    at most the first-order propagation written out in `_term_slack`; the sum
    of those is added to B_S.
Integer counts, configuration_index, strategies, noise_std, noise_kind and bin
bounds compare by equality.

Run as a script to regenerate tests/golden/utility_report/*.json: it runs the
reference's own perform_utility_analysis on LocalBackend over the cases of
utility_analysis_util.fixture_cases and the edge cases below, and records the
reports (and, for the edge cases, the per-partition output) as plain data.
"""
import bisect
import json
import math
import os

import numpy as np

from tests import utility_analysis_util as UA

ROOT = UA.ROOT
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "utility_report")
U = 2.0 ** -52
N_BUCKETS = 38
BOUNDS = tuple([0, 1] + [c * 10 ** i for i in range(1, 13) for c in (1, 2, 5)])
N_SEL, N_PER = 3, 20
# fixture slack per term of the 20 per-metric fields, in U (docstring)
FIXTURE_SLACK = (0, 0, 0, 0) + (0, 2, 0, 0, 0, 3, 4, 6) + (0, 4, 0, 0, 0, 5, 5, 7)


def bucket_of(size) -> int:
    if size < 0:
        return 0
    return bisect.bisect_right(BOUNDS, size) - 1


# ----------------------------------------------------------- restatement --
def metric_terms(s, cmin, cmax, el0, sl0, keep, sn):
    """The 20 per-partition terms of one metric, [20][P, K], in field order."""
    omk = 1 - keep
    linf_drop = cmin - cmax
    l0_drop = -el0
    after = (s - l0_drop) - linf_drop
    sel_drop = after * omk
    bias = (el0 + cmin) + cmax
    l0_var = sl0 * sl0
    var = l0_var + sn * sn
    rmse = np.sqrt(bias * bias + var)
    rmse_drop = keep * rmse + omk * np.abs(s)
    ab = [x * keep for x in (el0, l0_var, cmin, cmax, bias, var, rmse, rmse_drop)]
    zero = s == 0
    safe = np.where(zero, 1.0, s)
    s2 = safe * safe
    rel = [np.where(zero, 0.0, a / (s2 if i in (1, 5) else safe)) for i, a in enumerate(ab)]
    return [s + 0 * keep, l0_drop + 0 * keep, linf_drop + 0 * keep, sel_drop] + ab + rel


def _term_slack(s, cmin, cmax, el0, sl0, keep, sn, d):
    """First-order bound of how far each of the 20 terms moves when the inputs
    move by at most d = (ds, dcmin, dcmax, del0, dsl0, dkeep)."""
    ds, dcmin, dcmax, del0, dsl0, dkeep = d
    omk = 1 - keep
    after = (s + el0) - (cmin - cmax)
    bias = (el0 + cmin) + cmax
    dbias = del0 + dcmin + dcmax
    l0_var = sl0 * sl0
    dl0_var = 2 * np.abs(sl0) * dsl0 + dsl0 * dsl0
    var = l0_var + sn * sn
    rmse = np.sqrt(bias * bias + var)
    with np.errstate(divide="ignore", invalid="ignore"):
        drmse = np.where(rmse > 0, (np.abs(bias) * dbias + dbias * dbias + dl0_var) / rmse, dbias + np.sqrt(dl0_var))
    rmse_drop = keep * rmse + omk * np.abs(s)
    drmse_drop = dkeep * rmse + keep * drmse + dkeep * np.abs(s) + omk * ds
    x = (el0, l0_var, cmin, cmax, bias, var, rmse, rmse_drop)
    dx = (del0, dl0_var, dcmin, dcmax, dbias, dl0_var, drmse, drmse_drop)
    dab = [a * keep + np.abs(b) * dkeep + a * dkeep for a, b in zip(dx, x)]
    ab = [np.abs(b) * keep for b in x]
    zero = s == 0
    a_s = np.where(zero, 1.0, np.abs(s))
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.where(a_s > ds, a_s - ds, np.nan)  # no bound when s may be 0 on one side only
        drel = []
        for i in range(8):
            if i in (1, 5):
                drel.append(dab[i] / (lo * lo) + ab[i] * (2 * a_s * ds + ds * ds) / (a_s * a_s * lo * lo))
            else:
                drel.append(dab[i] / lo + ab[i] * ds / (a_s * lo))
        drel = [np.where(zero & (ds == 0), 0.0, np.where(np.isnan(v), np.inf, v)) for v in drel]
    dsel = (ds + del0 + dcmin + dcmax) * omk + np.abs(after) * dkeep
    return [ds + 0 * keep, del0 + 0 * keep, dcmin + dcmax + 0 * keep, dsel] + dab + drel


def restate_report(raw, keep, metrics, std_noise, public, exact_actual=False, fixture=False, slack=None):
    """(values [39, F, K], bounds [39, F, K], counts [39, 2]) of host arrays
    raw int [P, 2], keep float [P, K] (None when public), metrics float
    [M, 5, P, K], std_noise [M][K].  `slack`: None or (dmetrics [M, 5, P, K],
    dkeep [P, K]) bounds on the inputs."""
    raw = np.asarray(raw)
    M = 0 if metrics is None else len(metrics)
    P = raw.shape[0]
    K = metrics.shape[3] if M else keep.shape[1]
    keep_ = np.ones((P, K)) if public else np.asarray(keep, dtype=np.float64)
    dkeep = np.zeros((P, K)) if slack is None or public else slack[1]
    F = N_SEL + N_PER * M
    T = np.zeros((F, P, K))
    D = np.zeros((F, P, K))
    T[0], T[1], T[2] = keep_, keep_, keep_ * (1 - keep_)
    D[0], D[1], D[2] = dkeep, dkeep, dkeep * (np.abs(1 - 2 * keep_) + dkeep)
    for m in range(M):
        sn = np.asarray(std_noise[m], dtype=np.float64)[None, :]
        T[N_SEL + N_PER * m:N_SEL + N_PER * (m + 1)] = metric_terms(*metrics[m], keep_, sn)
        if slack is not None:
            D[N_SEL + N_PER * m:N_SEL + N_PER * (m + 1)] = _term_slack(*metrics[m], keep_, sn,
                                                                        tuple(slack[0][m]) + (dkeep,))
    part = raw[:, 0] > 0
    size = metrics[0, 0, :, 0] if M else raw[:, 0]
    bucket = np.array([bucket_of(x) for x in size])
    counts = np.zeros((N_BUCKETS + 1, 2), dtype=np.int64)
    vals = np.zeros((N_BUCKETS + 1, F, K))
    bnds = np.zeros((N_BUCKETS + 1, F, K))
    for e in range(N_BUCKETS + 1):
        idx = np.nonzero(part & ((bucket == e) | (e == N_BUCKETS)))[0]
        n = len(idx)
        if n == 0:
            continue
        empty = public & (raw[idx, 1] == 0)
        counts[e] = [n - int(empty.sum()), int(empty.sum())]
        S = np.zeros((F, K))
        B = np.zeros((F, K))
        for f in range(F):
            c = FIXTURE_SLACK[(f - N_SEL) % N_PER] if fixture and f >= N_SEL else 0
            for k in range(K):
                t = T[f, idx, k]
                S[f, k] = math.fsum(t)
                B[f, k] = (n + c) * U * math.fsum(np.abs(t)) + math.fsum(D[f, idx, k])
        if exact_actual:
            for m in range(M):
                B[N_SEL + N_PER * m] = 0.0
        vals[e], bnds[e] = S, B
        for m in range(M):
            base = N_SEL + N_PER * m
            for j in range(1, N_PER):
                den, bden = (S[base], B[base]) if j < 4 else (S[0], B[0])
                for k in range(K):
                    vals[e, base + j, k], bnds[e, base + j, k] = _scaled(
                        S[base + j, k], B[base + j, k], den[k], bden[k], one_if_zero=j < 4)
    return vals, bnds, counts


def _scaled(S, BS, W, BW, one_if_zero):
    """S * (W == 0 ? (1 or 0) : 1 / W) and its bound (docstring)."""
    if W == 0 and BW == 0:
        return (S, BS) if one_if_zero else (0.0, 0.0)
    a = abs(W)
    if BW >= a:
        return (S * (1.0 / W) if W != 0 else S), math.inf
    return S * (1.0 / W), (BS + abs(S) * BW / a) / (a - BW) + 3 * U * (abs(S) + BS) / (a - BW)


# ------------------------------------------------------------ flat records --
def _value_errors_list(v):
    b = v.bounding_errors
    return [b.l0.mean, b.l0.var, b.linf_min, b.linf_max, v.mean, v.variance, v.rmse, v.rmse_with_dropped_partitions]


def flatten_report(report, lower=None, upper=None):
    """Plain data of one UtilityReport (the reference's or the product's),
    without its histogram."""
    info = report.partitions_info
    kept = info.kept_partitions
    rec = dict(configuration=report.configuration_index, lower=lower, upper=upper,
               public_partitions=info.public_partitions, num_dataset_partitions=info.num_dataset_partitions,
               num_non_public_partitions=info.num_non_public_partitions,
               num_empty_partitions=info.num_empty_partitions,
               strategy=None if info.strategy is None else info.strategy.name,
               kept_partitions=None if kept is None else [float(kept.mean), float(kept.var)], metrics=None)
    if report.metric_errors is not None:
        rec["metrics"] = []
        for mu in report.metric_errors:
            d = mu.ratio_data_dropped
            assert mu.absolute_error.l1 == 0 and mu.absolute_error.l1_with_dropped_partitions == 0
            assert mu.relative_error.l1 == 0 and mu.relative_error.l1_with_dropped_partitions == 0
            rec["metrics"].append(dict(
                metric=str(mu.metric).split(".")[-1], noise_std=float(mu.noise_std), noise_kind=mu.noise_kind.name,
                values=[float(x) for x in [d.l0, d.linf, d.partition_selection] +
                        _value_errors_list(mu.absolute_error) + _value_errors_list(mu.relative_error)]))
    return rec


def flatten_reports(reports):
    """One record per configuration and bin: the all-partitions report
    (lower None) and then its histogram's bins."""
    out = []
    for r in sorted(reports, key=lambda r: r.configuration_index):
        out.append(flatten_report(r))
        for b in r.utility_report_histogram or []:
            assert b.report.utility_report_histogram is None
            out.append(flatten_report(b.report, b.partition_size_from, b.partition_size_to))
    return out


def records_of_arrays(vals, counts, public, strategies, std_noise, noise_kinds):
    """The flat records that `vals` / `counts` (restate_report's layout, or the
    device's) stand for; metric names are left out (None)."""
    K = vals.shape[2]
    M = (vals.shape[1] - N_SEL) // N_PER
    out = []
    for k in range(K):
        for e in [N_BUCKETS] + [b for b in range(N_BUCKETS) if counts[b].sum() > 0]:
            last = e == N_BUCKETS - 1
            rec = dict(configuration=k, lower=None if e == N_BUCKETS else BOUNDS[e],
                       upper=None if e == N_BUCKETS else (-1 if last else BOUNDS[e + 1]), public_partitions=public,
                       num_dataset_partitions=int(counts[e, 0]),
                       num_non_public_partitions=0 if public else None,
                       num_empty_partitions=int(counts[e, 1]) if public else None,
                       strategy=None if public else strategies[k],
                       kept_partitions=None if public else [float(vals[e, 1, k]), float(vals[e, 2, k])],
                       metrics=None, entry=e)
            if M:
                rec["metrics"] = [dict(metric=None, noise_std=float(std_noise[m][k]), noise_kind=noise_kinds[k],
                                       values=[float(x) for x in
                                               vals[e, N_SEL + N_PER * m + 1:N_SEL + N_PER * (m + 1), k]])
                                  for m in range(M)]
            out.append(rec)
    return out


EXACT_KEYS = ("configuration", "lower", "upper", "public_partitions", "num_dataset_partitions",
              "num_non_public_partitions", "num_empty_partitions", "strategy")


def assert_records_close(name, got, want, bnds, check_metric_names=False):
    """`got` and `want`: flat records in the same order; bnds [39, F, K] bounds
    the difference of every float; everything else is equal."""
    assert len(got) == len(want), (name, len(got), len(want))
    for g, w in zip(got, want):
        where = (name, w["configuration"], w["lower"])
        for key in EXACT_KEYS:
            assert g[key] == w[key], where + (key, g[key], w[key])
        e = N_BUCKETS if w["lower"] is None else bucket_of(w["lower"])
        k = w["configuration"]
        assert (g["kept_partitions"] is None) == (w["kept_partitions"] is None), where
        if w["kept_partitions"] is not None:
            for j in range(2):
                diff = abs(g["kept_partitions"][j] - w["kept_partitions"][j])
                assert diff <= bnds[e, 1 + j, k], where + ("kept", j, diff, bnds[e, 1 + j, k])
        assert (g["metrics"] is None) == (w["metrics"] is None), where
        for m, (gm, wm) in enumerate(zip(g["metrics"] or [], w["metrics"] or [])):
            assert gm["noise_std"] == wm["noise_std"] and gm["noise_kind"] == wm["noise_kind"], where + (m,)
            if check_metric_names:
                assert gm["metric"] == wm["metric"], where + (m,)
            assert len(gm["values"]) == len(wm["values"]) == N_PER - 1
            for j, (a, b) in enumerate(zip(gm["values"], wm["values"])):
                bound = bnds[e, N_SEL + N_PER * m + 1 + j, k]
                assert math.isfinite(a) and abs(a - b) <= bound, where + (m, j, a, b, abs(a - b), bound)


# --------------------------------------------------------------- fixture --
def edge_cases():
    """Pre-aggregated dyadic cases whose partition sizes sit on bucket edges:
    0 (a sum that cancels), just under 1, 1, 10, 19, 20, a negative total, 5e12
    and 1e13 (the last bucket, partition_size_to == -1)."""
    base = dict(l0=2, linf=3, min_sum=-8.0, max_sum=16.0, noise_kind="LAPLACE", strategy="TRUNCATED_GEOMETRIC",
                pre_threshold=None)
    sums = [[1.5, -1.5], [0.5, 0.25], [1.0], [4.0, 6.0], [19.0], [20.0], [-7.0, 2.0], [5e12], [1e13, 0.0]]
    pairs = [[pk, 1 + (i + pk) % 3, v, 2 ** ((i + pk) % 3)] for pk, vs in enumerate(sums) for i, v in enumerate(vs)]
    counts = [[1], [4, 6], [19], [5, 5, 5, 5], [0, 2]]
    cpairs = [[pk, c, float(c) / 2, 2 ** ((i + pk) % 2)] for pk, cs in enumerate(counts) for i, c in enumerate(cs)]
    return [
        dict(name="edge_private_sum_sizes", pairs=pairs, pre_aggregated=True, public_partitions=None,
             metrics=["SUM", "COUNT"], epsilon=1.0, delta=1e-5, base=base,
             multi=dict(max_partitions_contributed=[1, 2, 4], noise_kind=["LAPLACE", "GAUSSIAN", "LAPLACE"])),
        dict(name="edge_public_count_sizes", pairs=cpairs, pre_aggregated=True, public_partitions=[0, 1, 2, 3, 4, 9],
             metrics=["COUNT"], epsilon=1.0, delta=1e-5, base=dict(base, noise_kind="GAUSSIAN"),
             multi=dict(max_partitions_contributed=[1, 2], max_contributions_per_partition=[2, 8])),
    ]


def load_fixture():
    """Every recorded case: the case description (inputs, and `expected`, the
    reference's per-partition output) with `reports`, the flat records of the
    reference's perform_utility_analysis."""
    per_partition = {c["name"]: c for c in UA.load_fixture()}
    out = []
    for fname in sorted(os.listdir(GOLDEN_DIR)):
        if fname.endswith(".json"):
            with open(os.path.join(GOLDEN_DIR, fname)) as f:
                rec = json.load(f)
            case = rec["case"] if rec["case"] is not None else per_partition[rec["name"]]
            out.append(dict(case, reports=rec["reports"]))
    return out


def arrays_of_expected(case):
    """(partition keys, raw [P, 2], keep [P, K] | None, metrics [M, 5, P, K],
    std_noise [M][K], noise_kind [K]) of a case's recorded per-partition output."""
    exp = case["expected"]
    keys = sorted({e["partition"] for e in exp})
    K = 1 + max(e["configuration"] for e in exp)
    M = len(exp[0]["metrics"])
    public = case["public_partitions"] is not None
    raw = np.zeros((len(keys), 2), dtype=np.int64)
    keep = None if public else np.zeros((len(keys), K))
    metrics = np.zeros((M, 5, len(keys), K))
    std_noise = [[0.0] * K for _ in range(M)]
    noise_kind = [None] * K
    for e in exp:
        p, k = keys.index(e["partition"]), e["configuration"]
        raw[p] = e["raw"]
        if keep is not None:
            keep[p, k] = e["keep"]
        for m, rec in enumerate(e["metrics"]):
            metrics[m, :, p, k] = [rec[f] for f in UA.FIELDS]
            std_noise[m][k] = rec["std_noise"]
            noise_kind[k] = rec["noise_kind"]
    return keys, raw, keep, metrics, std_noise, noise_kind


def case_strategies(case):
    if case["public_partitions"] is not None:
        return None
    K = len(UA.case_configurations(case))
    multi = (case["multi"] or {}).get("partition_selection_strategy")
    return list(multi) if multi else [case["base"]["strategy"]] * K


def device_input_slack(case, keys, plans):
    """Bounds of 3f on the product's per-partition arrays against the
    reference's, as restate_report's `slack`: (dmetrics [M, 5, P, K], dkeep [P, K])."""
    pairs = UA.case_pairs(case)
    cfgs = UA.case_configurations(case)
    names = [m for m in UA.METRIC_ORDER if m in case["metrics"]]
    dm = np.zeros((len(names), 5, len(keys), len(cfgs)))
    dk = np.zeros((len(keys), len(cfgs)))
    for p, key in enumerate(keys):
        cnt, sm, npart = pairs[key]
        for k, cfg in enumerate(cfgs):
            if not UA.is_dyadic(case):
                for m, name in enumerate(names):
                    _, bounds = UA.restate_metric(name, cnt, sm, npart, cfg)
                    dm[m, :, p, k] = [bounds[f] for f in UA.FIELDS]
            if plans[k].keep_table is not None:
                val, path, length = UA.restate_keep(npart, cfg["l0"], UA.keep_fn_of_table(plans[k].keep_table))
                dk[p, k] = UA.keep_bound(val, path, len(npart), length)
    return dm, dk


def _record(case, lib):
    from analysis import utility_analysis
    options, ext, col, public = UA.build_options(case, lib)
    reports, per_partition = utility_analysis.perform_utility_analysis(col, lib.LocalBackend(), options, ext, public)
    flat = flatten_reports(list(reports))
    expected = []
    for (pk, k), m in per_partition:
        expected.append(dict(
            partition=pk, configuration=k, keep=None if public is not None else
            float(m.partition_selection_probability_to_keep),
            raw=[int(m.raw_statistics.privacy_id_count), int(m.raw_statistics.count)],
            metrics=[dict(aggregation=str(e.aggregation).split(".")[-1], std_noise=float(e.std_noise),
                          noise_kind=e.noise_kind.name, **{f: float(getattr(e, f)) for f in UA.FIELDS})
                     for e in m.metric_errors]))
    expected.sort(key=lambda e: (e["partition"], e["configuration"]))
    return flat, expected


def main():
    lib = UA._reference_lib()
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    shared = {c["name"] for c in UA.fixture_cases()}
    for case in UA.fixture_cases() + edge_cases():
        flat, expected = _record(case, lib)
        inline = None if case["name"] in shared else dict(case, expected=expected)
        with open(os.path.join(GOLDEN_DIR, case["name"] + ".json"), "w") as f:
            json.dump(dict(name=case["name"], case=inline, reports=flat), f, separators=(",", ":"))
        print(case["name"], len(flat), "records,", len({r["lower"] for r in flat}) - 1, "bins")


if __name__ == "__main__":
    main()
