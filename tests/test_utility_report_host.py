"""The cross-partition stage of utility analysis on the host (no GPU): the
NumPy restatement against the reports the reference recorded
(tests/golden/utility_report), the bucket lookup, the assembly of the
UtilityReport dataclasses from the kernel's output layout, and the argument
checks of the C entry points."""
import bisect
import ctypes
import dataclasses
import os

import numpy as np
import pytest

import pipelinedp_amd as pdp
from pipelinedp_amd import _native as N
from pipelinedp_amd import analysis
from pipelinedp_amd.analysis import utility_analysis as UAN
from tests import utility_report_util as R

FIXTURE = R.load_fixture()
IDS = [c["name"] for c in FIXTURE]


def test_fixture_is_complete():
    from tests import utility_analysis_util as UA
    assert sorted(IDS) == sorted(c["name"] for c in UA.fixture_cases() + R.edge_cases())
    by_name = {c["name"]: c for c in FIXTURE}
    bins = {n: sorted({r["lower"] for r in c["reports"] if r["lower"] is not None}) for n, c in by_name.items()}
    assert all(1 <= len(b) <= 5 for b in bins.values())
    assert bins["edge_private_sum_sizes"] == [0, 1, 10, 20, 5 * 10 ** 12]
    last = [r for r in by_name["edge_private_sum_sizes"]["reports"] if r["lower"] == 5 * 10 ** 12]
    assert last and all(r["upper"] == -1 and r["num_dataset_partitions"] == 2 for r in last)
    for name in ("raw_public_with_empty", "edge_public_count_sizes"):
        total = [r for r in by_name[name]["reports"] if r["lower"] is None]
        assert all(r["num_empty_partitions"] == 1 and r["num_non_public_partitions"] == 0 and
                   r["kept_partitions"] is None and r["strategy"] is None for r in total)


@pytest.mark.parametrize("case", FIXTURE, ids=IDS)
def test_restatement_equals_fixture(case):
    """The restatement, fed the reference's own per-partition output, gives the
    reference's reports within the fixture bound."""
    keys, raw, keep, metrics, std_noise, noise_kind = R.arrays_of_expected(case)
    public = case["public_partitions"] is not None
    vals, bnds, counts = R.restate_report(raw, keep, metrics, std_noise, public, exact_actual=case["pre_aggregated"],
                                          fixture=True)
    got = R.records_of_arrays(vals, counts, public, R.case_strategies(case), std_noise, noise_kind)
    assert np.isfinite(bnds).all()
    R.assert_records_close(case["name"], got, case["reports"], bnds)


def test_bucket_bounds_and_lookup():
    b = analysis.BUCKET_BOUNDS
    assert len(b) == N.UA_REPORT_BUCKETS == 38 and b[:5] == (0, 1, 10, 20, 50) and b[-1] == 5 * 10 ** 12
    assert all(float(x) == x for x in b) and b == R.BOUNDS
    probes = [-1e300, -1.0, -5e-324, 0.0, 5e-324, 0.999, 5e12, 1e13, 1e300]
    for x in b:
        probes += [float(x), float(np.nextafter(float(x), -np.inf)), float(np.nextafter(float(x), np.inf))]
    for x in probes:
        want = 0 if x < 0 else bisect.bisect_right(b, x) - 1
        assert UAN.bucket_index(x) == want == R.bucket_of(x), x
    assert UAN.bucket_index(19) == 2 and UAN.bucket_index(20) == 3 and UAN.bucket_index(0.99) == 0
    assert UAN.bucket_upper_bound(0) == 1 and UAN.bucket_upper_bound(36) == 5 * 10 ** 12
    assert UAN.bucket_upper_bound(37) == -1


def _hand_made(M, K, public=False):
    F = 3 + 20 * M
    report = np.arange(39 * F * K, dtype=np.float64).reshape(39, F, K) / 8
    counts = np.zeros((39, 2), dtype=np.int64)
    counts[2], counts[37] = ([3, 1] if public else [4, 0]), [2, 0]
    counts[38] = counts[:38].sum(axis=0)
    return report, counts


def test_assemble_private():
    report, counts = _hand_made(2, 3)
    names = [pdp.Metrics.SUM, pdp.Metrics.COUNT]
    std_noise = [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    kinds = [pdp.NoiseKind.LAPLACE, pdp.NoiseKind.GAUSSIAN, pdp.NoiseKind.LAPLACE]
    strategies = [pdp.PartitionSelectionStrategy.TRUNCATED_GEOMETRIC, pdp.PartitionSelectionStrategy.LAPLACE_THRESHOLDING,
                  pdp.PartitionSelectionStrategy.GAUSSIAN_THRESHOLDING]
    reports = UAN.assemble_reports(report, counts, names, std_noise, kinds, strategies)
    assert [r.configuration_index for r in reports] == [0, 1, 2]
    for k, r in enumerate(reports):
        assert isinstance(r, analysis.UtilityReport)
        info = r.partitions_info
        assert info == analysis.PartitionsInfo(False, 6, None, None, strategies[k],
                                               analysis.MeanVariance(report[38, 1, k], report[38, 2, k]))
        # empty buckets are left out; the last bucket's upper bound is -1
        assert [(b.partition_size_from, b.partition_size_to) for b in r.utility_report_histogram] == \
            [(10, 20), (5 * 10 ** 12, -1)]
        for e, b in zip((2, 37), r.utility_report_histogram):
            assert b.report.configuration_index == k and b.report.utility_report_histogram is None
            assert b.report.partitions_info.strategy == strategies[k]
            assert b.report.partitions_info.num_dataset_partitions == counts[e].sum() - counts[e, 1]
            assert b.report.partitions_info.kept_partitions.mean == report[e, 1, k]
        for m, mu in enumerate(r.metric_errors):
            f = report[38, 3 + 20 * m:23 + 20 * m, k]
            assert mu.metric == names[m] and mu.noise_std == std_noise[m][k] and mu.noise_kind == kinds[k]
            assert dataclasses.astuple(mu.ratio_data_dropped) == (f[1], f[2], f[3])
            a = mu.absolute_error
            assert (a.bounding_errors.l0.mean, a.bounding_errors.l0.var, a.bounding_errors.linf_min,
                    a.bounding_errors.linf_max, a.mean, a.variance, a.rmse, a.rmse_with_dropped_partitions) == \
                tuple(f[4:12])
            assert R._value_errors_list(mu.relative_error) == list(f[12:20])
            assert a.l1 == 0.0 and a.l1_with_dropped_partitions == 0.0
    # the flat record of the assembled dataclasses is the flat record of the arrays
    flat = R.flatten_reports(reports)
    want = R.records_of_arrays(report, counts, False, [s.name for s in strategies], std_noise, [k.name for k in kinds])
    R.assert_records_close("hand", flat, want, np.zeros_like(report))


def test_assemble_public_and_selection_only():
    report, counts = _hand_made(1, 2, public=True)
    reports = UAN.assemble_reports(report, counts, [pdp.Metrics.COUNT], [[1.0, 2.0]],
                                   [pdp.NoiseKind.GAUSSIAN] * 2, None)
    for r in reports:
        for rep, c in [(r, counts[38])] + [(b.report, counts[e]) for e, b in zip((2, 37), r.utility_report_histogram)]:
            assert rep.partitions_info == analysis.PartitionsInfo(True, int(c[0]), 0, int(c[1]), None, None)
    report, counts = _hand_made(0, 2)
    strategy = pdp.PartitionSelectionStrategy.TRUNCATED_GEOMETRIC
    reports = UAN.assemble_reports(report, counts, [], [], [None, None], [strategy] * 2)
    assert all(r.metric_errors is None and len(r.utility_report_histogram) == 2 for r in reports)
    assert all(b.report.metric_errors is None and b.report.partitions_info.strategy == strategy
               for r in reports for b in r.utility_report_histogram)


def test_to_relative():
    v = analysis.ValueErrors(analysis.ContributionBoundingErrors(analysis.MeanVariance(-2.0, 8.0), -1.0, -3.0),
                             mean=-6.0, variance=12.0, rmse=7.0, l1=0.0, rmse_with_dropped_partitions=9.0,
                             l1_with_dropped_partitions=0.0)
    r = v.to_relative(-2.0)
    assert R._value_errors_list(r) == [1.0, 2.0, 0.5, 1.5, 3.0, 3.0, -3.5, -4.5]
    assert R._value_errors_list(v.to_relative(0)) == [0] * 8
    assert analysis.DataDropInfo(1.0, 2.0, 3.0).partition_selection == 3.0
    assert analysis.MetricUtility(pdp.Metrics.SUM, 1.0, pdp.NoiseKind.LAPLACE, None, v, r).ratio_data_dropped is None
    assert analysis.UtilityReport(0, analysis.PartitionsInfo(True, 1)).utility_report_histogram is None


def test_c_abi_rejects_bad_arguments():
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = N.lib()
    need = ctypes.c_uint64(0)
    size = lib.pdp_utility_report_workspace_bytes
    assert size(100_000, 64, N.UA_COUNT | N.UA_SUM, ctypes.byref(need)) == 0
    # 5 B per partition and 43 fields x 64 doubles per 128 partitions
    assert 100_000 * 5 + 781 * 43 * 64 * 8 <= need.value < 100_000 * 6 + 900 * 43 * 64 * 8
    assert size(10, 64, N.UA_COUNT, None) == -1 and b"bytes" in lib.pdp_last_error()
    assert size(0, 64, N.UA_COUNT, ctypes.byref(need)) == -1 and b"n_partitions" in lib.pdp_last_error()
    assert size(1 << 31, 64, N.UA_COUNT, ctypes.byref(need)) == -4 and b"n_partitions" in lib.pdp_last_error()
    assert size(10, 0, N.UA_COUNT, ctypes.byref(need)) == -1 and b"n_configurations" in lib.pdp_last_error()
    assert size(10, N.MAX_CONFIGURATIONS + 1, N.UA_COUNT, ctypes.byref(need)) == -4
    assert b"PDP_MAX_CONFIGURATIONS" in lib.pdp_last_error()
    assert size(10, 1, 0x100, ctypes.byref(need)) == -1 and b"unknown utility analysis flags" in lib.pdp_last_error()
    assert size(10, 1, N.UA_PUBLIC, ctypes.byref(need)) == -1 and b"public partitions" in lib.pdp_last_error()
    assert size(10, 1, 0, ctypes.byref(need)) == 0  # selection only

    buf = ctypes.create_string_buffer(4096 + 256)
    host = (ctypes.addressof(buf) + 255) & ~255  # never dereferenced: every call below is refused first
    sn = (ctypes.c_double * 4)(1.0, 1.0, 1.0, 1.0)

    def call(raw=host, keep=host, metrics=host, P=10, K=1, flags=N.UA_COUNT, sn=sn, report=host, counts=host, ws=host,
             ws_bytes=1 << 40):
        return lib.pdp_utility_report(raw, keep, metrics, P, K, flags, sn, report, counts, ws, ws_bytes, None)
    assert call(raw=None) == -1 and b"raw_statistics" in lib.pdp_last_error()
    assert call(keep=None) == -1 and b"keep_probability" in lib.pdp_last_error()
    assert call(metrics=None) == -1 and b"metrics" in lib.pdp_last_error()
    assert call(sn=None) == -1 and b"std_noise" in lib.pdp_last_error()
    assert call(report=None) == -1 and b"report" in lib.pdp_last_error()
    assert call(counts=None) == -1 and b"counts" in lib.pdp_last_error()
    assert call(P=0) == -1 and call(P=1 << 31) == -4
    assert call(K=0) == -1 and call(K=N.MAX_CONFIGURATIONS + 1) == -4
    assert call(flags=0x10) == -1 and b"unknown utility analysis flags" in lib.pdp_last_error()
    assert call(flags=N.UA_PUBLIC) == -1 and b"public partitions" in lib.pdp_last_error()
    assert call(ws=None) == -3
    assert call(ws_bytes=16) == -3 and b"workspace too small" in lib.pdp_last_error()
    assert call(ws=host + 8) == -1 and b"aligned" in lib.pdp_last_error()
