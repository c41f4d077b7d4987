"""The C-ABI boundary (include/pipelinedp_amd.h) on the CPU: the library loads,
exports every declared entry point, its ctypes mirror has the C struct layout
and constants, and the host-only entry points (plan, workspace sizing, argument
validation, error reporting) behave.  No device work is launched."""
import ctypes
import os
import re
import subprocess

import pytest

from pipelinedp_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pipelinedp_amd.h")

STRUCTS = {
    "pdp_bound_config": N.BoundConfig,
    "pdp_bound_plan_info": N.BoundPlanInfo,
    "pdp_partition_accumulators": N.PartitionAccumulators,
    "pdp_select_config": N.SelectConfig,
    "pdp_metric_op": N.MetricOp,
    "pdp_histogram_bins": N.HistogramBins,
    "pdp_bound_stats": N.BoundStats,
}


def _header_text():
    with open(HEADER) as f:
        src = f.read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_functions():
    return sorted(set(re.findall(r"\b(pdp_[a-z0-9_]+)\s*\(", _header_text())))


def declared_constants():
    return {m.group(1): int(m.group(2), 0) for m in
            re.finditer(r"#define\s+PDP_([A-Z0-9_]+)\s+\(?(-?(?:0x[0-9A-Fa-f]+|\d+))\)?", _header_text())}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return N.lib()


def test_every_declared_function_is_exported(lib):
    fns = declared_functions()
    assert len(fns) >= 13
    assert set(fns) == set(N.EXPORTED_SYMBOLS)
    for name in fns:
        assert hasattr(lib, name), name


def test_constants_match_header():
    consts = declared_constants()
    skip = {"ABI_VERSION"}
    checked = 0
    for name, value in consts.items():
        if name.startswith("E_") or name == "OK" or name in skip:
            continue
        py = name[:-4] if name.endswith("_MAX") else name
        if hasattr(N, py):
            assert getattr(N, py) == value, name
            checked += 1
    assert checked >= 25
    assert consts["ABI_VERSION"] == N.ABI_VERSION


def test_struct_layouts_match_c(tmp_path):
    """sizeof / offsetof of every ABI struct, compiled by gcc from the header,
    equal the ctypes mirror's."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pipelinedp_amd.h"', "int main(void) {"]
    for cname, cls in STRUCTS.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{cname} {field} %zu\\n", offsetof({cname}, {field}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        s, f, v = line.split()
        got[(s, f)] = int(v)
    for cname, cls in STRUCTS.items():
        assert got[(cname, "size")] == ctypes.sizeof(cls), cname
        for field, _ in cls._fields_:
            assert got[(cname, field)] == getattr(cls, field).offset, (cname, field)


def _cfg(**kw):
    c = N.BoundConfig()
    c.n_rows, c.n_privacy_ids, c.n_partitions = 100_000_000, 1_000_000, 100_000
    c.l0, c.linf, c.value_kind, c.flags = 8, 2, N.VALUE_F64, N.ACC_NSUM
    c.min_value, c.max_value, c.middle = 0.0, 10.0, 5.0
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_abi_version_and_plan(lib):
    assert lib.pdp_abi_version() == N.ABI_VERSION
    info = N.BoundPlanInfo()
    assert lib.pdp_bound_plan(ctypes.byref(_cfg()), ctypes.byref(info)) == 0
    assert info.algorithm == N.ALGO_BUCKETED and info.merge == N.MERGE_RANGES
    assert info.pk_bits == 17 and info.n_ranges == 49
    assert info.n_buckets << info.bucket_bits >= 1_000_000
    assert info.lds_bytes <= 160 * 1024
    assert 64 - info.rand_shift >= 24
    # forced global path and forced atomic merge resolve as asked
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(algorithm=N.ALGO_GLOBAL_SKETCH)), ctypes.byref(info)) == 0
    assert info.algorithm == N.ALGO_GLOBAL_SKETCH and info.n_buckets == 0
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(merge=N.MERGE_ATOMIC)), ctypes.byref(info)) == 0
    assert info.merge == N.MERGE_ATOMIC
    # > 1024 ranges of 2,048 partitions: the two-level range merge, <= 256
    # coarse ranges in the bucket kernel (P = 1e7: 153 of 65,536 partitions)
    for merge in (N.MERGE_AUTO, N.MERGE_RANGES):
        assert lib.pdp_bound_plan(ctypes.byref(_cfg(n_partitions=10_000_000, merge=merge)), ctypes.byref(info)) == 0
        assert info.merge == N.MERGE_RANGES and info.n_ranges == 153


def test_sieve_plan(lib):
    """Threshold sieve (Plan.sieve): AUTO picks t = (l0 + 3 sqrt(l0) + 3) / (0.6 rows per id)
    up to 0.35 (C3: 0.154, C2: 0.325; C4 with 10 rows per id: off), a forced value is
    clamped to 1/2, < 0 is off, and small (one-level) plans never sieve."""
    info = N.BoundPlanInfo()
    c3 = dict(n_rows=1_000_000_000, n_privacy_ids=10_000_000, n_partitions=1_000_000, l0=2, linf=1)
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(**c3)), ctypes.byref(info)) == 0
    assert abs(info.sieve / 65536 - (2 + 3 * 2 ** 0.5 + 3) / 60) < 1e-4
    assert lib.pdp_bound_plan(ctypes.byref(_cfg()), ctypes.byref(info)) == 0  # C2
    assert abs(info.sieve / 65536 - (8 + 3 * 8 ** 0.5 + 3) / 60) < 1e-4
    c4 = dict(n_rows=125_000_000, n_privacy_ids=12_500_000, n_partitions=10_000_000, l0=4, linf=2)
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(**c4)), ctypes.byref(info)) == 0
    assert info.sieve == 0
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(**c4, sieve=4096)), ctypes.byref(info)) == 0
    assert info.sieve == 4096 and info.key_format == N.KEYS_PACKED64  # 8-byte level-2 records (row in the key)
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(**c3, sieve=-1)), ctypes.byref(info)) == 0
    assert info.sieve == 0
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(**c3, sieve=1 << 20)), ctypes.byref(info)) == 0
    assert info.sieve == 1 << 15
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(n_rows=1_000_000, n_privacy_ids=5000, sieve=4096)),
                              ctypes.byref(info)) == 0
    assert info.sieve == 0  # one bucket level: no tile-local level 1
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(merge=N.MERGE_ATOMIC, sieve=4096)), ctypes.byref(info)) == 0
    assert info.sieve == 0  # the fix-up appends pair records: range merge only
    # the side band: auto for t <= 1/4 at t2 = 2t (C3 yes, C2 no), forced on / off
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(**c3)), ctypes.byref(info)) == 0
    assert info.band == 2 * info.sieve
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(**c3, sieve_band=-1)), ctypes.byref(info)) == 0
    assert info.band == 0 and info.sieve > 0
    assert lib.pdp_bound_plan(ctypes.byref(_cfg()), ctypes.byref(info)) == 0  # C2
    assert info.band == 0
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(sieve_band=1)), ctypes.byref(info)) == 0
    assert info.band == 1 << 15  # 2t capped at 1/2
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(**c3, sieve=-1)), ctypes.byref(info)) == 0
    assert info.band == 0
    # the sieve's workspace holds the fix-up state and twice the pair records
    on, off = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib.pdp_bound_workspace_bytes(ctypes.byref(_cfg(**c3)), ctypes.byref(on)) == 0
    assert lib.pdp_bound_workspace_bytes(ctypes.byref(_cfg(**c3, sieve=-1)), ctypes.byref(off)) == 0
    assert on.value > off.value


def test_workspace_bytes(lib):
    small, big = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib.pdp_bound_workspace_bytes(ctypes.byref(_cfg(n_rows=1000)), ctypes.byref(small)) == 0
    assert lib.pdp_bound_workspace_bytes(ctypes.byref(_cfg()), ctypes.byref(big)) == 0
    assert 0 < small.value < big.value
    # bucketed, compact records: two levels of (4 B record + 4 B row), the
    # bucket kernel's candidate list (4 B key + 4 B index) + pair records
    # (8 B key + 8 B nsum per kept slot)
    assert big.value >= 100_000_000 * 24 + 1_000_000 * 8 * 16
    # + the sieve's side band: one 8 B (id, row) slot per row, and pair
    # records for the main launch and the band's two fix-up launches
    assert big.value < 100_000_000 * 34 + 3 * 1_000_000 * 8 * 16 + (64 << 20)
    wide = ctypes.c_uint64(0)
    assert lib.pdp_bound_workspace_bytes(ctypes.byref(_cfg(key_format=N.KEYS_WIDE)), ctypes.byref(wide)) == 0
    assert wide.value >= 100_000_000 * 36 + 1_000_000 * 8 * 16
    cb = ctypes.c_uint64(0)
    assert lib.pdp_compact_workspace_bytes(1 << 20, ctypes.byref(cb)) == 0 and cb.value > 0


@pytest.mark.parametrize("field,value,code,msg", [
    ("l0", -1, -4, b"l0"), ("linf", -1, -4, b"linf"),
    ("max_contributions", -1, -4, b"max_contributions"),
    ("n_rows", 1 << 32, -1, b"n_rows"), ("n_partitions", 0, -1, b"n_partitions"),
    ("n_privacy_ids", 0, -1, b"n_privacy_ids"), ("value_kind", 7, -1, b"value_kind"),
    ("algorithm", 9, -1, b"algorithm"), ("merge", 5, -1, b"merge"), ("key_format", 6, -1, b"key_format"),
])
def test_invalid_configs_are_rejected(lib, field, value, code, msg):
    info = N.BoundPlanInfo()
    rc = lib.pdp_bound_plan(ctypes.byref(_cfg(**{field: value})), ctypes.byref(info))
    assert rc == code
    assert msg in lib.pdp_last_error()


def test_pair_table_modes_plan(lib):
    """l0 = 0 (LinfSampler / NoOpSampler), max_contributions and
    rows_are_units resolve to the pair-table algorithm; their exclusions
    mirror AggregateParams (aggregate_params.py:344-369)."""
    info = N.BoundPlanInfo()
    for kw in (dict(l0=0), dict(l0=0, linf=0), dict(l0=0, linf=0, max_contributions=5),
               dict(l0=0, linf=0, rows_are_units=1)):
        assert lib.pdp_bound_plan(ctypes.byref(_cfg(**kw)), ctypes.byref(info)) == 0, kw
        assert info.algorithm == N.ALGO_PAIR_TABLE
        ws = ctypes.c_uint64(0)
        assert lib.pdp_bound_workspace_bytes(ctypes.byref(_cfg(**kw)), ctypes.byref(ws)) == 0
        assert ws.value > 0
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(l0=2, linf=0, max_contributions=5)), ctypes.byref(info)) == -1
    assert b"max_contributions" in lib.pdp_last_error()
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(l0=0, linf=1, rows_are_units=1)), ctypes.byref(info)) == -1
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(l0=0, algorithm=N.ALGO_BUCKETED)), ctypes.byref(info)) == -4
    # PAIR_TABLE with cross-partition sampling: L0 over the table's distinct pairs
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(l0=2, algorithm=N.ALGO_PAIR_TABLE)), ctypes.byref(info)) == 0
    assert info.algorithm == N.ALGO_PAIR_TABLE
    # bounds above 256 (l0, linf, max_contributions) resolve to the pair table
    for kw in (dict(l0=257), dict(l0=2, linf=300), dict(l0=100_000, linf=100_000),
               dict(l0=0, linf=0, max_contributions=10_000), dict(l0=2**31 - 1, linf=1)):
        assert lib.pdp_bound_plan(ctypes.byref(_cfg(**kw)), ctypes.byref(info)) == 0, kw
        assert info.algorithm == N.ALGO_PAIR_TABLE, kw
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(l0=300, algorithm=N.ALGO_BUCKETED)), ctypes.byref(info)) == -4
    # rows_are_units needs no privacy-id column
    cfg = _cfg(n_rows=10, l0=0, linf=0, rows_are_units=1)
    need = ctypes.c_uint64(0)
    lib.pdp_bound_workspace_bytes(ctypes.byref(cfg), ctypes.byref(need))
    rc = lib.pdp_bound_contributions(ctypes.byref(cfg), None, None, None, None, ctypes.c_void_p(256),
                                     need.value, None)
    assert rc == -1 and b"key columns" in lib.pdp_last_error()


def test_sum_int_needs_int_values(lib):
    info = N.BoundPlanInfo()
    rc = lib.pdp_bound_plan(ctypes.byref(_cfg(flags=N.ACC_SUM | N.SUM_INT)), ctypes.byref(info))
    assert rc == -1 and b"PDP_SUM_INT" in lib.pdp_last_error()


@pytest.mark.parametrize("bound", [float("nan"), float("inf"), -float("inf"), 2.5, 2.0 ** 63, -(2.0 ** 64)])
@pytest.mark.parametrize("fields,flags", [(("min_value", "max_value"), N.ACC_SUM | N.SUM_INT),
                                          (("min_sum", "max_sum"), N.SUM_PER_PARTITION | N.SUM_INT)])
def test_sum_int_needs_int64_bounds(lib, fields, flags, bound):
    """With PDP_SUM_INT the kernels clip in int64 with (long long)bound: a
    bound that is not finite, not integral or outside [-2^63, 2^63) is refused
    (-4) before any device work; the largest and smallest int64 bounds pass."""
    info = N.BoundPlanInfo()
    ok = dict(value_kind=N.VALUE_I64, flags=flags, min_value=0.0, max_value=7.0, min_sum=-3.0, max_sum=9.0)
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(**ok)), ctypes.byref(info)) == 0
    edge = dict(ok, **{fields[0]: -(2.0 ** 63), fields[1]: 2.0 ** 63 - 1024.0})
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(**edge)), ctypes.byref(info)) == 0
    for f in fields:
        cfg = _cfg(**dict(ok, **{f: bound}))
        assert lib.pdp_bound_plan(ctypes.byref(cfg), ctypes.byref(info)) == -4
        assert b"PDP_SUM_INT" in lib.pdp_last_error() and f.encode() in lib.pdp_last_error()
        nbytes = ctypes.c_uint64(0)
        assert lib.pdp_bound_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)) == -4
        rc = lib.pdp_bound_contributions(ctypes.byref(cfg), None, None, None, None, None, 0, None)
        assert rc == -4
    # the other pair of bounds is not cast with these flags: any value passes
    other = ("min_sum", "max_sum") if fields[0] == "min_value" else ("min_value", "max_value")
    free = dict(ok, **{other[0]: -float("inf"), other[1]: float("inf")})
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(**free)), ctypes.byref(info)) == 0


def test_null_arguments_are_rejected_before_device_work(lib):
    cfg = _cfg(n_rows=10)
    assert lib.pdp_bound_plan(ctypes.byref(cfg), None) == -1
    assert lib.pdp_bound_workspace_bytes(ctypes.byref(cfg), None) == -1
    assert lib.pdp_bound_plan(None, ctypes.byref(N.BoundPlanInfo())) == -1
    # workspace too small: refused before any launch
    rc = lib.pdp_bound_contributions(ctypes.byref(cfg), None, None, None, None, None, 0, None)
    assert rc == -3
    # key columns missing with a big enough (fake, never dereferenced) workspace pointer
    need = ctypes.c_uint64(0)
    lib.pdp_bound_workspace_bytes(ctypes.byref(cfg), ctypes.byref(need))
    rc = lib.pdp_bound_contributions(ctypes.byref(cfg), None, None, None, None, ctypes.c_void_p(256),
                                     need.value, None)
    assert rc == -1 and b"key columns" in lib.pdp_last_error()


def test_dataset_histograms_arguments(lib):
    need = ctypes.c_uint64(0)
    assert lib.pdp_dataset_histograms_workspace_bytes(1000, 100, 10, ctypes.byref(need)) == 0
    # pair table (1.5 slots of 32 bytes per row) + per-pid / per-partition arrays
    assert need.value >= 1500 * 32 + 100 * 8 + 10 * 16
    assert lib.pdp_dataset_histograms_workspace_bytes(-1, 100, 10, ctypes.byref(need)) == -1
    assert lib.pdp_dataset_histograms_workspace_bytes(10, 100, 10, None) == -1
    out = N.HistogramBins()  # every output NULL: refused before device work
    rc = lib.pdp_dataset_histograms(None, None, None, N.VALUE_F64, 10, 100, 10, ctypes.byref(out), None, 0, None)
    assert rc == -1 and b"output" in lib.pdp_last_error()
    fake = N.HistogramBins(*([256] * 8))  # never dereferenced: the shape checks fail first
    rc = lib.pdp_dataset_histograms(None, None, None, N.VALUE_F64, 1 << 31, 100, 10, ctypes.byref(fake), None, 0,
                                    None)
    assert rc == -4
    rc = lib.pdp_dataset_histograms(None, None, None, N.VALUE_F64, 10, 1 << 40, 1 << 30, ctypes.byref(fake),
                                    None, 0, None)
    assert rc == -4 and b"63 bits" in lib.pdp_last_error()
    rc = lib.pdp_dataset_histograms(None, None, None, N.VALUE_F64, 10, 100, 10, ctypes.byref(fake), None, 0, None)
    assert rc == -1 and b"workspace" in lib.pdp_last_error()


def test_debug_corrupt_flag_needs_test_hooks(lib, monkeypatch):
    """PDP_DEBUG_CORRUPT_RECORDS (it overwrites level-2 records on purpose)
    is rejected unless PIPELINEDP_AMD_TEST_HOOKS=1."""
    nbytes = ctypes.c_uint64(0)
    cfg = _cfg(flags=N.ACC_NSUM | N.DEBUG_CORRUPT_RECORDS)
    monkeypatch.delenv("PIPELINEDP_AMD_TEST_HOOKS", raising=False)
    assert lib.pdp_bound_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)) == -1
    assert b"test hook" in lib.pdp_last_error()
    monkeypatch.setenv("PIPELINEDP_AMD_TEST_HOOKS", "1")
    assert lib.pdp_bound_workspace_bytes(ctypes.byref(cfg), ctypes.byref(nbytes)) == 0


def test_sieve_threads_plan(lib):
    """sieve_threads: 0 (auto) and 1024 resolve to 1,024-thread level-1
    workgroups, 512 to two per CU when their LDS fits; other values fail."""
    info = N.BoundPlanInfo()
    c3 = dict(n_rows=1_000_000_000, n_privacy_ids=10_000_000, n_partitions=1_000_000, l0=2, linf=1)
    for want, got in ((0, 1024), (1024, 1024), (512, 512)):
        assert lib.pdp_bound_plan(ctypes.byref(_cfg(**c3, sieve_threads=want)), ctypes.byref(info)) == 0
        assert info.sieve > 0 and info.sieve_threads == got
    assert lib.pdp_bound_plan(ctypes.byref(_cfg(**c3, sieve=-1)), ctypes.byref(info)) == 0
    assert info.sieve_threads == 0
    nbytes = ctypes.c_uint64(0)
    assert lib.pdp_bound_workspace_bytes(ctypes.byref(_cfg(**c3, sieve_threads=256)), ctypes.byref(nbytes)) == -1


# ------------------------------------------------------- the release path --
# Argument validation of pdp_select.hip's entry points.  Every call below is
# refused (or, for the one pinned exception, accepted) before any device work;
# the non-NULL pointers are host dummies that are never dereferenced.
_DUMMY = ctypes.create_string_buffer(4096 + 16)
_HOST = (ctypes.addressof(_DUMMY) + 15) & ~15  # 16-byte aligned


def _noise(family="laplace", **kw):
    """A valid mechanism of `family`, then the C fields in kw overwritten."""
    from pipelinedp_amd import dp_computations as dpc
    c = {"laplace": dpc.laplace_noise_params(1.0, 1.0), "gaussian": dpc.gaussian_noise_params(2.0)}[family].to_c()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


BAD_NOISE = [
    ("laplace", dict(kind=7), b"bad noise kind"),
    ("laplace", dict(granularity=float("nan")), b"granularity must be finite"),
    ("laplace", dict(granularity=-1.0), b"granularity must be finite"),
    ("laplace", dict(scale=-1.0), b"scale must be finite"),
    ("laplace", dict(scale=float("inf")), b"scale must be finite"),
    ("laplace", dict(granularity=0.0), b"granularity 0 with a nonzero scale"),
    ("laplace", dict(lambda_=0.0), b"Laplace noise needs"),
    ("laplace", dict(lambda_=float("inf")), b"Laplace noise needs"),
    ("gaussian", dict(step=0), b"Gaussian noise needs"),
    ("gaussian", dict(step=1 << 32), b"Gaussian noise needs"),
    ("gaussian", dict(n=1.0), b"Gaussian noise needs"),
    ("gaussian", dict(bound=0.0), b"Gaussian noise needs"),
    ("gaussian", dict(coef=float("nan")), b"Gaussian noise needs"),
]
_BAD_NOISE_IDS = [f"{k}-{next(iter(kw))}={next(iter(kw.values()))}" for k, kw, _ in BAD_NOISE]


def _select_cfg(**kw):
    c = N.SelectConfig()
    c.n_partitions, c.strategy, c.max_rows_per_privacy_id = 10, N.SELECT_ALL_NONEMPTY, 1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _select(lib, cfg, row_count=_HOST, keep=_HOST):
    return lib.pdp_select_partitions(None if cfg is None else ctypes.byref(cfg), row_count, keep, None, None)


def test_select_partitions_arguments(lib):
    assert _select(lib, None) == -1 and b"NULL argument" in lib.pdp_last_error()
    assert _select(lib, _select_cfg(), keep=None) == -1 and b"NULL argument" in lib.pdp_last_error()
    assert _select(lib, _select_cfg(n_partitions=-1)) == -1 and b"n_partitions < 0" in lib.pdp_last_error()
    for strategy in (-1, 5):
        assert _select(lib, _select_cfg(strategy=strategy)) == -1 and b"bad strategy" in lib.pdp_last_error()
    assert _select(lib, _select_cfg(strategy=N.SELECT_PUBLIC)) == -1 and b"public_mask" in lib.pdp_last_error()
    tg = N.SELECT_TRUNCATED_GEOMETRIC
    assert _select(lib, _select_cfg(strategy=tg, keep_table_len=4)) == -1 and b"keep_prob" in lib.pdp_last_error()
    for length in (0, -3):
        assert _select(lib, _select_cfg(strategy=tg, keep_prob=_HOST, keep_table_len=length)) == -1
        assert b"keep_prob" in lib.pdp_last_error()
    for strategy, extra in ((N.SELECT_ALL_NONEMPTY, {}), (tg, dict(keep_prob=_HOST, keep_table_len=4)),
                            (N.SELECT_LAPLACE_THRESHOLDING, dict(noise=_noise()))):
        assert _select(lib, _select_cfg(strategy=strategy, **extra), row_count=None) == -1
        assert b"row_count" in lib.pdp_last_error()
    # a valid configuration of zero partitions is accepted without a launch
    assert _select(lib, _select_cfg(n_partitions=0)) == 0


@pytest.mark.parametrize("strategy", [N.SELECT_LAPLACE_THRESHOLDING, N.SELECT_GAUSSIAN_THRESHOLDING])
@pytest.mark.parametrize("kind,fields,msg", BAD_NOISE, ids=_BAD_NOISE_IDS)
def test_select_partitions_rejects_bad_noise(lib, strategy, kind, fields, msg):
    """Both thresholding strategies check their mechanism, whichever its kind."""
    assert _select(lib, _select_cfg(strategy=strategy, noise=_noise(kind, **fields))) == -1
    assert msg in lib.pdp_last_error()
    # the other strategies do not read the mechanism
    assert _select(lib, _select_cfg(n_partitions=0, noise=_noise(kind, **fields))) == 0


def test_compact_arguments(lib):
    need = ctypes.c_uint64(0)
    assert lib.pdp_compact_workspace_bytes(5000, ctypes.byref(need)) == 0 and need.value == 256
    assert lib.pdp_compact_workspace_bytes(-1, ctypes.byref(need)) == -1
    assert lib.pdp_compact_workspace_bytes(10, None) == -1
    assert lib.pdp_compact(_HOST, -1, _HOST, _HOST, _HOST, 256, None) == -1 and b"bad argument" in lib.pdp_last_error()
    assert lib.pdp_compact(_HOST, 10, _HOST, None, _HOST, 256, None) == -1 and b"bad argument" in lib.pdp_last_error()
    assert lib.pdp_compact(_HOST, 10, _HOST, _HOST, None, 256, None) == -3
    assert b"workspace too small" in lib.pdp_last_error()
    assert lib.pdp_compact(_HOST, 10, _HOST, _HOST, _HOST, 255, None) == -3
    # 4,096 elements per block count: 32 x 4,096 + 1 elements need 33 counts = 264 bytes -> 512
    assert lib.pdp_compact_workspace_bytes(32 * 4096 + 1, ctypes.byref(need)) == 0 and need.value == 512
    assert lib.pdp_compact(_HOST, 32 * 4096 + 1, _HOST, _HOST, _HOST, 256, None) == -3
    assert lib.pdp_compact(None, 10, _HOST, _HOST, _HOST, 256, None) == -1 and b"NULL argument" in lib.pdp_last_error()
    assert lib.pdp_compact(_HOST, 10, None, _HOST, _HOST, 256, None) == -1 and b"NULL argument" in lib.pdp_last_error()


def _acc(**missing):
    a = N.PartitionAccumulators()
    for name, _ in N.PartitionAccumulators._fields_:
        setattr(a, name, None if name in missing else _HOST)
    return a


def _op(kind, **kw):
    op = N.MetricOp()
    op.kind = kind
    for m in range(3):
        op.noise[m] = _noise()
    for j in range(4):
        op.out_col[j] = j
    for k, v in kw.items():
        setattr(op, k, v)
    return op


def _metrics(lib, ops, n_ops=None, *, index=_HOST, n_kept=10, acc=None, noised=_HOST, out=_HOST, stride=10,
             acc_null=False):
    arr = None if ops is None else (N.MetricOp * max(len(ops), 1))(*ops)
    n_ops = (0 if ops is None else len(ops)) if n_ops is None else n_ops
    acc = _acc() if acc is None else acc
    return lib.pdp_noise_metrics(arr, n_ops, index, n_kept, None, 0, None if acc_null else ctypes.byref(acc), 0,
                                 noised, out, stride, 1, None)


def test_noise_metrics_arguments(lib):
    count = [_op(N.OP_COUNT)]
    for n_ops in (-1, 9):
        assert _metrics(lib, count * 9, n_ops) == -1 and b"bad ops" in lib.pdp_last_error()
    assert _metrics(lib, None, 1) == -1 and b"bad ops" in lib.pdp_last_error()
    assert _metrics(lib, count, acc_null=True) == -1 and b"bad ops" in lib.pdp_last_error()
    assert _metrics(lib, count, n_kept=-1) == -1 and b"n_kept / out_stride" in lib.pdp_last_error()
    assert _metrics(lib, count, n_kept=10, stride=9) == -1 and b"n_kept / out_stride" in lib.pdp_last_error()
    assert _metrics(lib, count, index=None) == -1 and b"NULL argument" in lib.pdp_last_error()
    assert _metrics(lib, count, out=None) == -1 and b"NULL argument" in lib.pdp_last_error()
    assert _metrics(lib, [_op(99)]) == -1 and b"unknown op kind" in lib.pdp_last_error()
    assert _metrics(lib, [_op(0)]) == -1 and b"unknown op kind" in lib.pdp_last_error()
    assert _metrics(lib, count + [_op(99)]) == -1 and b"unknown op kind" in lib.pdp_last_error()  # every op is checked
    assert _metrics(lib, [], 0) == 0  # no ops: nothing to do


@pytest.mark.parametrize("kind,missing,msg", [
    (N.OP_COUNT, "count", b"COUNT needs"), (N.OP_SUM, "sum", b"SUM needs"),
    (N.OP_PRIVACY_ID_COUNT, "privacy_id_count", b"privacy_id_count"),
    (N.OP_MEAN, "count", b"MEAN needs"), (N.OP_MEAN, "normalized_sum", b"MEAN needs"),
    (N.OP_VARIANCE, "count", b"VARIANCE needs"), (N.OP_VARIANCE, "normalized_sum", b"VARIANCE needs"),
    (N.OP_VARIANCE, "normalized_sum_sq", b"VARIANCE needs"),
])
def test_noise_metrics_needs_each_ops_accumulator(lib, kind, missing, msg):
    assert _metrics(lib, [_op(kind)], acc=_acc(**{missing: True})) == -1
    assert msg in lib.pdp_last_error()


def test_noise_metrics_thresholded_pid_needs_the_noised_count(lib):
    assert _metrics(lib, [_op(N.OP_THRESHOLDED_PID)], noised=None) == -1
    assert b"THRESHOLDED_PID needs noised_count" in lib.pdp_last_error()


@pytest.mark.parametrize("op_kind,mech", [(N.OP_COUNT, 0), (N.OP_MEAN, 0), (N.OP_MEAN, 1), (N.OP_VARIANCE, 0),
                                          (N.OP_VARIANCE, 1), (N.OP_VARIANCE, 2)])
@pytest.mark.parametrize("kind,fields,msg", BAD_NOISE[:1] + BAD_NOISE[5:7] + BAD_NOISE[8:9],
                         ids=_BAD_NOISE_IDS[:1] + _BAD_NOISE_IDS[5:7] + _BAD_NOISE_IDS[8:9])
def test_noise_metrics_checks_every_mechanism(lib, op_kind, mech, kind, fields, msg):
    """MEAN's second and VARIANCE's second and third mechanisms are checked
    like the first, in an op that is not the first of its list."""
    op = _op(op_kind)
    op.noise[mech] = _noise(kind, **fields)
    assert _metrics(lib, [_op(N.OP_COUNT), op]) == -1
    assert msg in lib.pdp_last_error()


def test_noise_metrics_zero_kept_skips_the_op_checks(lib):
    """Pins today's order of checks: with n_kept == 0 pdp_noise_metrics returns
    PDP_OK before it validates the ops, so an unknown kind, a missing
    accumulator or a bad mechanism pass unnoticed there.  (n_ops, the ops
    pointer and out_stride are checked first and still refused.)"""
    bad = _op(N.OP_MEAN)
    bad.noise[1] = _noise(kind=7)
    for ops, acc in (([_op(99)], None), ([_op(N.OP_COUNT)], _acc(count=True)), ([bad], None)):
        assert _metrics(lib, ops, n_kept=0, stride=0, acc=acc) == 0
        assert _metrics(lib, ops, n_kept=10, acc=acc) == -1
    assert _metrics(lib, [_op(99)] * 9, n_kept=0, stride=0) == -1
    assert _metrics(lib, [_op(99)], n_kept=0, stride=-1) == -1


def test_add_noise_arguments(lib):
    ok = _noise()
    call = lib.pdp_add_noise
    assert call(_HOST, N.VALUE_F64, -1, ctypes.byref(ok), 1, 0, _HOST, None) == -1 and b"n must be" in lib.pdp_last_error()
    for kind in (N.VALUE_NONE, 3):
        assert call(_HOST, kind, 4, ctypes.byref(ok), 1, 0, _HOST, None) == -1 and b"value_kind" in lib.pdp_last_error()
    assert call(_HOST, N.VALUE_F64, 4, None, 1, 0, _HOST, None) == -1 and b"noise params are NULL" in lib.pdp_last_error()
    assert call(None, N.VALUE_F64, 4, ctypes.byref(ok), 1, 0, _HOST, None) == -1 and b"NULL argument" in lib.pdp_last_error()
    assert call(_HOST, N.VALUE_I64, 4, ctypes.byref(ok), 1, 0, None, None) == -1 and b"NULL argument" in lib.pdp_last_error()
    for values, out in ((_HOST + 8, _HOST), (_HOST, _HOST + 8), (_HOST + 4, _HOST + 4)):
        assert call(values, N.VALUE_F64, 4, ctypes.byref(ok), 1, 0, out, None) == -1
        assert b"16-byte aligned" in lib.pdp_last_error()
    assert call(None, N.VALUE_I64, 0, ctypes.byref(ok), 1, 0, None, None) == 0  # nothing to do


def test_vector_sum_metrics_arguments(lib):
    ok = _noise()

    def call(d=8, norm=N.NORM_L2, max_norm=1.0, n_kept=4, noise=ok, vacc=_HOST):
        return lib.pdp_vector_sum_metrics(vacc, d, norm, max_norm, None if noise is None else ctypes.byref(noise),
                                          _HOST, n_kept, None, 0, _HOST, 1, None)
    for d in (0, -1, N.MAX_VECTOR_SIZE + 1):
        assert call(d=d) == -4 and b"vector_size" in lib.pdp_last_error()
    for norm in (-1, 3):
        assert call(norm=norm) == -1 and b"norm_kind" in lib.pdp_last_error()
    for max_norm in (-1.0, float("nan"), -float("inf")):
        assert call(max_norm=max_norm) == -1 and b"max_norm" in lib.pdp_last_error()
    assert call(n_kept=-1) == -1 and b"n_kept" in lib.pdp_last_error()
    assert call(noise=_noise("gaussian", step=0)) == -1 and b"Gaussian noise needs" in lib.pdp_last_error()
    assert call(vacc=None) == -1 and b"NULL argument" in lib.pdp_last_error()
    assert call(d=N.MAX_VECTOR_SIZE, n_kept=0) == 0  # the largest size passes the checks; nothing kept: no launch
