"""bench.py on the GPU at a small C3 shape (2e6 rows, 2e4 privacy ids, 1e6
Zipf partitions), run in this process through bench.main:

* a plain run launches the timed path warmup + steps times and nothing else,
  and its line holds the headline figures;
* --dump-outputs writes the last timed step's outputs, the same from run to
  run and the same with --full (whose extra passes come after the dump).
"""
import json
import os

import numpy as np
import pytest

import bench
from pipelinedp_amd import executor as X

pytestmark = pytest.mark.gpu

ROWS, STEPS, WARMUP = 2_000_000, 3, 2
ARGS = ["--gpus", "1", "--rows", str(ROWS), "--privacy-ids", "20000", "--steps", str(STEPS), "--warmup", str(WARMUP)]
FILES = ["acc_count", "acc_normalized_sum", "acc_privacy_id_count", "metrics", "partition_index"]


def _run(capsys, *extra):
    bench.main([*ARGS, *extra])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    assert sorted(os.listdir(d)) == [f + ".npy" for f in FILES]
    return {f: np.load(os.path.join(d, f + ".npy")) for f in FILES}


def test_plain_run_times_the_steps_and_nothing_else(device, capsys, monkeypatch):
    calls = {"bound": 0, "select": 0}
    bound, select = X.bound_and_reduce, X.select_and_noise

    def counted_bound(*a, **kw):
        calls["bound"] += 1
        return bound(*a, **kw)

    def counted_select(*a, **kw):
        calls["select"] += 1
        return select(*a, **kw)

    monkeypatch.setattr(X, "bound_and_reduce", counted_bound)
    monkeypatch.setattr(X, "select_and_noise", counted_select)
    r = _run(capsys)
    assert calls == {"bound": WARMUP + STEPS, "select": WARMUP + STEPS}
    assert (r["steps"], r["warmup"], r["n_gpus"], r["full"]) == (STEPS, WARMUP, 1, False)
    assert (r["unit"], r["higher_is_better"], r["dtype"], r["workload_name"]) == ("rows/s", True, "f64", "c3")
    assert r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(ROWS / (r["ms_per_step"] * 1e-3), rel=1e-9)
    assert 0 < r["path_roofline"]["frac"] < 1
    assert 0 < r["partitions_kept"] <= 1_000_000
    # what --full adds is absent, not stale
    assert r["kernels"] is None and r["roofline"] is None and r["api"] is None and "secondary" not in r
    assert r["cpu_baseline"] is None and r["step_ms_spread"] is None


def test_dump_outputs_repeat_and_precede_the_full_passes(device, capsys, tmp_path):
    dirs = [str(tmp_path / d) for d in ("a", "b", "full")]
    ra = _run(capsys, "--dump-outputs", dirs[0])
    _run(capsys, "--dump-outputs", dirs[1])
    rf = _run(capsys, "--dump-outputs", dirs[2], "--full", "--no-cpu-baseline")
    a, b, f = (_load(d) for d in dirs)
    kept = ra["partitions_kept"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert a["partition_index"].shape == (kept,) and a["metrics"].shape == (kept, 3)
    assert (np.diff(a["partition_index"]) > 0).all() and a["partition_index"][-1] < 1_000_000
    assert a["acc_count"].shape == (1_000_000,)
    # Linf = 1: one row per kept (privacy id, partition) pair; L0 = 2 pairs per id at most
    assert (a["acc_count"] == a["acc_privacy_id_count"]).all()
    assert 0 < a["acc_count"].sum() <= 2 * 20000
    assert (a["acc_count"][a["partition_index"].astype(np.int64)] > 0).all()
    for other in (b, f):
        for name in ("partition_index", "acc_count", "acc_privacy_id_count"):
            np.testing.assert_array_equal(other[name], a[name])
        # fp64 atomic sums in another order: the parity bar of the GPU tests;
        # the noisy metrics snap to their mechanism's granularity (far below 1e-6)
        np.testing.assert_allclose(other["acc_normalized_sum"], a["acc_normalized_sum"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(other["metrics"], a["metrics"], rtol=0, atol=1e-6)
    assert rf["full"] and rf["kernels"] and rf["roofline"]["kernel"] in rf["kernels"]
    assert rf["api"]["ms_per_call"] > 0 and rf["step_ms_spread"]["n"] == STEPS
    assert rf["bound_plan"]["stats"] is not None and rf["partitions_kept"] == kept
