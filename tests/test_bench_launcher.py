"""bench.py --gpus N without WORLD_SIZE starts N ranks itself (verdict r1:
--gpus was ignored).  CPU check of the launcher: --dry-run joins a gloo group
instead of touching a GPU; rank 0 reports the world size it sees."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                         timeout=180, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_gpus_2_spawns_two_ranks():
    r = _run("--gpus", "2", "--dry-run")
    assert r == {"dry_run": True, "n_gpus": 2, "requested": 2}


def test_default_is_one_rank():
    assert _run("--dry-run")["n_gpus"] == 1


def test_pmc_join_checks_the_source_tree(tmp_path):
    """bench.py joins a PMC summary only for its workload, size AND kernel
    sources (verdict r03 weak #5: a stale tree's counters were reported)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench
    from tree_id import source_tree_id
    f = tmp_path / "c3_pmc.json"
    body = {"workload": "c3 n=1000 ", "kernels": {"k_sieve_l1": {"hbm_bytes": 123.0}}}
    f.write_text(json.dumps(dict(body, tree="0123456789abcdef")))
    traffic, src, refused = bench.load_pmc(str(f), "c3", 1000, 1)
    assert traffic == {} and src is None and "profiled tree" in refused
    f.write_text(json.dumps(dict(body, tree=source_tree_id())))
    traffic, src, refused = bench.load_pmc(str(f), "c3", 1000, 1)
    assert traffic == {"k_sieve_l1": 123.0} and refused is None
    traffic, src, refused = bench.load_pmc(str(f), "c3", 2000, 1)  # another size
    assert traffic == {} and "workload" in refused
    assert bench.load_pmc(str(f), "c3", 1000, 2) == ({}, None, None)  # N > 1: never joined


def test_plain_run_is_the_default():
    """--full and --dump-outputs are off unless asked for."""
    sys.path.insert(0, ROOT)
    import bench
    args = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (args.full, args.dump_outputs, args.steps, args.warmup) == (False, None, 7, 2)
    args = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert args.full and args.dump_outputs == "somewhere"


def test_dump_outputs_writes_float_arrays(tmp_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    keys = np.arange(10, dtype=np.int64) * 3
    names = bench.dump_outputs(str(tmp_path), {"keys": keys, "f32": np.ones((10, 2), np.float32),
                                               "scalar": np.int64(5), "absent": None})
    assert names == ["f32", "keys", "scalar"]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["f32.npy", "keys.npy", "scalar.npy"]
    got = np.load(tmp_path / "keys.npy")
    assert got.dtype == np.float64 and (got == keys).all()
    assert np.load(tmp_path / "f32.npy").dtype == np.float32
    assert np.load(tmp_path / "scalar.npy").tolist() == [5.0]


def test_dump_outputs_samples_the_same_rows_within_the_budget(tmp_path, monkeypatch):
    """Past the byte budget every array keeps the same seeded share of its
    rows: arrays of one length keep the same rows, and so do two runs."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    n = 1000
    arrays = {"keys": np.arange(n), "cols": np.arange(n)[:, None] * np.ones((1, 3)), "other": np.arange(77.0)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, rank=1, world=2)
    a = {k: np.load(tmp_path / "a" / f"{k}.rank1.npy") for k in arrays}
    b = {k: np.load(tmp_path / "b" / f"{k}.rank1.npy") for k in arrays}
    assert sum(v.nbytes for v in a.values()) <= 4000
    assert 0 < len(a["keys"]) < n and len(a["keys"]) == len(a["cols"]) and 0 < len(a["other"]) < 77
    assert (np.diff(a["keys"]) > 0).all()
    assert (a["cols"] == a["keys"][:, None]).all()  # the same rows of both
    assert all((a[k] == b[k]).all() for k in arrays)


def test_pmc_kernel_names_match_the_library_profiler():
    """rocprofv3 names the template instances; the PMC summary must file them
    under the library profiler's names, or bench.py joins no bytes for them."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from pmc_summary import short_name
    ns = "void pdp::(anonymous namespace)::"
    assert short_name(ns + "k_h_float<true>(pdp::(anonymous namespace)::HT, ...)") == "k_h_float_max"
    assert short_name(ns + "k_h_float<false>(pdp::(anonymous namespace)::HT, ...)") == "k_h_float"
    assert short_name(ns + "k_split_scatter_staged(pdp::(anonymous namespace)::KP, ...)") == "k_split_scatter"
    assert short_name(ns + "k_scatter_l2_local<3, 256>(pdp::(anonymous namespace)::KP, ...)") == "k_scatter_l2"
    assert short_name(ns + "k_sieve_l1<3, false, true, 1024>(pdp::(anonymous namespace)::KP, ...)") == "k_sieve_l1"
