"""Timing of DPEngine.calculate_private_contribution_bounds' device path on
1e8 rows, 1e6 privacy ids, 1e5 partitions, half of the partitions allowed,
inputs resident in HBM.

Reports, each as the median of --steps timed runs after --warmup untimed ones
(HIP events around the work; the whole API call by a host clock, since it ends
in device-to-host reads):
  filter_ms      pdp_filter_rows (executor.filter_rows, with its count read-back)
  torch_filter_ms  the yardstick: the same filter with torch on the same
                 tensors in the same process (keep = allowed[pk]; pid[keep]; pk[keep])
  histograms_ms  executor.dataset_histograms on the filtered columns, no values
  score_ms       pdp_l0_impact_dropped for every candidate bound
  api_ms         the whole DPEngine.calculate_private_contribution_bounds call
                 on a ColumnTable of the device columns (Gaussian noise)
and the spread (min, max) of each.  Prints one JSON line.

Usage: python tools/bench_private_bounds.py [--steps 5] [--warmup 2] [--rows N]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, PIDS, PARTS = 100_000_000, 1_000_000, 100_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=ROWS)
    args = ap.parse_args()
    import numpy as np
    import torch

    import pipelinedp_amd as pdp
    from pipelinedp_amd import executor as X
    from pipelinedp_amd import private_contribution_bounds as pcb

    if not torch.cuda.is_available():
        raise SystemExit("bench_private_bounds.py needs a GPU")
    d = torch.device("cuda", 0)
    g = torch.Generator(device=d).manual_seed(1)
    n = args.rows
    pid = torch.randint(0, PIDS, (n,), device=d, generator=g)
    pk = torch.randint(0, PARTS, (n,), device=d, generator=g)
    allowed = torch.zeros(PARTS, dtype=torch.uint8, device=d)
    allowed[::2] = 1
    allowed_bool = allowed.bool()

    def timed(fn):
        """(median, min, max) ms of fn over the timed runs, by HIP events."""
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}

    def torch_filter():
        keep = allowed_bool[pk]
        return pid[keep], pk[keep]

    out = {"rows": n, "privacy_ids": PIDS, "partitions": PARTS, "allowed_partitions": PARTS // 2,
           "steps": args.steps, "warmup": args.warmup, "unit": "ms"}
    # the two filters alternate, so that both see the same machine state
    out["filter_ms"] = timed(lambda: X.filter_rows(pid, pk, allowed, n_partitions=PARTS))
    out["torch_filter_ms"] = timed(torch_filter)
    out["filter_ms_again"] = timed(lambda: X.filter_rows(pid, pk, allowed, n_partitions=PARTS))
    fpid, fpk = X.filter_rows(pid, pk, allowed, n_partitions=PARTS)
    tpid, tpk = torch_filter()
    assert fpid.numel() == tpid.numel()
    assert int(fpid.sum()) == int(tpid.sum()) and int(fpk.sum()) == int(tpk.sum())
    out["rows_kept"] = int(fpid.numel())
    del tpid, tpk
    ws = X.BoundWorkspace()
    out["histograms_ms"] = timed(lambda: X.dataset_histograms(fpid, fpk, None, n_privacy_ids=PIDS,
                                                              n_partitions=PARTS, workspace=ws))
    raw = X.dataset_histograms(fpid, fpk, None, n_privacy_ids=PIDS, n_partitions=PARTS, workspace=ws)
    bound = PARTS // 2
    cands = torch.as_tensor(np.asarray(pcb.generate_possible_contribution_bounds(bound), dtype=np.int64)).to(d)
    out["candidates"] = int(cands.numel())
    out["score_ms"] = timed(lambda: X.l0_impact_dropped(raw["int_count"][0], bound, cands))
    del fpid, fpk, raw

    table = pdp.ColumnTable({"user": pid, "part": pk}, n_privacy_ids=PIDS, n_partitions=PARTS)
    ex = pdp.DataExtractors(privacy_id_extractor=pdp.ColumnExtractor("user"),
                            partition_extractor=pdp.ColumnExtractor("part"))
    params = pdp.CalculatePrivateContributionBoundsParams(
        aggregation_noise_kind=pdp.NoiseKind.GAUSSIAN, aggregation_eps=1.0, aggregation_delta=1e-6,
        calculation_eps=1.0, max_partitions_contributed_upper_bound=PARTS)
    partitions = list(range(0, PARTS, 2))
    engine = pdp.DPEngine(pdp.NaiveBudgetAccountant(total_epsilon=1.0, total_delta=1e-6), pdp.ColumnarBackend())
    api = []
    for i in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = engine.calculate_private_contribution_bounds(table, params, ex, partitions)
        torch.cuda.synchronize()
        if i >= args.warmup:
            api.append((time.perf_counter() - t0) * 1e3)
    out["api_ms"] = {"median": statistics.median(api), "min": min(api), "max": max(api)}
    out["api_first_call_note"] = "warm-up calls fill the Gaussian sigma cache (one bisection per candidate)"
    out["bound"] = res[0].max_partitions_contributed
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
