"""NumPy statement of pdp_merge_quantile_leaves (include/pipelinedp_amd.h) and
the inputs its tests share.

A case is a list of runs, each a list of n_partitions ascending uint16 arrays
(run s's codes of partition p).  Element j of run s of partition p, with code
x, goes to

    offsets[p] + j + #{codes <= x in the runs before s} + #{codes < x in the runs after s}

of the merged array: ties go by run, then by index, so the places of a
partition's elements are a permutation of its slots.
"""
import numpy as np


def flatten(case):
    """(runs uint16 [n_leaves], run_counts uint32 [n_runs, n_partitions]) in
    the layout the entry point reads: run-major, then partition-major."""
    counts = np.array([[len(seg) for seg in run] for run in case], dtype=np.uint32).reshape(len(case), -1)
    parts = [np.asarray(seg, dtype=np.uint16) for run in case for seg in run]
    runs = np.concatenate(parts) if parts else np.zeros(0, np.uint16)
    return runs.astype(np.uint16), counts


def merged_offsets(run_counts):
    """offsets[n_partitions + 1]: the exclusive scan of the column sums."""
    col = run_counts.astype(np.int64).sum(axis=0)
    return np.concatenate([[0], np.cumsum(col)]).astype(np.int64)


def merge_positions(runs, run_counts):
    """The destination of every element of `runs`, by the formula above."""
    n_runs, P = run_counts.shape
    run_off = np.concatenate([[0], np.cumsum(run_counts.astype(np.int64).ravel())])
    off = merged_offsets(run_counts)
    pos = np.empty(len(runs), dtype=np.int64)
    for p in range(P):
        segs = [runs[run_off[s * P + p]:run_off[s * P + p + 1]] for s in range(n_runs)]
        for s, seg in enumerate(segs):
            at = off[p] + np.arange(len(seg), dtype=np.int64)
            for r, other in enumerate(segs):
                if r != s:
                    at = at + np.searchsorted(other, seg, side="right" if r < s else "left")
            pos[run_off[s * P + p]:run_off[s * P + p] + len(seg)] = at
    return pos


def merge_by_positions(runs, run_counts):
    """(leaves, offsets) by scattering every element to its place."""
    pos = merge_positions(runs, run_counts)
    leaves = np.zeros(len(runs), dtype=np.uint16)
    leaves[pos] = runs
    return leaves, merged_offsets(run_counts)


def merge_by_sort(case):
    """(leaves, offsets) by np.sort of each partition's concatenated runs."""
    n_parts = len(case[0]) if case else 0
    per = [np.sort(np.concatenate([np.asarray(run[p], dtype=np.uint16) for run in case]).astype(np.uint16),
                   kind="stable") for p in range(n_parts)]
    leaves = np.concatenate(per) if per else np.zeros(0, np.uint16)
    return leaves.astype(np.uint16), np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.int64)


# ------------------------------------------------------------------ cases --
def _codes(rng, n):
    return np.sort(rng.integers(0, 65536, n).astype(np.uint16))


def uneven_case(n_runs, seed=0, n_partitions=70):
    """About 70 partitions of uneven sizes: every seventh is empty in every
    run, every fifth is empty in all runs but one, the others hold 0 .. 40
    codes a run (a narrow code range in some, so that runs tie)."""
    rng = np.random.default_rng(1000 + seed)
    case = [[None] * n_partitions for _ in range(n_runs)]
    for p in range(n_partitions):
        only = int(rng.integers(0, n_runs))
        for s in range(n_runs):
            if p % 7 == 3:
                n = 0
            elif p % 5 == 1:
                n = int(rng.integers(1, 30)) if s == only else 0
            else:
                n = int(rng.integers(0, 41))
            seg = _codes(rng, n)
            if p % 4 == 0:
                seg = np.sort((seg % 5).astype(np.uint16))
            case[s][p] = seg
    return case


def single_partition_case(n_runs, seed=0):
    rng = np.random.default_rng(2000 + seed)
    return [[_codes(rng, int(rng.integers(0, 90)))] for _ in range(n_runs)]


def ties_case():
    """Three runs: partition 0 holds one code 17 times in each run, partition
    1 the two ends of the code range."""
    same = np.full(17, 12345, dtype=np.uint16)
    ends = [np.array([0, 0, 65535], np.uint16), np.array([0, 65535, 65535], np.uint16),
            np.array([65535], np.uint16)]
    return [[same.copy(), ends[s]] for s in range(3)]


def long_run_case():
    """A run of 5,000 codes (it spans several workgroups) against one code,
    between two small partitions."""
    rng = np.random.default_rng(3000)
    return [[_codes(rng, 3), _codes(rng, 5000), _codes(rng, 2)],
            [_codes(rng, 4), np.array([31000], np.uint16), _codes(rng, 0)]]


def empty_case(n_runs, n_partitions=5):
    """n_leaves = 0."""
    return [[np.zeros(0, np.uint16) for _ in range(n_partitions)] for _ in range(n_runs)]


def empty_run_case():
    """Three runs of which the middle one is empty for every partition."""
    case = uneven_case(3, seed=7, n_partitions=9)
    case[1] = [np.zeros(0, np.uint16) for _ in case[1]]
    return case


def all_cases():
    """(name, case) of every shape the merge's tests walk."""
    out = []
    for n_runs in (1, 2, 3, 8):
        out.append((f"one_partition-r{n_runs}", single_partition_case(n_runs, n_runs)))
        out.append((f"uneven70-r{n_runs}", uneven_case(n_runs, n_runs)))
    out.append(("ties", ties_case()))
    out.append(("long_run", long_run_case()))
    out.append(("no_leaves-r1", empty_case(1)))
    out.append(("no_leaves-r3", empty_case(3)))
    out.append(("empty_run", empty_run_case()))
    return out
