"""The histogram oracle (oracle/histograms.py) on the edge tables of
tests/hist_edges_util.py, against a plain restatement of the reference that
shares no code with it: Python's bisect over list(np.linspace(...)), dict
group-bys, int / Fraction sums, and the logarithmic bin read off the decimal
digits of the value.  Every comparison is an equality.  The reference's own
bins on three of the float ranges and on the small distinct-count tables are
the fixtures float_edges / pre_float_edges / log_edges
(oracle/gen_golden_hist.py), which tests/test_histograms_host.py runs the
oracle against; here the restatement is held to them too."""
import bisect
from fractions import Fraction

import numpy as np
import pytest

from oracle import histograms as OH
from tests import hist_edges_util as E
from tests import hist_util as HU


# ------------------------------------------------------ plain restatement --
def plain_log_bin(v):
    """three leading decimal digits kept: [d1 d2 d3] * 10^k .. + 10^k"""
    s = str(int(v))
    if len(s) <= 3:
        return int(v), int(v) + 1
    w = 10 ** (len(s) - 3)
    return int(s[:3]) * w, int(s[:3]) * w + w


def plain_int_hist(values):
    bins = {}
    for v in values:
        lo, up = plain_log_bin(v)
        c, s, m = bins.get((lo, up), (0, 0, 0))
        bins[(lo, up)] = (c + 1, s + v, max(m, v))
    return [(lo, up) + bins[(lo, up)] for lo, up in sorted(bins)]


def _exact_sum(vals):
    """a single term as it is; several terms (all k/8: check_exact) in integers"""
    if len(vals) == 1:
        return vals[0]
    return float(sum(Fraction(v) for v in vals))


def plain_float_hist(values):
    mn, mx = min(values), max(values)
    lowers = [mn, mn] if mn == mx else list(np.linspace(mn, mx, 10001))
    bins = {}
    for v in values:
        i = len(lowers) - 2 if v == lowers[-1] else bisect.bisect_right(lowers, v) - 1
        bins.setdefault(i, []).append(v)
    return [(float(lowers[i]), float(lowers[i + 1]), len(vs), float(sum(Fraction(v) for v in vs)), max(vs))
            for i, vs in sorted(bins.items())]


def plain_histograms(pid, pk, val):
    pairs, parts, pid_rows = {}, {}, {}
    for u, k, v in zip(pid.tolist(), pk.tolist(), val.tolist()):
        pairs.setdefault((u, k), []).append(v)
        parts.setdefault(k, []).append(v)
        pid_rows[u] = pid_rows.get(u, 0) + 1
    l0, pk_pids = {}, {}
    for u, k in pairs:
        l0[u] = l0.get(u, 0) + 1
        pk_pids[k] = pk_pids.get(k, 0) + 1
    return {
        "l0_contributions_histogram": plain_int_hist(l0.values()),
        "l1_contributions_histogram": plain_int_hist(pid_rows.values()),
        "linf_contributions_histogram": plain_int_hist([len(v) for v in pairs.values()]),
        "linf_sum_contributions_histogram": plain_float_hist([_exact_sum(v) for v in pairs.values()]),
        "count_per_partition_histogram": plain_int_hist([len(v) for v in parts.values()]),
        "count_privacy_id_per_partition": plain_int_hist(pk_pids.values()),
        "sum_per_partition_histogram": plain_float_hist([_exact_sum(v) for v in parts.values()]),
    }


def _assert_same(got, want, what):
    assert set(got) == set(want) == set(OH.HIST_FIELDS)
    for f in OH.HIST_FIELDS:
        g, w = [tuple(b) for b in got[f]], [tuple(b) for b in want[f]]
        assert g == w, f"{what}/{f}: first difference {next((x for x in zip(g, w) if x[0] != x[1]), (len(g), len(w)))}"


TABLES = {f"float/{name}.{j}": (lambda name=name, j=j: E.float_edges(name)[j])
          for name in E.FLOAT_RANGES for j in range(len(E.float_edge_parts(name)))}
TABLES.update({
    "float/constant": E.float_constant,
    "float/signed_zeros": E.float_signed_zeros,
    "float/two_pairs": E.float_edges_two_pairs,
    "log/counts": E.log_counts,
    "log/distinct_small": lambda: E.log_distinct(E.LOG_DISTINCT_SMALL),
    "log/distinct_3628": lambda: E.log_distinct((3628,)),
    "log/distinct_3629": lambda: E.log_distinct((3629,)),
    "log/wave_partition": lambda: E.log_wave_bins("partition"),
    "log/wave_privacy_id": lambda: E.log_wave_bins("privacy_id"),
})
TABLES.update({f"structure/n{n}": (lambda n=n: E.structure(n)) for n in E.STRUCTURE_N if n <= 65537})
TABLES.update({f"structure/P{P}": (lambda P=P: E.structure(E.STRUCTURE_P_ROWS, P)) for P in E.STRUCTURE_P})


@pytest.mark.parametrize("name", sorted(TABLES))
def test_oracle_equals_plain_restatement(name):
    """building the table runs its self-checks (exactness, the edge is hit)"""
    pid, pk, val, U, P = TABLES[name]()
    assert 0 <= pid.min() and pid.max() < U and 0 <= pk.min() and pk.max() < P
    want = plain_histograms(pid, pk, val)
    _assert_same(OH.dataset_histograms(pid, pk, val), want, name)
    pre = HU.preaggregate(pid, pk, val)
    if E.weight_sums_clear_of_half(pre):
        _assert_same(OH.preaggregated_histograms(*pre), want, f"pre/{name}")
    else:
        assert name.startswith("structure/")  # random tables; every table built for its L0 / L1 is clear


@pytest.mark.parametrize("n", [n for n in E.STRUCTURE_N if n > 65537])
def test_large_structure_tables_build(n):
    """the self-checks of the sizes the CPU restatement is too slow for"""
    pid, pk, val, U, P = E.structure(n)
    assert len(pid) == n and pid.max() == U - 1 and pk.max() == P - 1


def test_builders_are_deterministic():
    for name in ("float/third.0", "log/distinct_small", "structure/n1537"):
        a, b = TABLES[name](), TABLES[name]()
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]


def test_check_exact_refuses_order_dependent_sums():
    one = np.zeros(2, np.int64)
    two = np.array([0, 1])
    E.check_exact(two, two, [0.1, 0.3])       # single terms: anything finite
    E.check_exact(one, one, [0.125, -3.5])    # several terms: k/8
    with pytest.raises(ValueError):
        E.check_exact(one, one, [0.1, 0.3])   # one pair, two values that are no k/8
    with pytest.raises(ValueError):
        E.check_exact(two, one, [0.1, 0.3])   # two pairs of one partition
    with pytest.raises(ValueError):
        E.check_exact(one, one, [2.0 ** 52, 2.0 ** 52])  # |k| adds up to 2^56
    with pytest.raises(ValueError):
        E.check_exact(two, two, [1.0, np.inf])


def test_weight_sum_check():
    assert not E.weight_sums_clear_of_half((None, None, None, [2, 2, 2, 1], [5, 5, 5, 7]))  # 3 x 1/2
    assert E.weight_sums_clear_of_half((None, None, None, [3, 3, 3, 1], [5, 5, 5, 7]))
    for d in E.LOG_DISTINCT:
        pid, pk, val, _, _ = E.log_distinct((d,))
        assert E.weight_sums_clear_of_half(HU.preaggregate(pid, pk, val)), d


def test_log_bins_at_the_decades():
    """known bins of _to_bin_lower_upper_logarithmic (computing_histograms.py:28-47;
    1234 -> [1230, 1240) is the reference test's), from the oracle, the
    digits and the host's index -> bounds table"""
    from pipelinedp_amd.dataset_histograms import computing_histograms as CH
    known = {1: (1, 2), 999: (999, 1000), 1000: (1000, 1010), 1001: (1000, 1010), 1009: (1000, 1010),
             1010: (1010, 1020), 1234: (1230, 1240), 9989: (9980, 9990), 9990: (9990, 10000), 9999: (9990, 10000),
             10000: (10000, 10100), 10001: (10000, 10100), 10099: (10000, 10100), 10100: (10100, 10200),
             99999: (99900, 100000), 100000: (100000, 101000), 100999: (100000, 101000), 101000: (101000, 102000)}
    bounds = {CH.log_bin_bounds(i) for i in range(1000 + 900 * 4)}
    for v, b in known.items():
        assert OH.log_bin(v) == b and plain_log_bin(v) == b and b in bounds, v
    for v in E.LOG_COUNTS + E.LOG_DISTINCT:
        assert OH.log_bin(v) == plain_log_bin(v) and plain_log_bin(v) in bounds, v


def test_wave_tables_fill_two_bins():
    for key, fields in (("partition", ("count_per_partition_histogram", "count_privacy_id_per_partition")),
                        ("privacy_id", ("l1_contributions_histogram", "l0_contributions_histogram"))):
        pid, pk, val, _, _ = E.log_wave_bins(key)
        got = OH.dataset_histograms(pid, pk, val)
        for f in fields:
            assert [tuple(b) for b in got[f]] == E.WAVE_BINS, (key, f)


def _table_of(fixture_name):
    """"float_edges/<range>.<part>" or "log_edges" -> the helper's table"""
    if fixture_name == "log_edges":
        return E.log_distinct(E.LOG_DISTINCT_SMALL)
    rng, part = fixture_name.split("/")[1].rsplit(".", 1)
    return E.float_edges(rng)[int(part)]


def test_fixture_covers_its_three_ranges():
    got = sorted(f["name"] for f in HU.fixtures() if f["name"].startswith("float_edges/"))
    want = sorted(f"float_edges/{r}.{j}" for r in E.FIXTURE_RANGES for j in range(len(E.float_edge_parts(r))))
    assert got == want == sorted(f["name"] for f in HU.pre_fixtures() if f["name"].startswith("float_edges/"))


@pytest.mark.parametrize("fx", [f for f in HU.fixtures() if f["name"].split("/")[0] in ("float_edges", "log_edges")],
                         ids=lambda f: f["name"])
def test_reference_fixture_equals_table_and_restatement(fx):
    """the committed fixture holds exactly the helper's table (the recipe
    builds it from the same builder), and the reference's recorded bins equal
    the plain restatement's, bit for bit"""
    pid, pk, val, _, _ = _table_of(fx["name"])
    assert [list(r) for r in zip(pid.tolist(), pk.tolist(), val.tolist())] == fx["rows"]
    _assert_same({f: e["bins"] for f, e in fx["expected"].items()}, plain_histograms(pid, pk, val), fx["name"])


@pytest.mark.parametrize("fx", [f for f in HU.pre_fixtures() if f["name"].startswith("float_edges/")],
                         ids=lambda f: f["name"])
def test_reference_preaggregated_fixture_equals_restatement(fx):
    pid, pk, val, _, _ = _table_of(fx["name"])
    _assert_same({f: e["bins"] for f, e in fx["expected"].items()}, plain_histograms(pid, pk, val), fx["name"])
    assert sorted(r[2] for r in fx["rows"]) == sorted(val.tolist())


def test_fixture_sizes():
    import glob
    import os
    sizes = {os.path.basename(p): os.path.getsize(p) for p in glob.glob(os.path.join(HU.GOLDEN, "*.json"))}
    new = [n for n in sizes if "_edges" in n]
    assert len(new) == 3 and all(sizes[n] <= sizes["dataset_histograms_heavy.json"] for n in new), sizes
