"""Drivers and comparisons for the release path (pdp_select.hip): selection,
compaction and the noisy metrics, called through the C ABI with buffers the
test owns, so that every byte a kernel must leave alone can be checked.

Every output buffer is pre-filled with a sentinel no kernel can produce here
(KEEP_FILL, INDEX_FILL, FILL).  The comparisons are equalities (NaN matches
NaN) with one exception, VARIANCE's column 0; see compare_metrics().
"""
import ctypes

import numpy as np

from oracle import columnar as O

KEEP_FILL = 0xAB       # keep[] is written 0 / 1 only
INDEX_FILL = -7        # index[] holds partition indices >= 0
FILL = -12345.678      # off every noise grid used by the tests
BIG_OFFSET = (1 << 33) + 5  # a global partition index with a nonzero high counter word


def _ptr(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def select(device, rc, sel, *, seed, partition_offset=0, public_mask=None, want_noised=True):
    """pdp_select_partitions on a row-count column.  sel: executor.SelectionSpec.
    Returns (keep uint8[P] device tensor, noised float64[P] device tensor or None)."""
    import torch
    from pipelinedp_amd import _native as N
    from pipelinedp_amd import dp_computations as dpc
    P = len(rc)
    trc = torch.as_tensor(np.asarray(rc, dtype=np.int64)).to(device)
    keep = torch.full((P,), KEEP_FILL, dtype=torch.uint8, device=device)
    noised = torch.full((P,), FILL, dtype=torch.float64, device=device) if want_noised else None
    sc = N.SelectConfig()
    sc.n_partitions, sc.partition_offset = P, int(partition_offset)
    sc.strategy = int(sel.strategy)
    sc.max_rows_per_privacy_id, sc.pre_threshold = int(sel.max_rows_per_privacy_id), int(sel.pre_threshold)
    hold = []
    if sel.keep_prob is not None:
        table = torch.as_tensor(np.ascontiguousarray(sel.keep_prob, dtype=np.float64)).to(device)
        hold.append(table)
        sc.keep_table_len, sc.keep_prob = int(table.numel()), table.data_ptr()
    sc.noise = (sel.noise or dpc.NO_NOISE).to_c()
    sc.threshold = float(sel.threshold)
    if public_mask is not None:
        mask = torch.as_tensor(np.asarray(public_mask, dtype=np.uint8)).to(device)
        hold.append(mask)
        sc.public_mask = mask.data_ptr()
    sc.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    N.check(N.lib().pdp_select_partitions(ctypes.byref(sc), _ptr(trc), _ptr(keep), _ptr(noised), None),
            "pdp_select_partitions")
    torch.cuda.synchronize()
    return keep, noised


def oracle_select(rc, sel, *, seed, partition_offset=0, public_mask=None):
    return O.select(rc, sel.strategy, max_rows_per_privacy_id=sel.max_rows_per_privacy_id,
                    pre_threshold=sel.pre_threshold, keep_prob=sel.keep_prob,
                    noise=None if sel.noise is None else sel.noise.as_dict(), threshold=sel.threshold,
                    public_mask=public_mask, seed=seed, partition_offset=partition_offset)


def compact(device, keep):
    """pdp_compact of a uint8 device tensor (or host array).  Returns
    (index int64[max(n, 1)] host array, pre-filled with INDEX_FILL; device count)."""
    import torch
    from pipelinedp_amd import _native as N
    if not isinstance(keep, torch.Tensor):
        keep = torch.as_tensor(np.asarray(keep, dtype=np.uint8)).to(device)
    n = int(keep.numel())
    lib = N.lib()
    need = ctypes.c_uint64(0)
    N.check(lib.pdp_compact_workspace_bytes(n, ctypes.byref(need)), "pdp_compact_workspace_bytes")
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=device)
    index = torch.full((max(n, 1),), INDEX_FILL, dtype=torch.int64, device=device)
    count = torch.full((1,), -1, dtype=torch.int64, device=device)
    N.check(lib.pdp_compact(_ptr(keep), n, _ptr(index), _ptr(count), _ptr(ws), ws.numel(), None), "pdp_compact")
    torch.cuda.synchronize()
    return index.cpu().numpy(), int(count.item())


def check_compaction(index, count, mask, what=""):
    """index[:count] == flatnonzero(mask), the device count is equal, and the
    rest of the index buffer is untouched."""
    want = np.flatnonzero(np.asarray(mask) != 0)
    assert count == len(want), (what, count, len(want))
    np.testing.assert_array_equal(index[:count], want, err_msg=str(what))
    assert (index[count:] == INDEX_FILL).all(), what


def noise_metrics(device, ops, index, n_kept, n_kept_dev, acc_np, *, seed, partition_offset=0, noised=None,
                  n_cols=None, stride=None):
    """pdp_noise_metrics into a FILL-ed out[n_cols, stride].  ops: MetricOpSpec
    list; index: int64 host array; n_kept_dev: None or the device-side count;
    noised: device tensor / host array / None.  Returns out as a host array."""
    import torch
    from pipelinedp_amd import _native as N
    from pipelinedp_amd import executor as X
    if n_cols is None:
        n_cols = 1 + max([c for o in ops for c in o.out_col] + [0])
    stride = max(len(index), 1) if stride is None else stride
    acc = {k: (None if v is None else torch.as_tensor(v).to(device)) for k, v in acc_np.items()}
    tindex = torch.as_tensor(np.asarray(index, dtype=np.int64)).to(device)
    tcount = None if n_kept_dev is None else torch.as_tensor([int(n_kept_dev)], dtype=torch.int64).to(device)
    if noised is not None and not isinstance(noised, torch.Tensor):
        noised = torch.as_tensor(np.asarray(noised, dtype=np.float64)).to(device)
    out = torch.full((n_cols, stride), FILL, dtype=torch.float64, device=device)
    c_ops = (N.MetricOp * max(len(ops), 1))(*[o.to_c() for o in ops])
    sum_is_int = 1 if (acc.get("sum") is not None and acc["sum"].dtype == torch.int64) else 0
    N.check(N.lib().pdp_noise_metrics(c_ops, len(ops), _ptr(tindex), int(n_kept), _ptr(tcount),
                                      int(partition_offset), ctypes.byref(X._acc_struct(acc)), sum_is_int,
                                      _ptr(noised), _ptr(out), stride, int(seed) & 0xFFFFFFFFFFFFFFFF, None),
            "pdp_noise_metrics")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def oracle_metrics(ops, index, acc_np, noised, *, seed, partition_offset=0, n_cols=None):
    """(want[n_cols, len(index)], {op position: (dp_mean, dp_mean_sq)})."""
    terms = {}
    sum_is_int = acc_np.get("sum") is not None and acc_np["sum"].dtype == np.int64
    want = O.noise_metrics([o.as_dict() for o in ops], index, acc_np, sum_is_int, noised, seed,
                           partition_offset=partition_offset, n_cols=n_cols, variance_terms=terms)
    return want, terms


def compare_metrics(got, want, ops, terms, what="", check_fill=True):
    """got, want: [n_cols, n].  Every column that an op writes equals the
    oracle's (the draws are grid values and every later operation is one
    correctly rounded fp64 operation on both sides), except VARIANCE's column
    0 = dp_mean_sq - dp_mean * dp_mean: the device compiler may contract it
    into one fma.  With u = 2^-53, the two-operation form errs by at most
    u dp_mean^2 + u |result| and the fma by u |result|, and |result| <=
    |dp_mean_sq| + dp_mean^2, so the two differ by at most
    3u dp_mean^2 + 2u |dp_mean_sq| <= 2^-51 (dp_mean^2 + |dp_mean_sq|).
    Columns no op writes must still hold FILL (check_fill: `got` was pre-filled)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    written = set()
    for o, op in enumerate(ops):
        cols = list(op.out_col)
        for j, c in enumerate(cols):
            if c < 0:
                continue
            written.add(c)
            if op.kind == O.OP_VARIANCE and j == 0:
                dp_mean, dp_mean_sq = terms[o]
                bound = 2.0 ** -51 * (dp_mean * dp_mean + np.abs(dp_mean_sq))
                err = np.abs(got[c] - want[c])
                bad = np.flatnonzero(~(err <= bound))
                assert len(bad) == 0, (what, "variance op", o, "col", c, bad[:5], got[c][bad[:5]], want[c][bad[:5]])
            else:
                np.testing.assert_array_equal(got[c], want[c], err_msg=f"{what}: op {o} out_col[{j}] = {c}")
    for c in range(got.shape[0] if check_fill else 0):
        if c not in written:
            assert (got[c] == FILL).all(), (what, "column", c, "was never asked for")


def public_select(device, mask):
    """executor.select_and_noise with the PUBLIC strategy and no ops: k_select
    copies the mask (as 0 / 1) and pdp_compact compacts it.  Returns (index, n_kept)."""
    import torch
    from pipelinedp_amd import executor as X
    P = len(mask)
    acc = dict.fromkeys(("count", "sum", "normalized_sum", "normalized_sum_sq"))
    acc["privacy_id_count"] = torch.zeros(P, dtype=torch.int64, device=device)
    sel = X.SelectionSpec(strategy=O.SELECT_PUBLIC)
    index, _, n_kept = X.select_and_noise(acc, selection=sel, ops=[], n_cols=0, seed_select=1, seed_noise=2,
                                          public_mask=torch.as_tensor(np.asarray(mask, dtype=np.uint8)).to(device))
    return index.cpu().numpy(), n_kept


def add_noise(device, values, noise, *, seed, index_offset):
    """executor.add_noise of a host column; returns the host result."""
    import torch
    from pipelinedp_amd import executor as X
    out = X.add_noise(torch.as_tensor(values).to(device), noise=noise, seed=seed, index_offset=index_offset)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def vector_sum_metrics(device, vacc, index, *, norm_kind, max_norm, noise, seed, partition_offset):
    import torch
    from pipelinedp_amd import executor as X
    out = X.vector_sum_metrics(torch.as_tensor(vacc).to(device), torch.as_tensor(index).to(device),
                               norm_kind=norm_kind, max_norm=max_norm, noise=noise, seed=seed,
                               partition_offset=partition_offset)
    torch.cuda.synchronize()
    return out.cpu().numpy()
