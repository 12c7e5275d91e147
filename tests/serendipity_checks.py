"""Float64 restatements of dr_history_distance, dr_serendipity_rerank and
dr_list_item_mean on the bf16-quantised table, an fp32 emulation of the
kernels' arithmetic, and the checkers the host and GPU tests share
(include/divrec_hip.h holds the contract). numpy only.

Bound of check_distance: |out - ref| <= (d + 16) * 2^-23 per element, the
worst-case fp32 accumulation error of d exact bf16 products, bounded through
Cauchy-Schwarz and doubled for the two norm terms (1.7e-5 at d = 128)."""
import numpy as np

MIN, MEAN = "min", "mean"


def bf16_round(a):
    """fp32 values rounded to bf16 (round to nearest even), as float32."""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def distance_bound(d):
    return (d + 16) * 2.0 ** -23


def fma32(a, b, c):
    """fp32 fused multiply-add a * b + c, correctly rounded: the product of two
    fp32 values is exact in float64; the sum is rounded to odd in float64
    (TwoSum tells whether it was exact), which a final rounding to fp32
    (53 >= 24 + 2 bits) turns into the single rounding of an fma."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float32).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    nudge = (err != 0) & even & np.isfinite(s)
    s = np.where(nudge, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _rows(rowptr, hist, u, n_items):
    h = np.asarray(hist[rowptr[u]:rowptr[u + 1]], dtype=np.int64)
    return h, h[(h >= 0) & (h < n_items)]


def reference_distance(lists, table, rowptr, hist, reduce):
    """float64 [n, C] on the (already bf16-valued) table."""
    E = np.asarray(table, dtype=np.float64)
    n_items = E.shape[0]
    nrm = np.sqrt((E * E).sum(1))
    inv = np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)
    U = E * inv[:, None]
    lists = np.asarray(lists, dtype=np.int64)
    out = np.zeros(lists.shape, dtype=np.float64)
    for u in range(lists.shape[0]):
        _, hv = _rows(rowptr, hist, u, n_items)
        ids = lists[u]
        live = (ids >= 0) & (ids < n_items)
        if hv.size and live.any():
            dist = 1.0 - U[ids[live]] @ U[hv].T
            out[u, live] = dist.min(1) if reduce == MIN else dist.mean(1)
        out[u, ids >= n_items] = np.nan
    return out


def emulate_distance(lists, table, rowptr, hist, reduce, variant=None):
    """The kernel's arithmetic in fp32 [n, C]. Gram elements and squared norms
    are formed in float64 and rounded once (exact for integer-valued tables,
    where the result is bit for bit the kernel's for MIN); 1/|e| is one fp32
    sqrt and one divide, the distance one fma. MEAN sums in float64 (the kernel:
    fp32 within a tile, double across). ``variant`` names a broken form the
    checkers must reject: "max", "raw_len", "empty_nan", "zero_norm_0"."""
    E = np.asarray(table, dtype=np.float64)
    n_items = E.shape[0]
    nsq = (E * E).sum(1).astype(np.float32)
    with np.errstate(divide="ignore"):
        w = np.where(nsq > 0, np.float32(1) / np.sqrt(nsq), np.float32(0)).astype(np.float32)
    lists = np.asarray(lists, dtype=np.int64)
    out = np.zeros(lists.shape, dtype=np.float32)
    for u in range(lists.shape[0]):
        raw, hv = _rows(rowptr, hist, u, n_items)
        ids = lists[u]
        live = (ids >= 0) & (ids < n_items)
        if hv.size and live.any():
            c = ids[live]
            g = (E[c] @ E[hv].T).astype(np.float32)
            dist = fma32(-g, w[hv][None, :] * w[c][:, None], np.float32(1))
            if variant == "zero_norm_0":
                dist = np.where((w[c][:, None] == 0) | (w[hv][None, :] == 0), np.float32(0), dist)
            if reduce == MIN:
                out[u, live] = dist.max(1) if variant == "max" else dist.min(1)
            else:
                den = raw.size if variant == "raw_len" else hv.size
                out[u, live] = (dist.astype(np.float64).sum(1) / den).astype(np.float32)
        elif variant == "empty_nan":
            out[u, live] = np.nan
        out[u, ids >= n_items] = np.nan
    return out


def check_distance(out, lists, table, rowptr, hist, reduce):
    """out fp32 [n, C] against the float64 restatement: NaN exactly where the
    list id is past the table, 0 for ids < 0 and for users without valid
    history, within distance_bound(d) elsewhere."""
    out = np.asarray(out)
    ref = reference_distance(lists, table, rowptr, hist, reduce)
    assert out.shape == ref.shape and out.dtype == np.float32
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(out), nan), "NaN exactly for list ids past the table"
    lists = np.asarray(lists)
    assert not out[lists < 0].any(), "empty slots get 0"
    n_items = np.asarray(table).shape[0]
    for u in range(lists.shape[0]):
        if _rows(rowptr, hist, u, n_items)[1].size == 0:
            assert not out[u][~nan[u]].any(), f"user {u} has no valid history: zeros"
    diff = np.abs(out.astype(np.float64) - ref)[~nan]
    bound = distance_bound(np.asarray(table).shape[1])
    worst = float(diff.max()) if diff.size else 0.0
    assert worst <= bound, f"max |out - ref| = {worst:.3e} above {bound:.3e}"
    return worst


def blend32(lam, scores, dist, fused=False):
    """fp32 lam * max(score, -FLT_MAX) + (1 - lam) * dist: two multiplies, one add."""
    lam = np.float32(lam)
    mu = np.float32(1) - lam
    s = np.asarray(scores, np.float32).copy()
    s[~(s >= -np.finfo(np.float32).max)] = -np.finfo(np.float32).max  # -inf, NaN
    d = np.asarray(dist, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if fused:
            return fma32(lam, s, mu * d)
        return (lam * s + mu * d).astype(np.float32)


def expected_rerank(cand_items, cand_scores, dist, n_items, lam, k_out, variant=None):
    """(items int32 [n, k_out], dist fp32 [n, k_out]) from the candidates' own
    distances: stable descending order of the fp32 value over the live
    candidates. Variants the checker must reject: "ties_high", "fma"."""
    cand_items = np.asarray(cand_items)
    n = cand_items.shape[0]
    items = np.full((n, k_out), -1, dtype=np.int32)
    od = np.zeros((n, k_out), dtype=np.float32)
    for u in range(n):
        ids = cand_items[u]
        live = np.flatnonzero((ids >= 0) & (ids < n_items))
        v = blend32(lam, cand_scores[u][live], dist[u][live], fused=variant == "fma")
        if variant == "ties_high":
            order = live[::-1][np.argsort(-v[::-1].astype(np.float64), kind="stable")]
        else:
            order = live[np.argsort(-v.astype(np.float64), kind="stable")]
        order = order[:k_out]
        items[u, :order.size] = ids[order]
        od[u, :order.size] = dist[u][order]
    return items, od


def check_rerank(out_items, out_dist, cand_items, cand_scores, dist, n_items, lam, k_out):
    """The picks equal exactly the stable descending order of the fp32 blend
    formed from ``dist`` (the kernel's own dr_history_distance of the
    candidates), and out_dist is bitwise the picks' entries of ``dist``."""
    want_items, want_dist = expected_rerank(cand_items, cand_scores, dist, n_items, lam, k_out)
    out_items = np.asarray(out_items)
    assert out_items.shape == want_items.shape
    bad = np.flatnonzero((out_items != want_items).any(1))
    assert bad.size == 0, f"picks differ for users {bad[:8].tolist()}"
    if out_dist is not None:
        assert np.array_equal(np.asarray(out_dist, np.float32).view(np.uint32),
                              want_dist.view(np.uint32)), "out_dist is not the picks' distances"


def reference_list_item_mean(recs, values):
    recs = np.asarray(recs, dtype=np.int64)
    values = np.asarray(values, dtype=np.float64)
    out = np.zeros(recs.shape[0], dtype=np.float64)
    for u in range(recs.shape[0]):
        ids = recs[u][(recs[u] >= 0) & (recs[u] < values.size)]
        out[u] = values[ids].mean() if ids.size else 0.0
    return out


# --------------------------------------------------------------------------- inputs
HIST_LENGTHS = (0, 1, 31, 32, 33, 100, 1000)
LONG_HISTORY = 5000
ZERO_ROWS = (0, 1)  # table rows that are all zero


def make_case(seed, C, d, n_users=70, n_items=700, integer=True):
    """(lists int32 [n, C], scores fp32 [n, C], table fp32 [n_items, d] of bf16
    values, rowptr int64, hist int32). History lengths cycle through
    HIST_LENGTHS, user 3 has LONG_HISTORY entries. Planted: rows ZERO_ROWS are
    zero and appear in lists and histories; position 0 of every list with a
    history is an item of that history; histories repeat items (drawn with
    replacement); equal scores on duplicate list items (value ties)."""
    rng = np.random.default_rng(seed)
    if integer:
        table = rng.integers(-3, 4, (n_items, d)).astype(np.float32)
    else:
        table = bf16_round(rng.standard_normal((n_items, d)).astype(np.float32))
    table[list(ZERO_ROWS)] = 0
    lens = [HIST_LENGTHS[u % len(HIST_LENGTHS)] for u in range(n_users)]
    if n_users > 3:
        lens[3] = LONG_HISTORY
    rowptr = np.zeros(n_users + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lens)
    hist = rng.integers(2, n_items, int(rowptr[-1])).astype(np.int32)
    lists = rng.integers(2, n_items, (n_users, C)).astype(np.int32)
    scores = rng.standard_normal((n_users, C)).astype(np.float32)
    for u in range(n_users):
        if lens[u]:
            lists[u, 0] = hist[rowptr[u]]  # a candidate the user already knows
            if lens[u] > 2:
                hist[rowptr[u] + 1] = ZERO_ROWS[0]
        if C > 4:
            lists[u, 2] = ZERO_ROWS[1]
            lists[u, C - 1] = lists[u, 1]  # a duplicate item with an equal score
            scores[u, C - 1] = scores[u, 1]
        if C > 8:
            scores[u, 6] = scores[u, 5]  # two items, one score: a tie wherever dist ties or lam = 1
    return lists, scores, table, rowptr, hist
