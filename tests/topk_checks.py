"""Shared checks for top-K lists (test helpers).

Integer-valued tables (int_table) make every bf16 / fp32 product and every
fp32 partial sum exact, so a scan's lists and scores must be IDENTICAL
(tolerance 0) to exact_topk: the float64 scores in (score desc, item id asc)
order, item -1 and score -inf in the slots without a ranked item. It is pinned
to the CPU oracle by tests/test_topk_checks_host.py.

On float tables a score depends on the summation order, so two correct
implementations (the reference's torch.sum, numpy's pairwise sum, the fp32 MFMA
fmaf chain, the bf16 MFMA) may order near-ties differently. The bar: a
list must equal the reference's wherever the reference's neighbouring exact
scores are separated by more than the score tolerance, and where it differs
it must still be a valid top-k of the exact scores within that tolerance.
"""
import numpy as np
import torch


def int_table(rng, n, d, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, size=(n, d)).astype(np.float32)


def _f64(x, device):
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device).double()


def exact_topk(U, I, k, *, thr=None, drop=None, frozen=None, device=None, block=256):
    """Exact float64 top-k, (score desc, item id asc): a stable descending sort
    over ascending ids of U @ nan_to_num(I).T. Never ranked: pairs of ``drop``
    (bool [users, items] or [items]), row r's ids ``frozen[r]``, and, with
    ``thr`` (float [users]), scores not strictly above thr[r]. Slots without a
    ranked item (also those past the catalog's size) hold item -1, score -inf.
    U, I: numpy arrays or torch tensors; device None: CUDA when available.
    Returns numpy (items int64 [n, k], scores float64 [n, k])."""
    device = device or ("cuda" if torch.cuda.is_available() else "cpu")
    Ud, Id = _f64(U, device), torch.nan_to_num(_f64(I, device))
    nu, ni = Ud.shape[0], Id.shape[0]
    m = min(k, ni)
    outi = np.full((nu, k), -1, dtype=np.int64)
    outs = np.full((nu, k), -np.inf, dtype=np.float64)
    dropd = None if drop is None else torch.from_numpy(np.asarray(drop, dtype=bool)).to(device)
    thrd = None if thr is None else _f64(thr, device)
    if frozen is not None:
        fptr = np.concatenate([[0], np.cumsum([len(f) for f in frozen])]).astype(np.int64)
        fcols = np.concatenate([np.asarray(f, dtype=np.int64) for f in frozen]
                               + [np.zeros(0, np.int64)])
    for b in range(0, nu, block):
        e = min(b + block, nu)
        sc = Ud[b:e] @ Id.T
        if dropd is not None:
            sc = sc.masked_fill(dropd if dropd.dim() == 1 else dropd[b:e], -np.inf)
        if frozen is not None and fptr[e] > fptr[b]:
            rows = np.repeat(np.arange(e - b), np.diff(fptr[b:e + 1]))
            cols = fcols[fptr[b]:fptr[e]]  # one scatter per block
            sc[torch.from_numpy(rows).to(device), torch.from_numpy(cols).to(device)] = -np.inf
        if thrd is not None:
            sc = sc.masked_fill(~(sc > thrd[b:e, None]), -np.inf)
        v, i = torch.sort(sc, dim=1, descending=True, stable=True)
        v, i = v[:, :m], i[:, :m]
        i = torch.where(torch.isneginf(v), torch.full_like(i, -1), i)
        outi[b:e, :m] = i.cpu().numpy()
        outs[b:e, :m] = v.cpu().numpy()
    return outi, outs


def assert_same_topk(scores, items, ref):
    """A scan's (scores, items) tensors equal ref = exact_topk(...), tolerance 0."""
    assert np.array_equal(items.cpu().numpy().astype(np.int64), ref[0])
    assert np.array_equal(scores.cpu().numpy().astype(np.float64), ref[1])


# fp32 dot product of width d: |computed - exact| <= c * eps32 * sum_j |u_j i_j|
# with c ~ d in the worst case; measured fmaf chains stay below ~1.5e-7 *
# sum|u_j i_j| (cdna_hip_programming.md, FP32-input MFMA) and torch's / numpy's
# blocked sums below that. 4e-7 covers both sides of a comparison.
FP32_REL = 4e-7


def fp32_row_tol(U, I, rel=FP32_REL):
    """Per-user score tolerance: rel * max_i sum_j |U[u,j] I[i,j]|."""
    A = np.abs(U.astype(np.float64)) @ np.abs(I.astype(np.float64)).T
    return rel * A.max(axis=1)


def gap_check(got, ref, U, I, frozen_csr, tol):
    """Number of users whose list differs from ``ref``; asserts each such list
    is a valid top-k of the exact (float64) scores within ``tol`` (a scalar or
    one value per user)."""
    S = U.astype(np.float64) @ I.astype(np.float64).T
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), (ref.shape[0],))
    bad = 0
    for u in range(ref.shape[0]):
        if np.array_equal(got[u], ref[u]):
            continue
        s = S[u].copy()
        if frozen_csr is not None:
            rowptr, cols = frozen_csr
            s[cols[rowptr[u]:rowptr[u + 1]]] = -np.inf
        t = tol[u]
        gs = s[got[u]]
        assert len(set(got[u].tolist())) == len(got[u]), u  # no duplicates
        assert np.all(np.isfinite(gs)), u                    # no excluded item
        assert np.all(np.diff(gs) <= 2 * t), u               # sorted within tol
        kth = np.sort(s)[::-1][len(ref[u]) - 1]
        assert np.all(gs >= kth - 2 * t), u
        must = np.nonzero(s > kth + 2 * t)[0]
        assert set(must.tolist()) <= set(got[u].tolist()), u
        bad += 1
    return bad
