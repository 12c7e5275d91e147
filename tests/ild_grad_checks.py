"""Helpers of the embedding-ILD gradient tests: the float64 reference of
dr_ild_embedding_backward (include/divrec_hip.h) as torch autograd of the
dense pair formula, ILD_u = (sum_{p<q} D(e_p, e_q)) / (k (k - 1)), with the
masking rules of the header (a zero-norm row's cosine pairs and pairs at
euclidean distance 0 are constants), a numpy restatement of the header's
closed forms (tests/test_ild_backward_host.py pins the one to the other), and
the tolerance of every gradient comparison."""
import functools

import numpy as np
import torch

KINDS = ("cosine", "dot", "euclidean")


def ild_f64(X: torch.Tensor, kind: str) -> torch.Tensor:
    """ILD of the lists whose rows are X [n, k, d] (float64), differentiable
    with respect to X: the dense pair formula."""
    n, k, _ = X.shape
    if kind == "dot":
        D = X @ X.transpose(1, 2)
    elif kind == "cosine":
        sq = X.pow(2).sum(2)
        ok = sq > 0  # a zero row: no direction, its pairs are constants
        norm = torch.where(ok, sq, torch.ones_like(sq)).sqrt()  # no sqrt'(0) in the graph
        unit = X / norm.unsqueeze(2) * ok.unsqueeze(2)
        D = 1.0 - unit @ unit.transpose(1, 2)
    elif kind == "euclidean":
        sq = (X.unsqueeze(2) - X.unsqueeze(1)).pow(2).sum(3)
        ok = sq > 0  # distance exactly 0: no direction, a constant
        D = torch.where(ok, sq, torch.ones_like(sq)).sqrt() * ok
    else:
        raise ValueError(kind)
    upper = torch.triu(torch.ones(k, k, dtype=torch.bool), 1)
    return (D * upper).sum((1, 2)) / (k * (k - 1))


def ild_grad_f64(table, recs, kind, grad_out=None, scale=1.0) -> np.ndarray:
    """d/d table of scale * sum_u grad_out[u] * ILD_u in float64, [n_items, d].
    A list holding an id outside the table adds nothing."""
    E = torch.tensor(np.asarray(table, np.float64)).requires_grad_(True)
    recs = torch.tensor(np.asarray(recs, np.int64))  # a copy: cached cases are read-only
    n, k = recs.shape
    go = torch.ones(n, dtype=torch.float64) if grad_out is None else \
        torch.tensor(np.asarray(grad_out, np.float64))
    keep = ((recs >= 0) & (recs < E.size(0))).all(1)
    recs, go = recs[keep], go[keep]
    if k < 2 or recs.size(0) == 0:
        return np.zeros(tuple(E.shape))
    # lists in chunks: the euclidean differences are [chunk, k, k, d]
    chunk = max(1, (1 << 23) // (k * k * E.size(1)))
    for a in range(0, recs.size(0), chunk):
        r = recs[a:a + chunk]
        (scale * (go[a:a + chunk] * ild_f64(E[r], kind)).sum()).backward()
    return E.grad.numpy()


def closed_form_grad_f64(table, recs, kind, grad_out=None, scale=1.0) -> np.ndarray:
    """The closed forms of include/divrec_hip.h evaluated in float64 (valid ids only)."""
    E = np.asarray(table, np.float64)
    recs = np.asarray(recs, np.int64)
    n, k = recs.shape
    G = np.zeros_like(E)
    for u in range(n):
        w = scale * (1.0 if grad_out is None else float(grad_out[u])) / (k * (k - 1))
        X = E[recs[u]]
        if kind == "dot":
            add = w * (X.sum(0) - X)
        elif kind == "cosine":
            norm = np.sqrt((X * X).sum(1))
            ok = norm > 0
            safe = np.where(ok, norm, 1.0)[:, None]
            unit = X / safe * ok[:, None]
            t = unit.sum(0) - unit
            add = -w * (t - (unit * t).sum(1, keepdims=True) * unit) / safe * ok[:, None]
        else:
            diff = X[:, None, :] - X[None, :, :]
            dist = np.sqrt((diff * diff).sum(2))
            inv = np.where(dist > 0, 1.0 / np.where(dist > 0, dist, 1.0), 0.0)
            add = w * (diff * inv[:, :, None]).sum(1)
        np.add.at(G, recs[u], add)
    return G


def grad_mismatch(got, ref):
    """(count, worst excess) of elements outside |got - ref| <= 1e-4 |ref| + 1e-5 A,
    A = max |ref| over the table: this project's kernel-against-float64 gradient
    bar plus a floor for elements that are sums of cancelling terms."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = 1e-4 * np.abs(ref) + 1e-5 * np.abs(ref).max()
    over = np.abs(got - ref) - bound
    return int((over > 0).sum()), float(over.max())


def assert_grad_close(got, ref):
    assert np.isfinite(np.asarray(got)).all()
    count, worst = grad_mismatch(got, ref)
    assert count == 0, f"{count} elements outside the tolerance, worst by {worst:.3e}"


@functools.lru_cache(maxsize=None)
def case(n_users, n_items, k, d, repeat=False, seed=0):
    """(table fp32 [n_items, d], recs int64 [n_users, k], grad_out fp32) of one
    test shape: normal table, random lists without repeats (position 1
    repeating position 0 with ``repeat``), random grad_out. Cached: shared and
    left unchanged by the tests that use it."""
    rng = np.random.default_rng(1000 * seed + 7 * n_users + 3 * k + d)
    table = rng.standard_normal((n_items, d)).astype(np.float32)
    recs = np.stack([rng.permutation(n_items)[:k] if k <= n_items
                     else rng.integers(0, n_items, k) for _ in range(n_users)]).astype(np.int64)
    if repeat:
        recs[:, 1] = recs[:, 0]
    grad_out = rng.standard_normal(n_users).astype(np.float32)
    for a in (table, recs, grad_out):
        a.setflags(write=False)
    return table, recs, grad_out


@functools.lru_cache(maxsize=None)
def case_reference(n_users, n_items, k, d, repeat, kind, with_grad_out=True, scale=1.0):
    table, recs, grad_out = case(n_users, n_items, k, d, repeat)
    ref = ild_grad_f64(table, recs, kind, grad_out if with_grad_out else None, scale)
    ref.setflags(write=False)
    return ref
