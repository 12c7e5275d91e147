"""Embedding-ILD gradient on the GPU: dr_ild_embedding_backward against the
float64 autograd reference of tests/ild_grad_checks.py, its autograd wiring in
IntraListDiversityScore, and diversity_pair_wise_train_loop.

Every gradient comparison uses ild_grad_checks.assert_grad_close:
|got - ref| <= 1e-4 |ref| + 1e-5 max|ref| (the fp32 closed forms sit at
<= 4e-7 max|ref| on the CPU; the atomics reorder the sums from run to run)."""
import os
import random

import numpy as np
import pytest
import torch

import oracle
from divrec import _backend, datasets, losses, metrics, models, ops, train
from divrec.losses import EmbeddingDistance, IntraListDiversityScore
from ild_grad_checks import KINDS, assert_grad_close, case, case_reference, ild_grad_f64

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = torch.device("cuda", 0)

# (n_users, n_items, k, d, position 1 repeats position 0)
SHAPES = [
    (64, 300, 2, 32, False),
    (64, 300, 10, 100, True),
    (64, 300, 100, 128, False),
    (33, 150, 128, 256, False),
    (64, 40, 37, 64, False),      # many shared rows
    (3000, 500, 10, 32, False),   # more lists than one pass of the grid
]


def on_device(a, dtype=None):
    return torch.tensor(np.asarray(a)).to(DEV, dtype)  # a copy: the cached cases are read-only


def run_kernel(table, recs, kind, rec_dtype=torch.int64, grad_out=None, scale=1.0, calls=1,
               **kw):
    T, R = on_device(table), on_device(recs, rec_dtype)
    go = None if grad_out is None else on_device(grad_out)
    G = torch.zeros_like(T)
    for _ in range(calls):
        ops.ild_embedding_backward(R, T, kind, G, grad_out=go, scale=scale, **kw)
    return G.cpu().numpy()


@pytest.mark.parametrize("rec_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:4])))
def test_kernel_against_float64(shape, kind, rec_dtype):
    table, recs, grad_out = case(*shape)
    got = run_kernel(table, recs, kind, rec_dtype, grad_out)
    assert_grad_close(got, case_reference(*shape, kind))


@pytest.mark.parametrize("rec_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_without_grad_out_and_with_scale(kind, rec_dtype):
    shape = SHAPES[1]
    table, recs, _ = case(*shape)
    got = run_kernel(table, recs, kind, rec_dtype, None, scale=0.5)
    assert_grad_close(got, case_reference(*shape, kind, False, 0.5))


@pytest.mark.parametrize("kind", KINDS)
def test_second_call_accumulates(kind):
    shape = SHAPES[4]
    table, recs, grad_out = case(*shape)
    got = run_kernel(table, recs, kind, torch.int64, grad_out, calls=2)
    assert_grad_close(got, 2.0 * case_reference(*shape, kind))


def test_k_of_one_adds_nothing():
    table, recs, _ = case(64, 300, 2, 32)
    assert not run_kernel(table, recs[:, :1], "cosine").any()


def test_cosine_zero_norm_row():
    """An all-zero item in half the lists: it gets no gradient and leaves the
    unit-row sum of its lists; nothing non-finite reaches the table."""
    table, recs, grad_out = (a.copy() for a in case(64, 300, 10, 100))
    zero = 0
    recs[recs == zero] = 1  # the zero item only where it is placed below
    table[zero] = 0.0
    recs[::2, 3] = zero
    got = run_kernel(table, recs, "cosine", torch.int64, grad_out)
    assert np.isfinite(got).all() and not got[zero].any()
    assert_grad_close(got, ild_grad_f64(table, recs, "cosine", grad_out))


@pytest.mark.parametrize("rec_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_range_contract(rec_dtype):
    table, recs, grad_out = (a.copy() for a in case(16, 300, 10, 100))
    recs[3, 7], recs[9, 0] = 300, -1
    ref = ild_grad_f64(table, recs, "cosine", grad_out)  # the other 14 lists
    err = _backend.error_counter(DEV)
    got = run_kernel(table, recs, "cosine", rec_dtype, grad_out, err=err, check=False)
    assert int(err.item()) == 2
    assert_grad_close(got, ref)
    with pytest.raises(IndexError):
        run_kernel(table, recs, "cosine", rec_dtype, grad_out)


# --------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("kind", KINDS)
def test_autograd_through_the_score(kind, reduction):
    shape = SHAPES[1]  # d = 100: the forward's table is padded, the gradient's is not
    table, recs, grad_out = case(*shape)
    n = recs.shape[0]
    W = torch.nn.Parameter(on_device(table))
    R = on_device(recs)
    score = IntraListDiversityScore(distance_matrix=EmbeddingDistance(W, kind, differentiable=True),
                                    reduction=reduction)
    out = score(None, R)
    assert out.grad_fn is not None
    # today's value, bit for bit: the same score without the flag, and the op itself
    today = IntraListDiversityScore(distance_matrix=EmbeddingDistance(W, kind), reduction=reduction)
    assert torch.equal(out.detach(), today(None, R))
    if reduction == "none":
        assert torch.equal(out.detach(), ops.ild_embedding(R, W.detach().to(torch.bfloat16), kind))
        (out * on_device(grad_out)).sum().backward()
        ref = case_reference(*shape, kind)
    else:
        (1.5 * out).backward()
        ref = ild_grad_f64(table, recs, kind, np.full(n, 1.5 / n if reduction == "mean" else 1.5))
    assert W.grad.shape == W.shape and not W.grad.is_sparse
    assert_grad_close(W.grad.cpu().numpy(), ref)


def test_autograd_is_opt_in():
    table, recs, _ = case(*SHAPES[1])
    W = torch.nn.Parameter(on_device(table))
    R = on_device(recs)
    on = IntraListDiversityScore(distance_matrix=EmbeddingDistance(W, "cosine", differentiable=True),
                                 reduction="none")
    off = IntraListDiversityScore(distance_matrix=EmbeddingDistance(W, "cosine"), reduction="none")
    with torch.no_grad():
        quiet = on(None, R)
    assert quiet.grad_fn is None and not quiet.requires_grad
    plain = off(None, R)
    assert plain.grad_fn is None and not plain.requires_grad
    assert torch.equal(quiet, plain) and torch.equal(on(None, R).detach(), plain)
    long_lists = torch.arange(129, device=DEV).remainder(300).reshape(1, 129)
    with pytest.raises(ValueError, match="128"):
        on(None, long_lists)
    assert off(None, long_lists).shape == (1,)  # the metric takes any length, as before


# --------------------------------------------------------------------------- the loop
def load(name):
    return np.load(os.path.join(GOLD, f"{name}.npz"), allow_pickle=False)


def mf_from(U, I):
    mf = models.MatrixFactorization(U.shape[0], I.shape[0], U.shape[1])
    with torch.no_grad():
        mf.user_embeddings.weight.copy_(torch.from_numpy(U))
        mf.item_embeddings.weight.copy_(torch.from_numpy(I))
    return mf.to(DEV)


def loop_setup(g):
    """(pair-wise data set, model) of the ``bpr_loop`` fixture, seeded as
    test_pair_wise_train_loop_golden seeds them."""
    data = datasets.UserItemInteractionsDataset(
        torch.from_numpy(g["train"]), user_features=datasets.Features(torch.zeros(12, 1), ["x"]),
        item_features=datasets.Features(torch.zeros(40, 1), ["x"]))
    mf = mf_from(g["U0"], g["I0"])
    random.seed(int(g["seed"]))
    return datasets.PairWiseDataset(data, max_sampled=int(g["max_sampled"])), mf


def diversity_of(mf, kind="cosine"):
    return IntraListDiversityScore(
        distance_matrix=EmbeddingDistance(mf.item_embeddings.weight, kind, differentiable=True))


def tables(mf):
    return (mf.user_embeddings.weight.detach().cpu().numpy(),
            mf.item_embeddings.weight.detach().cpu().numpy())


def test_loop_with_zero_weight_is_the_pair_wise_loop():
    """diversity_weight = 0 on the fused Adam path: the golden epoch of
    test_pair_wise_train_loop_golden at that test's tolerances."""
    g = load("bpr_loop")
    pw, mf = loop_setup(g)
    opt = torch.optim.Adam(mf.parameters(), lr=float(g["lr"]))
    mean_loss, (mean_auc,), mean_ild = train.diversity_pair_wise_train_loop(
        pw, mf, losses.LogSigmoidDifferenceLoss(), opt, diversity_of(mf), 0.0, 5,
        scores=[metrics.AUCScore()], batch_size=int(g["batch_size"]))
    assert mean_loss == pytest.approx(float(g["mean_loss"]), rel=1e-5)
    assert mean_auc == pytest.approx(float(g["mean_auc"]), abs=1e-6)
    U1, I1 = tables(mf)
    assert np.allclose(U1, g["U1"], atol=1e-5)
    assert np.allclose(I1, g["I1"], atol=1e-5)
    assert 0.0 < mean_ild < 1.0  # cosine ILD = (mean pair distance) / 2, distances in [0, 2]


@pytest.mark.parametrize("kind", KINDS)
def test_loop_takes_the_exact_step(kind):
    """One SGD step over one batch holding every triple: the tables move by
    -lr (g_bpr + g_reg), g_bpr from the oracle on the batch's triples and
    g_reg from the float64 reference over the initial weights' lists with
    scale = -weight / n_users. lr |g_reg| is at least 100 x the 1e-5 bar, so a
    missing or mis-scaled diversity term cannot pass."""
    g = load("bpr_loop")
    lam, lr, k, everything = 4.0, 0.25, 5, 1 << 20
    pw, mf = loop_setup(g)
    (batch,) = list(pw.loader(batch_size=everything))
    uid, pid, nid = (t.numpy() for t in batch[:3])
    users = torch.unique(batch[0])
    items, _ = mf.score_topk(k, user_ids=users)
    _, _, gU, gI = oracle.bpr_forward_backward(g["U0"], g["I0"], uid, pid, nid)
    g_reg = ild_grad_f64(g["I0"], items.cpu().numpy(), kind, None, scale=-lam / users.numel())
    assert np.abs(lr * g_reg).max() >= 100 * 1e-5
    pw, mf = loop_setup(g)  # reseeded: the loop draws the same triples
    opt = torch.optim.SGD(mf.parameters(), lr=lr)
    _, _, mean_ild = train.diversity_pair_wise_train_loop(
        pw, mf, losses.LogSigmoidDifferenceLoss(), opt, diversity_of(mf, kind), lam, k,
        batch_size=everything)
    U1, I1 = tables(mf)
    assert np.allclose(U1, g["U0"] - lr * gU, atol=1e-5)
    assert np.allclose(I1, g["I0"] - lr * (gI + g_reg), atol=1e-5)
    I0_bf16 = torch.from_numpy(g["I0"]).to(DEV, torch.bfloat16)
    assert mean_ild == pytest.approx(float(ops.ild_embedding(items, I0_bf16, kind).mean()), rel=1e-6)


def test_loop_sparse_adam_leaves_the_gradient_tables_zero():
    """The lazy step's touched rows include the lists' items."""
    g = load("bpr_loop")
    pw, mf = loop_setup(g)
    before = tables(mf)
    opt = torch.optim.SparseAdam(list(mf.parameters()), lr=float(g["lr"]))
    train.diversity_pair_wise_train_loop(
        pw, mf, losses.LogSigmoidDifferenceLoss(), opt, diversity_of(mf), 0.5, 5,
        batch_size=int(g["batch_size"]))
    assert not mf.item_embeddings.weight.grad.any()
    assert not mf.user_embeddings.weight.grad.any()
    assert not np.array_equal(tables(mf)[1], before[1])


def test_loop_bad_arguments():
    g = load("bpr_loop")
    pw, mf = loop_setup(g)
    before = tables(mf)
    opt = torch.optim.Adam(mf.parameters(), lr=0.01)
    I = mf.item_embeddings.weight
    plain = IntraListDiversityScore(distance_matrix=EmbeddingDistance(I, "cosine"))
    other = IntraListDiversityScore(
        distance_matrix=EmbeddingDistance(I.detach().clone(), "cosine", differentiable=True))
    dense = IntraListDiversityScore(distance_matrix=torch.zeros(40, 40))
    for diversity in (plain, other, dense):
        with pytest.raises(ValueError):
            train.diversity_pair_wise_train_loop(pw, mf, losses.LogSigmoidDifferenceLoss(), opt,
                                                 diversity, 0.5, 5, batch_size=64)
    with pytest.raises(ValueError):
        train.diversity_pair_wise_train_loop(pw, torch.nn.Linear(2, 2),
                                             losses.LogSigmoidDifferenceLoss(), opt,
                                             diversity_of(mf), 0.5, 5, batch_size=64)
    after = tables(mf)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
