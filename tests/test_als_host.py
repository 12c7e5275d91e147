"""ALS without a GPU: the numpy restatement of tests/als_checks.py against the
properties of the spec (normal equations, optimality, monotone descent),
datasets.interaction_csr on CPU tensors, dr_als_solve's argument checks (they
run before any HIP call) and the error paths of the Python doors."""
import ctypes

import numpy as np
import pytest
import torch

import als_checks as ac
from divrec import _backend, datasets, models, ops, train
from divrec.datasets import interaction_csr  # noqa: F401  (the module needs the feature)
from divrec.train import als_train_loop  # noqa: F401


# --------------------------------------------------------------------------- restatement
def test_restatement_solves_the_normal_equations():
    Y = ac.table(300, 32, 1)
    rows, w = ac.case_rows(300, 2, n=20)
    x = ac.solve(Y, rows, w, ac.ALPHA, 0.1, np.float64)
    G = ac.gram32(Y).astype(np.float64)
    for r, idx in enumerate(rows):
        if len(idx) == 0:
            assert not x[r].any()
            continue
        Yr, wr = Y[idx].astype(np.float64), w[r].astype(np.float64)
        A = G + ac.ALPHA * (Yr.T * wr) @ Yr + 0.1 * np.eye(32)
        b = ((1 + ac.ALPHA * wr)[:, None] * Yr).sum(0)
        assert np.linalg.norm(A @ x[r] - b) <= 1e-12 * np.linalg.norm(b)


def test_restatement_row_is_the_minimiser_of_the_objective():
    Y = ac.table(120, 32, 3)
    rows, w = ac.case_rows(120, 4, n=12)
    rows = [np.unique(idx) for idx in rows]  # the dense form has no repeats
    w = [x[:len(idx)] for x, idx in zip(w, rows)]
    X = ac._solve64(Y.astype(np.float64), rows, w, ac.ALPHA, 0.1)
    J = ac.objective(X, Y, rows, w, ac.ALPHA, 0.1)
    assert abs(J - ac.objective_dense(X, Y, rows, w, ac.ALPHA, 0.1)) <= 1e-10 * abs(J)
    rng = np.random.default_rng(0)
    for _ in range(8):
        step = 1e-3 * rng.standard_normal(X.shape)
        assert ac.objective(X + step, Y, rows, w, ac.ALPHA, 0.1) > J


def test_restatement_als_descends_at_every_half_step():
    pairs, scores = ac.interactions()
    rows, w = ac.pair_rows(pairs, scores, 200)
    hist = ac.als_f64(ac.table(200, 64, 7), ac.table(300, 64, 8), rows, w, ac.ALPHA, 0.1, 4)
    assert len(hist) == 9
    assert all(b < a for a, b in zip(hist, hist[1:])), hist


def test_restatement_error_figures():
    """E_ref of the float32 restatement: of the size the tolerance rule was
    written for (a few 1e-7; about 1e-5 on the ill-conditioned case)."""
    *_, e = ac.case(32, 300, 0.1, True)
    assert 5e-8 < e < 5e-6
    *_, e = ac.case(*ac.ILL, True)
    assert 5e-7 < e < 1e-4


# --------------------------------------------------------------------------- interaction_csr
def _data(pairs, scores=None, **kw):
    return datasets.UserItemInteractionsDataset(
        interactions=torch.from_numpy(pairs),
        interaction_scores=None if scores is None else torch.from_numpy(scores), **kw)


def _check_csr(got, rows, w):
    rowptr, cols, vals = (None if t is None else t.numpy() for t in got)
    want_ptr, want_cols, want_w = ac.csr(rows, w)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32
    assert np.array_equal(rowptr, want_ptr) and np.array_equal(cols, want_cols)
    if w is None:
        assert vals is None
    else:
        assert got[2].dtype == torch.float32
        np.testing.assert_allclose(vals, want_w, rtol=1e-6)


def test_interaction_csr_both_orientations_with_repeats_and_scores():
    pairs, scores = ac.interactions()
    rows, w = ac.pair_rows(pairs, scores, 200)
    t_rows, t_w = ac.transpose(rows, w, 300)
    data = _data(pairs, scores)
    assert len(np.unique(pairs, axis=0)) < len(pairs)  # the repeats are there
    _check_csr(datasets.interaction_csr(data, 200, 300, "cpu", "user", True), rows, w)
    _check_csr(datasets.interaction_csr(data, 200, 300, "cpu", "item", True), t_rows, t_w)
    _check_csr(datasets.interaction_csr(data, 200, 300, "cpu", "user"), rows, None)
    _check_csr(datasets.interaction_csr(data, 200, 300, "cpu", by="item"), t_rows, None)


def test_interaction_csr_empty_rows_and_larger_tables():
    pairs = np.array([[0, 5], [3, 1], [3, 1], [3, 0], [6, 5]], dtype=np.int64)
    scores = np.array([1.0, 2.0, 0.5, 4.0, 8.0], dtype=np.float32)
    data = _data(pairs, scores)
    rowptr, cols, vals = datasets.interaction_csr(data, 9, 8, "cpu", "user", True)
    assert rowptr.tolist() == [0, 1, 1, 1, 3, 3, 3, 4, 4, 4]  # users 1, 2, 4, 5, 7, 8 are empty
    assert cols.tolist() == [5, 0, 1, 5] and vals.tolist() == [1.0, 4.0, 2.5, 8.0]
    rowptr, cols, vals = datasets.interaction_csr(data, 9, 8, "cpu", "item", True)
    assert rowptr.tolist() == [0, 1, 2, 2, 2, 2, 4, 4, 4]
    assert cols.tolist() == [3, 3, 0, 6] and vals.tolist() == [4.0, 2.5, 1.0, 8.0]
    with pytest.raises(ValueError, match="more than"):
        datasets.interaction_csr(data, 6, 8, "cpu")
    with pytest.raises(ValueError, match="by must be"):
        datasets.interaction_csr(data, 9, 8, "cpu", by="row")
    empty = datasets.UserItemInteractionsDataset()
    rowptr, cols, vals = datasets.interaction_csr(empty, 3, 2, "cpu", "user", True)
    assert rowptr.tolist() == [0, 0, 0, 0] and cols.numel() == 0 and vals.numel() == 0


# --------------------------------------------------------------------------- C ABI
def _solve_rc(n_fixed=10, d=64, n_rows=4, alpha=1.0, reg=0.1, ptr=None):
    lib = _backend.load_library()
    rc = lib.dr_als_solve(ptr, n_fixed, d, ptr, ptr, ptr, None, n_rows, alpha, reg, ptr, None, None)
    return rc, lib.dr_last_error()


def test_als_solve_argument_errors_without_gpu():
    for d in (0, 48, 100, 256):
        rc, msg = _solve_rc(d=d)
        assert rc == -1 and b"dr_als_solve: d must be" in msg
    for reg in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg = _solve_rc(reg=reg)
        assert rc == -1 and b"reg must be > 0" in msg
    for alpha in (-0.5, float("nan"), float("inf")):
        rc, msg = _solve_rc(alpha=alpha)
        assert rc == -1 and b"alpha must be >= 0" in msg
    rc, msg = _solve_rc(n_rows=-1)
    assert rc == -1 and b"n_rows" in msg
    rc, msg = _solve_rc(n_fixed=1 << 31)
    assert rc == -1 and b"n_fixed_rows" in msg
    rc, msg = _solve_rc()
    assert rc == -1 and b"null pointer" in msg
    buf = (ctypes.c_float * 4)()
    rc, msg = _solve_rc(ptr=None, n_rows=0)
    assert rc == 0  # no rows: a no-op, whatever the pointers
    assert _solve_rc(ptr=ctypes.addressof(buf), n_rows=0)[0] == 0
    assert "dr_als_solve" in _backend.SIGNATURES and ops.ALS_WIDTHS == (32, 64, 128)


# --------------------------------------------------------------------------- doors
def test_gram_is_symmetric_float64_rounded_once():
    Y = ac.table(1000, 48, 11)
    g = ops.gram(torch.from_numpy(Y))
    assert g.dtype == torch.float32 and g.shape == (48, 48) and torch.equal(g, g.T)
    assert np.array_equal(g.numpy(), ac.gram32(Y))
    chunked = ops.GRAM_CHUNK_ROWS
    try:
        ops.GRAM_CHUNK_ROWS = 300  # several chunks
        g2 = ops.gram(torch.from_numpy(Y))
    finally:
        ops.GRAM_CHUNK_ROWS = chunked
    np.testing.assert_allclose(g2.numpy(), g.numpy(), rtol=1e-6, atol=1e-5)
    big = ac.table(2 * ops.GRAM_BLOCK_ROWS + 77, 48, 12)  # whole blocks and a remainder
    g3 = ops.gram(torch.from_numpy(big))
    assert torch.equal(g3, g3.T)
    np.testing.assert_allclose(g3.numpy(), ac.gram32(big), rtol=1e-6, atol=1e-5)


def test_als_train_loop_value_errors_come_before_the_device():
    pairs, scores = ac.interactions()
    data = _data(pairs, scores)
    mf = models.MatrixFactorization(200, 300, 16)  # on the CPU
    with pytest.raises(ValueError, match="do not cover"):
        train.als_train_loop(data, models.MatrixFactorization(150, 300, 16), 1)
    with pytest.raises(ValueError, match="do not cover"):
        train.als_train_loop(data, models.MatrixFactorization(200, 299, 16), 1)
    with pytest.raises(ValueError, match="embedding_dim <= 128"):
        train.als_train_loop(data, models.MatrixFactorization(200, 300, 129), 1)
    with pytest.raises(ValueError, match="MatrixFactorization"):
        train.als_train_loop(data, models.RandomModel(200, 300), 1)

    class Other(models.MatrixFactorization):
        def forward(self, user_id, item_id, user_features=None, item_features=None):
            return super().forward(user_id, item_id) * 2

    with pytest.raises(ValueError, match="MatrixFactorization"):
        train.als_train_loop(data, Other(200, 300, 16), 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        train.als_train_loop(data, mf, 1)
    assert "als_train_loop" in train.__all__ and "interaction_csr" in datasets.__all__


def test_model_doors_on_a_cpu_model():
    mf = models.MatrixFactorization(20, 30, 16)
    rowptr = torch.tensor([0, 2, 3], dtype=torch.int64)
    items = torch.tensor([1, 4, 7], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mf.fold_in_users(rowptr, items)
    v = torch.zeros(2, 16)
    with pytest.raises(ValueError, match="user_ids must be None"):
        mf.score_topk(5, user_ids=torch.tensor([0, 1]), user_vectors=v)
    with pytest.raises(ValueError, match="user_ids must be None"):
        mf.recommend_diverse(5, 10, user_ids=torch.tensor([0, 1]), user_vectors=v)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mf.score_topk(5, user_vectors=v)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_als_ops_fail_loudly_without_gpu():
    Y = torch.from_numpy(ac.table(30, 32, 0))
    rowptr, cols = torch.tensor([0, 1], dtype=torch.int64), torch.tensor([3], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.als_solve(Y, rowptr, cols)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.als_objective(Y[:1], Y, rowptr, cols, None, 1.0, 0.1)
