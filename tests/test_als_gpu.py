"""dr_als_solve on the GPU (ops.als_solve, train.als_train_loop and the model's
fold-in doors) against the float64 restatement of tests/als_checks.py by its
tolerance rule (the kernel's error <= 10 x the float32 restatement's, per
case), and the exact properties of the spec: empty rows exactly 0, bitwise
reproducibility whatever the grid, the padding and the row order, bad entries
counted, a bad pivot a NaN row."""
import functools

import numpy as np
import pytest
import torch

import als_checks as ac
from divrec import _backend, datasets, models, ops, train
from divrec.ops import als_objective, als_solve  # noqa: F401  (the module needs the feature)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(x):
    return None if x is None else torch.from_numpy(x).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(d, m, reg, weighted):
    """One case's inputs and references, computed once and shared (read-only)."""
    return ac.case(d, m, reg, weighted)


def _run(Y, rows, w, reg, alpha=ac.ALPHA, **kw):
    rowptr, cols, weights = ac.csr(rows, w)
    out = ops.als_solve(_dev(Y), _dev(rowptr), _dev(cols), _dev(weights), alpha=alpha, reg=reg, **kw)
    assert out.dtype == torch.float32 and out.shape == (len(rows), Y.shape[1])
    return out


def _judge(got, x64, rows, e_ref, what):
    e_gpu = ac.rel_err(got.double().cpu().numpy(), x64, rows)
    print(f"{what}: E_gpu = {e_gpu:.3e}, E_ref = {e_ref:.3e}, ratio = {e_gpu / e_ref:.2f}")
    assert e_gpu <= ac.FACTOR * e_ref, (what, e_gpu, e_ref)
    for r, idx in enumerate(rows):
        if len(idx) == 0:
            assert not got[r].any(), f"{what}: empty row {r} is not exactly 0"


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("d,m,reg", ac.CASES)
def test_als_solve_matches_the_float64_solve(d, m, reg, weighted):
    """Rows of 0, 1, chunk - 1, chunk, chunk + 1 and 200 entries and random
    lengths; d = 100 runs zero-padded at 128."""
    Y, rows, w, x64, e_ref = _case(d, m, reg, weighted)
    assert [len(x) for x in rows[:6]] == [0, 1, ac.CHUNK - 1, ac.CHUNK, ac.CHUNK + 1, 200]
    _judge(_run(Y, rows, w, reg), x64, rows, e_ref, f"d={d} m={m} reg={reg} weighted={weighted}")


def test_als_solve_ill_conditioned():
    d, m, reg = ac.ILL
    Y, rows, w, x64, e_ref = _case(d, m, reg, True)
    _judge(_run(Y, rows, w, reg), x64, rows, e_ref, "ill-conditioned 128 x 160")


def test_als_solve_bitwise_equalities():
    d, m, reg = 100, 500, 0.05
    Y, rows, w, _, _ = _case(d, m, reg, True)
    base = _run(Y, rows, w, reg)
    assert torch.equal(base, _run(Y, rows, w, reg))  # two calls
    # the table pre-padded to 128 columns: the same rows, then zeros
    wide = np.zeros((m, 128), dtype=np.float32)
    wide[:, :d] = Y
    padded = _run(wide, rows, w, reg)
    assert torch.equal(padded[:, :d], base) and not padded[:, d:].any()
    # few workgroups (many rows each) against the default grid
    with _backend.plan_knobs(scan_slots=2):
        assert torch.equal(base, _run(Y, rows, w, reg))
    # a permutation of the CSR rows permutes the output rows
    perm = np.random.default_rng(3).permutation(len(rows))
    shuffled = _run(Y, [rows[p] for p in perm], [w[p] for p in perm], reg)
    assert torch.equal(shuffled, base[torch.from_numpy(perm).to(DEV)])
    # out= is written in place and returned; a given gram is the default one
    rowptr, cols, weights = (_dev(x) for x in ac.csr(rows, w))
    out = torch.full((len(rows), d), 7.0, device=DEV)
    got = ops.als_solve(_dev(Y), rowptr, cols, weights, alpha=ac.ALPHA, reg=reg,
                        gram=ops.gram(_dev(Y)), out=out)
    assert got is out and torch.equal(out, base)


def test_als_solve_null_weights_are_ones():
    d, m, reg = 64, 600, 0.1
    Y, rows, _, _, _ = _case(d, m, reg, False)
    ones = [np.ones(len(x), dtype=np.float32) for x in rows]
    assert torch.equal(_run(Y, rows, None, reg), _run(Y, rows, ones, reg))


def test_als_solve_repeated_columns_count_once_per_occurrence():
    d, m, reg = 32, 300, 0.1
    Y = ac.table(m, d, 21)
    rows = [np.array([5, 9, 5, 5, 200], dtype=np.int64), np.array([5, 9, 200], dtype=np.int64)]
    w = [np.array([1, 2, 0.5, 1.5, 3], dtype=np.float32), np.array([3, 2, 3], dtype=np.float32)]
    x64 = ac.solve(Y, rows, w, ac.ALPHA, reg, np.float64)
    e_ref = ac.rel_err(ac.solve(Y, rows, w, ac.ALPHA, reg, np.float32), x64, rows)
    got = _run(Y, rows, w, reg)
    _judge(got, x64, rows, e_ref, "repeated columns")
    # A is the same for both rows (the weights of column 5 add up to 3), b is not
    assert not torch.allclose(got[0], got[1], rtol=1e-3)


def test_als_solve_bad_entries():
    d, m, reg = 64, 600, 0.1
    Y, rows, w, _, _ = _case(d, m, reg, True)
    bad_rows = [x.copy() for x in rows]
    bad_rows[4][7] = m          # the first id past the table
    bad_rows[9][0] = -3
    with pytest.raises(IndexError, match="2 entries"):
        _run(Y, bad_rows, w, reg)
    # unchecked: the entries contribute nothing
    valid = [(x >= 0) & (x < m) for x in bad_rows]
    kept_rows = [x[ok] for x, ok in zip(bad_rows, valid)]
    kept_w = [x[ok] for x, ok in zip(w, valid)]
    assert sum(len(x) for x in kept_rows) == sum(len(x) for x in rows) - 2
    x64 = ac.solve(Y, kept_rows, kept_w, ac.ALPHA, reg, np.float64)
    e_ref = ac.rel_err(ac.solve(Y, kept_rows, kept_w, ac.ALPHA, reg, np.float32), x64, kept_rows)
    got = _run(Y, bad_rows, w, reg, check=False)
    _judge(got, x64, kept_rows, e_ref, "bad entries skipped")
    # a NaN weight: that row is NaN, every other row is bitwise what it was
    base = _run(Y, rows, w, reg)
    nan_w = [x.copy() for x in w]
    nan_w[5][3] = np.nan
    got = _run(Y, rows, nan_w, reg, check=False)
    assert torch.isnan(got[5]).all()
    keep = torch.arange(len(rows), device=DEV) != 5
    assert torch.equal(got[keep], base[keep])
    # a negative weight large enough for a pivot <= 0: NaN too, and no hang
    neg_w = [x.copy() for x in w]
    neg_w[5][:] = -50.0
    got = _run(Y, rows, neg_w, reg, check=False)
    assert torch.isnan(got[5]).all() and torch.equal(got[keep], base[keep])


def test_als_solve_validates_its_arguments():
    Y, rows, w, _, _ = _case(64, 600, 0.1, True)
    rowptr, cols, weights = (_dev(x) for x in ac.csr(rows, w))
    Yd = _dev(Y)
    with pytest.raises(ValueError, match="reg must be"):
        ops.als_solve(Yd, rowptr, cols, weights, reg=0.0)
    with pytest.raises(ValueError, match="alpha must be"):
        ops.als_solve(Yd, rowptr, cols, weights, alpha=-1.0)
    with pytest.raises(ValueError, match="rowptr must rise"):
        ops.als_solve(Yd, rowptr[:-1], cols, weights)
    with pytest.raises(ValueError, match="cols must be int32"):
        ops.als_solve(Yd, rowptr, cols.to(torch.int64), weights)
    with pytest.raises(ValueError, match="embedding_dim <= 128"):
        ops.als_solve(torch.zeros(10, 130, device=DEV), rowptr, cols, weights)
    with pytest.raises(ValueError, match="gram must be"):
        ops.als_solve(Yd, rowptr, cols, weights, gram=torch.zeros(32, 32, device=DEV))
    empty = ops.als_solve(Yd, torch.zeros(1, dtype=torch.int64, device=DEV), cols[:0])
    assert empty.shape == (0, 64)
    zeros = ops.als_solve(Yd, torch.zeros(4, dtype=torch.int64, device=DEV), cols[:0])
    assert zeros.shape == (3, 64) and not zeros.any()


# --------------------------------------------------------------------------- trainer
U_, I_, D_ = 200, 300, 64
ALS_ALPHA, ALS_REG = 2.0, 0.1


def _data():
    pairs, scores = ac.interactions(U_, I_)
    return (datasets.UserItemInteractionsDataset(interactions=torch.from_numpy(pairs),
                                                 interaction_scores=torch.from_numpy(scores)),
            pairs, scores)


def _model(seed=0):
    torch.manual_seed(seed)
    return models.MatrixFactorization(U_, I_, D_).to(DEV)


def _tables(mf):
    return (mf.user_embeddings.weight.detach().cpu().numpy(),
            mf.item_embeddings.weight.detach().cpu().numpy())


@pytest.mark.parametrize("use_scores", [False, True])
def test_als_train_loop_descends_and_each_half_step_is_the_exact_solve(use_scores):
    data, pairs, scores = _data()
    rows, w = ac.pair_rows(pairs, scores, U_)
    if not use_scores:
        w = None
    t_rows, t_w = ac.transpose(rows, w, I_)
    mf = _model()
    hist = train.als_train_loop(data, mf, 0, ALS_ALPHA, ALS_REG, use_scores)
    assert len(hist) == 1
    for it in range(3):
        # one iteration at a time: each half-step against the float64 solve
        # given the GPU's own other table, so the trajectory is never a tolerance
        X0, Y0 = _tables(mf)
        version = mf.user_embeddings.weight._version
        step = train.als_train_loop(data, mf, 1, ALS_ALPHA, ALS_REG, use_scores)
        assert mf.user_embeddings.weight._version > version
        X1, Y1 = _tables(mf)
        assert len(step) == 3 and abs(step[0] - hist[-1]) <= 1e-9 * abs(hist[-1])
        hist += step[1:]
        for new, fixed, rr, ww, what in ((X1, Y0, rows, w, "users"), (Y1, X1, t_rows, t_w, "items")):
            x64 = ac.solve(fixed, rr, ww, ALS_ALPHA, ALS_REG, np.float64)
            e_ref = ac.rel_err(ac.solve(fixed, rr, ww, ALS_ALPHA, ALS_REG, np.float32), x64, rr)
            e_gpu = ac.rel_err(new.astype(np.float64), x64, rr)
            print(f"iteration {it} {what}: E_gpu = {e_gpu:.3e}, E_ref = {e_ref:.3e}")
            assert e_gpu <= ac.FACTOR * e_ref, (it, what, e_gpu, e_ref)
        want = ac.objective(X1, Y1, rows, w, ALS_ALPHA, ALS_REG)
        assert abs(hist[-1] - want) <= 1e-6 * abs(want)
    assert len(hist) == 7 and all(b < a for a, b in zip(hist, hist[1:])), hist


def test_als_train_loop_whole_run_and_scores_matter():
    data, pairs, scores = _data()
    rows, w = ac.pair_rows(pairs, scores, U_)
    mf = _model()
    hist = train.als_train_loop(data, mf, 3, ALS_ALPHA, ALS_REG, use_scores=True)
    assert len(hist) == 7 and all(b < a for a, b in zip(hist, hist[1:])), hist
    X, Y = _tables(mf)
    want = ac.objective(X, Y, rows, w, ALS_ALPHA, ALS_REG)
    assert abs(hist[-1] - want) <= 1e-6 * abs(want)
    plain = _model()
    assert train.als_train_loop(data, plain, 3, ALS_ALPHA, ALS_REG, compute_loss=False) == []
    assert not torch.allclose(plain.user_embeddings.weight, mf.user_embeddings.weight, rtol=1e-3)


def test_als_train_loop_odd_width_and_a_larger_model():
    """embedding_dim = 20 (padded to 32) and tables larger than the data: the
    extra users and items are empty rows, solved to exactly 0."""
    data, pairs, scores = _data()
    torch.manual_seed(1)
    mf = models.MatrixFactorization(U_ + 5, I_ + 3, 20).to(DEV)
    hist = train.als_train_loop(data, mf, 2, ALS_ALPHA, ALS_REG)
    assert len(hist) == 5 and all(b < a for a, b in zip(hist, hist[1:])), hist
    assert not mf.user_embeddings.weight[U_:].any() and not mf.item_embeddings.weight[I_:].any()
    assert mf.user_embeddings.weight[:U_].any()


# --------------------------------------------------------------------------- fold-in
def test_fold_in_reproduces_trained_users_and_feeds_every_scorer():
    data, pairs, scores = _data()
    rows, w = ac.pair_rows(pairs, scores, U_)
    mf = _model()
    train.als_train_loop(data, mf, 2, ALS_ALPHA, ALS_REG, use_scores=True, compute_loss=False)
    # refresh the users against the final item table: fold-in is that solve
    X, Y = _tables(mf)
    rowptr, cols, weights = ac.csr(rows, w)
    v = mf.fold_in_users(torch.from_numpy(rowptr), torch.from_numpy(cols),
                         torch.from_numpy(weights), alpha=ALS_ALPHA, reg=ALS_REG)
    assert v.shape == (U_, D_) and v.dtype == torch.float32 and v.device.type == "cuda"
    x64 = ac.solve(Y, rows, w, ALS_ALPHA, ALS_REG, np.float64)
    e_ref = ac.rel_err(ac.solve(Y, rows, w, ALS_ALPHA, ALS_REG, np.float32), x64, rows)
    e_gpu = ac.rel_err(v.double().cpu().numpy(), x64, rows)
    print(f"fold-in: E_gpu = {e_gpu:.3e}, E_ref = {e_ref:.3e}")
    assert e_gpu <= ac.FACTOR * e_ref
    with pytest.raises(IndexError):
        mf.fold_in_users(torch.tensor([0, 1]), torch.tensor([I_], dtype=torch.int32))

    some = v[:50].contiguous()
    items, sc = mf.score_topk(10, user_vectors=some)
    want_sc, want_items = ops.score_topk(some, mf.item_embeddings.weight.detach(), 10)
    assert torch.equal(items, want_items.to(torch.int64)) and torch.equal(sc, want_sc)
    # the model's own users, passed as vectors, are the model's own lists
    own_items, own_sc = mf.score_topk(10, user_ids=torch.arange(50))
    as_vec = mf.score_topk(10, user_vectors=mf.user_embeddings.weight[:50].detach().clone())
    assert torch.equal(as_vec[0], own_items) and torch.equal(as_vec[1], own_sc)
    labels = torch.arange(I_) % 7
    profile = ops.label_profile(torch.from_numpy(rowptr[:51]).to(DEV),
                                torch.from_numpy(cols[:rowptr[50]]).to(DEV), labels.to(DEV), 7)
    for method, extra in (("dpp", {}), ("mmr", {}),
                          ("calibrated", dict(item_labels=labels, user_profile=profile))):
        picks, psc = mf.recommend_diverse(10, 40, method=method, user_vectors=some, **extra)
        assert picks.shape == psc.shape == (50, 10) and picks.dtype == torch.int64
        assert (picks >= 0).all() and (picks < I_).all()
        cand, _ = mf.score_topk(40, user_vectors=some)
        assert all(set(p.tolist()) <= set(c.tolist()) for p, c in zip(picks.cpu(), cand.cpu()))
