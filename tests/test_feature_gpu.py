"""Feature-composed factorization on the GPU: dr_csr_row_sum against the
float64 restatement under the rule of tests/feature_checks.py (shown
satisfiable by tests/test_feature_host.py), its bitwise properties, the
autograd function, FeatureMatrixFactorization and its doors in divrec.train.
Fixed seeds; every case a few seconds at the most."""
import numpy as np
import pytest
import torch

import feature_checks as fc
import pairwise_checks as pc
from divrec import _backend, datasets, losses, metrics, models, ops, train
from divrec.datasets import feature_csr
from divrec.models import FeatureMatrixFactorization
from topk_checks import FP32_REL, gap_check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
L = ops.ROW_SUM_CHUNK


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def row_sum(T, rowptr, cols, w, out_dtype=torch.float32, **kw):
    """ops.csr_row_sum into an output pre-filled with NaN (an unwritten row shows)."""
    out = torch.full((len(rowptr) - 1, T.shape[1]), float("nan"), dtype=out_dtype, device=DEV)
    got = ops.csr_row_sum(dev(T), dev(rowptr), dev(cols), dev(w), out_dtype=out_dtype, out=out, **kw)
    assert got is out
    return out


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


# --------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("n_rows", fc.ROW_COUNTS)
@pytest.mark.parametrize("d", fc.WIDTHS)
def test_row_sum_against_float64(d, n_rows):
    """fp32 and bf16 output under the rule; the bf16 form is the fp32 one
    rounded once, bit for bit; empty rows are written (zeros, not the NaN fill)."""
    T, rowptr, cols, w = fc.case(d, n_rows)
    ref = fc.case_ref(d, n_rows)
    out = row_sum(T, rowptr, cols, w)
    fc.check_row_sum(out.cpu().numpy(), ref, what="fp32")
    empty = np.diff(rowptr) == 0
    assert not out.cpu().numpy()[empty].any()
    out16 = row_sum(T, rowptr, cols, w, out_dtype=torch.bfloat16)
    fc.check_row_sum(out16.to(torch.float64).cpu().numpy(), ref, bf16=True, what="bf16")
    assert np.array_equal(bits(out16), bits(out.to(torch.bfloat16)))


@pytest.mark.parametrize("n_rows", fc.ROW_COUNTS)
@pytest.mark.parametrize("d", fc.WIDTHS)
def test_row_sum_integer_cases_bit_for_bit(d, n_rows):
    T, rowptr, cols, w = fc.case(d, n_rows, integer=True)
    out64, _, _ = fc.case_ref(d, n_rows, integer=True)
    out = row_sum(T, rowptr, cols, w)
    assert np.array_equal(bits(out), out64.astype(np.float32).view(np.int32))


@pytest.mark.parametrize("d", [1, 7, 30, 512])
def test_row_sum_other_widths(d):
    """Widths that are no multiple of 4 (one float per lane) and the widest."""
    rng = np.random.default_rng(d)
    T = rng.standard_normal((50, d)).astype(np.float32)
    rows = [rng.integers(0, 50, n) for n in (3, 0, L + 3, 1)]
    rowptr, cols, w = fc.csr(rows, [rng.uniform(-1, 1, len(r)) for r in rows])
    ref = fc.row_sum_f64(T, rowptr, cols, w)
    fc.check_row_sum(row_sum(T, rowptr, cols, w).cpu().numpy(), ref, what=f"d={d}")
    out16 = row_sum(T, rowptr, cols, w, out_dtype=torch.bfloat16)
    fc.check_row_sum(out16.to(torch.float64).cpu().numpy(), ref, bf16=True, what=f"bf16 d={d}")


def _raw_row_sum(T, rowptr, cols, w, plan):
    """dr_csr_row_sum called directly, with or without the plan's lists."""
    Td, rp, c, wd = dev(T), dev(rowptr), dev(cols), dev(w)
    out = torch.full((len(rowptr) - 1, T.shape[1]), float("nan"), device=DEV)
    ws = torch.empty((max(plan.n_chunks, 1), T.shape[1]), device=DEV) if plan else None
    rc = _backend.lib().dr_csr_row_sum(
        Td.data_ptr(), T.shape[0], T.shape[1], rp.data_ptr(), c.data_ptr(), _backend.ptr(wd),
        len(rowptr) - 1, plan.lists.data_ptr() if plan else None, plan.n_chunks if plan else 0,
        plan.n_long if plan else 0, out.data_ptr(), _backend.DR_F32, _backend.ptr(ws),
        ws.numel() * 4 if plan else 0, None, _backend.stream(DEV))
    _backend.check(rc, "dr_csr_row_sum")
    return out


def test_plan_decides_who_sums_never_what():
    """Without a plan one group sums a long row's chunks itself: bitwise the
    planned result, on a case with long rows."""
    T, rowptr, cols, w = fc.case(128, 7)
    plan = ops.row_sum_plan(dev(rowptr))
    assert plan.n_long == 2 and plan.n_chunks == 2 + 4
    a = _raw_row_sum(T, rowptr, cols, w, plan)
    b = _raw_row_sum(T, rowptr, cols, w, None)
    assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(a), bits(row_sum(T, rowptr, cols, w)))


def test_row_sum_is_independent_of_position_neighbours_and_grid():
    """The same three rows (short, exactly L, 3 L + 5) alone in a CSR and at
    other places among 4000 random rows, on the full grid and on two CUs:
    bitwise equal outputs; so are two repeated calls."""
    rng = np.random.default_rng(11)
    T = rng.standard_normal((fc.TABLE_ROWS, 128)).astype(np.float32)
    rows, w = fc.independence_rows()
    alone = row_sum(T, *fc.csr(rows, w))
    fc.check_row_sum(alone.cpu().numpy(), fc.row_sum_f64(T, *fc.csr(rows, w)), what="alone")
    lens = rng.integers(0, 40, 4000)
    lens[100], lens[2500] = 2 * L + 1, L + 7  # other long rows among the neighbours
    many = [rng.integers(0, fc.TABLE_ROWS, n) for n in lens]
    many_w = [rng.uniform(-2, 2, n).astype(np.float32) for n in lens]
    at = (3999, 17, 1234)  # short row last, the long ones early and in the middle
    for k, r in enumerate(at):
        many[r], many_w[r] = rows[k], w[k]
    big = fc.csr(many, many_w)
    first = row_sum(T, *big)
    assert np.array_equal(bits(first[list(at)]), bits(alone))
    assert np.array_equal(bits(row_sum(T, *big)), bits(first))
    with _backend.plan_knobs(scan_slots=2):
        assert np.array_equal(bits(row_sum(T, *big)), bits(first))
        assert np.array_equal(bits(row_sum(T, *fc.csr(rows, w))), bits(alone))


def test_row_sum_skewed_transpose():
    """The transpose of a 5000-row map in which one feature is held by every
    row (one transposed row of 5000 entries: 10 chunks) and 200 features by
    one row each."""
    rowptr, cols, w, n_features = fc.skew_map()
    rt, ct, wt = ops.csr_transpose(dev(rowptr), dev(cols), dev(w), n_features)
    want = fc.transpose(rowptr, cols, w, n_features)
    assert np.array_equal(rt.cpu().numpy(), want[0]) and np.array_equal(ct.cpu().numpy(), want[1])
    assert np.array_equal(wt.cpu().numpy(), want[2])
    lens = np.diff(want[0])
    assert lens[0] == 5000 and (lens[1:201] == 1).all()
    G = np.random.default_rng(2).standard_normal((5000, 100)).astype(np.float32)
    plan = ops.row_sum_plan(rt)
    assert plan.n_chunks >= 10
    out = torch.full((n_features, 100), float("nan"), device=DEV)
    ops.csr_row_sum(dev(G), rt, ct, wt, plan=plan, out=out)
    fc.check_row_sum(out.cpu().numpy(), fc.row_sum_f64(G, *want), what="skewed transpose")


def test_out_of_range_column_is_counted_and_skipped():
    T, rowptr, cols, w = fc.case(100, 7)
    cols = cols.copy()
    bad = [int(rowptr[2]) + 3, int(rowptr[6]) + L + 9, int(rowptr[6]) + 2]  # a short row, two chunks
    cols[bad[0]], cols[bad[1]], cols[bad[2]] = fc.TABLE_ROWS, -1, 2 ** 30
    with pytest.raises(IndexError, match="out of range"):
        ops.csr_row_sum(dev(T), dev(rowptr), dev(cols), dev(w))
    err = _backend.error_counter(DEV)
    out = row_sum(T, rowptr, cols, w, err=err)
    assert int(err.item()) == 3
    fc.check_row_sum(out.cpu().numpy(), fc.row_sum_f64(T, rowptr, cols, w), what="bad columns")
    good = row_sum(*fc.case(100, 7))
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(bits(out[keep]), bits(good[keep]))  # every other row untouched


def test_ops_row_sum_value_errors():
    T, rowptr, cols, w = fc.case(8, 7)
    Td, rp, c = dev(T), dev(rowptr), dev(cols)
    with pytest.raises(ValueError, match="fp32 2-D"):
        ops.csr_row_sum(Td.double(), rp, c)
    with pytest.raises(ValueError, match="int32"):
        ops.csr_row_sum(Td, rp, c.long())
    with pytest.raises(ValueError, match="out_dtype"):
        ops.csr_row_sum(Td, rp, c, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="very rowptr"):
        ops.csr_row_sum(Td, rp.clone(), c, plan=ops.row_sum_plan(rp))
    with pytest.raises(ValueError, match="entries of cols"):
        ops.csr_row_sum(Td, rp, c[:-1])
    with pytest.raises(ValueError, match="columns"):
        ops.csr_row_sum(torch.zeros((4, 513), device=DEV), rp, c)
    assert ops.csr_row_sum(Td, torch.zeros(1, dtype=torch.int64, device=DEV), c[:0]).shape == (0, 8)


# --------------------------------------------------------------------------- autograd
def test_feature_sum_gradient_is_the_transposed_sum():
    rng = np.random.default_rng(5)
    n, m, d = 300, 40, 100
    rows = [rng.integers(0, m, k) for k in rng.integers(0, 6, n)]
    rows[7] = rng.integers(0, m, L + 20)
    rowptr, cols, w = fc.csr(rows, [rng.uniform(-1, 1, len(r)) for r in rows])
    S = fc.dense(rowptr, cols, w, m)
    table = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).to(DEV).requires_grad_()
    G = rng.standard_normal((n, d)).astype(np.float32)
    csr_map = ops.CsrMap(dev(rowptr), dev(cols), dev(w), m)
    out = ops.feature_sum(table, csr_map)
    fc.check_row_sum(out.detach().cpu().numpy(), fc.row_sum_f64(table.detach().cpu().numpy(),
                                                                rowptr, cols, w), what="forward")
    out.backward(dev(G))
    ref = fc.row_sum_f64(G, *fc.transpose(rowptr, cols, w, m))
    assert np.allclose(ref[0], S.T @ G.astype(np.float64), rtol=1e-12, atol=1e-12)
    fc.check_row_sum(table.grad.cpu().numpy(), ref, what="gradient")
    # reproducible: a second backward gives the same bits
    first = table.grad.clone()
    table.grad = None
    ops.feature_sum(table, csr_map).backward(dev(G))
    assert torch.equal(first, table.grad)


# --------------------------------------------------------------------------- the model
def _hybrid(d=32, n_users=60, n_items=90, seed=0):
    """A model over identity + one categorical + one numeric item feature and
    identity + one categorical user feature, with its float64 pieces."""
    rng = np.random.default_rng(seed)
    genre = rng.integers(0, 7, n_items).astype(np.float32)
    price = rng.uniform(-1, 1, n_items).astype(np.float32)
    age = rng.integers(0, 4, n_users).astype(np.float32)
    items = datasets.Features(torch.from_numpy(np.stack([genre, price], 1)), ["genre", "price"])
    users = datasets.Features(torch.from_numpy(age[:, None]), ["age"])
    um = feature_csr(users, categorical=("age",))
    im = feature_csr(items, categorical=("genre",), numeric=("price",))
    torch.manual_seed(seed)
    model = FeatureMatrixFactorization(um, im, d).to(DEV)
    pieces = {}
    for name, m, W in (("u", um, model.user_feature_embeddings), ("i", im, model.item_feature_embeddings)):
        csr = (m.rowptr.numpy(), m.cols.numpy(), m.weights.numpy())
        W64 = W.weight.detach().cpu().numpy().astype(np.float64)
        S = fc.dense(*csr, m.n_features)
        pieces[name] = dict(S=S, W=W64, T=S @ W64, mag=np.abs(S) @ np.abs(W64),
                            n=int(np.diff(csr[0]).max()))
    return model, im, pieces


def test_model_forward_against_float64():
    model, _, p = _hybrid()
    rng = np.random.default_rng(1)
    uid, iid = rng.integers(0, 60, 500), rng.integers(0, 90, 500)
    with torch.no_grad():
        got = model(torch.from_numpy(uid), torch.from_numpy(iid)).cpu().numpy()
    fc.check_row_sum(model.compose_items().detach().cpu().numpy(),
                     (p["i"]["T"], p["i"]["mag"], np.full(90, p["i"]["n"])), what="compose_items")
    ref = np.sum(p["u"]["T"][uid] * p["i"]["T"][iid], axis=1)
    # a d-term fp32 dot of two composed rows: the dot's own (d + 8) u sum|u i|
    # (pairwise_checks' margin) plus each side's composition error through the product
    mag = np.sum(p["u"]["mag"][uid] * p["i"]["mag"][iid], axis=1)
    tol = (32 + 8 + 2 * (max(p["u"]["n"], p["i"]["n"]) + 8)) * fc.U24 * mag
    print(f"forward: max abs err {np.abs(got - ref).max():.3g}, largest share of the bound "
          f"{(np.abs(got - ref) / tol).max():.3g}")
    assert np.all(np.abs(got - ref) <= tol)
    with pytest.raises(IndexError):
        model(torch.tensor([60]), torch.tensor([0]))


def test_model_gradients_against_float64():
    model, _, p = _hybrid()
    rng = np.random.default_rng(2)
    B = 512
    uid, iid = rng.integers(0, 60, B), rng.integers(0, 90, B)
    model(torch.from_numpy(uid), torch.from_numpy(iid)).sum().backward()
    for side, other, ids, oids, W in (("u", "i", uid, iid, model.user_feature_embeddings.weight),
                                      ("i", "u", iid, uid, model.item_feature_embeddings.weight)):
        g, gmag = np.zeros_like(p[side]["T"]), np.zeros_like(p[side]["T"])
        np.add.at(g, ids, p[other]["T"][oids])
        np.add.at(gmag, ids, p[other]["mag"][oids])
        ref = p[side]["S"].T @ g
        # every element is a sum of at most B composed rows, each composed from
        # at most n entries, gathered over a transposed row: no rounding path is
        # deeper than B + the longest transposed row + n, plus slack
        depth = B + int((p[side]["S"] != 0).sum(0).max()) + p[other]["n"] + 16
        tol = depth * fc.U24 * (np.abs(p[side]["S"]).T @ gmag)
        err = np.abs(W.grad.cpu().numpy() - ref)
        print(f"grad {side}: max abs err {err.max():.3g}, largest share of the bound "
              f"{np.nanmax(np.where(tol > 0, err / np.where(tol > 0, tol, 1), 0)):.3g}")
        assert np.all(err <= tol)


def _identity_pair(d, n_users=300, n_items=2000, seed=0):
    torch.manual_seed(seed)
    mf = models.MatrixFactorization(n_users, n_items, d).to(DEV)
    fm = FeatureMatrixFactorization(feature_csr(n_users), feature_csr(n_items), d).to(DEV)
    fm.load_state_dict({"user_feature_embeddings.weight": mf.user_embeddings.weight.detach(),
                        "item_feature_embeddings.weight": mf.item_embeddings.weight.detach()})
    return mf, fm


@pytest.mark.parametrize("d", [100, 128])
def test_identity_maps_are_matrix_factorization(d):
    """With identity maps the composed tables are the parameters, bit for bit:
    identical score_topk items and scores at both precisions and identical
    recommend_diverse picks."""
    mf, fm = _identity_pair(d)
    assert torch.equal(fm.compose_items().detach(), mf.item_embeddings.weight.detach())
    for precision in ("fp32", "bf16"):
        a, b = mf.score_topk(10, precision=precision), fm.score_topk(10, precision=precision)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    users = torch.arange(0, 300, 7)
    for method in ("dpp", "mmr"):
        a = mf.recommend_diverse(10, 50, method=method, user_ids=users)
        b = fm.recommend_diverse(10, 50, method=method, user_ids=users)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


class _Batches:
    """A PairWiseDataset stand-in over fixed host triples, in order."""

    def __init__(self, triples):
        self.triples = tuple(torch.from_numpy(t) for t in triples)

    def loader(self, batch_size, **_):
        for b in range(0, len(self.triples[0]), batch_size):
            u, p, n = (t[b:b + batch_size] for t in self.triples)
            yield u, p, n, None, None, None


def test_identity_maps_training_step_is_matrix_factorizations():
    """One pair_wise_train_loop batch (fused step, plain Adam) on identity
    maps against MatrixFactorization's step and the float64 step. Tolerance:
    pairwise_checks' own for that step: adam_ref's bounds for the Adam kernel
    given a gradient, plus what its BPR gradient tolerance (rtol 1e-4, atol
    1e-7: the composed gradients still come from the atomic kernel) lets
    through the first Adam step (feature_checks.adam_first_step_tolerance).
    Rows the batch does not touch have gradient exactly 0 and must not move."""
    d, lr, B = 100, 1e-2, 2048
    mf, fm = _identity_pair(d, 260, 400, seed=4)
    U0, I0, uid, pid, nid = pc.bpr_case(d, B=B, nu=260, ni=400, seed=77)
    uid, pid, nid = uid % 200, pid % 300, nid % 300  # the last rows of both tables: never touched
    with torch.no_grad():
        for m, names in ((mf, ("user_embeddings", "item_embeddings")),
                         (fm, ("user_feature_embeddings", "item_feature_embeddings"))):
            getattr(m, names[0]).weight.copy_(dev(U0)), getattr(m, names[1]).weight.copy_(dev(I0))
    loss = losses.LogSigmoidDifferenceLoss()
    out = []
    for m in (mf, fm):
        opt = torch.optim.Adam(m.parameters(), lr=lr)
        out.append(train.pair_wise_train_loop(_Batches((uid, pid, nid)), m, loss, opt,
                                              scores=[metrics.AUCScore()], batch_size=B))
    assert out[1][0] == pytest.approx(out[0][0], rel=1e-6) and out[1][1] == out[0][1]
    _, _, _, gU, gI, _ = pc.bpr_step_f64(U0, I0, uid, pid, nid, 1.0 / B)
    for p0, g64, a, b, ids in (
            (U0, gU, mf.user_embeddings.weight, fm.user_feature_embeddings.weight, uid),
            (I0, gI, mf.item_embeddings.weight, fm.item_feature_embeddings.weight,
             np.concatenate([pid, nid]))):
        zero = np.zeros_like(p0)
        ref = pc.adam_ref(p0, g64.astype(np.float32), zero, zero, 1, lr=lr)
        tol = ref[4] + fc.adam_first_step_tolerance(g64, lr)
        a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
        for name, got in (("MatrixFactorization", a), ("FeatureMatrixFactorization", b)):
            err = np.abs(got.astype(np.float64) - ref[0])
            print(f"{name}: max abs err {err.max():.3g}, largest share of the bound "
                  f"{(err / tol).max():.3g}")
            assert np.all(err <= tol), name
        assert np.all(np.abs(a.astype(np.float64) - b) <= 2 * tol)
        untouched = np.setdiff1d(np.arange(len(p0)), ids)
        assert len(untouched) and np.array_equal(b[untouched], p0[untouched])


def test_cold_start_items_through_saved_offsets():
    """Items the model has never seen, known by genre and price only:
    score_topk(item_vectors=compose_items(new map)) against a float64 scan of
    the float64-composed rows, gap-aware (tests/topk_checks.py)."""
    model, im, p = _hybrid(d=32)
    rng = np.random.default_rng(8)
    n_new = 400
    new = datasets.Features(torch.from_numpy(np.stack(
        [rng.integers(0, 9, n_new).astype(np.float32),  # genres 7 and 8 were never seen
         rng.uniform(-1, 1, n_new).astype(np.float32)], 1)), ["genre", "price"])
    new_map = feature_csr(new, offsets=im.offsets)
    assert new_map.n_features == im.n_features and int(new_map.cols.min()) >= 90
    rows = model.compose_items(new_map).detach()
    assert rows.shape == (n_new, 32)
    S = fc.dense(new_map.rowptr.numpy(), new_map.cols.numpy(), new_map.weights.numpy(),
                 im.n_features)
    I64, Imag = S @ p["i"]["W"], np.abs(S) @ np.abs(p["i"]["W"])
    fc.check_row_sum(rows.cpu().numpy(), (I64, Imag, np.full(n_new, 2)), what="new rows")
    items, scores = model.score_topk(10, item_vectors=rows)
    U64 = p["u"]["T"]
    ref = np.argsort(-(U64 @ I64.T), axis=1, kind="stable")[:, :10]
    # the scan's fp32 dot (FP32_REL) plus both sides' composition error through the product
    tol = (FP32_REL + 2 * (p["u"]["n"] + 8) * fc.U24) * (p["u"]["mag"] @ Imag.T).max(axis=1)
    differ = gap_check(items.cpu().numpy(), ref, U64, I64, None, tol)
    print(f"cold start: {differ} of 60 lists differ from the float64 order, all inside the gap")
    got_s = np.take_along_axis(U64 @ I64.T, items.cpu().numpy(), 1)
    assert np.all(np.abs(scores.cpu().numpy() - got_s) <= tol[:, None])
    picks, _ = model.recommend_diverse(5, 20, method="mmr", item_vectors=rows)
    assert picks.shape == (60, 5) and int(picks.max()) < n_new and int(picks.min()) >= 0
    with pytest.raises(ValueError, match="item_vectors"):
        model.score_topk(10, item_vectors=rows[:, :16])


def test_recommendation_doors_take_the_one_launch_path():
    """get_model_recommendations with the new model: score_topk's lists under
    the dataset's exclusions, and the model's forward (the per-user loop's
    scorer) is never entered; get_diverse_recommendations and
    recommendations_score_loop accept it too."""
    model, _, _ = _hybrid()
    rng = np.random.default_rng(3)
    pairs = np.unique(np.stack([rng.integers(0, 60, 900), rng.integers(0, 90, 900)], 1), axis=0)
    tr, te = torch.from_numpy(pairs[::2]), torch.from_numpy(pairs[1::2])
    mk = lambda x: datasets.UserItemInteractionsDataset(x, number_of_users=60, number_of_items=90)
    ds = datasets.RankingDataset(mk(te), frozen=mk(tr))
    calls = []
    model.register_forward_hook(lambda *a: calls.append(1))  # the per-user loop calls model(...)
    with torch.no_grad():
        model(torch.tensor([0]), torch.tensor([0]))
    assert calls == [1]  # the counter sees a forward
    calls.clear()
    recs = train.get_model_recommendations(ds, model, 10)
    assert not calls and recs.shape == (60, 10) and recs.device.type == "cpu"
    excl = ds.exclusion_csr()
    want, _ = model.score_topk(10, exclude=excl)
    assert torch.equal(recs, want.cpu())
    rowptr, cols = (t.numpy() for t in excl)
    for u in range(60):
        assert not set(recs[u].tolist()) & set(cols[rowptr[u]:rowptr[u + 1]].tolist())
    div = train.get_diverse_recommendations(ds, model, 5, 30, method="mmr")
    assert div.shape == (60, 5) and not calls
    p_at_k, = train.recommendations_score_loop(ds, model, [metrics.PrecisionAtKScore()], 10)
    assert 0.0 <= float(p_at_k) <= 1.0 and not calls


def test_training_descends_on_the_planted_data():
    """Three epochs of pair_wise_train_loop (the fused feature step + fused
    Adam) over genre features lower the epoch-mean loss each time, as the
    float64 restatement does (tests/test_feature_host.py)."""
    pairs, genre = fc.planted()
    items = datasets.Features(torch.from_numpy(genre.astype(np.float32)[:, None]), ["genre"])
    torch.manual_seed(0)
    model = FeatureMatrixFactorization(feature_csr(200), feature_csr(items, categorical=("genre",)),
                                       32).to(DEV)
    with torch.no_grad():
        for prm in model.parameters():
            prm.mul_(0.1)
    assert model.item_feature_embeddings.weight.shape == (300 + 12, 32)
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    ds = _Batches(fc.planted_triples(pairs, 300))
    hist = [train.pair_wise_train_loop(ds, model, losses.LogSigmoidDifferenceLoss(), opt,
                                       scores=[metrics.AUCScore()], batch_size=1024)
            for _ in range(3)]
    print("epoch-mean BPR losses:", [h[0] for h in hist], "AUC:", [h[1][0] for h in hist])
    assert hist[0][0] > hist[1][0] > hist[2][0]
    assert hist[2][1][0] > hist[0][1][0]
    # the generic path (another loss: forward + autograd, optimizer.step) trains it too
    before = model.item_feature_embeddings.weight.detach().clone()
    pw = _Batches(tuple(t[:512] for t in fc.planted_triples(pairs, 300)))

    class Hinge(losses.PairWiseLoss):
        def pair_wise(self, positives, negatives):
            return torch.relu(1.0 - (positives - negatives))

    train.pair_wise_train_loop(pw, model, Hinge(), opt, batch_size=512)
    assert not torch.equal(before, model.item_feature_embeddings.weight.detach())
