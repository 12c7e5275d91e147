"""dr_history_distance, dr_serendipity_rerank and dr_list_item_mean on the GPU
(through ops) against tests/serendipity_checks.py: every distance within
(d + 16) * 2^-23 of the float64 restatement, MIN bit for bit the fp32
emulation on integer-valued tables, every pick exactly the stable descending
order of the fp32 blend of the kernel's own distances; then the metrics and
the doors end to end on a 60-user, 300-item dataset."""
import functools

import numpy as np
import pytest
import torch

import serendipity_checks as sc
from divrec import _backend, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_ITEMS = 700
SIZES = (1, 31, 32, 33, 100, 128, 129, 1000, 1024)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(C, d, integer=True):
    return sc.make_case(100 + C + d, C, d, n_items=N_ITEMS, integer=integer)


def _table(table):
    return _dev(table).to(torch.bfloat16)


def _distance(case, reduce, lists=None, hist=None, **kw):
    lists_, _, table, rowptr, hist_ = case
    lists = lists_ if lists is None else lists
    hist = hist_ if hist is None else hist
    out = ops.history_distance(_dev(lists), _table(table), _dev(rowptr), _dev(hist), reduce, **kw)
    assert out.dtype == torch.float32 and out.shape == lists.shape
    return out.cpu().numpy()


def _check(case, reduce, out):
    lists, _, table, rowptr, hist = case
    worst = sc.check_distance(out, lists, table, rowptr, hist, reduce)
    print(f"max |out - f64| = {worst:.3e} (bound {sc.distance_bound(table.shape[1]):.3e})")
    if reduce == sc.MIN:  # integer-valued rows: every Gram element is exact
        emu = sc.emulate_distance(lists, table, rowptr, hist, reduce)
        assert np.array_equal(out.view(np.uint32), emu.view(np.uint32))
    with_hist = np.diff(rowptr) > 0
    # position 0 is an item of the user's own history: distance 0 within the bound
    if reduce == sc.MIN:
        assert (np.abs(out[with_hist, 0]) <= sc.distance_bound(table.shape[1])).all()
    if lists.shape[1] > 4:  # position 2 is a zero-norm row: distance 1 from everything
        assert (out[with_hist, 2] == 1).all()
    assert not out[~with_hist].any()


@pytest.mark.parametrize("reduce", [sc.MIN, sc.MEAN])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("C", SIZES)
def test_distance(C, d, reduce):
    case = _case(C, d)
    _check(case, reduce, _distance(case, reduce))


@pytest.mark.parametrize("reduce", [sc.MIN, sc.MEAN])
@pytest.mark.parametrize("C,d", [(100, 32), (129, 32), (100, 256), (1000, 256)])
def test_distance_other_widths(C, d, reduce):
    case = _case(C, d)
    _check(case, reduce, _distance(case, reduce))


@pytest.mark.parametrize("reduce", [sc.MIN, sc.MEAN])
@pytest.mark.parametrize("C", [100, 1000])
def test_distance_real_valued_rows(C, reduce):
    case = _case(C, 128, integer=False)
    lists, _, table, rowptr, hist = case
    out = _distance(case, reduce)
    print("max |out - f64| =", sc.check_distance(out, lists, table, rowptr, hist, reduce))


@pytest.mark.parametrize("reduce", [sc.MIN, sc.MEAN])
@pytest.mark.parametrize("C", [100, 1000])
def test_one_workgroup_loops_over_all_users(C, reduce):
    case = _case(C, 128)
    plain = _distance(case, reduce)
    with _backend.plan_knobs(scan_slots=1):
        one = _distance(case, reduce)
    _check(case, reduce, one)
    assert np.array_equal(one.view(np.uint32), plain.view(np.uint32))  # and run to run
    assert np.array_equal(_distance(case, reduce).view(np.uint32), plain.view(np.uint32))


@pytest.mark.parametrize("reduce", [sc.MIN, sc.MEAN])
@pytest.mark.parametrize("C", [100, 200])
def test_special_ids(C, reduce):
    lists, scores, table, rowptr, hist = _case(C, 64)
    lists, hist = lists.copy(), hist.copy()
    lists[:, 7] = -1
    lists[5, 9], lists[6, 11] = N_ITEMS, 2 ** 31 - 1
    hist[rowptr[4]:rowptr[4] + 10] = N_ITEMS + 3  # ten of user 4's 33 entries
    hist[rowptr[4] + 10] = -2
    hist[rowptr[2]:rowptr[3]] = N_ITEMS  # user 2's whole history (31 entries)
    case = (lists, scores, table, rowptr, hist)
    err = _backend.error_counter(torch.device(DEV))
    out = _distance(case, reduce, err=err)
    sc.check_distance(out, lists, table, rowptr, hist, reduce)
    assert np.isnan(out[5, 9]) and np.isnan(out[6, 11]) and not out[:, 7].any()
    assert not out[2].any()
    assert int(err.item()) == 2 + 11 + 31
    with pytest.raises(IndexError):
        _distance(case, reduce)
    # the re-rank: never picked, counted the same
    err = _backend.error_counter(torch.device(DEV))
    items, dist = ops.serendipity_rerank(_dev(lists), _dev(scores), _table(table), _dev(rowptr),
                                         _dev(hist), C, 0.5, reduce, err=err)
    items = items.cpu().numpy()
    assert int(err.item()) == 2 + 11 + 31
    assert (items[:, -1] == -1).all() and items[5, -2] == -1 and items[0, -2] >= 0
    assert items.max() < N_ITEMS
    dfull = np.nan_to_num(out)
    sc.check_rerank(items, dist.cpu().numpy(), lists, scores, dfull, N_ITEMS, 0.5, C)


@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("C,d,reduce", [(1, 64, sc.MIN), (33, 64, sc.MEAN), (100, 128, sc.MIN),
                                        (128, 128, sc.MEAN), (129, 64, sc.MIN),
                                        (1000, 128, sc.MIN), (1024, 128, sc.MEAN),
                                        (200, 32, sc.MIN), (200, 256, sc.MEAN)])
def test_rerank(C, d, reduce, lam):
    case = _case(C, d)
    lists, scores, table, rowptr, hist = case
    dfull = _distance(case, reduce)
    sc.check_distance(dfull, lists, table, rowptr, hist, reduce)
    args = (_dev(lists), _dev(scores), _table(table), _dev(rowptr), _dev(hist))
    for k_out in sorted({1, min(100, C), C}):
        items, dist = ops.serendipity_rerank(*args, k_out, lam, reduce)
        items, dist = items.cpu().numpy(), dist.cpu().numpy()
        sc.check_rerank(items, dist, lists, scores, dfull, N_ITEMS, lam, k_out)
        if lam == 1.0:  # the stable order by score
            order = np.argsort(-scores.astype(np.float64), axis=1, kind="stable")[:, :k_out]
            assert np.array_equal(items, np.take_along_axis(lists, order, 1))
    with _backend.plan_knobs(scan_slots=1):
        one, _ = ops.serendipity_rerank(*args, min(100, C), lam, reduce)
    want, _ = ops.serendipity_rerank(*args, min(100, C), lam, reduce)
    assert torch.equal(one, want)


def test_rerank_fewer_live_candidates_than_picks():
    lists, scores, table, rowptr, hist = _case(200, 64)
    lists = lists.copy()
    lists[:, 5:] = -1
    items, dist = ops.serendipity_rerank(_dev(lists), _dev(scores), _table(table), _dev(rowptr),
                                         _dev(hist), 100, 0.5, sc.MIN)
    items, dist = items.cpu().numpy(), dist.cpu().numpy()
    assert (items[:, 5:] == -1).all() and not dist[:, 5:].any() and (items[:, :5] >= 0).all()
    dfull = _distance((lists, scores, table, rowptr, hist), sc.MIN)
    sc.check_rerank(items, dist, lists, scores, dfull, N_ITEMS, 0.5, 100)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_list_item_mean(dtype):
    rng = np.random.default_rng(5)
    values = rng.random(300).astype(np.float32)
    recs = rng.integers(0, 300, (1000, 37))
    recs[rng.random(recs.shape) < 0.1] = -1
    recs[3], recs[4, 2], recs[9, 0] = -1, 300, 10 ** 6
    err = _backend.error_counter(torch.device(DEV))
    out = ops.list_item_mean(_dev(recs).to(dtype), _dev(values), err=err).cpu().numpy()
    ref = sc.reference_list_item_mean(recs, values)
    assert int(err.item()) == 2 and out[3] == 0
    assert np.abs(out - ref).max() <= 37 * 2.0 ** -24  # <= 37 fp32 adds of values in [0, 1)
    with pytest.raises(IndexError):
        ops.list_item_mean(_dev(recs).to(dtype), _dev(values))


def test_duplicate_history_entries():
    """A planted duplicate: MEAN counts the entry twice, MIN does not change."""
    lists, scores, table, rowptr, hist = _case(100, 64)
    hist = hist.copy()
    users = [u for u in range(len(rowptr) - 1) if rowptr[u + 1] - rowptr[u] >= 31]
    for u in users:
        hist[rowptr[u] + 2] = hist[rowptr[u] + 3]
    case = (lists, scores, table, rowptr, hist)
    for reduce in (sc.MIN, sc.MEAN):
        out = _distance(case, reduce)
        sc.check_distance(out, lists, table, rowptr, hist, reduce)
    # user 2 (31 entries): the mean over the multiset differs from the mean over the set
    u = users[0]
    E = table.astype(np.float64)
    nrm = np.sqrt((E * E).sum(1))
    unit = E / np.where(nrm > 0, nrm, 1)[:, None]
    row = hist[rowptr[u]:rowptr[u + 1]]
    multi = (1 - unit[lists[u]] @ unit[row].T).mean(1)
    once = (1 - unit[lists[u]] @ unit[np.unique(row)].T).mean(1)
    assert np.abs(multi - once).max() > 1e-3
    assert np.abs(out[u] - multi).max() <= sc.distance_bound(64)


# --------------------------------------------------------------------------- metrics and doors
N_U, N_I, DIM, K, CANDS = 60, 300, 24, 10, 50


@pytest.fixture(scope="module")
def door():
    from divrec import datasets, models
    rng = np.random.default_rng(23)
    mf = models.MatrixFactorization(N_U, N_I, DIM)
    with torch.no_grad():
        mf.user_embeddings.weight.copy_(torch.from_numpy(rng.standard_normal((N_U, DIM)) * 0.3))
        mf.item_embeddings.weight.copy_(torch.from_numpy(rng.standard_normal((N_I, DIM))))
    mf = mf.to(DEV)
    # user 0 has no history; the others 8 distinct items, popular items more often
    frozen = np.array([[u, i] for u in range(1, N_U)
                       for i in rng.choice(N_I // 3, 8, replace=False)])
    test = np.array([[u, i] for u in range(N_U) for i in rng.choice(N_I, 30, replace=False)])
    data = datasets.UserItemInteractionsDataset(torch.from_numpy(test), number_of_users=N_U,
                                                number_of_items=N_I)
    history = datasets.UserItemInteractionsDataset(torch.from_numpy(frozen), number_of_users=N_U,
                                                   number_of_items=N_I)
    rds = datasets.RankingDataset(data, frozen=history)
    table = mf.item_embeddings.weight.detach().to(torch.bfloat16).float().cpu().numpy()
    rowptr, items = (t.numpy() for t in rds.exclusion_csr())
    return mf, rds, history, table, rowptr, items, test, frozen


def test_scores_against_the_restatement(door):
    from divrec import metrics, train
    mf, rds, history, table, rowptr, hist, test, frozen = door
    top = train.get_model_recommendations(rds, mf, K)
    lists = top.numpy()
    for reduce in (sc.MIN, sc.MEAN):
        ref = sc.reference_distance(lists, table, rowptr, hist, reduce)
        kw = dict(dataset=rds.data, history=history, reduce=reduce, reduction="none")
        unexp = metrics.UnexpectednessScore(model=mf, **kw)
        seren = metrics.SerendipityScore(item_table=mf.item_embeddings.weight.detach().cpu(), **kw)
        got_u, got_s = train.recommendations_score_loop(rds, mf, [unexp, seren], K)
        assert got_u.shape == got_s.shape == (N_U,) and got_u.device.type == "cpu"
        # + the fp32 mean over K positions: K adds of partial sums below 2 K < 32
        # (half an ulp 2^-20 each), divided by K, and the divide's rounding
        bound = sc.distance_bound(DIM) + 2.0 ** -20 + 2.0 ** -23
        assert np.abs(got_u.numpy() - ref.mean(1)).max() <= bound
        assert got_u[0] == 0 and got_u[1:].min() > 0  # user 0 has no history
        pairs = set(map(tuple, test.tolist()))
        hit = np.array([[(u, int(i)) in pairs for i in lists[u]] for u in range(N_U)])
        assert hit.any() and not hit.all()
        assert np.abs(got_s.numpy() - (ref * hit).mean(1)).max() <= bound
        assert unexp._dev_table is not None and unexp._dev_table.shape == (N_I, 32)
        unexp.refresh()
        assert unexp._dev_table is None and unexp._dev_csr is None
        mean = metrics.UnexpectednessScore(model=mf, dataset=rds.data, history=history,
                                           reduce=reduce)
        assert abs(float(mean(None, top)) - ref.mean()) <= bound
    pop = np.bincount(np.unique(frozen, axis=0)[:, 1], minlength=N_I).astype(np.float64)
    values = {"self_information": -np.log2(np.maximum(pop, 1) / N_U),
              "popularity_complement": 1 - pop / pop.max()}
    for kind, val in values.items():
        nov = metrics.NoveltyScore(dataset=rds.data, history=history, kind=kind, reduction="none")
        got = nov(None, top).numpy()
        want = sc.reference_list_item_mean(lists, val)
        assert np.abs(got - want).max() <= (K + 2) * 2.0 ** -24 * val.max()
        assert torch.equal(nov.item_values(torch.device(DEV, 0)).cpu(),
                           metrics.novelty_item_values(torch.from_numpy(pop), N_U, kind))


def test_get_serendipitous_recommendations(door):
    from divrec import metrics, train
    mf, rds, history, table, rowptr, hist, _, _ = door
    excl = rds.exclusion_csr()
    cand, cand_sc = mf.score_topk(CANDS, exclude=excl)
    cand_np, sc_np = cand.to(torch.int32).cpu().numpy(), cand_sc.cpu().numpy()
    for reduce in (sc.MIN, sc.MEAN):
        rows = mf.item_embeddings.weight.detach().to(torch.bfloat16)
        dfull = ops.history_distance(cand.to(torch.int32), rows, excl[0].to(DEV), excl[1].to(DEV),
                                     reduce).cpu().numpy()
        sc.check_distance(dfull, cand_np, table, rowptr, hist, reduce)
        got = train.get_serendipitous_recommendations(rds, mf, K, CANDS, lam=0.5, reduce=reduce)
        assert got.dtype == torch.int64 and got.device.type == "cpu" and got.shape == (N_U, K)
        sc.check_rerank(got.numpy(), None, cand_np, sc_np, dfull, N_I, 0.5, K)
        items, dist = mf.recommend_serendipitous(K, CANDS, excl, lam=0.5, reduce=reduce,
                                                 exclude=excl)
        assert torch.equal(items.cpu(), got)
        sc.check_rerank(items.cpu().numpy(), dist.cpu().numpy(), cand_np, sc_np, dfull, N_I, 0.5, K)
        plain = train.get_serendipitous_recommendations(rds, mf, K, CANDS, lam=1.0, reduce=reduce)
        top = train.get_model_recommendations(rds, mf, K)
        assert torch.equal(plain, top)
        score = metrics.UnexpectednessScore(model=mf, dataset=rds.data, history=history,
                                            reduce=reduce)
        re_ranked, top_k = float(score(None, got)), float(score(None, top))
        print(f"mean unexpectedness ({reduce}): top-k {top_k:.4f}, lam = 0.5 {re_ranked:.4f}")
        assert re_ranked >= top_k
