"""dr_xquad_rerank, dr_aspect_profile and dr_aspect_coverage on the GPU (ops, the
model and train doors, metrics.AspectCoverageScore) against the float64 replay
of tests/xquad_checks.py: every step of every list a valid greedy step within
2 TOL_V, every out_cov within TOL_COV (both derived there), and the exact
properties of the spec: ties to the lowest position, lam = 1, a zero profile
and a zero matrix the stable score order, lists that end in -1 when no live
candidate is left."""
import numpy as np
import pytest
import torch

import xquad_checks as xc
from divrec import _backend, datasets, metrics, models, ops, train

pytestmark = pytest.mark.gpu

DEV = "cuda"
U24 = 2.0 ** -24


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _run(case, check=True, err=None):
    items, cov = ops.xquad_rerank(_dev(case.cand), _dev(case.sc), _dev(case.aspects),
                                  _dev(case.profile), case.k, case.lam, err=err, check=check)
    assert items.dtype == torch.int32 and cov.dtype == torch.float32
    assert items.shape == cov.shape == (case.n, case.k)
    # the finished list's coverage is the metric of that list
    metric = ops.aspect_coverage(items, _dev(case.aspects), _dev(case.profile))
    assert float((metric - cov[:, -1]).abs().max()) <= xc.TOL_COV
    return items.cpu().numpy(), cov.cpu().numpy()


@pytest.mark.parametrize("lam", xc.BASIC_LAMS)
def test_rerank_basic(lam):
    case = xc.basic_input(lam)
    got, cov = _run(case)
    assert xc.replay(got, cov, case) == 0
    if lam == 1.0:
        assert np.array_equal(got, xc.stable_topk(case))


@pytest.mark.parametrize("C,k,G", xc.SHAPES)
def test_rerank_shapes(C, k, G):
    case = xc.shape_input(C, k, G)
    got, cov = _run(case)
    assert xc.replay(got, cov, case) == 0
    if k == C:  # every candidate is picked once
        assert np.array_equal(np.sort(got, axis=1), np.sort(case.cand, axis=1))


def test_rerank_ties():
    case, pos, _ = xc.reference(xc.tie_input)
    got, cov = _run(case)
    assert np.array_equal(got, xc.items_at(case, pos))
    assert xc.replay(got, cov, case) == 0


def test_rerank_profiles():
    case, pos, _ = xc.reference(xc.profile_input)
    got, cov = _run(case)
    assert xc.replay(got, cov, case) == 0
    assert np.array_equal(got[0], xc.stable_topk(case)[0]) and (cov[0] == 0).all()  # zero profile
    # rows 4 (x 8) and 6 (/ 16) are row 3 up to an exact scale, row 5 holds a NaN
    # and a negative weight where row 3 holds 0: identical picks and values
    for u in (4, 5, 6):
        assert np.array_equal(got[u], got[3]) and np.array_equal(cov[u], cov[3])
    assert np.array_equal(got, xc.items_at(case, pos))
    assert (np.diff(cov, axis=1) >= 0).all() and (cov >= 0).all() and (cov <= 1 + xc.TOL_COV).all()
    # the one-hot row is covered by the first item of its aspect, binary: exactly 1 from there on
    assert cov[1, -1] == 1.0


def test_rerank_score_order_special_cases():
    """lam = 1, a zero profile and a zero matrix give the stable score order exactly."""
    base = xc.shape_input(257, 40, 19)
    base.sc[:, 100] = base.sc[:, 7]  # exact ties, broken by position
    for lam, aspects, profile in ((1.0, base.aspects, base.profile),
                                  (0.5, base.aspects, np.zeros_like(base.profile)),
                                  (0.5, np.zeros_like(base.aspects), base.profile),
                                  (0.0, np.zeros_like(base.aspects), base.profile)):
        case = xc.Case(base.cand, base.sc, aspects, profile, base.k, lam)
        got, cov = _run(case)
        want = xc.stable_topk(case) if lam > 0 else case.cand[:, :case.k]  # lam = 0: all values 0
        assert np.array_equal(got, want)
        if lam != 1.0:
            assert (cov == 0).all()


def test_rerank_aspect_values_behave_as_clamped():
    raw, clamped = xc.aspect_value_input(), xc.aspect_value_input(clamped=True)
    got, cov = _run(raw)
    got2, cov2 = _run(clamped)
    assert np.array_equal(got, got2) and np.array_equal(cov, cov2)
    assert xc.replay(got, cov, raw) == 0 and np.isfinite(cov).all()


def test_rerank_invalid_input():
    case, pos, _ = xc.reference(xc.invalid_input)
    with pytest.raises(IndexError, match=f"{xc.INVALID_ERR} entries"):
        _run(case)
    got, cov = _run(case, check=False)
    assert xc.replay(got, cov, case) == 0
    mine = torch.zeros(1, dtype=torch.int32, device=DEV)
    again, _ = _run(case, err=mine)  # the caller's counter: no raise
    assert int(mine.item()) == xc.INVALID_ERR and np.array_equal(again, got)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.empty((case.n, case.k), dtype=torch.int32, device=DEV)
    c, s, prof, asp = _dev(case.cand), _dev(case.sc), _dev(case.profile), _dev(case.aspects)
    rc = _backend.lib().dr_xquad_rerank(
        c.data_ptr(), s.data_ptr(), case.n, case.C, asp.data_ptr(), asp.size(0), case.G,
        prof.data_ptr(), case.k, case.lam, out.data_ptr(), None, err.data_ptr(),
        _backend.stream(torch.device(DEV, torch.cuda.current_device())))
    assert rc == 0 and int(err.item()) == xc.INVALID_ERR == xc.live_and_rows(case)[2]
    assert np.array_equal(out.cpu().numpy(), got)  # out_cov = NULL changes no pick
    live, _, _ = xc.live_and_rows(case)
    for u in range(case.n):
        dead = set(case.cand[u][~live[u]].tolist()) - {-1}
        assert not dead & set(got[u].tolist())
        n_live = int(live[u].sum())
        assert (got[u, :min(n_live, case.k)] >= 0).all() and (got[u, n_live:] == -1).all()
    assert (cov[4, 20:] == cov[4, 19]).all()  # the list ended: the coverage of the list as it stands
    assert (got[5] == -1).all() and (cov[5] == 0).all()
    # a NaN and a -inf score count as -FLT_MAX: the float64 greedy leaves them out of 30 picks
    assert not {int(case.cand[3, 5]), int(case.cand[3, 17])} & set(got[3].tolist())
    assert pos[3].min() >= 0


def test_rerank_many_users_per_workgroup():
    case, _, _ = xc.reference(xc.many_users_input)
    got, cov = _run(case)
    with _backend.plan_knobs(scan_slots=2):  # hundreds of users per workgroup
        got2, cov2 = _run(case)
    assert np.array_equal(got, got2) and np.array_equal(cov, cov2)
    assert xc.replay(got2, cov2, case) == 0  # every user


def test_rerank_empty_and_bad_arguments():
    case = xc.shape_input(63, 63, 2)
    c, s, asp, prof = _dev(case.cand), _dev(case.sc), _dev(case.aspects), _dev(case.profile)
    items, cov = ops.xquad_rerank(c[:0], s[:0], asp, prof[:0], 10, 0.5)
    assert items.shape == cov.shape == (0, 10)
    with pytest.raises(ValueError):
        ops.xquad_rerank(c, s, asp, prof[:3], 10, 0.5)
    with pytest.raises(ValueError):
        ops.xquad_rerank(c, s, asp.to(torch.float64), prof, 10, 0.5)
    with pytest.raises(ValueError):
        ops.xquad_rerank(c, s, torch.ones((5000, 65), device=DEV),
                         torch.ones((case.n, 65), device=DEV), 10, 0.5)
    with pytest.raises(ValueError):
        ops.xquad_rerank(c, s, asp, torch.ones((case.n, 3), device=DEV), 10, 0.5)
    with pytest.raises(RuntimeError, match="k_out"):
        ops.xquad_rerank(c, s, asp, prof, 64, 0.5)
    with pytest.raises(RuntimeError, match="lambda"):
        ops.xquad_rerank(c, s, asp, prof, 10, 1.5)
    wide = torch.zeros((2, 1024), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r"C \* G must be <= 32768"):
        ops.xquad_rerank(wide, wide.float(), torch.ones((5000, 33), device=DEV),
                         torch.ones((2, 33), device=DEV), 10, 0.5)


# --------------------------------------------------------------------------- aspect_profile
ROW_LENGTHS = [0, 1, 63, 64, 65, 200]


def _history(rng, lengths, ni):
    rows = [rng.integers(0, ni, m) for m in lengths]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rowptr, np.concatenate(rows).astype(np.int32), rows


def _profile_f64(A, row):
    s = xc.clamp(A)[row].astype(np.float64).sum(axis=0)
    return s / s.sum() if s.sum() > 0 else np.zeros(A.shape[1])


@pytest.mark.parametrize("fractional", [False, True])
def test_aspect_profile(fractional):
    rng = np.random.default_rng(281 + fractional)
    G, ni = 19, 5000
    A = xc.multi_hot(rng, ni, G, fractional=fractional)
    A[:50] = 0
    rowptr, items, rows = _history(rng, ROW_LENGTHS + [7], ni)
    rows[-1][:] = rng.integers(0, 50, 7)  # a row of all-zero items
    items[rowptr[-2]:] = rows[-1]
    got = ops.aspect_profile(_dev(rowptr), _dev(items), _dev(A)).cpu().numpy()
    assert got.shape == (len(rows), G) and got.dtype == np.float32
    for r, row in enumerate(rows):
        want = _profile_f64(A, row)
        # L rounded adds in the numerator, the same in the denominator, one divide; values <= 1
        assert np.abs(got[r] - want).max() <= (2 * len(row) + 1) * U24, r
        if not fractional:  # exact integers and one fp32 divide
            cnt = A[row].sum(axis=0, dtype=np.float32)
            exact = cnt / cnt.sum(dtype=np.float32) if cnt.sum() else np.zeros(G, np.float32)
            assert np.array_equal(got[r].view(np.uint32), exact.view(np.uint32)), r
    assert not got[0].any() and not got[-1].any()  # the empty row and the all-zero row
    with _backend.plan_knobs(scan_slots=1):  # another grid: the same bits
        again = ops.aspect_profile(_dev(rowptr), _dev(items), _dev(A)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    empty = ops.aspect_profile(_dev(rowptr[:1]), _dev(items[:0]), _dev(A))
    assert empty.shape == (0, G)
    none = ops.aspect_profile(_dev(np.zeros(4, np.int64)), _dev(items[:0]), _dev(A))
    assert none.shape == (3, G) and not none.any()


def test_aspect_profile_skips_and_counts_bad_entries():
    rng = np.random.default_rng(283)
    G, ni = 6, 400
    A = xc.multi_hot(rng, ni, G)
    rowptr, items, _ = _history(rng, [50, 7, 70], ni)
    items[[3, 10, 52, 120]] = [ni, -4, 2**31 - 1, ni + 5]  # outside the matrix: never read
    rows = [items[:50], items[50:57], items[57:]]
    with pytest.raises(IndexError, match="4 entries"):
        ops.aspect_profile(_dev(rowptr), _dev(items), _dev(A))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.aspect_profile(_dev(rowptr), _dev(items), _dev(A), err=err).cpu().numpy()
    assert int(err.item()) == 4
    for r, row in enumerate(rows):
        cnt = A[row[(row >= 0) & (row < ni)]].sum(axis=0, dtype=np.float32)
        assert np.array_equal(got[r], cnt / cnt.sum(dtype=np.float32))


# --------------------------------------------------------------------------- aspect_coverage
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_aspect_coverage(dtype):
    rng = np.random.default_rng(285)
    G, ni, n, k = 19, 5000, 40, 100
    A = xc.multi_hot(rng, ni, G, fractional=True)
    recs = rng.integers(0, ni, (n, k)).astype(dtype)
    for u in range(10, n):  # -1 tails of every length; the last lists are -1 alone
        recs[u, max(0, k - 4 * (u - 9)):] = -1
    assert (recs[-1] == -1).all() and (recs[10, -4:] == -1).all() and recs[10, -5] >= 0
    profile = xc.history_profile(rng, A, n)
    profile[3] = 0

    def want(r):
        c = np.where((r >= 0)[:, :, None], xc.clamp(A)[np.maximum(r, 0)], 0)
        return xc.coverage_f64(xc.normalise(profile), c)

    got = ops.aspect_coverage(_dev(recs), _dev(A), _dev(profile)).cpu().numpy()
    assert np.abs(got - want(recs)).max() <= xc.TOL_COV
    assert got[3] == 0 and got[-1] == 0 and (got >= 0).all() and (got <= 1 + xc.TOL_COV).all()
    bad = recs.copy()
    bad[0, 0], bad[1, 5] = ni, ni + 7
    with pytest.raises(IndexError, match="2 entries"):
        ops.aspect_coverage(_dev(bad), _dev(A), _dev(profile))
    got = ops.aspect_coverage(_dev(bad), _dev(A), _dev(profile), check=False).cpu().numpy()
    skipped = recs.copy()
    skipped[0, 0], skipped[1, 5] = -1, -1
    assert np.abs(got - want(skipped)).max() <= xc.TOL_COV
    # binary aspects under a uniform profile: subtopic recall, a multiple of 1 / G
    B = xc.multi_hot(rng, ni, G)
    uni = ops.aspect_coverage(_dev(recs[:, :5].copy()), _dev(B),
                              torch.ones((n, G), device=DEV)).cpu().numpy()
    seen = np.stack([B[r[r >= 0]].any(axis=0).sum() if (r >= 0).any() else 0 for r in recs[:, :5]])
    assert np.abs(uni - seen / G).max() <= xc.TOL_COV
    assert ops.aspect_coverage(_dev(recs[:, :0].copy()), _dev(A), _dev(profile)).eq(0).all()


# --------------------------------------------------------------------------- doors
@pytest.fixture(scope="module")
def door():
    U, E, frozen, A = xc.door_fixture()
    mf = models.MatrixFactorization(xc.DOOR_USERS, xc.DOOR_ITEMS, xc.DOOR_D)
    with torch.no_grad():
        mf.user_embeddings.weight.copy_(torch.from_numpy(U))
        mf.item_embeddings.weight.copy_(torch.from_numpy(E))
    mf = mf.to(DEV)
    feats = datasets.Features(features=torch.from_numpy(A), feature_names=list(xc.DOOR_NAMES))
    test = torch.from_numpy(np.stack([np.arange(xc.DOOR_USERS),
                                      np.arange(xc.DOOR_USERS) % xc.DOOR_ITEMS], 1))
    data = datasets.UserItemInteractionsDataset(test, item_features=feats,
                                                number_of_users=xc.DOOR_USERS,
                                                number_of_items=xc.DOOR_ITEMS)
    history = datasets.UserItemInteractionsDataset(torch.from_numpy(frozen),
                                                   number_of_users=xc.DOOR_USERS,
                                                   number_of_items=xc.DOOR_ITEMS)
    return mf, datasets.RankingDataset(data, frozen=history), history, torch.from_numpy(A)


def _hand_composition(mf, rds, A):
    excl = rds.exclusion_csr()
    profile = ops.aspect_profile(excl[0].to(DEV), excl[1].to(DEV), A.to(DEV))
    cand, cand_sc = mf.score_topk(xc.DOOR_CANDIDATES, exclude=excl)
    want, _ = ops.xquad_rerank(cand.to(torch.int32), cand_sc, A.to(DEV), profile, xc.DOOR_K,
                               xc.DOOR_LAM)
    return want.to(torch.int64), profile, excl


def test_rerank_door_case():
    """The CPU form of the door fixture (float64 scan) through the kernel."""
    case = xc.door_case()
    got, cov = _run(case)
    assert xc.replay(got, cov, case) == 0


def test_recommend_diverse_xquad_is_the_hand_composition(door):
    mf, rds, _, A = door
    want, profile, excl = _hand_composition(mf, rds, A)
    items, scores = mf.recommend_diverse(xc.DOOR_K, xc.DOOR_CANDIDATES, method="xquad",
                                         lam=xc.DOOR_LAM, exclude=excl, item_aspects=A,
                                         aspect_profile=profile)
    assert items.dtype == torch.int64 and items.shape == scores.shape == want.shape
    assert torch.equal(items, want) and bool((items >= 0).all())
    cand, cand_sc = mf.score_topk(xc.DOOR_CANDIDATES, exclude=excl)
    at = (cand[:, None, :] == items[:, :, None]).to(torch.int64).argmax(dim=2)
    assert torch.equal(scores, cand_sc.gather(1, at))


def test_get_diverse_recommendations_xquad(door):
    mf, rds, _, A = door
    want, _, _ = _hand_composition(mf, rds, A)
    got = train.get_diverse_recommendations(rds, mf, xc.DOOR_K, xc.DOOR_CANDIDATES, method="xquad",
                                            lam=xc.DOOR_LAM, items_aspect_features=xc.DOOR_NAMES)
    assert got.dtype == torch.int64 and got.device.type == "cpu"
    assert torch.equal(got, want.cpu())
    same = train.get_diverse_recommendations(rds, mf, xc.DOOR_K, xc.DOOR_CANDIDATES, method="xquad",
                                             lam=1.0, items_aspect_features=xc.DOOR_NAMES)
    assert torch.equal(same, train.get_model_recommendations(rds, mf, xc.DOOR_K))


def test_aspect_coverage_score_in_the_score_loop(door):
    mf, rds, history, A = door
    _, profile, _ = _hand_composition(mf, rds, A)
    kw = dict(dataset=rds.data, history=history, items_aspect_features=xc.DOOR_NAMES)
    none = metrics.AspectCoverageScore(reduction="none", **kw)
    mean = metrics.AspectCoverageScore(**kw)
    total = metrics.AspectCoverageScore(reduction="sum", **kw)
    recall = metrics.AspectCoverageScore(uniform=True, reduction="none", **kw)
    per_user, avg, tot, rec = train.recommendations_score_loop(rds, mf, [none, mean, total, recall],
                                                               xc.DOOR_K)
    top = train.get_model_recommendations(rds, mf, xc.DOOR_K)
    want = ops.aspect_coverage(top.to(DEV), A.to(DEV), profile).cpu()
    assert torch.equal(per_user, want) and per_user.shape == (xc.DOOR_USERS,)
    assert torch.equal(avg, want.sum(0) / xc.DOOR_USERS) and torch.equal(tot, want.sum(0))
    assert none._dev_profile is not None and torch.equal(none._dev_profile, profile)
    # uniform: subtopic recall at k, the share of the 19 aspects a list touches
    seen = torch.stack([A[row].any(dim=0).sum() for row in top]).float() / xc.DOOR_G
    assert float((rec - seen).abs().max()) <= xc.TOL_COV
    none.refresh()
    assert none._dev_profile is None and none._dev_aspects is None
    # the re-ranker's purpose, as a property: at least half the margin the float64
    # greedy shows on this fixture (xquad_checks.door_property: 0.872 against 0.930)
    xquad = train.get_diverse_recommendations(rds, mf, xc.DOOR_K, xc.DOOR_CANDIDATES,
                                              method="xquad", lam=xc.DOOR_LAM,
                                              items_aspect_features=xc.DOOR_NAMES)
    cpu_top, cpu_xquad = xc.door_property()
    print(f"mean coverage: top-k {float(avg):.4f}, xquad {float(mean(None, xquad)):.4f}; "
          f"float64 {cpu_top:.4f}, {cpu_xquad:.4f}")
    assert cpu_xquad > cpu_top
    assert float(mean(None, xquad)) - float(avg) >= 0.5 * (cpu_xquad - cpu_top)
