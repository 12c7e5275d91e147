"""dr_calibrated_rerank, dr_label_profile and dr_calibration_kl on the GPU (ops,
the model and train doors, metrics.CalibrationScore) against the float64 replay
of tests/calibration_checks.py: every step of every list a valid greedy step
within 2 TOL_V, every out_kl within TOL_V (derived there), and the exact
properties of the spec: ties to the lowest position, lam = 1 and a zero profile
the stable score order, lists that end in -1 when no live candidate is left."""
import numpy as np
import pytest
import torch

import calibration_checks as cc
from divrec import _backend, datasets, metrics, models, ops, train

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _run(case, check=True, labels_dtype=None):
    labels = case.labels if labels_dtype is None else case.labels.astype(labels_dtype)
    items, kl = ops.calibrated_rerank(_dev(case.cand), _dev(case.sc), _dev(labels),
                                      _dev(case.profile), case.k, case.lam, check=check)
    assert items.dtype == torch.int32 and kl.dtype == torch.float32
    assert items.shape == kl.shape == (case.n, case.k)
    # the finished list's calibration value is the metric of that list
    metric = ops.calibration_kl(items, _dev(labels), _dev(case.profile))
    assert float((metric - kl[:, -1]).abs().max()) <= cc.TOL_V
    return items.cpu().numpy(), kl.cpu().numpy()


def _stable_topk(case):
    order = np.argsort(-case.sc, axis=1, kind="stable")[:, :case.k]
    return np.take_along_axis(case.cand, order, axis=1)


@pytest.mark.parametrize("lam", cc.BASIC_LAMS)
def test_rerank_basic(lam):
    """lam = 0 is where candidates of one label tie at every step."""
    case = cc.basic_input(lam)
    got, kl = _run(case)
    assert cc.replay(got, kl, case) == 0
    if lam == 1.0:
        assert np.array_equal(got, _stable_topk(case))
    if lam == 0.0:  # the value is the label's alone: a pick is the first live position of its label
        live, lab, _ = cc.live_and_labels(case)
        for u in range(case.n):
            taken = np.zeros(case.G, dtype=np.int64)
            for it in got[u]:
                j = int(np.flatnonzero(case.cand[u] == it)[0])  # ids are distinct in a list
                g = int(lab[u, j])
                assert j == np.flatnonzero(live[u] & (lab[u] == g))[taken[g]]
                taken[g] += 1


@pytest.mark.parametrize("C,k,G", cc.SHAPES)
def test_rerank_shapes(C, k, G):
    case = cc.shape_input(C, k, G)
    got, kl = _run(case, labels_dtype=np.int64 if G == 64 else None)
    assert cc.replay(got, kl, case) == 0
    if k == C:  # every candidate is picked once
        assert np.array_equal(np.sort(got, axis=1), np.sort(case.cand, axis=1))
    if G == 1:
        assert np.array_equal(got, _stable_topk(case))


def test_rerank_ties():
    case, pos, _ = cc.reference(cc.tie_input)
    got, kl = _run(case)
    assert np.array_equal(got, cc.items_at(case, pos))
    assert cc.replay(got, kl, case) == 0


def test_rerank_profiles():
    case, pos, _ = cc.reference(cc.profile_input)
    got, kl = _run(case)
    assert cc.replay(got, kl, case) == 0
    assert np.array_equal(got[0], _stable_topk(case)[0]) and (kl[0] == 0).all()  # zero profile
    # rows 4 (x 8) and 6 (/ 16) are row 3 up to an exact scale, row 5 holds a NaN
    # and a negative weight where row 3 holds 0: identical picks and values
    for u in (4, 5, 6):
        assert np.array_equal(got[u], got[3]) and np.array_equal(kl[u], kl[3])
    # the one-hot row: its label first while that pays, and a finite KL throughout
    assert np.isfinite(kl).all() and (kl >= -cc.TOL_V).all()
    # row 1 has p = 0 on the most frequent label: the float64 greedy agrees on it
    assert (case.labels[case.cand[1]] == 2).sum() >= 60
    assert np.array_equal(got[1], cc.items_at(case, pos)[1])


def test_rerank_invalid_input():
    case, pos, _ = cc.reference(cc.invalid_input)
    with pytest.raises(IndexError):
        _run(case)
    got, kl = _run(case, check=False)
    assert cc.replay(got, kl, case) == 0
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.empty((case.n, case.k), dtype=torch.int32, device=DEV)
    c, s, prof = _dev(case.cand), _dev(case.sc), _dev(case.profile)
    lab32 = _dev(case.labels.astype(np.int32))
    rc = _backend.lib().dr_calibrated_rerank(
        c.data_ptr(), s.data_ptr(), case.n, case.C, lab32.data_ptr(), lab32.numel(), case.G,
        prof.data_ptr(), case.k, case.lam, out.data_ptr(), None, err.data_ptr(),
        _backend.stream(torch.device(DEV, torch.cuda.current_device())))
    assert rc == 0 and int(err.item()) == cc.INVALID_ERR == cc.live_and_labels(case)[2]
    assert np.array_equal(out.cpu().numpy(), got)  # out_kl = NULL changes no pick
    live, _, _ = cc.live_and_labels(case)
    for u in range(case.n):
        dead = set(case.cand[u][~live[u]].tolist()) - {-1}
        assert not dead & set(got[u].tolist())
        n_live = int(live[u].sum())
        assert (got[u, :min(n_live, case.k)] >= 0).all() and (got[u, n_live:] == -1).all()
    assert (kl[4, 20:] == kl[4, 19]).all()  # the list ended: the KL of the list as it stands
    assert (got[5] == -1).all() and np.allclose(kl[5], -np.log(cc.ALPHA), atol=cc.TOL_V)


def test_rerank_many_users_per_wave():
    case, _, _ = cc.reference(cc.many_users_input)
    got, kl = _run(case)
    with _backend.plan_knobs(scan_slots=2):  # tens of users per wave
        got2, kl2 = _run(case)
    assert np.array_equal(got, got2) and np.array_equal(kl, kl2)
    assert cc.replay(got2, kl2, case) == 0  # every user


def test_rerank_empty_and_bad_arguments():
    case = cc.shape_input(63, 63, 2)
    c, s, lab, prof = _dev(case.cand), _dev(case.sc), _dev(case.labels), _dev(case.profile)
    items, kl = ops.calibrated_rerank(c[:0], s[:0], lab, prof[:0], 10, 0.5)
    assert items.shape == kl.shape == (0, 10)
    with pytest.raises(ValueError):
        ops.calibrated_rerank(c, s, lab, prof[:3], 10, 0.5)
    with pytest.raises(ValueError):
        ops.calibrated_rerank(c, s, lab.to(torch.float32), prof, 10, 0.5)
    with pytest.raises(ValueError):
        ops.calibrated_rerank(c, s, lab, torch.ones((case.n, 65), device=DEV), 10, 0.5)
    with pytest.raises(RuntimeError, match="k_out"):
        ops.calibrated_rerank(c, s, lab, prof, 64, 0.5)


# --------------------------------------------------------------------------- label_profile
def _history(rng, lengths, ni):
    rows = [rng.integers(0, ni, m) for m in lengths]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rowptr, np.concatenate(rows).astype(np.int32), rows


def test_label_profile_is_bincount_over_total():
    rng = np.random.default_rng(181)
    G, ni = 19, 5000
    labels = rng.integers(0, G, ni)
    rowptr, items, rows = _history(rng, [0, 1, 300, 0, 64, 65, 1000], ni)
    for lab in (labels.astype(np.int32), labels.astype(np.int64)):
        got = ops.label_profile(_dev(rowptr), _dev(items), _dev(lab), G).cpu().numpy()
        for r, row in enumerate(rows):
            cnt = np.bincount(labels[row], minlength=G).astype(np.float32)
            want = cnt / np.float32(len(row)) if len(row) else np.zeros(G, np.float32)
            assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32)), r
    empty = ops.label_profile(_dev(rowptr[:1]), _dev(items[:0]), _dev(labels), G)
    assert empty.shape == (0, G)
    none = ops.label_profile(_dev(np.zeros(4, np.int64)), _dev(items[:0]), _dev(labels), G)
    assert none.shape == (3, G) and not none.any()


def test_label_profile_skips_and_counts_bad_entries():
    rng = np.random.default_rng(182)
    G, ni = 6, 400
    labels = rng.integers(0, G, ni)
    labels[:5], labels[5:9] = -1, G
    rowptr, items, rows = _history(rng, [50, 7], ni)
    items[[3, 10, 52]] = [ni, -4, 2**31 - 1]  # outside the table: never read
    rows = [items[:50], items[50:]]
    bad = sum(int(((row < 0) | (row >= ni)).sum()) for row in rows)
    bad += sum(int(np.isin(row, np.arange(9)).sum()) for row in rows)
    assert bad >= 3
    with pytest.raises(IndexError, match=f"{bad} entries"):
        ops.label_profile(_dev(rowptr), _dev(items), _dev(labels), G)
    got = ops.label_profile(_dev(rowptr), _dev(items), _dev(labels), G, check=False).cpu().numpy()
    for r, row in enumerate(rows):
        ok = row[(row >= 9) & (row < ni)]
        want = np.bincount(labels[ok], minlength=G).astype(np.float32) / np.float32(len(ok))
        assert np.array_equal(got[r], want)


# --------------------------------------------------------------------------- calibration_kl
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_calibration_kl(dtype):
    rng = np.random.default_rng(183)
    G, ni, n, k = 19, 5000, 40, 100
    labels = rng.integers(0, G, ni).astype(np.int32)
    recs = rng.integers(0, ni, (n, k)).astype(dtype)
    for u in range(10, n):  # -1 tails of every length; the last lists are -1 alone
        recs[u, max(0, k - 4 * (u - 9)):] = -1
    assert (recs[-1] == -1).all() and (recs[10, -4:] == -1).all() and recs[10, -5] >= 0
    profile = cc.history_profile(rng, labels, G, n)
    profile[3] = 0
    got = ops.calibration_kl(_dev(recs), _dev(labels), _dev(profile)).cpu().numpy()
    cnt = np.zeros((n, G))
    for u in range(n):
        cnt[u] = np.bincount(labels[recs[u][recs[u] >= 0]], minlength=G)
    want = cc.kl_list(cc.normalise(profile), cnt)
    assert np.abs(got - want).max() <= cc.TOL_V
    assert got[3] == 0 and abs(got[-1] + np.log(cc.ALPHA)) <= cc.TOL_V
    bad = recs.copy()
    bad[0, 0], bad[1, 5] = ni, ni + 7
    with pytest.raises(IndexError, match="2 entries"):
        ops.calibration_kl(_dev(bad), _dev(labels), _dev(profile))
    got = ops.calibration_kl(_dev(bad), _dev(labels), _dev(profile), check=False).cpu().numpy()
    cnt[0, labels[recs[0, 0]]] -= 1
    cnt[1, labels[recs[1, 5]]] -= 1
    assert np.abs(got - cc.kl_list(cc.normalise(profile), cnt)).max() <= cc.TOL_V


# --------------------------------------------------------------------------- doors
@pytest.fixture(scope="module")
def door():
    U, E, frozen, labels = cc.door_fixture()
    mf = models.MatrixFactorization(cc.DOOR_USERS, cc.DOOR_ITEMS, cc.DOOR_D)
    with torch.no_grad():
        mf.user_embeddings.weight.copy_(torch.from_numpy(U))
        mf.item_embeddings.weight.copy_(torch.from_numpy(E))
    mf = mf.to(DEV)
    feats = datasets.Features(features=torch.from_numpy(labels).reshape(-1, 1),
                              feature_names=["partition"])
    test = torch.from_numpy(np.stack([np.arange(cc.DOOR_USERS),
                                      np.arange(cc.DOOR_USERS) % cc.DOOR_ITEMS], 1))
    data = datasets.UserItemInteractionsDataset(test, item_features=feats,
                                                number_of_users=cc.DOOR_USERS,
                                                number_of_items=cc.DOOR_ITEMS)
    history = datasets.UserItemInteractionsDataset(torch.from_numpy(frozen),
                                                   number_of_users=cc.DOOR_USERS,
                                                   number_of_items=cc.DOOR_ITEMS)
    return mf, datasets.RankingDataset(data, frozen=history), history, torch.from_numpy(labels)


def _hand_composition(mf, rds, labels):
    excl = rds.exclusion_csr()
    profile = ops.label_profile(excl[0].to(DEV), excl[1].to(DEV), labels.to(DEV), cc.DOOR_G)
    cand, cand_sc = mf.score_topk(cc.DOOR_CANDIDATES, exclude=excl)
    want, _ = ops.calibrated_rerank(cand.to(torch.int32), cand_sc, labels.to(DEV), profile,
                                    cc.DOOR_K, cc.DOOR_LAM)
    return want.to(torch.int64), profile, excl


def test_recommend_diverse_calibrated_is_the_hand_composition(door):
    mf, rds, _, labels = door
    want, profile, excl = _hand_composition(mf, rds, labels)
    items, scores = mf.recommend_diverse(cc.DOOR_K, cc.DOOR_CANDIDATES, method="calibrated",
                                         lam=cc.DOOR_LAM, exclude=excl, item_labels=labels,
                                         user_profile=profile, n_labels=cc.DOOR_G)
    assert items.dtype == torch.int64 and items.shape == scores.shape == want.shape
    assert torch.equal(items, want) and bool((items >= 0).all())
    cand, cand_sc = mf.score_topk(cc.DOOR_CANDIDATES, exclude=excl)
    at = (cand[:, None, :] == items[:, :, None]).to(torch.int64).argmax(dim=2)
    assert torch.equal(scores, cand_sc.gather(1, at))


def test_get_diverse_recommendations_calibrated(door):
    mf, rds, _, labels = door
    want, _, _ = _hand_composition(mf, rds, labels)
    got = train.get_diverse_recommendations(rds, mf, cc.DOOR_K, cc.DOOR_CANDIDATES,
                                            method="calibrated", lam=cc.DOOR_LAM)
    assert got.dtype == torch.int64 and got.device.type == "cpu"
    assert torch.equal(got, want.cpu())
    same = train.get_diverse_recommendations(rds, mf, cc.DOOR_K, cc.DOOR_CANDIDATES,
                                             method="calibrated", lam=1.0)
    assert torch.equal(same, train.get_model_recommendations(rds, mf, cc.DOOR_K))


def test_calibration_score_in_the_score_loop(door):
    mf, rds, history, labels = door
    _, profile, _ = _hand_composition(mf, rds, labels)
    none = metrics.CalibrationScore(dataset=rds.data, history=history, reduction="none")
    mean = metrics.CalibrationScore(dataset=rds.data, history=history)
    total = metrics.CalibrationScore(dataset=rds.data, history=history, reduction="sum")
    per_user, avg, tot = train.recommendations_score_loop(rds, mf, [none, mean, total], cc.DOOR_K)
    top = train.get_model_recommendations(rds, mf, cc.DOOR_K)
    want = ops.calibration_kl(top.to(DEV), labels.to(DEV), profile).cpu()
    assert torch.equal(per_user, want) and per_user.shape == (cc.DOOR_USERS,)
    assert torch.equal(avg, want.sum(0) / cc.DOOR_USERS) and torch.equal(tot, want.sum(0))
    assert none._dev_profile is not None and torch.equal(none._dev_profile, profile)
    # the re-ranker's purpose, as a property (calibration_checks.door_property
    # shows the float64 greedy's margin on this fixture: 0.439 against 0.674)
    calibrated = train.get_diverse_recommendations(rds, mf, cc.DOOR_K, cc.DOOR_CANDIDATES,
                                                   method="calibrated", lam=cc.DOOR_LAM)
    assert float(mean(None, calibrated)) < float(avg)
    assert cc.door_property()[1] < cc.door_property()[0]
