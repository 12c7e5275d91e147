"""Calibrated re-rank, host side: the float64 greedy of tests/calibration_checks.py
against the directly evaluated objective, its exact special cases, the replay's
own behaviour, the measured tolerance, the ABI of the three exports (argument
checks run before any HIP call) and the host validation of the doors. No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import calibration_checks as cc
from divrec import _backend, datasets, metrics, models, ops, train

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "divrec_hip.h")


def _tiny(seed, C, G, lam=0.5, k=None, profile=None):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, G, 40)
    cand = rng.choice(40, C, replace=False)[None]
    prof = rng.random((1, G)) if profile is None else np.asarray(profile)[None]
    return cc.Case(cand, rng.standard_normal((1, C)), labels, prof, k or C, lam)


def _objective(case, chosen):
    """lam sum s - (1 - lam) KL(p || q~(list)) of the positions ``chosen`` of user 0,
    written out from the definition."""
    p = cc.normalise(case.profile)[0]
    lab = case.labels[case.cand[0, list(chosen)]]
    q = np.bincount(lab, minlength=case.G) / len(chosen)
    qt = (1 - cc.ALPHA) * q + cc.ALPHA * p
    kl = sum(p[g] * np.log(p[g] / qt[g]) for g in range(case.G) if p[g] > 0)
    return case.lam * float(case.sc[0, list(chosen)].astype(np.float64).sum()) - (1 - case.lam) * kl


@pytest.mark.parametrize("seed,C,G,lam", [(1, 8, 3, 0.5), (2, 7, 2, 0.3), (3, 8, 3, 0.0),
                                          (4, 5, 3, 0.8)])
def test_every_step_maximises_the_objective(seed, C, G, lam):
    case = _tiny(seed, C, G, lam)
    pos, kl, _ = cc.greedy(case)
    for t in range(case.k):
        done = list(pos[0, :t])
        rest = [i for i in range(C) if i not in done]
        best = max(rest, key=lambda i: (_objective(case, done + [i]), -i))
        assert _objective(case, done + [int(pos[0, t])]) >= _objective(case, done + [best]) - 1e-12
        p = cc.normalise(case.profile)
        cnt = np.bincount(case.labels[case.cand[0, pos[0, :t + 1]]], minlength=G)[None]
        assert abs(kl[0, t] - cc.kl_list(p, cnt.astype(np.float64))[0]) <= 1e-12


def test_score_order_special_cases():
    """lam = 1, G = 1 and a zero profile row each give the stable order by score."""
    for case in (_tiny(5, 8, 3, lam=1.0), _tiny(6, 8, 1, lam=0.4),
                 _tiny(7, 8, 3, lam=0.4, profile=[0.0, 0.0, 0.0]),
                 _tiny(8, 8, 3, lam=0.4, profile=[np.nan, -2.0, 0.0])):
        case.sc[0, 3] = case.sc[0, 6]  # a tie: position 3 first
        want = np.argsort(-case.sc[0], kind="stable")
        assert np.array_equal(cc.greedy(case)[0][0], want)
        assert np.array_equal(cc.greedy(case, f32=True)[0][0], want)


def test_tolerance_is_ten_times_the_measured_error():
    worst = cc.measure_tol_v()
    assert cc.TOL_V >= worst > 0
    assert 9 * worst <= cc.TOL_V <= 11 * worst  # the figure beside TOL_V is this one


def test_tie_and_profile_inputs_have_no_near_ties():
    """The float32 restatement's greedy picks exactly the float64 greedy's
    lists on the tie and profile inputs, so the GPU tests may ask for equality."""
    case = cc.profile_input()
    assert np.array_equal(cc.greedy(case)[0], cc.greedy(case, f32=True)[0])
    case = cc.tie_input()
    assert np.array_equal(cc.greedy(case)[0], cc.greedy(case, f32=True)[0])
    assert (case.sc == np.round(case.sc)).all()
    p = cc.normalise(case.profile)
    assert p[0, 0] == p[0, 1]


def test_replay_accepts_the_greedy_and_rejects_changes():
    case = cc.shape_input(65, 10, 64)
    pos, kl, _ = cc.greedy(case)
    picks = cc.items_at(case, pos)
    assert cc.replay(picks, kl, case) == 0
    off = kl.copy()
    off[2, 4] += 3 * cc.TOL_V
    assert cc.replay(picks, off, case) == 1
    # a pick swapped for a clearly worse live candidate
    worse = picks.copy()
    worse[0, 0] = case.cand[0, -1]
    assert cc.replay(worse, kl, case) >= 1
    # a list that ends while live candidates remain
    short = picks.copy()
    short[1, -1] = -1
    assert cc.replay(short, kl, case) >= 1
    # the invalid input: lists that do end, with the KL repeated
    case = cc.invalid_input()
    pos, kl, _ = cc.greedy(case)
    assert (pos[4, 20:] == -1).all() and (pos[4, :20] >= 0).all() and (pos[5] == -1).all()
    assert (kl[4, 20:] == kl[4, 19]).all()
    assert abs(kl[5, 0] + np.log(cc.ALPHA)) <= 1e-6  # an empty list: -log(alpha) sum p
    assert cc.live_and_labels(case)[2] == cc.INVALID_ERR
    assert cc.replay(cc.items_at(case, pos), kl, case) == 0


def test_door_fixture_property_holds_in_float64():
    top, calibrated = cc.door_property()
    assert calibrated < 0.75 * top  # 0.439 against 0.674


def test_symbols_are_declared_bound_and_exported():
    text = open(HEADER).read()
    for name in ("dr_calibrated_rerank", "dr_label_profile", "dr_calibration_kl"):
        assert re.search(r"^int %s\(" % name, text, re.M)
        assert _backend.SIGNATURES[name][0] is ctypes.c_int
        assert hasattr(_backend.load_library(), name)
    assert re.search(r"^#define DR_CALIB_ALPHA 0.01f$", text, re.M)
    assert re.search(r"^#define DR_CALIB_MAX_LABELS 64$", text, re.M)
    assert len(_backend.SIGNATURES["dr_calibrated_rerank"][1]) == 14
    assert _backend.SIGNATURES["dr_calibrated_rerank"][1][9] is ctypes.c_float
    assert ops.CALIB_MAX_LABELS == cc.MAX_LABELS == 64
    assert callable(ops.calibrated_rerank) and callable(ops.label_profile)
    assert callable(ops.calibration_kl) and "CalibrationScore" in metrics.__all__
    assert "calibrated" in models.matrix_factorization.RERANKERS


def test_argument_errors_without_gpu():
    lib = _backend.load_library()
    one = ctypes.c_void_p(8)  # a non-NULL pointer the checks never dereference

    def rerank(n=4, C=100, n_items=10, G=5, k_out=10, lam=0.5, ptr=one):
        return lib.dr_calibrated_rerank(ptr, ptr, n, C, ptr, n_items, G, ptr, k_out, lam, ptr,
                                        None, None, None)

    assert rerank(C=1025) == -2 and b"C must be <= 1024" in lib.dr_last_error()
    assert rerank(G=65) == -2 and b"G must be <= 64" in lib.dr_last_error()
    assert rerank(C=0) == -1 and rerank(G=0) == -1 and rerank(k_out=0) == -1
    assert rerank(k_out=101) == -1 and b"k_out must be in [1, C]" in lib.dr_last_error()
    assert rerank(lam=1.5) == -1 and rerank(lam=float("nan")) == -1
    assert rerank(n_items=0) == -1 and b"empty label table" in lib.dr_last_error()
    assert rerank(ptr=None) == -1 and b"null pointer" in lib.dr_last_error()
    assert rerank(n=0, ptr=None) == 0  # no users: a no-op success
    assert rerank(n=0, C=2000) == -2
    assert lib.dr_label_profile(one, one, 3, one, 10, 65, one, None, None) == -2
    assert lib.dr_label_profile(one, one, 3, one, 0, 5, one, None, None) == -1
    assert lib.dr_label_profile(None, None, 0, None, 10, 5, None, None, None) == 0
    i32 = _backend.DR_I32
    assert lib.dr_calibration_kl(one, i32, 3, 10, one, 10, 65, one, one, None, None) == -2
    assert lib.dr_calibration_kl(one, _backend.DR_F32, 3, 10, one, 10, 5, one, one, None, None) == -1
    assert b"DR_I32 or DR_I64" in lib.dr_last_error()
    assert lib.dr_calibration_kl(None, i32, 0, 10, None, 10, 5, None, None, None, None) == 0


def _ranking_dataset(n_users=6, n_items=40, feature="partition", n_labels=4, frozen=True):
    inter = torch.LongTensor([[u, (3 * u) % n_items] for u in range(n_users)])
    feats = None
    if feature is not None:
        feats = datasets.Features(features=(torch.arange(n_items) % n_labels).reshape(-1, 1),
                                  feature_names=[feature])
    data = datasets.UserItemInteractionsDataset(inter, item_features=feats,
                                                number_of_users=n_users, number_of_items=n_items)
    fr = None
    if frozen:
        fr = datasets.UserItemInteractionsDataset(
            torch.LongTensor([[u, (5 * u + 1) % n_items] for u in range(n_users)]),
            number_of_users=n_users, number_of_items=n_items)
    return datasets.RankingDataset(data, frozen=fr)


def test_doors_validate_on_the_host():
    """Bad arguments raise ValueError before anything touches a device (the
    models here live on the CPU)."""
    mf = models.MatrixFactorization(6, 40, 8)
    labels, profile = torch.arange(40) % 4, torch.ones(6, 4)
    with pytest.raises(ValueError, match="item_labels and user_profile"):
        mf.recommend_diverse(5, 10, method="calibrated")
    with pytest.raises(ValueError, match="item_labels and user_profile"):
        mf.recommend_diverse(5, 10, method="calibrated", item_labels=labels)
    with pytest.raises(ValueError, match="item_labels and user_profile"):
        mf.recommend_diverse(5, 10, method="calibrated", user_profile=profile)
    with pytest.raises(ValueError, match="one row per user"):
        mf.recommend_diverse(5, 10, method="calibrated", item_labels=labels,
                             user_profile=profile[:3])
    with pytest.raises(ValueError, match="n_labels"):
        mf.recommend_diverse(5, 10, method="calibrated", item_labels=labels, user_profile=profile,
                             n_labels=5)
    with pytest.raises(ValueError, match="n_labels"):
        mf.recommend_diverse(5, 10, method="calibrated", item_labels=labels,
                             user_profile=torch.ones(6, 65))
    with pytest.raises(ValueError, match="a label for each"):
        mf.recommend_diverse(5, 10, method="calibrated", item_labels=labels[:30],
                             user_profile=profile)
    with pytest.raises(ValueError, match="method must be one of"):
        mf.recommend_diverse(5, 10, method="greedy")
    with pytest.raises(ValueError, match='belong to method "calibrated"'):
        mf.recommend_diverse(5, 10, method="dpp", item_labels=labels)

    with pytest.raises(ValueError, match="method must be one of"):
        train.get_diverse_recommendations(_ranking_dataset(), mf, 5, 10, method="greedy")
    with pytest.raises(ValueError, match="frozen"):
        train.get_diverse_recommendations(_ranking_dataset(frozen=False), mf, 5, 10,
                                          method="calibrated")
    with pytest.raises(ValueError, match="no item feature 'partition'"):
        train.get_diverse_recommendations(_ranking_dataset(feature=None), mf, 5, 10,
                                          method="calibrated")
    with pytest.raises(ValueError, match="no item feature 'genre'"):
        train.get_diverse_recommendations(_ranking_dataset(), mf, 5, 10, method="calibrated",
                                          items_partition_feature="genre")
    mf80 = models.MatrixFactorization(6, 80, 8)
    with pytest.raises(ValueError, match=r"labels in \[0, 64\)"):
        train.get_diverse_recommendations(_ranking_dataset(n_items=80, n_labels=65), mf80, 5, 10,
                                          method="calibrated")
    with pytest.raises(ValueError, match="no item feature"):
        metrics.CalibrationScore(dataset=_ranking_dataset(feature=None).data)
    score = metrics.CalibrationScore(dataset=_ranking_dataset().data, reduction="none")
    assert score.n_labels == 4 and score.history is score.dataset and not score.reduce
