"""xQuAD re-rank, host side: the float64 greedy of tests/xquad_checks.py against
the directly evaluated objective, its exact special cases, the replay's own
behaviour, the measured tolerances, the ABI of the three exports (argument
checks run before any HIP call) and the host validation of the doors. No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import xquad_checks as xc
from divrec import _backend, datasets, metrics, models, ops, train

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "divrec_hip.h")


def _tiny(seed, C, G, lam=0.5, k=None, profile=None, aspects=None, fractional=True):
    rng = np.random.default_rng(seed)
    A = xc.multi_hot(rng, 40, G, fractional=fractional) if aspects is None else aspects
    cand = rng.choice(40, C, replace=False)[None]
    prof = rng.random((1, G)) if profile is None else np.asarray(profile)[None]
    return xc.Case(cand, rng.standard_normal((1, C)), A, prof, k or C, lam)


def _objective(case, chosen):
    """lam sum s + (1 - lam) sum_a p_a (1 - prod (1 - c)) of the positions
    ``chosen`` of user 0, written out from the definition."""
    p = xc.normalise(case.profile)[0]
    c = xc.clamp(case.aspects)[case.cand[0, list(chosen)]].astype(np.float64)
    cov = sum(p[a] * (1 - np.prod(1 - c[:, a])) for a in range(case.G))
    return case.lam * float(case.sc[0, list(chosen)].astype(np.float64).sum()) + (1 - case.lam) * cov


@pytest.mark.parametrize("seed,C,G,lam", [(1, 8, 3, 0.5), (2, 7, 2, 0.3), (3, 8, 5, 0.0),
                                          (4, 5, 3, 0.8)])
def test_every_step_maximises_the_objective(seed, C, G, lam):
    """The greedy's value is the marginal gain of the list objective, and its
    coverage column is the closed form of the list so far."""
    case = _tiny(seed, C, G, lam)
    pos, cov, _, _ = xc.greedy(case)
    _, c, _ = xc.live_and_rows(case)
    p = xc.normalise(case.profile)
    for t in range(case.k):
        done = list(pos[0, :t])
        rest = [i for i in range(C) if i not in done]
        best = max(rest, key=lambda i: (_objective(case, done + [i]), -i))
        assert _objective(case, done + [int(pos[0, t])]) >= _objective(case, done + [best]) - 1e-12
        assert abs(cov[0, t] - xc.coverage_f64(p, c[:, pos[0, :t + 1]])[0]) <= 1e-12


def test_score_order_special_cases():
    """lam = 1, a zero profile row and an all-zero matrix each give the stable order by score."""
    zero = np.zeros((40, 3), dtype=np.float32)
    for case in (_tiny(5, 8, 3, lam=1.0), _tiny(7, 8, 3, lam=0.4, profile=[0.0, 0.0, 0.0]),
                 _tiny(8, 8, 3, lam=0.4, profile=[np.nan, -2.0, 0.0]),
                 _tiny(9, 8, 3, lam=0.4, aspects=zero)):
        case.sc[0, 3] = case.sc[0, 6]  # a tie: position 3 first
        want = np.argsort(-case.sc[0], kind="stable")
        assert np.array_equal(xc.greedy(case)[0][0], want)
        assert np.array_equal(xc.greedy(case, f32=True)[0][0], want)
        assert np.array_equal(xc.stable_topk(case)[0], case.cand[0, want])


def test_coverage_is_monotone_bounded_and_the_closed_form():
    for case in (xc.shape_input(257, 40, 19), xc.shape_input(65, 10, 64), xc.invalid_input(),
                 xc.aspect_value_input()):
        pos, cov, _, _ = xc.greedy(case)
        assert (np.diff(cov, axis=1) >= -1e-15).all() and (cov >= 0).all() and (cov <= 1 + 1e-12).all()
        _, c, _ = xc.live_and_rows(case)
        rows = np.arange(case.n)[:, None]
        picked = np.where((pos >= 0)[:, :, None], c[rows, np.maximum(pos, 0)], 0)
        closed = xc.coverage_f64(xc.normalise(case.profile), picked)
        assert np.abs(cov[:, -1] - closed).max() <= 1e-12


def test_tolerances_are_ten_times_the_measured_error():
    worst_v, worst_c = xc.measure_tol()
    assert worst_v > 0 and worst_c > 0
    # the figures beside TOL_V and TOL_COV are these, to their three printed digits
    assert f"{10 * worst_v:.2e}" == f"{xc.TOL_V:.2e}"
    assert f"{10 * worst_c:.2e}" == f"{xc.TOL_COV:.2e}"
    doc = xc.__doc__
    assert f"{worst_v:.2e}" in doc and f"{worst_c:.2e}" in doc


def test_tie_and_profile_inputs_have_no_near_ties():
    """The float32 restatement's greedy picks exactly the float64 greedy's
    lists on the tie and profile inputs, so the GPU tests may ask for equality."""
    case = xc.profile_input()
    assert np.array_equal(xc.greedy(case)[0], xc.greedy(case, f32=True)[0])
    case = xc.tie_input()
    assert np.array_equal(xc.greedy(case)[0], xc.greedy(case, f32=True)[0])
    assert (case.sc == np.round(case.sc)).all()
    p = xc.normalise(case.profile)
    assert p[0, 0] == p[0, 1]
    # many bit-equal aspect rows: six kinds over 300 candidates
    assert len(np.unique(case.aspects[case.cand[0]], axis=0)) <= 6


def test_aspect_value_input_equals_its_clamped_copy():
    raw, clamped = xc.aspect_value_input(), xc.aspect_value_input(clamped=True)
    a = raw.aspects
    assert np.isnan(a).any() and np.isinf(a).any() and (a < 0).any() and (a > 1).any()
    assert (a == 0).all(axis=1).any()
    assert np.array_equal(xc.greedy(raw)[0], xc.greedy(clamped)[0])


def test_replay_accepts_the_greedy_and_rejects_changes():
    case = xc.shape_input(65, 10, 64)
    pos, cov, _, _ = xc.greedy(case)
    picks = xc.items_at(case, pos)
    assert xc.replay(picks, cov, case) == 0
    off = cov.copy()
    off[2, 4] += 3 * xc.TOL_COV
    assert xc.replay(picks, off, case) == 1
    # two picks swapped across a value gap larger than 2 TOL_V
    _, c, _ = xc.live_and_rows(case)
    v0 = xc.values_f64(case, np.ones_like(case.cand, dtype=bool), c, xc.normalise(case.profile))
    last = int(np.argmin(v0[0]))
    assert v0[0, pos[0, 0]] - v0[0, last] > 2 * xc.TOL_V and last not in pos[0]
    swapped = picks.copy()
    swapped[0, 0] = case.cand[0, last]
    assert xc.replay(swapped, cov, case) >= 1
    # a list that ends while live candidates remain
    short = picks.copy()
    short[1, -1] = -1
    assert xc.replay(short, cov, case) >= 1
    # the invalid input: lists that do end, with the coverage repeated
    case = xc.invalid_input()
    pos, cov, _, _ = xc.greedy(case)
    assert (pos[4, 20:] == -1).all() and (pos[4, :20] >= 0).all() and (pos[5] == -1).all()
    assert (cov[4, 20:] == cov[4, 19]).all() and (cov[5] == 0).all()
    assert xc.live_and_rows(case)[2] == xc.INVALID_ERR
    assert xc.replay(xc.items_at(case, pos), cov, case) == 0
    # a NaN and a -inf score count as -FLT_MAX: live, and the last two picked
    assert set(pos[3, :].tolist()).isdisjoint({5, 17})


def test_replay_passes_every_input_on_the_float64_picks():
    for case in (xc.tie_input(), xc.profile_input(), xc.aspect_value_input(),
                 xc.shape_input(63, 63, 2), xc.shape_input(1, 1, 1)):
        pos, cov, _, _ = xc.greedy(case)
        assert xc.replay(xc.items_at(case, pos), cov, case) == 0, case.name


def test_shapes_reach_the_limits():
    assert (1024, 128, 32) in xc.SHAPES and (512, 100, 64) in xc.SHAPES
    assert 1024 * 32 == 512 * 64 == xc.MAX_CELLS == ops.XQUAD_MAX_CELLS
    assert xc.MAX_ASPECTS == ops.XQUAD_MAX_ASPECTS == 64
    frac = [xc.shape_input(*s).aspects for s in xc.SHAPES]
    assert sum(bool(((a > 0) & (a < 1)).any()) for a in frac) == len(xc.SHAPES) // 2


def test_door_fixture_property_holds_in_float64():
    top, xquad = xc.door_property()
    assert xquad - top > 0.04  # 0.872 against 0.930


def test_symbols_are_declared_bound_and_exported():
    text = open(HEADER).read()
    for name in ("dr_xquad_rerank", "dr_aspect_profile", "dr_aspect_coverage"):
        assert re.search(r"^int %s\(" % name, text, re.M)
        assert _backend.SIGNATURES[name][0] is ctypes.c_int
        assert hasattr(_backend.load_library(), name)
    assert re.search(r"^#define DR_XQUAD_MAX_ASPECTS 64$", text, re.M)
    assert re.search(r"^#define DR_XQUAD_MAX_CELLS 32768$", text, re.M)
    assert len(_backend.SIGNATURES["dr_xquad_rerank"][1]) == 14
    assert _backend.SIGNATURES["dr_xquad_rerank"][1][9] is ctypes.c_float
    assert len(_backend.SIGNATURES["dr_aspect_profile"][1]) == 9
    assert len(_backend.SIGNATURES["dr_aspect_coverage"][1]) == 11
    assert callable(ops.xquad_rerank) and callable(ops.aspect_profile)
    assert callable(ops.aspect_coverage)
    assert "AspectCoverageScore" in metrics.__all__ and "aspect_matrix" in metrics.__all__
    assert "xquad" in models.matrix_factorization.RERANKERS


def test_argument_errors_without_gpu():
    lib = _backend.load_library()
    one = ctypes.c_void_p(8)  # a non-NULL pointer the checks never dereference

    def rerank(n=4, C=100, n_items=10, G=5, k_out=10, lam=0.5, ptr=one):
        return lib.dr_xquad_rerank(ptr, ptr, n, C, ptr, n_items, G, ptr, k_out, lam, ptr, None,
                                   None, None)

    table = [  # (arguments, code, message)
        (dict(C=1025), -2, b"C must be <= 1024"),
        (dict(C=0), -1, b"C must be >= 1"),
        (dict(G=65), -2, b"G must be <= 64"),
        (dict(G=0), -1, b"G must be >= 1"),
        (dict(C=1024, G=33), -2, b"C * G must be <= 32768"),
        (dict(C=513, G=64), -2, b"C * G must be <= 32768"),
        (dict(k_out=0), -1, b"k_out must be in [1, C]"),
        (dict(k_out=101), -1, b"k_out must be in [1, C]"),
        (dict(lam=1.5), -1, b"lambda must be in [0, 1]"),
        (dict(lam=-0.1), -1, b"lambda must be in [0, 1]"),
        (dict(lam=float("nan")), -1, b"lambda must be in [0, 1]"),
        (dict(n=-1), -1, b"n_users must be >= 0"),
        (dict(n_items=-1), -1, b"n_items in [0, 2^31)"),
        (dict(n_items=2**31 - 1), -1, b"n_items in [0, 2^31)"),
        (dict(n_items=0), -1, b"empty aspect matrix"),
        (dict(ptr=None), -1, b"null pointer"),
    ]
    for kwargs, code, message in table:
        assert rerank(**kwargs) == code, kwargs
        assert lib.dr_last_error().startswith(b"dr_xquad_rerank: "), kwargs
        assert message in lib.dr_last_error(), kwargs
    assert rerank(n=0, ptr=None) == 0            # no users: a no-op success
    assert rerank(n=0, n_items=0, ptr=None) == 0  # and no matrix needed
    assert rerank(n=0, C=2000) == -2             # the limits hold without users too
    assert rerank(n=0, C=1024, G=33) == -2
    assert rerank(C=1024, G=32, k_out=128, ptr=None) == -1  # at the cell limit: past the checks
    assert b"null pointer" in lib.dr_last_error()
    assert rerank(C=512, G=64, ptr=None) == -1 and b"null pointer" in lib.dr_last_error()

    assert lib.dr_aspect_profile(one, one, 3, one, 10, 65, one, None, None) == -2
    assert lib.dr_aspect_profile(one, one, 3, one, 0, 5, one, None, None) == -1
    assert b"empty aspect matrix" in lib.dr_last_error()
    assert lib.dr_aspect_profile(one, one, -1, one, 10, 5, one, None, None) == -1
    assert lib.dr_aspect_profile(None, one, 3, one, 10, 5, one, None, None) == -1
    assert lib.dr_aspect_profile(None, None, 0, None, 10, 5, None, None, None) == 0
    i32 = _backend.DR_I32
    assert lib.dr_aspect_coverage(one, i32, 3, 10, one, 10, 65, one, one, None, None) == -2
    assert lib.dr_aspect_coverage(one, _backend.DR_F32, 3, 10, one, 10, 5, one, one, None, None) == -1
    assert b"DR_I32 or DR_I64" in lib.dr_last_error()
    assert lib.dr_aspect_coverage(one, i32, 3, 10, one, 0, 5, one, one, None, None) == -1
    assert lib.dr_aspect_coverage(one, i32, 3, 10, None, 10, 5, one, one, None, None) == -1
    assert lib.dr_aspect_coverage(None, i32, 0, 10, None, 10, 5, None, None, None, None) == 0


GENRES = ["g0", "g1", "g2"]


def _ranking_dataset(n_users=6, n_items=40, names=GENRES, frozen=True):
    inter = torch.LongTensor([[u, (3 * u) % n_items] for u in range(n_users)])
    feats = None
    if names:
        cols = torch.stack([(torch.arange(n_items) % (a + 2) == 0).to(torch.int64)
                            for a in range(len(names))], dim=1)
        feats = datasets.Features(features=cols, feature_names=list(names))
    data = datasets.UserItemInteractionsDataset(inter, item_features=feats,
                                                number_of_users=n_users, number_of_items=n_items)
    fr = None
    if frozen:
        fr = datasets.UserItemInteractionsDataset(
            torch.LongTensor([[u, (5 * u + 1) % n_items] for u in range(n_users)]),
            number_of_users=n_users, number_of_items=n_items)
    return datasets.RankingDataset(data, frozen=fr)


def test_aspect_matrix():
    data = _ranking_dataset().data
    A = metrics.aspect_matrix(data, ["g2", "g0"])
    assert A.dtype == torch.float32 and A.shape == (40, 2) and A.is_contiguous()
    assert torch.equal(A[:, 0], (torch.arange(40) % 4 == 0).float())
    assert torch.equal(A[:, 1], (torch.arange(40) % 2 == 0).float())
    with pytest.raises(ValueError, match="no item feature 'genre'"):
        metrics.aspect_matrix(data, ["g0", "genre"])
    with pytest.raises(ValueError, match="no item feature 'g0'"):
        metrics.aspect_matrix(_ranking_dataset(names=None).data, ["g0"])
    with pytest.raises(ValueError, match="at least one"):
        metrics.aspect_matrix(data, [])
    with pytest.raises(ValueError, match="at most 64"):
        metrics.aspect_matrix(data, ["g0"] * 65)


def test_doors_validate_on_the_host():
    """Bad arguments raise ValueError before anything touches a device (the
    models here live on the CPU)."""
    mf = models.MatrixFactorization(6, 40, 8)
    aspects, profile = torch.ones(40, 3), torch.ones(6, 3)
    with pytest.raises(ValueError, match="item_aspects and aspect_profile"):
        mf.recommend_diverse(5, 10, method="xquad")
    with pytest.raises(ValueError, match="item_aspects and aspect_profile"):
        mf.recommend_diverse(5, 10, method="xquad", item_aspects=aspects)
    with pytest.raises(ValueError, match="item_aspects and aspect_profile"):
        mf.recommend_diverse(5, 10, method="xquad", aspect_profile=profile)
    with pytest.raises(ValueError, match="one row per user"):
        mf.recommend_diverse(5, 10, method="xquad", item_aspects=aspects,
                             aspect_profile=profile[:3])
    with pytest.raises(ValueError, match="one row per user"):
        mf.recommend_diverse(5, 10, method="xquad", item_aspects=aspects,
                             aspect_profile=torch.ones(6, 4))
    with pytest.raises(ValueError, match="a row for each of the 40 items"):
        mf.recommend_diverse(5, 10, method="xquad", item_aspects=aspects[:30],
                             aspect_profile=profile)
    with pytest.raises(ValueError, match="a row for each"):
        mf.recommend_diverse(5, 10, method="xquad", item_aspects=aspects[:, 0],
                             aspect_profile=profile)
    with pytest.raises(ValueError, match="n_aspects <= 64, got 65"):
        mf.recommend_diverse(5, 10, method="xquad", item_aspects=torch.ones(40, 65),
                             aspect_profile=torch.ones(6, 65))
    big = models.MatrixFactorization(6, 2000, 8)
    with pytest.raises(ValueError, match="at most 682 candidates fit with 48 aspects"):
        big.recommend_diverse(5, 700, method="xquad", item_aspects=torch.ones(2000, 48),
                              aspect_profile=torch.ones(6, 48))
    with pytest.raises(ValueError, match='belong to method "xquad"'):
        mf.recommend_diverse(5, 10, method="dpp", item_aspects=aspects)
    with pytest.raises(ValueError, match='belong to method "xquad"'):
        mf.recommend_diverse(5, 10, method="calibrated", item_labels=torch.arange(40) % 4,
                             user_profile=torch.ones(6, 4), aspect_profile=profile)
    # the existing messages stay word for word
    with pytest.raises(ValueError, match='belong to method "calibrated"'):
        mf.recommend_diverse(5, 10, method="dpp", item_labels=torch.arange(40) % 4)
    with pytest.raises(ValueError, match='belong to method "calibrated", not \'xquad\''):
        mf.recommend_diverse(5, 10, method="xquad", item_labels=torch.arange(40) % 4,
                             item_aspects=aspects, aspect_profile=profile)
    with pytest.raises(ValueError, match=r"method must be one of \['calibrated', 'dpp', 'mmr', "
                                         r"'xquad'\]"):
        mf.recommend_diverse(5, 10, method="greedy")

    with pytest.raises(ValueError, match="needs items_aspect_features"):
        train.get_diverse_recommendations(_ranking_dataset(), mf, 5, 10, method="xquad")
    with pytest.raises(ValueError, match="frozen"):
        train.get_diverse_recommendations(_ranking_dataset(frozen=False), mf, 5, 10,
                                          method="xquad", items_aspect_features=GENRES)
    with pytest.raises(ValueError, match="no item feature 'genre'"):
        train.get_diverse_recommendations(_ranking_dataset(), mf, 5, 10, method="xquad",
                                          items_aspect_features=["g0", "genre"])
    with pytest.raises(ValueError, match="no item feature 'g0'"):
        train.get_diverse_recommendations(_ranking_dataset(names=None), mf, 5, 10, method="xquad",
                                          items_aspect_features=GENRES)
    many = [f"a{i}" for i in range(65)]
    with pytest.raises(ValueError, match="at most 64"):
        train.get_diverse_recommendations(_ranking_dataset(names=many), mf, 5, 10, method="xquad",
                                          items_aspect_features=many)
    with pytest.raises(ValueError, match='belongs to method "xquad"'):
        train.get_diverse_recommendations(_ranking_dataset(), mf, 5, 10, method="mmr",
                                          items_aspect_features=GENRES)

    with pytest.raises(ValueError, match="no item feature"):
        metrics.AspectCoverageScore(dataset=_ranking_dataset(names=None).data,
                                    items_aspect_features=GENRES)
    score = metrics.AspectCoverageScore(dataset=_ranking_dataset().data,
                                        items_aspect_features=GENRES, reduction="none")
    assert score.n_aspects == 3 and score.history is score.dataset and not score.reduce
    assert not score.uniform and score.aspects.shape == (40, 3)
    uni = metrics.AspectCoverageScore(dataset=_ranking_dataset().data, uniform=True,
                                      items_aspect_features=GENRES[:2])
    assert uni.uniform and uni.n_aspects == 2
