"""DPP re-rank, host side: the float64 greedy of tests/dpp_checks.py against
numpy.linalg.slogdet and a brute-force argmax, the replay's own behaviour, the
dr_dpp_rerank ABI's argument checks (they run before any HIP call) and the host
validation of the model and train doors. No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import oracle
from divrec import _backend, datasets, models, ops, train
from dpp_checks import (EPS, TOL_R, TOL_V, _Cholesky, _unit_rows, dpp_check_positions,
                        dpp_greedy_f64, residual_error_f32)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "divrec_hip.h")


def _small(seed=3, ni=400, d=16, C=50):
    rng = np.random.default_rng(seed)
    E = oracle.as_bf16_f32(rng.standard_normal((ni, d)).astype(np.float32))
    cand = rng.choice(ni, C, replace=False).astype(np.int32)
    return cand, rng.standard_normal(C).astype(np.float32), E


def _gram(cand, E):
    X = E[cand].astype(np.float64)
    X /= np.sqrt((X * X).sum(1))[:, None]
    return X @ X.T


def test_residuals_are_log_det_increments():
    """log(resid_t) = slogdet(S_{Y_t}) - slogdet(S_{Y_{t-1}}) to 1e-12 (50 x 16, 8 picks)."""
    cand, sc, E = _small()
    pos, resid, _, _ = dpp_greedy_f64(cand, sc, E, 8, 0.4)
    S = _gram(cand, E)
    prev = 0.0
    for t in range(8):
        Y = pos[:t + 1]
        sign, ld = np.linalg.slogdet(S[np.ix_(Y, Y)])
        assert sign > 0 and abs(np.log(resid[t]) - (ld - prev)) <= 1e-12
        prev = ld


def test_picks_are_the_brute_force_argmax():
    """At lam = 0.4 every pick is the argmax of lam s + (1 - lam) dlogdet over the unpicked."""
    cand, sc, E = _small(seed=4)
    lam = 0.4
    pos, _, _, _ = dpp_greedy_f64(cand, sc, E, 8, lam)
    S = _gram(cand, E)
    for t in range(8):
        Y = list(pos[:t])
        base = np.linalg.slogdet(S[np.ix_(Y, Y)])[1] if Y else 0.0
        val = np.full(len(cand), -np.inf)
        for i in range(len(cand)):
            if i not in Y:
                Z = Y + [i]
                val[i] = lam * sc[i] + (1 - lam) * (np.linalg.slogdet(S[np.ix_(Z, Z)])[1] - base)
        assert int(np.argmax(val)) == pos[t]


def test_first_pick_at_lam_zero_is_position_zero():
    cand, sc, E = _small(seed=5)
    pos, resid, _, _ = dpp_greedy_f64(cand, sc, E, 4, 0.0)
    assert pos[0] == 0 and resid[0] == 1.0


def test_replay_accepts_the_greedy_and_rejects_a_swap():
    cand, sc, E = _small(seed=6)
    lam = 0.5
    pos, resid, _, _ = dpp_greedy_f64(cand, sc, E, 8, lam)
    picks = cand[pos][None]
    assert dpp_check_positions(picks, resid[None], cand[None], sc[None], E, lam) == 0
    # two neighbouring picks swapped across a value gap above TOL_V at their
    # step: the first of the two is then not the step's best (tol_r = 1 takes
    # the residual records out of the verdict, so the value test alone rejects)
    ch = _Cholesky(_unit_rows(cand, E)[0], 8)
    for t in range(7):
        val = lam * sc.astype(np.float64) + (1 - lam) * np.log(np.maximum(ch.r, 1e-300))
        if val[pos[t]] - val[pos[t + 1]] > 100 * TOL_V:
            break
        ch.pick(int(pos[t]))
    else:
        raise AssertionError("no step with a clear gap: choose another seed")
    swapped = picks.copy()
    swapped[0, [t, t + 1]] = swapped[0, [t + 1, t]]
    assert dpp_check_positions(swapped, resid[None], cand[None], sc[None], E, lam, tol_r=1.0) >= 1
    assert dpp_check_positions(swapped, resid[None], cand[None], sc[None], E, lam) >= 1
    # a list that ends while eligible candidates remain is wrong too
    short, short_r = picks.copy(), resid[None].copy()
    short[0, -1], short_r[0, -1] = -1, 0.0
    assert dpp_check_positions(short, short_r, cand[None], sc[None], E, lam) == 1


def test_float32_restatement_is_within_the_tolerance():
    """The fp32 basis form tracks the float64 Cholesky to a tenth of TOL_R on a
    config-5 shaped list (the figure beside TOL_R comes from the same function)."""
    from dpp_checks import config5_inputs
    cand, sc, E = config5_inputs(64, 777, n=2)
    pos, _, _, _ = dpp_greedy_f64(cand[0], sc[0], E, 48, 0.3)
    assert 0 < residual_error_f32(pos, cand[0], E) <= TOL_R / 10 * 1.0001
    assert EPS == 1e-4 and TOL_V == 1e-4


def test_symbol_is_declared_bound_and_exported():
    text = open(HEADER).read()
    assert re.search(r"^int dr_dpp_rerank\(", text, re.M)
    assert re.search(r"^#define DR_DPP_EPS 1e-4f$", text, re.M)
    res, args = _backend.SIGNATURES["dr_dpp_rerank"]
    assert res is ctypes.c_int and len(args) == 13 and args[8] is ctypes.c_float
    assert hasattr(_backend.load_library(), "dr_dpp_rerank")
    assert callable(ops.dpp_rerank) and ops.DPP_WIDTHS == (64, 128)
    assert "get_diverse_recommendations" in train.__all__


def test_argument_errors_without_gpu():
    lib = _backend.load_library()
    one = ctypes.c_void_p(8)  # a non-NULL pointer the checks never dereference

    def call(n_users=4, C=100, n_items=10, d=128, k_out=10, lam=0.5, ptr=one):
        return lib.dr_dpp_rerank(ptr, ptr, n_users, C, ptr, n_items, d, k_out, lam, ptr, None, None,
                                 None)

    assert call(C=2000) == -1 and b"C must be in [1, 1024]" in lib.dr_last_error()
    assert call(C=0) == -1
    assert call(k_out=101) == -1 and b"k_out must be" in lib.dr_last_error()
    assert call(C=200, k_out=129) == -1 and b"k_out must be" in lib.dr_last_error()
    assert call(k_out=0) == -1
    assert call(lam=1.5) == -1 and b"lambda must be in [0, 1]" in lib.dr_last_error()
    assert call(lam=float("nan")) == -1
    assert call(n_items=0) == -1 and b"empty item table" in lib.dr_last_error()
    assert call(d=100) == -2 and b"d must be 64 or 128" in lib.dr_last_error()
    assert call(ptr=None) == -1 and b"null pointer" in lib.dr_last_error()
    assert call(n_users=0, ptr=None) == 0  # no users: a no-op success
    assert call(n_users=0, C=2000) == -1


def _ranking_dataset(n_users=6, n_items=40):
    inter = torch.LongTensor([[u, (3 * u) % n_items] for u in range(n_users)])
    data = datasets.UserItemInteractionsDataset(inter, number_of_users=n_users,
                                                number_of_items=n_items)
    return datasets.RankingDataset(data)


def test_doors_validate_on_the_host():
    """Bad arguments raise ValueError before anything touches a device (the
    models here live on the CPU)."""
    mf = models.MatrixFactorization(6, 2000, 8)
    for kw in (dict(k=5, candidates=10, method="greedy"), dict(k=11, candidates=10),
               dict(k=5, candidates=1025), dict(k=0, candidates=10),
               dict(k=5, candidates=50, n_items=40)):  # candidates above the catalog
        with pytest.raises(ValueError):
            mf.recommend_diverse(**kw)
    rds = _ranking_dataset()
    mf = models.MatrixFactorization(6, 40, 8)
    for kw in (dict(number_of_recommendations=5, candidates=10, method="greedy"),
               dict(number_of_recommendations=11, candidates=10),
               dict(number_of_recommendations=5, candidates=1025)):
        with pytest.raises(ValueError):
            train.get_diverse_recommendations(rds, mf, **kw)
    with pytest.raises(ValueError, match="MatrixFactorization"):
        train.get_diverse_recommendations(rds, models.RandomModel(6, 40), 5, 10)

    class Tweaked(models.MatrixFactorization):  # its own forward: not the MF fast path
        def forward(self, *a, **kw):
            return super().forward(*a, **kw) * 2

    with pytest.raises(ValueError, match="MatrixFactorization"):
        train.get_diverse_recommendations(rds, Tweaked(6, 40, 8), 5, 10)
    with pytest.raises(ValueError, match="fewer than"):  # 40 items - 0 frozen < candidates asked
        train.get_diverse_recommendations(rds, mf, 45, 50)
