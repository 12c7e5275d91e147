"""dr_dpp_rerank on the GPU (ops.dpp_rerank and the model / train doors) against
the float64 replay of tests/dpp_checks.py: every pick a valid greedy step within
TOL_V, every residual within TOL_R (both derived there), and the exact
properties of the spec: ties to the lowest position, lam = 1 the stable top-k,
lists that end in -1 when nobody is eligible."""
import numpy as np
import pytest
import torch

import dpp_checks as dc
from divrec import _backend, datasets, models, ops, train

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bf16(x):
    return torch.from_numpy(x).to(DEV).to(torch.bfloat16)


def _run(cand, sc, E, k, lam, check=True):
    items, resid = ops.dpp_rerank(torch.from_numpy(cand).to(DEV), torch.from_numpy(sc).to(DEV),
                                  _bf16(E), k, lam, check=check)
    assert items.dtype == torch.int32 and resid.dtype == torch.float32
    assert items.shape == resid.shape == (cand.shape[0], k)
    return items.cpu().numpy(), resid.cpu().numpy()


def _stable_topk(cand, sc, k):
    order = np.argsort(-sc, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(cand, order, axis=1)


@pytest.mark.parametrize("lam", [1.0, 0.7, 0.3])
def test_dpp_rerank_basic(lam):
    cand, sc, E = dc.basic_inputs()
    got, resid = _run(cand, sc, E, 40, lam)
    assert dc.judge(got, resid, cand, sc, E, lam) == 0
    if lam == 1.0:
        assert np.array_equal(got, _stable_topk(cand, sc, 40))


@pytest.mark.parametrize("d,C,kout,lam", dc.CONFIG5)
def test_dpp_rerank_config5_shapes(d, C, kout, lam):
    """C not a multiple of 32, the maximum C, k_out = d and k_out = 128."""
    cand, sc, E = dc.config5_inputs(d, C)
    got, resid = _run(cand, sc, E, kout, lam)
    assert dc.judge(got, resid, cand, sc, E, lam) == 0
    if lam == 0.0:  # r starts at exactly 1: an exact tie that position 0 wins
        assert np.array_equal(got[:, 0], cand[:, 0]) and (resid[:, 0] == 1.0).all()


def test_dpp_rerank_ties():
    (flat, flat_sc), (runs, runs_sc), E = dc.tie_inputs()
    got, _ = _run(flat, flat_sc, E, 100, 1.0)  # equal scores: positions 0..99 in order
    assert np.array_equal(got, flat[:, :100])
    got, resid = _run(runs, runs_sc, E, 100, 0.5)
    assert dc.judge(got, resid, runs, runs_sc, E, 0.5) == 0
    # 100 distinct items: the copies of a pick fall to residual 0 with it and
    # are never eligible. The replay above resolves each pick to the lowest
    # live position of its item, the first of its run (the copies are equal in
    # row and score, so the output's item ids cannot tell them apart), and the
    # float64 greedy itself picks only first positions on this input.
    for u in range(runs.shape[0]):
        assert len(set(got[u].tolist())) == 100 and (got[u] >= 0).all()
        assert (dc.dpp_greedy_f64(runs[u], runs_sc[u], E, 100, 0.5)[0] % 10 == 0).all()


def test_dpp_rerank_rank_exhaustion():
    cand, sc, E = dc.exhaustion_inputs()
    got, resid = _run(cand, sc, E, 20, 0.5)
    assert (got[:, :8] >= 0).all() and (got[:, 8:] == -1).all()
    assert (resid[:, :8] > 0.05).all() and (resid[:, 8:] == 0).all()
    assert dc.judge(got, resid, cand, sc, E, 0.5) == 0


def test_dpp_rerank_invalid_candidates():
    cand, sc, E = dc.invalid_inputs()
    kout = 40
    got, resid = _run(cand, sc, E, kout, 0.5)
    assert dc.judge(got, resid, cand, sc, E, 0.5) == 0
    assert got[0, :].tolist().count(int(cand[0, 3])) == 0  # the zero-norm row
    for u in range(cand.shape[0]):
        n_live = int(dc._unit_rows(cand[u], E)[1].sum())  # ids >= 0 with a non-zero row
        assert (got[u, :min(n_live, kout)] >= 0).all()
        assert (got[u, n_live:] == -1).all() and (resid[u, n_live:] == 0).all()
    bad = cand.copy()
    bad[2, 7] = E.shape[0] + 5  # an id past the table
    with pytest.raises(IndexError):
        _run(bad, sc, E, kout, 0.5)
    got, resid = _run(bad, sc, E, kout, 0.5, check=False)
    assert not (got == E.shape[0] + 5).any()
    assert dc.dpp_check_positions(got, resid, bad, sc, E, 0.5) == 0


def test_dpp_rerank_several_users_per_workgroup():
    cand, sc, E = dc.multi_user_inputs()
    lam, kout = 0.3, 48
    got, resid = _run(cand, sc, E, kout, lam)
    with _backend.plan_knobs(scan_slots=4):  # 10 users per workgroup
        got4, resid4 = _run(cand, sc, E, kout, lam)
    assert np.array_equal(got, got4) and np.array_equal(resid, resid4)
    users = np.concatenate([np.arange(6), np.random.default_rng(7).choice(np.arange(6, 40), 6,
                                                                          replace=False), [9, 37]])
    assert dc.judge(got4[users], resid4[users], cand[users], sc[users], E, lam) == 0


def test_dpp_rerank_width_padding():
    rng = np.random.default_rng(71)
    E = dc._table(rng, 4000, 100)
    cand, sc = dc._lists(rng, 4000, 5, 250), rng.standard_normal((5, 250)).astype(np.float32)
    c, s = torch.from_numpy(cand).to(DEV), torch.from_numpy(sc).to(DEV)
    a = ops.dpp_rerank(c, s, _bf16(E), 30, 0.5)
    b = ops.dpp_rerank(c, s, ops.pad_columns(_bf16(E), 128), 30, 0.5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    empty = ops.dpp_rerank(c[:0], s[:0], _bf16(E), 30, 0.5)
    assert empty[0].shape == (0, 30) and empty[1].shape == (0, 30)


# --------------------------------------------------------------------------- doors
N_USERS, N_ITEMS, D = 943, 1682, 32


@pytest.fixture(scope="module")
def door():
    rng = np.random.default_rng(81)
    mf = models.MatrixFactorization(N_USERS, N_ITEMS, D)
    with torch.no_grad():
        mf.user_embeddings.weight.copy_(torch.from_numpy(
            rng.standard_normal((N_USERS, D)).astype(np.float32)))
        mf.item_embeddings.weight.copy_(torch.from_numpy(
            rng.standard_normal((N_ITEMS, D)).astype(np.float32)))
    mf = mf.to(DEV)
    frozen = torch.from_numpy(np.stack([np.repeat(np.arange(N_USERS), 20),
                                        rng.integers(0, N_ITEMS, 20 * N_USERS)], axis=1))
    frozen = torch.unique(frozen, dim=0)
    test = torch.from_numpy(np.stack([np.arange(N_USERS), rng.integers(0, N_ITEMS, N_USERS)], 1))
    mk = lambda x: datasets.UserItemInteractionsDataset(x, number_of_users=N_USERS,  # noqa: E731
                                                        number_of_items=N_ITEMS)
    return mf, datasets.RankingDataset(mk(test), frozen=mk(frozen)), frozen.numpy()


@pytest.mark.parametrize("method", ["dpp", "mmr"])
def test_recommend_diverse_is_the_hand_composition(door, method):
    mf, rds, frozen = door
    excl = rds.exclusion_csr()
    items, scores = mf.recommend_diverse(20, 200, method=method, lam=0.4, exclude=excl)
    assert items.dtype == torch.int64 and items.shape == scores.shape == (N_USERS, 20)
    cand, cand_sc = mf.score_topk(200, exclude=excl)
    table = mf.bf16_tables()[1]
    if method == "dpp":
        want = ops.dpp_rerank(cand.to(torch.int32), cand_sc, table, 20, 0.4)[0]
    else:
        want = ops.mmr_rerank(cand.to(torch.int32), cand_sc, table, 20, 0.4)
    assert torch.equal(items, want.to(torch.int64)) and bool((items >= 0).all())
    # the scores are the picks' scan scores
    at = (cand[:, None, :] == items[:, :, None]).to(torch.int64).argmax(dim=2)
    assert torch.equal(scores, cand_sc.gather(1, at))
    got = items.cpu().numpy()
    banned = set(map(tuple, frozen.tolist()))
    assert not any((u, int(i)) in banned for u in range(N_USERS) for i in got[u])


@pytest.mark.parametrize("method", ["dpp", "mmr"])
def test_get_diverse_recommendations(door, method):
    mf, rds, _ = door
    top = train.get_model_recommendations(rds, mf, 20)
    same = train.get_diverse_recommendations(rds, mf, 20, 200, method=method, lam=1.0)
    assert same.dtype == torch.int64 and same.device.type == "cpu"
    assert torch.equal(same, top)  # lam = 1: relevance alone, the plain top-k
    div = train.get_diverse_recommendations(rds, mf, 20, 200, method=method, lam=0.3)
    table = mf.bf16_tables()[1]
    ild = lambda r: float(ops.ild_embedding(r.to(DEV), table, "cosine").mean())  # noqa: E731
    assert ild(div) > ild(top)  # the re-ranker's purpose, as a property
