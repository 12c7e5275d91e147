"""History distance and serendipity re-rank, host side: the checkers of
tests/serendipity_checks.py admit the fp32 emulation of the kernels and reject
broken variants; the argument checks of the three C entries run before any HIP
call; the ValueErrors of ops, doors and metrics; NoveltyScore's item values by
hand; the existing re-rank doors are untouched. No GPU."""
import numpy as np
import pytest
import torch

import serendipity_checks as sc
from divrec import _backend, ops, train

BF16 = _backend.DR_BF16


def _case(C=40, d=64, integer=True):
    return sc.make_case(7, C, d, n_users=16, n_items=200, integer=integer)


@pytest.mark.parametrize("reduce", [sc.MIN, sc.MEAN])
@pytest.mark.parametrize("integer", [True, False])
def test_checker_admits_the_emulation(reduce, integer):
    lists, _, table, rowptr, hist = _case(integer=integer)
    lists[1, 5], lists[2, 7] = -1, 200  # an empty slot, an id past the table
    hist[rowptr[2]:rowptr[2] + 1] = 999  # a history entry past the table
    out = sc.emulate_distance(lists, table, rowptr, hist, reduce)
    sc.check_distance(out, lists, table, rowptr, hist, reduce)
    assert np.isnan(out[2, 7]) and out[1, 5] == 0 and not out[0].any()  # user 0: no history


@pytest.mark.parametrize("reduce,variant", [(sc.MIN, "max"), (sc.MEAN, "raw_len"),
                                            (sc.MIN, "empty_nan"), (sc.MEAN, "empty_nan"),
                                            (sc.MIN, "zero_norm_0"), (sc.MEAN, "zero_norm_0")])
def test_checker_rejects_broken_distances(reduce, variant):
    lists, _, table, rowptr, hist = _case()
    hist[rowptr[3]:rowptr[3] + 40] = -5  # invalid entries: the raw length is not the valid count
    if variant == "zero_norm_0":  # a user whose whole history is the zero row: every distance is 1
        hist[rowptr[1]:rowptr[2]] = sc.ZERO_ROWS[0]
    out = sc.emulate_distance(lists, table, rowptr, hist, reduce, variant=variant)
    with pytest.raises(AssertionError):
        sc.check_distance(out, lists, table, rowptr, hist, reduce)


def test_zero_norm_rows_have_distance_one():
    lists, _, table, rowptr, hist = _case()
    out = sc.emulate_distance(lists, table, rowptr, hist, sc.MEAN)
    ref = sc.reference_distance(lists, table, rowptr, hist, sc.MEAN)
    with_hist = np.diff(rowptr) > 0
    assert (out[with_hist, 2] == 1).all() and (ref[with_hist, 2] == 1).all()


def test_fma_emulation_is_one_rounding():
    a = np.float32(1 + 2.0 ** -12)  # a * a = 1 + 2^-11 + 2^-24: the fp32 product drops the last term
    c = -np.float32(1 + 2.0 ** -11)
    assert sc.fma32(a, a, c) == np.float32(2.0 ** -24)
    assert np.float32(a * a) + c == 0


@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
def test_rerank_checker_admits_and_rejects(lam):
    lists, scores, table, rowptr, hist = _case(C=40)
    lists[4, 9], lists[5, 3] = -1, 500
    dist = sc.emulate_distance(lists, table, rowptr, hist, sc.MIN)
    items, od = sc.expected_rerank(lists, scores, dist, 200, lam, 10)
    sc.check_rerank(items, od, lists, scores, dist, 200, lam, 10)
    assert 500 not in items and -1 not in items  # neither is live, 38 others are
    if lam == 1.0:  # the stable order by score
        live = (lists[0] >= 0) & (lists[0] < 200)
        order = np.flatnonzero(live)[np.argsort(-scores[0][live].astype(np.float64), kind="stable")]
        assert np.array_equal(items[0], lists[0][order[:10]])
    high, hd = sc.expected_rerank(lists, scores, dist, 200, lam, 40, variant="ties_high")
    with pytest.raises(AssertionError):
        sc.check_rerank(high, hd, lists, scores, dist, 200, lam, 40)
    # fewer live candidates than k_out end in -1 with distance 0
    few = np.full_like(lists, -1)
    few[:, :3] = lists[:, :3]
    items, od = sc.expected_rerank(few, scores, dist, 200, lam, 10)
    assert (items[:, 3:] == -1).all() and not od[:, 3:].any()


def test_rerank_checker_rejects_a_fused_blend():
    """Among 1000 close values a fused blend orders some pair differently."""
    rng = np.random.default_rng(11)
    n, C = 8, 1000
    items = np.tile(np.arange(C, dtype=np.int32), (n, 1))
    scores = (1 + rng.integers(0, 4096, (n, C)) * 2.0 ** -12).astype(np.float32)
    dist = (1 + rng.integers(0, 4096, (n, C)) * 2.0 ** -12).astype(np.float32)
    lam = 0.3
    plain = sc.expected_rerank(items, scores, dist, C, lam, C)
    fused = sc.expected_rerank(items, scores, dist, C, lam, C, variant="fma")
    assert not np.array_equal(plain[0], fused[0])
    sc.check_rerank(*plain, items, scores, dist, C, lam, C)
    with pytest.raises(AssertionError):
        sc.check_rerank(*fused, items, scores, dist, C, lam, C)


def test_c_entries_check_arguments_before_any_hip_call():
    lib = _backend.load_library()
    err = lambda: lib.dr_last_error()  # noqa: E731
    hd = lambda n, C, ni, d, red: lib.dr_history_distance(  # noqa: E731
        None, n, C, None, ni, d, None, None, red, None, None, None)
    rr = lambda n, C, ni, d, red, k, lam: lib.dr_serendipity_rerank(  # noqa: E731
        None, None, n, C, None, ni, d, None, None, red, k, lam, None, None, None, None)
    for C in (0, 1025):
        assert hd(4, C, 10, 128, 0) == -1 and b"C must be in [1, 1024]" in err()
        assert rr(4, C, 10, 128, 0, 1, 0.5) == -1 and b"C must be in [1, 1024]" in err()
    assert rr(4, 100, 10, 128, 0, 101, 0.5) == -1 and b"k_out must be in [1, C]" in err()
    assert rr(4, 100, 10, 128, 0, 0, 0.5) == -1 and b"k_out" in err()
    for lam in (-0.1, 1.5, float("nan")):
        assert rr(4, 100, 10, 128, 0, 10, lam) == -1 and b"lambda must be in [0, 1]" in err()
    for d in (0, 16, 48, 512):
        assert hd(4, 100, 10, d, 0) == -2 and b"d must be one of 32, 64, 128, 256" in err()
        assert rr(4, 100, 10, d, 0, 10, 0.5) == -2 and b"d must be one of" in err()
    assert hd(4, 100, 10, 128, 2) == -1 and b"reduce must be" in err()
    assert hd(-1, 100, 10, 128, 0) == -1 and b"n_users" in err()
    assert hd(4, 100, 0, 128, 0) == -1 and b"empty item table" in err()
    assert rr(4, 100, 0, 128, 1, 10, 0.5) == -1 and b"empty item table" in err()
    assert hd(4, 100, 10, 128, 0) == -1 and b"null pointer" in err()
    assert rr(4, 100, 10, 128, 0, 10, 0.5) == -1 and b"null pointer" in err()
    # no users: a no-op success, whatever the pointers
    assert hd(0, 100, 10, 128, 1) == 0 and rr(0, 100, 10, 64, 0, 10, 1.0) == 0
    lm = lambda dt, n, k, ni: lib.dr_list_item_mean(None, dt, n, k, None, ni, None, None, None)  # noqa: E731
    assert lm(0, 4, 10, 10) == -1 and b"DR_I32 or DR_I64" in err()
    assert lm(_backend.DR_I32, -1, 10, 10) == -1 and lm(_backend.DR_I32, 4, -1, 10) == -1
    assert lm(_backend.DR_I64, 4, 10, 10) == -1 and b"null pointer" in err()
    assert lm(_backend.DR_I64, 0, 10, 10) == 0


def test_ops_exist_and_existing_doors_are_unchanged():
    for name in ("history_distance", "serendipity_rerank", "list_item_mean"):
        assert callable(getattr(ops, name))
    assert ops.HISTORY_WIDTHS == (32, 64, 128, 256) and ops.HISTORY_MAX_C == 1024
    assert train.utils.RERANKERS == ("dpp", "mmr", "calibrated", "xquad")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_ops_fail_loudly_without_gpu():
    t = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.history_distance(torch.zeros(2, 3, dtype=torch.int32), t,
                             torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))


def test_novelty_item_values_by_hand():
    """Five items seen by 4, 2, 1, 1 and 0 of 4 users. Self-information is
    -log2(pop / n_users) with an unseen item counted as pop = 1; the popularity
    complement 1 - pop / max pop. The per-list mean of the restatement follows."""
    from divrec import metrics
    pop = torch.tensor([4, 2, 1, 1, 0], dtype=torch.int32)
    info = metrics.novelty_item_values(pop, 4, "self_information")
    assert info.dtype == torch.float32 and info.tolist() == [0.0, 1.0, 2.0, 2.0, 2.0]
    comp = metrics.novelty_item_values(pop, 4, "popularity_complement")
    assert comp.tolist() == [0.0, 0.5, 0.75, 0.75, 1.0]
    assert metrics.novelty_item_values(torch.zeros(3), 4, "popularity_complement").tolist() == [1, 1, 1]
    with pytest.raises(ValueError, match="kind must be one of"):
        metrics.novelty_item_values(pop, 4, "rarity")
    recs = np.array([[0, 1, 2], [4, -1, 9], [-1, -1, -1]])
    assert sc.reference_list_item_mean(recs, info.numpy()).tolist() == [1.0, 2.0, 0.0]


def test_relevance_flags():
    from divrec import metrics
    inter = torch.LongTensor([[0, 3], [0, 5], [1, 3], [2, 0], [0, 3]])
    recs = torch.LongTensor([[3, 4, 5], [5, 3, -1], [0, 9, 1]])
    flags = metrics.relevance_flags(inter, recs, 6)  # item 9 is outside the catalog
    assert flags.tolist() == [[True, False, True], [False, True, False], [True, False, False]]
    assert not metrics.relevance_flags(torch.zeros((0, 2), dtype=torch.int64), recs, 6).any()


def _ranking_dataset(n_users=6, n_items=40, frozen=True):
    from divrec import datasets
    inter = torch.LongTensor([[u, (3 * u) % n_items] for u in range(n_users)])
    data = datasets.UserItemInteractionsDataset(inter, number_of_users=n_users,
                                                number_of_items=n_items)
    fr = None
    if frozen:
        fr = datasets.UserItemInteractionsDataset(
            torch.LongTensor([[u, (5 * u + 1) % n_items] for u in range(n_users)]),
            number_of_users=n_users, number_of_items=n_items)
    return datasets.RankingDataset(data, frozen=fr)


def test_doors_validate_on_the_host():
    """Bad arguments raise ValueError before anything touches a device."""
    from divrec import models
    mf = models.MatrixFactorization(6, 40, 8)
    rowptr, items = torch.zeros(7, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    with pytest.raises(ValueError, match="history must be a CSR"):
        mf.recommend_serendipitous(5, 10, (rowptr[:5], items))
    with pytest.raises(ValueError, match="history must be a CSR"):
        mf.recommend_serendipitous(5, 10, (rowptr, items.view(0, 1)))
    with pytest.raises(ValueError, match="history must be a CSR"):
        mf.recommend_serendipitous(5, 10, rowptr)
    with pytest.raises(ValueError, match="history must be a CSR"):  # one row per listed user
        mf.recommend_serendipitous(5, 10, (rowptr, items), user_ids=torch.arange(3))
    with pytest.raises(ValueError, match="need 1 <= k <= candidates"):
        mf.recommend_serendipitous(11, 10, (rowptr, items))
    with pytest.raises(ValueError, match="need 1 <= k <= candidates"):
        mf.recommend_serendipitous(5, 41, (rowptr, items))
    with pytest.raises(ValueError, match="lam must be in"):
        mf.recommend_serendipitous(5, 10, (rowptr, items), lam=1.5)
    with pytest.raises(ValueError, match="reduce must be"):
        mf.recommend_serendipitous(5, 10, (rowptr, items), reduce="max")
    with pytest.raises(ValueError, match="user_ids must be None"):
        mf.recommend_serendipitous(5, 10, (rowptr, items), user_ids=torch.arange(6),
                                   user_vectors=torch.zeros(6, 8))
    assert hasattr(models.FeatureMatrixFactorization, "recommend_serendipitous")
    with pytest.raises(ValueError, match="frozen interactions: the dataset has none"):
        train.get_serendipitous_recommendations(_ranking_dataset(frozen=False), mf, 5, 10)
    with pytest.raises(ValueError, match="needs a MatrixFactorization"):
        train.get_serendipitous_recommendations(_ranking_dataset(), models.RandomModel(6, 40), 5, 10)
    with pytest.raises(ValueError, match="needs a MatrixFactorization"):  # too few item rows
        train.get_serendipitous_recommendations(_ranking_dataset(n_items=50), mf, 5, 10)
    with pytest.raises(ValueError, match="number_of_recommendations <= candidates"):
        train.get_serendipitous_recommendations(_ranking_dataset(), mf, 20, 10)


def test_metrics_validate_on_the_host():
    from divrec import metrics, models
    data = _ranking_dataset().data
    with pytest.raises(ValueError, match="kind must be one of"):
        metrics.NoveltyScore(dataset=data, kind="rarity")
    with pytest.raises(ValueError, match="exactly one of item_table and model"):
        metrics.UnexpectednessScore(dataset=data)
    with pytest.raises(ValueError, match="exactly one of item_table and model"):
        metrics.UnexpectednessScore(dataset=data, item_table=torch.zeros(40, 8),
                                    model=models.MatrixFactorization(6, 40, 8))
    with pytest.raises(ValueError, match="item_embeddings"):
        metrics.SerendipityScore(dataset=data, model=models.RandomModel(6, 40))
    with pytest.raises(ValueError, match="reduce must be"):
        metrics.UnexpectednessScore(dataset=data, item_table=torch.zeros(40, 8), reduce="max")
    score = metrics.UnexpectednessScore(dataset=data, item_table=torch.zeros(30, 8))
    with pytest.raises(ValueError, match="item table must be"):
        score._rows()
    ok = metrics.SerendipityScore(dataset=data, item_table=torch.zeros(40, 8), reduce="mean",
                                  reduction="none")
    assert ok.hist_reduce == "mean" and ok.reduction == "none" and ok.history is data
