"""topk_checks.exact_topk, the one exact top-k of the score-scan tests, pinned
to the CPU oracle (oracle.recommend_topk / oracle.topk_order) without a GPU:
7 users x 40 items, d = 8, integer tables in [-1, 1] (scores in [-8, 8]: many
ties), every rule of the function on its own.
"""
import numpy as np
import pytest

import oracle
from topk_checks import exact_topk, int_table

NU, NI, D = 7, 40, 8
KS = [1, 5, 40, 50]  # 50: longer than the catalog


def _tables():
    rng = np.random.default_rng(740)
    U, I = int_table(rng, NU, D, -1, 1), int_table(rng, NI, D, -1, 1)
    S = U @ I.T
    assert min(len(np.unique(r)) for r in S) < NI // 2  # tied scores in every row
    return U, I


def _padded(rows, k):
    """Per-user (items, scores) of any length <= k as exact_topk returns them."""
    outi = np.full((len(rows), k), -1, dtype=np.int64)
    outs = np.full((len(rows), k), -np.inf, dtype=np.float64)
    for r, (i, s) in enumerate(rows):
        outi[r, :len(i)], outs[r, :len(i)] = i, s
    return outi, outs


def _oracle_rows(U, I, k, frozen):
    rows = []
    for u in range(U.shape[0]):
        i, s = oracle.recommend_topk(U, I, k, users=[u], frozen=[frozen[u]], return_scores=True)
        rows.append((i[0], s[0]))
    return rows


def _check(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])


@pytest.mark.parametrize("k", KS)
def test_plain_lists_and_padding(k):
    U, I = _tables()
    ref_i, ref_s = oracle.recommend_topk(U, I, k, return_scores=True)
    assert ref_i.shape[1] == min(k, NI)
    _check(exact_topk(U, I, k, device="cpu"), _padded(list(zip(ref_i, ref_s)), k))


@pytest.mark.parametrize("k", KS)
def test_frozen_rows_of_length_0_1_39(k):
    U, I = _tables()
    rng = np.random.default_rng(741)
    frozen = [np.sort(rng.choice(NI, size=n, replace=False)) for n in (0, 1, 39, 1, 0, 39, 5)]
    best = int(np.argsort(-(I @ U[3]), kind="stable")[0])
    frozen[3] = np.array([best])  # the one frozen id is the user's first item
    _check(exact_topk(U, I, k, frozen=frozen, device="cpu"), _padded(_oracle_rows(U, I, k, frozen), k))


@pytest.mark.parametrize("k", KS)
def test_threshold_is_strict(k):
    """thr[u] is a score user u has (its 3rd best, tied with others): those
    items are not ranked; -inf ranks all, +inf none."""
    U, I = _tables()
    S = (U @ I.T).astype(np.float32)
    thr = np.sort(S, axis=1)[:, -3].copy()
    thr[1], thr[5] = -np.inf, np.inf
    assert all((S[u] == thr[u]).any() for u in (0, 2, 3, 4, 6))
    rows = []
    for u in range(NU):
        cands = np.nonzero(S[u] > thr[u])[0]
        o = oracle.topk_order(S[u, cands], k)
        rows.append((cands[o], S[u, cands][o]))
    assert any(0 < len(i) < min(k, NI) for i, _ in rows) or k == 1
    _check(exact_topk(U, I, k, thr=thr, device="cpu"), _padded(rows, k))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("per_user", [False, True])
def test_nan_item_row_dropped(k, per_user):
    U, I = _tables()
    I[13] = np.nan
    drop = np.zeros((NU, NI) if per_user else NI, dtype=bool)
    drop[..., 13] = True
    want = _padded(_oracle_rows(U, I, k, [[13]] * NU), k)
    assert not np.isin(13, want[0])
    _check(exact_topk(U, I, k, drop=drop, device="cpu"), want)


def test_torch_tables_and_blocks():
    """Torch tensors (bf16 holds these integers exactly) and a block size
    below the user count give the same lists."""
    import torch

    U, I = _tables()
    frozen = [[u, 39 - u] for u in range(NU)]
    want = exact_topk(U, I, 5, frozen=frozen, device="cpu")
    got = exact_topk(torch.from_numpy(U).to(torch.bfloat16), torch.from_numpy(I), 5, frozen=frozen,
                     device="cpu", block=3)
    _check(got, want)
