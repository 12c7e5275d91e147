"""dr_mmr_rerank on the GPU (ops.mmr_rerank) against tests/mmr_checks.py. On the
exact inputs (entries in {-1, 0, +1}, scores a / 64, lam a multiple of 1 / 4:
every value exact in fp32) the lists must equal the integer greedy's element for
element, ties to the lowest position included: no tolerance, every user. The
special values of the contract (zero-norm rows, -inf and NaN scores) against
the fp32 restatement under the contract. Float inputs at shapes no other test
runs against the float64 replay at TOL_V."""
import numpy as np
import pytest
import torch

import mmr_checks as mc
from divrec import _backend, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _run(cand, sc, E, k, lam):
    out = ops.mmr_rerank(torch.from_numpy(cand).to(DEV), torch.from_numpy(sc).to(DEV),
                         torch.from_numpy(E).to(DEV).to(torch.bfloat16), k, lam)
    assert out.dtype == torch.int32 and out.shape == (cand.shape[0], k)
    return out.cpu().numpy()


def _want_int(cand, sc, E, k, lam):
    return np.stack([mc.picks_of(cand[u], mc.mmr_greedy_int(cand[u], sc[u], E, k, lam)[0])
                     for u in range(len(cand))])


def _want_f32(cand, sc, E, k, lam):
    return np.stack([mc.picks_of(cand[u], mc.mmr_greedy_f32(cand[u], sc[u], E, k, lam))
                     for u in range(len(cand))])


def _assert_lists(got, want):
    for u in range(len(want)):
        at = np.flatnonzero(got[u] != want[u])
        assert at.size == 0, (f"user {u}: first difference at pick {at[0]}: got "
                              f"{got[u, at[0]:at[0] + 4]}, want {want[u, at[0]:at[0] + 4]}")


@pytest.mark.parametrize("d,nnz,C,k,lam", mc.EXACT_SHAPES)
def test_mmr_exact_shapes(d, nnz, C, k, lam):
    cand, sc, E = mc.exact_inputs(d, nnz, C)
    got = _run(cand, sc, E, k, lam)
    _assert_lists(got, _want_int(cand, sc, E, k, lam))
    if lam == 1.0:
        assert np.array_equal(got, mc.stable_topk(cand, sc, k))


@pytest.mark.parametrize("d,lam", mc.FOLD_SHAPES)
def test_mmr_two_pass_fold(d, lam):
    """One batch of 63 picks, folded in passes of 32 + 31; the order of the
    last 8 picks is the fold's result (tests/test_mmr_host.py)."""
    cand, sc, E = mc.fold_inputs(d)
    _assert_lists(_run(cand, sc, E, 72, lam), _want_int(cand, sc, E, 72, lam))


@pytest.mark.parametrize("layout", ["tile", "repeat"])
@pytest.mark.parametrize("lam", [0.0, 0.5, 0.75])
def test_mmr_forced_picks_and_bound_ties(layout, lam):
    cand, sc, E = mc.dup_inputs(layout)
    _assert_lists(_run(cand, sc, E, 100, lam), _want_int(cand, sc, E, 100, lam))


def test_mmr_exact_prefetched_users():
    """7 users on two workgroups: all but each workgroup's first are prefetched."""
    d, nnz, C, k, lam = mc.EXACT_SHAPES[1]
    cand, sc, E = mc.exact_inputs(d, nnz, C, n=7)
    free = _run(cand, sc, E, k, lam)
    with _backend.plan_knobs(scan_slots=2):
        capped = _run(cand, sc, E, k, lam)
    want = _want_int(cand, sc, E, k, lam)
    _assert_lists(capped, want)
    _assert_lists(free, want)


@pytest.mark.parametrize("lam", [1.0, 0.5])
def test_mmr_zero_norm_rows(lam):
    """A zero row has cosine 0 with every row and stays eligible on its score:
    as a first pick, in the middle, three at once."""
    cand, sc, E = mc.zero_norm_inputs()
    got = _run(cand, sc, E, 100, lam)
    _assert_lists(got, _want_f32(cand, sc, E, 100, lam))
    _assert_lists(got, _want_int(cand, sc, E, 100, lam))
    if lam == 1.0:
        assert np.array_equal(got, mc.stable_topk(cand, sc, 100))


@pytest.mark.parametrize("C", [20, 300])  # without and with bounds
@pytest.mark.parametrize("lam", [1.0, 0.5, 0.0])
def test_mmr_nonfinite_scores(C, lam):
    """-inf and NaN scores count as -FLT_MAX: live, never replaced by -1; at
    lam > 0 they come last in position order, at lam = 0 they compete on the
    max term alone."""
    cand, sc, E = mc.nonfinite_inputs(C)
    got = _run(cand, sc, E, C, lam)
    assert (got >= 0).all()
    _assert_lists(got, _want_f32(cand, sc, E, C, lam))
    if lam > 0:
        for u in range(3):
            clamped = np.flatnonzero(~np.isfinite(sc[u]))
            assert np.array_equal(got[u, C - len(clamped):], cand[u][clamped])


def test_mmr_users_of_a_workgroup_are_independent():
    """Workgroup 0: full, all -1, three live candidates, full; workgroup 1: a
    zero-norm first pick, full, a -inf tail. Every list equals the list of a
    call with that user alone."""
    cand, sc, E = mc.independence_inputs()
    with _backend.plan_knobs(scan_slots=2):
        got = _run(cand, sc, E, 100, 0.5)
    for u in range(7):
        alone = _run(cand[u:u + 1], sc[u:u + 1], E, 100, 0.5)
        assert np.array_equal(got[u], alone[0]), u
    _assert_lists(got, _want_f32(cand, sc, E, 100, 0.5))


@pytest.mark.parametrize("d,C,k,lam", mc.FLOAT_SHAPES)
def test_mmr_float_replay(d, C, k, lam):
    cand, sc, E = mc.float_inputs(d, C)
    got = _run(cand, sc, E, k, lam)
    assert mc.mmr_check_positions(got, cand, sc, E, lam, mc.TOL_V) == 0
    assert all(len(set(got[u].tolist())) == k for u in range(len(cand)))
