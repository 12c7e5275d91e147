"""MMR re-rank, host side: the checkers of tests/mmr_checks.py checked on the
CPU. The integer greedy against the fp32 restatement on every exact input of
tests/test_mmr_gpu.py, the conditions those inputs must meet to exercise the
kernel's tie paths, the float64 replay's own verdicts, and that the inputs with
special values tell the contract from the behaviour before it. No GPU."""
import numpy as np
import pytest

import mmr_checks as mc
from mmr_checks import mmr_check_positions, mmr_greedy_f32, mmr_greedy_f64, mmr_greedy_int


def _both(cand, sc, E, k, lam):
    """(positions, tie steps) per user, the fp32 restatement asserted equal."""
    out = []
    for u in range(len(cand)):
        pos, ties = mmr_greedy_int(cand[u], sc[u], E, k, lam)
        assert np.array_equal(pos, mmr_greedy_f32(cand[u], sc[u], E, k, lam)), u
        out.append((pos, ties))
    return out


@pytest.mark.parametrize("d,nnz,C,k,lam", mc.EXACT_SHAPES)
def test_integer_greedy_is_the_fp32_restatement_and_ties_often(d, nnz, C, k, lam):
    cand, sc, E = mc.exact_inputs(d, nnz, C)
    assert (E * E).sum(1).tolist() == [nnz] * len(E) and set(np.unique(E)) <= {-1.0, 0.0, 1.0}
    assert np.array_equal(np.rint(sc * 64) / 64, sc) and (sc >= 0).all() and (sc < 1).all()
    res = _both(cand, sc, E, k, lam)
    assert all((pos >= 0).all() and len(set(pos.tolist())) == k for pos, _ in res)
    if C > 1:  # a list of one has nothing to tie with
        assert 3 * sum(t for _, t in res) >= len(cand) * k
    if lam == 1.0:
        assert np.array_equal(np.stack([cand[u][res[u][0]] for u in range(len(cand))]),
                              mc.stable_topk(cand, sc, k))


@pytest.mark.parametrize("layout", ["tile", "repeat"])
@pytest.mark.parametrize("lam", [0.0, 0.5, 0.75])
def test_duplicate_inputs(layout, lam):
    cand, sc, E = mc.dup_inputs(layout)
    assert all(len(set(cand[u].tolist())) == 64 for u in range(3))
    wave_of = np.arange(1024) % 8  # wave w owns the positions = w (mod 8)
    for u in range(3):
        per_wave = [len(set(wave_of[cand[u] == it].tolist())) for it in cand[u, :64]]
        assert set(per_wave) == ({1} if layout == "tile" else {8})
    res = _both(cand, sc, E, 100, lam)
    assert all(3 * t >= 100 for _, t in res)


@pytest.mark.parametrize("d,lam", mc.FOLD_SHAPES)
def test_fold_inputs_need_both_passes(d, lam):
    """The first 64 picks are the positions below 64, every one of them at a
    value above what any of 64..71 had after the first pick (the batch's
    bounds: so one batch makes picks 2..64, 63 of them), and the last 8 are
    64..71 out of position order: their order is the fold's 63 cosines."""
    cand, sc, E = mc.fold_inputs(d)
    L = int(lam * 256)
    for u, (pos, _) in enumerate(_both(cand, sc, E, 72, lam)):
        assert sorted(pos[:64].tolist()) == list(range(64))
        tail = pos[64:].tolist()
        assert sorted(tail) == list(range(64, 72)) and tail != sorted(tail)
        _, _, values = mmr_greedy_int(cand[u], sc[u], E, 72, lam, trace=True)
        X = E[cand[u]].astype(np.int64)
        bound = (L * (-256) * 64 - (256 - L) * 64 * (X[64:] @ X[pos[0]])).max()
        assert min(values[1:64]) > bound
        # folding only the first pass of 32 picks would order the tail differently
        half = (X[64:] @ X[pos[:33]].T).max(1)
        full = (X[64:] @ X[pos[:64]].T).max(1)
        assert not np.array_equal(half, full)


def _float_user(seed=0):
    cand, sc, E = mc.float_inputs(32, 500, n=1)
    return cand, sc, E


def test_replay_accepts_the_greedy_and_rejects_what_is_wrong():
    cand, sc, E = _float_user()
    lam, k = 0.5, 40
    cand[0, [3, 17]] = -1
    pos = mmr_greedy_f64(cand[0], sc[0], E, k, lam)
    picks = mc.picks_of(cand[0], pos)[None]
    assert (picks >= 0).all()
    assert mmr_check_positions(picks, cand, sc, E, lam, mc.TOL_V) == 0
    assert mmr_check_positions(mc.picks_of(cand[0], mmr_greedy_f32(cand[0], sc[0], E, k, lam))[None],
                               cand, sc, E, lam, mc.TOL_V) == 0
    # two neighbouring picks of clearly different value swapped
    X = E[np.maximum(cand[0], 0)].astype(np.float64)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    pen = np.zeros(cand.shape[1])
    for t in range(k - 1):
        val = lam * sc[0] - (1 - lam) * pen
        if val[pos[t]] - val[pos[t + 1]] > 100 * mc.TOL_V:
            break
        sim = X @ X[pos[t]]
        pen = sim if t == 0 else np.maximum(pen, sim)
    else:
        raise AssertionError("no step with a clear gap: choose another seed")
    swapped = picks.copy()
    swapped[0, [t, t + 1]] = swapped[0, [t + 1, t]]
    assert mmr_check_positions(swapped, cand, sc, E, lam, mc.TOL_V) >= 1
    dead = picks.copy()  # a dead candidate: an id no live position holds
    dead[0, 5] = [i for i in range(mc.NI) if i not in set(cand[0].tolist())][0]
    assert mmr_check_positions(dead, cand, sc, E, lam, mc.TOL_V) >= 1
    twice = picks.copy()  # a repeated position
    twice[0, 6] = twice[0, 2]
    assert mmr_check_positions(twice, cand, sc, E, lam, mc.TOL_V) >= 1
    early = picks.copy()  # -1 while somebody is live
    early[0, -1] = -1
    assert mmr_check_positions(early, cand, sc, E, lam, mc.TOL_V) == 1


def test_replay_judges_the_end_of_a_short_list():
    cand, sc, E = _float_user()
    keep = cand[0, [4, 40, 400]].copy()
    cand[0] = -1
    cand[0, [4, 40, 400]] = keep
    pos = mmr_greedy_f64(cand[0], sc[0], E, 6, 0.5)
    assert (pos[:3] >= 0).all() and (pos[3:] == -1).all()
    picks = mc.picks_of(cand[0], pos)[None]
    assert mmr_check_positions(picks, cand, sc, E, 0.5, mc.TOL_V) == 0
    late = picks.copy()  # a live id after the live ones ran out
    late[0, 4] = keep[0]
    assert mmr_check_positions(late, cand, sc, E, 0.5, mc.TOL_V) == 1
    past = cand.copy()  # an id past the table is a dead slot, as -1 is
    past[0, 7] = E.shape[0] + 3
    assert mmr_check_positions(picks, past, sc, E, 0.5, mc.TOL_V) == 0


def test_replay_follows_the_contract():
    """A zero-norm row has cosine 0 and stays eligible; -inf and NaN scores
    count as -FLT_MAX: the replay accepts the contract's lists and rejects the
    lists of the behaviour before it."""
    cand, sc, E = mc.zero_norm_inputs()
    for lam in (1.0, 0.5):
        new = np.stack([mc.picks_of(cand[u], mmr_greedy_f32(cand[u], sc[u], E, 40, lam)) for u in range(3)])
        old = np.stack([mc.picks_of(cand[u], mmr_greedy_f32(cand[u], sc[u], E, 40, lam, zero_rule="old"))
                        for u in range(3)])
        assert mmr_check_positions(new, cand, sc, E, lam, mc.TOL_V) == 0
        assert mmr_check_positions(old, cand, sc, E, lam, mc.TOL_V) >= 3
    cand, sc, E = mc.nonfinite_inputs(20)
    new = np.stack([mc.picks_of(cand[u], mmr_greedy_f32(cand[u], sc[u], E, 20, 0.5)) for u in range(3)])
    assert mmr_check_positions(new, cand, sc, E, 0.5, mc.TOL_V) == 0
    old = np.stack([mc.picks_of(cand[u], mmr_greedy_f32(cand[u], sc[u], E, 20, 0.5, zero_rule="old"))
                    for u in range(3)])
    assert mmr_check_positions(old, cand, sc, E, 0.5, mc.TOL_V) >= 3


@pytest.mark.parametrize("lam", [1.0, 0.5])
def test_zero_norm_inputs_tell_the_rules_apart(lam):
    cand, sc, E = mc.zero_norm_inputs()
    assert ((E[cand[2, [3, 77, 200]]] == 0).all() and (E[cand[0, 5]] == 0).all()
            and (E[cand[1, 150]] == 0).all())
    for u in range(3):
        new = mmr_greedy_f32(cand[u], sc[u], E, 100, lam)
        assert np.array_equal(new, mmr_greedy_int(cand[u], sc[u], E, 100, lam)[0])
        assert not np.array_equal(new, mmr_greedy_f32(cand[u], sc[u], E, 100, lam, zero_rule="old"))
    assert mmr_greedy_f32(cand[0], sc[0], E, 100, lam)[0] == 5  # the zero row is the first pick
    assert 150 in mmr_greedy_f32(cand[1], sc[1], E, 100, lam)[1:].tolist()
    if lam == 1.0:
        got = np.stack([cand[u][mmr_greedy_f32(cand[u], sc[u], E, 100, lam)] for u in range(3)])
        assert np.array_equal(got, mc.stable_topk(cand, sc, 100))


@pytest.mark.parametrize("C", [20, 300])
@pytest.mark.parametrize("lam", [1.0, 0.5, 0.0])
def test_nonfinite_inputs_tell_the_rules_apart(C, lam):
    cand, sc, E = mc.nonfinite_inputs(C)
    assert np.isinf(sc[0]).any() and np.isnan(sc[1]).any() and np.isinf(sc[2]).any() and np.isnan(sc[2]).any()
    for u in range(3):
        new = mmr_greedy_f32(cand[u], sc[u], E, C, lam)
        assert sorted(new.tolist()) == list(range(C))  # nobody live is replaced by -1
        assert not np.array_equal(new, mmr_greedy_f32(cand[u], sc[u], E, C, lam, zero_rule="old"))
        clamped = np.flatnonzero(~np.isfinite(sc[u]))
        if lam > 0:  # the clamped ones come last, in position order
            assert np.array_equal(new[C - len(clamped):], clamped)
        else:  # they compete on the max term alone: one of them is among the early picks
            assert not np.array_equal(new[C - len(clamped):], clamped)


def test_independence_inputs_are_what_they_say():
    cand, sc, E = mc.independence_inputs()
    want = [mmr_greedy_f32(cand[u], sc[u], E, 100, 0.5) for u in range(7)]
    assert (want[2] == -1).all()
    assert sorted(want[4][:3].tolist()) == [9, 500, 1001] and (want[4][3:] == -1).all()
    assert want[1][0] == 130 and (E[cand[1, 130]] == 0).all()
    assert sorted(want[5][:60].tolist()) == list(range(60)) and want[5][60:].tolist() == list(range(60, 100))
    assert all((want[u] >= 0).all() for u in (0, 1, 3, 5, 6))


def test_value_gap_is_the_recorded_one():
    """TOL_V is at least 10 times the fp32 restatement's worst value gap; the
    figure in the module docstring is what measure_value_gap finds (one shape
    here, all of them with python tests/mmr_checks.py)."""
    assert mc.TOL_V == 1e-4 and mc.TOL_V >= 10 * mc.VALUE_GAP_F32
    d, C, k, lam = mc.FLOAT_SHAPES[1]
    cand, sc, E = mc.float_inputs(d, C)
    gap = max(mc.value_gap_f32(cand[u], sc[u], E, k, lam) for u in range(len(cand)))
    assert 0 < gap <= mc.VALUE_GAP_F32
