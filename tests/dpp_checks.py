"""CPU side of the DPP re-rank tests (dr_dpp_rerank, include/divrec_hip.h): the
spec as a float64 greedy, a float64 replay that judges a kernel's picks, a
float32 restatement of the kernel's basis form that measures fp32 against
float64, and the seeded inputs of tests/test_dpp_gpu.py. No GPU, no torch.

Tolerances of the replay:

* TOL_R bounds |r_fp32 - r_float64| of a residual. It is 10 x the worst
  difference the float32 restatement (``residual_error_f32``: the kernel's
  arithmetic, numpy's summation order) shows over every live candidate at every
  step on every input of tests/test_dpp_gpu.py, measured on the CPU by
  ``measure_tol_r`` (python tests/dpp_checks.py): 6.77e-7, at the d = 128,
  C = 1000, k_out = 100, lam = 0.5 shape (3.6e-7 to 6.8e-7 over the inputs). The
  factor 10 is for the kernel's different summation order at the same precision.
* TOL_V = 1e-4 bounds the value gap of a pick to the step's best value (the MMR
  tests' number). Every pick on these inputs has a float64 residual >= 0.05
  (``assert_inputs`` checks it; the smallest is 0.059, the last picks of the
  d = 128, k_out = 128, lam = 0 shape, and >= 0.116 on every other input), so an
  fp32 residual error of the measured size moves log r by at most 6.77e-7 /
  0.059 = 1.2e-5, and one of the whole TOL_R by 5.8e-5 at r >= 0.116.
"""
import numpy as np

import oracle

EPS = 1e-4       # DR_DPP_EPS
TOL_R = 6.77e-6  # 10 x 6.77e-7 (measure_tol_r, CPU)
TOL_V = 1e-4


def _unit_rows(cand, E):
    """(float64 unit rows [C, d], live [C]) of one user's candidates: empty
    slots (< 0), ids past the table and zero-norm rows are not live."""
    cand = np.asarray(cand, dtype=np.int64)
    live = (cand >= 0) & (cand < E.shape[0])
    X = E[np.where(live, cand, 0)].astype(np.float64)
    nrm = np.sqrt((X * X).sum(1))
    live &= nrm > 0
    X = X / np.where(nrm > 0, nrm, 1.0)[:, None]
    return X, live


def _value(lam, sc, r):
    return lam * np.asarray(sc, dtype=np.float64) + (1.0 - lam) * np.log(r)


class _Cholesky:
    """Incremental Cholesky of the cosine Gram of one user's candidates."""

    def __init__(self, X, k):
        self.X = X
        self.c = np.zeros((k, X.shape[0]))
        self.r = np.ones(X.shape[0])
        self.t = 0

    def pick(self, j):
        t = self.t
        e = (self.X @ self.X[j] - self.c[:t].T @ self.c[:t, j]) / np.sqrt(self.r[j])
        self.c[t] = e
        self.r = self.r - e * e
        self.t = t + 1


def dpp_greedy_f64(cand, sc, E, k, lam):
    """The spec in float64 for one user: (positions [k], resid [k], final r [C],
    live-and-unpicked [C]); position -1 / resid 0 once nobody is eligible."""
    X, live = _unit_rows(cand, E)
    ch = _Cholesky(X, k)
    pos = np.full(k, -1, dtype=np.int64)
    resid = np.zeros(k)
    for t in range(k):
        elig = live & (ch.r > EPS)
        if not elig.any():
            break
        val = np.where(elig, _value(lam, sc, np.where(elig, ch.r, 1.0)), -np.inf)
        j = int(np.argmax(val))  # the first maximum: the lowest position
        pos[t], resid[t] = j, ch.r[j]
        ch.pick(j)
        live[j] = False
    return pos, resid, ch.r, live


def dpp_check_positions(picks, resid, cand, sc, E, lam, tol_v=TOL_V, tol_r=TOL_R):
    """Float64 replay that follows the kernel's picks (item ids [n, k]) and
    residuals [n, k]; returns the number of bad picks. A pick must be a live
    candidate (the lowest live position holding that item) whose float64 value
    is within tol_v of the step's maximum, whose float64 residual is above
    eps - tol_r and within tol_r of the kernel's. A -1 is right only when no
    live candidate has a residual above eps + tol_r, and carries resid 0. The
    replay continues from the kernel's pick, so one near-tie does not cascade."""
    picks, resid = np.asarray(picks), np.asarray(resid)
    bad = 0
    for u in range(picks.shape[0]):
        X, live = _unit_rows(cand[u], E)
        ch = _Cholesky(X, picks.shape[1])
        for t in range(picks.shape[1]):
            it = int(picks[u, t])
            if it < 0:
                bad += int((live & (ch.r > EPS + tol_r)).any() or resid[u, t] != 0)
                continue
            at = np.flatnonzero(live & (np.asarray(cand[u]) == it))
            if at.size == 0:  # not a live candidate (or picked twice)
                bad += 1
                continue
            j = int(at[0])
            elig = live & (ch.r > EPS)
            best = _value(lam, sc[u], np.where(elig, ch.r, 1.0))[elig].max() if elig.any() else -np.inf
            rj = ch.r[j]
            ok = rj > EPS - tol_r and abs(float(resid[u, t]) - rj) <= tol_r
            ok = ok and _value(lam, sc[u][j], max(rj, 1e-300)) >= best - tol_v
            bad += int(not ok)
            ch.pick(j)
            live[j] = False
    return bad


def assert_inputs(cand, sc, E, k, lam):
    """The conditions under which TOL_V and the eligibility threshold can be
    judged, asserted on the float64 greedy of every user: no pick has a
    residual below 0.05, and no live candidate ends with a residual in
    [eps / 4, 4 eps]. A failure means the seed is wrong, not the kernel.
    Returns the greedy's (positions, resid) per user."""
    out = []
    for u in range(len(cand)):
        pos, resid, r, left = dpp_greedy_f64(cand[u], sc[u], E, k, lam)
        assert (resid[pos >= 0] >= 0.05).all(), (u, resid[pos >= 0].min())
        assert not ((r[left] >= EPS / 4) & (r[left] <= 4 * EPS)).any(), u
        out.append((pos, resid))
    return out


def judge(picks, resid, cand, sc, E, lam):
    """Input conditions, then the replay: the number of bad picks."""
    assert_inputs(cand, sc, E, np.asarray(picks).shape[1], lam)
    return dpp_check_positions(picks, resid, cand, sc, E, lam)


def residual_error_f32(pos, cand, E):
    """Float32 restatement of the kernel's basis form (unit rows, CGS2 against
    the basis, e_i = <b_t, x_i>, r_i -= e_i^2) following the picks ``pos`` of one
    user, beside the float64 Cholesky following the same picks: the worst
    |r32 - r64| over the live candidates and steps."""
    X64, live = _unit_rows(cand, E)
    ch = _Cholesky(X64, len(pos))
    f = np.float32
    rows = E[np.where(live, np.asarray(cand, dtype=np.int64), 0)].astype(f)
    nsq = (rows * rows).sum(1, dtype=f)
    inv = np.where(nsq > 0, f(1) / np.sqrt(np.where(nsq > 0, nsq, f(1))), f(0)).astype(f)
    r = np.ones(len(cand), dtype=f)
    B = np.zeros((len(pos), E.shape[1]), dtype=f)
    worst = 0.0
    for t, j in enumerate(pos):
        if j < 0:
            break
        v = rows[j] * inv[j]
        for _ in range(2):
            v = v - (B[:t] @ v) @ B[:t]
        invn = f(1) / np.sqrt((v * v).sum(dtype=f))
        B[t] = v * invn
        e = (rows @ v) * inv * invn
        r = r - e * e
        ch.pick(int(j))
        worst = max(worst, float(np.abs(r.astype(np.float64) - ch.r)[live].max()))
    return worst


# --------------------------------------------------------------------------- inputs
def _table(rng, ni, d, scale=1.0):
    return oracle.as_bf16_f32((rng.standard_normal((ni, d)) * scale).astype(np.float32))


def _lists(rng, ni, n, C):
    return np.stack([rng.choice(ni, C, replace=False) for _ in range(n)]).astype(np.int32)


def basic_inputs():
    """d = 128, 5000 items, 8 users, C = 300, N(0, 1) scores."""
    rng = np.random.default_rng(11)
    E = _table(rng, 5000, 128)
    return _lists(rng, 5000, 8, 300), rng.standard_normal((8, 300)).astype(np.float32), E


CONFIG5 = [(128, 1000, 100, 0.5), (128, 1024, 100, 0.9), (64, 777, 48, 0.3), (64, 1024, 64, 0.0),
           (128, 1000, 128, 0.0)]


def config5_inputs(d, C, n=12, ni=20000):
    """Config-5 shaped lists: rows N(0, 1/sqrt(d)), scores sorted descending."""
    rng = np.random.default_rng(1000 * d + C)
    E = _table(rng, ni, d, 1.0 / np.sqrt(d))
    sc = -np.sort(-rng.random((n, C)), axis=1).astype(np.float32)
    return _lists(rng, ni, n, C), sc, E


def tie_inputs():
    """d = 128, C = 1000: (lists of distinct items with all scores equal; lists
    of 100 items each repeated 10 times in a run, one score per item)."""
    rng = np.random.default_rng(31)
    E = _table(rng, 20000, 128, 1.0 / np.sqrt(128))
    flat = _lists(rng, 20000, 4, 1000)
    flat_sc = np.full((4, 1000), 0.25, dtype=np.float32)
    runs = np.repeat(_lists(rng, 20000, 4, 100), 10, axis=1)
    runs_sc = np.repeat(rng.random((4, 100)).astype(np.float32), 10, axis=1)
    return (flat, flat_sc), (runs, runs_sc), E


def exhaustion_inputs():
    """A d = 64 table of rank 8 (small integers in the first 8 columns)."""
    rng = np.random.default_rng(41)
    E = np.zeros((3000, 64), dtype=np.float32)
    E[:, :8] = rng.integers(-3, 4, size=(3000, 8))
    E[(E == 0).all(1), 0] = 1.0
    return _lists(rng, 3000, 4, 200), rng.standard_normal((4, 200)).astype(np.float32), E


def invalid_inputs():
    """The layout of test_mmr_rerank_invalid_candidates: d = 64, C = 200, user u
    with 35 u empty slots; one candidate of user 0 names a zero-norm row."""
    rng = np.random.default_rng(5)
    E = _table(rng, 3000, 64)
    cand = _lists(rng, 3000, 6, 200)
    for u in range(6):
        cand[u, rng.choice(200, 35 * u, replace=False)] = -1
    E[cand[0, 3]] = 0.0  # a zero-norm row: never eligible
    return cand, rng.standard_normal((6, 200)).astype(np.float32), E


def multi_user_inputs():
    """40 users, C = 777, d = 64, empty slots on later users."""
    rng = np.random.default_rng(61)
    E = _table(rng, 20000, 64, 1.0 / 8)
    cand = _lists(rng, 20000, 40, 777)
    for u in range(9, 40, 7):
        cand[u, rng.choice(777, 60, replace=False)] = -1
    sc = -np.sort(-rng.random((40, 777)), axis=1).astype(np.float32)
    return cand, sc, E


def measure_tol_r():
    """Worst |r32 - r64| of the float32 restatement over the GPU tests' inputs,
    following the float64 greedy's picks; also the smallest picked residual."""
    cases = [("basic lam=%.1f" % lam, basic_inputs(), 40, lam) for lam in (1.0, 0.7, 0.3)]
    cases += [("config5 %s" % (c,), config5_inputs(c[0], c[1]), c[2], c[3]) for c in CONFIG5]
    (flat, flat_sc), (runs, runs_sc), E = tie_inputs()
    cases += [("ties flat", (flat, flat_sc, E), 100, 1.0), ("ties runs", (runs, runs_sc, E), 100, 0.5)]
    cases += [("exhaustion", exhaustion_inputs(), 20, 0.5), ("invalid", invalid_inputs(), 40, 0.5),
              ("multi user", multi_user_inputs(), 48, 0.3)]
    worst_all = 0.0
    for name, (cand, sc, E), k, lam in cases:
        worst, rmin = 0.0, 1.0
        for u, (pos, resid) in enumerate(assert_inputs(cand, sc, E, k, lam)):
            worst = max(worst, residual_error_f32(pos, cand[u], E))
            rmin = min(rmin, resid[pos >= 0].min())
        print(f"{name:40s} worst |r32 - r64| = {worst:.2e}   min picked r64 = {rmin:.3f}")
        worst_all = max(worst_all, worst)
    print(f"worst over all inputs: {worst_all:.2e}")
    return worst_all


if __name__ == "__main__":
    measure_tol_r()
