"""CPU side of the xQuAD re-rank tests (dr_xquad_rerank, dr_aspect_profile,
dr_aspect_coverage; include/divrec_hip.h): the spec as a float64 greedy, a
float64 replay that judges a kernel's picks step by step, a float32
restatement of the kernel's arithmetic that measures fp32 against float64, and
the seeded inputs of tests/test_xquad_gpu.py. No GPU, no torch. Every function
works on all users of an input at once.

TOL_V bounds |value_fp32 - value_float64| of a candidate's value
lam * s + (1 - lam) * sum_a m_a c_a, TOL_COV the same for a list's coverage
sum_a (p_a - m_a). Each is 10 x the worst difference that the float32
restatement (``F32State``: the kernel's operations one by one, csrc/xquad.hip:
the profile's pairwise tree sum, div summed once in aspect order, then per pick
and covered aspect delta = m c, m -= delta, div -= delta c, cov += delta, no
fused multiply-add) shows on the float64 greedy's picks: for the value over
every live candidate at every step, for the coverage at every step, of every
input of tests/test_xquad_gpu.py (``measure_tol``; python tests/xquad_checks.py):

    input                         value      coverage
    basic lam = 1.0               0.00e+00   1.56e-07
    basic lam = 0.5               3.80e-08   2.38e-07
    basic lam = 0.0               2.38e-08   1.30e-07
    shape (1, 1, 1)               2.98e-08   0.00e+00
    shape (63, 63, 2)             5.11e-08   3.01e-07
    shape (65, 10, 64)            3.05e-08   4.57e-08
    shape (257, 40, 19)           3.61e-08   4.26e-07
    shape (1024, 128, 32)         3.29e-08   2.40e-07
    shape (512, 100, 64)          2.95e-08   3.42e-07
    shape (1000, 100, 3)          4.47e-08   0.00e+00
    ties                          0.00e+00   0.00e+00
    profiles                      5.96e-08   1.99e-08
    aspect values                 6.70e-08   1.19e-07
    invalid                       7.46e-08   5.96e-08
    many users                    1.31e-07   1.56e-07
    door                          7.69e-08   2.21e-07

The factor 10 covers what the restatement does not see. The replay allows a
pick 2 x TOL_V below the step's float64 maximum (the pick's and the best
candidate's fp32 values are each off by up to TOL_V) and out_cov TOL_COV around
the float64 coverage; it leaves no step and no user out.
"""
import functools

import numpy as np

from calibration_checks import normalise  # the profile rules are the calibrated re-rank's

MAX_ASPECTS = 64    # DR_XQUAD_MAX_ASPECTS
MAX_CELLS = 32768   # DR_XQUAD_MAX_CELLS
TOL_V = 1.31e-6     # 10 x 1.31e-7 (measure_tol, CPU)
TOL_COV = 4.26e-6   # 10 x 4.26e-7 (measure_tol, CPU)
FLT_MAX = float(np.finfo(np.float32).max)


class Case:
    """One input of dr_xquad_rerank: cand int32 [n, C], sc fp32 [n, C], aspects
    fp32 [n_items, G], profile fp32 [n, G], k picks at trade-off lam."""

    def __init__(self, cand, sc, aspects, profile, k, lam, name=""):
        self.cand = np.ascontiguousarray(cand, dtype=np.int32)
        self.sc = np.ascontiguousarray(sc, dtype=np.float32)
        self.aspects = np.ascontiguousarray(aspects, dtype=np.float32)
        self.profile = np.ascontiguousarray(profile, dtype=np.float32)
        self.k, self.lam, self.name = int(k), float(np.float32(lam)), name
        self.G = self.profile.shape[1]
        self.n, self.C = self.cand.shape
        assert self.aspects.shape[1] == self.G


# --------------------------------------------------------------------------- the spec
def clamp(aspects):
    """c = min(max(x, 0), 1), NaN counts as 0 (fp32 in, fp32 out: exact)."""
    a = np.asarray(aspects, dtype=np.float32)
    return np.clip(np.where(np.isnan(a), np.float32(0), a), 0, 1).astype(np.float32)


def live_and_rows(case):
    """(live [n, C], c fp32 [n, C, G]: the clamped rows, 0 where not live, err):
    ids < 0 are empty slots; ids >= n_items are counted in err."""
    cand = case.cand.astype(np.int64)
    ni = len(case.aspects)
    live = (cand >= 0) & (cand < ni)
    c = clamp(case.aspects)[np.where(live, cand, 0)]
    c[~live] = 0
    return live, c, int((cand >= ni).sum())


def scores_f64(case):
    """-inf and NaN count as -FLT_MAX."""
    s = np.where(np.isnan(case.sc), -np.inf, case.sc).astype(np.float64)
    return np.maximum(s, -FLT_MAX)


def values_f64(case, live, c, m):
    """value_i = lam s_i + (1 - lam) sum_a m_a c_{i,a} [n, C] in float64, -inf where not live."""
    div = np.einsum("ncg,ng->nc", c.astype(np.float64), m)
    return np.where(live, case.lam * scores_f64(case) + (1.0 - case.lam) * div, -np.inf)


def coverage_f64(p, c_list):
    """sum_a p_a (1 - prod_j (1 - c_{j,a})) [n] of lists with rows c_list [n, k, G]."""
    return (p * (1.0 - np.prod(1.0 - c_list.astype(np.float64), axis=1))).sum(axis=1)


def _tree_sum(x):
    """Sum of 64 fp32 columns in the pairwise order of the kernel's DPP wave sum."""
    while x.shape[1] > 1:
        x = (x[:, 0::2] + x[:, 1::2]).astype(np.float32)
    return x


def profile_f32(profile):
    """p as the kernel forms it (common.h, profile_entry): fp32 [n, G]."""
    f = np.float32
    w = np.zeros((len(profile), 64), dtype=f)
    G = profile.shape[1]
    w[:, :G] = np.maximum(np.where(np.isnan(profile), f(0), profile), f(0))
    total = _tree_sum(w)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(total > 0, (w / total).astype(f), f(0))
    return p[:, :G].astype(f)


class F32State:
    """The kernel's arithmetic in float32, operation by operation (xquad.hip):
    div_i = sum_a p_a c_{i,a} summed once from 0 in aspect order; value_i =
    (lam s_i) + (mu div_i), mu = 1 - lam; after a pick, for each aspect a in
    order: delta = m_a c_{pick,a}, m_a -= delta, cov += delta, div_i -= delta
    c_{i,a} (an aspect with c_{pick,a} = 0 has delta = 0, which changes nothing,
    so the kernel's skip needs no restating)."""

    def __init__(self, case, live, c):
        f = np.float32
        self.case, self.live, self.c = case, live, c
        self.m = profile_f32(case.profile)
        self.div = np.zeros((case.n, case.C), dtype=f)
        for a in range(case.G):
            self.div = (self.div + (self.m[:, a, None] * c[:, :, a]).astype(f)).astype(f)
        s = np.maximum(np.where(np.isnan(case.sc), -np.inf, case.sc).astype(f), -np.finfo(f).max)
        self.ls = (f(case.lam) * s).astype(f)
        self.mu = f(1) - f(case.lam)
        self.cov = np.zeros(case.n, dtype=f)

    def values(self, live):
        v = (self.ls + (self.mu * self.div).astype(np.float32)).astype(np.float32)
        return np.where(live, v, -np.inf).astype(np.float32)

    def pick(self, go, j):
        """Rows ``go`` pick position j."""
        f = np.float32
        rows = np.arange(self.case.n)
        cp = np.where(go[:, None], self.c[rows, j], f(0))
        for a in np.flatnonzero((cp != 0).any(axis=0)):
            delta = (self.m[:, a] * cp[:, a]).astype(f)
            self.m[:, a] = (self.m[:, a] - delta).astype(f)
            self.cov = (self.cov + delta).astype(f)
            self.div = (self.div - (delta[:, None] * self.c[:, :, a]).astype(f)).astype(f)


def greedy(case, f32=False):
    """The spec for every user of ``case``: (positions [n, k] (-1 once no live
    candidate is left), cov [n, k] float64, worst |value32 - value64| over the
    live candidates of every step, worst |cov32 - cov64| over every step).
    Float64 picks; with ``f32`` the float32 restatement picks instead."""
    live, c, _ = live_and_rows(case)
    p = normalise(case.profile)
    m = p.copy()
    st = F32State(case, live, c)
    rows = np.arange(case.n)
    pos = np.full((case.n, case.k), -1, dtype=np.int64)
    cov = np.zeros((case.n, case.k))
    worst_v = worst_c = 0.0
    for t in range(case.k):
        v64 = values_f64(case, live, c, m)
        v32 = st.values(live)
        if live.any():
            worst_v = max(worst_v, float(np.abs(v32[live].astype(np.float64) - v64[live]).max()))
        go = live.any(axis=1)
        j = np.argmax(v32 if f32 else v64, axis=1)  # the first maximum: the lowest position
        pos[go, t] = j[go]
        live[rows[go], j[go]] = False
        m = np.where(go[:, None], m * (1.0 - c[rows, j].astype(np.float64)), m)
        st.pick(go, j)
        cov[:, t] = (p - m).sum(axis=1)
        worst_c = max(worst_c, float(np.abs(st.cov.astype(np.float64) - cov[:, t]).max()))
    return pos, cov, worst_v, worst_c


@functools.lru_cache(maxsize=None)
def reference(builder, *args):
    """(case, float64 positions, float64 cov) of ``builder(*args)``, computed once."""
    case = builder(*args)
    return (case,) + greedy(case)[:2]


def items_at(case, pos):
    """Item ids [n, k] of positions (-1 stays -1)."""
    return np.where(pos >= 0, np.take_along_axis(case.cand, np.maximum(pos, 0), axis=1), -1)


def stable_topk(case):
    """The stable order by score of the live candidates: ids [n, k], -1 past the live ones."""
    live, _, _ = live_and_rows(case)
    s = np.where(live, scores_f64(case), -np.inf)
    order = np.argsort(-s, axis=1, kind="stable")[:, :case.k]
    ids = np.take_along_axis(case.cand, order, axis=1)
    return np.where(np.take_along_axis(live, order, axis=1), ids, -1)


def replay(picks, out_cov, case, tol_v=TOL_V, tol_cov=TOL_COV):
    """Float64 replay that follows the kernel's own picks (item ids [n, k]) and
    out_cov [n, k], every step of every list; returns the number of bad steps.
    A pick must be a live candidate (of the live positions that hold the id,
    the one of highest value, lowest first) whose float64 value is within
    2 tol_v of the step's maximum over the live candidates, and the lowest live
    position with its score bits and a bit-equal clamped aspect row. out_cov
    must be within tol_cov of the float64 coverage of the list after the step.
    A -1 is right exactly when no live candidate is left, and repeats the
    coverage of the list as it stands."""
    picks, out_cov = np.asarray(picks), np.asarray(out_cov, dtype=np.float64)
    live, c, _ = live_and_rows(case)
    p = normalise(case.profile)
    m = p.copy()
    rows = np.arange(case.n)
    bits = case.sc.view(np.uint32)
    cbits = c.view(np.uint32)
    bad = 0
    for t in range(picks.shape[1]):
        it = picks[:, t].astype(np.int64)
        val = values_f64(case, live, c, m)
        match = live & (case.cand == it[:, None])
        j = np.argmax(np.where(match, val, -np.inf), axis=1)
        found = match.any(axis=1) & (it >= 0)
        ended = it < 0
        wrong = np.where(ended, live.any(axis=1), ~found)
        near = val[rows, j] >= val.max(axis=1) - 2 * tol_v
        same = live & (bits == bits[rows, j][:, None])
        same &= (cbits == cbits[rows, j][:, None, :]).all(axis=2)
        lowest = np.argmax(same, axis=1) == j
        wrong |= found & ~(near & lowest)
        live[rows[found], j[found]] = False
        m = np.where(found[:, None], m * (1.0 - c[rows, j].astype(np.float64)), m)
        wrong |= ~(np.abs(out_cov[:, t] - (p - m).sum(axis=1)) <= tol_cov)
        bad += int(wrong.sum())
    return bad


# --------------------------------------------------------------------------- inputs
def multi_hot(rng, ni, G, fractional=False):
    """fp32 [ni, G]: one to three aspects per item (fewer where the draws
    repeat), binary, or drawn in (0, 1) with ``fractional``."""
    A = np.zeros((ni, G), dtype=np.float32)
    count = rng.integers(1, 4, ni)
    for r in range(3):
        col = rng.integers(0, G, ni)
        use = np.flatnonzero(r < count)
        val = 0.05 + 0.9 * rng.random(len(use)) if fractional else 1.0
        A[use, col[use]] = val
    return A


def _lists(rng, ni, n, C):
    return np.stack([rng.choice(ni, C, replace=False) for _ in range(n)]).astype(np.int32)


def _sorted_scores(rng, n, C):
    return -np.sort(-rng.random((n, C)), axis=1).astype(np.float32)


def history_profile(rng, aspects, n, length=100):
    """fp32 [n, G]: aspect shares of ``length`` random items per user, as dr_aspect_profile gives."""
    c = clamp(aspects)
    hist = np.stack([c[rng.choice(len(c), min(length, len(c)), replace=False)].sum(axis=0)
                     for _ in range(n)]).astype(np.float32)
    total = hist.sum(axis=1, keepdims=True)
    return np.where(total > 0, hist / np.where(total > 0, total, 1), 0).astype(np.float32)


def basic_input(lam=0.5):
    """n = 12, C = 1000 -> 100, G = 19, 20000 items, sorted scores, binary multi-hot aspects."""
    rng = np.random.default_rng(201)
    A = multi_hot(rng, 20000, 19)
    return Case(_lists(rng, 20000, 12, 1000), _sorted_scores(rng, 12, 1000), A,
                history_profile(rng, A, 12), 100, lam, f"basic lam = {lam:.1f}")


BASIC_LAMS = (1.0, 0.5, 0.0)
# (C, k_out, G): one candidate; a partial wave with k_out = C; one lane past a
# wave with a lane per aspect; one candidate past the workgroup; the two shapes
# exactly at the cell limit; three aspects at the flagship C. Every second
# shape draws fractional coverages.
SHAPES = [(1, 1, 1), (63, 63, 2), (65, 10, 64), (257, 40, 19), (1024, 128, 32), (512, 100, 64),
          (1000, 100, 3)]


def shape_input(C, k, G, n=6, ni=5000):
    rng = np.random.default_rng(1000 * C + G)
    A = multi_hot(rng, ni, G, fractional=SHAPES.index((C, k, G)) % 2 == 1)
    return Case(_lists(rng, ni, n, C), _sorted_scores(rng, n, C), A, history_profile(rng, A, n),
                k, 0.5, f"shape {(C, k, G)}")


def tie_input():
    """C = 300 -> 60, scores small integers, G = 4, every item one of six
    aspect rows, p = (1/4, 1/4, 3/8, 1/8): aspects 0 and 1 weigh the same, so
    equal scores tie exactly across bit-different rows too."""
    rng = np.random.default_rng(231)
    kinds = np.float32([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 1, 0],
                        [0, 1, 1, 0]])
    A = kinds[rng.integers(0, len(kinds), 3000)]
    sc = rng.integers(0, 3, (6, 300)).astype(np.float32)
    return Case(_lists(rng, 3000, 6, 300), sc, A, np.tile(np.float32([2, 2, 3, 1]), (6, 1)), 60,
                0.5, "ties")


def profile_input():
    """C = 200 -> 40, G = 5; one candidate list and one score row for all seven
    users, who differ in the profile row alone: 0 zero, 1 one-hot, 2 a zero on
    the commonest aspect, 3 unnormalised, 4 = row 3 x 8, 5 = row 3 with a NaN
    and a negative weight where it holds 0, 6 = row 3 / 16."""
    rng = np.random.default_rng(241)
    A = np.zeros((4000, 5), dtype=np.float32)
    A[np.arange(4000), rng.choice(5, 4000, p=[0.15, 0.15, 0.4, 0.15, 0.15])] = 1
    extra = rng.random(4000) < 0.4
    A[extra, rng.integers(0, 5, 4000)[extra]] = 1
    cand = np.tile(_lists(rng, 4000, 1, 200), (7, 1))
    sc = np.tile(rng.standard_normal((1, 200)).astype(np.float32), (7, 1))
    base = np.float32([5, 0, 3, 7, 0])
    prof = np.stack([np.zeros(5, np.float32), np.float32([0, 0, 0, 4, 0]),
                     np.float32([1, 2, 0, 3, 2]), base, base * 8,
                     np.float32([5, np.nan, 3, 7, -2]), base / np.float32(16)])
    return Case(cand, sc, A, prof, 40, 0.5, "profiles")


def aspect_value_input(clamped=False):
    """C = 150 -> 30, G = 6: a matrix with entries -0.5, 1.5, NaN, +inf and
    all-zero rows among fractional ones; with ``clamped`` its clamped copy."""
    rng = np.random.default_rng(251)
    A = multi_hot(rng, 2000, 6, fractional=True)
    A[rng.random(2000) < 0.1] = 0
    for val in (-0.5, 1.5, np.nan, np.inf):
        A[rng.integers(0, 2000, 300), rng.integers(0, 6, 300)] = val
    profile = history_profile(rng, A, 6)
    return Case(_lists(rng, 2000, 6, 150), rng.standard_normal((6, 150)).astype(np.float32),
                clamp(A) if clamped else A, profile, 30, 0.5, "aspect values")


INVALID_ERR = 4 + 2  # invalid_input: users 2 and 5


def invalid_input():
    """C = 120 -> 30, G = 6, 2000 items. User 0: clean. User 1: 20 empty slots.
    User 2: 4 ids past the table. User 3: a NaN and a -inf score.
    User 4: 100 empty slots, so 20 live candidates for 30 picks. User 5: 2 ids
    past the table and nothing else live."""
    rng = np.random.default_rng(261)
    A = multi_hot(rng, 2000, 6)
    cand = _lists(rng, 2000, 6, 120)
    sc = rng.standard_normal((6, 120)).astype(np.float32)
    cand[1, rng.choice(120, 20, replace=False)] = -1
    cand[2, rng.choice(120, 4, replace=False)] = [2000, 2001, 2**31 - 1, 5000]
    sc[3, [5, 17]] = [np.nan, -np.inf]
    cand[4, rng.choice(120, 100, replace=False)] = -1
    cand[5, :] = -1
    cand[5, [7, 99]] = [2000, 123456]
    return Case(cand, sc, A, history_profile(rng, A, 6), 30, 0.5, "invalid")


def many_users_input():
    """n = 3000, C = 64 -> 8, G = 7: many users per workgroup of a capped grid."""
    rng = np.random.default_rng(271)
    A = multi_hot(rng, 3000, 7)
    cand = rng.integers(0, 3000, (3000, 64)).astype(np.int32)  # ids may repeat in a list
    cand[rng.random((3000, 64)) < 0.05] = -1
    return Case(cand, rng.standard_normal((3000, 64)).astype(np.float32), A,
                history_profile(rng, A, 3000, 30), 8, 0.5, "many users")


# --------------------------------------------------------------------------- door fixture
DOOR_USERS, DOOR_ITEMS, DOOR_D, DOOR_G = 300, 1682, 32, 19
DOOR_K, DOOR_CANDIDATES, DOOR_LAM = 20, 200, 0.5
DOOR_NAMES = [f"genre_{a}" for a in range(DOOR_G)]


@functools.lru_cache(maxsize=None)
def door_fixture():
    """(user table, item table fp32; frozen [m, 2] int64 unique (user, item)
    pairs, 30 draws per user, each user's history skewed to three of the 19
    aspects; aspects fp32 [items, 19], one to three per item)."""
    rng = np.random.default_rng(281)
    U = (rng.standard_normal((DOOR_USERS, DOOR_D)) / 8).astype(np.float32)  # scores of sd 0.7
    E = rng.standard_normal((DOOR_ITEMS, DOOR_D)).astype(np.float32)
    A = multi_hot(rng, DOOR_ITEMS, DOOR_G)
    pairs = []
    for u in range(DOOR_USERS):
        w = np.where(A[:, rng.choice(DOOR_G, 3, replace=False)].any(axis=1), 8.0, 1.0)
        for i in rng.choice(DOOR_ITEMS, 30, replace=False, p=w / w.sum()):
            pairs.append((u, int(i)))
    return U, E, np.unique(np.array(pairs, dtype=np.int64), axis=0), A


@functools.lru_cache(maxsize=None)
def door_case():
    """The door fixture as a Case: the float64 scan's top candidates (scores
    rounded to fp32), profiles from the frozen pairs."""
    U, E, frozen, A = door_fixture()
    s = U.astype(np.float64) @ E.astype(np.float64).T
    s[frozen[:, 0], frozen[:, 1]] = -np.inf
    cand = np.argsort(-s, axis=1, kind="stable")[:, :DOOR_CANDIDATES].astype(np.int32)
    sc = np.take_along_axis(s, cand.astype(np.int64), axis=1).astype(np.float32)
    hist = np.zeros((DOOR_USERS, DOOR_G), dtype=np.float32)
    np.add.at(hist, frozen[:, 0], A[frozen[:, 1]])
    profile = hist / hist.sum(axis=1, keepdims=True)
    return Case(cand, sc, A, profile, DOOR_K, DOOR_LAM, "door")


@functools.lru_cache(maxsize=None)
def door_property():
    """(mean coverage of the plain top-k lists, mean coverage of the float64
    greedy's lists at DOOR_LAM) on the door fixture: the property the GPU door
    test asserts, with its margin shown on the CPU."""
    case = door_case()
    _, c, _ = live_and_rows(case)
    p = normalise(case.profile)
    pos = greedy(case)[0]
    rows = np.arange(case.n)[:, None]
    return (float(coverage_f64(p, c[:, :DOOR_K]).mean()),
            float(coverage_f64(p, c[rows, pos]).mean()))


def all_inputs():
    """Every input of tests/test_xquad_gpu.py's re-rank tests."""
    cases = [basic_input(lam) for lam in BASIC_LAMS]
    cases += [shape_input(*s) for s in SHAPES]
    return cases + [tie_input(), profile_input(), aspect_value_input(), invalid_input(),
                    many_users_input(), door_case()]


@functools.lru_cache(maxsize=None)
def measure_tol(verbose=False):
    """(worst |value32 - value64| over every live candidate and step, worst
    |cov32 - cov64| over every step) of the float32 restatement on the GPU
    tests' inputs, on the float64 picks."""
    worst_v = worst_c = 0.0
    for case in all_inputs():
        _, _, wv, wc = greedy(case)
        if verbose:
            print(f"    {case.name:28s}  {wv:.2e}   {wc:.2e}")
        worst_v, worst_c = max(worst_v, wv), max(worst_c, wc)
    return worst_v, worst_c


if __name__ == "__main__":
    print("    input                         value      coverage")
    print("worst over all inputs: value %.2e, coverage %.2e" % measure_tol(verbose=True))
    print("door fixture: mean coverage top-k %.4f, xquad %.4f" % door_property())
