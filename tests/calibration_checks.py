"""CPU side of the calibrated re-rank tests (dr_calibrated_rerank,
dr_label_profile, dr_calibration_kl; include/divrec_hip.h): the spec as a
float64 greedy, a float64 replay that judges a kernel's picks step by step, a
float32 restatement of the kernel's arithmetic that measures fp32 against
float64, and the seeded inputs of tests/test_calibration_gpu.py. No GPU, no
torch. Every function works on all users of an input at once.

TOL_V bounds |value_fp32 - value_float64| of a candidate's value
lam * s - (1 - lam) * KL. It is 10 x the worst difference the float32
restatement (``values_f32``: the kernel's formula, base sum plus the two-term
correction per category, numpy's summation order and log) shows over every live
candidate at every step of every input of tests/test_calibration_gpu.py,
replayed on the float64 greedy's picks by ``measure_tol_v`` (python
tests/calibration_checks.py): 8.62e-7 (the basic input at lam = 0, where the
value is the KL alone; 7.5e-8 to 6.6e-7 on the others). The factor 10 covers
the kernel's own summation order and logf. The replay allows a pick 2 x TOL_V
below the step's float64 maximum (the pick's and the best candidate's fp32
values are each off by up to TOL_V) and out_kl TOL_V around the float64 KL.
"""
import functools

import numpy as np

ALPHA = float(np.float32(0.01))  # DR_CALIB_ALPHA, the fp32 constant's value
MAX_LABELS = 64                  # DR_CALIB_MAX_LABELS
TOL_V = 8.62e-6                  # 10 x 8.62e-7 (measure_tol_v, CPU)


class Case:
    """One input of dr_calibrated_rerank: cand int32 [n, C], sc fp32 [n, C],
    labels int [n_items], profile fp32 [n, G], k picks at trade-off lam."""

    def __init__(self, cand, sc, labels, profile, k, lam, name=""):
        self.cand = np.ascontiguousarray(cand, dtype=np.int32)
        self.sc = np.ascontiguousarray(sc, dtype=np.float32)
        self.labels = np.ascontiguousarray(labels)
        self.profile = np.ascontiguousarray(profile, dtype=np.float32)
        self.k, self.lam, self.name = int(k), float(np.float32(lam)), name
        self.G = self.profile.shape[1]
        self.n, self.C = self.cand.shape


# --------------------------------------------------------------------------- the spec
def normalise(w, dtype=np.float64):
    """p = max(w, 0) / sum max(w, 0) per row (NaN counts as 0; a zero row stays zero)."""
    w = np.asarray(w, dtype=dtype)
    w = np.maximum(np.where(np.isnan(w), 0, w), 0).astype(dtype)
    s = w.sum(axis=1, keepdims=True, dtype=dtype)
    return np.where(s > 0, w / np.where(s > 0, s, 1), 0).astype(dtype)


def live_and_labels(case):
    """(live [n, C], label [n, C] (0 where not live), err): ids < 0 are empty
    slots; ids >= n_items and labels outside [0, G) are counted in err."""
    cand = case.cand.astype(np.int64)
    inside = (cand >= 0) & (cand < len(case.labels))
    lab = np.asarray(case.labels, dtype=np.int64)[np.where(inside, cand, 0)]
    live = inside & (lab >= 0) & (lab < case.G)
    err = int((cand >= len(case.labels)).sum() + (inside & ~live).sum())
    return live, np.where(live, lab, 0), err


def _terms(p, share):
    """p log(p / q~) with q~ = (1 - alpha) share + alpha p, 0 where p = 0 (float64)."""
    q = (1.0 - ALPHA) * share + ALPHA * p
    ok = p > 0
    return np.where(ok, p * np.log(np.where(ok, p, 1.0) / np.where(ok, q, 1.0)), 0.0)


def kl_list(p, cnt):
    """KL(p || q~) [n] of lists with label counts cnt [n, G] (q = 0 for an empty list)."""
    total = cnt.sum(axis=1, keepdims=True)
    return _terms(p, cnt / np.maximum(total, 1)).sum(axis=1)


def kl_per_label(p, cnt):
    """KL_c [n, G]: KL(p || q~) of each list with one more item of label c."""
    t1 = cnt.sum(axis=1, keepdims=True) + 1
    a, b = _terms(p, cnt / t1), _terms(p, (cnt + 1) / t1)
    return a.sum(axis=1, keepdims=True) - a + b


def values_f64(case, live, lab, p, cnt):
    """value_i = lam s_i - (1 - lam) KL_{l(i)} [n, C] in float64, -inf where not live."""
    kl = np.take_along_axis(kl_per_label(p, cnt), lab, axis=1)
    s = np.maximum(np.where(np.isnan(case.sc), -np.inf, case.sc).astype(np.float64),
                   -float(np.finfo(np.float32).max))
    return np.where(live, case.lam * s - (1.0 - case.lam) * kl, -np.inf)


def values_f32(case, live, lab, p32, logp32, cnt):
    """The kernel's arithmetic in float32 (calibration.hip): per category
    a = p (log p - log q~(n)), b = p (log p - log q~(n + 1)) with the shares
    n / (t + 1) formed as n * (1 / (t + 1)) and q~ as one fma, KL_c = (sum a -
    a_c) + b_c, value = (lam s) + (-(mu KL_c)), mu = 1 - lam."""
    f = np.float32
    inv = (f(1) / (cnt.sum(axis=1, keepdims=True) + 1).astype(f)).astype(f)
    alpha, one_m = f(ALPHA), f(1) - f(ALPHA)

    def term(n):
        share = (n.astype(f) * inv).astype(f)
        q = (one_m.astype(np.float64) * share + (alpha * p32).astype(f)).astype(f)  # fmaf
        ok = p32 > 0
        return np.where(ok, p32 * (logp32 - np.log(np.where(ok, q, f(1)))), f(0)).astype(f)

    a, b = term(cnt), term(cnt + 1)
    klc = ((a.sum(axis=1, keepdims=True, dtype=f) - a) + b).astype(f)
    mu = f(1) - f(case.lam)
    gain = np.take_along_axis((-(mu * klc)).astype(f), lab, axis=1)
    s = np.maximum(np.where(np.isnan(case.sc), -np.inf, case.sc).astype(f), -np.finfo(f).max)
    return np.where(live, (f(case.lam) * s).astype(f) + gain, -np.inf).astype(f)


def _profile_f32(case):
    p32 = normalise(case.profile, np.float32)
    return p32, np.log(np.where(p32 > 0, p32, np.float32(1))).astype(np.float32)


def greedy(case, f32=False):
    """The spec for every user of ``case``: (positions [n, k] (-1 once no live
    candidate is left), kl [n, k], worst |value32 - value64| over the live
    candidates of every step). Float64 picks; with ``f32`` the float32
    restatement picks instead."""
    live, lab, _ = live_and_labels(case)
    p = normalise(case.profile)
    p32, logp32 = _profile_f32(case)
    cnt = np.zeros((case.n, case.G))
    rows = np.arange(case.n)
    pos = np.full((case.n, case.k), -1, dtype=np.int64)
    kl = np.zeros((case.n, case.k))
    kl_cur = kl_list(p, cnt)
    worst = 0.0
    for t in range(case.k):
        v64 = values_f64(case, live, lab, p, cnt)
        v32 = values_f32(case, live, lab, p32, logp32, cnt)
        if live.any():
            worst = max(worst, float(np.abs(v32[live].astype(np.float64) - v64[live]).max()))
        go = live.any(axis=1)
        j = np.argmax(v32 if f32 else v64, axis=1)  # the first maximum: the lowest position
        pos[go, t] = j[go]
        live[rows[go], j[go]] = False
        cnt[rows[go], lab[rows[go], j[go]]] += 1
        kl_cur = np.where(go, kl_list(p, cnt), kl_cur)
        kl[:, t] = kl_cur
    return pos, kl, worst


@functools.lru_cache(maxsize=None)
def reference(builder, *args):
    """(case, float64 positions, float64 kl) of ``builder(*args)``, computed once."""
    case = builder(*args)
    return (case,) + greedy(case)[:2]


def items_at(case, pos):
    """Item ids [n, k] of positions (-1 stays -1)."""
    return np.where(pos >= 0, np.take_along_axis(case.cand, np.maximum(pos, 0), axis=1), -1)


def replay(picks, out_kl, case, tol_v=TOL_V):
    """Float64 replay that follows the kernel's own picks (item ids [n, k]) and
    out_kl [n, k], every step of every list; returns the number of bad steps.
    A pick must be a live candidate (of the live positions that hold the id,
    the one of highest value, lowest first) whose float64 value is within
    2 tol_v of the step's maximum over the live candidates, and the lowest live
    position with its score bits and label. out_kl must be within tol_v of the
    float64 KL of the list after the step. A -1 is right exactly when no live
    candidate is left, and repeats the KL of the list as it stands."""
    picks, out_kl = np.asarray(picks), np.asarray(out_kl, dtype=np.float64)
    live, lab, _ = live_and_labels(case)
    p = normalise(case.profile)
    cnt = np.zeros((case.n, case.G))
    rows = np.arange(case.n)
    bits = case.sc.view(np.uint32)
    bad = 0
    for t in range(picks.shape[1]):
        it = picks[:, t].astype(np.int64)
        val = values_f64(case, live, lab, p, cnt)
        match = live & (case.cand == it[:, None])
        j = np.argmax(np.where(match, val, -np.inf), axis=1)
        found = match.any(axis=1) & (it >= 0)
        ended = it < 0
        wrong = np.where(ended, live.any(axis=1), ~found)
        near = val[rows, j] >= val.max(axis=1) - 2 * tol_v
        same = live & (bits == bits[rows, j][:, None]) & (lab == lab[rows, j][:, None])
        lowest = np.argmax(same, axis=1) == j
        wrong |= found & ~(near & lowest)
        live[rows[found], j[found]] = False
        cnt[rows[found], lab[rows[found], j[found]]] += 1
        wrong |= ~(np.abs(out_kl[:, t] - kl_list(p, cnt)) <= tol_v)
        bad += int(wrong.sum())
    return bad


# --------------------------------------------------------------------------- inputs
def _lists(rng, ni, n, C):
    return np.stack([rng.choice(ni, C, replace=False) for _ in range(n)]).astype(np.int32)


def _sorted_scores(rng, n, C):
    return -np.sort(-rng.random((n, C)), axis=1).astype(np.float32)


def history_profile(rng, labels, G, n, length=100):
    """fp32 [n, G]: label shares of ``length`` random items per user, as dr_label_profile gives."""
    hist = np.stack([np.bincount(labels[rng.choice(len(labels), length, replace=False)],
                                 minlength=G) for _ in range(n)])
    return (hist.astype(np.float32) / np.float32(length)).astype(np.float32)


def basic_input(lam=0.5):
    """n = 12, C = 1000 -> 100, G = 19, 20000 items, config-5 shaped sorted scores."""
    rng = np.random.default_rng(101)
    labels = rng.integers(0, 19, 20000).astype(np.int32)
    return Case(_lists(rng, 20000, 12, 1000), _sorted_scores(rng, 12, 1000), labels,
                history_profile(rng, labels, 19, 12), 100, lam, "basic")


BASIC_LAMS = (1.0, 0.5, 0.0)
# (C, k_out, G): one candidate; a partial last lane group with k_out = C; one
# lane past a group with a full wave of categories; the maximum C; config 5
SHAPES = [(1, 1, 1), (63, 63, 2), (65, 10, 64), (1024, 128, 64), (1000, 100, 3)]


def shape_input(C, k, G, n=6, ni=5000):
    rng = np.random.default_rng(1000 * C + G)
    labels = rng.integers(0, G, ni).astype(np.int32)
    return Case(_lists(rng, ni, n, C), _sorted_scores(rng, n, C), labels,
                history_profile(rng, labels, G, n), k, 0.5, f"shape {(C, k, G)}")


def tie_input():
    """C = 300 -> 60, scores small integers, G = 4 with p = (1/4, 1/4, 3/8, 1/8):
    categories 0 and 1 are bit-equal, so equal scores tie exactly across them."""
    rng = np.random.default_rng(131)
    labels = rng.integers(0, 4, 3000).astype(np.int32)
    sc = rng.integers(0, 3, (6, 300)).astype(np.float32)
    return Case(_lists(rng, 3000, 6, 300), sc, labels, np.tile(np.float32([2, 2, 3, 1]), (6, 1)),
                60, 0.5, "ties")


def profile_input():
    """C = 200 -> 40, G = 5; one candidate list and one score row for all seven
    users, who differ in the profile row alone: 0 zero, 1 p_2 = 0 for the most
    frequent label, 2 one-hot, 3 unnormalised, 4 = row 3 x 8, 5 = row 3 with a
    NaN and a negative weight where it holds 0, 6 = row 3 / 16."""
    rng = np.random.default_rng(141)
    labels = rng.choice(5, 4000, p=[0.15, 0.15, 0.4, 0.15, 0.15]).astype(np.int32)
    cand = np.tile(_lists(rng, 4000, 1, 200), (7, 1))
    sc = np.tile(rng.standard_normal((1, 200)).astype(np.float32), (7, 1))
    base = np.float32([5, 0, 3, 7, 0])
    prof = np.stack([np.zeros(5, np.float32), np.float32([1, 2, 0, 3, 2]),
                     np.float32([0, 0, 0, 4, 0]), base, base * 8,
                     np.float32([5, np.nan, 3, 7, -2]), base / np.float32(16)])
    return Case(cand, sc, labels, prof, 40, 0.5, "profiles")


INVALID_ERR = 4 + 3 + 5 + 2  # invalid_input: users 2, 3 (labels -1, then G) and 5


def invalid_input():
    """C = 120 -> 30, G = 6, 2000 items of which ten carry label -1 and ten
    label G. User 0: clean. User 1: 20 empty slots. User 2: 4 ids past the
    table. User 3: 3 candidates of label -1 and 5 of label G. User 4: 100
    empty slots, so 20 live candidates for 30 picks. User 5: 2 ids past the
    table and nothing else live."""
    rng = np.random.default_rng(151)
    labels = rng.integers(0, 6, 2000).astype(np.int32)
    labels[:10], labels[10:20] = -1, 6
    cand = (20 + _lists(rng, 1980, 6, 120)).astype(np.int32)
    cand[1, rng.choice(120, 20, replace=False)] = -1
    cand[2, rng.choice(120, 4, replace=False)] = [2000, 2001, 2**31 - 1, 5000]
    cand[3, rng.choice(120, 8, replace=False)] = [0, 1, 2, 10, 11, 12, 13, 14]
    cand[4, rng.choice(120, 100, replace=False)] = -1
    cand[5, :] = -1
    cand[5, [7, 99]] = [2000, 123456]
    return Case(cand, rng.standard_normal((6, 120)).astype(np.float32), labels,
                history_profile(rng, np.clip(labels, 0, 5), 6, 6), 30, 0.5, "invalid")


def many_users_input():
    """n = 3000, C = 64 -> 8, G = 7: many users per wave of a capped grid."""
    rng = np.random.default_rng(161)
    labels = rng.integers(0, 7, 3000).astype(np.int32)
    cand = rng.integers(0, 3000, (3000, 64)).astype(np.int32)  # ids may repeat in a list
    cand[rng.random((3000, 64)) < 0.05] = -1
    return Case(cand, rng.standard_normal((3000, 64)).astype(np.float32), labels,
                history_profile(rng, labels, 7, 3000, 30), 8, 0.5, "many users")


def all_inputs():
    """Every input of tests/test_calibration_gpu.py's re-rank tests."""
    cases = [basic_input(lam) for lam in BASIC_LAMS]
    cases += [shape_input(*s) for s in SHAPES]
    return cases + [tie_input(), profile_input(), invalid_input(), many_users_input()]


def measure_tol_v(verbose=False):
    """Worst |value32 - value64| of the float32 restatement over every live
    candidate and step of the GPU tests' inputs, on the float64 picks."""
    worst_all = 0.0
    for case in all_inputs():
        worst = greedy(case)[2]
        if verbose:
            print(f"{case.name:24s} lam = {case.lam:.1f}  worst |v32 - v64| = {worst:.2e}")
        worst_all = max(worst_all, worst)
    return worst_all


# --------------------------------------------------------------------------- door fixture
DOOR_USERS, DOOR_ITEMS, DOOR_D, DOOR_G = 300, 1682, 32, 5
DOOR_K, DOOR_CANDIDATES, DOOR_LAM = 20, 200, 0.5


@functools.lru_cache(maxsize=None)
def door_fixture():
    """(user table, item table fp32; frozen [m, 2] int64 unique (user, item)
    pairs, 30 draws per user, each user's history from two of the five labels
    by preference; labels int64 [items])."""
    rng = np.random.default_rng(171)
    U = (rng.standard_normal((DOOR_USERS, DOOR_D)) / 8).astype(np.float32)  # scores of sd 0.7
    E = rng.standard_normal((DOOR_ITEMS, DOOR_D)).astype(np.float32)
    labels = rng.integers(0, DOOR_G, DOOR_ITEMS).astype(np.int64)
    pairs = []
    for u in range(DOOR_USERS):
        w = np.where(np.isin(labels, rng.choice(DOOR_G, 2, replace=False)), 8.0, 1.0)
        for i in rng.choice(DOOR_ITEMS, 30, replace=False, p=w / w.sum()):
            pairs.append((u, int(i)))
    return U, E, np.unique(np.array(pairs, dtype=np.int64), axis=0), labels


@functools.lru_cache(maxsize=None)
def door_property():
    """(mean KL of the plain top-k lists, mean KL of the float64 greedy's lists
    at DOOR_LAM) on the door fixture, scores in float64 rounded to fp32: the
    property the GPU door test asserts, with its margin shown on the CPU."""
    U, E, frozen, labels = door_fixture()
    s = U.astype(np.float64) @ E.astype(np.float64).T
    s[frozen[:, 0], frozen[:, 1]] = -np.inf
    cand = np.argsort(-s, axis=1, kind="stable")[:, :DOOR_CANDIDATES].astype(np.int32)
    sc = np.take_along_axis(s, cand.astype(np.int64), axis=1).astype(np.float32)
    hist = np.zeros((DOOR_USERS, DOOR_G))
    np.add.at(hist, (frozen[:, 0], labels[frozen[:, 1]]), 1)
    profile = (hist.astype(np.float32) / hist.sum(1, keepdims=True).astype(np.float32))
    case = Case(cand, sc, labels, profile, DOOR_K, DOOR_LAM, "door")
    p = normalise(case.profile)

    def mean_kl(pos):
        cnt = np.zeros((case.n, case.G))
        np.add.at(cnt, (np.repeat(np.arange(case.n), pos.shape[1]),
                        labels[items_at(case, pos)].ravel()), 1)
        return float(kl_list(p, cnt).mean())

    top = np.tile(np.arange(DOOR_K), (case.n, 1))
    return mean_kl(top), mean_kl(greedy(case)[0])


if __name__ == "__main__":
    print(f"worst over all inputs: {measure_tol_v(verbose=True):.2e}")
    print("door fixture: mean KL top-k %.4f, calibrated %.4f" % door_property())
