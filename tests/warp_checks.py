"""Helpers of the WARP tests: a numpy restatement of the counter-based draw
hash (csrc/common.h, draw_bits), the float64 restatement of dr_warp_fwd_bwd
(include/divrec_hip.h is the specification; the reference project has no
WARP, so the restatement is the pin), a float32 emulation of the kernel's
operation order (what a correct kernel may differ from float64 by, and, with
``bug=``, what a broken kernel would write), the shared inputs, and
``check_warp``, which tests/test_warp_gpu.py applies to the kernel's outputs
and tests/test_warp_host.py to the emulation and to its broken variants.

A violation test ``s_n > s_p - margin`` whose two sides are closer than the
fp32 error of the dot products may legitimately go either way: such a pair is
``undecided`` and everything after it in the pair's trial order depends on the
way it went. ``check_warp`` leaves those pairs out of the neg / trials
comparison (at most 1 % of the valid pairs) and compares the batch's loss and
gradients against a restatement that is told how the kernel decided them."""
import math

import numpy as np

from pairwise_checks import F, _fma32, csr

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
UNDECIDED_CAP = 0.01


# --------------------------------------------------------------------------- draws
def _u64(x):
    return np.asarray(x).astype(np.uint64)


def mix64(z):
    """splitmix64 finaliser on uint64 arrays (wrapping arithmetic)."""
    z = _u64(z)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_bits(seed, pos, draw, attempt):
    """csrc/common.h draw_bits on broadcastable integer arrays -> uint64."""
    with np.errstate(over="ignore"):
        seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
        one = np.uint64(1)
        z = mix64(seed + np.uint64(0x9E3779B97F4A7C15) * (_u64(pos) + one))
        z = mix64(z ^ (np.uint64(0xD1B54A32D192ED03) * (_u64(draw) + one)))
        return mix64(z + np.uint64(0x8CB92BA72F3D8DD7) * (_u64(attempt) + one))


def candidates(seed, pair_base, n_pairs, max_trials, n_items):
    """int64 [n_pairs, max_trials]: trial t of pair b draws
    draw_bits(seed, pair_base + b, 0, t) % n_items."""
    pos = np.arange(n_pairs, dtype=np.int64)[:, None] + int(pair_base)
    t = np.arange(max_trials, dtype=np.int64)[None, :]
    return (draw_bits(seed, pos, 0, t) % np.uint64(n_items)).astype(np.int64)


# --------------------------------------------------------------------------- shared pieces
def _member(csr_, nu, ni):
    """bool [nu, ni]: item in the user's CSR row (all False without a CSR)."""
    m = np.zeros((nu, ni), bool)
    if csr_ is not None:
        rowptr, items = csr_
        rows = np.repeat(np.arange(nu), np.diff(rowptr))
        m[rows, np.asarray(items, np.int64)] = True
    return m


def _skipped(case, cand, ok):
    """bool [B, T]: the draw is the positive itself, a listed positive or an
    excluded item (rows of invalid pairs: all True)."""
    nu, ni = case["U"].shape[0], case["I"].shape[0]
    uid, pid = np.asarray(case["uid"], np.int64), np.asarray(case["pid"], np.int64)
    skip = np.ones(cand.shape, bool)
    u = uid[ok][:, None]
    skip[ok] = ((cand[ok] == pid[ok][:, None]) | _member(case.get("pos"), nu, ni)[u, cand[ok]]
                | _member(case.get("excl"), nu, ni)[u, cand[ok]])
    return skip


def _valid(case):
    uid, pid = np.asarray(case["uid"], np.int64), np.asarray(case["pid"], np.int64)
    return (uid >= 0) & (uid < case["U"].shape[0]) & (pid >= 0) & (pid < case["I"].shape[0])


def _weight(ni, trials):
    """log(max(1, (n_items - 1) // trials)) in float64; trials >= 1."""
    return np.log(np.maximum(1, (ni - 1) // np.maximum(trials, 1)).astype(np.float64))


# --------------------------------------------------------------------------- float64 restatement
def warp_step_f64(case, forced=None):
    """The specification in float64. ``case``: U, I (fp32 tables), uid, pid,
    pos / excl (CSR pairs or None), max_trials, margin, seed, pair_base,
    grad_scale. Returns a dict: loss, neg, trials, gU, gI (float64 / int64),
    valid, undecided (per pair: some scored trial up to the stopping one has
    |s_p - margin - s_n| <= (d + 8) 2^-24 (sum|u p| + sum|u c| + |margin|)),
    and ``case`` itself. ``forced`` = (mask, neg, trials): the pairs of the
    mask take the given outcome instead of their own (check_warp feeds the
    kernel's outcome of the undecided pairs)."""
    U, I = np.asarray(case["U"], np.float64), np.asarray(case["I"], np.float64)
    uid, pid = np.asarray(case["uid"], np.int64), np.asarray(case["pid"], np.int64)
    T, margin = int(case["max_trials"]), float(case["margin"])
    B, (ni, d) = len(uid), I.shape
    ok = _valid(case)
    cand = candidates(case["seed"], case["pair_base"], B, T, max(ni, 1))
    skip = _skipped(case, cand, ok)
    S, A = U @ I.T, np.abs(U) @ np.abs(I).T  # every score, and every sum |u_k i_k|
    u, p = np.where(ok, uid, 0), np.where(ok, pid, 0)
    sp, ap = S[u, p], A[u, p]
    sn = S[u[:, None], cand]
    gap = sp[:, None] - margin - sn
    viol = ~skip & (gap < 0)
    has = viol.any(axis=1)
    first = np.where(has, viol.argmax(axis=1), T - 1)
    trials = np.where(has, first + 1, T)
    close = ~skip & (np.abs(gap) <= (d + 8) * 2.0 ** -24 * (ap[:, None] + A[u[:, None], cand]
                                                             + abs(margin)))
    undecided = ok & (close & (np.arange(T)[None, :] <= first[:, None])).any(axis=1)
    neg = np.where(has, cand[np.arange(B), first], -1)
    if forced is not None:
        mask, f_neg, f_trials = forced
        neg = np.where(mask, np.asarray(f_neg, np.int64), neg)
        trials = np.where(mask, np.asarray(f_trials, np.int64), trials)
        has = neg >= 0
    neg, trials, has = np.where(ok, neg, -1), np.where(ok, trials, 0), has & ok
    L = np.where(has, _weight(ni, trials), 0.0)
    s_neg = S[u, np.where(has, neg, 0)]
    loss = np.where(has, L * (margin - sp + s_neg), 0.0)
    loss[~ok] = np.nan
    g = (L * float(case["grad_scale"]))[has, None]
    gU, gI = np.zeros_like(U), np.zeros_like(I)
    np.add.at(gU, uid[has], g * (I[neg[has]] - I[pid[has]]))
    np.add.at(gI, pid[has], -g * U[uid[has]])
    np.add.at(gI, neg[has], g * U[uid[has]])
    return dict(loss=loss, neg=neg, trials=trials, gU=gU, gI=gI, valid=ok, undecided=undecided,
                case=case)


# --------------------------------------------------------------------------- fp32 emulation
def scores_f32(U, I):
    """fp32 [nu, ni]: every <U[u], I[i]> in the kernel's order (the dot of
    pairwise_checks.bpr_emulate_f32): lane l of 32 sums row elements l,
    l + 32, ... with fp32 FMAs, then a 5-step xor tree adds the lanes."""
    U, I = np.asarray(U, F), np.asarray(I, F)
    d = U.shape[1]
    E = -(-d // 32)
    pad = lambda t: np.pad(t, ((0, 0), (0, E * 32 - d))).reshape(len(t), E, 32)
    u, i = pad(U), pad(I)
    lanes = np.arange(32)
    s = np.zeros((len(U), len(I), 32), F)
    for e in range(E):
        s = _fma32(u[:, None, e], i[None, :, e], s)
    for m in (16, 8, 4, 2, 1):
        s = s + s[:, :, lanes ^ m]
    return s[:, :, 0]


BUGS = ("trials_off_by_one", "weight_from_n_items", "positive_accepted", "skip_not_counted",
        "no_negative_gradient", "gradient_without_violator")


def warp_emulate_f32(case, bug=None):
    """(loss fp32, neg int64, trials int32, gU fp32, gI fp32) in the kernel's
    operation order: fp32 scores and violation tests, the chosen triple's
    reported hinge in float64 (pure fp32 misses the loss bound near a hinge of
    0, by up to 2.4e-6 on these inputs: the weight, up to log 299, multiplies
    the dot products' error). ``bug`` (one of BUGS) plants one deliberate error."""
    assert bug is None or bug in BUGS
    U, I = np.asarray(case["U"], F), np.asarray(case["I"], F)
    uid, pid = np.asarray(case["uid"], np.int64), np.asarray(case["pid"], np.int64)
    T, margin = int(case["max_trials"]), F(case["margin"])
    B, ni = len(uid), I.shape[0]
    ok = _valid(case)
    cand = candidates(case["seed"], case["pair_base"], B, T, max(ni, 1))
    skip = _skipped(case, cand, ok)
    if bug == "positive_accepted":
        skip[ok] = False
    S = scores_f32(U, I)
    u, p = np.where(ok, uid, 0), np.where(ok, pid, 0)
    sp = S[u, p]
    sn = S[u[:, None], cand]
    viol = ~skip & (sn > (sp - margin)[:, None])
    has = viol.any(axis=1) & ok
    first = np.where(has, viol.argmax(axis=1), T - 1)
    trials = np.where(has, first + 1, T)
    if bug == "skip_not_counted":
        counted = np.cumsum(~skip, axis=1)[np.arange(B), first]
        trials = np.where(has, counted, T)
    if bug == "trials_off_by_one":
        trials = np.where(has, trials + 1, T)
    neg = np.where(has, cand[np.arange(B), first], -1)
    rank = ((ni if bug == "weight_from_n_items" else ni - 1) // np.maximum(trials, 1))
    L = np.where(has & (rank > 1), np.log(np.maximum(rank, 1).astype(F)), F(0)).astype(F)
    # the chosen triple's hinge margin + <u, c - p> in float64, as the kernel reports it
    U64, I64 = U.astype(np.float64), I.astype(np.float64)
    hinge = np.float64(margin) + np.sum(U64[u] * (I64[np.where(has, neg, 0)] - I64[p]), axis=1)
    loss = np.where(has, L.astype(np.float64) * hinge, 0.0).astype(F)
    loss[~ok] = np.nan
    upd = has.copy()
    c = neg.copy()
    if bug == "gradient_without_violator":  # the last scored draw updated as if it had violated
        last = np.where((~skip).any(axis=1), T - 1 - (~skip)[:, ::-1].argmax(axis=1), 0)
        extra = ok & ~has & (~skip).any(axis=1)
        c = np.where(extra, cand[np.arange(B), last], c)
        L = np.where(extra, F(math.log(max(1, (ni - 1) // T))), L).astype(F)
        upd = has | extra
    g = (L * F(case["grad_scale"])).astype(F)[upd, None]
    gU, gI = np.zeros_like(U), np.zeros_like(I)
    np.add.at(gU, uid[upd], g * I[c[upd]] - g * I[pid[upd]])
    np.add.at(gI, pid[upd], -g * U[uid[upd]])
    if bug != "no_negative_gradient":
        np.add.at(gI, c[upd], g * U[uid[upd]])
    return (loss, np.where(ok, neg, -1), np.where(ok, trials, 0).astype(np.int32), gU, gI)


# --------------------------------------------------------------------------- the assertions
def check_warp(got, ref, what=""):
    """The WARP assertions on a kernel's (loss, neg, trials, grad_user,
    grad_item) against ``ref = warp_step_f64(case)``; a gradient may be None
    (not asked for).
    * an invalid pair has loss NaN, neg -1, trials 0; no valid pair has NaN;
    * neg and trials equal the restatement's on every decided pair, and at
      most 1 % of the valid pairs are undecided;
    * an undecided pair's outcome is still one the draws allow: its neg is
      the candidate of trial ``trials``, a draw that is not skipped, or -1
      with every trial used up;
    * a pair without a violator has loss exactly 0 and trials = max_trials;
    * loss rtol 1e-5 / atol 1e-6 and gradients rtol 1e-4 / atol 1e-7 (the
      bounds of pairwise_checks.check_bpr) against the restatement, which on
      a batch with undecided pairs is told the kernel's outcome of those.
    Returns the undecided share."""
    loss, neg, trials, gU, gI = got
    case = ref["case"]
    ok, und = ref["valid"], ref["undecided"]
    T = int(case["max_trials"])
    neg, trials = np.asarray(neg, np.int64), np.asarray(trials, np.int64)
    share = int(und.sum()) / max(int(ok.sum()), 1)
    assert np.array_equal(np.isnan(loss), ~ok)
    assert (neg[~ok] == -1).all() and (trials[~ok] == 0).all()
    dec = ok & ~und
    assert np.array_equal(neg[dec], ref["neg"][dec]), "violators differ on decided pairs"
    assert np.array_equal(trials[dec], ref["trials"][dec]), "trial counts differ on decided pairs"
    assert und.sum() <= UNDECIDED_CAP * ok.sum()
    none = ok & (neg < 0)
    assert (loss[none] == 0).all() and (trials[none] == T).all()
    told = ref
    if und.any():
        cand = candidates(case["seed"], case["pair_base"], len(neg), T, case["I"].shape[0])
        skip = _skipped(case, cand, ok)
        w = und & (neg >= 0)
        assert ((trials[w] >= 1) & (trials[w] <= T)).all()
        at = np.clip(trials[w] - 1, 0, T - 1)
        assert np.array_equal(cand[w, at], neg[w]) and not skip[w, at].any()
        told = warp_step_f64(case, forced=(und, neg, trials))
    v = ok
    errs = [float(np.max(np.abs(loss[v] - told["loss"][v]), initial=0.0))]
    errs += [float(np.max(np.abs(g - r))) if g is not None else float("nan")
             for g, r in ((gU, told["gU"]), (gI, told["gI"]))]
    print(f"{what} B={len(neg)} d={case['U'].shape[1]}: max abs err loss {errs[0]:.3g} "
          f"gU {errs[1]:.3g} gI {errs[2]:.3g}; undecided {int(und.sum())} ({100 * share:.3f} %); "
          f"no violator {int(none.sum())}; mean trials {trials[ok].mean() if ok.any() else 0:.2f}")
    assert np.allclose(loss[v], told["loss"][v], rtol=1e-5, atol=1e-6), "loss"
    if gU is not None:
        assert np.allclose(gU, told["gU"], rtol=1e-4, atol=1e-7), "grad_user"
    if gI is not None:
        assert np.allclose(gI, told["gI"], rtol=1e-4, atol=1e-7), "grad_item"
    return share


# --------------------------------------------------------------------------- shared inputs
WARP_WIDTHS = [33, 64, 100, 128, 512]
NU, NI, N_POS, N_EXCL = 200, 300, 10, 20


def warp_case(d, regime="random", exclude=False, B=4096, max_trials=32, margin=1.0, seed=None):
    """bpr_case-style inputs (200 x 300 tables, standard_normal * 0.3 in fp32,
    rng seed d unless given), 10 positives per user, B pairs of a uniform user
    and one of its positives. ``regime`` "random": the positives are random
    items; "planted": each user's 10 top-scoring items, so pairs run through
    every trial count and a share of them finds no violator. ``exclude``: 20
    random excluded items per user."""
    rng = np.random.default_rng(d if seed is None else seed)
    U = (rng.standard_normal((NU, d)) * 0.3).astype(F)
    I = (rng.standard_normal((NI, d)) * 0.3).astype(F)
    if regime == "planted":
        S = U.astype(np.float64) @ I.astype(np.float64).T
        rows = [np.argsort(-S[u], kind="stable")[:N_POS] for u in range(NU)]
    else:
        rows = [rng.choice(NI, N_POS, replace=False) for _ in range(NU)]
    uid = rng.integers(0, NU, B)
    pid = np.array([rows[u][j] for u, j in zip(uid, rng.integers(0, N_POS, B))], np.int64)
    excl = csr([rng.choice(NI, N_EXCL, replace=False) for _ in range(NU)]) if exclude else None
    return dict(U=U, I=I, uid=uid, pid=pid, pos=csr(rows), excl=excl, max_trials=max_trials,
                margin=margin, seed=1000 + d, pair_base=0, grad_scale=1.0 / B)


_REFS = {}


def warp_ref(d, regime, exclude):
    """(case, warp_step_f64(case)) of warp_case(d, regime, exclude), computed
    once and shared; treat both as read-only."""
    key = (d, regime, exclude)
    if key not in _REFS:
        case = warp_case(d, regime, exclude)
        _REFS[key] = (case, warp_step_f64(case))
    return _REFS[key]
