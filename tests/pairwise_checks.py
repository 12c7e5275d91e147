"""Helpers of the pairwise-training and ranking-metric tests: float64 numpy
restatements of dr_bpr_fwd_bwd and dr_rank_metrics (include/divrec_hip.h),
pinned to the reference's fixtures by tests/test_pairwise_host.py; float32
emulations of the kernels' operation order (what a correct kernel may differ
from float64 by); and the assertion helpers that tests/test_pairwise_gpu.py
applies to the kernels' outputs. The host file feeds the same helpers
deliberately wrong outputs and the emulations, so each bound is shown on the
CPU to reject a broken kernel and to admit a correct one.

oracle.adam_step (float64) and oracle.sparse_adam_rows (fp32, bit-exact) stay
the Adam references."""
import math
import os

import numpy as np

import oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden")
F = np.float32
LOG2 = math.log(2.0)


def load(name):
    return np.load(os.path.join(GOLD, f"{name}.npz"), allow_pickle=False)


# --------------------------------------------------------------------------- BPR
def bpr_step_f64(U, I, uid, pid, nid, grad_scale):
    """(sp, sn, loss, grad_user, grad_item, margin) in float64: the scores
    u.p and u.n, the per-triple loss max(-x, 0) + log1p(exp(-|x|)) of
    x = sp - sn, and the gradients of sum(loss) * grad_scale. A triple with
    any id outside its table gets sp / sn / loss / margin NaN and adds nothing.
    margin[b] = (d + 8) 2^-24 (sum|u p| + sum|u n|) bounds the fp32 error of
    sp - sn for a d-term FMA dot product plus a 5-step tree: inside it a hit
    flag may legitimately differ from sp >= sn."""
    U, I = np.asarray(U, np.float64), np.asarray(I, np.float64)
    uid, pid, nid = (np.asarray(a, np.int64) for a in (uid, pid, nid))
    ok = ((uid >= 0) & (uid < U.shape[0]) & (pid >= 0) & (pid < I.shape[0])
          & (nid >= 0) & (nid < I.shape[0]))
    u, p, n = U[uid[ok]], I[pid[ok]], I[nid[ok]]
    sp, sn, loss, margin = (np.full(uid.shape, np.nan) for _ in range(4))
    sp[ok], sn[ok] = np.sum(u * p, axis=1), np.sum(u * n, axis=1)
    x = sp[ok] - sn[ok]
    loss[ok] = np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    margin[ok] = (U.shape[1] + 8) * 2.0 ** -24 * (np.abs(u * p).sum(1) + np.abs(u * n).sum(1))
    # d loss / dx = -sigmoid(-x), in the form that never overflows
    e = np.exp(-np.abs(x))
    g = (-np.where(x >= 0, e / (1.0 + e), 1.0 / (1.0 + e)) * grad_scale)[:, None]
    gU, gI = np.zeros_like(U), np.zeros_like(I)
    np.add.at(gU, uid[ok], g * (p - n))
    np.add.at(gI, pid[ok], g * u)
    np.add.at(gI, nid[ok], -g * u)
    return sp, sn, loss, gU, gI, margin


def bpr_case(d, B=4096, nu=200, ni=300, scale=0.3, seed=None):
    """The random inputs of the BPR tests (seed = d unless given): tables
    standard_normal * scale in fp32, then B uniform triples."""
    rng = np.random.default_rng(d if seed is None else seed)
    U = (rng.standard_normal((nu, d)) * scale).astype(F)
    I = (rng.standard_normal((ni, d)) * scale).astype(F)
    return U, I, rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)


def _fma32(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def bpr_emulate_f32(U, I, uid, pid, nid):
    """(loss fp32, hit) of valid triples in the kernel's own operation order:
    lane l of 32 sums row elements l, l + 32, ... with fp32 FMAs, a 5-step
    xor tree adds the lanes, then the loss in fp32."""
    U, I = np.asarray(U, F), np.asarray(I, F)
    d = U.shape[1]
    E = -(-d // 32)
    pad = lambda t: np.pad(t, ((0, 0), (0, E * 32 - d))).reshape(len(t), E, 32)
    u, p, n = pad(U[uid]), pad(I[pid]), pad(I[nid])
    lanes = np.arange(32)

    def dot(a, b):
        s = np.zeros((len(a), 32), F)
        for e in range(E):
            s = _fma32(a[:, e], b[:, e], s)
        for m in (16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ m]
        return s[:, 0]

    sp, sn = dot(u, p), dot(u, n)
    x = sp - sn
    loss = np.maximum(-x, F(0)) + np.log1p(np.exp(-np.abs(x)))
    return loss.astype(F), (sp >= sn).astype(np.int32)


def check_bpr(got, ref, pid, nid, cap=0.01, what=""):
    """The BPR assertions on a kernel's (loss, hit, grad_user, grad_item); a
    gradient may be None (not asked for). Per-triple loss rtol 1e-5 / atol
    1e-6, gradients rtol 1e-4 / atol 1e-7, hit == (sp >= sn) wherever
    |sp - sn| > margin with at most ``cap`` of the valid triples left out; a
    triple with pid == nid has loss log 2 and hit 1; an invalid triple has
    loss NaN and hit 0. Returns the share of triples the margin left out."""
    loss, hit, gU, gI = got
    sp, sn, rloss, rU, rI, margin = ref
    ok = ~np.isnan(rloss)
    decided = ok & (np.abs(sp - sn) > margin)
    left = int((ok & ~decided).sum())
    share = left / max(int(ok.sum()), 1)
    errs = [float(np.max(np.abs(loss[ok] - rloss[ok]), initial=0.0))]
    errs += [float(np.max(np.abs(g - r))) if g is not None else float("nan")
             for g, r in ((gU, rU), (gI, rI))]
    print(f"{what} B={len(rloss)} d={rU.shape[1]}: max abs err loss {errs[0]:.3g} gU {errs[1]:.3g} "
          f"gI {errs[2]:.3g}; inside the hit margin {left} ({100 * share:.3f} %)")
    assert np.array_equal(np.isnan(loss), ~ok)
    assert not hit[~ok].any()
    assert np.allclose(loss[ok], rloss[ok], rtol=1e-5, atol=1e-6)
    assert np.array_equal(hit[decided], (sp >= sn)[decided].astype(hit.dtype))
    assert left <= cap * ok.sum()
    same = ok & (np.asarray(pid) == np.asarray(nid))
    assert np.allclose(loss[same], LOG2, rtol=1e-5, atol=1e-6) and (hit[same] == 1).all()
    if gU is not None:
        assert np.allclose(gU, rU, rtol=1e-4, atol=1e-7)
    if gI is not None:
        assert np.allclose(gI, rI, rtol=1e-4, atol=1e-7)
    return share


# --------------------------------------------------------------------------- rank metrics
def rank_metrics_f64(recs, rowptr, items):
    """(precision, recall, AP, NDCG) per row of ``recs`` [n, k] in float64, by
    the formulas at the head of csrc/rank_metrics.hip: hits / k, hits / the
    raw count of positives (duplicates kept; NaN without positives),
    sum_p cumhits(p) / (p + 1) / k and sum_p rel(p) / log2(p + 2) over the
    same sum of all positions."""
    recs = np.asarray(recs, np.int64)
    n, k = recs.shape
    disc = 1.0 / np.log2(np.arange(2, k + 2))
    out = np.zeros((4, n))
    for u in range(n):
        pos = np.asarray(items[rowptr[u]:rowptr[u + 1]], np.int64)
        rel = np.isin(recs[u], pos).astype(np.float64)
        out[0, u] = rel.sum() / k
        out[1, u] = rel.sum() / len(pos) if len(pos) else np.nan
        out[2, u] = (np.cumsum(rel) / np.arange(1, k + 1)).sum() / k
        out[3, u] = (rel * disc).sum() / disc.sum()
    return tuple(out)


def rank_emulate_f32(recs, rowptr, items):
    """The kernel's fp32 operation order: lane l of 64 adds positions l,
    l + 64, ... in order, then a 6-step xor tree; integer hit counts."""
    recs = np.asarray(recs, np.int64)
    n, k = recs.shape
    nb = -(-k // 64)
    lanes = np.arange(64)
    p = np.arange(nb * 64)
    live = p < k
    disc = np.log2((p + 2).astype(F)).astype(F)
    out = np.zeros((4, n), F)

    def wave_sum(terms):  # [nb * 64] fp32 -> fp32
        s = np.zeros(64, F)
        for b in range(nb):
            s = s + terms[b * 64:(b + 1) * 64]
        for m in (32, 16, 8, 4, 2, 1):
            s = s + s[lanes ^ m]
        return s[0]

    for u in range(n):
        pos = np.asarray(items[rowptr[u]:rowptr[u + 1]], np.int64)
        rel = np.zeros(nb * 64, bool)
        rel[:k] = np.isin(recs[u], pos)
        cum = np.cumsum(rel)
        hits = int(cum[-1])
        z = F(0)
        ap = wave_sum(np.where(live, cum.astype(F) / (p + 1).astype(F), z))
        dcg = wave_sum(np.where(live, rel.astype(F) / disc, z))
        idcg = wave_sum(np.where(live, F(1) / disc, z))
        out[0, u] = F(hits) / F(k)
        out[1, u] = F(hits / len(pos)) if len(pos) else np.nan
        out[2, u] = ap / F(k)
        out[3, u] = dcg / idcg
    return tuple(out)


def check_rank(got, ref, what=""):
    """Precision and recall at rel 1e-6, AP and NDCG at rel 1e-5 / abs 1e-7
    (the larger of the two, as pytest.approx); recall NaN exactly where the
    restatement's is."""
    names = ("precision", "recall", "ap", "ndcg")
    worst = []
    for g, r in zip(got, ref):
        fin = ~np.isnan(r)
        worst.append(float(np.max(np.abs(np.asarray(g, np.float64)[fin] - r[fin]), initial=0.0)))
    print(f"{what}: max abs err " + " ".join(f"{n} {w:.3g}" for n, w in zip(names, worst)))
    for name, g, r, rel, ab in zip(names, got, ref, (1e-6, 1e-6, 1e-5, 1e-5),
                                   (1e-12, 1e-12, 1e-7, 1e-7)):
        g = np.asarray(g, np.float64)
        assert g.shape == r.shape, name
        assert np.array_equal(np.isnan(g), np.isnan(r)), name
        fin = ~np.isnan(r)
        assert np.all(np.abs(g[fin] - r[fin]) <= np.maximum(rel * np.abs(r[fin]), ab)), name


def csr(rows):
    """A list of per-user positives -> (rowptr int64, items int32 sorted per row)."""
    rowptr = np.zeros(len(rows) + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate([np.sort(np.asarray(r, np.int32)) for r in rows] +
                           [np.zeros(0, np.int32)])
    return rowptr, items.astype(np.int32)


# --------------------------------------------------------------------------- Adam
def adam_emulate_f32(p, g, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0):
    """adam_kernel's sequence of fp32 roundings (csrc/bpr.hip) in numpy:
    returns (param, exp_avg, exp_avg_sq) fp32."""
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    w1, b2, w2 = F(1.0 - beta1), F(beta2), F(1.0 - beta2)
    bc2_sqrt = F((1.0 - beta2 ** step) ** 0.5)
    neg_step = F(-(lr / (1.0 - beta1 ** step)))
    if wd != 0.0:
        g = g + F(wd) * p
    m = m + w1 * (g - m) if w1 < F(0.5) else g - (g - m) * (F(1) - w1)
    v = v * b2
    v = v + w2 * g * g
    denom = np.sqrt(v) / bc2_sqrt + F(eps)
    return p + neg_step * m / denom, m, v


def adam_ref(p, g, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0):
    """One float64 step (oracle.adam_step) from an fp32 state, with the bounds
    a correct fp32 kernel keeps: (param, exp_avg, exp_avg_sq, delta, tol_p,
    tol_m, tol_v); delta is the float64 update param_ref - param.

    With u = 2^-24 (one fp32 rounding, relative):
    * exp_avg_sq is a sum of non-negative terms: rtol 1e-6 (its three to four
      roundings are about 2e-7).
    * exp_avg = m + w (g - m) cancels when the two terms have opposite signs,
      so a purely relative bound does not hold for a correct kernel either
      (the fp32 emulation is off by up to 0.47 relative where the result is
      ~1e-7 of its terms). The roundings are: g - m, the fp32 weight, the
      product, and the final add or subtract; the first three are relative to
      c (|g| + |m|) at most, c = min(w, 1 - w) the factor of the branch the
      lerp takes, the last to the result: tol_m = u (|m_ref| + 4 c (|g| + |m|)).
    * weight decay makes g_eff = g + wd p from three more roundings, relative
      to |g| + |wd p|: that error reaches exp_avg times w and exp_avg_sq times
      2 (1 - beta2) |g_eff|.
    * param = p + delta: 1.5 u |p_ref| for the final add, 1e-5 |delta_ref| for
      the roundings of the quotient (about six operations, 4e-7), and what
      tol_m and the weight-decay part of tol_v let through:
      (lr / bc1) tol_m / denom and |delta| tol_v_wd / (2 exp_avg_sq).
    Measured on the fp32 emulation over test_pairwise_host.py's cases (up to
    1 049 089 elements): without the cancellation terms it misses plain
    relative bounds by far (exp_avg 0.47; exp_avg_sq 1.3e-3 with weight
    decay, 2.2e-7 without; param 1.1e-4 of the step past one rounding), and
    it uses at most 0.75 of tol_m, 0.23 of tol_v and 0.67 of tol_p."""
    u = 2.0 ** -24
    p64, g64, m64, v64 = (np.asarray(a, np.float64) for a in (p, g, m, v))
    p1, m1, v1 = oracle.adam_step(p64, g64, m64, v64, step, lr, beta1, beta2, eps, wd)
    delta = p1 - p64
    g_eff = g64 + wd * p64
    dg = 3 * u * (np.abs(g64) + np.abs(wd * p64)) if wd else np.zeros_like(g64)
    w = 1.0 - beta1
    tol_m = u * (np.abs(m1) + 4 * min(w, 1 - w) * (np.abs(g_eff) + np.abs(m64))) + w * dg
    tol_v_wd = 2 * (1.0 - beta2) * np.abs(g_eff) * dg
    tol_v = 1e-6 * np.abs(v1) + tol_v_wd
    denom = np.sqrt(v1) / math.sqrt(1 - beta2 ** step) + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        through_v = np.nan_to_num(np.abs(delta) * tol_v_wd / (2 * v1), posinf=0.0)
    tol_p = (1.5 * u * np.abs(p1) + 1e-5 * np.abs(delta) + lr / (1 - beta1 ** step) * tol_m / denom
             + through_v)
    return p1, m1, v1, delta, tol_p, tol_m, tol_v


def check_adam(got, ref, what=""):
    """One dense Adam step (param, exp_avg, exp_avg_sq) against adam_ref of
    the same input state, within adam_ref's bounds."""
    p, m, v = (np.asarray(a, np.float64) for a in got)
    rp, rm, rv, delta, tol_p, tol_m, tol_v = ref
    with np.errstate(divide="ignore", invalid="ignore"):
        use = [float(np.nanmax(np.abs(a - r) / t, initial=0.0))
               for a, r, t in ((p, rp, tol_p), (m, rm, tol_m), (v, rv, tol_v))]
        past = (np.abs(p - rp) - 2.0 ** -24 * np.abs(rp)) / np.abs(delta)
        rel = float(np.nanmax(np.where(delta != 0, past, 0.0), initial=0.0))
    print(f"{what} n={p.size}: largest error as a share of its bound: param {use[0]:.3g} "
          f"exp_avg {use[1]:.3g} exp_avg_sq {use[2]:.3g}; param error past one rounding, as a "
          f"share of the step: {rel:.3g}")
    assert np.all(np.abs(m - rm) <= tol_m), "exp_avg"
    assert np.all(np.abs(v - rv) <= tol_v), "exp_avg_sq"
    assert np.all(np.abs(p - rp) <= tol_p), "param"


# --------------------------------------------------------------------------- shared inputs
BPR_WIDTHS = [1, 31, 32, 33, 64, 96, 160, 192, 224, 257, 300, 384, 385, 512]  # every instance
ADAM_CASES = [(0.9, 0.999, 0.0), (0.3, 0.9, 0.0), (0.9, 0.999, 0.01)]  # beta1, beta2, weight decay
ADAM_SIZES = [1, 255, 10007, 4096 * 256 + 513]  # the last one runs the grid-stride loop


def adam_inputs(n, seed):
    """(param, three gradients, and the moments a late step starts from), fp32."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n).astype(F),
            [rng.standard_normal(n).astype(F) for _ in range(3)],
            (rng.standard_normal(n) * 0.1).astype(F),
            (rng.standard_normal(n) ** 2 * 0.5).astype(F))


def bpr_runs_case(d=100, seed=16):
    """The reference's m x m triple layout (users in order, each positive
    repeated m times in a row, the negatives cycled), with one user held for
    five consecutive blocks (2000 triples: about 125 groups flush into one
    gradient row) and one item id that is both a positive and a negative run
    of the same user."""
    rng = np.random.default_rng(seed)
    nu, ni, m, n_users = 50, 400, 20, 45
    U = (rng.standard_normal((nu, d)) * 0.3).astype(F)
    I = (rng.standard_normal((ni, d)) * 0.3).astype(F)
    users = rng.choice(nu, n_users)
    users[10:15] = users[10]
    pos = rng.integers(0, ni, (n_users, m))
    neg = rng.integers(0, ni, (n_users, m))
    neg[7, 4] = pos[7, 2]
    uid = np.repeat(users, m * m)
    pid = np.repeat(pos, m, axis=1).reshape(-1)
    nid = np.tile(neg, (1, m)).reshape(-1)
    return U, I, uid, pid, nid


RANK_ITEMS = 2000
RANK_LAYOUTS = 9


def rank_case(k, n_users, seed=0):
    """(recs int64 [n_users, k], rowptr, items): lists of distinct items and,
    user by user in turn, positives that are: the list from position 64 on;
    its first 64; the whole list; no listed item; exactly positions 63, 64 and
    k - 1; 12 random items with two repeated; 5000 random items (duplicates
    kept); none at all; one listed item."""
    rng = np.random.default_rng(1000 * k + n_users + seed)
    recs = np.stack([rng.choice(RANK_ITEMS, k, replace=False) for _ in range(n_users)])
    rows = []
    for u in range(n_users):
        r = recs[u]
        lay = (u + k) % RANK_LAYOUTS
        if lay == 0:
            rows.append(r[64:])
        elif lay == 1:
            rows.append(r[:64])
        elif lay == 2:
            rows.append(r)
        elif lay == 3:
            rows.append(np.setdiff1d(np.arange(RANK_ITEMS), r)[:40])
        elif lay == 4:
            rows.append(np.unique(r[[min(63, k - 1), min(64, k - 1), k - 1]]))
        elif lay == 5:
            some = rng.integers(0, RANK_ITEMS, 12)
            rows.append(np.concatenate([some, some[:2], r[:1], r[:1]]))
        elif lay == 6:
            rows.append(rng.integers(0, RANK_ITEMS, 5000))
        elif lay == 7:
            rows.append(np.zeros(0, np.int64))
        else:
            rows.append(r[k // 2:k // 2 + 1])
    return (recs,) + csr(rows)
