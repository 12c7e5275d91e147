"""CPU side of the MMR re-rank tests (dr_mmr_rerank, include/divrec_hip.h): the
kernel's arithmetic restated in fp32 for one user, the same greedy in int64 for
inputs on which every value is exact, the float64 replay that judges a kernel's
picks within a tolerance, and the seeded inputs of tests/test_mmr_gpu.py. No
GPU, no torch.

The contract (header comment of dr_mmr_rerank):

* a live candidate's score is max(s, -FLT_MAX), NaN counting as -FLT_MAX;
* 1/|e| = 0 for a row whose fp32 sum of squares is 0, so its cosine with every
  row (itself included) is 0 and it stays eligible on its score;
* dead slots are ids < 0 and ids >= n_items; ties go to the lowest position;
  the list ends in -1 once nobody is live.

Exact inputs. Item rows have entries in {-1, 0, +1} with exactly nnz non-zeros,
nnz = 64 or 16, so the sum of squares is nnz, 1/|e| is exactly 0.125 or 0.25 and
a cosine is b / nnz, b the integer dot product. Scores are a / 64 and lam is
L / 256 with L in {0, 64, 128, 192, 256}. Every product and sum of the kernel is
then exact in fp32 (a value is an integer below 2^24 over 2^14 nnz), and
L a nnz - (256 - L) 64 max_b is that value in integers: ``mmr_greedy_int`` is
the one right answer, ties included, and a kernel's list must equal it element
for element. This rests on the library's build: build_native.py passes no
fast-math flag, so HIP's fp32 divide and sqrt are the correctly rounded ones
(1 / sqrt(64) is exactly 0.125) and the fma is not contracted differently.

TOL_V = 1e-4 bounds the value gap of a pick to the step's best value in the
float64 replay (``mmr_check_positions``). ``measure_value_gap`` (python
tests/mmr_checks.py) measures the worst |value_fp32 - value_float64| of the
fp32 restatement over every live candidate at every step of the float inputs
of tests/test_mmr_gpu.py: 8.94e-8 (FLOAT_SHAPES in order: 8.94e-8 at d = 1,
5.96e-8 at d = 32, 4.99e-8 at d = 100, 4.44e-8 at d = 128). TOL_V is 1118 times
that; at least 10 times is asked, the factor 10 standing for the kernel's
different summation order at the same precision (the reasoning of dpp_checks.py).
"""
import numpy as np

import oracle

FLT_MAX = float(np.finfo(np.float32).max)
TOL_V = 1e-4
VALUE_GAP_F32 = 8.94e-8  # measure_value_gap, CPU
F = np.float32
_ORD_NEG_INF = 0x007FFFFF  # the key of -inf: what the kernel's dead slots carry


def _ord(val):
    """fp32 values -> the kernel's 32-bit value order as int64 (-0 counts as
    +0; NaN sorts above +inf, as a positive quiet NaN's bits do)."""
    v = np.asarray(val, dtype=F) + F(0)
    u = v.view(np.uint32).astype(np.int64)
    o = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(v), 0xFFFFFFFF, o)


def _live(cand, n_items):
    cand = np.asarray(cand, dtype=np.int64)
    return cand, (cand >= 0) & (cand < n_items)


def contract_scores(sc):
    """-inf and NaN count as -FLT_MAX."""
    s = np.asarray(sc, dtype=np.float64)
    return np.maximum(np.where(np.isnan(s), -FLT_MAX, s), -FLT_MAX)


def _greedy_f32(cand, sc, E, k, lam, n_items, zero_rule, on_step=None):
    assert zero_rule in ("contract", "old")
    cand, live = _live(cand, E.shape[0] if n_items is None else n_items)
    X = E[np.where(live, cand, 0)].astype(np.float64)
    nsq = (X * X).sum(1).astype(F)
    s = np.asarray(sc, dtype=F)
    with np.errstate(all="ignore"):
        if zero_rule == "contract":
            inv = np.where(nsq > 0, F(1) / np.sqrt(np.where(nsq > 0, nsq, F(1))), F(0)).astype(F)
            s = contract_scores(s).astype(F)
        else:
            inv = (F(1) / np.sqrt(nsq)).astype(F)
        lamf = F(lam)
        mu = F(1) - lamf
        ls = (lamf * s).astype(F)
        pen = np.full(len(cand), -np.inf, dtype=F)
        pos = np.full(k, -1, dtype=np.int64)
        for t in range(k):
            if not live.any():
                break
            # one rounding: the product is exact in float64
            val = ls if t == 0 else (-np.float64(mu) * pen.astype(np.float64)
                                     + ls.astype(np.float64)).astype(F)
            key = np.where(live, _ord(val), -1)
            j = int(np.argmax(key))  # the first maximum: the lowest position
            if zero_rule == "old" and key[j] <= _ORD_NEG_INF:
                break  # a value of -inf is a dead slot's key: "the rest are -1"
            if on_step is not None:
                on_step(t, val, live, j)
            pos[t] = j
            live[j] = False
            acc = (X @ X[j]).astype(F)
            pen = np.fmax(pen, (acc * inv) * inv[j])  # fmax drops NaN, as fmaxf does
    return pos


def mmr_greedy_f32(cand, sc, E, k, lam, n_items=None, zero_rule="contract"):
    """The kernel's arithmetic restated for one user: positions [k] in pick
    order, -1 once nobody is live. inv = 1 / sqrt(sum of squares) and cos =
    (acc * inv_c) * inv_p in fp32, acc the exact dot product rounded once; the
    first value is lam * s, later ones the single-rounded fma(-mu, pen, lam * s)
    with mu = fp32(1) - fp32(lam); the first maximum wins. zero_rule "old" keeps
    the behaviour before the contract (inv = inf for a zero row, scores as they
    come, a live value of -inf taken for a dead slot): it exists so the host
    tests can show that an input tells the two rules apart."""
    return _greedy_f32(cand, sc, E, k, lam, n_items, zero_rule)


def mmr_greedy_int(cand, sc, E, k, lam, n_items=None, trace=False):
    """The same greedy in int64 on exact inputs (module docstring), zero rows
    under the contract included (b = 0). Returns (positions [k], the number of
    steps at which two or more live candidates share the maximum); with
    ``trace`` also the picked value of every step, in units of 1 / (2^14 nnz)."""
    cand, live = _live(cand, E.shape[0] if n_items is None else n_items)
    X = np.rint(E[np.where(live, cand, 0)]).astype(np.int64)
    assert np.array_equal(X, E[np.where(live, cand, 0)]) and np.abs(X).max() <= 1
    nsq = (X * X).sum(1)
    n = int(nsq.max())
    assert n in (16, 64) and np.isin(nsq, (0, n)).all()
    a = np.rint(np.asarray(sc, dtype=np.float64) * 64).astype(np.int64)
    assert np.array_equal(a / 64.0, np.asarray(sc, dtype=np.float64))
    L = int(round(lam * 256))
    assert L / 256.0 == lam and L in (0, 64, 128, 192, 256)
    pos = np.full(k, -1, dtype=np.int64)
    max_b, ties, values = np.zeros(len(cand), dtype=np.int64), 0, []
    lowest = np.iinfo(np.int64).min
    for t in range(k):
        if not live.any():
            break
        val = np.where(live, L * a * n - (256 - L) * 64 * max_b, lowest)
        j = int(np.argmax(val))
        ties += int((val == val[j]).sum() > 1)
        values.append(int(val[j]))
        pos[t] = j
        live[j] = False
        b = X @ X[j]
        max_b = b if t == 0 else np.maximum(max_b, b)
    return (pos, ties, values) if trace else (pos, ties)


def mmr_check_positions(picks, cand, sc, E, lam, tol):
    """float64 replay that also handles invalid candidates (-1, or an id past
    the table): each pick must be a live candidate whose MMR value is within tol
    of the step maximum, and -1 must appear exactly when no live candidate is
    left. Under the contract: a zero-norm row has cosine 0 with every row, and
    -inf and NaN scores count as -FLT_MAX."""
    bad = 0
    for u in range(cand.shape[0]):
        valid = (cand[u] >= 0) & (cand[u] < E.shape[0])
        X = E[np.where(valid, cand[u], 0)].astype(np.float64)
        nrm = np.linalg.norm(X, axis=1, keepdims=True)
        nrm[(X.astype(F) ** 2).sum(1, dtype=F) == 0] = np.inf  # fp32 sum of squares 0: cosine 0
        Xn = X / nrm
        sims = Xn @ Xn.T
        s = contract_scores(sc[u])
        alive = valid.copy()
        pen = None
        for it in picks[u]:
            if not alive.any():
                bad += int(it != -1)
                continue
            val = lam * s - (1 - lam) * (pen if pen is not None else 0.0)
            val[~alive] = -np.inf
            hits = np.nonzero(alive & (cand[u] == it))[0]
            if len(hits) == 0 or val[hits].max() < val.max() - tol:
                bad += 1
                continue
            j = hits[np.argmax(val[hits])]
            alive[j] = False
            pen = sims[:, j] if pen is None else np.maximum(pen, sims[:, j])
    return bad


def mmr_greedy_f64(cand, sc, E, k, lam):
    """The spec in float64 for one user (positions [k]), by the replay's own
    arithmetic: what the replay must accept."""
    cand, live = _live(cand, E.shape[0])
    X = E[np.where(live, cand, 0)].astype(np.float64)
    nrm = np.linalg.norm(X, axis=1, keepdims=True)
    nrm[nrm == 0] = np.inf
    Xn = X / nrm
    s = contract_scores(sc)
    pos = np.full(k, -1, dtype=np.int64)
    pen = np.zeros(len(cand))
    for t in range(k):
        if not live.any():
            break
        j = int(np.argmax(np.where(live, lam * s - (1 - lam) * pen, -np.inf)))
        pos[t] = j
        live[j] = False
        sim = Xn @ Xn[j]
        pen = sim if t == 0 else np.maximum(pen, sim)
    return pos


def value_gap_f32(cand, sc, E, k, lam):
    """Worst |value_fp32 - value_float64| over the live candidates and steps of
    one user, the float64 max terms following the fp32 restatement's picks."""
    cand, live = _live(cand, E.shape[0])
    X = E[np.where(live, cand, 0)].astype(np.float64)
    nrm = np.linalg.norm(X, axis=1, keepdims=True)
    nrm[nrm == 0] = np.inf
    Xn = X / nrm
    s = contract_scores(sc)
    state = {"pen": np.zeros(len(cand)), "worst": 0.0}

    def on_step(t, val, alive, j):
        v64 = lam * s - (1 - lam) * state["pen"]
        state["worst"] = max(state["worst"], float(np.abs(val.astype(np.float64) - v64)[alive].max()))
        sim = Xn @ Xn[j]
        state["pen"] = sim if t == 0 else np.maximum(state["pen"], sim)

    _greedy_f32(cand, sc, E, k, lam, None, "contract", on_step)
    return state["worst"]


def picks_of(cand, pos):
    """Item ids of positions (-1 stays -1)."""
    cand, pos = np.asarray(cand), np.asarray(pos)
    return np.where(pos >= 0, cand[np.maximum(pos, 0)], -1).astype(np.int32)


def stable_topk(cand, sc, k):
    order = np.argsort(-sc, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(cand, order, axis=1)


# --------------------------------------------------------------------------- inputs
NI = 3000  # rows of every seeded table


def exact_table(rng, ni, d, nnz):
    """Rows with entries in {-1, 0, +1}, exactly nnz non-zeros each."""
    E = np.zeros((ni, d), dtype=np.float32)
    cols = np.argsort(rng.random((ni, d)), axis=1)[:, :nnz]
    np.put_along_axis(E, cols, rng.choice(np.array([-1.0, 1.0], dtype=np.float32), (ni, nnz)), axis=1)
    return E


def _lists(rng, ni, n, C):
    return np.stack([rng.choice(ni, C, replace=False) for _ in range(n)]).astype(np.int32)


def _scores64(rng, shape):
    return (rng.integers(0, 64, shape) / 64.0).astype(np.float32)


# (d, nnz, C, k_out, lam): 100 and 32 are padded widths; C = k_out = 1024 empties
# every tile of every wave; C around 8 and 64 leaves waves with 0, 1, 8 or 9
# candidates; the last is lam = 1, the stable top-k by score
EXACT_SHAPES = ([(64, 64, 1024, 100, .5), (128, 64, 1000, 100, .25), (128, 64, 777, 64, .75),
                 (64, 16, 300, 300, .5), (64, 64, 1024, 1024, .5), (128, 64, 1024, 1024, 0.),
                 (100, 64, 513, 100, .5), (32, 16, 257, 257, .25)]
                + [(128, 64, C, C, .5) for C in (1, 2, 7, 8, 9, 63, 64, 65)]
                + [(64, 64, 1024, 100, 1.)])
# Short lists tie too rarely with 64 score levels: below C = 128 the scores take
# C // 8 levels (one level below 16: the max term alone decides), and the seeds
# of C = 7, 8, 9 are the first at which a third of the steps tie (a condition on
# the input that mmr_greedy_int alone decides; a list of one cannot tie).
_SEEDS = {7: 10, 8: 1, 9: 5}


def exact_inputs(d, nnz, C, n=3):
    """(cand [n, C] of distinct items, scores a / 64 in [0, 1), E) of one shape."""
    rng = np.random.default_rng(_SEEDS.get(C, 0) + 100000 * d + 1000 * nnz + C)
    E = exact_table(rng, NI, d, nnz)
    cand = _lists(rng, NI, n, C)
    levels = 64 if C >= 128 else max(1, C // 8)
    return cand, (rng.integers(0, levels, (n, C)) / 64.0).astype(np.float32), E


FOLD_SHAPES = [(64, .5), (128, .5), (64, .25), (128, .25)]  # (d, lam), C = k_out = 72


def fold_inputs(d):
    """C = 72: positions 64..71 score -4, the rest a / 64 in [0, 1). Wave w owns
    the positions = w (mod 8): eight probes and one far-away bound, so the batch
    after the first pick makes 63 picks and folds them in passes of 32 + 31."""
    rng = np.random.default_rng(7200 + d)
    E = exact_table(rng, NI, d, 64)
    sc = _scores64(rng, (3, 72))
    sc[:, 64:] = -4.0
    return _lists(rng, NI, 3, 72), sc, E


def dup_inputs(layout):
    """64 distinct items, 16 copies each with equal scores, C = 1024, d = 128.
    "tile": copies 64 apart, all 16 in one wave (nine or more equal top values
    in that wave: forced picks); "repeat": copies in a run, two per wave (ties
    across waves, and between a probe and a bound)."""
    rng = np.random.default_rng({"tile": 640, "repeat": 641}[layout])
    E = exact_table(rng, NI, 128, 64)
    items, sc = _lists(rng, NI, 3, 64), _scores64(rng, (3, 64))
    if layout == "tile":
        return np.tile(items, (1, 16)), np.tile(sc, (1, 16)), E
    return np.repeat(items, 16, axis=1), np.repeat(sc, 16, axis=1), E


def zero_norm_inputs():
    """d = 128, C = 300, exact; the table's last three rows are zero. User 0: a
    zero row with the best score (1.0: the first pick); user 1: one in the
    middle of the picks (score 0.875); user 2: three at once (1.0, 0.875, 0.75)."""
    rng = np.random.default_rng(300)
    E = np.concatenate([exact_table(rng, NI, 128, 64), np.zeros((3, 128), np.float32)])
    cand, sc = _lists(rng, NI, 3, 300), _scores64(rng, (3, 300))
    for u, at, ids, s in ((0, [5], [NI], [1.0]), (1, [150], [NI + 1], [0.875]),
                          (2, [3, 77, 200], [NI, NI + 1, NI + 2], [1.0, 0.875, 0.75])):
        cand[u, at], sc[u, at] = ids, s
    return cand, sc, E


def nonfinite_inputs(C):
    """d = 128, exact, with -inf (user 0), NaN (user 1) and both (user 2) on a
    fifth of the live candidates (at least 4)."""
    rng = np.random.default_rng(900 + C)
    E = exact_table(rng, NI, 128, 64)
    cand, sc = _lists(rng, NI, 3, C), _scores64(rng, (3, C))
    m = max(4, C // 5)
    for u, vals in ((0, [-np.inf]), (1, [np.nan]), (2, [-np.inf, np.nan])):
        at = rng.choice(C, m, replace=False)
        sc[u, at] = np.resize(np.array(vals, dtype=np.float32), m)
    return cand, sc, E


def independence_inputs():
    """7 users, C = 1024, d = 128, exact. With two workgroups, workgroup 0 runs
    users 0, 2, 4, 6 (full, all -1, three live candidates, full) and workgroup 1
    users 1, 3, 5 (a zero-norm first pick, full, 60 finite scores and a -inf
    tail)."""
    rng = np.random.default_rng(1024)
    E = np.concatenate([exact_table(rng, NI, 128, 64), np.zeros((1, 128), np.float32)])
    cand, sc = _lists(rng, NI, 7, 1024), _scores64(rng, (7, 1024))
    cand[2] = -1
    keep = cand[4, [9, 500, 1001]].copy()
    cand[4] = -1
    cand[4, [9, 500, 1001]] = keep
    cand[1, 130], sc[1, 130] = NI, 1.0
    sc[5, 60:] = -np.inf
    return cand, sc, E


# (d, C, k_out, lam): widths and the full-length list that no other test runs
FLOAT_SHAPES = [(1, 200, 50, .5), (32, 500, 100, .5), (100, 777, 100, .5), (128, 1024, 1024, .5)]


def float_inputs(d, C, n=4):
    """Rows of bf16-rounded N(0, 1 / sqrt(d)), scores sorted descending."""
    rng = np.random.default_rng(5000 * d + C)
    E = oracle.as_bf16_f32((rng.standard_normal((NI, d)) / np.sqrt(d)).astype(np.float32))
    sc = -np.sort(-rng.random((n, C)), axis=1).astype(np.float32)
    return _lists(rng, NI, n, C), sc, E


def measure_value_gap():
    worst_all = 0.0
    for d, C, k, lam in FLOAT_SHAPES:
        cand, sc, E = float_inputs(d, C)
        worst = max(value_gap_f32(cand[u], sc[u], E, k, lam) for u in range(len(cand)))
        print(f"d={d:4d} C={C:5d} k_out={k:5d} lam={lam}: worst |v32 - v64| = {worst:.2e}")
        worst_all = max(worst_all, worst)
    print(f"worst over all inputs: {worst_all:.2e}; TOL_V / worst = {TOL_V / worst_all:.0f}")
    return worst_all


if __name__ == "__main__":
    measure_value_gap()
