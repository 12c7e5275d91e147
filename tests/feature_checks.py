"""CPU side of the feature-composition tests (dr_csr_row_sum,
include/divrec_hip.h; FeatureMatrixFactorization): numpy restatements, the CSR
builders, the seeded inputs of tests/test_feature_gpu.py. No GPU, no torch.

Tolerance rule of the row sum. For row r with n_r entries, per element x,
    |out - ref64| <= (n_r + 8) * 2^-24 * sum_e |w_e * table[c_e, x]|
the standard bound of an n-term fp32 sum of products (each term passes through
at most n roundings of relative size 2^-24), with slack for the chunk adds: no
fixed order the kernel may choose has a deeper rounding path than
n_r + ceil(n_r / L). For bf16 output 2^-8 * |ref64| is added (one rounding to
8 significant bits). tests/test_feature_host.py shows the bound satisfiable:
the fp32 sequential restatement below stays inside it on every GPU case.
"""
import functools

import numpy as np

F = np.float32
L = 512  # ops.ROW_SUM_CHUNK, asserted equal by the host test
U24 = 2.0 ** -24


# --------------------------------------------------------------------------- CSR builders
def csr(rows, w=None):
    """Lists of per-row columns (and weights) -> (rowptr int64, cols int32,
    weights float32 or None)."""
    rowptr = np.zeros(len(rows) + 1, np.int64)
    rowptr[1:] = np.cumsum([len(x) for x in rows])
    cols = np.concatenate([np.asarray(x, np.int64) for x in rows] + [np.zeros(0, np.int64)])
    weights = None
    if w is not None:
        weights = np.concatenate([np.asarray(x, F) for x in w] + [np.zeros(0, F)]).astype(F)
    return rowptr, cols.astype(np.int32), weights


def row_of_entry(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def transpose(rowptr, cols, weights, n_cols):
    """The transposed CSR by a stable sort by column: transposed row c lists
    its source rows ascending, repeated entries in their original order."""
    order = np.argsort(cols, kind="stable")
    rowptr_t = np.zeros(n_cols + 1, np.int64)
    rowptr_t[1:] = np.cumsum(np.bincount(cols.astype(np.int64), minlength=n_cols))
    return (rowptr_t, row_of_entry(rowptr)[order].astype(np.int32),
            None if weights is None else weights[order])


def dense(rowptr, cols, weights, n_cols):
    """The small dense form S [n_rows, n_cols] (float64), repeats summed."""
    S = np.zeros((len(rowptr) - 1, n_cols))
    w = np.ones(len(cols)) if weights is None else weights.astype(np.float64)
    np.add.at(S, (row_of_entry(rowptr), cols.astype(np.int64)), w)
    return S


def feature_csr_np(n, categorical=(), numeric=(), identity=True, vocab=None):
    """divrec.datasets.feature_csr restated: ``categorical`` / ``numeric`` are
    lists of [n] arrays. Returns (rowptr, cols, weights, n_features, vocab);
    with ``vocab`` (a former call's: (list of value arrays, their offsets,
    numeric ids, n_features)) new rows are mapped into that space: no identity
    entry, unknown values dropped."""
    rows, w = [[] for _ in range(n)], [[] for _ in range(n)]
    new = vocab is None
    nxt = 0
    if new:
        values, offs, num_ids = [], [], []
        if identity:
            for r in range(n):
                rows[r].append(r), w[r].append(1.0)
            nxt = n
    else:
        values, offs, num_ids, n_features = vocab
    for j, col in enumerate(categorical):
        col = np.asarray(col)
        ok = (col >= 0) & (col == np.floor(col))
        if new:
            values.append(np.unique(col[ok].astype(np.int64)))
            offs.append(nxt)
            nxt += len(values[j])
        for r in range(n):
            if ok[r] and int(col[r]) in values[j]:
                rows[r].append(offs[j] + int(np.searchsorted(values[j], int(col[r]))))
                w[r].append(1.0)
    for j, col in enumerate(numeric):
        if new:
            num_ids.append(nxt)
            nxt += 1
        for r in range(n):
            rows[r].append(num_ids[j]), w[r].append(float(col[r]))
    if new:
        n_features = nxt
    return csr(rows, w) + (n_features, (values, offs, num_ids, n_features))


# --------------------------------------------------------------------------- the row sum
def row_sum_f64(table, rowptr, cols, weights):
    """(out float64 [n, d], mag float64 [n, d] = sum_e |w_e table[c_e]|, n_r):
    entries with a column outside the table add nothing."""
    T = np.asarray(table, np.float64)
    n, (m, d) = len(rowptr) - 1, T.shape
    c = cols.astype(np.int64)
    ok = (c >= 0) & (c < m)
    w = (np.ones(len(c)) if weights is None else weights.astype(np.float64)) * ok
    terms = w[:, None] * T[np.where(ok, c, 0)]
    out, mag = np.zeros((n, d)), np.zeros((n, d))
    rows = row_of_entry(rowptr)
    np.add.at(out, rows, terms)
    np.add.at(mag, rows, np.abs(terms))
    return out, mag, np.diff(rowptr)


def row_sum_f32_sequential(table, rowptr, cols, weights, chunk=L):
    """The kernel's order restated in fp32 without FMA: a row's entries in
    chunks of ``chunk``, each summed from 0 in entry order (product rounded,
    then the add), the chunk sums added in chunk order. float32 [n, d]."""
    T = np.asarray(table, F)
    n, (m, d) = len(rowptr) - 1, T.shape
    c = cols.astype(np.int64)
    ok = (c >= 0) & (c < m)
    w = np.where(ok, F(1) if weights is None else weights.astype(F), F(0)).astype(F)
    c = np.where(ok, c, 0)
    out = np.zeros((n, d), F)
    # all chunks advance together, one entry position at a time
    beg = np.concatenate([np.arange(rowptr[r], max(rowptr[r + 1], rowptr[r] + 1), chunk)
                          for r in range(n)]).astype(np.int64)
    owner = np.concatenate([np.full(len(range(rowptr[r], max(rowptr[r + 1], rowptr[r] + 1), chunk)), r)
                            for r in range(n)])
    end = np.minimum(beg + chunk, rowptr[owner + 1])
    acc = np.zeros((len(beg), d), F)
    for p in range(chunk):
        live = np.nonzero(beg + p < end)[0]
        if not len(live):
            break
        e = beg[live] + p
        acc[live] = acc[live] + (w[e][:, None] * T[c[e]]).astype(F)
    first = np.ones(len(beg), bool)
    first[1:] = owner[1:] != owner[:-1]
    for k in range(len(beg)):  # chunk order within a row
        out[owner[k]] = acc[k] if first[k] else out[owner[k]] + acc[k]
    return out


def bound(mag, n_r, ref64=None, bf16=False):
    b = (n_r[:, None] + 8) * U24 * mag
    return b + 2.0 ** -8 * np.abs(ref64) if bf16 else b


def check_row_sum(got, ref, bf16=False, what=""):
    """``got`` [n, d] (any float dtype) against row_sum_f64's triple under the rule."""
    out64, mag, n_r = ref
    got = np.asarray(got, np.float64)
    assert got.shape == out64.shape, what
    assert not np.isnan(got).any(), f"{what}: NaN left in the output (an unwritten row?)"
    tol = bound(mag, n_r, out64, bf16)
    err = np.abs(got - out64)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = float(np.nanmax(np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0)),
                                initial=0.0))
    print(f"{what} n={got.shape[0]} d={got.shape[1]}: max abs err {err.max(initial=0.0):.3g}, "
          f"largest share of the bound {share:.3g}")
    assert np.all(err <= tol), what


# --------------------------------------------------------------------------- cases
WIDTHS = (8, 100, 128, 260)
ROW_COUNTS = (1, 7, 4097)
SPECIAL = (0, 1, L - 1, L, L + 1, 3 * L + 5)
TABLE_ROWS = 300


def case_lengths(n_rows, d, rng):
    """Row lengths of a case: the special lengths wherever there is room (a
    one-row case takes one of them, by width), a long row LAST."""
    if n_rows == 1:
        return [SPECIAL[(2 + WIDTHS.index(d)) % len(SPECIAL)] if d != 260 else 3 * L + 5]
    if n_rows == 7:
        return [1, 0, L - 1, L, L + 1, 2, 3 * L + 5]
    lens = rng.integers(0, 13, n_rows).tolist()
    for k, s in enumerate(SPECIAL):
        lens[17 + 300 * k] = s
    lens[-1] = 3 * L + 5
    return lens


@functools.lru_cache(maxsize=None)
def case(d, n_rows, integer=False):
    """(table fp32 [300, d], rowptr, cols, weights or None) of one kernel
    case, seeded by its shape. Weights: NULL on every other case, else given
    with a tenth of them zero. A repeated column is forced into every row of at
    least two entries among the first rows. ``integer``: table values in
    [-3, 3] and weights in [-2, 2], integers, so that every sum is exact."""
    rng = np.random.default_rng(1000 * d + n_rows)
    lens = case_lengths(n_rows, d, rng)
    rows = [rng.integers(0, TABLE_ROWS, n) for n in lens]
    for r in rows[:64]:
        if len(r) >= 2:
            r[1] = r[0]
    weighted = (WIDTHS.index(d) + ROW_COUNTS.index(n_rows)) % 2 == 0
    if integer:
        T = rng.integers(-3, 4, (TABLE_ROWS, d)).astype(F)
        w = [rng.integers(-2, 3, n).astype(F) for n in lens]
    else:
        T = rng.standard_normal((TABLE_ROWS, d)).astype(F)
        w = [np.where(rng.random(n) < 0.1, 0.0, rng.uniform(-2.0, 2.0, n)).astype(F) for n in lens]
    return (T,) + csr(rows, w if weighted else None)


@functools.lru_cache(maxsize=None)
def case_ref(d, n_rows, integer=False):
    return row_sum_f64(*case(d, n_rows, integer))


def independence_rows(seed=3):
    """The three rows of the independence test (short, exactly L, 3 L + 5) as
    (cols, weights) lists over TABLE_ROWS columns."""
    rng = np.random.default_rng(seed)
    lens = (5, L, 3 * L + 5)
    return ([rng.integers(0, TABLE_ROWS, n) for n in lens],
            [rng.uniform(-2.0, 2.0, n).astype(F) for n in lens])


def skew_map(n_rows=5000, n_single=200, seed=9):
    """A 5000-row map (rowptr, cols, weights, n_features): feature 0 is held
    by EVERY row, features 1 .. 200 by one row each, 30 more features at random."""
    rng = np.random.default_rng(seed)
    n_features = 1 + n_single + 30
    rows = [[0] + rng.integers(1 + n_single, n_features, 2).tolist() for _ in range(n_rows)]
    for f, r in enumerate(rng.choice(n_rows, n_single, replace=False)):
        rows[r].append(1 + f)
    w = [rng.uniform(0.5, 1.5, len(x)).astype(F) for x in rows]
    return csr(rows, w) + (n_features,)


# --------------------------------------------------------------------------- training, float64
def planted(n_users=200, n_items=300, n_genres=12, per_user=8, seed=21):
    """The planted-structure data: every item has one of 12 genres, every user
    likes two genres and its positives are drawn from them. Returns
    (interactions int64 [n, 2], item genre int64 [n_items])."""
    rng = np.random.default_rng(seed)
    genre = rng.integers(0, n_genres, n_items)
    pairs = []
    for u in range(n_users):
        liked = rng.choice(n_genres, 2, replace=False)
        pool = np.nonzero(np.isin(genre, liked))[0]
        for i in rng.choice(pool, min(per_user, len(pool)), replace=False):
            pairs.append((u, int(i)))
    return np.asarray(pairs, np.int64), genre.astype(np.int64)


def planted_triples(pairs, n_items, negatives=4, seed=0):
    """(uid, pid, nid): every positive with ``negatives`` uniform non-positives."""
    rng = np.random.default_rng(seed)
    pos = {}
    for u, i in pairs:
        pos.setdefault(int(u), set()).add(int(i))
    uid, pid, nid = [], [], []
    for u, i in pairs:
        for _ in range(negatives):
            j = int(rng.integers(0, n_items))
            while j in pos[int(u)]:
                j = int(rng.integers(0, n_items))
            uid.append(u), pid.append(i), nid.append(j)
    return tuple(np.asarray(a, np.int64) for a in (uid, pid, nid))


def bpr_f64(U, I, uid, pid, nid):
    """(mean loss, grad_U, grad_I) of the 'mean' reduction in float64."""
    u, p, n = U[uid], I[pid], I[nid]
    x = np.sum(u * (p - n), axis=1)
    loss = np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    e = np.exp(-np.abs(x))
    g = (-np.where(x >= 0, e / (1.0 + e), 1.0 / (1.0 + e)) / len(x))[:, None]
    gU, gI = np.zeros_like(U), np.zeros_like(I)
    np.add.at(gU, uid, g * (p - n))
    np.add.at(gI, pid, g * u)
    np.add.at(gI, nid, -g * u)
    return float(loss.mean()), gU, gI


class AdamF64:
    """torch.optim.Adam's plain update in float64, one state per table."""

    def __init__(self, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        self.lr, self.b1, self.b2, self.eps, self.t, self.state = lr, beta1, beta2, eps, 0, {}

    def step(self, tables, grads):
        self.t += 1
        for k, (p, g) in enumerate(zip(tables, grads)):
            m, v = self.state.get(k, (np.zeros_like(p), np.zeros_like(p)))
            m = self.b1 * m + (1 - self.b1) * g
            v = self.b2 * v + (1 - self.b2) * g * g
            self.state[k] = (m, v)
            denom = np.sqrt(v) / np.sqrt(1 - self.b2 ** self.t) + self.eps
            p -= self.lr / (1 - self.b1 ** self.t) * m / denom


def feature_step_f64(Wu, Wi, Su, Si, batch, adam):
    """One whole training step in float64, in place: compose (S @ W) -> BPR
    gradients of the composed tables -> transposed sums (S^T @ g) -> Adam.
    Returns the batch's mean loss (before the step)."""
    U, I = Su @ Wu, Si @ Wi
    loss, gU, gI = bpr_f64(U, I, *batch)
    adam.step((Wu, Wi), (Su.T @ gU, Si.T @ gI))
    return loss


def train_f64(Wu, Wi, Su, Si, triples, epochs, batch_size, lr):
    """Epoch-mean losses of ``epochs`` passes over ``triples`` in order."""
    Wu, Wi = Wu.astype(np.float64).copy(), Wi.astype(np.float64).copy()
    adam, hist = AdamF64(lr), []
    n = len(triples[0])
    for _ in range(epochs):
        losses = [feature_step_f64(Wu, Wi, Su, Si, tuple(t[b:b + batch_size] for t in triples), adam)
                  for b in range(0, n, batch_size)]
        hist.append(float(np.mean(losses)))
    return hist


def adam_first_step_tolerance(g64, lr, eps=1e-8, g_rtol=1e-4, g_atol=1e-7):
    """How far the FIRST Adam step p - lr g / (|g| + eps) may move when the
    gradient is only known to tests/pairwise_checks.py's BPR gradient tolerance
    (rtol 1e-4, atol 1e-7: fp32 atomics reorder its sums): the step's slope in
    g is lr eps / (|g| + eps)^2, taken at the smallest |g| the tolerance
    allows; never more than the step's full range 2 lr."""
    dg = g_rtol * np.abs(g64) + g_atol
    low = np.maximum(np.abs(g64) - dg, 0.0)
    return np.minimum(lr * eps / (low + eps) ** 2 * dg, 2 * lr)
