"""CPU side of the ALS tests (dr_als_solve, include/divrec_hip.h): the spec as
a numpy restatement in a chosen precision, the objective, a brute-force
transpose, and the seeded inputs of tests/test_als_gpu.py. No GPU, no torch.

Tolerance rule (the project's usual one): for a case, ``E_ref`` is the error of
the float32 restatement against the float64 one,
``max over non-empty rows of |x32 - x64|_2 / |x64|_2`` (``rel_err``), and the
kernel must satisfy the same quantity <= ``FACTOR`` * ``E_ref``, computed in
the test for that case. FACTOR = 10: the kernel sums and eliminates in another
order than LAPACK, which moves error constants by small factors, while every
defect worth catching (a dropped chunk tail, a wrong weight, a missing reg, a
transposed tile, a stale LDS read) moves x by 1e-3 or more. With N(0, 1)
tables and alpha = 2, E_ref is 4e-7 to 7e-7 on the well-conditioned cases and
about 1e-5 on the 128 x 160 one (kappa(G + reg I) about 270).
"""
import numpy as np

FACTOR = 10.0
ALPHA = 2.0
CHUNK = 32   # item rows per LDS buffer of the kernel (csrc/als.hip kChunk)
N_ROWS = 70
# (d, fixed rows, reg): every row is judged
CASES = [(32, 300, 0.1), (64, 600, 0.1), (128, 600, 0.1), (128, 600, 1e-3), (100, 500, 0.05)]
ILL = (128, 160, 0.1)  # fewer than 2 d rows: kappa(G + reg I) about 270


def gram32(Y):
    """Y^T Y in float64, symmetric, rounded once to float32 (ops.gram)."""
    g = Y.astype(np.float64).T @ Y.astype(np.float64)
    return ((g + g.T) * 0.5).astype(np.float32)


def solve(Y, rows, w, alpha, reg, dtype):
    """x_r = (G + alpha sum_i w_i y_i y_i^T + reg I)^-1 sum_i (1 + alpha w_i) y_i
    for every row, assembled and solved (np.linalg.cholesky) in ``dtype``;
    float64 [n, d]. ``rows``: a list of index arrays, ``w``: a list of weight
    arrays or None. Indices outside the table must have been removed."""
    dt = np.dtype(dtype).type
    Yd, G = Y.astype(dtype), gram32(Y).astype(dtype)
    d = Y.shape[1]
    out = np.zeros((len(rows), d))
    for r, idx in enumerate(rows):
        if len(idx) == 0:
            continue
        Yr = Yd[np.asarray(idx, dtype=np.int64)]
        wr = (np.ones(len(idx)) if w is None else np.asarray(w[r])).astype(dtype)
        A = G + dt(alpha) * ((Yr.T * wr) @ Yr) + dt(reg) * np.eye(d, dtype=dtype)
        b = ((dt(1) + dt(alpha) * wr)[:, None] * Yr).sum(0, dtype=dtype)
        L = np.linalg.cholesky(A)
        assert L.dtype == np.dtype(dtype)
        out[r] = np.linalg.solve(L.T, np.linalg.solve(L, b))
    return out


def rel_err(x, x64, rows):
    """max over non-empty rows of |x - x64|_2 / |x64|_2."""
    worst = 0.0
    for r, idx in enumerate(rows):
        if len(idx):
            worst = max(worst, float(np.linalg.norm(x[r] - x64[r]) / np.linalg.norm(x64[r])))
    return worst


def objective(X, Y, rows, w, alpha, reg):
    """J = sum_r [x_r^T G x_r + sum_{i in r} (c (1 - s)^2 - s^2)] + reg (|X|^2 + |Y|^2)
    in float64, G = Y^T Y unrounded."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    G = Y.T @ Y
    J = float(((X @ G) * X).sum()) + reg * float((X * X).sum() + (Y * Y).sum())
    for r, idx in enumerate(rows):
        if len(idx):
            s = Y[np.asarray(idx, dtype=np.int64)] @ X[r]
            c = 1.0 + alpha * (np.ones(len(idx)) if w is None else np.asarray(w[r], dtype=np.float64))
            J += float((c * (1.0 - s) ** 2 - s * s).sum())
    return J


def objective_dense(X, Y, rows, w, alpha, reg):
    """The same J as the sum over ALL pairs of c (p - s)^2 (rows without
    repeated columns)."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    C, P = np.ones((X.shape[0], Y.shape[0])), np.zeros((X.shape[0], Y.shape[0]))
    for r, idx in enumerate(rows):
        for k, i in enumerate(idx):
            C[r, i] = 1.0 + alpha * (1.0 if w is None else float(w[r][k]))
            P[r, i] = 1.0
    return float((C * (P - X @ Y.T) ** 2).sum()) + reg * float((X * X).sum() + (Y * Y).sum())


def transpose(rows, w, n_cols):
    """(rows, w) of the transposed pattern by brute force; columns ascending."""
    t_rows, t_w = [[] for _ in range(n_cols)], [[] for _ in range(n_cols)]
    for r, idx in enumerate(rows):
        for k, i in enumerate(idx):
            t_rows[int(i)].append(r)
            t_w[int(i)].append(1.0 if w is None else float(w[r][k]))
    return ([np.asarray(x, dtype=np.int64) for x in t_rows],
            None if w is None else [np.asarray(x, dtype=np.float32) for x in t_w])


def csr(rows, w=None):
    """(rowptr int64 [n + 1], cols int32, weights float32 or None)."""
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(x) for x in rows])
    cols = np.concatenate([np.asarray(x, dtype=np.int64) for x in rows] + [np.zeros(0, np.int64)])
    weights = None
    if w is not None:
        weights = np.concatenate([np.asarray(x, dtype=np.float32) for x in w]
                                 + [np.zeros(0, np.float32)]).astype(np.float32)
    return rowptr, cols.astype(np.int32), weights


# --------------------------------------------------------------------------- inputs
def table(m, d, seed):
    return np.random.default_rng(seed).standard_normal((m, d)).astype(np.float32)


FORCED_LENGTHS = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 200, 0, 2 * CHUNK)


def case_rows(m, seed, n=N_ROWS):
    """``n`` rows over ``m`` columns: the forced lengths (empty, one entry,
    around a chunk, several chunks) first, then random lengths in [1, 120];
    weights from U(0.5, 5). A row longer than m repeats columns."""
    rng = np.random.default_rng(seed)
    lengths = list(FORCED_LENGTHS) + rng.integers(1, 121, n - len(FORCED_LENGTHS)).tolist()
    rows = [rng.choice(m, L, replace=L > m).astype(np.int64) for L in lengths]
    w = [rng.uniform(0.5, 5.0, L).astype(np.float32) for L in lengths]
    return rows, w


def case(d, m, reg, weighted, seed=0):
    """(Y, rows, w or None, x64, E_ref) of one solver case."""
    Y = table(m, d, 1000 + seed + d + m)
    rows, w = case_rows(m, 2000 + seed + d + m)
    if not weighted:
        w = None
    x64 = solve(Y, rows, w, ALPHA, reg, np.float64)
    e_ref = rel_err(solve(Y, rows, w, ALPHA, reg, np.float32), x64, rows)
    return Y, rows, w, x64, e_ref


def interactions(n_users=200, n_items=300, n=3000, seed=5):
    """(pairs int64 [n, 2] with repeats, scores float32 [n]) of the trainer tests."""
    rng = np.random.default_rng(seed)
    pairs = np.stack([rng.integers(0, n_users, n), rng.integers(0, n_items, n)], 1)
    pairs[-200:] = pairs[:200]  # repeated pairs
    return pairs.astype(np.int64), rng.uniform(0.5, 5.0, n).astype(np.float32)


def pair_rows(pairs, scores, n_users):
    """Per-user (sorted unique items, summed scores) of ``interactions``."""
    rows, w = [], []
    for u in range(n_users):
        mine = pairs[:, 0] == u
        items, inv = np.unique(pairs[mine, 1], return_inverse=True)
        s = np.zeros(len(items))
        np.add.at(s, inv, scores[mine].astype(np.float64))
        rows.append(items.astype(np.int64))
        w.append(s.astype(np.float32))
    return rows, w


def als_f64(X, Y, rows, w, alpha, reg, iterations):
    """Float64 ALS from the tables (X, Y): the objective before and after every
    half-step."""
    t_rows, t_w = transpose(rows, w, Y.shape[0])
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    hist = [objective(X, Y, rows, w, alpha, reg)]
    for _ in range(iterations):
        X = _solve64(Y, rows, w, alpha, reg)
        hist.append(objective(X, Y, rows, w, alpha, reg))
        Y = _solve64(X, t_rows, t_w, alpha, reg)
        hist.append(objective(X, Y, rows, w, alpha, reg))
    return hist


def _solve64(Y, rows, w, alpha, reg):
    """``solve`` wholly in float64 (the Gram matrix unrounded)."""
    G, d = Y.T @ Y, Y.shape[1]
    out = np.zeros((len(rows), d))
    for r, idx in enumerate(rows):
        if len(idx):
            Yr = Y[idx]
            wr = np.ones(len(idx)) if w is None else np.asarray(w[r], dtype=np.float64)
            A = G + alpha * ((Yr.T * wr) @ Yr) + reg * np.eye(d)
            out[r] = np.linalg.solve(A, ((1.0 + alpha * wr)[:, None] * Yr).sum(0))
    return out
