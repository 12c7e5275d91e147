"""The direct-store survivor path of the score scan (DESIGN.md §3.1,
"Survivors per score register"): the scans that append survivors straight to
their users' candidate buffers (bf16 d >= 128 at CAP 512 / 1024, fp32 d >= 64)
store them in one block per score register r = 0..15: the ballot of
`score[r] > threshold` picks the lanes, each takes a slot from its user's
counter and stores the key of the block's compile-time row. The shapes here are
the smallest at which that can go wrong: every register and both half-waves
(one survivor at each of a tile's 32 rows, all 32 at once), both half-lanes of
one user in one block, several survivors in one lane, a partial last tile cut
inside and between the halves' 4-row groups, a NaN row (the hot test fires,
nothing is stored), counters across stages, compactions, units and chunk
units, and one case for each other instantiation of the path (and bf16
d = 64, the staged path).

Every shape runs unseeded (ops.score_topk) and through the caller-seeded
entry (init_thr): both kernel instantiations.

Rule and tolerance are those of tests/topk_checks.py: integer-valued tables,
lists and scores IDENTICAL (tolerance 0) to exact_topk.
"""
import functools

import numpy as np
import pytest
import torch

from divrec import ops
from topk_checks import assert_same_topk, exact_topk, int_table

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 128
PLANT = 9 * D  # score of a planted (user, item) pair: every product is 3 * 3


def _dev(x, dtype=torch.bfloat16):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).to(dtype)


def _empty_csr(nu):
    return (torch.zeros(nu + 1, dtype=torch.int64, device=DEV),
            torch.zeros(0, dtype=torch.int32, device=DEV))


def _both(U, I, k, thr=None, drop=None, exclude=None, dtype=torch.bfloat16):
    """The unseeded scan against the exact top-k, then the caller-seeded scan
    (thresholds thr, -inf where None) against the exact top-k above thr."""
    nu, ni = U.shape[0], I.shape[0]
    Ut, It = _dev(U, dtype), _dev(I, dtype)
    ex = exclude if exclude is not None or k <= ni else _empty_csr(nu)
    s, it = ops.score_topk(Ut, It, k, exclude=ex)
    assert_same_topk(s, it, exact_topk(U, I, k, drop=drop))
    t = np.full(nu, -np.inf, dtype=np.float32) if thr is None else np.asarray(thr, np.float32)
    s, it = ops.score_topk(Ut, It, k, exclude=exclude, init_thr=torch.from_numpy(t).to(DEV))
    assert_same_topk(s, it, exact_topk(U, I, k, thr=t, drop=drop))


@functools.lru_cache(maxsize=None)
def _tables(d=D):
    rng = np.random.default_rng(5150 + d)
    return int_table(rng, 2100, d), int_table(rng, 2405, d)


def _planted(user, rows, flips):
    """32 users x 64 items; item rows `rows` equal user `user`'s row of +-3
    but for flips[i] entries of opposite sign: scores PLANT - 18 * flips[i],
    far above every other score (|3 * a sum of 128 values in [-3, 3]|, a
    standard deviation of 68)."""
    rng = np.random.default_rng(77 + 64 * user + rows[0])
    U, I = int_table(rng, 32, D), int_table(rng, 64, D)
    pat = rng.choice(np.array([-3.0, 3.0], dtype=np.float32), size=D)
    U[user] = pat
    for row, f in zip(rows, flips):
        I[row] = pat
        I[row, :f] = -pat[:f]
    sc = U.astype(np.float64) @ I.astype(np.float64).T
    sc[user, list(rows)] = -np.inf
    assert sc.max() < PLANT - 18 * max(flips) - 100
    return U, I


@pytest.mark.parametrize("k", [32, 8])
def test_every_register_both_halves_exact(k):
    """One tile from -inf: all 16 blocks store for every lane."""
    U, I = _tables()
    _both(U[:64], I[:32], k)


@pytest.mark.parametrize("p", range(32))
def test_one_survivor_at_every_row_exact(p):
    """One key of the whole seeded scan, at row p of the second tile: one
    block stores one lane's key, the 15 blocks around it nothing."""
    user = (7 * p + 3) % 32
    U, I = _planted(user, [32 + p], [0])
    _both(U, I, 8, thr=np.full(32, PLANT - 1.0))


@pytest.mark.parametrize("p", [0, 3, 24])
def test_both_half_lanes_of_a_user_in_one_block_exact(p):
    """Rows p and p + 4 are the same score register in the user's two
    half-wave lanes: both keys (equal scores) in one block."""
    U, I = _planted(5 + p, [32 + p, 32 + p + 4], [0, 0])
    _both(U, I, 8, thr=np.full(32, PLANT - 1.0))


def test_three_survivors_in_one_lane_exact():
    """Rows 0, 1 and 8 of the tile are registers 0, 1 and 4 of one lane."""
    U, I = _planted(17, [32, 33, 40], [1, 0, 2])
    _both(U, I, 8, thr=np.full(32, PLANT - 18.0 * 2 - 1.0))


@pytest.mark.parametrize("extra", [1, 4, 5, 8, 13, 31])
def test_partial_last_tile_exact(extra):
    """Rows past the catalog's end repeat its last row in the tile: never
    stored."""
    U, I = _tables()
    _both(U[:64], I[:32 + extra], 64)


def test_nan_item_row_never_stored_exact():
    """A NaN row fires the hot test of every user; the strict > admits none
    of its scores, and the other rows' lists are as without it."""
    U, I = _tables()
    I = I[:96].copy()
    I[40] = np.nan
    drop = np.zeros(96, dtype=bool)
    drop[40] = True
    _both(U[:64], I, 16, drop=drop)


@pytest.mark.parametrize("excl", [False, True])
def test_counters_across_stages_compactions_and_units_exact(excl):
    """Three workgroups (the last one partial), nine stages and a partial last
    tile, every user's buffer compacted several times from -inf."""
    U, I = _tables()
    nu, ni, k = U.shape[0], I.shape[0], 100
    drop = exclude = None
    if excl:
        rng = np.random.default_rng(99)
        cols = np.sort(np.stack([rng.choice(ni, size=5, replace=False) for _ in range(nu)]), axis=1)
        drop = np.zeros((nu, ni), dtype=bool)
        np.put_along_axis(drop, cols, True, axis=1)
        exclude = (torch.arange(0, 5 * nu + 1, 5, dtype=torch.int64, device=DEV),
                   torch.from_numpy(cols.reshape(-1).astype(np.int32)).to(DEV))
    _both(U, I, k, drop=drop, exclude=exclude)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_exclusion_rows_of_length_0_1_5_exact(dtype):
    """3 users x 8 items, k = 4, exclusion rows that are empty, of one and of
    five (three items left: a padded list). A catalog this small is never
    compacted, so the rows are searched by the finalize's drop_excluded alone,
    not by dr::sorted_contains: the next test reaches that one."""
    rng = np.random.default_rng(808)
    U, I = int_table(rng, 3, D), int_table(rng, 8, D)
    rows = [[], [3], [1, 2, 4, 6, 7]]
    drop = np.zeros((3, 8), dtype=bool)
    for u, r in enumerate(rows):
        drop[u, r] = True
    exclude = (torch.tensor([0, 0, 1, 6], dtype=torch.int64, device=DEV),
               torch.tensor(sum(rows, []), dtype=torch.int32, device=DEV))
    _both(U, I, 4, drop=drop, exclude=exclude, dtype=dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_exclusion_rows_of_length_0_1_5_in_a_compaction_exact(dtype):
    """The compaction's search of the exclusion rows (dr::sorted_contains): 3
    users x 2100 items, k = 4, rows that are empty, of one and of five.

    That a compaction runs with the planted rows in the buffer follows from the
    plan: above 2048 items no plan keeps every key; a threshold stays -inf
    until its buffer's first compaction, which comes at the end of the first
    stage that leaves more than k + 32 + 96 = 132 keys, so until then every row
    is stored, rows 0..63 (the shortest stage) among them. That compaction
    looks every stored id up in the user's row: its first entry, its last
    entry, the ids between, below and above them.

    What a wrong answer does: the planted rows score 1024 and more, every other
    row below 512. User 2's row excludes its five planted rows; user 1's
    excludes the best of its four. An entry the search misses leaves k planted
    keys in the buffer, the new threshold rises above every other score, and
    the list ends short (the finalize drops the excluded keys by a search of
    its own). An id found that is not in the row loses a stored key."""
    ni, k = 2100, 4
    rng = np.random.default_rng(909)
    U, I = int_table(rng, 3, D), int_table(rng, ni, D)
    rows = [[], [30], [1, 9, 22, 40, 63]]
    planted = {1: ([30, 3, 31, 50], [0, 1, 2, 3]), 2: (rows[2], [0, 0, 1, 1, 2])}
    for u, (rws, flips) in planted.items():
        U[u] = rng.choice(np.array([-3.0, 3.0], dtype=np.float32), size=D)
        for row, f in zip(rws, flips):
            I[row] = U[u]
            I[row, :f] = -U[u, :f]
    sc = U.astype(np.float64) @ I.astype(np.float64).T
    for u, (rws, flips) in planted.items():
        assert np.array_equal(sc[u, rws], PLANT - 18.0 * np.asarray(flips))
        assert sc[u, rws].min() >= 1024
        sc[u, rws] = -np.inf
    assert sc.max() < 512
    plan = ops.score_topk_plan(3, ni, dtype, D, k)
    assert plan["tail_chunks"] == 1 and plan["sample_stride"] == 0 and plan["head_keys"] < ni
    drop = np.zeros((3, ni), dtype=bool)
    for u, r in enumerate(rows):
        drop[u, r] = True
    exclude = (torch.tensor([0, 0, 1, 6], dtype=torch.int64, device=DEV),
               torch.tensor(sum(rows, []), dtype=torch.int32, device=DEV))
    _both(U, I, k, drop=drop, exclude=exclude, dtype=dtype)


def test_split_units_exact():
    """One user block on a many-CU grid: the catalog is split into chunk
    units, each compacted to end_keep keys at its end."""
    nu, ni, k = 200, 16384 + 37, 100
    rng = np.random.default_rng(616)
    U, I = int_table(rng, nu, D), int_table(rng, ni, D)
    assert ops.score_topk_plan(nu, ni, torch.bfloat16, D, k)["tail_chunks"] > 1
    _both(U, I, k)


@pytest.mark.parametrize("d,dtype,k", [(256, torch.bfloat16, 100), (512, torch.bfloat16, 100),
                                       (128, torch.float32, 100), (128, torch.bfloat16, 300),
                                       (64, torch.bfloat16, 100)])
def test_other_instantiations_exact(d, dtype, k):
    """bf16 d = 256 and 512, fp32 d = 128, bf16 d = 128 at CAP 1024, and the
    staged bf16 d = 64 scan, which the per-register blocks do not touch."""
    if d == D and dtype == torch.bfloat16:
        assert ops.score_topk_plan(300, 700, dtype, d, k)["cap"] == 1024
    U, I = _tables(d)
    _both(U[:300], I[:700], k, dtype=dtype)
