"""The 16x16x32 bf16 MFMA form of the d = 128 direct-store score scans
("The other MFMA shape"): items on M, users on N; lane l holds
user 16 ut + l % 16, k = 32 s + 8 (l / 16) .. +7 of each user tile ut, reads
item row 16 half + l % 16, and ends a tile with 8 scores of one user, rows
16 half + 4 (l / 16) + j. The shapes here are the smallest at which that can go
wrong: every k index against its own user element (one-hot item rows), one
survivor at each of a tile's 32 rows with the user moving over all 8 user
tiles of a wave and to the last wave of a 1024-user block, up to four lanes of
one user in one block, several registers of one lane, a partial last tile cut
at every kind of place in the 4-row groups and the two halves, a NaN row, user
counts off the tile, CAP 1024, and one float-table case.

Every case runs unseeded (ops.score_topk) and through the caller-seeded entry
(init_thr), at d = 128 bf16. They hold for either MFMA shape.

Integer-valued tables in [-3, 3]: lists and scores must be IDENTICAL (tolerance
0) to tests/topk_checks.py's exact_topk. The float case uses the gap-aware rule and the
tolerance of tests/test_hip_kernels.py::test_score_topk_float_tolerance.
"""
import numpy as np
import pytest
import torch

from divrec import ops
from test_scan_survivors import D, DEV, PLANT, _both, _tables
from topk_checks import int_table

pytestmark = pytest.mark.gpu


def _planted(nu, user, rows, flips):
    """nu users x 64 items; item rows `rows` equal user `user`'s row of +-3
    but for flips[i] entries of opposite sign: scores PLANT - 18 * flips[i],
    far above every other score (|3 * a sum of 128 values in [-3, 3]|, a
    standard deviation of 68)."""
    rng = np.random.default_rng(1600 + 64 * user + rows[0])
    U, I = int_table(rng, nu, D), int_table(rng, 64, D)
    pat = rng.choice(np.array([-3.0, 3.0], dtype=np.float32), size=D)
    U[user] = pat
    for row, f in zip(rows, flips):
        I[row] = pat
        I[row, :f] = -pat[:f]
    sc = U.astype(np.float64) @ I.astype(np.float64).T
    sc[user, list(rows)] = -np.inf
    assert sc.max() < PLANT - 18 * max(flips) - 100
    return U, I


def test_k_mapping_one_hot_items_exact():
    """Item k is 3 e_k, so user u's score of it is 3 U[u, k]: a k index that
    met another user element, in any k-step or lane group, changes a list."""
    rng = np.random.default_rng(3216)
    U = int_table(rng, 64, D)
    I = 3.0 * np.eye(D, dtype=np.float32)
    _both(U, I, 32)


@pytest.mark.parametrize("p", range(32))
def test_one_survivor_at_every_row_exact(p):
    """One key of the whole seeded scan, at row p of the second tile; the
    user moves over all 8 user tiles of the wave."""
    user = (37 * p + 5) % 128
    U, I = _planted(128, user, [32 + p], [0])
    _both(U, I, 8, thr=np.full(128, PLANT - 1.0))


def test_survivor_at_the_far_end_of_a_block_exact():
    """The same in a whole 1024-user block, the user in its last wave."""
    U, I = _planted(1024, 1000, [32 + 21], [0])
    _both(U, I, 8, thr=np.full(1024, PLANT - 1.0))


@pytest.mark.parametrize("p", [0, 3, 17, 18])
def test_four_lanes_of_a_user_in_one_block_exact(p):
    """Rows p, p + 4, p + 8 and p + 12 are one score register in the user's
    four lanes: four keys of equal score take slots from one counter in one
    block."""
    U, I = _planted(128, (11 * p + 70) % 128, [32 + p, 36 + p, 40 + p, 44 + p], [0, 0, 0, 0])
    _both(U, I, 8, thr=np.full(128, PLANT - 1.0))


@pytest.mark.parametrize("rows,flips", [((2, 18), (0, 0)), ((13, 29), (1, 0)),
                                        ((4, 5, 21), (1, 0, 2)), ((10, 11, 27), (0, 0, 0))])
def test_several_registers_of_one_lane_exact(rows, flips):
    """Rows p and p + 16 are the two halves' registers of one lane; rows p,
    p + 1 and p + 17 three of its registers."""
    U, I = _planted(128, 16 * rows[0] % 128 + 9, [32 + r for r in rows], flips)
    _both(U, I, 8, thr=np.full(128, PLANT - 18.0 * max(flips) - 1.0))


@pytest.mark.parametrize("extra", [1, 3, 4, 5, 12, 15, 16, 17, 20, 31])
def test_partial_last_tile_exact(extra):
    """Rows past the catalog's end repeat its last row in the tile: never
    stored, wherever the end cuts the 4-row groups and the halves."""
    U, I = _tables()
    _both(U[:128], I[:32 + extra], 64)


def test_nan_item_row_never_stored_exact():
    """A NaN row fires the hot test of every user; the strict > admits none
    of its scores, and the other rows' lists are as without it."""
    U, I = _tables()
    I = I[:96].copy()
    I[40] = np.nan
    drop = np.zeros(96, dtype=bool)
    drop[40] = True
    _both(U[:128], I, 16, drop=drop)


@pytest.mark.parametrize("nu", [5, 1024 + 17])
def test_user_counts_off_the_tile_exact(nu):
    """Padded lanes (users past the count) never store into a real user's
    buffer: 5 users of one tile, and a second block of 17."""
    U, I = _tables()
    _both(U[:nu], I[:100], 16)


def test_cap_1024_exact():
    assert ops.score_topk_plan(300, 700, torch.bfloat16, D, 300)["cap"] == 1024
    U, I = _tables()
    _both(U[:300], I[:700], 300)


def test_float_tables_within_tolerance():
    """N(0, 1/sqrt(d)) bf16 tables, 2048 users x 50 000 items, k = 100, against
    float64 with the gap-aware rule: every score within tol of its float64
    value, lists sorted, every returned item at or above the exact k-th score
    - 2 tol, every item above the k-th + 2 tol returned."""
    nu, ni, k = 2048, 50_000, 100
    g = torch.Generator(device=DEV).manual_seed(1632)
    U = (torch.randn(nu, D, generator=g, device=DEV) / D ** 0.5).to(torch.bfloat16)
    I = (torch.randn(ni, D, generator=g, device=DEV) / D ** 0.5).to(torch.bfloat16)
    tol = 1e-5 * np.sqrt(D / 64)
    outs = [ops.score_topk(U, I, k),
            ops.score_topk(U, I, k, init_thr=torch.full((nu,), -float("inf"), device=DEV))]
    I64 = I.double()
    for b in range(0, nu, 256):
        S = U[b:b + 256].double() @ I64.T  # the reference, once for both entries
        kth = torch.topk(S, k, dim=1).values[:, k - 1:k]
        must = S > kth + 2 * tol
        for s, it in outs:
            sb, ib = s[b:b + 256].double(), it[b:b + 256].long()
            assert bool((ib >= 0).all())
            true = torch.gather(S, 1, ib)
            assert bool(((sb - true).abs() <= tol).all())
            assert bool((sb[:, 1:] <= sb[:, :-1]).all())
            assert bool((true >= kth - 2 * tol).all())
            hit = torch.zeros_like(must).scatter_(1, ib, True)
            assert not bool((must & ~hit).any())
