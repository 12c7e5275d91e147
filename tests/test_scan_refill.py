"""The d = 128 score scan's ring refill ("The stage
boundary"): the bf16 d = 128 scans compute a lane's DMA source chunk once per
stage. The shapes here sit on the edges of the refill and of the boundary's
exact VMEM count: catalogs of a whole number of stages, one row / one tile /
two tiles + 5 rows more, one row less than a whole number (a short last stage,
a partial last tile whose rows are clamped to the slice end), user counts on
both sides of a workgroup (1024 users at d = 128), both d = 128 instances
(k = 100: CAP 512, 288-row stages; k = 1000: the staged CAP-2048 instance,
224-row stages), split tails whose chunk units start mid-catalog and end in a
short stage, scans from -inf whose every stage floods the buffers (survivor
stores and compactions between the refills), and seeded scans with a forced
rescan.

Rule and tolerance are those of tests/topk_checks.py: integer-valued tables,
lists and scores IDENTICAL (tolerance 0) to exact_topk.

Catalogs stay above 2048 rows (at or below, the keep-every-key plan runs and
nothing is compacted), so the 224-row cases use 10 stages where the 288-row
cases use 8.
"""
import functools

import numpy as np
import pytest
import torch

from divrec import _backend, ops
from topk_checks import assert_same_topk, exact_topk, int_table

pytestmark = pytest.mark.gpu

DEV = "cuda"
NU_MAX = 1100
STAGE = {100: 288, 1000: 224}   # rows per stage of the d = 128 instance that k selects
STAGES = {100: 8, 1000: 10}     # whole stages of the small catalogs (above 2048 rows)


def _catalogs(k):
    s, n = STAGE[k], STAGES[k]
    return [n * s, n * s + 1, n * s + 32, n * s + 64 + 5, (n + 1) * s - 1]


assert _catalogs(100) == [2304, 2305, 2336, 2373, 2591]


def _bf16(x):
    return torch.from_numpy(x).to(DEV).to(torch.bfloat16)


def _check(U, I, k, **knobs):
    with _backend.plan_knobs(**knobs):
        s, it = ops.score_topk(_bf16(U), _bf16(I), k)
    assert_same_topk(s, it, exact_topk(U, I, k))


@functools.lru_cache(maxsize=None)
def _tables(d, ascending=False):
    """One user and one item table per width, sliced by the cases. ascending:
    users non-negative and item rows in ascending order of their row sum, so
    scores trend upwards along the catalog and EVERY stage of a scan from -inf
    floods the buffers (survivor stores after every refill, compactions at
    the stage ends)."""
    rng = np.random.default_rng(1280 + d + (7 if ascending else 0))
    U = int_table(rng, NU_MAX, d, 0 if ascending else -3, 3)
    I = int_table(rng, 2600, d)
    if ascending:
        I = I[np.argsort(I.sum(axis=1), kind="stable")]
    return U, I


@functools.lru_cache(maxsize=None)
def _small_ref(d, k, ni, ascending=False):
    """Exact lists of all NU_MAX users over the first ni rows (shared by the
    user counts: a user's list does not depend on the other users)."""
    U, I = _tables(d, ascending)
    return exact_topk(U, I[:ni], k)


@pytest.mark.parametrize("nu", [1, 33, 1024, 1100])
@pytest.mark.parametrize("stage_case", range(5))
@pytest.mark.parametrize("k", [100, 1000])
def test_stage_counts_exact(k, stage_case, nu):
    """Whole-catalog units (scans from -inf) over 8 (10) stages, + 1 row,
    + 1 tile, + 2 tiles + 5 rows, and one row short of a stage more."""
    ni = _catalogs(k)[stage_case]
    plan = ops.score_topk_plan(nu, ni, torch.bfloat16, 128, k)
    assert plan["cap"] == (512 if k == 100 else 2048) and plan["tail_chunks"] == 1
    assert plan["sample_stride"] == 0  # below 2^18 rows: no guess, a scan from -inf
    U, I = _tables(128)
    s, it = ops.score_topk(_bf16(U[:nu]), _bf16(I[:ni]), k)
    ref_i, ref_s = _small_ref(128, k, ni)
    assert_same_topk(s, it, (ref_i[:nu], ref_s[:nu]))


@pytest.mark.parametrize("k", [100, 1000])
def test_flooding_stages_exact(k):
    """Scores ascend along the catalog: from -inf the stages keep admitting
    rows, so survivor stores follow every refill and stages end in
    compactions (the exact VMEM count carries both). That the data does so is
    checked on the exact scores with lower bounds: a threshold only changes at
    a stage end and never exceeds the k-th best score so far, so every row
    beating the k-th best of the EARLIER stages is stored; a compaction keeps
    at least k keys; a buffer above the plan's flush bound at a stage end is
    compacted."""
    ni = _catalogs(k)[3]
    U, I = _tables(128, True)
    S = U.astype(np.float64) @ I[:ni].astype(np.float64).T
    stage = STAGE[k]
    flush = k + 32 + 96 if k == 100 else 2048 - stage  # flush_at of the two plans
    cnt = np.zeros(NU_MAX, dtype=np.int64)   # lower bound of each user's buffer fill
    sure = np.zeros(NU_MAX, dtype=np.int64)  # stage ends that certainly compact
    for s0 in range(0, ni, stage):
        kth = np.sort(S[:, :s0], axis=1)[:, -k] if s0 >= k else np.full(NU_MAX, -np.inf)
        cnt += (S[:, s0:s0 + stage] > kth[:, None]).sum(axis=1)
        full = cnt > flush
        sure += full
        cnt[full] = k
    print("certain compactions per user: min", sure.min(), "median", np.median(sure))
    assert sure.min() >= 1 and np.median(sure) >= (3 if k == 100 else 1)
    s, it = ops.score_topk(_bf16(U), _bf16(I[:ni]), k)
    ref_i, ref_s = _small_ref(128, k, ni, True)
    assert_same_topk(s, it, (ref_i, ref_s))


@pytest.mark.parametrize("k,ni", [(100, 29 * 288 + 28 * 288 + 37), (1000, 37 * 224 + 36 * 224 + 37)])
def test_split_tail_short_last_stage_exact(k, ni):
    """Four workgroup slots, two user blocks: each block's catalog is split in
    two chunk units. The second starts mid-catalog (row 8352 / 8288) and ends
    with a stage of one tile + 5 rows."""
    rng = np.random.default_rng(4100 + k)
    U, I = int_table(rng, NU_MAX, 128), int_table(rng, ni, 128)
    with _backend.plan_knobs(scan_slots=4):
        plan = ops.score_topk_plan(NU_MAX, ni, torch.bfloat16, 128, k)
    assert plan["tail_chunks"] == 2 and plan["head_blocks"] == 0
    assert plan["chunk_items"] % STAGE[k] == 0 and (ni - plan["chunk_items"]) % STAGE[k] == 37
    _check(U, I, k, scan_slots=4)


@pytest.mark.parametrize("k,ni", [(100, 911 * 288 + 37), (1000, 1171 * 224 + 37)])
def test_seeded_scan_exact(k, ni):
    """Catalogs of 2^18 rows and more start from guessed thresholds (the
    seeded instantiation); the last stage is one tile + 5 rows."""
    rng = np.random.default_rng(4200 + k)
    plan = ops.score_topk_plan(NU_MAX, ni, torch.bfloat16, 128, k)
    assert plan["sample_stride"] > 0
    _check(int_table(rng, NU_MAX, 128), int_table(rng, ni, 128), k)


@pytest.mark.parametrize("slots", [None, 3])
def test_forced_rescan_from_minus_inf_exact(slots):
    """Hot sampled rows (the best items of every non-negative user) put the
    guessed threshold at the hot score, which fewer than k items pass: every
    user fails the guess and is rescanned from -inf, in whole-catalog units
    and (three slots for two user blocks: a split tail) in device-planned
    chunks. The hot rows lead the catalog, so the rescan's first stages flood
    the buffers. The call's failure counts prove the rescan ran for every
    user."""
    rng = np.random.default_rng(4300)
    ni, k = 911 * 288 + 37, 100
    U = int_table(rng, NU_MAX, 128, 0, 3)
    I = int_table(rng, ni, 128)
    plan = ops.score_topk_plan(NU_MAX, ni, torch.bfloat16, 128, k)
    assert plan["sample_stride"] == 32 and plan["sample_rank"] < 30
    I[np.arange(30) * 32] = 3.0  # 30 hot sample rows >= the sample rank, < k
    stats = {}
    with _backend.plan_knobs(**({"scan_slots": slots} if slots else {})):
        s, it = ops.score_topk(_bf16(U), _bf16(I), k, stats=stats)
    print("guess failures", stats["guess_failures"])
    assert stats["guess_failures"] == [NU_MAX, NU_MAX]  # both tiers failed: rescanned from -inf
    assert_same_topk(s, it, exact_topk(U, I, k))


@pytest.mark.parametrize("d", [64, 256])
def test_other_widths_keep_their_boundary_exact(d):
    """d = 64 (two 56-KB slots, 448-row stages) and d = 256 (three 32-KB
    slots, 64-row stages) keep the general refill addressing; the boundary code is
    shared, so one case each: a last stage of two tiles + 5 rows (d = 64) or
    one tile + 5 rows (d = 256), more than one workgroup at d = 256."""
    ni = 5 * 448 + 64 + 5
    U, I = _tables(d)
    s, it = ops.score_topk(_bf16(U), _bf16(I[:ni]), 100)
    ref_i, ref_s = _small_ref(d, 100, ni)
    assert_same_topk(s, it, (ref_i, ref_s))
