"""The d = 128 score scan's ring refill issued by waves 0-3 alone (DESIGN.md
§3.1, "The stage boundary"): in the bf16 d = 128 scans with 288-row stages
(k = 100: CAP 512, seeded and from -inf) four waves issue the whole stage, 18
DMA instructions each, one instruction of one wave moving rows
16 j + 4 wave + lane / 16 of the stage; waves 4-7 issue nothing and wait for
no VMEM at the boundary. (The staged k = 1000 instance keeps eight issuers
and the cases of tests/test_scan_refill.py.) The shapes here pin what that
row-to-issuer mapping
can get wrong and tests/test_scan_refill.py does not: a slice end inside each
16-row half of a tile (the clamp of rows past the end cuts inside one wave's
4-row piece, or exactly between two instruction rounds), catalogs of one stage
and less (the prologue's refill alone), several units on one workgroup (the
counters of the waves that issue nothing and the ring restart carry over),
split tails, a seeded scan whose every user is rescanned, and one d = 64 and
one fp32 d = 128 case for the instances that keep eight issuers.

Rule and tolerance are those of tests/topk_checks.py: integer-valued tables,
lists and scores IDENTICAL (tolerance 0) to exact_topk.
"""
import functools

import numpy as np
import pytest
import torch

from divrec import _backend, ops
from topk_checks import assert_same_topk, exact_topk, int_table

pytestmark = pytest.mark.gpu

DEV = "cuda"
NU_MAX = 2100  # three workgroups' users at d = 128 (1024 per workgroup)
STAGE = 288    # rows per stage of the CAP-512 d = 128 instance


def _bf16(x):
    return torch.from_numpy(x).to(DEV).to(torch.bfloat16)


def _f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


@functools.lru_cache(maxsize=None)
def _tables(d):
    rng = np.random.default_rng(1290 + d)
    return int_table(rng, NU_MAX, d), int_table(rng, 2400, d)


@functools.lru_cache(maxsize=None)
def _small_ref(d, k, ni):
    """Exact lists of all NU_MAX users over the first ni rows (shared by the
    user counts: a user's list does not depend on the other users)."""
    U, I = _tables(d)
    return exact_topk(U, I[:ni], k)


@pytest.mark.parametrize("extra", [15, 16, 17, 31])
def test_slice_end_inside_a_tile_half_exact(extra):
    """Eight whole stages, then a last stage of 15 / 16 / 17 / 31 rows: the
    last row sits in wave 3's piece of round 0, is the first row of round 1,
    its second, or wave 3's last row of round 1."""
    ni, k, nu = 8 * STAGE + extra, 100, 1100
    plan = ops.score_topk_plan(nu, ni, torch.bfloat16, 128, k)
    assert plan["cap"] == 512 and plan["tail_chunks"] == 1 and plan["sample_stride"] == 0
    U, I = _tables(128)
    s, it = ops.score_topk(_bf16(U[:nu]), _bf16(I[:ni]), k)
    ref_i, ref_s = _small_ref(128, k, ni)
    assert_same_topk(s, it, (ref_i[:nu], ref_s[:nu]))


@pytest.mark.parametrize("nu", [33, 1100])
@pytest.mark.parametrize("ni", [1, 15, 16, 17, 287, 288, 289])
def test_one_stage_and_shorter_exact(ni, nu):
    """The keep-every-key plan: one stage or less is the prologue's refill
    alone (289 rows: one boundary refill of a single row)."""
    k = 10
    plan = ops.score_topk_plan(nu, ni, torch.bfloat16, 128, k)
    assert plan["cap"] >= ni and plan["head_keys"] >= max(ni, k)
    U, I = _tables(128)
    exclude = None
    if ni < k:  # a list longer than the catalog is only taken with an exclusion CSR: an empty one
        exclude = (torch.zeros(nu + 1, dtype=torch.int64, device=DEV),
                   torch.zeros(0, dtype=torch.int32, device=DEV))
    s, it = ops.score_topk(_bf16(U[:nu]), _bf16(I[:ni]), k, exclude=exclude)
    ref_i, ref_s = _small_ref(128, k, ni)
    assert_same_topk(s, it, (ref_i[:nu], ref_s[:nu]))


@pytest.mark.parametrize("slots", [1, 2])
def test_consecutive_units_on_one_workgroup_exact(slots):
    """Three user blocks on one or two workgroups: a workgroup runs unit after
    unit, each restarting the ring after the unit end's __syncthreads with the
    counters of all eight waves reset."""
    ni, k = 8 * STAGE + 64 + 5, 100
    U, I = _tables(128)
    with _backend.plan_knobs(scan_slots=slots):
        plan = ops.score_topk_plan(NU_MAX, ni, torch.bfloat16, 128, k)
        assert plan["cap"] == 512
        s, it = ops.score_topk(_bf16(U), _bf16(I[:ni]), k)
    ref_i, ref_s = _small_ref(128, k, ni)
    assert_same_topk(s, it, (ref_i, ref_s))


@pytest.mark.parametrize("extra", [15, 17])
def test_split_tail_exact(extra):
    """Four workgroup slots, two user blocks: each block's catalog is split in
    two chunk units; the second starts mid-catalog and ends in a stage of
    15 / 17 rows."""
    ni, k, nu = 29 * STAGE + 28 * STAGE + extra, 100, 1100
    rng = np.random.default_rng(4400 + extra)
    U, I = int_table(rng, nu, 128), int_table(rng, ni, 128)
    with _backend.plan_knobs(scan_slots=4):
        plan = ops.score_topk_plan(nu, ni, torch.bfloat16, 128, k)
        assert plan["tail_chunks"] == 2 and plan["head_blocks"] == 0
        assert plan["chunk_items"] % STAGE == 0 and (ni - plan["chunk_items"]) % STAGE == extra
        s, it = ops.score_topk(_bf16(U), _bf16(I), k)
    assert_same_topk(s, it, exact_topk(U, I, k))


@pytest.mark.parametrize("extra,slots", [(15, None), (17, 3)])
def test_seeded_scan_forced_rescan_exact(extra, slots):
    """Hot sampled rows put every user's guessed threshold where fewer than k
    items pass: the seeded scan runs, every user fails and is rescanned from
    -inf, in whole-catalog units and (three slots for two user blocks) in
    device-planned chunks. The catalog ends 15 / 17 rows into a stage."""
    rng = np.random.default_rng(4500 + extra)
    ni, k, nu = 911 * STAGE + extra, 100, 1100
    U = int_table(rng, nu, 128, 0, 3)
    I = int_table(rng, ni, 128)
    plan = ops.score_topk_plan(nu, ni, torch.bfloat16, 128, k)
    assert plan["sample_stride"] == 32 and plan["sample_rank"] < 30
    I[np.arange(30) * 32] = 3.0  # 30 hot sample rows >= the sample rank, < k
    stats = {}
    with _backend.plan_knobs(**({"scan_slots": slots} if slots else {})):
        s, it = ops.score_topk(_bf16(U), _bf16(I), k, stats=stats)
    assert stats["guess_failures"] == [nu, nu]  # both tiers failed: rescanned from -inf
    assert_same_topk(s, it, exact_topk(U, I, k))


@pytest.mark.parametrize("d,dtype,ni", [(64, "bf16", 5 * 448 + 15), (128, "f32", 33 * 64 + 17)])
def test_eight_issuer_instances_exact(d, dtype, ni):
    """bf16 d = 64 (two 56-KB slots, 448-row stages) and fp32 d = 128 (three
    32-KB slots, 64-row stages) keep eight issuers and the general addressing;
    the boundary code is shared, so one case each (three workgroups at fp32)."""
    k, nu = 100, 1100
    U, I = _tables(d)
    t = _f32 if dtype == "f32" else _bf16
    s, it = ops.score_topk(t(U[:nu]), t(I[:ni]), k)
    ref_i, ref_s = _small_ref(d, k, ni)
    assert_same_topk(s, it, (ref_i[:nu], ref_s[:nu]))
