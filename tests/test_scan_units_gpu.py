"""The seeded main scan's unit queue and graded tail chunks on the GPU.

The workgroups of dr_score_topk's seeded main scan claim their units from a
device word (TopkArgs::unit_queue), and the chunks of a split tail block are
graded, longest first (tail_chunk_bounds). Lists must not depend on either:
every case compares with the exact top-k (tests/topk_checks.py; integer tables,
so scores are exact and ties go by item id) and with the same call under
another plan. Catalogs are 2^18 + 293 rows, the shortest the planner seeds
and splits (not a multiple of a stage or a tile); the floor knob is one stage,
so chunks really are graded at that length.
"""
import ctypes

import numpy as np
import pytest
import torch

from divrec import _backend, ops
from topk_checks import assert_same_topk, exact_topk, int_table

pytestmark = pytest.mark.gpu

NI = (1 << 18) + 293
STAGE = {128: 288, 64: 448}  # rows per stage by row bytes / 2 (CAP 512)


def _dev(x, dtype=torch.bfloat16):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda").to(dtype)


@pytest.fixture(scope="module")
def base():
    """d = 128 tables, 6 * 1024 + 37 users, and the exact top-114 of every
    user (its first 100 columns are the exact top-100)."""
    rng = np.random.default_rng(20261)
    U, I = int_table(rng, 6 * 1024 + 37, 128), int_table(rng, NI, 128)
    return {"U": U, "I": I, "Ud": _dev(U), "Id": _dev(I), "ref": exact_topk(U, I, 114)}


def _ref(base, k, n=None):
    items, scores = base["ref"]
    return items[:n, :k], scores[:n, :k]


def _call(Ud, Id, k, n_users=None, user_ids=None, excl=None, ws=None, counts=False):
    """dr_score_topk on the caller's workspace (None: a fresh one). Returns
    (scores, items, workspace[, fail counts])."""
    L = _backend.lib()
    dt = _backend.dtype_code(Ud.dtype)
    w = ops.score_width(Ud.dtype, Ud.size(1))
    n = user_ids.numel() if user_ids is not None else (Ud.size(0) if n_users is None else n_users)
    need = L.dr_score_topk_workspace(n, Id.size(0), dt, w, k)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert ws.numel() >= need
    s = torch.empty(n, k, device="cuda")
    it = torch.empty(n, k, dtype=torch.int32, device="cuda")
    rowptr, cols = excl if excl is not None else (None, None)
    rc = L.dr_score_topk(Ud.data_ptr(), _backend.ptr(user_ids), n, Id.data_ptr(), Id.size(0), 0, dt,
                         w, k, _backend.ptr(rowptr), _backend.ptr(cols), s.data_ptr(),
                         it.data_ptr(), ws.data_ptr(), ws.numel(),
                         _backend.stream(torch.device("cuda", torch.cuda.current_device())))
    _backend.check(rc, "dr_score_topk")
    torch.cuda.synchronize()
    if not counts:
        return s, it, ws
    fc = (ctypes.c_int32 * 2)()
    _backend.check(L.dr_score_topk_fail_counts(ws.data_ptr(), n, Id.size(0), dt, w, k,
                                               ctypes.addressof(fc)), "dr_score_topk_fail_counts")
    return s, it, ws, [int(fc[0]), int(fc[1])]


def _chunks(n, dtype, d, k):
    """(c, boundaries) of the plan in force (dr_score_topk_tail_chunks)."""
    out, nc = (ctypes.c_int64 * 17)(), ctypes.c_int(0)
    w = ops.score_width(dtype, d)
    _backend.check(_backend.lib().dr_score_topk_tail_chunks(n, NI, _backend.dtype_code(dtype), w, k,
                                                            out, 17, ctypes.byref(nc)),
                   "dr_score_topk_tail_chunks")
    return nc.value, [int(x) for x in out[:nc.value + 1]]


def _graded(c, b, stage):
    """The chunks are not the equal ones."""
    per = -(-(-(-NI // c)) // stage) * stage
    return b != [min(j * per, NI) for j in range(c + 1)]


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_tail_blocks_graded_queue_twice_on_one_workspace(base):
    """4 slots, 7 user blocks: 4 head blocks, 3 tail blocks of 4 graded chunks
    (the last block partial), 16 units for 4 workgroups. The lists equal the
    exact top-k and those of the plan without a tail split and of the static
    loop; a second call on the same workspace (the queue word zeroed again,
    another claim order) gives the same bytes."""
    k, n = 100, base["U"].shape[0]
    with _backend.plan_knobs(scan_slots=4, scan_floor=STAGE[128]):
        plan = ops.score_topk_plan(n, NI, torch.bfloat16, 128, k)
        c, b = _chunks(n, torch.bfloat16, 128, k)
        assert plan["head_blocks"] == 4 and plan["user_blocks"] == 7 and plan["grid"] == 4
        assert plan["tail_chunks"] == c == 4 and plan["sample_stride"] > 0
        assert _graded(c, b, STAGE[128]) and b[1] - b[0] > b[2] - b[1] > b[3] - b[2]
        s1, i1, ws = _call(base["Ud"], base["Id"], k)
        first = (s1.clone(), i1.clone())
        s2, i2, _ = _call(base["Ud"], base["Id"], k, ws=ws)
        with _backend.plan_knobs(scan_split=1):
            assert ops.score_topk_plan(n, NI, torch.bfloat16, 128, k)["tail_chunks"] == 1
            whole = _call(base["Ud"], base["Id"], k)[:2]
        with _backend.plan_knobs(scan_queue=0):
            assert not _graded(*_chunks(n, torch.bfloat16, 128, k), STAGE[128])
            static = _call(base["Ud"], base["Id"], k)[:2]
    assert_same_topk(s1, i1, _ref(base, k))
    assert _same(first, (s2, i2)) and _same(first, whole) and _same(first, static)


@pytest.mark.parametrize("slots", [1, 64])
def test_one_workgroup_and_a_grid_of_all_units(base, slots):
    """scan_slots = 1: one workgroup claims all 7 units in order. 64 slots: the
    7 blocks are all tail blocks of 9 chunks, 63 units on a grid of 63 (the
    planner never launches more workgroups than units), so a workgroup that
    starts late may find the queue empty and leaves by the same test that ends
    every workgroup's loop."""
    k, n = 100, base["U"].shape[0]
    with _backend.plan_knobs(scan_slots=slots, scan_floor=STAGE[128]):
        plan = ops.score_topk_plan(n, NI, torch.bfloat16, 128, k)
        units = plan["head_blocks"] + (plan["user_blocks"] - plan["head_blocks"]) * plan["tail_chunks"]
        assert plan["sample_stride"] > 0
        assert (units, plan["grid"]) == ((7, 1) if slots == 1 else (63, 63))
        s, it, _ = _call(base["Ud"], base["Id"], k)
    assert_same_topk(s, it, _ref(base, k))


def test_duplicate_ids_and_exclusions_in_tail_blocks(base):
    """User ids permuted and repeated, and an exclusion CSR (random items, and
    the best items of some users) over head and tail blocks alike."""
    rng = np.random.default_rng(20262)
    k, nu = 100, base["U"].shape[0]
    users = np.concatenate([rng.permutation(nu)[:nu - 60], rng.integers(0, nu, 60)]).astype(np.int64)
    frozen = [rng.choice(NI, size=int(rng.integers(0, 30)), replace=False) for _ in users]
    ref_i = base["ref"][0]
    for p in range(4096, len(users), 53):  # positions of the tail blocks
        frozen[p] = np.union1d(frozen[p], ref_i[users[p], :12])
    rowptr = np.concatenate([[0], np.cumsum([len(f) for f in frozen])]).astype(np.int64)
    cols = np.concatenate([np.sort(f) for f in frozen]).astype(np.int32)
    excl = (torch.from_numpy(rowptr).cuda(), torch.from_numpy(cols).cuda())
    with _backend.plan_knobs(scan_slots=4, scan_floor=STAGE[128]):
        assert _graded(*_chunks(len(users), torch.bfloat16, 128, k), STAGE[128])
        s, it, _ = _call(base["Ud"], base["Id"], k, user_ids=torch.from_numpy(users).cuda(), excl=excl)
    assert_same_topk(s, it, exact_topk(base["U"][users], base["I"], k, frozen=frozen))


def test_rescans_follow_the_queued_scan_on_one_workspace():
    """Hot sampled rows: the best items of every non-negative user sit at the
    first sample positions, more of them than the guess's safe rank and fewer
    than k, so both guessed thresholds admit only those items and the users
    fail both tiers. The static second-tier and fallback rescans then run
    after the queued main scan on the same workspace; the fail counts (words 0
    to 2 of the block whose word 3 is the queue) are those of the call without
    a queue, and the lists are exact."""
    rng = np.random.default_rng(20263)
    k, nu = 100, 4 * 1024 + 37
    U = np.concatenate([int_table(rng, nu - 1500, 128, 0, 3), int_table(rng, 1500, 128, -3, 0)])
    U = U[rng.permutation(nu)]
    I = int_table(rng, NI, 128)
    with _backend.plan_knobs(scan_slots=4, scan_floor=STAGE[128]):
        plan = ops.score_topk_plan(nu, NI, torch.bfloat16, 128, k)
        assert plan["tail_chunks"] > 1 and plan["head_blocks"] == 4
        assert 1 <= plan["first_tier_rank"] < plan["sample_rank"] < k - 8  # two tiers
        n_hot = plan["sample_rank"] + 4
        I[np.arange(n_hot) * plan["sample_stride"]] = 3.0
        Ud, Id = _dev(U), _dev(I)
        assert _graded(*_chunks(nu, torch.bfloat16, 128, k), STAGE[128])
        s, it, _, fc = _call(Ud, Id, k, counts=True)
        with _backend.plan_knobs(scan_queue=0):
            s0, i0, _, fc0 = _call(Ud, Id, k, counts=True)
    failing = int(((U >= 0).all(1) & (U > 0).any(1)).sum())
    assert fc == fc0 and fc[0] >= failing > 0 and fc[1] >= failing
    assert_same_topk(s, it, exact_topk(U, I, k))
    assert _same((s, it), (s0, i0))


def test_seven_chunks_meet_the_1024_key_finalize(base):
    """k = 114, 3 user blocks on 7 slots: every block is a tail block of c = 7
    chunks, whose 7 * (k + 32) = 1022 end-compacted keys per user meet the
    1024-key finalize; 21 units for 7 workgroups, graded."""
    k, n = 114, 3 * 1024
    with _backend.plan_knobs(scan_slots=7, scan_floor=STAGE[128]):
        plan = ops.score_topk_plan(n, NI, torch.bfloat16, 128, k)
        assert plan["tail_chunks"] == 7 and plan["head_blocks"] == 0 and plan["grid"] == 7
        assert plan["tail_keys"] == 7 * (k + 32) and plan["sample_stride"] > 0
        assert _graded(*_chunks(n, torch.bfloat16, 128, k), STAGE[128])
        s, it, _ = _call(base["Ud"], base["Id"], k, n_users=n)
    assert_same_topk(s, it, _ref(base, k, n))


@pytest.fixture(scope="module")
def narrow():
    rng = np.random.default_rng(20264)
    U, I = int_table(rng, 3 * 2048 + 100, 64), int_table(rng, NI, 64)
    return {"U": U, "I": I, "ref": exact_topk(U, I, 100)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_other_row_widths_split_tail(narrow, dtype):
    """d = 64 bf16 (2048 users per workgroup, survivors staged in LDS) and d =
    64 fp32 (1024 per workgroup, the fp32 MFMA): 4 user blocks on 3 slots, one
    tail block of 3 graded chunks. Their seeded main scans are given the queue
    like the d = 128 one (the kernel's unit loop is one template)."""
    k = 100
    n = 3 * (2048 if dtype == torch.bfloat16 else 1024) + 100
    stage = STAGE[64] if dtype == torch.bfloat16 else STAGE[128]
    Ud, Id = _dev(narrow["U"][:n], dtype), _dev(narrow["I"], dtype)
    with _backend.plan_knobs(scan_slots=3, scan_floor=stage):
        plan = ops.score_topk_plan(n, NI, dtype, 64, k)
        assert plan["tail_chunks"] == 3 and plan["head_blocks"] == 3 and plan["sample_stride"] > 0
        assert _graded(*_chunks(n, dtype, 64, k), stage)
        s, it, _ = _call(Ud, Id, k)
        with _backend.plan_knobs(scan_split=1):
            whole = _call(Ud, Id, k)[:2]
    assert_same_topk(s, it, (narrow["ref"][0][:n], narrow["ref"][1][:n]))
    assert _same((s, it), whole)
