"""The catalog chunks of a split tail block (host only, no device work).

tail_chunk_bounds (csrc/score_scan_plan.h) through its two exports:
dr_tail_chunk_bounds, the rule on (n_items, c, stage items, floor), and
dr_score_topk_tail_chunks, the chunks dr_score_topk's main scan uses for a
call shape. The kernel calls the same function, so what holds here holds for
the units it scans.
"""
import ctypes
import os
import sys

import pytest

from divrec import _backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import topk_plan_table  # noqa: E402

STAGES = (288, 224, 448)  # rows per stage: d = 128, d = 128 long lists (CAP 2048), d = 64


def bounds(n_items, c, stage, floor):
    out = (ctypes.c_int64 * (c + 1))()
    rc = _backend.load_library().dr_tail_chunk_bounds(n_items, c, stage, floor, out)
    assert rc == 0, (n_items, c, stage, floor)
    return [int(x) for x in out]


def equal_chunks(n_items, c, stage):
    """The plan before the unit queue: c chunks of Plan::chunk_items rows."""
    per = -(-(-(-n_items // c)) // stage) * stage
    return [min(j * per, n_items) for j in range(c + 1)]


def _sweep():
    for stage in STAGES:
        lengths = {1, 31, 33, stage - 1, stage, stage + 1, 3 * stage + 5, 7 * stage, 16 * stage - 1,
                   16 * stage, 17 * stage + 3, 100 * stage + 77, (1 << 18) + 293, 1_250_000,
                   10_000_000, (1 << 31) - 2}
        for n in sorted(lengths):
            for c in (1, 2, 3, 5, 6, 7, 10, 16):
                floors = {1, stage, 2 * stage + 1, 65536, -(-n // c), max(1, n // c - 1), n,
                          (1 << 31) - 1}
                for floor in sorted(floors):
                    yield n, c, stage, floor


def test_bounds_sweep():
    """Every boundary a stage multiple (or the catalog's end), exact coverage,
    lengths that never increase, no empty chunk unless the catalog has fewer
    than c stages, c = 1 the whole catalog, no chunk of a graded plan below
    the floor, and a floor at or above n_items / c gives the equal chunks."""
    graded = 0
    for n, c, stage, floor in _sweep():
        b = bounds(n, c, stage, floor)
        key = (n, c, stage, floor)
        assert b[0] == 0 and b[-1] == n, key
        assert all(x % stage == 0 or x == n for x in b), key  # empty chunks sit at the end
        lens = [b[j + 1] - b[j] for j in range(c)]
        assert all(x >= 0 for x in lens), key
        assert all(lens[j] >= lens[j + 1] for j in range(c - 1)), key
        stages = -(-n // stage)
        if stages >= c:
            assert min(lens) > 0, key
        else:  # one stage each while they last
            assert lens == [min(stage, n - min(j * stage, n)) for j in range(c)], key
        if c == 1:
            assert b == [0, n], key
        eq = equal_chunks(n, c, stage)
        if floor * c >= n:
            # The old plan is this special case. Where the old formula left a
            # chunk empty although the catalog has a stage for each (fewer
            # than c * c stages: ceil(S / c) * (c - 1) >= S), "no empty chunk"
            # wins and the longer chunks give way; elsewhere the two agree.
            if stages < c or all(eq[j + 1] > eq[j] for j in range(c)):
                assert b == eq, key
            else:
                assert stages < c * c, key
        elif b != eq and stages >= c * c:
            graded += 1
            # the first chunk is half the catalog's stages, the second half of
            # the rest or an equal share of it, and no chunk (in whole stages,
            # the last one's partial stage counted) is below the floor
            assert c >= 3 and lens[0] == (stages // 2) * stage, key
            rest = stages - stages // 2
            assert -(-lens[1] // stage) in (rest // 2, -(-rest // (c - 1))), key
            floor_stages = -(-min(floor, n) // stage)
            assert min(-(-x // stage) for x in lens) >= floor_stages, key
    assert graded > 300  # the sweep does reach graded plans


def test_headline_grading():
    """1M x 10M, d = 128, k = 100 on 256 slots: c = 6 chunks of about 1/2, 1/4,
    1/8, 1/16, 1/32 and 1/32 of the catalog at the default floor."""
    b = bounds(10_000_000, 6, 288, 65536)
    lens = [b[j + 1] - b[j] for j in range(6)]
    for ln, frac in zip(lens, (2, 4, 8, 16, 32, 32)):
        assert abs(ln - 10_000_000 / frac) <= 2 * 288, lens
    assert bounds(10_000_000, 6, 288, 10_000_000) == equal_chunks(10_000_000, 6, 288)


def test_bounds_argument_errors():
    L = _backend.load_library()
    out = (ctypes.c_int64 * 17)()
    assert L.dr_tail_chunk_bounds(0, 2, 288, 1, out) == -1
    assert L.dr_tail_chunk_bounds(1 << 31, 2, 288, 1, out) == -1
    assert L.dr_tail_chunk_bounds(1000, 0, 288, 1, out) == -1
    assert L.dr_tail_chunk_bounds(1000, 17, 288, 1, out) == -1
    assert L.dr_tail_chunk_bounds(1000, 2, 100, 1, out) == -1
    assert L.dr_tail_chunk_bounds(1000, 2, 288, 0, out) == -1
    assert L.dr_tail_chunk_bounds(1000, 2, 288, 1, None) == -1


def _stage_items(dtype, d, cap):
    w = d if dtype == "bf16" else 2 * d
    if w == 128 and cap == 2048:
        return 57344 // (32 * w * 2) * 32
    nbytes = 73728 if w == 128 else (57344 if w <= 64 else 32768)
    return nbytes // (32 * w * 2) * 32


def test_every_plan_table_shape():
    """Over tools/topk_plan_table.py's shapes: the plan values and workspace
    sizes are the recorded ones (tests/fixtures/topk_plans.json; grading moves
    none of them), the export's chunk count is the plan's tail_chunks, its
    chunks are whole stages covering the catalog, and they are graded only
    where the seeded main scan has more units than workgroups."""
    import json
    L = _backend.load_library()
    with open(topk_plan_table.FIXTURE) as f:
        recorded = {json.dumps(r["shape"], sort_keys=True): r for r in json.load(f)}
    n_graded = 0
    for row in topk_plan_table.shapes():
        u, i, dt, d, k, knobs = row
        got = topk_plan_table.measure(row)
        want = recorded[json.dumps(row, sort_keys=True)]
        assert got == {x: want[x] for x in got}, row
        if got["rc"] != 0:
            continue
        plan = got["plan"]
        code = {"bf16": _backend.DR_BF16, "f32": _backend.DR_F32}[dt]
        out = (ctypes.c_int64 * 17)()
        nc = ctypes.c_int(0)
        with _backend.plan_knobs(scan_slots=256, **knobs):
            assert L.dr_score_topk_tail_chunks(u, i, code, d, k, out, 17, ctypes.byref(nc)) == 0
        c = nc.value
        assert c == plan[3], row
        b = [int(x) for x in out[:c + 1]]
        stage = _stage_items(dt, d, plan[6])
        assert b[0] == 0 and b[-1] == i and all(x % stage == 0 for x in b[:-1]), row
        eq = equal_chunks(i, c, stage)
        units = plan[2] + (plan[1] - plan[2]) * c
        if b != eq and -(-i // stage) < c * c:
            # a keep-all plan's stage-long chunks: equal but for the chunks the
            # old formula left empty (test_bounds_sweep)
            assert plan[6] >= i and all(b[j + 1] > b[j] for j in range(c)), row
        elif b != eq:
            n_graded += 1
            assert plan[7] > 0 and units > plan[5], row  # seeded, more units than workgroups
            assert min(-(-(b[j + 1] - b[j]) // stage) for j in range(c)) >= -(-65536 // stage), row
        else:
            assert eq[1] == min(plan[4], i), row  # chunk_items is the nominal equal length
    assert n_graded > 0


@pytest.mark.parametrize("floor,want", [(None, True), (1 << 30, False)])
def test_floor_and_queue_knobs(floor, want):
    """scan_floor moves the grading (a floor above the catalog: equal chunks),
    scan_queue = 0 turns it off with the queue; neither moves a plan value."""
    L = _backend.load_library()
    bf16 = _backend.DR_BF16
    out, nc = (ctypes.c_int64 * 17)(), ctypes.c_int(0)
    plan0 = (ctypes.c_int64 * 13)()
    plan1 = (ctypes.c_int64 * 13)()
    with _backend.plan_knobs(scan_slots=256):
        assert L.dr_score_topk_plan(1_000_000, 10_000_000, bf16, 128, 100, plan0, 13) == 0
        ws0 = L.dr_score_topk_workspace(1_000_000, 10_000_000, bf16, 128, 100)
        with _backend.plan_knobs(**({} if floor is None else {"scan_floor": floor})):
            assert L.dr_score_topk_tail_chunks(1_000_000, 10_000_000, bf16, 128, 100, out, 17,
                                               ctypes.byref(nc)) == 0
            assert L.dr_score_topk_plan(1_000_000, 10_000_000, bf16, 128, 100, plan1, 13) == 0
            assert L.dr_score_topk_workspace(1_000_000, 10_000_000, bf16, 128, 100) == ws0
        assert nc.value == 6 and list(plan0) == list(plan1)
        eq = equal_chunks(10_000_000, 6, 288)
        assert ([int(x) for x in out[:7]] != eq) == want
        with _backend.plan_knobs(scan_queue=0):
            assert L.dr_score_topk_tail_chunks(1_000_000, 10_000_000, bf16, 128, 100, out, 17,
                                               ctypes.byref(nc)) == 0
            assert [int(x) for x in out[:7]] == eq
            assert L.dr_score_topk_workspace(1_000_000, 10_000_000, bf16, 128, 100) == ws0
    assert L.dr_set_plan_knob(11, 31.0) == -1 and L.dr_set_plan_knob(12, 2.0) == -1
