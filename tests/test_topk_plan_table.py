"""The planner of csrc/score_topk.hip against its recorded table (host only).

tests/fixtures/topk_plans.json holds, for a few hundred call shapes that
straddle every planner edge (users, catalog rows, k, table dtype and width,
the A/B knobs), the 13 values of dr_score_topk_plan and the workspace sizes of
dr_score_topk, dr_score_topk_seeded and dr_sample_thresholds, recorded by
tools/topk_plan_table.py under scan_slots = 256 (no device dependence). The
built library must give every row again, value for value.
"""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "topk_plan_table", os.path.join(ROOT, "tools", "topk_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plans_and_workspaces_match_the_recorded_table():
    rec = _recorder()
    with open(rec.FIXTURE) as f:
        want = json.load(f)
    shapes = rec.shapes()
    assert len(want) == len(shapes) >= 300
    seeded = split = keep_all = 0
    for row, shape in zip(want, shapes):
        assert row["shape"] == shape  # the fixture was recorded over this very list
        got = rec.measure(shape)
        assert got == {k: row[k] for k in got}, shape
        assert got["rc"] == 0  # every shape of the table has a plan
        p = got["plan"]
        seeded += p[7] > 0
        split += p[3] > 1 and p[2] > 0
        keep_all += p[7] == 0 and p[6] >= shape[1] and shape[1] > 1
    # the table reaches every kind of plan
    assert seeded > 50 and split > 20 and keep_all > 5
