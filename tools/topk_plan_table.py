"""The planner's table: plans and workspace sizes of the scoring entry points
over shapes that straddle every planner edge (host only, no device work).

    python tools/topk_plan_table.py            # print the table of the built library
    python tools/topk_plan_table.py --write    # record tests/fixtures/topk_plans.json

tests/test_topk_plan_table.py compares the built library with the recorded
table row by row, so a change to csrc/score_topk.hip that is meant to keep the
plans (a refactor) proves it. Record a new table only with a change that is
meant to move a plan. Every row runs under scan_slots = 256, so the table does
not depend on the device.

A row: [users, items, dtype, d, k, knobs] -> rc and the 13 values of
dr_score_topk_plan, dr_score_topk_workspace, dr_score_topk_seeded_workspace,
and dr_sample_thresholds_workspace at the row's sample (S rows, rank ks; a
row without a guess asks for min(items, 2^17) rows at rank min(k, 256)).
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diversity-recommendations_amd"))

from divrec import _backend as B  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "fixtures", "topk_plans.json")

USERS = (1, 943, 16384, 16385, 262144, 1_000_000)
ITEMS = (1, 1682, 2048, 2049, 100_000, 2 ** 18 - 1, 2 ** 18, 1_250_000, 5_000_000, 2 ** 23,
         2 ** 23 + 1, 10_000_000)
KS = (1, 10, 100, 255, 256, 1000, 1024)
TABLES = (("bf16", 32), ("bf16", 128), ("bf16", 256), ("bf16", 512), ("f32", 32), ("f32", 128),
          ("f32", 256))
KNOBS = ({"scan_split": 1}, {"sample_dense": 0}, {"scan_seed": 0}, {"scan_seed": 1})


def shapes():
    """[users, items, dtype, d, k, knobs] of every row, in a fixed order."""
    rows = []
    for u in USERS:  # every users x items edge at the headline's table and k
        for i in ITEMS:
            rows.append([u, i, "bf16", 128, 100, {}])
    for k in KS:  # every k edge over every catalog edge, a split-tail user count
        for i in ITEMS:
            rows.append([16385, i, "bf16", 128, k, {}])
    for dt, d in TABLES:  # every table form: keep-all, plain, seeded, long catalogs
        for u in (943, 16385, 1_000_000):
            for i in (1682, 2049, 2 ** 18, 10_000_000):
                for k in (10, 1000):
                    rows.append([u, i, dt, d, k, {}])
    for kn in KNOBS:  # the A/B knobs on the seedable shapes
        for u in (16385, 1_000_000):
            for i in (2 ** 18, 1_250_000, 2 ** 23 + 1, 10_000_000):
                for k in (100, 1000):
                    rows.append([u, i, "bf16", 128, k, kn])
    seen, out = set(), []
    for r in rows:
        key = json.dumps(r, sort_keys=True)
        if key not in seen:
            seen.add(key)
            out.append(r)
    return out


def measure(row):
    """rc, the 13 plan values and the three workspace sizes of one row."""
    u, i, dt, d, k, knobs = row
    L = B.load_library()
    code = {"bf16": B.DR_BF16, "f32": B.DR_F32}[dt]
    out = (ctypes.c_int64 * 13)()
    with B.plan_knobs(scan_slots=256, **knobs):
        rc = L.dr_score_topk_plan(u, i, code, d, k, out, 13)
        plan = [int(x) for x in out] if rc == 0 else []
        S, ks = (plan[8], plan[9]) if rc == 0 and plan[8] > 0 else (min(i, 2 ** 17), min(k, 256))
        return {"rc": rc, "plan": plan,
                "ws": int(L.dr_score_topk_workspace(u, i, code, d, k)),
                "ws_seeded": int(L.dr_score_topk_seeded_workspace(u, i, code, d, k)),
                "ws_sample": int(L.dr_sample_thresholds_workspace(u, S, code, d, ks))}


def table():
    return [{"shape": r, **measure(r)} for r in shapes()]


def main():
    rows = table()
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
        print(f"{len(rows)} rows -> {FIXTURE}")
    else:
        for r in rows:
            print(json.dumps(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
