"""Timing of dr_csr_row_sum (the feature-composition row sum and its transposed
backward) in ONE process, beside the same product by torch on the same GPU:
``torch.nn.functional.embedding_bag(mode="sum", per_sample_weights=...)`` and a
``torch.sparse`` CSR matrix times the dense table.

    python tools/feature_time.py [--rows 1000000] [--per-row 10] [--features 100000]
                                 [--d 128] [--reps 5] [--warmup 2] [--out FILE]

Three shapes, all with ``--rows * --per-row`` weighted entries:
  * forward: ``--rows`` rows of ``--per-row`` uniform entries over a
    ``--features`` x ``--d`` table (composing a table from feature embeddings);
  * backward, Zipf: the TRANSPOSE of a ``--rows``-row map whose feature
    popularity is proportional to 1 / rank: ``--features`` rows over a
    ``--rows`` x ``--d`` gradient table, the most popular feature one row of
    about a twelfth of all entries;
  * backward, uniform: the transpose of a map with uniform popularity (the
    same entries, evenly loaded rows): what the split rule is judged against.
It prints one JSON line stamped with dr_build_id: per shape the kernel's ms per
call (HIP events, median / min / max over ``--reps`` after ``--warmup``), its
algorithmic bytes (nnz d 4 read + rows d 4 written) over its time as TB/s and
as a share of the random whole-row gather ceiling (5.5 TB/s) and of 8 TB/s,
both baselines' ms and their ratio to the kernel, the largest difference to
embedding_bag's result; then the Zipf / uniform backward ratio beside the
uniform case's own run-to-run spread. ``--out`` appends the line to a file (the
records under profiles/feature_sum/ were written this way).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diversity-recommendations_amd"))
import torch  # noqa: E402

from divrec import _backend, ops  # noqa: E402
from _timing import timed  # noqa: E402  (tools/_timing.py)

GATHER_CEILING_TBS = 5.5  # random whole rows >= 1 KB into registers (lower end of the measured range)
HBM_PEAK_TBS = 8.0


def measure(name, table, rowptr, cols, weights, dev, reps, warmup):
    """One shape: the kernel with its plan, embedding_bag, sparse CSR mm."""
    n, (m, d), nnz = rowptr.numel() - 1, table.shape, cols.numel()
    plan = ops.row_sum_plan(rowptr)
    kern = timed(lambda: ops.csr_row_sum(table, rowptr, cols, weights, plan=plan, check=False),
                 dev, reps, warmup)
    cols64, offsets = cols.to(torch.int64), rowptr[:-1].contiguous()
    bag_call = lambda: torch.nn.functional.embedding_bag(  # noqa: E731
        cols64, table, offsets, mode="sum", per_sample_weights=weights)
    bag = timed(bag_call, dev, reps, warmup)
    S = torch.sparse_csr_tensor(rowptr, cols64, weights, size=(n, m))
    spmm = timed(lambda: S @ table, dev, reps, warmup)
    got = ops.csr_row_sum(table, rowptr, cols, weights, plan=plan, check=False)
    diff = float((got - bag_call()).abs().max())
    lens = rowptr[1:] - rowptr[:-1]
    nbytes = (nnz + n) * d * 4
    tbs = nbytes / (kern["median_ms"] * 1e-3) / 1e12
    best = min(bag["median_ms"], spmm["median_ms"])
    return {"shape": name, "rows": n, "table_rows": m, "d": d, "entries": nnz,
            "max_row": int(lens.max()), "median_row": float(lens.median()),
            "chunks": plan.n_chunks, "long_rows": plan.n_long,
            "kernel": kern, "algorithmic_bytes": nbytes, "kernel_tbs": tbs,
            "share_of_gather_ceiling": tbs / GATHER_CEILING_TBS,
            "share_of_hbm_peak": tbs / HBM_PEAK_TBS,
            "embedding_bag": bag, "sparse_csr_mm": spmm,
            "faster_baseline_over_kernel": best / kern["median_ms"],
            "max_abs_diff_to_embedding_bag": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--per-row", type=int, default=10)
    ap.add_argument("--features", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="also append the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, f, d, nnz = args.rows, args.features, args.d, args.rows * args.per_row
    rng = np.random.default_rng(23)
    torch.manual_seed(23)
    rowptr = (torch.arange(n + 1, dtype=torch.int64) * args.per_row).to(dev)
    weights = torch.rand(nnz, device=dev) + 0.5
    uniform = torch.from_numpy(rng.integers(0, f, nnz).astype(np.int32)).to(dev)
    p = 1.0 / np.arange(1, f + 1)
    zipf = torch.from_numpy(rng.permutation(f)[rng.choice(f, nnz, p=p / p.sum())]
                            .astype(np.int32)).to(dev)
    feature_table = torch.randn((f, d), device=dev)
    grad_table = torch.randn((n, d), device=dev)

    shapes = [measure("forward_uniform", feature_table, rowptr, uniform, weights, dev,
                      args.reps, args.warmup)]
    for name, cols in (("backward_zipf", zipf), ("backward_uniform", uniform)):
        rt, ct, wt = ops.csr_transpose(rowptr, cols, weights, f)
        shapes.append(measure(name, grad_table, rt, ct, wt, dev, args.reps, args.warmup))
    by = {s["shape"]: s for s in shapes}
    uni = by["backward_uniform"]["kernel"]
    rec = {"measurement": "csr_row_sum", "chunk": ops.ROW_SUM_CHUNK, "reps": args.reps,
           "warmup": args.warmup, "timer": "hip events", "build_id": _backend.build_id(),
           "device": torch.cuda.get_device_name(dev),
           "gather_ceiling_tbs": GATHER_CEILING_TBS, "hbm_peak_tbs": HBM_PEAK_TBS,
           "shapes": shapes,
           "zipf_over_uniform_backward": by["backward_zipf"]["kernel"]["median_ms"] / uni["median_ms"],
           "uniform_backward_spread": (uni["max_ms"] - uni["min_ms"]) / uni["median_ms"]}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
