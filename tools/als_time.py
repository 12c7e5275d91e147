"""Timing of dr_als_solve (one implicit-feedback ALS half-step) in ONE process,
beside what a user had before it: the same half-step as batched torch on the
same GPU (padded histories, einsum for the normal matrices,
torch.linalg.cholesky and cholesky_solve, ``--torch-batch`` rows per batch).

    python tools/als_time.py [--rows 1000000] [--fixed 1000000] [--d 128] [--per-row 100]
                             [--dist uniform|zipf] [--max-len 4096] [--torch-rows 4096]
                             [--sort-rows] [--reps 3] [--out FILE]

The CSR has ``--rows`` rows over a random N(0, 1) table of ``--fixed`` rows,
``--rows * --per-row`` entries in all: ``uniform`` gives every row ``--per-row``
entries, ``zipf`` gives row lengths proportional to 1 / rank (ranks dealt to
the rows at random, lengths clipped to [1, --max-len]) with the same total.
``--sort-rows`` hands the kernel the rows longest first (a host-side
permutation of the CSR, undone on the output; both are inside the timed call).
It prints one JSON line stamped with dr_build_id: the kernel's ms per call (HIP
events, median / min / max over ``--reps`` after ``--warmup``), the FMA floor
(sum over rows of n_r d^2 + d^3 / 3 FMAs at the fp32 vector peak) and the
kernel's share of it, torch's ms at ``--torch-rows`` rows scaled per row, the
ratio of the two, and the largest relative difference of the two results.
``--out`` appends the line to a file (the records under profiles/als/ were
written this way).
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

FP32_VECTOR_TFLOPS = 157.3  # MI355X vendor peak; one FMA = 2 FLOP


def row_lengths(n, per_row, dist, max_len, seed):
    """int64 [n] row lengths with the sum n * per_row."""
    if dist == "uniform":
        return np.full(n, per_row, dtype=np.int64)
    total = n * per_row
    weight = 1.0 / np.arange(1, n + 1, dtype=np.float64)
    lo, hi = 0.0, float(total) * 16
    for _ in range(100):  # the scale at which the clipped lengths add up to the total
        mid = 0.5 * (lo + hi)
        if np.clip(np.floor(weight * mid), 1, max_len).sum() < total:
            lo = mid
        else:
            hi = mid
    lengths = np.clip(np.floor(weight * hi), 1, max_len).astype(np.int64)
    lengths[-1] += total - lengths.sum()  # the rounding's remainder (small, maybe negative)
    lengths = np.maximum(lengths, 1)
    return np.random.default_rng(seed).permutation(lengths)


def torch_half_step(Y, G, rowptr, cols, alpha, reg, batch):
    """The half-step as batched torch ops over padded histories."""
    n, d = rowptr.numel() - 1, Y.size(1)
    out = torch.empty((n, d), dtype=torch.float32, device=Y.device)
    eye = reg * torch.eye(d, device=Y.device)
    for r0 in range(0, n, batch):
        ptr = rowptr[r0:r0 + batch + 1]
        lens = ptr[1:] - ptr[:-1]
        width = int(lens.max())
        at = torch.arange(width, device=Y.device)
        live = at[None, :] < lens[:, None]
        idx = cols[(ptr[:-1, None] + at[None, :]).clamp_(max=cols.numel() - 1)].to(torch.int64)
        rows = Y[idx] * live[..., None]
        A = G + alpha * torch.einsum("bld,ble->bde", rows, rows) + eye
        b = (1.0 + alpha) * rows.sum(1)
        L = torch.linalg.cholesky(A)
        out[r0:r0 + batch] = torch.cholesky_solve(b[..., None], L)[..., 0]
    return out


def sorted_solve(Y, G, rowptr, cols, alpha, reg):
    """als_solve over the rows longest first: the CSR permuted on the host
    side, the output rows put back."""
    lens = rowptr[1:] - rowptr[:-1]
    order = torch.argsort(lens, descending=True, stable=True)
    new_ptr = torch.zeros_like(rowptr)
    new_ptr[1:] = torch.cumsum(lens[order], 0)
    # entry e of the new row k is entry e of the old row order[k]
    src = torch.repeat_interleave(rowptr[:-1][order] - new_ptr[:-1], lens[order]) \
        + torch.arange(cols.numel(), device=cols.device)
    x = ops.als_solve(Y, new_ptr, cols[src], alpha=alpha, reg=reg, gram=G, check=False)
    out = torch.empty_like(x)
    out[order] = x
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--fixed", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--per-row", type=int, default=100)
    ap.add_argument("--dist", choices=("uniform", "zipf"), default="uniform")
    ap.add_argument("--max-len", type=int, default=4096)
    ap.add_argument("--alpha", type=float, default=40.0)
    ap.add_argument("--reg", type=float, default=0.1)
    ap.add_argument("--torch-rows", type=int, default=4096)
    ap.add_argument("--torch-batch", type=int, default=4096)
    ap.add_argument("--sort-rows", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="", help="also append the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, m, d = args.rows, args.fixed, args.d
    torch.manual_seed(13)
    Y = torch.randn((m, d), device=dev)
    lengths = row_lengths(n, args.per_row, args.dist, args.max_len, 17)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.from_numpy(np.cumsum(lengths))
    rowptr = rowptr.to(dev)
    nnz = int(lengths.sum())
    cols = torch.randint(0, m, (nnz,), device=dev, dtype=torch.int32)
    G = ops.gram(Y)

    if args.sort_rows:
        call = lambda: sorted_solve(Y, G, rowptr, cols, args.alpha, args.reg)  # noqa: E731
    else:
        call = lambda: ops.als_solve(Y, rowptr, cols, alpha=args.alpha, reg=args.reg, gram=G,  # noqa: E731
                                     check=False)
    kern = timed(call, dev, args.reps, args.warmup)
    gram_ms = timed(lambda: ops.gram(Y), dev, 1, 1)

    nt = min(args.torch_rows, n)
    sub_ptr = rowptr[:nt + 1].contiguous()
    sub_cols = cols[:int(sub_ptr[-1])].contiguous()
    tor = timed(lambda: torch_half_step(Y, G, sub_ptr, sub_cols, args.alpha, args.reg,
                                        args.torch_batch), dev, max(1, args.reps - 1), 1)
    got = call()[:nt]
    want = torch_half_step(Y, G, sub_ptr, sub_cols, args.alpha, args.reg, args.torch_batch)
    diff = float(((got - want).norm(dim=1) / want.norm(dim=1)).max())

    fmas = float((lengths.astype(np.float64) * d * d + d ** 3 / 3.0).sum())
    floor_ms = 2.0 * fmas / (FP32_VECTOR_TFLOPS * 1e12) * 1e3
    sub_share = float(lengths[:nt].sum()) / nnz  # torch's rows by their share of the entries
    scaled = tor["median_ms"] * n / nt
    rec = {"measurement": "als_solve", "rows": n, "fixed_rows": m, "d": d, "entries": nnz,
           "dist": args.dist, "max_row": int(lengths.max()), "sorted_rows": bool(args.sort_rows),
           "alpha": args.alpha, "reg": args.reg, "reps": args.reps, "warmup": args.warmup,
           "timer": "hip events", "build_id": _backend.build_id(),
           "device": torch.cuda.get_device_name(dev),
           "als_kernel": kern, "ms_per_1m_rows": kern["median_ms"] * 1e6 / n,
           "gram_ms": gram_ms["median_ms"],
           "fma_floor_ms": floor_ms, "share_of_fma_floor": floor_ms / kern["median_ms"],
           "torch_batched": {**tor, "rows": nt, "batch": args.torch_batch,
                             "share_of_entries": sub_share, "scaled_to_rows_ms": scaled},
           "torch_over_kernel": scaled / kern["median_ms"],
           "max_rel_diff_to_torch": diff}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
