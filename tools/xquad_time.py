"""Timing of dr_xquad_rerank (greedy aspect-coverage re-rank over a multi-hot
item-aspect matrix) in ONE process, beside dr_mmr_rerank and
dr_calibrated_rerank on the same candidates (context only) and beside what a
user had before it: the same greedy as batched torch ops on the same GPU
(k_out dependent steps, each an argmax over [n, C] and one [n, C] update per
aspect).

    python tools/xquad_time.py [--users 262144] [--items 200000] [--cands 1000] [--k 100]
                               [--d 128] [--aspects 19] [--history 100] [--lam 0.5]
                               [--torch-users 1024] [--reps 3] [--out FILE]

The candidates are the model's own top-``--cands`` lists (MatrixFactorization
.score_topk of a random model, bf16 scoring); every item draws one to three of
``--aspects`` binary aspects once, and a user's profile is dr_aspect_profile
of a synthetic history of ``--history`` random items. The torch greedy restates
the kernel's fp32 arithmetic operation by operation (the pairwise order of the
profile's wave sum, div summed in aspect order, one separate multiply and add
per update, the lowest position among equal values), so its picks must all
equal the kernel's: the tool asserts that. It prints one JSON line stamped with
dr_build_id: the kernel's ms per call (HIP events, median / min / max over
``--reps`` after ``--warmup``) and per 1M users, the LDS bytes the incremental
and the full-recompute form read per step as the budget beside it, torch's ms
at ``--torch-users`` lists scaled per list and the ratio of the two, the two
small kernels, and the mean coverage of the plain top-k lists and of the
re-ranked ones. ``--out`` appends the line to a file (the records under
profiles/xquad/ were written this way).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diversity-recommendations_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from divrec import _backend, models, ops  # noqa: E402
from _timing import timed  # noqa: E402  (tools/_timing.py)

FLT_MAX = float(np.finfo(np.float32).max)


def _tree_sum(x):
    """Sum of 64 columns in the pairwise order of the kernel's DPP wave sum."""
    while x.size(1) > 1:
        x = x[:, 0::2] + x[:, 1::2]
    return x


def multi_hot(ni, G, dev):
    """fp32 [ni, G]: one to three binary aspects per item (fewer where the draws repeat)."""
    A = torch.zeros((ni, G), device=dev)
    count = torch.randint(1, 4, (ni,), device=dev)
    rows = torch.arange(ni, device=dev)
    for r in range(3):
        use = r < count
        A[rows[use], torch.randint(0, G, (ni,), device=dev)[use]] = 1.0
    return A


def torch_xquad(cand, sc, aspects, profile, k, lam):
    """The spec's greedy as torch tensor ops over a batch of users, in the
    kernel's own fp32 arithmetic (include/divrec_hip.h, csrc/xquad.hip)."""
    n, C = cand.shape
    ni, G = aspects.shape
    dev = cand.device
    rows = torch.arange(n, device=dev)
    live = (cand >= 0) & (cand < ni)
    c = torch.nan_to_num(aspects, nan=0.0, posinf=1.0).clamp(0, 1)[cand.clamp(0, ni - 1).long()]
    c = c * live[:, :, None]
    w = torch.zeros((n, 64), device=dev)
    w[:, :G] = torch.nan_to_num(profile, nan=0.0).clamp_min(0)
    total = _tree_sum(w)
    m = torch.where(total > 0, w / total, torch.zeros_like(w))[:, :G].contiguous()
    div = torch.zeros((n, C), device=dev)
    for a in range(G):
        div = div + m[:, a, None] * c[:, :, a]
    neg_inf = torch.full_like(sc, float("-inf"))
    ls = torch.where(live, np.float32(lam).item() * sc.nan_to_num(nan=-FLT_MAX).clamp_min(-FLT_MAX),
                     neg_inf)
    mu = float(np.float32(1) - np.float32(lam))
    position = torch.arange(C, device=dev).expand(n, C)
    out = torch.full((n, k), -1, dtype=torch.int32, device=dev)
    for t in range(k):
        val = ls + mu * div
        best = val.max(dim=1, keepdim=True).values
        j = torch.where(val == best, position, C).min(dim=1).values  # the lowest position
        some = best[:, 0] > float("-inf")
        j = j.clamp_max(C - 1)
        out[:, t] = torch.where(some, cand[rows, j], torch.full_like(cand[rows, j], -1))
        delta = m * (c[rows, j] * some[:, None])
        m = m - delta
        for a in range(G):  # a zero delta changes nothing: the kernel's skip needs no restating
            div = div - delta[:, a, None] * c[:, :, a]
        ls[rows[some], j[some]] = float("-inf")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=262_144)
    ap.add_argument("--items", type=int, default=200_000)
    ap.add_argument("--cands", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--aspects", type=int, default=19)
    ap.add_argument("--history", type=int, default=100)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--torch-users", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="", help="also append the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, ni, C, k, d, lam, G = (args.users, args.items, args.cands, args.k, args.d, args.lam,
                              args.aspects)
    torch.manual_seed(11)
    mf = models.MatrixFactorization(n, ni, d).to(dev)
    with torch.no_grad():
        items, sc = mf.score_topk(C, precision="bf16")
    cand = items.to(torch.int32)
    del items
    table = mf.bf16_tables()[1]
    A = multi_hot(ni, G, dev)
    rowptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * args.history
    hist = torch.randint(0, ni, (n * args.history,), dtype=torch.int32, device=dev)
    prof_t = timed(lambda: ops.aspect_profile(rowptr, hist, A, check=False), dev, args.reps,
                   args.warmup)
    profile = ops.aspect_profile(rowptr, hist, A)

    xq = timed(lambda: ops.xquad_rerank(cand, sc, A, profile, k, lam, check=False), dev,
               args.reps, args.warmup)
    picks, cov = ops.xquad_rerank(cand, sc, A, profile, k, lam)
    metric_t = timed(lambda: ops.aspect_coverage(picks, A, profile, check=False), dev, args.reps,
                     args.warmup)
    cov_top = float(ops.aspect_coverage(cand[:, :k].contiguous(), A, profile).mean())
    cov_xq = float(cov[:, -1].mean())
    per_pick = float(A[picks[:1024].long().clamp_min(0)].sum(dim=2).mean())  # aspects per pick

    # context: the two other re-rankers on the same candidates (the calibrated
    # one over each item's first aspect as its partition label)
    mmr = timed(lambda: ops.mmr_rerank(cand, sc, table, k, lam, check=False), dev, args.reps,
                args.warmup)
    labels = A.argmax(dim=1).to(torch.int32)
    lab_profile = ops.label_profile(rowptr, hist, labels, G)
    del hist
    cal = timed(lambda: ops.calibrated_rerank(cand, sc, labels, lab_profile, k, lam, check=False),
                dev, args.reps, args.warmup)

    nt = min(args.torch_users, n)
    sub, sub_sc, sub_p = cand[:nt].contiguous(), sc[:nt].contiguous(), profile[:nt].contiguous()
    tor = timed(lambda: torch_xquad(sub, sub_sc, A, sub_p, k, lam), dev, max(1, args.reps - 1), 1)
    want = torch_xquad(sub, sub_sc, A, sub_p, k, lam)
    different = int((picks[:nt] != want).sum())
    assert different == 0, f"{different} of {nt * k} picks differ from the torch greedy"

    per_m = 1e6 / n
    scaled = tor["median_ms"] * n / nt
    rec = {"measurement": "xquad_rerank", "users": n, "items": ni, "cands": C, "k": k, "d": d,
           "aspects": G, "history": args.history, "lam": lam, "reps": args.reps,
           "warmup": args.warmup, "timer": "hip events", "build_id": _backend.build_id(),
           "device": torch.cuda.get_device_name(dev),
           "xquad_kernel": xq, "xquad_ms_per_1m_users": xq["median_ms"] * per_m,
           "xquad_us_per_user_step": xq["median_ms"] * 1e3 / (n * k),
           "aspects_per_pick": per_pick,
           "lds_bytes_per_step_incremental": per_pick * C * 4,
           "lds_bytes_per_step_full_recompute": G * C * 4,
           "aspect_profile_kernel": prof_t, "aspect_coverage_kernel": metric_t,
           "mean_coverage_top_k": cov_top, "mean_coverage_xquad": cov_xq,
           "mmr_kernel": mmr, "mmr_ms_per_1m_users": mmr["median_ms"] * per_m,
           "calibrated_kernel": cal, "calibrated_ms_per_1m_users": cal["median_ms"] * per_m,
           "torch_greedy": {**tor, "users": nt, "scaled_to_users_ms": scaled,
                            "ms_per_1m_users": tor["median_ms"] * 1e6 / nt},
           "torch_over_kernel": scaled / xq["median_ms"],
           "picks_compared": nt * k, "picks_different_from_torch": different}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
