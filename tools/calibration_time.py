"""Timing of dr_calibrated_rerank (greedy calibrated re-rank over item partition
labels) in ONE process, beside dr_mmr_rerank on the same candidates (context
only) and beside what a user had before it: the same greedy as batched torch
ops on the same GPU (k_out dependent steps of a few dozen launches over [n, C]
tensors with gathers).

    python tools/calibration_time.py [--users 262144] [--items 200000] [--cands 1000] [--k 100]
                                     [--d 128] [--labels 19] [--history 100] [--lam 0.5]
                                     [--torch-users 1024] [--reps 3] [--out FILE]

The candidates are the model's own top-``--cands`` lists (MatrixFactorization
.score_topk of a random model, bf16 scoring); every item draws one of
``--labels`` labels once, and a user's profile is dr_label_profile of a
synthetic history of ``--history`` random items. The torch greedy restates the
kernel's fp32 arithmetic operation by operation (the pairwise order of the
wave sums included), so its picks must all equal the kernel's: the tool
asserts that. It prints one JSON line stamped with dr_build_id: the kernel's
ms per call (HIP events, median / min / max over ``--reps`` after ``--warmup``)
and per 1M users, the candidate stream (users C 8 bytes) at the HBM peak as the
floor it stands on, torch's ms at ``--torch-users`` lists scaled per list and
the ratio of the two. ``--out`` appends the line to a file (the records under
profiles/calibration/ were written this way).
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

HBM_TBS = 8.0                       # MI355X vendor peak
ALPHA = float(np.float32(0.01))     # DR_CALIB_ALPHA
ONE_M = float(np.float32(1) - np.float32(0.01))
FLT_MAX = float(np.finfo(np.float32).max)


def _tree_sum(x):
    """Sum of 64 columns in the pairwise order of the kernel's DPP wave sum."""
    while x.size(1) > 1:
        x = x[:, 0::2] + x[:, 1::2]
    return x


def torch_calibrated(cand, sc, labels, profile, k, lam):
    """The spec's greedy as torch tensor ops over a batch of users, in the
    kernel's own fp32 arithmetic (include/divrec_hip.h, csrc/calibration.hip)."""
    n, C = cand.shape
    G, ni = profile.size(1), labels.numel()
    dev = cand.device
    rows = torch.arange(n, device=dev)
    live = (cand >= 0) & (cand < ni)
    lab = labels[cand.clamp(0, ni - 1).to(torch.int64)].to(torch.int64)
    live &= (lab >= 0) & (lab < G)
    lab = torch.where(live, lab, torch.zeros_like(lab))
    w = torch.zeros((n, 64), device=dev)
    w[:, :G] = torch.nan_to_num(profile, nan=0.0).clamp_min(0)
    total = _tree_sum(w)
    p = torch.where(total > 0, w / total, torch.zeros_like(w))
    pos = p > 0
    logp = torch.where(pos, torch.log(p), torch.zeros_like(p))
    neg_inf = torch.full_like(sc, float("-inf"))
    ls = torch.where(live, np.float32(lam).item() * sc.clamp_min(-FLT_MAX), neg_inf)
    mu = float(np.float32(1) - np.float32(lam))
    cnt = torch.zeros((n, 64), device=dev)
    out = torch.full((n, k), -1, dtype=torch.int32, device=dev)

    def term(count, inv):
        share = count * inv
        q = (share.double() * ONE_M + (ALPHA * p).double()).float()  # fmaf
        return torch.where(pos, p * (logp - torch.log(q)), torch.zeros_like(p))

    for t in range(k):
        inv = float(np.float32(1) / np.float32(t + 1))
        a, b = term(cnt, inv), term(cnt + 1, inv)
        klc = (_tree_sum(a) - a) + b
        val = ls + (-(mu * klc)).gather(1, lab)
        j = val.argmax(dim=1)  # the first maximum: the lowest position
        some = val[rows, j] > float("-inf")
        out[:, t] = torch.where(some, cand[rows, j], torch.full_like(cand[rows, j], -1))
        cnt[rows[some], lab[rows, j][some]] += 1
        ls[rows[some], j[some]] = float("-inf")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=262_144)
    ap.add_argument("--items", type=int, default=200_000)
    ap.add_argument("--cands", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--labels", type=int, default=19)
    ap.add_argument("--history", type=int, default=100)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--torch-users", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="", help="also append the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, ni, C, k, d, lam, G = (args.users, args.items, args.cands, args.k, args.d, args.lam,
                              args.labels)
    torch.manual_seed(11)
    mf = models.MatrixFactorization(n, ni, d).to(dev)
    with torch.no_grad():
        items, sc = mf.score_topk(C, precision="bf16")
    cand = items.to(torch.int32)
    del items
    table = mf.bf16_tables()[1]
    labels = torch.randint(0, G, (ni,), dtype=torch.int32, device=dev)
    rowptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * args.history
    hist = torch.randint(0, ni, (n * args.history,), dtype=torch.int32, device=dev)
    prof_t = timed(lambda: ops.label_profile(rowptr, hist, labels, G, check=False), dev,
                   args.reps, args.warmup)
    profile = ops.label_profile(rowptr, hist, labels, G)
    del hist

    cal = timed(lambda: ops.calibrated_rerank(cand, sc, labels, profile, k, lam, check=False),
                dev, args.reps, args.warmup)
    picks, kl = ops.calibrated_rerank(cand, sc, labels, profile, k, lam)
    metric_t = timed(lambda: ops.calibration_kl(picks, labels, profile, check=False), dev,
                     args.reps, args.warmup)
    kl_top = float(ops.calibration_kl(cand[:, :k].contiguous(), labels, profile).mean())
    kl_cal = float(kl[:, -1].mean())
    mmr = timed(lambda: ops.mmr_rerank(cand, sc, table, k, lam, check=False), dev, args.reps,
                args.warmup)

    nt = min(args.torch_users, n)
    sub, sub_sc, sub_p = cand[:nt].contiguous(), sc[:nt].contiguous(), profile[:nt].contiguous()
    tor = timed(lambda: torch_calibrated(sub, sub_sc, labels, sub_p, k, lam), dev,
                max(1, args.reps - 1), 1)
    want = torch_calibrated(sub, sub_sc, labels, sub_p, k, lam)
    different = int((picks[:nt] != want).sum())
    assert different == 0, f"{different} of {nt * k} picks differ from the torch greedy"

    per_m = 1e6 / n
    stream_ms = n * C * 8 / (HBM_TBS * 1e12) * 1e3
    scaled = tor["median_ms"] * n / nt
    rec = {"measurement": "calibrated_rerank", "users": n, "items": ni, "cands": C, "k": k, "d": d,
           "labels": G, "history": args.history, "lam": lam, "reps": args.reps,
           "warmup": args.warmup, "timer": "hip events", "build_id": _backend.build_id(),
           "device": torch.cuda.get_device_name(dev),
           "calibrated_kernel": cal, "calibrated_ms_per_1m_users": cal["median_ms"] * per_m,
           "candidate_stream_bytes": n * C * 8, "stream_floor_ms": stream_ms,
           "stream_floor_share": stream_ms / cal["median_ms"],
           "label_profile_kernel": prof_t, "calibration_kl_kernel": metric_t,
           "mean_kl_top_k": kl_top, "mean_kl_calibrated": kl_cal,
           "mmr_kernel": mmr, "mmr_ms_per_1m_users": mmr["median_ms"] * per_m,
           "torch_greedy": {**tor, "users": nt, "scaled_to_users_ms": scaled,
                            "ms_per_1m_users": tor["median_ms"] * 1e6 / nt},
           "torch_over_kernel": scaled / cal["median_ms"],
           "picks_compared": nt * k, "picks_different_from_torch": different}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
