"""Timing of dr_history_distance (min and mean) and dr_serendipity_rerank in ONE
process, beside what a user had before them: the same computation as batched
torch ops on the same GPU (bf16 row gather, fp32 ``bmm``, normalise, ``amin`` /
``mean``, blend, stable ``sort``; ``--torch-users`` users per batch).

    python tools/serendipity_time.py [--users 262144] [--items 200000] [--cands 1000] [--k 100]
                                     [--d 128] [--history 100] [--zipf 1.0] [--max-history 16384]
                                     [--lam 0.5] [--torch-users 1024] [--reps 3] [--out FILE]

The candidates are the model's own top-``--cands`` lists (MatrixFactorization
.score_topk of a random model, bf16 scoring). Two history CSRs with the same
total: ``--history`` random items per user, and Zipf lengths (length of the
user of rank r proportional to r^-zipf, at most ``--max-history``, users
shuffled). Before timing, every kernel distance of the first ``--torch-users``
users is compared with torch's (both accumulate in fp32 in another order: at
most 2 (d + 16) 2^-23 apart), and every pick: equal, or a different candidate
whose blended value at that rank is within the same distance of torch's.
The torch form runs on the uniform histories only (a ragged batch would need
padding to the longest row) and gathers bf16 rows but multiplies in fp32: a
bf16 ``bmm`` output would round every cosine to 8 bits.
One JSON line stamped with dr_build_id: ms per call (HIP events, median / min /
max over ``--reps`` after ``--warmup``), the bytes each user's rows hold,
(C + |H|) d 2, over the time as GB/s beside the random 256-B row gather rate
of the embedding ILD (``--ild-gbs``, DESIGN 3.3 / bench.py's ild_roofline), the
Gram MFMA count ceil(C/32) ceil(|H|/32) d/16 per user as TFLOP/s, torch's ms
scaled per user and the ratios. ``--out`` appends the line to a file (the
records under profiles/serendipity/ were written this way).
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


def zipf_lengths(n, total, s, cap, gen):
    """int64 [n]: lengths proportional to rank^-s, clipped to cap, summing to
    ``total`` (within rounding: the remainder goes to the shortest rows), shuffled."""
    raw = torch.arange(1, n + 1, dtype=torch.float64) ** -s
    lo, hi = 0.0, float(total) * 1e3
    for _ in range(80):  # the scale at which the clipped lengths sum to total
        mid = (lo + hi) / 2
        if float((raw * mid).clamp(max=cap).sum()) < total:
            lo = mid
        else:
            hi = mid
    lens = (raw * lo).clamp(max=cap).floor().to(torch.int64)
    short = int(total - lens.sum())
    if short > 0:
        lens[n - short:] += 1
    return lens[torch.randperm(n, generator=gen)]


def torch_distance(cand, table, hist, reduce):
    """fp32 [n, C] for histories of one length (hist int32 [n, H])."""
    x = table[cand.long()].float()
    y = table[hist.long()].float()
    g = torch.bmm(x, y.transpose(1, 2))
    nx, ny = x.square().sum(2), y.square().sum(2)
    wx = torch.where(nx > 0, nx.rsqrt(), torch.zeros_like(nx))
    wy = torch.where(ny > 0, ny.rsqrt(), torch.zeros_like(ny))
    dist = 1.0 - g * wx[:, :, None] * wy[:, None, :]
    return dist.amin(2) if reduce == "min" else dist.mean(2)


def torch_rerank(cand, sc, table, hist, reduce, k, lam):
    dist = torch_distance(cand, table, hist, reduce)
    lam32 = float(np.float32(lam))
    val = lam32 * sc.nan_to_num(nan=-FLT_MAX).clamp_min(-FLT_MAX) + float(np.float32(1) - np.float32(lam)) * dist
    order = torch.sort(val, dim=1, descending=True, stable=True)
    top = order.indices[:, :k]
    return cand.gather(1, top), dist.gather(1, top), order.values[:, :k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=262_144)
    ap.add_argument("--items", type=int, default=200_000)
    ap.add_argument("--cands", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--history", type=int, default=100)
    ap.add_argument("--zipf", type=float, default=1.0)
    ap.add_argument("--max-history", type=int, default=16384)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--torch-users", type=int, default=1024)
    ap.add_argument("--ild-gbs", type=float, default=5250.0,
                    help="random 256-B row gather rate of the embedding ILD, GB/s")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="", help="also append the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, ni, C, k, d, lam, H = (args.users, args.items, args.cands, args.k, args.d, args.lam,
                              args.history)
    torch.manual_seed(11)
    gen = torch.Generator().manual_seed(12)
    mf = models.MatrixFactorization(n, ni, d).to(dev)
    with torch.no_grad():
        items, sc = mf.score_topk(C, precision="bf16")
    cand = items.to(torch.int32)
    del items
    table = mf.bf16_tables()[1]
    rowptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * H
    hist = torch.randint(0, ni, (n * H,), dtype=torch.int32, device=dev)
    lens = zipf_lengths(n, n * H, args.zipf, args.max_history, gen)
    z_rowptr = torch.zeros(n + 1, dtype=torch.int64)
    z_rowptr[1:] = lens.cumsum(0)
    z_rowptr = z_rowptr.to(dev)
    z_hist = torch.randint(0, ni, (int(z_rowptr[-1]),), dtype=torch.int32, device=dev)

    # ---- every pick and distance of the first users against torch, before timing
    nt = min(args.torch_users, n)
    sub, sub_sc = cand[:nt].contiguous(), sc[:nt].contiguous()
    sub_hist = hist[: nt * H].view(nt, H)
    bound = 2 * (d + 16) * 2.0 ** -23
    checks = {}
    for reduce in ("min", "mean"):
        got = ops.history_distance(sub, table, rowptr[: nt + 1], hist[: nt * H], reduce)
        want = torch_distance(sub, table, sub_hist, reduce)
        worst = float((got - want).abs().max())
        assert worst <= bound, f"{reduce}: distances differ from torch by {worst:.3e} > {bound:.3e}"
        checks[f"max_abs_distance_diff_{reduce}"] = worst
    picks, pdist = ops.serendipity_rerank(sub, sub_sc, table, rowptr[: nt + 1], hist[: nt * H], k,
                                          lam, "min")
    t_items, t_dist, t_val = torch_rerank(sub, sub_sc, table, sub_hist, "min", k, lam)
    ids_sorted, order = sub.sort(dim=1)  # candidate ids are distinct per user
    at = torch.searchsorted(ids_sorted, picks.contiguous()).clamp_(max=C - 1)
    p_sc = sub_sc.gather(1, order.gather(1, at))
    p_val = float(np.float32(lam)) * p_sc + float(np.float32(1) - np.float32(lam)) * pdist
    different = picks != t_items
    apart = float((p_val - t_val).abs().max())
    assert apart <= bound, f"a pick's value is {apart:.3e} from torch's at its rank (> {bound:.3e})"
    checks.update(picks_compared=nt * k, picks_different_from_torch=int(different.sum()),
                  max_abs_value_diff_at_rank=apart)

    # ---- timing
    t = {}
    for name, rp, hs in (("uniform", rowptr, hist), ("zipf", z_rowptr, z_hist)):
        for reduce in ("min", "mean"):
            t[f"distance_{reduce}_{name}"] = timed(
                lambda: ops.history_distance(cand, table, rp, hs, reduce, check=False), dev,
                args.reps, args.warmup)
        t[f"rerank_min_{name}"] = timed(
            lambda: ops.serendipity_rerank(cand, sc, table, rp, hs, k, lam, "min", check=False),
            dev, args.reps, args.warmup)
    tor = {}
    for reduce in ("min", "mean"):
        tor[f"distance_{reduce}"] = timed(lambda: torch_distance(sub, table, sub_hist, reduce), dev,
                                          max(1, args.reps - 1), 1)
    tor["rerank_min"] = timed(lambda: torch_rerank(sub, sub_sc, table, sub_hist, "min", k, lam),
                              dev, max(1, args.reps - 1), 1)

    bytes_user = (C + H) * d * 2
    mfma_user = -(-C // 32) * -(-H // 32) * (d // 16)
    flop_user = mfma_user * 2 * 32 * 32 * 16

    def model(ms):
        gbs = bytes_user * n / (ms * 1e-3) / 1e9
        return {"gb_per_s": gbs, "fraction_of_ild_gather_rate": gbs / args.ild_gbs,
                "gram_tflops": flop_user * n / (ms * 1e-3) / 1e12}

    ratios = {key: tor[key]["median_ms"] * n / nt / t[f"{key}_uniform"]["median_ms"] for key in tor}
    rec = {"measurement": "serendipity", "users": n, "items": ni, "cands": C, "k": k, "d": d,
           "history": H, "zipf": args.zipf, "max_history": int(lens.max()), "lam": lam,
           "reps": args.reps, "warmup": args.warmup, "timer": "hip events",
           "build_id": _backend.build_id(), "library": os.path.basename(str(_backend.lib_path())),
           "device": torch.cuda.get_device_name(dev),
           "kernel": t, "bytes_per_user": bytes_user, "gram_mfma_per_user": mfma_user,
           "ild_gather_gb_per_s": args.ild_gbs,
           "byte_model": {key: model(v["median_ms"]) for key, v in t.items() if "uniform" in key},
           "zipf_over_uniform": {key: t[f"{key}_zipf"]["median_ms"] / t[f"{key}_uniform"]["median_ms"]
                                 for key in tor},
           "torch": {key: {**v, "users": nt, "scaled_to_users_ms": v["median_ms"] * n / nt}
                     for key, v in tor.items()},
           "torch_over_kernel": ratios, "checks": checks}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    for key, r in ratios.items():  # the acceptance: below the batched-torch time in the same run
        assert r > 1.0, f"{key}: the kernel is not faster than batched torch (ratio {r:.2f})"


if __name__ == "__main__":
    main()
