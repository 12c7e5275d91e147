"""Timing of dr_dpp_rerank (greedy DPP MAP re-rank) in ONE process, beside
dr_mmr_rerank on the same inputs (context only) and beside what a user had
before it: the same greedy in torch on the same GPU (batched gather, bmm Gram,
the Cholesky recurrence as tensor ops, k_out steps of a dozen launches).

    python tools/dpp_time.py [--users 262144] [--items 200000] [--cands 1000] [--k 100] [--d 128]
                             [--lam 0.5] [--torch-users 1024] [--reps 3] [--out FILE]

The candidates are the model's own top-``--cands`` lists (MatrixFactorization
.score_topk of a random model, bf16 scoring) over its bf16 item table. It
prints one JSON line stamped with dr_build_id: the kernels' ms per call (HIP
events, median / min / max over ``--reps`` after ``--warmup``) and per 1M
users, the share of the candidate pass's MAC budget (users C d k_out MACs at the
fp32 vector peak), torch's ms at ``--torch-users`` lists scaled per list, the
ratio of the two, and how many of torch's picks the kernel's lists share
(fp32 near-ties may differ). ``--out`` appends the line to a file (the records
under profiles/dpp/ were written this way).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diversity-recommendations_amd"))
import torch  # noqa: E402

from divrec import _backend, models, ops  # noqa: E402
from _timing import timed  # noqa: E402  (tools/_timing.py)

FP32_VECTOR_TFLOPS = 157.3  # MI355X vendor peak; one MAC = 2 FLOP
DPP_EPS = 1e-4              # DR_DPP_EPS


def torch_dpp(cand, sc, table, k, lam):
    """The spec's greedy as torch tensor ops over a batch of users: gather,
    bmm Gram, then per pick an argmax and the incremental Cholesky row."""
    n, C = cand.shape
    X = table[cand.to(torch.int64)].float()
    X = X / X.norm(dim=2, keepdim=True)
    S = torch.bmm(X, X.transpose(1, 2))
    rows = torch.arange(n, device=cand.device)
    r = torch.ones((n, C), device=cand.device)
    c = torch.zeros((n, k, C), device=cand.device)
    live = cand >= 0
    out = torch.full((n, k), -1, dtype=torch.int32, device=cand.device)
    for t in range(k):
        ok = live & (r > DPP_EPS)
        val = torch.where(ok, lam * sc + (1.0 - lam) * torch.log(r.clamp_min(1e-30)),
                          torch.full_like(sc, float("-inf")))
        j = val.argmax(dim=1)
        some = ok.any(dim=1)
        rj = r[rows, j].clamp_min(DPP_EPS)
        cj = c[rows, :t, j]
        e = (S[rows, j] - torch.einsum("ntc,nt->nc", c[:, :t], cj)) / rj.sqrt().unsqueeze(1)
        e = e * some.unsqueeze(1)
        c[:, t] = e
        r = r - e * e
        out[:, t] = torch.where(some, cand[rows, j], torch.full_like(cand[rows, j], -1))
        live[rows[some], j[some]] = False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=262_144)
    ap.add_argument("--items", type=int, default=200_000)
    ap.add_argument("--cands", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--torch-users", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="", help="also append the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, ni, C, k, d, lam = args.users, args.items, args.cands, args.k, args.d, args.lam
    torch.manual_seed(11)
    mf = models.MatrixFactorization(n, ni, d).to(dev)
    with torch.no_grad():
        items, sc = mf.score_topk(C, precision="bf16")
    cand = items.to(torch.int32)
    del items
    table = mf.bf16_tables()[1]

    dpp = timed(lambda: ops.dpp_rerank(cand, sc, table, k, lam, check=False), dev, args.reps,
                args.warmup)
    mmr = timed(lambda: ops.mmr_rerank(cand, sc, table, k, lam, check=False), dev, args.reps,
                args.warmup)
    nt = min(args.torch_users, n)
    sub, sub_sc = cand[:nt].contiguous(), sc[:nt].contiguous()
    tor = timed(lambda: torch_dpp(sub, sub_sc, table, k, lam), dev, max(1, args.reps - 1), 1)
    got = ops.dpp_rerank(sub, sub_sc, table, k, lam, check=False)[0]
    want = torch_dpp(sub, sub_sc, table, k, lam)
    same = float((got == want).float().mean())
    shared = float((got.sort(dim=1).values == want.sort(dim=1).values).float().mean())

    per_m = 1e6 / n
    macs = n * C * d * k
    budget_ms = 2.0 * macs / (FP32_VECTOR_TFLOPS * 1e12) * 1e3
    scaled = tor["median_ms"] * n / nt
    rec = {"measurement": "dpp_rerank", "users": n, "items": ni, "cands": C, "k": k, "d": d,
           "lam": lam, "reps": args.reps, "warmup": args.warmup, "timer": "hip events",
           "build_id": _backend.build_id(), "device": torch.cuda.get_device_name(dev),
           "dpp_kernel": dpp, "dpp_ms_per_1m_users": dpp["median_ms"] * per_m,
           "candidate_pass_macs": macs, "mac_budget_ms": budget_ms,
           "share_of_mac_budget": budget_ms / dpp["median_ms"],
           "mmr_kernel": mmr, "mmr_ms_per_1m_users": mmr["median_ms"] * per_m,
           "torch_greedy": {**tor, "users": nt, "scaled_to_users_ms": scaled,
                            "ms_per_1m_users": tor["median_ms"] * 1e6 / nt},
           "torch_over_kernel": scaled / dpp["median_ms"],
           "picks_equal_to_torch": same, "sorted_lists_equal_to_torch": shared}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
