"""Timing of dr_ild_embedding_backward (the embedding ILD's gradient) in ONE
process, beside what a user had before it: torch autograd on the GPU over the
dense pair formula (gather [n, k, d], bmm, distances, reduce, backward with
respect to the gathered rows, one index_add_ into the dense gradient table).

    python tools/ild_backward_time.py [--users 1000000] [--items 1000000] [--k 100] [--d 128]
                                      [--torch-users 8192] [--reps 5] [--out FILE]

Two list sources over one fp32 item table:
  uniform  every id drawn uniformly from the catalog (no shared head);
  topk     the lists MatrixFactorization.score_topk gives for a random model
           (bf16 scoring): lists that share their head items, the contended
           case of the atomics (the record carries how shared they are).
Per source and kind it prints one JSON line stamped with dr_build_id: the
kernel's ms per call (HIP events, median / min / max over ``--reps`` after
``--warmup``), the fraction of its float-atomic budget (users k d 4 B at
1.3 TB/s), torch's ms at ``--torch-users`` lists scaled per list to
``--users``, and the ratio of the two. ``--out`` appends the lines to a file
(the records under profiles/ild_backward/ were written this way).
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

ATOMIC_TBS = 1.3  # chip-wide fp32 atomic add rate, contiguous 128-B segments
KINDS = ("cosine", "dot", "euclidean")


def torch_ild_sum(E, kind):
    """sum_u ILD_u of the gathered rows E [n, k, d] by the dense pair formula."""
    k = E.size(1)
    G = torch.bmm(E, E.transpose(1, 2))
    upper = torch.triu(torch.ones(k, k, dtype=torch.bool, device=E.device), 1)
    if kind == "dot":
        D = G
    else:
        nsq = torch.diagonal(G, dim1=1, dim2=2)
        if kind == "cosine":
            D = 1.0 - G / torch.sqrt(nsq.unsqueeze(2) * nsq.unsqueeze(1))
        else:  # the square root only where a pair counts (its derivative at 0 is inf)
            sq = nsq.unsqueeze(2) + nsq.unsqueeze(1) - 2.0 * G
            D = torch.where(upper, sq.clamp_min(1e-12), torch.ones_like(sq)).sqrt()
    return (D * upper).sum() / (k * (k - 1))


def sharing(recs, n_items):
    """How shared the lists' rows are: distinct items, and the adds into the
    most listed one."""
    counts = torch.bincount(recs.reshape(-1).to(torch.int64), minlength=n_items)
    return {"distinct_items": int((counts > 0).sum()), "max_lists_per_item": int(counts.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--torch-users", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, ni, k, d = args.users, args.items, args.k, args.d
    torch.manual_seed(11)
    mf = models.MatrixFactorization(n, ni, d).to(dev)
    W = mf.item_embeddings.weight.detach()
    g = torch.Generator(device=dev).manual_seed(12)
    sources = {"uniform": torch.randint(0, ni, (n, k), generator=g, device=dev, dtype=torch.int32)}
    with torch.no_grad():
        items, _ = mf.score_topk(k, precision="bf16")
    sources["topk"] = items.to(torch.int32)
    del items
    G = torch.zeros_like(W)
    atomic_bytes = n * k * d * 4
    budget_ms = atomic_bytes / (ATOMIC_TBS * 1e12) * 1e3
    nt = min(args.torch_users, n)
    for source, recs in sources.items():
        shared = sharing(recs, ni)
        for kind in KINDS:
            kern = timed(lambda: ops.ild_embedding_backward(recs, W, kind, G, check=False), dev,
                         args.reps, args.warmup)
            sub = recs[:nt].to(torch.int64)

            def torch_step():
                # per-list work only (it is scaled per list): the gradient of the
                # gathered rows, then one index_add_ into the dense table
                E = W[sub].requires_grad_(True)
                torch_ild_sum(E, kind).backward()
                G.index_add_(0, sub.reshape(-1), E.grad.reshape(-1, d))

            tor = timed(torch_step, dev, args.reps, args.warmup)
            scaled = tor["median_ms"] * n / nt
            rec = {"measurement": "ild_embedding_backward", "source": source, "kind": kind,
                   "users": n, "items": ni, "k": k, "d": d, "reps": args.reps,
                   "warmup": args.warmup, "timer": "hip events",
                   "build_id": _backend.build_id(), "device": torch.cuda.get_device_name(dev),
                   **shared, "kernel": kern, "atomic_bytes": atomic_bytes,
                   "atomic_budget_ms": budget_ms,
                   "fraction_of_atomic_budget": budget_ms / kern["median_ms"],
                   "torch_autograd": {**tor, "users": nt, "scaled_to_users_ms": scaled},
                   "torch_over_kernel": scaled / kern["median_ms"]}
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
