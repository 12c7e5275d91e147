"""Timing of the WARP step (dr_warp_fwd_bwd) in ONE process, in the style of
tools/pointwise_ab.py and tools/row_runs_ab.py.

    python diversity-recommendations_amd/build_native.py --variant warp_r1 -D DR_WARP_ROUND=1
    python diversity-recommendations_amd/build_native.py --variant warp_r2 -D DR_WARP_ROUND=2
    python diversity-recommendations_amd/build_native.py --variant warp_flat4 -D DR_WARP_FIRST=4
    python tools/warp_time.py --libs product,warp_r1,warp_r2,warp_flat4 [--rounds 7] \
        [--out profiles/warp/warp_time.json]

Shape: 1M x 1M tables, d = 128, 1M (user, positive) pairs, max_trials 100,
margin 1, one positive per user (the positives CSR), no exclusions. Regimes:

  random   tables N(0, 0.1^2): every score is far inside the margin, the first
           draw violates (few trials per pair);
  planted  tables N(0, 0.42^2) (a random item scores N(0, 2^2) against a user)
           and each pair's positive row moved towards its user,
           I[p] += beta U[u] with beta uniform in [0.1, 0.25], so the positive
           is among the user's top-scoring items: pairs run long, and a share
           of them finds no violator.

Per regime, stamped with dr_build_id:
  * the kernel alone (HIP events around the one C call, gradient tables
    preallocated), for every library of --libs interleaved round-robin: the
    first tag is the shipped build (trial 0 alone, then rounds of
    DR_WARP_ROUND = 4 rows in flight), the others are builds at another
    DR_WARP_ROUND (dr_warp_round() says which) or, warp_flat4, with the first
    round as wide as the others (DR_WARP_FIRST = 4);
  * mean trials and the no-violator share, from the kernel's own outputs;
  * the algorithmic bytes per pair, (2 + scored trials) d 4 read and, with a
    violator, 3 d 4 added with atomics, as times at 8 TB/s and at the 1.3 TB/s
    fp32-atomic rate of DESIGN.md §3.6 (a skipped draw is not scored: with one
    positive per user in a catalog of 1M, 1 draw in a million);
  * the same step as batched torch on the same GPU: all B x T candidates of
    ops.warp_candidates' stream (drawn on the host and uploaded beforehand,
    outside the timed window), masked, scored, the first violator by argmax,
    the gradients by index_add_, in chunks that fit memory; its neg and
    trials are compared with the kernel's (torch's dot products round in
    another order, so a violation test within an fp32 rounding of its bar may
    go the other way: the record counts the differing pairs);
  * dr_bpr_fwd_bwd on the same pairs with uniform negatives, for context.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "diversity-recommendations_amd"))
import torch  # noqa: E402

from divrec import _backend as B  # noqa: E402
from divrec import ops  # noqa: E402
from variant_bench import lib_for  # noqa: E402

HBM_TBS = 8.0     # MI355X HBM3E peak
ATOMIC_TBS = 1.3  # chip-wide fp32 atomic add rate, contiguous 128-B segments
CALLS = ("dr_warp_fwd_bwd", "dr_warp_round", "dr_bpr_fwd_bwd", "dr_build_id", "dr_last_error")


def load(tag):
    lib = lib_for(tag)
    for fn in CALLS:
        f = getattr(lib, fn)
        f.restype, f.argtypes = B.SIGNATURES[fn]
    return lib


def make_regime(name, n, d, dev, g):
    """(U, I, uid, pid, positives CSR) of a regime: n users, n items, n pairs."""
    sigma = 0.1 if name == "random" else 0.42
    U = torch.randn(n, d, generator=g, device=dev) * sigma
    I = torch.randn(n, d, generator=g, device=dev) * sigma
    item_of = torch.randperm(n, generator=g, device=dev)  # user u's one positive
    if name == "planted":
        beta = 0.1 + 0.15 * torch.rand(n, generator=g, device=dev)
        I[item_of] += beta[:, None] * U
    uid = torch.randperm(n, generator=g, device=dev)  # every user once, shuffled
    pid = item_of[uid]
    rowptr = torch.arange(n + 1, dtype=torch.int64, device=dev)
    return U, I, uid, pid.contiguous(), (rowptr, item_of.to(torch.int32).contiguous())


def warp_call(lib, U, I, uid, pid, pos, T, margin, seed, out, gU, gI, dev):
    loss, neg, trials = out
    rc = lib.dr_warp_fwd_bwd(U.data_ptr(), U.size(0), I.data_ptr(), I.size(0), U.size(1),
                             uid.data_ptr(), pid.data_ptr(), uid.numel(), pos[0].data_ptr(),
                             pos[1].data_ptr(), None, None, T, margin, seed, 0,
                             1.0 / uid.numel(), loss.data_ptr(), neg.data_ptr(),
                             trials.data_ptr(), gU.data_ptr(), gI.data_ptr(), None,
                             torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, lib.dr_last_error()


def torch_step(U, I, uid, pid, pos, cand, T, margin, gU, gI, chunk):
    """The same step in batched torch: (loss, neg, trials), gradients added
    into gU / gI. ``cand`` int32 [B, T] on the tables' device. ``pos``: the
    positives CSR, searched as sorted keys user * n_items + item."""
    n_items = I.size(0)
    rowptr, items = pos
    rows = torch.repeat_interleave(torch.arange(rowptr.numel() - 1, device=U.device),
                                   rowptr[1:] - rowptr[:-1])
    keys = rows * n_items + items.to(torch.int64)  # sorted: rows ascending, items sorted per row
    n = uid.numel()
    loss = torch.empty(n, dtype=torch.float32, device=U.device)
    neg = torch.empty(n, dtype=torch.int64, device=U.device)
    trials = torch.empty(n, dtype=torch.int32, device=U.device)
    scale = 1.0 / n
    for b0 in range(0, n, chunk):
        u, p = uid[b0:b0 + chunk], pid[b0:b0 + chunk]
        c = cand[b0:b0 + chunk].to(torch.int64)
        ur, pr = U[u], I[p]
        sp = torch.sum(ur * pr, dim=1)
        sn = torch.bmm(I[c], ur[:, :, None])[:, :, 0]
        q = u[:, None] * n_items + c
        at = torch.searchsorted(keys, q).clamp_(max=keys.numel() - 1)
        skip = (c == p[:, None]) | (keys[at] == q)
        viol = ~skip & (sn > (sp - margin)[:, None])
        has = viol.any(dim=1)
        first = torch.argmax(viol.to(torch.int8), dim=1)
        tr = torch.where(has, first + 1, torch.full_like(first, T))
        cn = torch.gather(c, 1, first[:, None])[:, 0]
        rank = torch.clamp((n_items - 1) // tr, min=1)
        L = torch.where(has, torch.log(rank.float()), torch.zeros_like(sp))
        s_neg = torch.gather(sn, 1, first[:, None])[:, 0]
        loss[b0:b0 + chunk] = torch.where(has, L * (margin - sp + s_neg), torch.zeros_like(sp))
        neg[b0:b0 + chunk] = torch.where(has, cn, torch.full_like(cn, -1))
        trials[b0:b0 + chunk] = tr.to(torch.int32)
        g = (L * scale)[:, None]
        gU.index_add_(0, u, g * (I[cn] - pr))
        gI.index_add_(0, p, -g * ur)
        gI.index_add_(0, cn, g * ur)
    return loss, neg, trials


def timed(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1)


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


def measure(name, libs, n, d, T, margin, rounds, torch_reps, chunk, dev):
    g = torch.Generator(device=dev).manual_seed(17 if name == "random" else 29)
    U, I, uid, pid, pos = make_regime(name, n, d, dev, g)
    seed = 2024
    gU, gI = torch.zeros_like(U), torch.zeros_like(I)
    out = (torch.empty(n, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
           torch.empty(n, dtype=torch.int32, device=dev))
    tags = list(libs)
    arms = {t: (lambda t=t: warp_call(libs[t], U, I, uid, pid, pos, T, margin, seed, out, gU, gI,
                                      dev)) for t in tags}
    nid = torch.randint(0, n, (n,), generator=g, device=dev)
    hit = torch.empty(n, dtype=torch.int32, device=dev)

    def bpr():
        rc = libs[tags[0]].dr_bpr_fwd_bwd(U.data_ptr(), n, I.data_ptr(), n, d, uid.data_ptr(),
                                          pid.data_ptr(), nid.data_ptr(), n, 1.0 / n,
                                          out[0].data_ptr(), hit.data_ptr(), gU.data_ptr(),
                                          gI.data_ptr(), None,
                                          torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0

    arms["bpr (context)"] = bpr
    times = {k: [] for k in arms}
    for r in range(-2, rounds):  # two warm-up rounds, then round-robin
        for k, fn in arms.items():
            ms = timed(fn, dev)
            if r >= 0:
                times[k].append(ms)
    # the shipped build's outputs; every other build must reproduce neg and trials
    arms[tags[0]]()
    loss, neg, trials = (t.clone() for t in out)
    same_across_builds = True
    for t in tags[1:]:
        arms[t]()
        same_across_builds &= bool(torch.equal(out[1], neg) and torch.equal(out[2], trials))
    has = neg >= 0
    mean_trials = float(trials.double().mean())
    rec = {"regime": name, "users": n, "items": n, "d": d, "pairs": n, "max_trials": T,
           "margin": margin, "rounds": rounds, "timer": "hip events",
           "device": torch.cuda.get_device_name(dev),
           "build_ids": {t: libs[t].dr_build_id().decode() for t in tags},
           "rows_in_flight": {t: int(libs[t].dr_warp_round()) for t in tags},
           "first_round": "trial 0 alone (DR_WARP_FIRST = 1), but as wide as the others in warp_flat*",
           "shipped": tags[0], "mean_trials": mean_trials,
           "no_violator_share": float((~has).double().mean()),
           "neg_and_trials_equal_across_builds": same_across_builds,
           "kernel": {k: summary(v) for k, v in times.items()}}
    read_bytes = (2 * n + float(trials.double().sum())) * d * 4
    atomic_bytes = 3 * float(has.double().sum()) * d * 4
    ship = rec["kernel"][tags[0]]["median_ms"]
    rec["algorithmic"] = {
        "read_bytes": read_bytes, "atomic_bytes": atomic_bytes,
        "read_ms_at_8TBs": read_bytes / (HBM_TBS * 1e12) * 1e3,
        "atomic_ms_at_1.3TBs": atomic_bytes / (ATOMIC_TBS * 1e12) * 1e3,
    }
    floor = max(rec["algorithmic"]["read_ms_at_8TBs"], rec["algorithmic"]["atomic_ms_at_1.3TBs"])
    rec["algorithmic"]["bound"] = ("atomics" if floor == rec["algorithmic"]["atomic_ms_at_1.3TBs"]
                                   else "reads")
    rec["algorithmic"]["shipped_share_of_bound"] = floor / ship
    # batched torch on the same candidates
    cand = ops.warp_candidates(seed, 0, n, T, n).to(dev)
    tU, tI = torch.zeros_like(U), torch.zeros_like(I)
    run = lambda: torch_step(U, I, uid, pid, pos, cand, T, margin, tU, tI, chunk)
    run()  # warm-up
    t_times = [timed(run, dev) for _ in range(torch_reps)]
    _, t_neg, t_trials = run()
    differ = (t_neg != neg) | (t_trials != trials)
    rec["torch"] = {**summary(t_times), "reps": torch_reps, "chunk": chunk,
                    "pairs_with_other_neg_or_trials": int(differ.sum()),
                    "neg_and_trials_equal": not bool(differ.any())}
    rec["torch_over_shipped_median"] = rec["torch"]["median_ms"] / ship
    for t in tags[1:]:
        rec.setdefault("shipped_over", {})[t] = ship / rec["kernel"][t]["median_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="product", help="tags, the shipped build first")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1_000_000, help="users = items = pairs")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--max-trials", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=16384, help="pairs per torch chunk")
    ap.add_argument("--out", default="", help="also write the JSON records to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    libs = {t: load(t) for t in args.libs.split(",")}
    recs = []
    for name in ("random", "planted"):
        rec = measure(name, libs, args.pairs, args.dim, args.max_trials, 1.0, args.rounds,
                      args.torch_reps, args.chunk, dev)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")
    assert not math.isnan(recs[0]["mean_trials"])


if __name__ == "__main__":
    main()
