"""A/B timing of the point-wise MSE step in ONE process: the generic path
(dr_gather_dot, torch elementwise loss, dr_gather_dot_backward, torch's Adam:
what point_wise_train_loop ran before dr_mse_fwd_bwd existed) against the
fused path, interleaved on the same inputs.

    python tools/pointwise_ab.py --shape ml100k [--reps 10] [--out FILE]
    python tools/pointwise_ab.py --shape 1m     [--reps 10] [--out FILE]

  ml100k  the reference experiment's shape (movie_lens_100k_mf_mse: 943 x 1682,
          d = 100, 90 000 interactions, batch_size 100, Adam lr 1e-3): one
          epoch of point_wise_train_loop, over PointWiseDataset and over
          DevicePointWiseDataset. Wall time, device-synchronised.
  1m      the config-3-like step (1M x 1M, d = 128, one batch of 1M uniform
          pairs): the kernel alone (HIP events; gradient tables preallocated
          in both arms) and kernel + dense Adam (point_wise_train_loop over
          that one batch). The fused kernel's time is stated as a fraction of
          its float-atomic budget, 2 d 4 B per pair at 1.3 TB/s.

The generic arm is the loops' own generic branch on this build: run_loop's
``fused=False`` argument turns the fast-path test off for the call. Prints one
JSON line per measurement (median / min / max ms per arm over ``--reps``
repetitions after ``--warmup``, and whether the fused arm's range lies wholly
below the generic arm's), each stamped with dr_build_id.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diversity-recommendations_amd"))
import torch  # noqa: E402

from divrec import _backend, datasets, losses, models, ops, train  # noqa: E402
from divrec.train import utils as train_utils  # noqa: E402

ATOMIC_TBS = 1.3  # chip-wide fp32 atomic add rate, contiguous 128-B segments


class OneBatch:
    """A point-wise data set of one device batch."""

    def __init__(self, uid, iid, target):
        self.batch = (uid, iid, None, None, target)

    def loader(self, **_):
        yield self.batch


def run_loop(dataset, model, optimizer, fused, **loader_params):
    """point_wise_train_loop with the fast path on, or (fused=False) off."""
    keep = train_utils._mse_fast_path
    if not fused:
        train_utils._mse_fast_path = lambda *a: False
    try:
        return train.point_wise_train_loop(dataset, model, losses.MSELoss(), optimizer,
                                           **loader_params)
    finally:
        train_utils._mse_fast_path = keep


def wall_ms(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1)


def ab(name, arms, timer, dev, reps, warmup, extra):
    """arms: {"generic": fn, "fused": fn}, run round-robin."""
    times = {k: [] for k in arms}
    for r in range(warmup + reps):
        for k, fn in arms.items():
            ms = timer(fn, dev)
            if r >= warmup:
                times[k].append(ms)
    rec = {"measurement": name, "reps": reps, "warmup": warmup, "build_id": _backend.build_id(),
           "device": torch.cuda.get_device_name(dev), **extra, "arms": {}}
    for k, v in times.items():
        rec["arms"][k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    a = rec["arms"]
    rec["speedup_median"] = a["generic"]["median_ms"] / a["fused"]["median_ms"]
    rec["fused_range_below_generic"] = a["fused"]["max_ms"] < a["generic"]["min_ms"]
    return rec


def shape_ml100k(dev, reps, warmup):
    nu, ni, d, n, bs = 943, 1682, 100, 90_000, 100
    g = torch.Generator().manual_seed(100)
    # grouped by user, like the MovieLens file after the experiment's split
    users = torch.sort(torch.randint(0, nu, (n,), generator=g)).values
    inter = torch.stack([users, torch.randint(0, ni, (n,), generator=g)], dim=1)
    scores = torch.randint(1, 6, (n,), generator=g).float()
    data = datasets.UserItemInteractionsDataset(
        inter, scores, number_of_users=nu, number_of_items=ni,
        user_features=datasets.Features(torch.zeros(nu, 1), ["x"]),
        item_features=datasets.Features(torch.zeros(ni, 1), ["x"]))
    out = []
    for kind, ds in (("PointWiseDataset", datasets.PointWiseDataset(data)),
                     ("DevicePointWiseDataset", datasets.DevicePointWiseDataset(data, device=dev))):
        arms = {}
        for arm in ("generic", "fused"):
            torch.manual_seed(1)
            mf = models.MatrixFactorization(nu, ni, d).to(dev)
            opt = torch.optim.Adam(mf.parameters(), lr=1e-3)
            arms[arm] = (lambda mf=mf, opt=opt, arm=arm:
                         run_loop(ds, mf, opt, arm == "fused", batch_size=bs))
        out.append(ab(f"ml100k epoch, {kind}", arms, wall_ms, dev, reps, warmup,
                      {"users": nu, "items": ni, "d": d, "interactions": n, "batch_size": bs,
                       "batches": n // bs, "timer": "wall"}))
    return out


def shape_1m(dev, reps, warmup):
    nu = ni = B = 1_000_000
    d = 128
    g = torch.Generator(device=dev).manual_seed(3)
    mf = models.MatrixFactorization(nu, ni, d).to(dev)
    with torch.no_grad():
        mf.user_embeddings.weight.mul_(0.1)
        mf.item_embeddings.weight.mul_(0.1)
    U, I = mf.user_embeddings.weight.data, mf.item_embeddings.weight.data
    uid = torch.randint(0, nu, (B,), generator=g, device=dev)
    iid = torch.randint(0, ni, (B,), generator=g, device=dev)
    target = torch.randint(1, 6, (B,), generator=g, device=dev).float()
    gU, gI = torch.zeros_like(U), torch.zeros_like(I)

    def generic_kernels():
        pred = ops.gather_dot(U, I, uid, iid, check=False)
        e = target - pred
        loss = torch.sum(e * e, dim=0) / B
        ops.gather_dot_backward(U, I, uid, iid, e * (-2.0 / B), gU, gI)
        return loss

    def fused_kernel():
        _, sq = ops.mse_fwd_bwd(U, I, uid, iid, target, 1.0 / B, gU, gI, check=False)
        return torch.sum(sq, dim=0) / B

    budget_ms = 2 * d * 4 * B / (ATOMIC_TBS * 1e12) * 1e3
    rec = ab("1M-pair step, kernels alone", {"generic": generic_kernels, "fused": fused_kernel},
             event_ms, dev, reps, warmup,
             {"users": nu, "items": ni, "d": d, "batch": B, "timer": "hip events",
              "atomic_bytes": 2 * d * 4 * B, "atomic_budget_ms": budget_ms})
    rec["fused_fraction_of_atomic_budget"] = budget_ms / rec["arms"]["fused"]["median_ms"]
    out = [rec]
    del gU, gI
    arms = {}
    one = OneBatch(uid, iid, target)
    for arm in ("generic", "fused"):
        m = models.MatrixFactorization(nu, ni, d).to(dev)
        m.load_state_dict(mf.state_dict())
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        arms[arm] = lambda m=m, opt=opt, arm=arm: run_loop(one, m, opt, arm == "fused")
    out.append(ab("1M-pair step, kernel + dense Adam", arms, wall_ms, dev, reps, warmup,
                  {"users": nu, "items": ni, "d": d, "batch": B, "timer": "wall"}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["ml100k", "1m"], required=True)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    recs = (shape_ml100k if args.shape == "ml100k" else shape_1m)(dev, max(args.reps, 10),
                                                                  args.warmup)
    for rec in recs:
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
