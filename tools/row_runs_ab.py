"""A/B of the training-step kernels (dr_bpr_fwd_bwd, dr_mse_fwd_bwd,
dr_gather_dot_backward) between builds of the library in one process, as
tools/mmr_ab.py does for dr_mmr_rerank: first what must be equal bit for bit,
then interleaved timing rounds (HIP events).

    python tools/row_runs_ab.py --libs parent,product [--rounds 7] [--out FILE]

A tag NAME is divrec/_lib/libdivrec_hip_NAME.so (tools/variant_bench.py), the
first tag the base the others are held to. Equal bit for bit at every width of
WIDTHS: loss / hit / pred of 4096 samples (the arithmetic order per sample),
and the gradient tables of a batch of 16 (one span, hence one group: its
atomics have one order; the MF backward's 16 pairs touch 16 distinct rows).
Timed at bench.py's bpr and gather shapes and tools/pointwise_ab.py's 1m shape
(1M x 1M tables, d = 128) and again at d = 100; ``within_base_spread`` says
that a tag's median is not above the base's slowest round.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "diversity-recommendations_amd"))
import torch  # noqa: E402

from divrec import _backend as B  # noqa: E402
from variant_bench import lib_for  # noqa: E402

WIDTHS = [1, 31, 32, 33, 64, 96, 100, 128, 160, 192, 224, 256, 257, 300, 384, 385, 512]
CALLS = ("dr_bpr_fwd_bwd", "dr_mse_fwd_bwd", "dr_gather_dot_backward")
DEV = torch.device("cuda", 0)


def load(tag):
    lib = lib_for(tag)
    for fn in CALLS + ("dr_build_id",):
        f = getattr(lib, fn)
        f.restype, f.argtypes = B.SIGNATURES[fn]
    return lib


def ptr(t):
    return None if t is None else t.data_ptr()


def call(lib, fn, U, I, ids, *rest):
    """One C call on the current stream; ``rest`` are its arguments after the
    id columns (tensors by pointer), the stream excepted."""
    rc = getattr(lib, fn)(U.data_ptr(), U.size(0), I.data_ptr(), I.size(0), U.size(1),
                          *(t.data_ptr() for t in ids), ids[0].numel(),
                          *(ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in rest),
                          torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0, lib.dr_last_error()


def outputs(lib, d, g):
    """Everything that has one value whatever the schedule, at width d."""
    nu, ni, n = 200, 300, 4096
    U = torch.randn(nu, d, generator=g, device=DEV) * 0.3
    I = torch.randn(ni, d, generator=g, device=DEV) * 0.3
    uid, pid, nid = (torch.randint(0, hi, (n,), generator=g, device=DEV) for hi in (nu, ni, ni))
    uid[5], pid[77] = nu, -1  # two samples out of range
    target = torch.randint(1, 6, (n,), generator=g, device=DEV).float()
    got = {}
    f32 = lambda *shape: torch.zeros(*shape, device=DEV)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=DEV)
    for m in (n, 16):  # the whole batch: per-sample outputs; its last 16: gradients too
        ids = [t[n - m:].contiguous() for t in (uid, pid, nid)]
        loss, hit, gU, gI, err = f32(m), i32(m), f32(nu, d), f32(ni, d), i32(1)
        call(lib, "dr_bpr_fwd_bwd", U, I, ids, 1.0 / m, loss, hit, gU, gI, err)
        got.update({f"bpr loss B={m}": loss, f"bpr hit B={m}": hit, f"bpr err B={m}": err})
        if m == 16:
            got.update({"bpr grad_user B=16": gU, "bpr grad_item B=16": gI})
        pred, sq, gU, gI, err = f32(m), f32(m), f32(nu, d), f32(ni, d), i32(1)
        call(lib, "dr_mse_fwd_bwd", U, I, ids[:2] + [target[n - m:].contiguous()], 1.0 / m, pred, sq,
             gU, gI, err)
        got.update({f"mse pred B={m}": pred, f"mse loss B={m}": sq, f"mse err B={m}": err})
        if m == 16:
            got.update({"mse grad_user B=16": gU, "mse grad_item B=16": gI})
        pred, sq = f32(m), f32(m)
        call(lib, "dr_mse_fwd_bwd", U, I, ids[:2] + [target[n - m:].contiguous()], 0.0, pred, sq,
             None, None, None)
        got.update({f"mse forward-only pred B={m}": pred, f"mse forward-only loss B={m}": sq})
    ids = [torch.randperm(hi, generator=g, device=DEV)[:16] for hi in (nu, ni)]
    gU, gI, err = f32(nu, d), f32(ni, d), i32(1)
    call(lib, "dr_gather_dot_backward", U, I, ids, target[:16].contiguous(), gU, gI, err)
    got.update({"gather grad_user n=16": gU, "gather grad_item n=16": gI, "gather err n=16": err})
    return {k: t.cpu() for k, t in got.items()}


def timed_cases(d, g):
    """name -> (C call, arguments): the shapes of bench.py --workload bpr /
    gather and tools/pointwise_ab.py --shape 1m, at width d."""
    n_rows, n, m = 1_000_000, 1 << 20, 20
    U = torch.randn(n_rows, d, generator=g, device=DEV) * 0.1
    I = torch.randn(n_rows, d, generator=g, device=DEV) * 0.1
    gU, gI = torch.zeros_like(U), torch.zeros_like(I)
    rand = lambda count: torch.randint(0, n_rows, (count,), generator=g, device=DEV)
    uni = [rand(n), rand(n), rand(n)]
    users = n // (m * m)  # PairWiseDataset's m x m product, users in order
    pos, neg = rand(users * m).view(users, m), rand(users * m).view(users, m)
    mxm = [torch.arange(users, device=DEV).repeat_interleave(m * m),
           pos.repeat_interleave(m, dim=1).reshape(-1), neg.repeat(1, m).reshape(-1)]
    loss, hit = torch.empty(n, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    pairs = [rand(1_000_000), rand(1_000_000)]
    target = torch.randint(1, 6, (1_000_000,), generator=g, device=DEV).float()
    pred, sq = torch.empty(1_000_000, device=DEV), torch.empty(1_000_000, device=DEV)
    big = [rand(1 << 23), rand(1 << 23)]
    gout = torch.randn(1 << 23, generator=g, device=DEV)
    return {
        "bpr uniform": ("dr_bpr_fwd_bwd", U, I, uni, 1.0 / n, loss, hit, gU, gI, None),
        "bpr m x m": ("dr_bpr_fwd_bwd", U, I, mxm, 1.0 / mxm[0].numel(), loss, hit, gU, gI, None),
        "mse train": ("dr_mse_fwd_bwd", U, I, pairs + [target], 1e-6, pred, sq, gU, gI, None),
        "mse forward": ("dr_mse_fwd_bwd", U, I, pairs + [target], 0.0, pred, sq, None, None, None),
        "gather backward": ("dr_gather_dot_backward", U, I, big, gout, gU, gI, None),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="", help="also write the JSON record to this file")
    args = ap.parse_args()
    tags = args.libs.split(",")
    libs = {t: load(t) for t in tags}
    rec = {"device": torch.cuda.get_device_name(DEV), "rounds": args.rounds, "base": tags[0],
           "build_ids": {t: libs[t].dr_build_id().decode() for t in tags},
           "bitwise": {"widths": WIDTHS, "differing": {t: {} for t in tags[1:]}}, "timing": []}
    for d in WIDTHS:
        outs = {t: outputs(libs[t], d, torch.Generator(device=DEV).manual_seed(d)) for t in tags}
        base = outs[tags[0]]
        assert int(base["bpr err B=4096"]) == 2  # the two bad samples were counted
        for t in tags[1:]:
            for k, v in outs[t].items():  # fp32 compared by its bits
                if not torch.equal(v.view(torch.int32), base[k].view(torch.int32)):
                    worst = (v.double() - base[k].double()).abs().nan_to_num().max().item()
                    rel = worst / max(base[k].double().abs().nan_to_num().max().item(), 1e-300)
                    rec["bitwise"]["differing"][t].setdefault(k, []).append(
                        {"d": d, "max_abs_diff": worst, "over_max_abs_value": rel})
    for t, diff in rec["bitwise"]["differing"].items():
        print(f"{t} against {tags[0]}, not equal bit for bit: " +
              (", ".join(f"{k} at d = {[e['d'] for e in v]}" for k, v in diff.items()) or "nothing"),
              file=sys.stderr, flush=True)
    for d in (128, 100):
        for name, (fn, *a) in timed_cases(d, torch.Generator(device=DEV).manual_seed(d)).items():
            times = {t: [] for t in tags}
            for r in range(-2, args.rounds):  # two warm-up rounds
                for t in tags:
                    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    e0.record()
                    call(libs[t], fn, *a)
                    e1.record()
                    torch.cuda.synchronize(DEV)
                    if r >= 0:
                        times[t].append(e0.elapsed_time(e1))
            row = {"case": name, "d": d, "tags": {}}
            for t in tags:
                row["tags"][t] = {"median_ms": statistics.median(times[t]), "min_ms": min(times[t]),
                                  "max_ms": max(times[t])}
                row["tags"][t]["within_base_spread"] = \
                    row["tags"][t]["median_ms"] <= row["tags"][tags[0]]["max_ms"]
            rec["timing"].append(row)
            print(f"d={d} {name}: " + " ".join(
                f"{t}={v['median_ms']:.3f} [{v['min_ms']:.3f}-{v['max_ms']:.3f}]"
                for t, v in row["tags"].items()), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
