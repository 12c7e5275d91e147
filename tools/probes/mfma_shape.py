"""Run tools/probes/mfma_shape.hip: TFLOP/s and in-kernel clock of 32x32x16 and
16x16x32 bf16 MFMA loops on random operands, one 512-thread workgroup per CU,
at the clock the chip sustains.

Two arm pairs: `reg` keeps both operands in registers; `lds` is the score
scan's d = 128 tile step (B in 128 VGPRs, A re-read from a swizzled LDS image
with 8 ds_read_b128 per 1024 MFMA cycles). Each arm runs back-to-back ~20-ms
launches for --seconds before it is timed and for --seconds while it is timed
(a short single launch runs above the sustained clock and ranks the shapes by
cycles alone). The shapes alternate for --rounds rounds. The clock is
d(s_memtime) / d(s_memrealtime) x 100 MHz around the loop of the last timed
launch, median over workgroups. Prints one JSON line and writes it to --out.

    hipcc --offload-arch=gfx950 -O3 -shared -fPIC tools/probes/mfma_shape.hip -o tools/probes/libmfma_shape.so
    python tools/probes/mfma_shape.py --out profiles/mfma16/probe.json
"""
import argparse
import ctypes
import json
import math
import os
import statistics

import torch

HERE = os.path.dirname(os.path.abspath(__file__))

# flops per wave and iteration: reg 4 x 32x32x16 (or 8 x 16x16x32) MFMAs; lds one 128 x 32 x 128 tile step
FLOPS_PER_WAVE_ITER = {"reg": 4 * 2 * 32 * 32 * 16, "lds": 2 * 128 * 32 * 128}
ITERS = {"reg": 150000, "lds": 16000}  # ~20 ms a launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.2, help="back-to-back launches before, and while, an arm is timed")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    lib = ctypes.CDLL(os.path.join(HERE, "libmfma_shape.so"))
    lib.probe_mfma.restype = ctypes.c_int
    lib.probe_mfma.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    g = torch.Generator(device=dev).manual_seed(7)
    src = torch.randn(1 << 23, device=dev, generator=g).to(torch.bfloat16)  # 16 MiB = 2^20 uint4, the kernels' index mask
    out = torch.empty(cus * 512, device=dev)
    stamps = torch.zeros(cus * 4, device=dev, dtype=torch.int64)
    stream = torch.cuda.current_stream().cuda_stream

    def launch(kind, shape, n):
        for _ in range(n):
            assert lib.probe_mfma(shape, int(kind == "lds"), src.data_ptr(), cus, ITERS[kind], out.data_ptr(),
                                  stamps.data_ptr(), stream) == 0

    def timed(kind, shape, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(kind, shape, n)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    arms = {}
    for kind in ("reg", "lds"):
        flops = cus * 8 * FLOPS_PER_WAVE_ITER[kind] * ITERS[kind]
        res = {32: {"tflops": [], "clock_ghz": []}, 16: {"tflops": [], "clock_ghz": []}}
        for rnd in range(args.rounds):
            for shape in (32, 16):
                n = max(1, math.ceil(args.seconds * 1e3 * 3 / timed(kind, shape, 3)))
                launch(kind, shape, n)  # untimed, straight into the timed launches
                ms = timed(kind, shape, n)
                st = stamps.view(cus, 4).cpu()
                clk = ((st[:, 2] - st[:, 0]).double() / (st[:, 3] - st[:, 1]).double() * 0.1).tolist()
                res[shape]["tflops"].append(flops * n / (ms * 1e-3) / 1e12)
                res[shape]["clock_ghz"].append(statistics.median(clk))
        t32, t16 = res[32]["tflops"], res[16]["tflops"]
        spread32 = (max(t32) - min(t32)) / statistics.median(t32)
        ratio = [b / a for a, b in zip(t32, t16)]
        arms[kind] = {"iters": ITERS[kind], "32x32x16": res[32], "16x16x32": res[16],
                      "ratio_16_over_32": ratio, "spread_32x32x16": spread32,
                      "faster_16x16x32": min(t16) > max(t32) and statistics.median(ratio) - 1 > spread32}
    rec = {"cus": cus, "seconds": args.seconds, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev),
           "arms": arms}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
