"""HIP-event timing of the ``*_time.py`` tools: ms of one call; median / min / max of
``reps`` calls after ``warmup`` untimed ones."""
import statistics

import torch


def event_ms(fn, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1)


def timed(fn, dev, reps, warmup):
    ms = [event_ms(fn, dev) for _ in range(warmup + reps)][warmup:]
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}
