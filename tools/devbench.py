"""What the bench_*_device.py tools share: timing one enqueue, alternating the variants of a comparison, a percentile, and the
two generators of entry lengths. The tools reduce the raw per-run lists themselves (medians, p10 / p90) and print their own JSON."""
import time

import numpy as np
import torch


def once(fn, stream, timing="both"):
    """One fn() on `stream`, timed. timing="both": the stream is drained first -> (wall ms from the first enqueue to the end of
    the stream, hipEvent ms); "wall": the same wall ms alone, ended by a stream synchronise, no events on the stream; "event":
    hipEvent ms alone, the stream not drained first (back-to-back runs, as a caller's pipeline issues them)."""
    if timing == "wall":
        stream.synchronize()
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if timing == "both":
        stream.synchronize()
        t0 = time.perf_counter()
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return ((time.perf_counter() - t0) * 1e3, a.elapsed_time(b)) if timing == "both" else a.elapsed_time(b)


def alternating(fns, runs, warmup, stream, timing="both"):
    """-> per function the list of what once() gave per run; run i times every function once, in turn"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    stream.synchronize()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            ms[k].append(once(fn, stream, timing))
    return ms


def pct(sorted_vals, p):
    return sorted_vals[min(len(sorted_vals) - 1, max(0, round(p * (len(sorted_vals) - 1))))]


def _scaled(raw, total):
    lens = np.maximum(1, np.floor(raw * (total / raw.sum()))).astype(np.int64)
    lens[np.argmax(lens)] += total - int(lens.sum())
    assert lens.min() >= 1 and int(lens.sum()) == total
    return [int(x) for x in lens]


def lengths_log(n, total, seed):
    """n lengths, log-uniform from 4 bytes to 64 MiB, scaled to add up to total"""
    rng = np.random.default_rng(seed)
    return _scaled(np.exp(rng.uniform(np.log(4.0), np.log(64.0 * (1 << 20)), n)), total)


def lengths_uniform(n, total, seed):
    """n lengths, uniform within +-50 % of total / n, adding up to total"""
    rng = np.random.default_rng(seed)
    return _scaled(rng.uniform(0.5, 1.5, n), total)
