"""What the codec benches (jpegdec_bench.py, pngdec_bench.py, png_bench.py) measure with: HIP-event time of a call, the profiler's
kernel shares, Pillow on 1 and 16 threads, and a stage run with a flag off and on alternately."""
from __future__ import annotations

import io
import re
import statistics
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image


def device_time(fn, reps: int) -> float:
    """Median over `reps` calls of the HIP-event time of one call, in seconds, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    return statistics.median(times)


def kernel_shares(fn, pattern: str):
    """{kernel name: device seconds} of one call for the kernels whose names match `pattern`, from torch's profiler; None where it
    does not see the library's kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            m = re.search(pattern, e.key)
            if m:
                out[m.group(0)] = out.get(m.group(0), 0.0) + getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e6
        return out or None
    except Exception:
        return None


def pillow_decode(data: bytes) -> int:
    return np.asarray(Image.open(io.BytesIO(data))).size


def pillow_times(fn, items) -> dict:
    """{threads: (wall seconds per item of fn, its results)} for 1 thread (over an eighth of `items`, at least 4) and a pool of 16."""
    torch.set_num_threads(1)
    out = {}
    for threads in (1, 16):
        sub = items[:max(4, len(items) // 8)] if threads == 1 else items
        t0 = time.perf_counter()
        if threads == 1:
            got = [fn(x) for x in sub]
        else:
            with ThreadPoolExecutor(max_workers=threads) as pool:
                got = list(pool.map(fn, sub))
        out[threads] = ((time.perf_counter() - t0) / len(sub), got)
    return out


def alternate(run, rounds: int) -> dict:
    """run(flag, round) -> seconds, flag off and on alternately -> {flag: [seconds]}; the first run of each route is a warm-up"""
    times = {False: [], True: []}
    for r in range(rounds + 1):
        for flag in (False, True):
            dt = run(flag, r)
            if r > 0:
                times[flag].append(dt)
    return times
