"""Timing helpers shared by tools/bench_covariance.py, tools/bench_pairwise.py
and tools/bench_pca_project.py."""
import statistics
import time


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def timed_events(fn, reps, before=None):
    """Device-event ms of ``reps`` calls of ``fn`` after two warm-up calls;
    ``before`` runs ahead of each call, outside the timed span."""
    import torch
    out = []
    for i in range(reps + 2):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            out.append(a.elapsed_time(b))
    return out


def timed_host(fn, reps):
    """Host-clock ms of ``reps`` synchronised calls of ``fn`` after one warm-up call."""
    import torch
    out = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= 1:
            out.append(1e3 * (time.perf_counter() - t))
    return out
