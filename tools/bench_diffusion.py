#!/usr/bin/env python
"""Timing of ``DiffusionMap(solver="device")`` (csrc/diffusion.hip and the block
solver of rmsf_amd/eigen.py over ``KernelOps``) on one MI355X, median of
``--reps`` after a warm-up.

Matrices [F, F]: Euclidean distances of F points in the plane, built on the
device and symmetric in their bits -- 6 planted states with unit normal noise
(tools/bench_cluster.py's, without its outliers); epsilon is the mean squared
distance.

Per shape:
  * ``pass``: rmsf_diffusion_kernel alone, device events, the distances
    restored before each call outside the timed span.  It reads 8 F^2 bytes
    and writes 8 F^2: bytes per second against ``--hbm-peak``, and against
    torch's ``exp(-(d * d) / eps)`` followed by ``sum(1)`` on the same device
    (out of place: it also needs a second matrix).
  * ``run``: ``DiffusionMap(d, eps, n_eigenvectors=3, solver="device").run()``
    with ``d`` an HBM tensor (its copy included), host clock around the call,
    against, on the same matrix,
      - ``host``: today's route, the copy to the host and ``solver="host"``
        (numpy's ``eigh`` of all F pairs);
      - ``torch``: what a user could write on the device -- ``torch.exp``, the
        row sums, the conjugate matrix, ``torch.linalg.eigh``.
    Either baseline is O(F^3) and is taken up to ``--eigh-max`` frames only;
    above, it is recorded as not measured.  A baseline whose first call took t
    seconds is repeated min(reps, budget / t) times in all.
``end_to_end``: ``DiffusionMap(DistanceMatrix(traj), ...)`` at 214 atoms x
4,096 frames, device solver against host solver.

    python tools/bench_diffusion.py [--out profiles/diffusion_map.json] [--reps 7] [--frames 4096,20000]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_events, timed_host  # noqa: E402  (beside this file)

K = 3


def points_matrix(n, device, block=2048):
    """f64 [n, n] in HBM, symmetric in its bits: (a - b)^2 = (b - a)^2 exactly."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(n)
    k = 6
    side = 10.0 * k ** 0.5
    centres = torch.rand((k, 2), generator=g, dtype=torch.float64) * side
    w = 1.0 / (1.0 + torch.arange(k, dtype=torch.float64))
    member = torch.multinomial(w, n, replacement=True, generator=g)
    x = (centres[member] + torch.randn((n, 2), generator=g, dtype=torch.float64)).to(device)
    d = torch.empty((n, n), dtype=torch.float64, device=device)
    for r in range(0, n, block):
        dx = x[r:r + block, None, 0] - x[None, :, 0]
        dy = x[r:r + block, None, 1] - x[None, :, 1]
        d[r:r + block] = torch.sqrt(dx * dx + dy * dy)
    return d


def host_once(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t), out


def torch_route(d, eps):
    import torch
    k = torch.exp(-(d * d) / eps)
    rs = k.sum(1).rsqrt()
    k *= rs[:, None]
    k *= rs[None, :]
    w, v = torch.linalg.eigh(k)
    return w.flip(0)[:K + 1].cpu().numpy(), (v.flip(1)[:, :K + 1] * rs[:, None]).cpu().numpy()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffusion_map.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", default="4096,20000")
    ap.add_argument("--hbm-peak", type=float, default=8.0, help="HBM peak in TB/s")
    ap.add_argument("--eigh-max", type=int, default=8192, help="the O(F^3) baselines are taken up to this many frames")
    ap.add_argument("--baseline-budget-s", type=float, default=25.0,
                    help="a baseline whose first call took t seconds is repeated min(reps, budget / t) times in all")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from rmsf_amd import DiffusionMap, DistanceMatrix
    from rmsf_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("bench_diffusion needs a HIP device; nothing is measured without one")
    dev = torch.device("cuda", 0)
    eng = Engine(dev)
    result = {"device": torch.cuda.get_device_name(0), "hbm_peak_tbs": a.hbm_peak, "reps": a.reps,
              "n_eigenvectors": K, "shapes": {}}

    def repeat(fn, first_ms):
        """first call included: min(reps, budget / t) calls in all, at least one."""
        ms = [first_ms]
        more = min(a.reps, int(a.baseline_budget_s * 1e3 / max(first_ms, 1e-3))) - 1
        for _ in range(max(more, 0)):
            ms.append(host_once(fn)[0])
        return ms

    for n in [int(s) for s in a.frames.split(",") if s]:
        free = torch.cuda.mem_get_info(dev)[0]
        if 8 * n * n * 4 > free:        # the distances, the pass's working copy, torch's K, a row block
            result["shapes"][f"{n}"] = {"skipped": f"four [{n}, {n}] f64 matrices do not fit {free} bytes of free HBM"}
            print(n, "skipped: free HBM", free, flush=True)
            continue
        d = points_matrix(n, dev)
        eps = float((d * d).mean())
        work = torch.empty_like(d)
        pass_ms = timed_events(lambda: eng.diffusion_kernel(work, eps), a.reps, before=lambda: work.copy_(d))
        torch_pass_ms = timed_events(lambda: torch.exp(-(d * d) / eps).sum(1), a.reps)
        del work
        pm = statistics.median(pass_ms)
        entry = {
            "n_frames": n, "epsilon": eps, "matrix_bytes": 8 * n * n,
            "pass": spread(pass_ms), "pass_tbs": 16 * n * n / (pm * 1e-3) / 1e12,
            "pass_hbm_share": 16 * n * n / (pm * 1e-3) / 1e12 / a.hbm_peak,
            "torch_exp_and_sum": spread(torch_pass_ms), "torch_pass_over_pass": statistics.median(torch_pass_ms) / pm,
        }
        state = {}

        def device_run():
            state["dm"] = DiffusionMap(d, eps, n_eigenvectors=K, solver="device").run()

        run_ms = timed_host(device_run, a.reps)
        r = state["dm"].results
        rm = statistics.median(run_ms)
        entry.update({"run": spread(run_ms), "n_iter": int(r.solver_info["n_iter"]),
                      "eigenvalues": [float(x) for x in r.eigenvalues],
                      "worst_residual": float(r.solver_info["residuals"].max())})
        if n <= a.eigh_max:
            def host_route():
                return DiffusionMap(d.cpu().numpy(), eps).run().results

            first, hr = host_once(host_route)
            ms = repeat(host_route, first)
            entry["host_with_d2h"] = spread(ms)
            entry["host_over_device"] = statistics.median(ms) / rm
            entry["host_max_dlambda"] = float(np.abs(hr.eigenvalues[:K + 1] - r.eigenvalues).max())
            del hr
            host_once(lambda: torch_route(d, eps))                       # warm-up: not kept
            first, (tw, _) = host_once(lambda: torch_route(d, eps))
            ms = repeat(lambda: torch_route(d, eps), first)
            entry["torch_eigh"] = spread(ms)
            entry["torch_over_device"] = statistics.median(ms) / rm
            entry["torch_max_dlambda"] = float(np.abs(tw - r.eigenvalues).max())
        else:
            entry["host_with_d2h"] = entry["torch_eigh"] = None
            entry["baselines"] = f"not measured: eigh of all {n} pairs is O(F^3), --eigh-max is {a.eigh_max}"
        result["shapes"][f"{n}"] = entry
        print(n, json.dumps(entry), flush=True)
        del d, state
        torch.cuda.empty_cache()

    # end to end: 214 atoms x 4,096 frames, 8 states of 2 A displacement, 0.3 A noise (tools/bench_cluster.py's)
    n_atoms, n_frames = 214, 4096
    g = torch.Generator(device="cpu").manual_seed(214)
    base = torch.rand((n_atoms, 3), generator=g) * 100.0
    disp = torch.randn((8, n_atoms, 3), generator=g)
    disp /= (disp ** 2).sum(dim=(1, 2), keepdim=True).div(n_atoms).sqrt()
    member = torch.multinomial(1.0 / (1.0 + torch.arange(8.0)), n_frames, replacement=True, generator=g)
    traj = (base + 2.0 * disp[member] + 0.3 * torch.randn((n_frames, n_atoms, 3), generator=g)).to(dev)
    dist = DistanceMatrix(traj).run().results.dist_matrix
    eps = float(np.median(dist * dist))
    del dist
    state = {}

    def new():
        state["new"] = DiffusionMap(DistanceMatrix(traj), eps, n_eigenvectors=K, solver="device").run().results

    def old():
        return DiffusionMap(DistanceMatrix(traj), eps).run().results

    new_ms = timed_host(new, a.reps)
    first, o = host_once(old)
    old_ms = repeat(old, first)
    r = state["new"]
    result["end_to_end"] = {
        "n_atoms": n_atoms, "n_frames": n_frames, "epsilon": eps, "n_iter": int(r.solver_info["n_iter"]),
        "eigenvalues": [float(x) for x in r.eigenvalues],
        "device_solver_run": spread(new_ms), "host_solver_run": spread(old_ms),
        "max_dlambda": float(np.abs(o.eigenvalues[:K + 1] - r.eigenvalues).max()),
        "host_over_device": statistics.median(old_ms) / statistics.median(new_ms),
    }
    print("end_to_end", json.dumps(result["end_to_end"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
