#!/usr/bin/env python
"""Timing of the device eigen-solver (csrc/eigen_block.hip, rmsf_amd/eigen.py)
on one MI355X.  Medians of ``--reps`` (7), after warm-up; run it twice for the
second figure of a pair.

  * ``symm``: rmsf_symm_block (Y = M Q) against torch's f64 ``M @ Q`` on the
    same device and data, at 642^2 and 10,023^2 with 16, 32 and 48 columns:
    device events around ``--inner`` back-to-back calls, the two candidates
    alternating.  Beside each, the two derived floors: ``hbm_floor_ms`` = 8 n^2
    bytes at the 8 TB/s peak, ``mfma_floor_ms`` = 2 n_pad^2 16 NT flops at the
    measured 77.7 TFLOP/s of v_mfma_f64_16x16x4_f64.
  * ``solve``: top_eigenpairs (host clock around a synchronised call) on the
    covariance of a planted-mode trajectory (three collective modes over 0.3 A
    noise: k = 3 sits in front of a wide gap, k = 10 and 40 in the flat noise
    bulk) at 214 x 20k and 3,341 x 4,096 frames, and on a designed power-law
    spectrum 100 (1 + i)^-2 of the same sizes, k = 10 and 40.  Against
    ``numpy.linalg.eigh`` of the host matrix, its device-to-host copy
    included; at 10,023^2 the host is timed once (``--host-large``: minutes).
    A solve that does not converge is recorded as such, with its iterations.
    ``residual_floor``: the largest of the k = 10 residuals of the power-law
    matrix 20 iterations past convergence (tol = 0), beside n 2^-53.
  * ``run``: ``PCA(align="average").run()`` at 214 x 20k, ``solver="host"``
    (the path before the device solver) against ``"device"``, host clock.

    python tools/bench_pca_eig.py [--out profiles/pca_eig.json] [--reps 7] [--inner 20] [--host-large]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_host  # noqa: E402  (beside this file)

HBM_PEAK_TBS = 8.0
MFMA_F64_TFLOPS = 77.7   # tools/ubench_mfma_f64.hip, profiles/ubench_mfma_f64.txt
SIZES = [("214_x_20000", 214, 20_000), ("3341_x_4096", 3341, 4096)]


def timed_pair(fns, reps, inner):
    """Per-call ms of each of ``fns``, alternating, after two warm-up rounds."""
    import torch
    out = [[] for _ in fns]
    for i in range(reps + 2):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                out[j].append(a.elapsed_time(b) / inner)
    return out


def planted(n_atoms, n_frames, seed=0):
    """f32 [F, n_atoms, 3] in HBM: base positions in a 100 A box, three
    collective modes of 2.0, 1.4 and 1.0 A per atom, 0.3 A noise (the recipe
    of tests/test_gpu_pca_eig.py without the rigid motion, generated on the
    device)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(1000 * seed + 7 * n_atoms + n_frames)
    kw = {"device": "cuda", "dtype": torch.float64, "generator": g}
    base = 100.0 * torch.rand(n_atoms, 3, **kw)
    modes = torch.randn(3, n_atoms, 3, **kw)
    modes /= torch.sqrt((modes ** 2).sum(dim=(1, 2), keepdim=True) / n_atoms)
    amp = torch.randn(n_frames, 3, **kw) * torch.tensor([2.0, 1.4, 1.0], device="cuda", dtype=torch.float64)
    x = base + torch.einsum("fk,kac->fac", amp, modes) + 0.3 * torch.randn(n_frames, n_atoms, 3, **kw)
    return x.float().contiguous()


def power_law_matrix(n, seed=1):
    """U diag(100 (1 + i)^-2) U^T in HBM, symmetric in its bits."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    u, _ = torch.linalg.qr(torch.randn(n, n, device="cuda", dtype=torch.float64, generator=g))
    lam = 100.0 * (1.0 + torch.arange(n, device="cuda", dtype=torch.float64)) ** -2.0
    m = (u * lam[None, :]) @ u.T
    del u
    return (0.5 * (m + m.T)).contiguous()


def bench_symm(eng, n, reps, inner):
    import torch
    g = torch.Generator(device="cuda").manual_seed(n)
    m = torch.randn(n, n, device="cuda", dtype=torch.float64, generator=g)
    m = (m + m.T).contiguous()
    out = {}
    for cols in (16, 32, 48):
        q = torch.randn(n, cols, device="cuda", dtype=torch.float64, generator=g)
        y = eng.empty(n, cols)
        need = eng.symm_block_workspace_bytes(n, cols)
        work = eng.empty(need // 8) if need else None
        new_ms, torch_ms = timed_pair([lambda: eng.symm_block(m, n, q, cols, y, work), lambda: m @ q], reps, inner)
        nm, tm = statistics.median(new_ms), statistics.median(torch_ms)
        n_pad = 48 * (-(-n // 48))
        ref = m @ q
        out[f"cols{cols}"] = {
            "workspace_bytes": need, "new": spread(new_ms), "torch": spread(torch_ms), "new_over_torch": nm / tm,
            "not_slower_than_torch": nm <= tm,
            "hbm_floor_ms": 8.0 * n * n / (HBM_PEAK_TBS * 1e12) * 1e3,
            "mfma_floor_ms": 2.0 * n_pad * n_pad * 16 * (cols // 16) / (MFMA_F64_TFLOPS * 1e12) * 1e3,
            "hbm_tbs": 8.0 * n * n / (nm * 1e-3) / 1e12,
            "max_abs_diff_vs_torch_rel": float((y - ref).abs().max() / ref.abs().max()),
        }
        print("symm", n, cols, json.dumps(out[f"cols{cols}"]), flush=True)
    return out


def bench_solve(matrix, ks, reps, host_reps, floor_k=0):
    """top_eigenpairs per k, and numpy.linalg.eigh of the host copy (``host_reps`` = 0: not timed)."""
    import numpy as np
    import torch

    from rmsf_amd.eigen import PCAConvergenceError, top_eigenpairs
    out = {"n": int(matrix.shape[0])}
    for k in ks:
        state = {}

        def solve():
            try:
                state["info"] = top_eigenpairs(matrix, k)[2]
            except PCAConvergenceError as e:
                state["info"] = e.info

        ms = timed_host(solve, reps)
        info = state["info"]
        out[f"k{k}"] = {"solve": spread(ms), "n_iter": info["n_iter"], "converged": bool(info["converged"]),
                        "block": info["block"], "rank": info["rank"],
                        "max_residual": float(np.max(info["residuals"])),
                        "ms_per_iteration": statistics.median(ms) / max(1, info["n_iter"])}
        print("solve", out["n"], k, json.dumps(out[f"k{k}"]), flush=True)
    if floor_k:
        # the f64 floor of the residual: iterate well past convergence with a tolerance nothing meets
        n_iter = out[f"k{floor_k}"]["n_iter"]
        try:
            top_eigenpairs(matrix, floor_k, tol=0.0, max_iter=n_iter + 20)
        except PCAConvergenceError as e:
            out["residual_floor"] = {"k": floor_k, "n_iter": e.info["n_iter"],
                                     "max_residual": float(np.max(e.info["residuals"])),
                                     "n_2^-53": out["n"] * 2.0 ** -53}
            print("floor", out["n"], json.dumps(out["residual_floor"]), flush=True)
    if host_reps:
        print(f"host eigh of {out['n']}^2, {host_reps} time(s) ...", flush=True)
        ms = []
        for _ in range(host_reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            np.linalg.eigh(matrix.cpu().numpy())
            ms.append(1e3 * (time.perf_counter() - t))
        out["host_eigh_with_d2h"] = spread(ms)
        for k in ks:
            out[f"k{k}"]["device_over_host"] = out[f"k{k}"]["solve"]["median_ms"] / statistics.median(ms)
        print("host", out["n"], json.dumps(out["host_eigh_with_d2h"]), flush=True)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_eig.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--host-large", action="store_true", help="also time numpy.linalg.eigh at 10,023^2, once (minutes)")
    ap.add_argument("--parts", default="symm,solve,run", help="comma-separated parts to run")
    a = ap.parse_args(argv)
    parts = set(a.parts.split(","))

    import torch

    from rmsf_amd import PCA
    from rmsf_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("bench_pca_eig needs a HIP device; nothing is measured without one")
    eng = Engine(torch.device("cuda", 0))
    result = {"device": torch.cuda.get_device_name(0), "hbm_peak_tbs": HBM_PEAK_TBS,
              "mfma_f64_tflops": MFMA_F64_TFLOPS, "inner_calls": a.inner}
    if "symm" in parts:
        result["symm"] = {f"n{n}": bench_symm(eng, n, a.reps, a.inner) for n in (642, 10_023)}
        torch.cuda.empty_cache()
    if "solve" in parts:
        result["solve"] = {}
        for name, n_atoms, n_frames in SIZES:
            small = n_atoms == 214
            host_reps = a.reps if small else (1 if a.host_large else 0)
            p = PCA(planted(n_atoms, n_frames), align="average", exact=False, solver="device", n_components=3).run()
            result["solve"][f"planted_{name}"] = bench_solve(p.results.covariance, (3, 10, 40), a.reps, host_reps)
            del p
            torch.cuda.empty_cache()
            result["solve"][f"power_law_{3 * n_atoms}"] = bench_solve(power_law_matrix(3 * n_atoms), (10, 40), a.reps,
                                                                     a.reps if small else 0, floor_k=10)
            torch.cuda.empty_cache()
    if "run" in parts:
        x = planted(214, 20_000)
        result["run_214_x_20000"] = {}
        for k in (3, 10):
            entry = {}
            for solver in ("host", "device"):
                def run():
                    try:
                        PCA(x, align="average", exact=False, solver=solver, n_components=k).run()
                        entry[f"{solver}_converged"] = True
                    except RuntimeError:
                        entry[f"{solver}_converged"] = False
                entry[solver] = spread(timed_host(run, a.reps))
            entry["device_over_host"] = entry["device"]["median_ms"] / entry["host"]["median_ms"]
            result["run_214_x_20000"][f"k{k}"] = entry
            print("run", k, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
