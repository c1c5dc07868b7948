#!/usr/bin/env python
"""Timing of the matrix-free PCA (csrc/pca_backproject.hip,
rmsf_amd.eigen.TrajectoryOps, PCA(solver="matrix_free")) on one MI355X.
Medians of ``--reps`` (7) with min-max, after two warm-ups.

  * ``kernel``: rmsf_pca_backproject alone (no alignment, raw floats) against
    torch's ``(x[:, sel].double().reshape(F, -1) - mean).T @ P`` on the same
    device and data, 16 and 48 columns, at 214 x 20k, 214 of 47,681 x 20k
    (gathered), 3,341 x 4,096 and 100,000 x 256: device events around
    ``--inner`` back-to-back calls, the two candidates alternating.  Beside
    each, the two derived floors: ``hbm_floor_ms`` = 12 n F + 8 F b + 8 3n b
    bytes at the 8 TB/s peak, ``mfma_floor_ms`` = the padded flops 2 (48
    ceil(n / 16)) (32 ceil(F / 32)) (16 ceil(b / 16)) at the measured 77.7
    TFLOP/s of v_mfma_f64_16x16x4_f64.
  * ``solve``: on the planted-mode trajectory of the same shapes,
    align="average": one ``TrajectoryOps.symm`` product of 16 columns (device
    events; the records exist), ``top_eigenpairs`` over it for k = 3 and 10
    (host clock), and ``PCA(...).run()`` end to end, RMSF sweeps included,
    ``solver="matrix_free"`` beside ``solver="device"`` (covariance formation
    included) where the matrix fits.  A solve that does not converge is
    recorded as such, with its iterations.
  * ``headline``: 100,000 atoms x 20,000 frames in HBM (24 GB; the matrix
    would be 720 GB), align=None and align="average", k = 3, end to end.

    python tools/bench_pca_matrix_free.py [--out profiles/pca_matrix_free.json] [--reps 7] [--inner 20]
                                          [--parts kernel,solve,headline]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_events, timed_host  # noqa: E402  (beside this file)

HBM_PEAK_TBS = 8.0
MFMA_F64_TFLOPS = 77.7   # tools/ubench_mfma_f64.hip, profiles/ubench_mfma_f64.txt
# (name, selected atoms, atoms of a frame, frames)
SHAPES = [("214_x_20000", 214, 214, 20_000), ("214_of_47681_x_20000", 214, 47_681, 20_000),
          ("3341_x_4096", 3341, 3341, 4096), ("100000_x_256", 100_000, 100_000, 256)]
REQUIRED = ("214_x_20000", "3341_x_4096")   # the kernel must not be slower than torch's composition here
MATRIX_MAX_ATOMS = 40_000                    # above, 8 (3n)^2 bytes is over half the HBM: no solver="device"


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


def planted(n_atoms, n_frames, seed=0, chunk=512):
    """f32 [F, n_atoms, 3] in HBM: base positions in a 100 A box, three
    collective modes of 2.0, 1.4 and 1.0 A per atom, 0.3 A noise (the recipe
    of tests/test_gpu_pca_project.py without the rigid motion), generated on
    the device ``chunk`` frames at a time."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(1000 * seed + 7 * n_atoms + n_frames)
    kw = {"device": "cuda", "dtype": torch.float64, "generator": g}
    base = 100.0 * torch.rand(n_atoms, 3, **kw)
    modes = torch.randn(3, n_atoms, 3, **kw)
    modes /= torch.sqrt((modes ** 2).sum(dim=(1, 2), keepdim=True) / n_atoms)
    sigma = torch.tensor([2.0, 1.4, 1.0], device="cuda", dtype=torch.float64)
    x = torch.empty(n_frames, n_atoms, 3, device="cuda", dtype=torch.float32)
    for f0 in range(0, n_frames, chunk):
        n = min(chunk, n_frames - f0)
        amp = torch.randn(n, 3, **kw) * sigma
        x[f0:f0 + n] = base + torch.einsum("fk,kac->fac", amp, modes) + 0.3 * torch.randn(n, n_atoms, 3, **kw)
    return x


def selection(n_sel, n_atoms):
    import numpy as np
    return None if n_sel == n_atoms else np.linspace(0, n_atoms - 1, n_sel).astype(np.int64)


def floors(n_sel, n_frames, cols):
    hbm = (12.0 * n_sel * n_frames + 8.0 * n_frames * cols + 8.0 * 3 * n_sel * cols) / (HBM_PEAK_TBS * 1e12) * 1e3
    flops = 2.0 * (48 * -(-n_sel // 16)) * (32 * -(-n_frames // 32)) * (16 * -(-cols // 16))
    return hbm, flops / (MFMA_F64_TFLOPS * 1e12) * 1e3


def bench_kernel(eng, n_sel, n_atoms, n_frames, reps, inner):
    import torch
    g = torch.Generator(device="cuda").manual_seed(n_atoms + n_frames)
    x = 100.0 * torch.rand(n_frames, n_atoms, 3, device="cuda", dtype=torch.float32, generator=g)
    sel = selection(n_sel, n_atoms)
    sel_dev = eng.sel_tensor(sel)
    sel_long = None if sel is None else sel_dev.long()
    rows = x if sel is None else x[:, sel_long]
    mean = rows.double().reshape(n_frames, -1).mean(dim=0).contiguous()
    del rows
    out = {}
    for cols in (16, 48):
        p = torch.randn(n_frames, cols, device="cuda", dtype=torch.float64, generator=g)
        y = eng.empty(3 * n_sel, cols)
        need = eng.pca_backproject_workspace_bytes(n_frames, n_sel, cols)
        work = eng.empty(need // 8) if need else None

        def new():
            eng.pca_backproject(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, None, None, mean, p, cols, y,
                                False, work)

        def composed():
            xs = x if sel_long is None else x[:, sel_long]
            return (xs.double().reshape(n_frames, -1) - mean).T @ p

        new_ms, torch_ms = timed_pair([new, composed], reps, inner)
        nm, tm = statistics.median(new_ms), statistics.median(torch_ms)
        hbm, mfma = floors(n_sel, n_frames, cols)
        ref = composed()
        out[f"cols{cols}"] = {
            "workspace_bytes": need, "new": spread(new_ms), "torch": spread(torch_ms), "new_over_torch": nm / tm,
            "not_slower_than_torch": nm <= tm, "hbm_floor_ms": hbm, "mfma_floor_ms": mfma,
            "hbm_floor_over_new": hbm / nm, "mfma_floor_over_new": mfma / nm,
            "max_abs_diff_vs_torch_rel": float((y - ref).abs().max() / ref.abs().max()),
        }
        del ref
        print("kernel", n_sel, n_atoms, n_frames, cols, json.dumps(out[f"cols{cols}"]), flush=True)
    return out


def timed_run(make, reps):
    """Host-clock ms of ``make().run()``; (spread, last solver_info or None, converged)."""
    state = {}

    def run():
        p = make()
        try:
            p.run()
            state["info"], state["ok"] = p.results.get("solver_info"), True
        except RuntimeError as e:   # PCAConvergenceError
            state["info"], state["ok"] = getattr(e, "info", None), False

    ms = timed_host(run, reps)
    info = state["info"]
    return {"run": spread(ms), "converged": state["ok"], "n_iter": None if info is None else int(info["n_iter"])}


def bench_solve(eng, x, sel, align, ks, reps, with_device, product_cols=16):
    import numpy as np
    import torch

    from rmsf_amd import PCA
    from rmsf_amd.eigen import PCAConvergenceError, TrajectoryOps, top_eigenpairs
    n_frames = int(x.shape[0])
    kw = dict(select=sel, align=align, exact=False)
    out = {}
    p = PCA(x, n_components=ks[0], solver="matrix_free", **kw).run()
    r, last = p.results, p._rmsf._last_run
    ops = TrajectoryOps(last["source"], last["frames"], r.mean, n_frames - 1, masses=last["masses"],
                        aligned=align is not None, exact=last["exact"], ref=last["ref"], refinfo=last["refinfo"],
                        engine=eng)
    q = ops.put(np.random.default_rng(0).standard_normal((ops.n, product_cols)))
    ops.symm(q)   # (the records, the scratch)
    out["symm_product"] = dict(spread(timed_events(lambda: ops.symm(q), reps)), cols=product_cols)
    print("symm", json.dumps(out["symm_product"]), flush=True)
    for k in ks:
        state = {}

        def solve():
            try:
                state["info"] = top_eigenpairs(None, k, ops=ops)[2]
            except PCAConvergenceError as e:
                state["info"] = e.info

        ms = timed_host(solve, reps)
        info = state["info"]
        entry = {"solve": spread(ms), "n_iter": info["n_iter"], "converged": bool(info["converged"]),
                 "block": info["block"], "max_residual": float(np.max(info["residuals"])),
                 "ms_per_iteration": statistics.median(ms) / max(1, info["n_iter"])}
        entry["matrix_free_end_to_end"] = timed_run(
            lambda: PCA(x, n_components=k, solver="matrix_free", **kw), reps)
        if with_device:
            entry["device_end_to_end"] = timed_run(lambda: PCA(x, n_components=k, solver="device", **kw), reps)
            entry["matrix_free_over_device"] = (entry["matrix_free_end_to_end"]["run"]["median_ms"]
                                                / entry["device_end_to_end"]["run"]["median_ms"])
        out[f"k{k}"] = entry
        print("solve", k, json.dumps(entry), flush=True)
    del ops, p
    torch.cuda.empty_cache()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_matrix_free.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--parts", default="kernel,solve,headline", help="comma-separated parts to run")
    a = ap.parse_args(argv)
    parts = set(a.parts.split(","))

    import torch

    from rmsf_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("bench_pca_matrix_free needs a HIP device; nothing is measured without one")
    eng = Engine(torch.device("cuda", 0))
    result = {"device": torch.cuda.get_device_name(0), "hbm_peak_tbs": HBM_PEAK_TBS,
              "mfma_f64_tflops": MFMA_F64_TFLOPS, "inner_calls": a.inner}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    if "kernel" in parts:
        result["kernel"] = {}
        for name, n_sel, n_atoms, n_frames in SHAPES:
            result["kernel"][name] = bench_kernel(eng, n_sel, n_atoms, n_frames, a.reps, a.inner)
            torch.cuda.empty_cache()
            save()
        result["requirement_met"] = all(result["kernel"][s][c]["not_slower_than_torch"]
                                        for s in REQUIRED for c in ("cols16", "cols48"))
    if "solve" in parts:
        result["solve"] = {}
        for name, n_sel, n_atoms, n_frames in SHAPES:
            x = planted(n_atoms, n_frames)
            result["solve"][name] = bench_solve(eng, x, selection(n_sel, n_atoms), "average", (3, 10), a.reps,
                                                with_device=n_sel <= MATRIX_MAX_ATOMS)
            del x
            torch.cuda.empty_cache()
            save()
    if "headline" in parts:
        x = planted(100_000, 20_000)
        result["headline_100000_x_20000"] = {"trajectory_bytes": x.numel() * 4, "matrix_bytes": 8 * 300_000 ** 2}
        for align in (None, "average"):
            result["headline_100000_x_20000"][f"align_{align}"] = bench_solve(eng, x, None, align, (3,), a.reps,
                                                                             with_device=False)
            save()
        del x
    save()
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
