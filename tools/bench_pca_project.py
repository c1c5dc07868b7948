#!/usr/bin/env python
"""Timing of the PCA projection (csrc/pca_project.hip) on one MI355X.

Per shape (selected atoms x frames, HBM-resident f32 rows) and component
count k, device events on the launching stream around ``--inner`` back-to-back
calls (the kernels run for tens of microseconds; one call would time the
clock), two warm-up repetitions, then ``--reps`` timed ones, the two
candidates alternating; median / min / max per call reported:
  * ``new``: rmsf_pca_project, no alignment (raw floats);
  * ``composed``: what the library allowed before this kernel, on the same
    device and data: ``(x[:, sel].double().reshape(F, -1) - mean) @ V`` in
    torch -- an F x 3n f64 intermediate written and reread;
  * ``hbm_fraction``: the selected atoms' f32 bytes (12 n_sel F) over the
    ``new`` time, against the 8 TB/s HBM peak (a gathered selection moves
    whole cache lines on top of that);
  * ``mfma_tflops``: the f64 MFMA work issued (padding included) over the
    ``new`` time;
  * ``aligned``: ``PCA(align="average").run()`` and its ``transform()`` on the
    same frames, host clock around a device synchronise, median of ``--reps``
    -- where run() is feasible (its [3n, 3n] matrix goes through
    numpy.linalg.eigh on the host, so only at 214 selected atoms).

    python tools/bench_pca_project.py [--out profiles/pca_project.json] [--reps 7] [--inner 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_host  # noqa: E402  (beside this file)

SHAPES = [  # name, atoms per frame, selected atoms, frames, aligned PCA feasible
    ("214_x_20000_dense", 214, 214, 20_000, True),
    ("214_of_47681_x_20000", 47_681, 214, 20_000, True),
    ("3341_x_4096_dense", 3341, 3341, 4096, False),
    ("100000_x_256_splitk", 100_000, 100_000, 256, False),
]
COMPONENTS = (10, 48)
HBM_PEAK_TBS = 8.0


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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_project.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--shapes", default=None, help="comma-separated shape names (default: all)")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from rmsf_amd import PCA
    from rmsf_amd.engine import Engine
    from rmsf_amd.synth import generate, motion_table

    if not torch.cuda.is_available():
        raise SystemExit("bench_pca_project needs a HIP device; nothing is measured without one")
    eng = Engine(torch.device("cuda", 0))
    want = None if a.shapes is None else set(a.shapes.split(","))
    result = {"device": torch.cuda.get_device_name(0), "hbm_peak_tbs": HBM_PEAK_TBS, "inner_calls": a.inner,
              "shapes": {}}
    for name, n_atoms, n_sel, n_frames, pca_ok in SHAPES:
        if want is not None and name not in want:
            continue
        x = generate(eng, n_atoms, 0, n_frames, seed=1, motion=motion_table(2, n_frames))
        sel = None if n_sel == n_atoms else np.arange(n_sel) * (n_atoms // n_sel)
        sel_dev = eng.sel_tensor(sel)
        idx = None if sel is None else torch.as_tensor(sel, device=x.device)
        n = 3 * n_sel
        xs = x if idx is None else x.index_select(1, idx)
        mean = xs.double().mean(dim=0).reshape(-1).contiguous()
        del xs
        entry = {"n_atoms": n_atoms, "n_sel": n_sel, "n_frames": n_frames}
        for k in COMPONENTS:
            g = torch.Generator(device="cpu").manual_seed(k)
            v, _ = torch.linalg.qr(torch.randn(n, k, dtype=torch.float64, generator=g))
            v = v.contiguous().to(x.device)
            need = eng.pca_project_workspace_bytes(n_frames, n_sel, k)
            work = eng.empty(need // 8) if need else None
            out = eng.empty(n_frames, k)

            def new():
                eng.pca_project(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, None, None, mean, v, k, out,
                                work)

            def composed():
                xg = x if idx is None else x.index_select(1, idx)
                return (xg.double().reshape(n_frames, -1) - mean) @ v

            new_ms, comp_ms = timed_pair([new, composed], a.reps, a.inner)
            diff = float((out - composed()).abs().max())
            nm, cm = statistics.median(new_ms), statistics.median(comp_ms)
            n_nt = min(3, -(-k // 16))
            mfma_flop = 2.0 * (-(-n_frames // 16)) * 16 * (-(-k // 48)) * 16 * n_nt * 96 * (-(-n_sel // 32))
            entry[f"k{k}"] = {
                "workspace_bytes": need, "new": spread(new_ms), "composed": spread(comp_ms),
                "new_over_composed": nm / cm, "not_slower_than_composed": nm <= cm,
                "hbm_fraction": 12.0 * n_sel * n_frames / (nm * 1e-3) / (HBM_PEAK_TBS * 1e12),
                "mfma_tflops": mfma_flop / (nm * 1e-3) / 1e12,
                "max_abs_diff_vs_composed_A": diff,
            }
            if pca_ok:
                state = {}

                def run():
                    state["p"] = PCA(x, select=sel, align="average", exact=False, n_components=k).run()

                run_ms = timed_host(run, a.reps)
                tr_ms = timed_host(lambda: state["p"].transform(as_tensor=True), a.reps)
                entry[f"k{k}"]["aligned"] = {"run": spread(run_ms), "transform": spread(tr_ms)}
                del state
            else:
                entry[f"k{k}"]["aligned"] = None
            print(name, k, json.dumps(entry[f"k{k}"]), flush=True)
            del v, out, work
        if not pca_ok:
            entry["aligned_note"] = ("PCA.run() is not timed here: its [3n, 3n] f64 matrix goes through "
                                     "numpy.linalg.eigh on the host (minutes at 10,023^2) or exceeds half the "
                                     "HBM (300,000^2)")
        result["shapes"][name] = entry
        del x, mean
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
