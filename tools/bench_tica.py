#!/usr/bin/env python
"""Timing of the time-lagged co-moment (csrc/covariance.hip, the LAGGED
instantiation of its tile body) and of TICA on one MI355X.

Per shape (selected atoms x frames, HBM-resident f32 rows, lag 10):
  * ``kernel``: rmsf_lagged_comoment_accumulate + rmsf_lagged_comoment_finish
    alone (align=None, shift = frame 0), device events per repetition;
  * ``torch``: the same contraction as a user would write it on the same
    device, its f64 copy of the frames included: ``d = x.double() - s;
    d[:N].T @ d[lag:]``;
  * ``covariance``: the unchanged rmsf_covariance_accumulate +
    rmsf_covariance_finish over the same N frames -- the triangle against the
    lagged kernel's full square.
Rates count N (3n)^2 multiply-adds (2 FLOP each); ``mfma_tflops`` is what the
matrix cores run, whole 48 x 48 tiles of the full square over whole stages of
32 pairs, the figure to hold against the measured f64 MFMA issue rate
(``--mfma-peak``, default 77.7 TFLOP/s).  ``run``: ``TICA(...).run()`` end to
end at 214 x 20,000 against ``PCA(solver="host")`` (host clock, both with
their host eigen-solve).

    python tools/bench_tica.py [--out profiles/tica.json] [--reps 7] [--mfma-peak TFLOPS]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_events, timed_host  # noqa: E402  (beside this file)

LAG = 10
SHAPES = [  # name, atoms per frame, selected atoms, frames
    ("214_x_20000_dense", 214, 214, 20000),
    ("214_of_47681_x_20000", 47681, 214, 20000),
    ("3341_x_4096_dense", 3341, 3341, 4096),
]
RUN_SHAPE = "214_x_20000_dense"


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tica.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mfma-peak", type=float, default=77.7,
                    help="measured f64 MFMA issue rate in TFLOP/s (tools/ubench_mfma_f64)")
    ap.add_argument("--shapes", default=None, help="comma-separated shape names (default: all)")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from rmsf_amd import PCA, TICA
    from rmsf_amd.engine import Engine
    from rmsf_amd.synth import generate, motion_table

    if not torch.cuda.is_available():
        raise SystemExit("bench_tica needs a HIP device; nothing is measured without one")
    eng = Engine(torch.device("cuda", 0))
    want = None if a.shapes is None else set(a.shapes.split(","))
    result = {"device": torch.cuda.get_device_name(0), "mfma_peak_tflops": a.mfma_peak, "lag": LAG, "shapes": {}}
    for name, n_atoms, n_sel, n_frames in SHAPES:
        if want is not None and name not in want:
            continue
        x = generate(eng, n_atoms, 0, n_frames, seed=1, motion=motion_table(2, n_frames))
        sel = None if n_sel == n_atoms else np.arange(n_sel) * (n_atoms // n_sel)
        sel_dev = eng.sel_tensor(sel)
        n, n_pairs = 3 * n_sel, n_frames - LAG
        idx = None if sel is None else torch.as_tensor(sel, device=x.device)
        rows = x[0] if idx is None else x[0][idx]
        shift = rows.reshape(-1).double()
        s, cov, t = eng.zeros(n, n), eng.zeros(n, n), eng.zeros(n)
        need = eng.lagged_comoment_workspace_bytes(n_sel, n_pairs)
        need_cov = eng.covariance_workspace_bytes(n_sel, n_pairs)
        work = eng.empty(max(need, need_cov) // 8) if max(need, need_cov) else None
        b_ptr = x.data_ptr() + 4 * LAG * x.stride(0)

        def kernel():
            eng.lagged_comoment_accumulate(x.data_ptr(), x.stride(0), b_ptr, x.stride(0), n_pairs, n_sel, sel_dev,
                                           None, None, None, shift, s, work)
            eng.lagged_comoment_finish(s, t, n, 2 * n_pairs)

        def covariance():
            eng.covariance_accumulate(x.data_ptr(), x.stride(0), n_pairs, n_sel, sel_dev, None, None, shift, cov, t,
                                      work)
            eng.covariance_finish(cov, t, n, n_pairs)

        def zero():
            s.zero_()
            cov.zero_()
            t.zero_()

        def baseline():
            xs = x if idx is None else x.index_select(1, idx)
            d = xs.reshape(n_frames, n).double() - shift
            return d[:n_pairs].T @ d[LAG:]

        k_ms = timed_events(kernel, a.reps, zero)
        m_kernel = s.clone()                      # t = 0: S + S^T
        c_ms = timed_events(covariance, a.reps, zero)
        t_ms = timed_events(baseline, a.reps)
        m_torch = baseline()
        m_torch = m_torch + m_torch.T
        err = float((m_kernel - m_torch).abs().max() / m_torch.abs().max())
        del m_torch, m_kernel

        n_tiles = -(-n_sel // 16)
        madd = n_pairs * n * n
        stages = -(-n_pairs // 32)
        mfma_flop = 2.0 * n_tiles * n_tiles * 48 * 48 * 32 * stages
        km, cm, tm = statistics.median(k_ms), statistics.median(c_ms), statistics.median(t_ms)
        entry = {
            "n_atoms": n_atoms, "n_sel": n_sel, "n_frames": n_frames, "n_pairs": n_pairs, "workspace_bytes": need,
            "kernel": spread(k_ms), "torch": spread(t_ms), "covariance": spread(c_ms),
            "kernel_tflops": 2.0 * madd / (km * 1e-3) / 1e12,
            "torch_tflops": 2.0 * madd / (tm * 1e-3) / 1e12,
            "mfma_tflops": mfma_flop / (km * 1e-3) / 1e12,
            "kernel_over_torch": km / tm,
            "kernel_over_covariance": km / cm,
            "max_rel_diff_vs_torch": err,
        }
        if a.mfma_peak:
            entry["mfma_share_of_peak"] = entry["mfma_tflops"] / a.mfma_peak
        if name == RUN_SHAPE:
            reps = max(3, a.reps // 2)
            entry["run_tica"] = spread(timed_host(lambda: TICA(x, LAG, select=sel, align="average").run(), reps))
            entry["run_pca_host"] = spread(timed_host(lambda: PCA(x, select=sel, align="average").run(), reps))
        result["shapes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del x, s, cov, t, work
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
