#!/usr/bin/env python
"""Timing of the positional covariance (csrc/covariance.hip) on one MI355X.

Per shape (selected atoms x frames, HBM-resident f32 rows):
  * ``kernel``: rmsf_covariance_accumulate + rmsf_covariance_finish alone
    (align=None, shift = frame 0), device events per repetition;
  * ``torch``: the same contraction as a user would write it on the same
    device, conversion included: ``d = x.double() - s; d.T @ d``;
  * ``run``: the whole ``align="average"`` pipeline with and without
    ``covariance=True`` (host clock around a synchronised run).
Rates count F (3n)^2 multiply-adds (2 FLOP each) of the full matrix; the
kernel issues MFMAs for the upper block triangle only (``mfma_tflops`` is
what the matrix cores actually run, the figure to hold against
tools/ubench_mfma_f64's issue rate, ``--mfma-peak``).

    python tools/bench_covariance.py [--out profiles/covariance.json] [--reps 7] [--mfma-peak TFLOPS]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_events, timed_host  # noqa: E402  (beside this file)

SHAPES = [  # name, atoms per frame, selected atoms, frames
    ("214_of_47681_x_20000", 47681, 214, 20000),
    ("214_x_20000_dense", 214, 214, 20000),
    ("3341_x_4000_dense", 3341, 3341, 4000),
]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mfma-peak", type=float, default=None,
                    help="measured f64 MFMA issue rate in TFLOP/s (tools/ubench_mfma_f64)")
    ap.add_argument("--shapes", default=None, help="comma-separated shape names (default: all)")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from rmsf_amd.engine import Engine
    from rmsf_amd.pipeline import run_pipeline
    from rmsf_amd.sources import DeviceSource, FrameList
    from rmsf_amd.synth import generate, motion_table

    if not torch.cuda.is_available():
        raise SystemExit("bench_covariance needs a HIP device; nothing is measured without one")
    eng = Engine(torch.device("cuda", 0))
    want = None if a.shapes is None else set(a.shapes.split(","))
    result = {"device": torch.cuda.get_device_name(0), "mfma_peak_tflops": a.mfma_peak, "shapes": {}}
    for name, n_atoms, n_sel, n_frames in SHAPES:
        if want is not None and name not in want:
            continue
        x = generate(eng, n_atoms, 0, n_frames, seed=1, motion=motion_table(2, n_frames))
        sel = None if n_sel == n_atoms else np.arange(n_sel) * (n_atoms // n_sel)
        sel_dev = eng.sel_tensor(sel)
        n = 3 * n_sel
        rows = x[0] if sel is None else x[0][torch.as_tensor(sel, device=x.device)]
        shift = rows.reshape(-1).double()
        cov, t1 = eng.zeros(n, n), eng.zeros(n)
        need = eng.covariance_workspace_bytes(n_sel, n_frames)
        work = eng.empty(need // 8) if need else None

        def kernel():
            eng.covariance_accumulate(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, None, None, shift, cov,
                                      t1, work)
            eng.covariance_finish(cov, t1, n, n_frames)

        def zero():
            cov.zero_()
            t1.zero_()

        idx = None if sel is None else torch.as_tensor(sel, device=x.device)

        def baseline():
            xs = x if idx is None else x.index_select(1, idx)
            d = xs.reshape(n_frames, n).double() - shift
            return d.T @ d

        k_ms = timed_events(kernel, a.reps, zero)
        m_kernel = cov.clone()
        t_ms = timed_events(baseline, a.reps)
        # same sums: the baseline's, centred as the finish centres the kernel's
        xs = x if idx is None else x.index_select(1, idx)
        s1 = (xs.reshape(n_frames, n).double() - shift).sum(0)
        m_torch = baseline() - torch.outer(s1, s1) / n_frames
        err = float((m_kernel - m_torch).abs().max() / m_torch.diagonal().max())
        del m_torch, xs

        src = DeviceSource(x, sel)
        fl = FrameList(n_frames)
        off_ms = timed_host(lambda: run_pipeline(eng, src, fl, align="average"), max(3, a.reps // 2))
        on_ms = timed_host(lambda: run_pipeline(eng, src, fl, align="average", covariance=True),
                           max(3, a.reps // 2))

        n_tiles = -(-n_sel // 16)
        madd = n_frames * n * n
        stages = -(-n_frames // 32)
        mfma_flop = 2.0 * (n_tiles * (n_tiles + 1) // 2) * 48 * 48 * 32 * stages
        km = statistics.median(k_ms)
        entry = {
            "n_atoms": n_atoms, "n_sel": n_sel, "n_frames": n_frames, "workspace_bytes": need,
            "kernel": spread(k_ms), "torch": spread(t_ms),
            "kernel_tflops": 2.0 * madd / (km * 1e-3) / 1e12,
            "torch_tflops": 2.0 * madd / (statistics.median(t_ms) * 1e-3) / 1e12,
            "mfma_tflops": mfma_flop / (km * 1e-3) / 1e12,
            "kernel_over_torch": km / statistics.median(t_ms),
            "max_rel_diff_vs_torch": err,
            "run_average": spread(off_ms), "run_average_covariance": spread(on_ms),
        }
        if a.mfma_peak:
            entry["mfma_share_of_peak"] = entry["mfma_tflops"] / a.mfma_peak
        result["shapes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del x, cov, t1, work, m_kernel, src
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
