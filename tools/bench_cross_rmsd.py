#!/usr/bin/env python
"""Timing of the cross RMSD matrix d[i, j] = RMSD(A_i, B_j) (csrc/pairwise.hip,
k_pw_tiles over the tile rectangle) on one MI355X.

Per shape (frames of A x frames of B x selected atoms, HBM-resident f32 rows),
device events per repetition after two warm-up repetitions, median / min / max
reported; the two paths alternate repetition by repetition within one call:
  * ``new``: rmsf_pairwise_centres of either side + rmsf_cross_rmsd
    (superposition on); ``row_argmin`` is timed on its own;
  * ``baseline``: what the library allowed before this kernel, on the same
    device and data: ``DistanceMatrix``'s engine path (rmsf_pairwise_centres +
    rmsf_pairwise_rmsd) on the F_a + F_b frames of both inputs in one tensor
    (concatenated outside the timed span), then the [:F_a, F_a:] block copied
    out;
  * ``mfma_tflops``: the f64 MFMA rate the contraction achieves (the MFMAs it
    issues over the tile rectangle, padding included, over the ``new`` time), to
    hold against tools/ubench_mfma_f64's issue rate (``--mfma-peak``);
  * ``hbm_share``: the bytes that must move at least once -- the selected rows
    of both sides (whole 64-byte lines of a gathered atom) and the matrix --
    over the ``new`` time, against ``--hbm-peak``.

    python tools/bench_cross_rmsd.py [--out profiles/cross_rmsd.json] [--reps 7] [--mfma-peak 77.7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_events  # noqa: E402  (beside this file)

SHAPES = [  # name, frames of A, frames of B, atoms per frame, selected atoms
    ("20000_x_64_x_214", 20_000, 64, 214, 214),
    ("4096_x_4096_x_214", 4096, 4096, 214, 214),
    ("4096_x_256_x_3341", 4096, 256, 3341, 3341),
    ("4096_x_64_x_214_of_47681", 4096, 64, 47681, 214),
    ("256_x_16_x_100000_splitk", 256, 16, 100_000, 100_000),
]


def alternate(fns, reps):
    """Device-event ms of each of ``fns``, called in turn ``reps`` times after
    two warm-up rounds."""
    import torch
    out = [[] for _ in fns]
    for i in range(reps + 2):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                out[k].append(a.elapsed_time(b))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_rmsd.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mfma-peak", type=float, default=77.7,
                    help="measured f64 MFMA issue rate in TFLOP/s (tools/ubench_mfma_f64)")
    ap.add_argument("--hbm-peak", type=float, default=8.0, help="HBM peak in TB/s")
    ap.add_argument("--shapes", default=None, help="comma-separated shape names (default: all)")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from rmsf_amd.engine import Engine
    from rmsf_amd.synth import generate, motion_table

    if not torch.cuda.is_available():
        raise SystemExit("bench_cross_rmsd needs a HIP device; nothing is measured without one")
    eng = Engine(torch.device("cuda", 0))
    want = None if a.shapes is None else set(a.shapes.split(","))
    result = {"device": torch.cuda.get_device_name(0), "mfma_peak_tflops": a.mfma_peak,
              "hbm_peak_tbs": a.hbm_peak, "shapes": {}}
    for name, f_a, f_b, n_atoms, n_sel in SHAPES:
        if want is not None and name not in want:
            continue
        n_cat = f_a + f_b
        cat = generate(eng, n_atoms, 0, n_cat, seed=1, motion=motion_table(2, n_cat))
        xa, xb = cat[:f_a], cat[f_a:]           # the two inputs: views of the concatenation
        sel = None if n_sel == n_atoms else np.arange(n_sel) * (n_atoms // n_sel)
        sel_dev = eng.sel_tensor(sel)
        need = eng.cross_workspace_bytes(f_a, f_b, n_sel)
        work = eng.empty(need // 8) if need else None
        out = eng.empty(f_a, f_b)
        base_need = eng.pairwise_workspace_bytes(n_cat, n_sel)
        base_work = eng.empty(base_need // 8) if base_need else None
        base_out = eng.empty(n_cat, n_cat)
        block = eng.empty(f_a, f_b)

        def new():
            ca, ga = eng.pairwise_centres(xa.data_ptr(), xa.stride(0), f_a, n_sel, sel_dev, None, True)
            cb, gb = eng.pairwise_centres(xb.data_ptr(), xb.stride(0), f_b, n_sel, sel_dev, None, True)
            eng.cross_rmsd(xa.data_ptr(), xa.stride(0), f_a, sel_dev, ca, ga, xb.data_ptr(), xb.stride(0), f_b,
                           sel_dev, cb, gb, n_sel, None, float(n_sel), out, superpose=True, cutoff=1e-5, work=work)

        def baseline():
            c, g = eng.pairwise_centres(cat.data_ptr(), cat.stride(0), n_cat, n_sel, sel_dev, None, True)
            eng.pairwise_rmsd(cat.data_ptr(), cat.stride(0), n_cat, n_sel, sel_dev, None, float(n_sel), c, g,
                              base_out, superpose=True, cutoff=1e-5, work=base_work)
            block.copy_(base_out[:f_a, f_a:])

        new_ms, base_ms = alternate((new, baseline), a.reps)
        diff = float((out - block).abs().max())
        argmin_ms = timed_events(lambda: eng.row_argmin(out), a.reps)

        tiles = -(-f_a // 16) * -(-f_b // 16)
        stages = -(-n_sel // 32)
        mfma_flop = 2.0 * tiles * 48 * 48 * 32 * stages
        atom_bytes = 12 if sel is None else 64
        must_move = atom_bytes * n_sel * n_cat + 8 * f_a * f_b
        nm, bm = statistics.median(new_ms), statistics.median(base_ms)
        entry = {
            "n_frames_a": f_a, "n_frames_b": f_b, "n_atoms": n_atoms, "n_sel": n_sel, "workspace_bytes": need,
            "pairs_new": f_a * f_b, "pairs_baseline": n_cat * (n_cat - 1) // 2,
            "new": spread(new_ms), "baseline": spread(base_ms), "row_argmin": spread(argmin_ms),
            "new_over_baseline": nm / bm,
            "mfma_tflops": mfma_flop / (nm * 1e-3) / 1e12,
            "must_move_bytes": must_move, "hbm_tbs": must_move / (nm * 1e-3) / 1e12,
            "max_abs_diff_vs_baseline_A": diff,
        }
        if a.mfma_peak:
            entry["mfma_share_of_peak"] = entry["mfma_tflops"] / a.mfma_peak
        if a.hbm_peak:
            entry["hbm_share"] = entry["hbm_tbs"] / a.hbm_peak
        result["shapes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del cat, xa, xb, out, work, base_out, base_work, block
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
