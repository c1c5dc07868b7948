#!/usr/bin/env python
"""Timing of the all-pairs RMSD matrix (csrc/pairwise.hip) on one MI355X.

Per shape (selected atoms x frames, HBM-resident f32 rows), device events per
repetition after two warm-up repetitions, median / min / max reported:
  * ``new``: rmsf_pairwise_centres + rmsf_pairwise_rmsd (superposition on);
    ``new_plain`` the same without superposition (no Newton epilogue), and
    ``centres`` the first kernel alone;
  * ``composed``: what the library allowed before this kernel, on the same
    device and data: the centred f64 Gram matrix X X^T by ``torch``
    (conversion and centring included), regrouped to [F^2, 9], then
    ``Engine.qcp_batch`` -- every pair twice, rotations included.  Its frames
    are reduced (``composed_frames``) where its 9 F^2 doubles, their regrouped
    copy and the F^2 rotations would not fit in half the free HBM;
  * ``mfma_tflops``: the f64 MFMA rate the contraction achieves (the MFMAs it
    issues over the upper block triangle, padding included, over the ``new``
    time), to hold against tools/ubench_mfma_f64's issue rate (``--mfma-peak``).

    python tools/bench_pairwise.py [--out profiles/pairwise_rmsd.json] [--reps 7] [--mfma-peak 77.7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_events  # noqa: E402  (beside this file)

SHAPES = [  # name, atoms per frame, selected atoms, frames
    ("214_x_4096_dense", 214, 214, 4096),
    ("3341_x_4096_dense", 3341, 3341, 4096),
    ("214_of_47681_x_4096", 47681, 214, 4096),
    ("100000_x_256_splitk", 100_000, 100_000, 256),
]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairwise_rmsd.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mfma-peak", type=float, default=77.7,
                    help="measured f64 MFMA issue rate in TFLOP/s (tools/ubench_mfma_f64)")
    ap.add_argument("--shapes", default=None, help="comma-separated shape names (default: all)")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from rmsf_amd.engine import Engine
    from rmsf_amd.synth import generate, motion_table

    if not torch.cuda.is_available():
        raise SystemExit("bench_pairwise needs a HIP device; nothing is measured without one")
    eng = Engine(torch.device("cuda", 0))
    want = None if a.shapes is None else set(a.shapes.split(","))
    result = {"device": torch.cuda.get_device_name(0), "mfma_peak_tflops": a.mfma_peak, "shapes": {}}
    for name, n_atoms, n_sel, n_frames in SHAPES:
        if want is not None and name not in want:
            continue
        x = generate(eng, n_atoms, 0, n_frames, seed=1, motion=motion_table(2, n_frames))
        sel = None if n_sel == n_atoms else np.arange(n_sel) * (n_atoms // n_sel)
        sel_dev = eng.sel_tensor(sel)
        idx = None if sel is None else torch.as_tensor(sel, device=x.device)
        need = eng.pairwise_workspace_bytes(n_frames, n_sel)
        work = eng.empty(need // 8) if need else None
        out = eng.empty(n_frames, n_frames)
        state = {}

        def centres(per_frame=True):
            state["c"], state["g"] = eng.pairwise_centres(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, None,
                                                          per_frame)

        def new(superpose=True):
            centres(superpose)
            eng.pairwise_rmsd(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, None, float(n_sel), state["c"],
                              state["g"], out, superpose=superpose, cutoff=1e-5, work=work)

        # the composed baseline, on as many frames as fit: 9 F^2 doubles three
        # times over (Gram, regrouped, rotations) and 3 F^2 more (E0, N, rmsd)
        free = torch.cuda.mem_get_info(0)[0]
        fb = n_frames
        while 8 * 30 * fb * fb > free // 2:
            fb //= 2

        def composed():
            xs = x[:fb] if idx is None else x[:fb].index_select(1, idx)
            d = xs.double()
            d = d - d.mean(dim=1, keepdim=True)
            g = (d * d).sum(dim=(1, 2))
            rows = d.permute(0, 2, 1).reshape(3 * fb, n_sel)            # row 3 f + c
            gram = rows @ rows.T
            a9 = gram.view(fb, 3, fb, 3).permute(0, 2, 1, 3).reshape(fb * fb, 9).contiguous()
            e0 = (0.5 * (g[:, None] + g[None, :])).reshape(-1).contiguous()
            cnt = torch.full((fb * fb,), float(n_sel), dtype=torch.float64, device=x.device)
            _, rmsd = eng.qcp_batch(a9, e0, cnt)
            return rmsd.view(fb, fb)

        new_ms = timed_events(new, a.reps)
        m_new = out[:fb, :fb].clone()
        plain_ms = timed_events(lambda: new(False), a.reps)
        cen_ms = timed_events(centres, a.reps)
        comp_ms = timed_events(composed, a.reps)
        m_comp = composed()
        off = ~torch.eye(fb, dtype=torch.bool, device=x.device)
        diff = float((m_new - m_comp)[off].abs().max())
        del m_comp, m_new, off
        torch.cuda.empty_cache()

        n_tiles = -(-n_frames // 16)
        stages = -(-n_sel // 32)
        mfma_flop = 2.0 * (n_tiles * (n_tiles + 1) // 2) * 48 * 48 * 32 * stages
        nm, cm = statistics.median(new_ms), statistics.median(comp_ms)
        entry = {
            "n_atoms": n_atoms, "n_sel": n_sel, "n_frames": n_frames, "workspace_bytes": need,
            "new": spread(new_ms), "new_plain": spread(plain_ms), "centres": spread(cen_ms),
            "composed": spread(comp_ms), "composed_frames": fb,
            "new_over_composed": nm / cm if fb == n_frames else None,
            "mfma_tflops": mfma_flop / (nm * 1e-3) / 1e12,
            "max_abs_diff_vs_composed_A": diff,
        }
        if a.mfma_peak:
            entry["mfma_share_of_peak"] = entry["mfma_tflops"] / a.mfma_peak
        result["shapes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del x, out, work, state
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
