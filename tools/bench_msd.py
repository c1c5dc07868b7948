#!/usr/bin/env python
"""Timing of the mean squared displacement kernels (csrc/msd.hip) on one MI355X.

Per shape (atoms x frames, HBM-resident f32 rows of a random walk wrapped into a
cubic box, every atom followed, msd_type xyz), free and with the box (nojump):
  * ``planes``: rmsf_msd_planes alone -- the widening, the unwrap chain and the
    transpose into atom-major f64 planes;
  * ``lags``: rmsf_msd_lags alone -- the windowed sums, the fold where the
    origins are split, and the particle mean;
both by device events per repetition, median of ``--reps`` with min and max,
as are the two torch routes.

Beside them, on the unwrapped planes of the same run (as f64 [F, n, 3]):
  * ``torch_direct``: the composition a user could write in torch on the same
    device and data, an f64 loop over the lags of
    ``((x[tau:] - x[:F - tau]) ** 2).sum(-1).mean(0)`` -- the particle mean
    alone, it never forms the per-particle matrix;
  * ``torch_fft``: the FFT autocorrelation route in f64 (S1 by a cumulative sum,
    S2 by ``rfft`` / ``irfft`` of length 2 F, every lag at once, cut to n_lags),
    with its largest relative deviation from the kernel's per-particle values
    over the lags >= 1.

``derived_floor_ms`` is counted, not measured: 9 f64 vector instructions a term
(3 subtractions, 3 products, 2 sums, 1 accumulate) at 4 clocks a wave of 64
terms, over the n * sum over tau of (F - tau) terms, on 256 CUs x 4 SIMDs at
``--clock-ghz`` (2.4).  The LDS reads, the staging and the selects of the ragged
steps are not in it.

    python tools/bench_msd.py [--out profiles/msd.json] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_events  # noqa: E402  (beside this file)

SHAPES = [  # name, atoms, frames, max_lag (None: all lags)
    ("214_x_20000_lag_2000", 214, 20000, 2000),
    ("4096_x_4096_all_lags", 4096, 4096, None),
    ("4096_x_1000_all_lags", 4096, 1000, None),
    ("32768_x_1000_lag_500", 32768, 1000, 500),
]
VALU_CLOCKS_PER_TERM_WAVE = 9 * 4
SIMDS = 256 * 4
BOX = 50.0
STEP = 0.6      # A a frame and coordinate: an atom crosses a face every few thousand frames


def trajectory(torch, n_atoms, n_frames, seed):
    """f32 [F, n, 3] in HBM: a random walk wrapped into the box."""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    walk = torch.rand((1, n_atoms, 3), generator=g, device="cuda:0", dtype=torch.float64) * BOX
    walk = walk + torch.cumsum(STEP * torch.randn((n_frames, n_atoms, 3), generator=g, device="cuda:0",
                                                  dtype=torch.float64), dim=0)
    return (walk - BOX * torch.floor(walk / BOX)).float().contiguous()


def msd_fft(torch, r, n_lags):
    """f64 [n_lags, n] from r f64 [F, n, 3]: msd = S1 - 2 S2 (Calandrini et al. 2011)."""
    n_frames = r.shape[0]
    d = (r * r).sum(-1)                                                    # [F, n]
    zero = torch.zeros_like(d[:1])
    # S1(m) = (2 sum D - sum over j <= m of (D[j - 1] + D[F - j])) / (F - m), with D[-1] = D[F] = 0
    take = torch.cat([zero, d[:-1]]) + torch.cat([zero, d.flip(0)[:-1]])
    count = (n_frames - torch.arange(n_frames, device=r.device, dtype=torch.float64))[:, None]
    s1 = (2.0 * d.sum(0, keepdim=True) - torch.cumsum(take, dim=0)) / count
    s2 = torch.zeros_like(d)
    for c in range(3):
        f = torch.fft.rfft(r[:, :, c], n=2 * n_frames, dim=0)
        s2 += torch.fft.irfft(f * f.conj(), n=2 * n_frames, dim=0)[:n_frames]
    return (s1 - 2.0 * s2 / count)[:n_lags]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msd.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-reps", type=int, default=None, help="repetitions of the two torch routes (default: --reps)")
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--shapes", default=None, help="comma-separated shape names (default: all)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch routes")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from rmsf_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("bench_msd needs a HIP device; nothing is measured without one")
    eng = Engine(torch.device("cuda", 0))
    want = None if a.shapes is None else set(a.shapes.split(","))
    result = {"device": torch.cuda.get_device_name(0), "clock_ghz": a.clock_ghz, "box_edge": BOX,
              "valu_clocks_per_wave_of_terms": VALU_CLOCKS_PER_TERM_WAVE, "shapes": {}}
    for k, (name, n, n_frames, max_lag) in enumerate(SHAPES):
        if want is not None and name not in want:
            continue
        x = trajectory(torch, n, n_frames, seed=k + 1)
        n_lags = n_frames if max_lag is None else max_lag + 1
        lag_block, chunk, n_splits = eng.msd_plan(n, n_frames, n_lags)
        n_terms = n * sum(n_frames - t for t in range(n_lags))
        floor_ms = 1e3 * (n_terms / 64) * VALU_CLOCKS_PER_TERM_WAVE / (SIMDS * a.clock_ghz * 1e9)
        entry = {"n_atoms": n, "n_frames": n_frames, "n_lags": n_lags, "terms": n_terms, "derived_floor_ms": floor_ms,
                 "plan": {"lag_block": lag_block, "origin_chunk": chunk, "n_splits": n_splits}}
        planes = eng.empty(n, 3, eng.msd_plane_ld(n_frames))
        out, mean = eng.empty(n_lags, n), eng.empty(n_lags)
        boxes = np.full((n_frames, 3), BOX)
        for mode in ("free", "nojump"):
            box = boxes if mode == "nojump" else None
            p_ms = timed_events(lambda: eng.msd_planes(x.data_ptr(), x.stride(0), n_frames, n, None, n, box=box,
                                                       out=planes), a.reps)
            view = planes[:, :, :n_frames]
            l_ms = timed_events(lambda: eng.msd_lags(view, n_frames, n_lags, 7, out=out, mean=mean), a.reps)
            lm = statistics.median(l_ms)
            entry[mode] = {"planes": spread(p_ms), "lags": spread(l_ms), "lags_over_floor": lm / floor_ms,
                           "msd_at_largest_lag": float(mean[-1].item())}
        # the torch routes, on the unwrapped planes (left by the nojump run above)
        if not a.no_torch:
            r = planes[:, :, :n_frames].permute(2, 0, 1).contiguous()          # f64 [F, n, 3]

            def direct():
                ts = torch.empty(n_lags, dtype=torch.float64, device=r.device)
                for tau in range(n_lags):
                    ts[tau] = ((r[tau:] - r[:n_frames - tau]) ** 2).sum(-1).mean(0).mean()
                return ts

            d_ms = timed_events(direct, a.torch_reps or a.reps)
            f_ms = timed_events(lambda: msd_fft(torch, r, n_lags), a.torch_reps or a.reps)
            torch.cuda.synchronize()
            lm = entry["nojump"]["lags"]["median_ms"]
            ts, by_fft = direct(), msd_fft(torch, r, n_lags)
            dev_direct = float(((ts[1:] - mean[1:]).abs() / mean[1:]).max().item()) if n_lags > 1 else 0.0
            dev_fft = float(((by_fft[1:] - out[1:]).abs() / out[1:]).max().item()) if n_lags > 1 else 0.0
            entry.update({"torch_direct": spread(d_ms), "torch_fft": spread(f_ms),
                          "lags_over_torch_direct": lm / statistics.median(d_ms),
                          "lags_over_torch_fft": lm / statistics.median(f_ms),
                          "torch_direct_max_rel_dev_of_mean": dev_direct,
                          "torch_fft_max_rel_dev_by_particle": dev_fft})
            del r, ts, by_fft
        result["shapes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del x, planes, out, mean
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
