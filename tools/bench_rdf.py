#!/usr/bin/env python
"""Timing of the radial distribution kernel (csrc/rdf.hip) on one MI355X.

Per shape (atoms x frames, HBM-resident f32 rows, the atoms against themselves
by the symmetric route, range (0, 15) A, 75 bins), free and periodic:
  * ``rdf``: rmsf_rdf_counts alone (the threshold copy, the zeroing and the
    kernel), device events per repetition;
  * ``rdf_torch``: the composition a user could write in torch on the same
    device and data -- per batch of frames (and block of rows) the f64
    differences of each coordinate, ``d - L * round(d * (1 / L))`` with a box,
    the squares, the root, ``torch.bucketize`` against the edges and
    ``torch.bincount``.  One [batch, rows, n] f64 tensor is at most
    ``--batch-bytes`` (1 GiB), stated as ``torch_batch``.  bucketize with
    ``right=True`` is the definition's rule (e_k <= d < e_(k+1)); d == rmax is
    folded into the last bin and the self pairs (d = 0, bin 0) are taken out,
    so the counts are compared for equality everywhere;
  * ``contact_counts``: rmsf_contact_counts at radius = rmax on the same frames
    (free space only: it takes no box) -- the bare distance tile, what the
    image term and the binning cost over it.

``derived_floor_ms`` is counted, not measured: the VALU issue cycles of the
compiled frame loop of k_rdf_counts a pair and frame, in range or not.  In free
space 10 f64 instructions (3 subtractions, 3 products, 2 sums, 2 compares
against the range) and the f64 -> f32 conversion, 4 clocks a wave each (a
quarter wave a clock); v_sqrt_f32, 8; and 7 f32 / integer instructions (the
guess: subtract, multiply, convert, clamp twice, select, the table address), 2
each: 66 clocks.  A box adds 12 f64 instructions (3 products with 1 / L, 3
v_rndne_f64, 3 products with L, 3 subtractions): 114 clocks.  That is taken
over the pair-frames of whole 64 x 64 tiles on or above the diagonal, 64 pairs
a wave, on 256 CUs x 4 SIMDs at ``--clock-ghz`` (2.4).  The LDS reads (24
coordinates and 16 threshold pairs a lane and frame), the waits for them, the
staging, and what a pair in range adds (two compares, the LDS add, a walk
where the guess missed) are not in the floor.  With ``--nbins 1`` the kernel
has no guess and no table: the 10 f64 instructions and 2 integer ones, 44.

    python tools/bench_rdf.py [--out profiles/rdf.json] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_events  # noqa: E402  (beside this file)

RANGE = (0.0, 15.0)
NBINS = 75
WATER = 4096 / 49.7 ** 3       # oxygens / A^3
SHAPES = [  # name, atoms, frames, kind
    ("214_x_20000_chain", 214, 20000, "chain"),
    ("3341_x_4096_chain", 3341, 4096, "chain"),
    ("4096_x_1000_water", 4096, 1000, "gas"),
    ("32768_x_64_water", 32768, 64, "gas"),
]
VALU_CLOCKS_PER_PAIR_FRAME = {"free": 66, "periodic": 114}     # a wave of 64 pairs; see above
VALU_CLOCKS_ONE_BIN = {"free": 44, "periodic": 92}
SIMDS = 256 * 4


def trajectory(torch, n_atoms, n_frames, kind, seed):
    """(x f32 [F, n, 3] in HBM, the box edge).  chain: bench_contacts' atoms, 0.05
    / A^3 in a cube with 0.5 A of noise a frame, in a box 30 A wider than the
    cube; gas: fresh uniform points every frame at water's number density."""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    x = torch.empty((n_frames, n_atoms, 3), dtype=torch.float32, device="cuda:0")
    step = max(1, (1 << 28) // (12 * n_atoms))
    if kind == "chain":
        side = (n_atoms / 0.05) ** (1.0 / 3.0)
        base = torch.rand((n_atoms, 3), generator=g, device="cuda:0") * side
        for f0 in range(0, n_frames, step):
            f1 = min(n_frames, f0 + step)
            x[f0:f1] = base + 0.5 * torch.randn((f1 - f0, n_atoms, 3), generator=g, device="cuda:0")
        return x, side + 30.0
    side = (n_atoms / WATER) ** (1.0 / 3.0)
    for f0 in range(0, n_frames, step):
        f1 = min(n_frames, f0 + step)
        x[f0:f1] = torch.rand((f1 - f0, n_atoms, 3), generator=g, device="cuda:0") * side
    return x, side


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdf.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch-bytes", type=int, default=1 << 30)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--shapes", default=None, help="comma-separated shape names (default: all)")
    ap.add_argument("--torch-reps", type=int, default=None, help="repetitions of the torch composition (default: --reps)")
    ap.add_argument("--nbins", type=int, default=NBINS)
    ap.add_argument("--lib", default=None, help="a variant build of the library to time rmsf_rdf_counts from "
                                                "(tools/build_ab.sh); the baselines stay the tree's")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition (variant builds)")
    a = ap.parse_args(argv)
    nbins = a.nbins

    import numpy as np
    import torch

    from rmsf_amd._lib import call, load
    from rmsf_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("bench_rdf needs a HIP device; nothing is measured without one")
    eng = Engine(torch.device("cuda", 0))
    rdf_lib = load(a.lib) if a.lib else load()
    want = None if a.shapes is None else set(a.shapes.split(","))
    edges = torch.as_tensor(np.linspace(*RANGE, nbins + 1)).to("cuda:0")
    need = int(load().rmsf_rdf_counts_workspace_bytes(nbins))
    work = torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "range": RANGE, "nbins": nbins,
              "library": a.lib or "in-tree", "clock_ghz": a.clock_ghz,
              "valu_clocks_per_wave_pair_frame": VALU_CLOCKS_ONE_BIN if nbins == 1 else VALU_CLOCKS_PER_PAIR_FRAME, "shapes": {}}
    unequal = []
    for k, (name, n, n_frames, kind) in enumerate(SHAPES):
        if want is not None and name not in want:
            continue
        x, side = trajectory(torch, n, n_frames, kind, seed=k + 1)
        tile_a, tile_b, chunk, n_splits = eng.rdf_counts_plan(n, n, n_frames, True)
        tiles = -(-n // tile_a)
        pair_frames = tiles * (tiles + 1) // 2 * tile_a * tile_b * n_frames
        out = torch.empty(nbins, dtype=torch.int64, device=x.device)
        entry = {"n_atoms": n, "n_frames": n_frames, "box_edge": side, "tile_pair_frames": pair_frames,
                 "plan": {"tile_a": tile_a, "tile_b": tile_b, "frame_chunk": chunk, "n_splits": n_splits}}
        # one [frames, rows, n] f64 tensor of the composition within --batch-bytes
        rows = max(1, min(n, a.batch_bytes // (8 * n)))
        fb = max(1, min(n_frames, a.batch_bytes // (8 * rows * n)))
        entry["torch_batch"] = {"frames": fb, "rows": rows}
        for mode in ("free", "periodic"):
            h_box = d_box = None
            if mode == "periodic":
                h_box = np.ascontiguousarray(np.tile([side] * 3 + [1.0 / side] * 3, (n_frames, 1)))
                d_box = torch.as_tensor(h_box).to(x.device)
            L, iL = side, 1.0 / side

            def rdf():
                rc = rdf_lib.rmsf_rdf_counts(x.data_ptr(), x.stride(0), n_frames, n, None, None, n, None, None, n, 1, 0, 0,
                                             None if d_box is None else d_box.data_ptr(),
                                             None if h_box is None else h_box.ctypes.data, RANGE[0], RANGE[1], nbins,
                                             out.data_ptr(), work.data_ptr(), need, eng.stream)
                assert rc == 0, rdf_lib.rmsf_last_error()

            def rdf_torch():
                """int64 [nbins] of the composition.  Bucket nbins + 1 holds d >= rmax, of
                which d == rmax belongs to the last bin: one more compare and sum."""
                total = torch.zeros(nbins + 2, dtype=torch.int64, device=x.device)
                closed = torch.zeros((), dtype=torch.int64, device=x.device)
                for f0 in range(0, n_frames, fb):
                    xs = x[f0:f0 + fb].double()
                    for r0 in range(0, n, rows):
                        d2 = None
                        for c in range(3):
                            d = xs[:, r0:r0 + rows, None, c] - xs[:, None, :, c]
                            if mode == "periodic":
                                d = d - L * torch.round(d * iL)
                            d2 = d * d if d2 is None else d2 + d * d
                        dist = d2.sqrt_()
                        total += torch.bincount(torch.bucketize(dist, edges, right=True).reshape(-1),
                                                minlength=nbins + 2)
                        closed += (dist == RANGE[1]).sum()
                counts = total[1:nbins + 1].clone()
                counts[nbins - 1] += closed
                counts[0] -= n * n_frames                                  # the self pairs, d = 0
                return counts

            k_ms = timed_events(rdf, a.reps)
            e = {"rdf": spread(k_ms)}
            km = statistics.median(k_ms)
            clocks = (VALU_CLOCKS_ONE_BIN if nbins == 1 else VALU_CLOCKS_PER_PAIR_FRAME)[mode]
            floor_ms = 1e3 * (pair_frames / 64) * clocks / (SIMDS * a.clock_ghz * 1e9)
            e.update({"derived_floor_ms": floor_ms, "rdf_over_floor": km / floor_ms,
                      "pairs_in_range": int(out.sum().item()),
                      "share_in_range": float(out.sum().item()) / (n * (n - 1) * n_frames)})
            if not a.no_torch:
                t_ms = timed_events(rdf_torch, a.torch_reps or a.reps)
                tm = statistics.median(t_ms)
                rdf()
                torch.cuda.synchronize()
                diff = (out - rdf_torch()).abs()
                same = not bool(diff.any())
                e.update({"rdf_torch": spread(t_ms), "rdf_over_torch": km / tm, "counts_equal_torch": same,
                          "counts_max_abs_diff_torch": int(diff.max().item())})
                if not same:
                    unequal.append((name, mode))
            if mode == "free":
                cc = torch.empty((n, n), dtype=torch.int32, device=x.device)

                def contact_counts():
                    call("rmsf_contact_counts", x.data_ptr(), x.stride(0), n_frames, n, None, None, n, None, None, n,
                         1, RANGE[1], cc.data_ptr(), cc.stride(0), None, 0, eng.stream)

                c_ms = timed_events(contact_counts, a.reps)
                torch.cuda.synchronize()
                total_contacts = int(cc.to(torch.int64).sum().item()) - n * n_frames   # less the diagonal
                e.update({"contact_counts": spread(c_ms), "rdf_over_contact_counts": km / statistics.median(c_ms),
                          # d <= rmax against the histogram's total: the same pairs
                          "contact_total_equals_histogram": total_contacts == e["pairs_in_range"]})
                del cc
            entry[mode] = e
        result["shapes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del x, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    assert not unequal, f"the kernel's counts differ from the torch composition's: {unequal}"
    return 0


if __name__ == "__main__":
    sys.exit(main())
