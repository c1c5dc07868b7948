#!/usr/bin/env python
"""Timing of the contact kernels (csrc/contacts.hip) on one MI355X.

Per shape (selected atoms x frames, HBM-resident f32 rows, radius 4.5 A):
  * ``counts``: rmsf_contact_counts alone, the selection against itself by the
    symmetric route, device events per repetition;
  * ``counts_torch``: the composition a user could write in torch on the same
    device and data -- per batch of frames the f64 differences of each
    coordinate, their squares, the compare and the sum over frames.  The
    batch is sized so that one [batch, n, n] f64 tensor is at most
    ``--batch-bytes`` (1 GiB), stated as ``torch_batch_frames``;
  * ``fraction_hard`` / ``fraction_soft`` (dense shapes): rmsf_contact_fraction
    over the native pairs of frame 0, against ``fraction_torch``: gathered
    f64 rows of the pairs, the distance, the compare, the mean over pairs.
The counts of the kernel and of torch are compared for equality, as are the
hard-cut counts a frame.

``derived_floor_ms`` is counted, not measured: the compiled frame loop of
k_contact_counts issues 9 f64 VALU instructions (3 subtractions, 3 products, 2
sums, 1 compare) and 1 integer add-with-carry per pair and frame, each a
quarter wave a clock, on 256 CUs x 4 SIMDs at ``--clock-ghz`` (2.4), over the
pair-frames of whole 64 x 64 tiles on or above the diagonal.

The atoms are uniform in a cube at 0.05 atoms / A^3 with 0.5 A of noise a
frame, so that an atom has about 19 others within 4.5 A, as a folded chain's
heavy atoms do; the sparse shape selects every 222nd atom of 47,681.

    python tools/bench_contacts.py [--out profiles/contacts.json] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_events  # noqa: E402  (beside this file)

RADIUS = 4.5
DENSITY = 0.05
SHAPES = [  # name, atoms per frame, selected atoms, frames
    ("214_x_20000_dense", 214, 214, 20000),
    ("214_of_47681_x_20000", 47681, 214, 20000),
    ("3341_x_4096_dense", 3341, 3341, 4096),
]
VALU_PER_PAIR_FRAME = 10      # the compiled frame loop: 9 f64 instructions and 1 v_addc a pair
LANES_PER_CLOCK = 256 * 4 * 16


def trajectory(torch, n_atoms, n_frames, seed):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    side = (n_atoms / DENSITY) ** (1.0 / 3.0)
    base = torch.rand((n_atoms, 3), generator=g, device="cuda:0") * side
    x = torch.empty((n_frames, n_atoms, 3), dtype=torch.float32, device="cuda:0")
    step = max(1, (1 << 28) // (12 * n_atoms))
    for f0 in range(0, n_frames, step):
        f1 = min(n_frames, f0 + step)
        x[f0:f1] = base + 0.5 * torch.randn((f1 - f0, n_atoms, 3), generator=g, device="cuda:0")
    return x


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contacts.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch-bytes", type=int, default=1 << 30)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--shapes", default=None, help="comma-separated shape names (default: all)")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from rmsf_amd import contact_threshold_sq
    from rmsf_amd._lib import call
    from rmsf_amd.contacts import native_pairs
    from rmsf_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("bench_contacts needs a HIP device; nothing is measured without one")
    eng = Engine(torch.device("cuda", 0))
    want = None if a.shapes is None else set(a.shapes.split(","))
    t_sq = contact_threshold_sq(RADIUS)
    result = {"device": torch.cuda.get_device_name(0), "radius": RADIUS, "clock_ghz": a.clock_ghz,
              "valu_per_pair_frame": VALU_PER_PAIR_FRAME, "shapes": {}}
    for k, (name, n_atoms, n_sel, n_frames) in enumerate(SHAPES):
        if want is not None and name not in want:
            continue
        x = trajectory(torch, n_atoms, n_frames, seed=k + 1)
        sel = None if n_sel == n_atoms else np.arange(n_sel) * (n_atoms // n_sel)
        idx = None if sel is None else torch.as_tensor(sel, device=x.device)
        out = torch.empty((n_sel, n_sel), dtype=torch.int32, device=x.device)
        tile_a, tile_b, chunk, n_splits = eng.contact_counts_plan(n_sel, n_sel, n_frames, True)

        h_sel, d_sel = eng._rows(sel)            # uploaded once: the launches alone are timed
        sel_args = (None, None) if sel is None else (d_sel.data_ptr(), h_sel.ctypes.data)

        def counts():
            call("rmsf_contact_counts", x.data_ptr(), x.stride(0), n_frames, n_atoms, *sel_args, n_sel, *sel_args,
                 n_sel, 1, RADIUS, out.data_ptr(), out.stride(0), None, 0, eng.stream)

        fb = max(1, min(n_frames, a.batch_bytes // (8 * n_sel * n_sel)))

        def counts_torch():
            total = torch.zeros((n_sel, n_sel), dtype=torch.int64, device=x.device)
            for f0 in range(0, n_frames, fb):
                xs = x[f0:f0 + fb] if idx is None else x[f0:f0 + fb].index_select(1, idx)
                xs = xs.double()
                d2 = None
                for c in range(3):
                    d = xs[:, :, None, c] - xs[:, None, :, c]
                    d2 = d * d if d2 is None else d2 + d * d
                total += (d2 <= t_sq).sum(dim=0)
            return total

        k_ms = timed_events(counts, a.reps)
        t_ms = timed_events(counts_torch, a.reps)
        same = bool(torch.equal(out.to(torch.int64), counts_torch()))
        tiles = -(-n_sel // tile_a)
        pair_frames = tiles * (tiles + 1) // 2 * tile_a * tile_b * n_frames
        floor_ms = 1e3 * pair_frames * VALU_PER_PAIR_FRAME / (LANES_PER_CLOCK * a.clock_ghz * 1e9)
        km, tm = statistics.median(k_ms), statistics.median(t_ms)
        entry = {"n_atoms": n_atoms, "n_sel": n_sel, "n_frames": n_frames,
                 "plan": {"tile_a": tile_a, "tile_b": tile_b, "frame_chunk": chunk, "n_splits": n_splits},
                 "counts": spread(k_ms), "counts_torch": spread(t_ms), "torch_batch_frames": fb,
                 "counts_equal_torch": same, "counts_over_torch": km / tm,
                 "tile_pair_frames": pair_frames, "derived_floor_ms": floor_ms, "counts_over_floor": km / floor_ms}
        if sel is None:
            ref = x[0].cpu().numpy()
            pairs, r0 = native_pairs(ref, ref, RADIUS)
            n_pairs = len(pairs)
            pa, pb = (torch.as_tensor(pairs[:, c], device=x.device) for c in (0, 1))
            (h_pa, d_pa), (h_pb, d_pb) = eng._rows(pairs[:, 0]), eng._rows(pairs[:, 1])
            d_r0 = torch.as_tensor(r0, device=x.device)
            q = {m: eng.empty(n_frames) for m in (0, 2)}
            n_hard = torch.empty(n_frames, dtype=torch.int32, device=x.device)

            def fraction(method):
                return lambda: call("rmsf_contact_fraction", x.data_ptr(), x.stride(0), n_frames, n_atoms, n_atoms,
                                    None, None, d_pa.data_ptr(), d_pb.data_ptr(), h_pa.ctypes.data, h_pb.ctypes.data,
                                    d_r0.data_ptr(), n_pairs, RADIUS, method, 5.0, 1.8, q[method].data_ptr(),
                                    n_hard.data_ptr(), eng.stream)

            pb_frames = max(1, min(n_frames, a.batch_bytes // (24 * n_pairs)))

            # a tensor divisor: torch divides by a Python scalar as a product with its reciprocal, an ulp off n / P
            p_dev = torch.tensor(float(n_pairs), dtype=torch.float64, device=x.device)

            def fraction_torch():
                n = torch.empty(n_frames, dtype=torch.int64, device=x.device)
                for f0 in range(0, n_frames, pb_frames):
                    xs = x[f0:f0 + pb_frames]
                    d = xs.index_select(1, pa).double() - xs.index_select(1, pb).double()
                    n[f0:f0 + pb_frames] = ((d * d).sum(dim=2).sqrt() <= RADIUS).sum(dim=1)
                return n, n.double() / p_dev

            h_ms = timed_events(fraction(0), a.reps)
            s_ms = timed_events(fraction(2), a.reps)
            f_ms = timed_events(fraction_torch, a.reps)
            n_torch, q_torch = fraction_torch()
            entry.update({"n_pairs": n_pairs, "fraction_hard": spread(h_ms), "fraction_soft": spread(s_ms),
                          "fraction_torch": spread(f_ms), "fraction_torch_batch_frames": pb_frames,
                          "fraction_equal_torch": bool(torch.equal(n_hard.to(torch.int64), n_torch)
                                                       and torch.equal(q[0], q_torch)),
                          "fraction_hard_over_torch": statistics.median(h_ms) / statistics.median(f_ms)})
        result["shapes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del x, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
