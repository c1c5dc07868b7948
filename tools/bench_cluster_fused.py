#!/usr/bin/env python
"""Timing of the two routes from a trajectory in HBM to its neighbour bits
(``Cluster``'s input to the GROMOS loop) on one MI355X:

  * ``stored``: rmsf_pairwise_centres + rmsf_pairwise_rmsd, which writes the
    F x F f64 matrix (8 F^2 bytes), + rmsf_adjacency_pack, which reads it once;
  * ``fused``:  rmsf_pairwise_centres + rmsf_pairwise_adjacency, whose epilogue
    writes the bits (F^2 / 8 bytes) and whose second pass counts them.

Each is timed alone (device events; the output buffers of either route come
from torch's caching allocator inside the timed span) and through
``Cluster(traj, matrix="f64" | "bits").run()`` (host clock around synchronised
calls: the loop synchronises once a batch itself), median of ``--reps`` after a
warm-up, with the min and max.  At each shape the two routes' words, counts
and labels are compared for equality and the peak HBM of either ``run()``
(``torch.cuda.max_memory_allocated``) is recorded.  A shape whose f64 matrix
does not fit half the free HBM is run on the fused route alone (``--only-bits``
shapes: 200,000 frames, 5 GB of bits where the matrix would be 320 GB); there
the check is that every frame's neighbour count is its cluster's size, which
the planted states imply.

Trajectories: 214 atoms, 8 states of 2 A displacement per atom with
populations ~ 1 / (1 + index), 0.3 A noise, cutoff 1.5 A -- the end-to-end shape
of tools/bench_cluster.py, whose ``Cluster.run()`` time at the parent commit
(profiles/cluster.json) is copied into the result for comparison.

    python tools/bench_cluster_fused.py [--out profiles/cluster_fused.json] [--reps 7]
        [--frames 4096,20000,60000] [--only-bits 200000]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_events, timed_host  # noqa: E402  (beside this file)

N_ATOMS, N_STATES, RADIUS, ZERO_CUTOFF = 214, 8, 1.5, 1e-5


def states_traj(n_frames, device, block=16384):
    """f32 [n_frames, 214, 3] in HBM, built there a block at a time."""
    import torch
    g = torch.Generator(device=device).manual_seed(n_frames)
    base = torch.rand((N_ATOMS, 3), generator=g, device=device) * 100.0
    disp = torch.randn((N_STATES, N_ATOMS, 3), generator=g, device=device)
    disp /= (disp ** 2).sum(dim=(1, 2), keepdim=True).div(N_ATOMS).sqrt()
    w = 1.0 / (1.0 + torch.arange(float(N_STATES), device=device))
    member = torch.multinomial(w, n_frames, replacement=True, generator=g)
    traj = torch.empty((n_frames, N_ATOMS, 3), dtype=torch.float32, device=device)
    for r in range(0, n_frames, block):
        m = member[r:r + block]
        traj[r:r + block] = base + 2.0 * disp[m] + 0.3 * torch.randn((len(m), N_ATOMS, 3), generator=g, device=device)
    return traj


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_fused.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", default="4096,20000,60000", help="shapes run on both routes")
    ap.add_argument("--only-bits", default="200000", help="shapes run on the fused route alone")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from rmsf_amd import Cluster
    from rmsf_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("bench_cluster_fused needs a HIP device; nothing is measured without one")
    dev = torch.device("cuda", 0)
    eng = Engine(dev)
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "n_atoms": N_ATOMS, "cutoff": RADIUS,
              "shapes": {}}
    parent = os.path.join(ROOT, "profiles", "cluster.json")
    if os.path.exists(parent):
        with open(parent) as f:
            e2e = json.load(f).get("end_to_end", {})
        result["parent_cluster_run"] = {"n_frames": e2e.get("n_frames"), **e2e.get("cluster_run", {})}

    def shapes(text):
        return [int(s) for s in text.split(",") if s]

    for n, paired in [(n, True) for n in shapes(a.frames)] + [(n, False) for n in shapes(a.only_bits)]:
        torch.cuda.empty_cache()
        free = torch.cuda.mem_get_info(dev)[0]
        matrix_bytes, nw = 8 * n * n, (n + 63) // 64
        bit_bytes = 8 * n * nw
        key = f"{n}"
        if 12 * n * N_ATOMS + 2 * (bit_bytes + (matrix_bytes if paired else 0)) > free:
            result["shapes"][key] = {"skipped": f"does not fit {free} bytes of free HBM"}
            print(key, "skipped: free HBM", free, flush=True)
            continue
        traj = states_traj(n, dev)
        ptr, fstride = traj.data_ptr(), traj.stride(0)
        need = eng.pairwise_workspace_bytes(n, N_ATOMS)
        work = eng.empty(need // 8) if need else None
        state = {}

        def centres():
            return eng.pairwise_centres(ptr, fstride, n, N_ATOMS, None, None, True)

        def fused():
            centre, g = centres()
            adj = torch.empty((n, nw), dtype=torch.int64, device=dev)
            count = torch.empty(n, dtype=torch.int32, device=dev)
            eng.pairwise_adjacency(ptr, fstride, n, N_ATOMS, None, None, float(N_ATOMS), centre, g, adj, count, RADIUS,
                                   superpose=True, zero_cutoff=ZERO_CUTOFF, work=work)
            state["fused"] = (adj, count)

        def stored():
            centre, g = centres()
            out = eng.empty(n, n)
            eng.pairwise_rmsd(ptr, fstride, n, N_ATOMS, None, None, float(N_ATOMS), centre, g, out, superpose=True,
                              cutoff=ZERO_CUTOFF, work=work)
            state["stored"] = eng.adjacency_pack(out, RADIUS)

        def run(form):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            ms = timed_host(lambda: state.__setitem__(form, Cluster(traj, cutoff=RADIUS, matrix=form).run().results),
                            a.reps)
            return ms, torch.cuda.max_memory_allocated(dev) - before

        entry = {"n_frames": n, "traj_bytes": traj.numel() * 4, "matrix_bytes": matrix_bytes, "bit_bytes": bit_bytes,
                 "workspace_bytes": need}
        fused_ms = timed_events(fused, a.reps)
        entry["fused"] = spread(fused_ms)
        fused_adj, fused_count = state.pop("fused")
        if paired:
            stored_ms = timed_events(stored, a.reps)
            entry["stored"] = spread(stored_ms)
            stored_adj, stored_count = state.pop("stored")
            entry["same_words"] = bool(torch.equal(fused_adj, stored_adj))
            entry["same_counts"] = bool(torch.equal(fused_count, stored_count))
            entry["stored_over_fused"] = statistics.median(stored_ms) / statistics.median(fused_ms)
            del stored_adj, stored_count
        del fused_adj, fused_count
        torch.cuda.empty_cache()
        bits_ms, bits_peak = run("bits")
        rb = state.pop("bits")
        entry["cluster_run_bits"] = spread(bits_ms)
        entry["cluster_run_bits_peak_bytes"] = bits_peak
        entry["n_clusters"], entry["largest"] = rb.n_clusters, int(rb.sizes[0])
        # the states are further apart than the cutoff and tighter than it: every frame's neighbours are its
        # cluster (the one check of a shape that has no stored route to compare with)
        entry["neighbours_are_the_cluster"] = bool(np.array_equal(rb.n_neighbours, rb.sizes[rb.labels]))
        assert rb.matrix_form == "bits"
        if paired:
            torch.cuda.empty_cache()
            f64_ms, f64_peak = run("f64")
            rf = state.pop("f64")
            assert rf.matrix_form == "f64"
            entry["cluster_run_f64"] = spread(f64_ms)
            entry["cluster_run_f64_peak_bytes"] = f64_peak
            entry["same_labels"] = bool(np.array_equal(rb.labels, rf.labels) and np.array_equal(rb.centres, rf.centres)
                                        and np.array_equal(rb.n_neighbours, rf.n_neighbours))
            entry["run_f64_over_bits"] = statistics.median(f64_ms) / statistics.median(bits_ms)
        result["shapes"][key] = entry
        print(key, json.dumps(entry), flush=True)
        del traj, work

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
