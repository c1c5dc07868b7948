#!/usr/bin/env python
"""Timing of the GROMOS clustering of an RMSD matrix (csrc/clustering.hip) on
one MI355X: rmsf_adjacency_pack + rmsf_cluster_gromos with the f64 matrix
already in HBM, host clock around synchronised calls (the loop synchronises
once a batch itself, so device events would not span it), median of ``--reps``
after a warm-up.

Matrices [F, F]: Euclidean distances of F points in the plane, built on the
device and symmetric in their bits -- 6 planted states with unit normal noise
and one point in ten a uniform outlier -- in three forms:
  * ``planted``:    cutoff 2.0, tens to hundreds of clusters;
  * ``singletons``: cutoff 0, below every distance: F clusters of one frame;
  * ``one``:        cutoff inf: one cluster.

Against, on the same device and matrix:
  * ``torch``: what a user could write before this kernel -- ``adj = d <= c``,
    then per cluster a masked argmax, a row AND and the sum of the members'
    rows (the matrix is symmetric, so this is the masked column sum read along
    rows), with the ``.item()`` and ``nonzero`` synchronisations it needs;
  * ``numpy``: the same loop on the host copy, the device-to-host copy of the
    f64 matrix included.
torch.argmax does not promise the first maximum, so the torch loop's clusters
may differ where counts tie; its cluster count is reported, not compared.

Reported per shape: times, clusters per second, the pack's bytes per second
(it reads 8 F^2 bytes once) against ``--hbm-peak``, and the loop's microseconds
per cluster.  ``end_to_end``: ``Cluster(traj).run()`` at 214 atoms x 4,096
frames against ``DistanceMatrix(traj).run()`` followed by the numpy loop.

    python tools/bench_cluster.py [--out profiles/cluster.json] [--reps 7] [--frames 4096,20000,60000]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_timing import spread, timed_events, timed_host  # noqa: E402  (beside this file)

FORMS = (("planted", 2.0), ("singletons", 0.0), ("one", float("inf")))


def points_matrix(n, device, block=2048):
    """f64 [n, n] in HBM, symmetric in its bits: (a - b)^2 = (b - a)^2 exactly."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(n)
    k = 6
    side = 10.0 * k ** 0.5
    centres = torch.rand((k, 2), generator=g, dtype=torch.float64) * side
    w = 1.0 / (1.0 + torch.arange(k, dtype=torch.float64))
    member = torch.multinomial(w, n, replacement=True, generator=g)
    x = centres[member] + torch.randn((n, 2), generator=g, dtype=torch.float64)
    out = torch.randperm(n, generator=g)[: n // 10]
    x[out] = torch.rand((len(out), 2), generator=g, dtype=torch.float64) * (side + 10.0) - 5.0
    x = x.to(device)
    d = torch.empty((n, n), dtype=torch.float64, device=device)
    for r in range(0, n, block):
        dx = x[r:r + block, None, 0] - x[None, :, 0]
        dy = x[r:r + block, None, 1] - x[None, :, 1]
        d[r:r + block] = torch.sqrt(dx * dx + dy * dy)
    return d


def torch_loop(d, cut):
    import torch
    n = d.shape[0]
    adj = d <= cut
    adj.fill_diagonal_(True)
    counts = adj.sum(1)
    active = torch.ones(n, dtype=torch.bool, device=d.device)
    labels = torch.empty(n, dtype=torch.int64, device=d.device)
    minus = torch.full_like(counts, -1)
    k = 0
    while True:
        val, c = torch.where(active, counts, minus).max(0)
        if val.item() < 0:
            break
        mem = adj[c] & active
        labels[mem] = k
        active &= ~mem
        counts -= adj[mem].sum(0)
        k += 1
    return labels, k


def numpy_loop(d, cut):
    import numpy as np
    adj = d <= cut
    n = len(adj)
    adj[np.arange(n), np.arange(n)] = True
    counts = adj.sum(1)
    active = np.ones(n, dtype=bool)
    labels = np.empty(n, dtype=np.int64)
    k = 0
    while active.any():
        c = int(np.argmax(np.where(active, counts, -1)))
        mem = adj[c] & active
        labels[mem] = k
        active &= ~mem
        counts -= adj[mem].sum(0)
        k += 1
    return labels, k


def host_once(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t), out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", default="4096,20000,60000")
    ap.add_argument("--hbm-peak", type=float, default=8.0, help="HBM peak in TB/s")
    ap.add_argument("--baseline-budget-s", type=float, default=25.0,
                    help="a baseline whose first call took t seconds is repeated min(reps, budget / t) times in all")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from rmsf_amd import Cluster, DistanceMatrix
    from rmsf_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("bench_cluster needs a HIP device; nothing is measured without one")
    dev = torch.device("cuda", 0)
    eng = Engine(dev)
    result = {"device": torch.cuda.get_device_name(0), "hbm_peak_tbs": a.hbm_peak, "reps": a.reps, "shapes": {}}

    def repeat(fn, first_ms):
        """first call included: min(reps, budget / t) calls in all, at least one."""
        ms = [first_ms]
        more = min(a.reps, int(a.baseline_budget_s * 1e3 / max(first_ms, 1e-3))) - 1
        for _ in range(max(more, 0)):
            ms.append(host_once(fn)[0])
        return ms

    for n in [int(s) for s in a.frames.split(",") if s]:
        free = torch.cuda.mem_get_info(dev)[0]
        if 8 * n * n * 1.6 > free:      # the matrix, a row block of its construction, the bits, torch's bool copy
            result["shapes"][f"{n}"] = {"skipped": f"a [{n}, {n}] f64 matrix does not fit {free} bytes of free HBM"}
            print(n, "skipped: free HBM", free, flush=True)
            continue
        d = points_matrix(n, dev)
        big = 8 * n * n > 8 * 2 ** 30
        for form, cut in FORMS:
            state = {}

            def device_path():
                adj, count = eng.adjacency_pack(d, cut)
                state["out"] = eng.cluster_gromos(adj, count)

            total = timed_host(device_path, a.reps)
            pack = timed_events(lambda: eng.adjacency_pack(d, cut), a.reps)
            adj, count = eng.adjacency_pack(d, cut)
            loop = timed_host(lambda: eng.cluster_gromos(adj, count), a.reps)
            label, centre, size = state["out"]
            k = int(centre.numel())
            tm, pm, lm = (statistics.median(v) for v in (total, pack, loop))
            entry = {
                "n_frames": n, "cutoff": cut if cut != float("inf") else "inf", "n_clusters": k,
                "largest": int(size[0]), "singletons": int((size == 1).sum()),
                "matrix_bytes": 8 * n * n, "bit_bytes": 8 * n * ((n + 63) // 64),
                "pack_and_loop": spread(total), "pack": spread(pack), "loop": spread(loop),
                "clusters_per_s": k / (tm * 1e-3),
                "pack_tbs": 8 * n * n / (pm * 1e-3) / 1e12, "pack_hbm_share": 8 * n * n / (pm * 1e-3) / 1e12 / a.hbm_peak,
                "loop_us_per_cluster": 1e3 * lm / k,
            }
            del adj, count
            # the torch composition on the same matrix (not the F-iteration singleton loop of the largest shapes)
            if big and form == "singletons":
                entry["torch"] = None
            else:
                first, (_, tk) = host_once(lambda: torch_loop(d, cut))       # warm-up: not kept
                first, (tl, tk) = host_once(lambda: torch_loop(d, cut))
                ms = repeat(lambda: torch_loop(d, cut), first)
                entry["torch"] = spread(ms)
                entry["torch_n_clusters"] = tk
                entry["torch_same_labels"] = bool(torch.equal(tl, label.to(torch.int64)))
                entry["torch_over_device"] = statistics.median(ms) / tm
            if big:
                entry["numpy"] = None
            else:
                def numpy_path():
                    return numpy_loop(d.cpu().numpy(), cut)
                first, (nl, nk) = host_once(numpy_path)
                ms = repeat(numpy_path, first)
                entry["numpy_with_d2h"] = spread(ms)
                entry["numpy_same_labels"] = bool(np.array_equal(nl, label.cpu().numpy()))
                entry["numpy_over_device"] = statistics.median(ms) / tm
            result["shapes"][f"{n}_{form}"] = entry
            print(f"{n}_{form}", json.dumps(entry), flush=True)
        del d
        torch.cuda.empty_cache()

    # end to end: 214 atoms x 4,096 frames, 8 states of 2 A displacement, 0.3 A noise
    n_atoms, n_frames, radius = 214, 4096, 1.5
    g = torch.Generator(device="cpu").manual_seed(214)
    base = torch.rand((n_atoms, 3), generator=g) * 100.0
    disp = torch.randn((8, n_atoms, 3), generator=g)
    disp /= (disp ** 2).sum(dim=(1, 2), keepdim=True).div(n_atoms).sqrt()
    member = torch.multinomial(1.0 / (1.0 + torch.arange(8.0)), n_frames, replacement=True, generator=g)
    traj = (base + 2.0 * disp[member] + 0.3 * torch.randn((n_frames, n_atoms, 3), generator=g)).to(dev)

    def new():
        return Cluster(traj, cutoff=radius).run().results

    def old():
        return numpy_loop(DistanceMatrix(traj).run().results.dist_matrix, radius)

    new_ms, old_ms = timed_host(new, a.reps), timed_host(old, a.reps)
    r, (ol, ok) = new(), old()
    result["end_to_end"] = {
        "n_atoms": n_atoms, "n_frames": n_frames, "cutoff": radius, "n_clusters": r.n_clusters,
        "cluster_run": spread(new_ms), "distance_matrix_run_then_numpy_loop": spread(old_ms),
        "same_labels": bool(np.array_equal(r.labels, ol)),
        "old_over_new": statistics.median(old_ms) / statistics.median(new_ms),
    }
    print("end_to_end", json.dumps(result["end_to_end"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
