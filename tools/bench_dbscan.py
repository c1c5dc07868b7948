#!/usr/bin/env python
"""Timing of DBSCAN on the neighbour bits (csrc/dbscan.hip) on one MI355X:
host clock around synchronised calls (the component loop synchronises once a
batch of rounds itself, so device events would not span it), median of
``--reps`` after a warm-up, with min and max.

``shapes``: tools/bench_cluster.py's planted matrices [F, F] (6 states in the
plane, unit noise, one point in ten an outlier), eps 2.0, min_samples 5, the
bits already in HBM: ``rmsf_cluster_dbscan`` alone -- its rounds, the bytes a
round reads (the core rows' words, 8 * n_core * words) and those bytes over the
whole call's time against ``--hbm-peak`` (the call also holds the init, id and
label launches and one host read a batch of rounds, so this is a floor of the
round kernel's rate).  Against, where present (``"not run"`` where not):
  * ``sklearn``: the device-to-host copy of the f64 matrix, then
    ``sklearn.cluster.DBSCAN(metric="precomputed")``;
  * ``scipy``: the same copy, the threshold and
    ``scipy.sparse.csgraph.connected_components`` on the core rows (components
    only: no border rows, no ids);
  * ``torch``: the masked-min loop on the same device and matrix -- ``adj = d
    <= eps``, then every core row takes the lowest label among its core
    neighbours until nothing changes, one ``.item()`` a round; a row block at
    a time, so that the [F, F] int64 temporary stays within ``--torch-block``
    rows.
The host baselines are run up to ``--host-max-frames`` frames.

``end_to_end``: ``DBSCAN(traj, eps=1.5, min_samples=5).run()`` on
tools/bench_cluster_fused.py's trajectories (214 atoms, 8 states) with the
matrix stored (``matrix="f64"``) and fused (``matrix="bits"``).

    python tools/bench_dbscan.py [--out profiles/dbscan.json] [--reps 7] [--frames 4096,20000,60000]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mdanalysis-mpi_amd")]

from bench_cluster import points_matrix  # noqa: E402  (beside this file)
from bench_cluster_fused import N_ATOMS, RADIUS, states_traj  # noqa: E402
from bench_timing import spread, timed_host  # noqa: E402

EPS, MIN_SAMPLES = 2.0, 5


def torch_loop(d, eps, m, block):
    """(labels of the core rows' components, -1 elsewhere; rounds): plain masked-min propagation."""
    import torch
    n = d.shape[0]
    adj = d <= eps
    adj.fill_diagonal_(True)
    core = adj.sum(1) >= m
    adj &= core[None, :]
    low = torch.arange(n, device=d.device)
    big = torch.full((), n, device=d.device)
    rounds = 0
    while True:
        rounds += 1
        new = low.clone()
        for r in range(0, n, block):
            new[r:r + block] = torch.where(adj[r:r + block], low[None, :], big).min(1).values
        new = torch.where(core, new, low)
        if bool(torch.equal(new, low)):
            break
        low = new
    return torch.where(core, low, torch.full_like(low, -1)), rounds


def host_once(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t), out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", default="4096,20000,60000")
    ap.add_argument("--hbm-peak", type=float, default=8.0, help="HBM peak in TB/s")
    ap.add_argument("--host-max-frames", type=int, default=20000)
    ap.add_argument("--torch-block", type=int, default=8192)
    ap.add_argument("--baseline-budget-s", type=float, default=20.0,
                    help="a baseline whose first call took t seconds is repeated min(reps, budget / t) times in all")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from rmsf_amd import DBSCAN
    from rmsf_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("bench_dbscan needs a HIP device; nothing is measured without one")
    try:
        from sklearn.cluster import DBSCAN as SkDBSCAN
    except ImportError:
        SkDBSCAN = None
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        connected_components = None
    dev = torch.device("cuda", 0)
    eng = Engine(dev)
    result = {"device": torch.cuda.get_device_name(0), "hbm_peak_tbs": a.hbm_peak, "reps": a.reps, "eps": EPS,
              "min_samples": MIN_SAMPLES, "shapes": {}, "end_to_end": {}}

    def repeat(fn, first_ms):
        """first call included: min(reps, budget / t) calls in all, at least one."""
        ms = [first_ms]
        more = min(a.reps, int(a.baseline_budget_s * 1e3 / max(first_ms, 1e-3))) - 1
        for _ in range(max(more, 0)):
            ms.append(host_once(fn)[0])
        return ms

    frames = [int(s) for s in a.frames.split(",") if s]
    for n in frames:
        torch.cuda.empty_cache()
        free = torch.cuda.mem_get_info(dev)[0]
        if 8 * n * n * 1.6 > free:
            result["shapes"][f"{n}"] = {"skipped": f"a [{n}, {n}] f64 matrix does not fit {free} bytes of free HBM"}
            continue
        d = points_matrix(n, dev)
        adj, count = eng.adjacency_pack(d, EPS)
        state = {}

        def loop():
            state["out"] = eng.cluster_dbscan(adj, count, MIN_SAMPLES)

        ms = timed_host(loop, a.reps)
        label, core, k, rounds = state["out"]
        labels = label.cpu().numpy().astype(np.int64)
        core_bits = np.unpackbits(core.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
        n_core, nw = int(core_bits.sum()), (n + 63) // 64
        round_bytes = 8 * n_core * nw
        med = statistics.median(ms)
        entry = {
            "n_frames": n, "n_clusters": k, "n_core": n_core, "n_noise": int((labels < 0).sum()), "n_rounds": rounds,
            "neighbours_mean": float(count.double().mean()), "bit_bytes": 8 * n * nw, "round_bytes": round_bytes,
            "loop": spread(ms), "loop_ms_per_round": med / rounds,
            "round_bytes_over_loop_tbs": rounds * round_bytes / (med * 1e-3) / 1e12,
            "round_bytes_over_loop_hbm_share": rounds * round_bytes / (med * 1e-3) / 1e12 / a.hbm_peak,
        }
        # the masked-min loop in torch on the same device and matrix
        first, _ = host_once(lambda: torch_loop(d, EPS, MIN_SAMPLES, a.torch_block))      # warm-up: not kept
        first, (tl, tr) = host_once(lambda: torch_loop(d, EPS, MIN_SAMPLES, a.torch_block))
        tms = repeat(lambda: torch_loop(d, EPS, MIN_SAMPLES, a.torch_block), first)
        tl = tl.cpu().numpy()
        same = all(len(set(tl[core_bits & (labels == c)])) == 1 for c in range(k)) and len(set(tl[core_bits])) == k
        entry.update(torch=spread(tms), torch_rounds=tr, torch_same_components=bool(same),
                     torch_over_device=statistics.median(tms) / med)
        if n > a.host_max_frames:
            entry["sklearn_with_d2h"] = entry["scipy_with_d2h"] = "not run"
        else:
            if SkDBSCAN is None:
                entry["sklearn_with_d2h"] = "not run"
            else:
                def sk():
                    return SkDBSCAN(eps=EPS, min_samples=MIN_SAMPLES, metric="precomputed").fit(d.cpu().numpy()).labels_
                first, sl = host_once(sk)
                sms = repeat(sk, first)
                entry.update(sklearn_with_d2h=spread(sms), sklearn_same_labels=bool(np.array_equal(sl, labels)),
                             sklearn_over_device=statistics.median(sms) / med)
            if connected_components is None:
                entry["scipy_with_d2h"] = "not run"
            else:
                def sp():
                    h = d.cpu().numpy() <= EPS
                    c = h.sum(1) >= MIN_SAMPLES
                    return connected_components(csr_matrix(h[np.ix_(c, c)]), directed=False)[0]
                first, sk_n = host_once(sp)
                pms = repeat(sp, first)
                entry.update(scipy_with_d2h=spread(pms), scipy_same_count=bool(sk_n == k),
                             scipy_over_device=statistics.median(pms) / med)
        result["shapes"][f"{n}"] = entry
        print(n, json.dumps(entry), flush=True)
        del d, adj, count
    for n in frames:
        torch.cuda.empty_cache()
        free = torch.cuda.mem_get_info(dev)[0]
        if 12 * n * N_ATOMS + 2.5 * 8 * n * n > free:
            result["end_to_end"][f"{n}"] = {"skipped": f"does not fit {free} bytes of free HBM"}
            continue
        traj = states_traj(n, dev)
        entry = {"n_frames": n, "n_atoms": N_ATOMS, "eps": RADIUS, "min_samples": MIN_SAMPLES}
        ref = None
        for route, name in (("f64", "stored"), ("bits", "fused")):
            state = {}

            def run():
                state["r"] = DBSCAN(traj, eps=RADIUS, min_samples=MIN_SAMPLES, matrix=route).run().results

            entry[name] = spread(timed_host(run, a.reps))
            r = state["r"]
            entry.update(n_clusters=r.n_clusters, n_noise=r.n_noise, n_rounds=r.n_rounds)
            if ref is None:
                ref = r.labels
            else:
                entry["same_labels"] = bool(np.array_equal(ref, r.labels))
        result["end_to_end"][f"{n}"] = entry
        print("end_to_end", n, json.dumps(entry), flush=True)
        del traj
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
