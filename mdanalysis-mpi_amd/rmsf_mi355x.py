#!/usr/bin/env python3
"""Script mode: ``RMSF.py`` on MI355X.

    # RMSF.py's own run (mpirun -n P python RMSF.py) -> one process per GPU
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \\
        --master-addr 127.0.0.1 --master-port 29500 rmsf_mi355x.py \\
        --topology adk.gro --trajectory adk.xtc

    # without MDAnalysis: a synthetic trajectory generated in HBM
    python rmsf_mi355x.py --synthetic 100000 2000 --align frame0

Without MDAnalysis, a .gro or .psf topology and an .xtc, .dcd (or
multi-frame .gro) trajectory are read natively (rmsf_amd.topology /
rmsf_amd.xtc / rmsf_amd.dcd) and the selection is evaluated by the native
subset of the selection language (BASELINE C1: adk PSF/DCD).

Defaults mirror RMSF.py: selection "protein and name CA" (RMSF.py:77),
ref_frame 0 (RMSF.py:63), the two-sweep average alignment (RMSF.py:89-140),
frame blocks per rank (RMSF.py:65-69) with the per-rank range printed as at
RMSF.py:74, the ranks' statistics merged by a reduce to rank 0
(RMSF.py:143's ``comm.reduce(root=0)``; ``--merge all`` / ``scatter`` for the
all-reduce / the reduce-scatter by atom slices) and the RMSF computed on
rank 0 (RMSF.py:145-146) -- which this script also writes out (``--out``),
where RMSF.py only says "#Do something with RMSF" (RMSF.py:147).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np


def main(argv=None) -> int:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--topology")
    ap.add_argument("--trajectory")
    ap.add_argument("--select", default="protein and name CA")
    ap.add_argument("--synthetic", nargs=2, type=int, metavar=("N_ATOMS", "N_FRAMES"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--align", choices=["average", "frame0", "none"], default="average")
    ap.add_argument("--ref-frame", type=int, default=0)
    ap.add_argument("--out", default=None, help="write rank 0's RMSF (.npy)")
    ap.add_argument("--merge", choices=["root", "all", "scatter"], default="root",
                    help="N>1: reduce to rank 0 (RMSF.py:143, default), all-reduce, or reduce-scatter by atom slices")
    ap.add_argument("--exact", action="store_true",
                    help="with --align none: RMSF.py:120-146 with the script's own arithmetic, bit for bit "
                         "(per-frame Welford, ranks reduced by second_order_moments in comm.reduce's order)")
    ap.add_argument("--merge-order", choices=["mpi4py", "rank"], default="mpi4py",
                    help="--exact, N>1: the order RMSF.py:143's comm.reduce applies second_order_moments in "
                         "(mpi4py: its default binomial tree; rank: rank order)")
    ap.add_argument("--covariance", default=None, metavar="OUT.npy",
                    help="also write the positional covariance of the (aligned) selected coordinates, f64 "
                         "[3n, 3n] (co-moment / n_frames; not with --merge scatter), on rank 0")
    ap.add_argument("--dist-matrix", default=None, metavar="OUT.npy",
                    help="also write the all-pairs RMSD matrix of the selected atoms' frames, f64 [F, F] "
                         "(rmsf_amd.DistanceMatrix; each pair superposed unless --align none; one process only)")
    ap.add_argument("--cluster", default=None, metavar="OUT.npy",
                    help="also write the GROMOS cluster of every frame, int64 [F], clusters numbered from the largest "
                         "(rmsf_amd.Cluster on the RMSD matrix --dist-matrix writes, which stays in HBM; needs "
                         "--cluster-cutoff; one process only)")
    ap.add_argument("--cluster-cutoff", type=float, default=None, metavar="C",
                    help="--cluster: the cluster radius in A, frames within C of each other are neighbours")
    ap.add_argument("--cluster-matrix", choices=["auto", "f64", "bits"], default=None,
                    help="--cluster / --dbscan: 'f64' stores the F x F RMSD matrix in HBM and packs it into neighbour bits; "
                         "'bits' has the pair kernel write the bits and stores no matrix (F^2 / 8 bytes: what fits "
                         "at 10^5 - 10^6 frames); 'auto' (the default) takes 'f64' where it fits and 'bits' where "
                         "it does not")
    ap.add_argument("--dbscan", default=None, metavar="OUT.npy",
                    help="also write the DBSCAN cluster of every frame, int64 [F], -1 for noise, clusters numbered by "
                         "their first core frame (rmsf_amd.DBSCAN on the RMSD matrix --dist-matrix writes, which stays "
                         "in HBM; needs --dbscan-eps; --cluster-matrix applies; one process only)")
    ap.add_argument("--dbscan-eps", type=float, default=None, metavar="E",
                    help="--dbscan: the neighbourhood radius in A, frames within E of each other are neighbours")
    ap.add_argument("--dbscan-min-samples", type=int, default=None, metavar="M",
                    help="--dbscan: a frame with at least M frames within E, itself included, is a core frame "
                         "(default 5; 1 is single linkage)")
    ap.add_argument("--diffusion-map", default=None, metavar="OUT.npy",
                    help="also write the diffusion-map embedding of the frames at time 1, f64 [F, K]: the first K "
                         "diffusion coordinates of the RMSD matrix --dist-matrix writes, which stays in HBM "
                         '(rmsf_amd.DiffusionMap, solver="device"; needs --diffusion-epsilon and --n-eigenvectors; '
                         "one process only)")
    ap.add_argument("--diffusion-epsilon", type=float, default=None, metavar="E",
                    help="--diffusion-map: the kernel's scale in A^2, K = exp(-d^2 / E)")
    ap.add_argument("--n-eigenvectors", type=int, default=None, metavar="K",
                    help="--diffusion-map: the number of diffusion coordinates, 1..39")
    ap.add_argument("--cross-rmsd", default=None, metavar="OUT.npy",
                    help="also write the RMSD of every frame of the trajectory to every frame of --cross-with, "
                         "f64 [F, F_b] (rmsf_amd.CrossDistanceMatrix; each pair superposed unless --align none; "
                         "one process only; not with --synthetic)")
    ap.add_argument("--cross-with", default=None, metavar="TRAJ",
                    help="--cross-rmsd: the second trajectory (or reference structures), of the same topology and "
                         "selection")
    ap.add_argument("--pca-transform", default=None, metavar="OUT.npy",
                    help="also run rmsf_amd.PCA on the same input with --align and write the projection of the "
                         "frames on its components, f64 [F, K] (PCA.transform; one process only)")
    ap.add_argument("--n-components", type=int, default=None, metavar="K",
                    help="--pca-transform: the number of components (default: all 3n)")
    ap.add_argument("--pca-solver", choices=["host", "device", "matrix_free"], default="host",
                    help="--pca-transform: numpy.linalg.eigh on the host, or the first --n-components (<= 40) modes "
                         "by subspace iteration on the device: 'device' with the matrix staying in HBM, "
                         "'matrix_free' from the trajectory alone, with no 3n x 3n matrix (any number of atoms)")
    ap.add_argument("--tica", default=None, metavar="OUT.npz",
                    help="also run rmsf_amd.TICA on the same input with --align and write its eigenvalues, "
                         "timescales, components [3n, K] and mean [n, 3] (one process only; K: --n-components, "
                         "default every direction the covariance keeps)")
    ap.add_argument("--tica-lag", type=int, default=None, metavar="L",
                    help="--tica: the lag, in frames of the run's list")
    ap.add_argument("--contact-map", default=None, metavar="OUT.npy",
                    help="also write the contact counts of the selection against itself, int64 [n, n]: the frames in "
                         "which two atoms are within --contact-radius of each other (rmsf_amd.ContactMap; no periodic "
                         "images; one process only)")
    ap.add_argument("--contacts", default=None, metavar="OUT.npy",
                    help="also write the fraction of native contacts along the trajectory, f64 [F, 2] of frame and "
                         "Q: the pairs within --contact-radius in the first frame (rmsf_amd.Contacts; one process "
                         "only)")
    ap.add_argument("--contact-radius", type=float, default=None, metavar="R",
                    help="--contact-map / --contacts: the contact distance in A (default 4.5)")
    ap.add_argument("--contacts-method", choices=["hard_cut", "radius_cut", "soft_cut"], default=None,
                    help="--contacts: how a pair counts towards Q (default hard_cut)")
    ap.add_argument("--rdf", default=None, metavar="OUT.npz",
                    help="also write the radial distribution function of the selection against itself (or against "
                         "--rdf-select-b): bins, edges, count and rdf (rmsf_amd.InterRDF; one process only).  "
                         "Without --rdf-box the run is in free space and rdf is the density-normalised count")
    ap.add_argument("--rdf-range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="--rdf: the range of distances in A (default 0 15)")
    ap.add_argument("--rdf-nbins", type=int, default=None, metavar="N", help="--rdf: the number of bins (default 75)")
    ap.add_argument("--rdf-box", nargs="+", default=None, metavar="file|LX LY LZ",
                    help="--rdf: 'file' for the boxes of an .xtc trajectory, or three edges in A of one orthorhombic "
                         "box; distances then follow the minimum image and rdf is normalised by the volume")
    ap.add_argument("--rdf-select-b", default=None, metavar="SEL",
                    help="--rdf: the second group, a selection string read as --select is (natively read "
                         "topologies only)")
    ap.add_argument("--msd", default=None, metavar="OUT.npz",
                    help="also write the mean squared displacement of the selected atoms: delta_t_values, timeseries "
                         "[n_lags] and msds_by_particle [n_lags, n] (rmsf_amd.EinsteinMSD; one process only).  "
                         "With --msd-box the trajectory is unwrapped by the nojump rule first")
    ap.add_argument("--msd-type", choices=["xyz", "xy", "yz", "xz", "x", "y", "z"], default=None,
                    help="--msd: the coordinates of the displacement (default xyz)")
    ap.add_argument("--msd-max-lag", type=int, default=None, metavar="L",
                    help="--msd: the largest lag in frames (default: the number of frames less one)")
    ap.add_argument("--msd-box", nargs="+", default=None, metavar="file|LX LY LZ",
                    help="--msd: 'file' for the boxes of an .xtc trajectory, or three edges in A of one orthorhombic "
                         "box, to unwrap the trajectory with (unwrap='nojump')")
    ap.add_argument("--msd-dt", type=float, default=None, metavar="DT",
                    help="--msd: the time between two frames, for delta_t_values (default 1)")
    a = ap.parse_args(argv)
    msd_box = None
    if not a.msd and (a.msd_type or a.msd_max_lag is not None or a.msd_box or a.msd_dt is not None):
        ap.error("--msd-type, --msd-max-lag, --msd-box and --msd-dt need --msd OUT.npz")
    if a.msd:
        if int(os.environ.get("WORLD_SIZE", 1)) > 1:
            ap.error("--msd runs in one process (no torch.distributed launch)")
        if a.msd_max_lag is not None and a.msd_max_lag < 0:
            ap.error("--msd-max-lag must not be negative")
        if a.msd_max_lag is not None and a.synthetic and a.msd_max_lag >= a.synthetic[1]:
            ap.error("--msd-max-lag must be below the number of frames")
        if a.msd_dt is not None and not abs(a.msd_dt) < float("inf"):
            ap.error("--msd-dt must be finite")
        if a.msd_box == ["file"]:
            if not (a.trajectory and a.trajectory.lower().endswith(".xtc")):
                ap.error("--msd-box file needs an .xtc --trajectory")
            msd_box = "file"
        elif a.msd_box is not None:
            try:
                msd_box = [float(v) for v in a.msd_box]
            except ValueError:
                msd_box = []
            if len(msd_box) != 3 or not all(0.0 < v < float("inf") for v in msd_box):
                ap.error("--msd-box takes 'file' or three positive finite edges LX LY LZ")
    rdf_box = None
    if not a.rdf and (a.rdf_range or a.rdf_nbins is not None or a.rdf_box or a.rdf_select_b):
        ap.error("--rdf-range, --rdf-nbins, --rdf-box and --rdf-select-b need --rdf OUT.npz")
    if a.rdf:
        if int(os.environ.get("WORLD_SIZE", 1)) > 1:
            ap.error("--rdf runs in one process (no torch.distributed launch)")
        lo, hi = a.rdf_range or (0.0, 15.0)
        if not 0.0 <= lo < hi < float("inf"):
            ap.error("--rdf-range needs 0 <= LO < HI, both finite")
        if a.rdf_nbins is not None and not 1 <= a.rdf_nbins <= 2048:
            ap.error("--rdf-nbins must be in 1..2048")
        if a.rdf_box == ["file"]:
            if not (a.trajectory and a.trajectory.lower().endswith(".xtc")):
                ap.error("--rdf-box file needs an .xtc --trajectory")
            rdf_box = "file"
        elif a.rdf_box is not None:
            try:
                rdf_box = [float(v) for v in a.rdf_box]
            except ValueError:
                rdf_box = []
            if len(rdf_box) != 3 or not all(0.0 < v < float("inf") for v in rdf_box):
                ap.error("--rdf-box takes 'file' or three positive finite edges LX LY LZ")
            if hi > 0.5 * min(rdf_box):
                ap.error("--rdf-range ends over half the shortest --rdf-box edge")
        if a.rdf_select_b and a.synthetic:
            ap.error("--rdf-select-b needs a topology")
    if a.contact_radius is not None and not (a.contact_map or a.contacts):
        ap.error("--contact-radius needs --contact-map or --contacts")
    if a.contact_radius is not None and not 0.0 < a.contact_radius < float("inf"):
        ap.error("--contact-radius must be positive and finite")
    if a.contacts_method and not a.contacts:
        ap.error(f"--contacts-method {a.contacts_method} needs --contacts")
    if (a.contact_map or a.contacts) and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--contact-map and --contacts run in one process (no torch.distributed launch)")
    if bool(a.tica) != (a.tica_lag is not None):
        ap.error("--tica OUT.npz and --tica-lag L go together")
    if a.tica and a.tica_lag < 1:
        ap.error("--tica-lag must be at least 1")
    if a.tica and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--tica runs in one process (no torch.distributed launch)")
    if a.pca_transform and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--pca-transform runs in one process (no torch.distributed launch)")
    if a.pca_transform and a.merge == "scatter":
        ap.error("--pca-transform needs --merge root or all")
    if a.pca_solver != "host" and not a.pca_transform:
        ap.error(f"--pca-solver {a.pca_solver} needs --pca-transform")
    if a.pca_solver != "host" and a.n_components is None:
        ap.error(f"--pca-solver {a.pca_solver} needs --n-components")
    if a.dist_matrix and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--dist-matrix runs in one process (no torch.distributed launch)")
    if bool(a.cluster) != (a.cluster_cutoff is not None):
        ap.error("--cluster OUT.npy and --cluster-cutoff C go together")
    if a.cluster_matrix and not (a.cluster or a.dbscan):
        ap.error(f"--cluster-matrix {a.cluster_matrix} needs --cluster or --dbscan")
    if a.cluster and not a.cluster_cutoff >= 0.0:
        ap.error("--cluster-cutoff must be >= 0")
    if a.cluster and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--cluster runs in one process (no torch.distributed launch)")
    if bool(a.dbscan) != (a.dbscan_eps is not None):
        ap.error("--dbscan OUT.npy and --dbscan-eps E go together")
    if a.dbscan_min_samples is not None and not a.dbscan:
        ap.error("--dbscan-min-samples needs --dbscan")
    if a.dbscan and not a.dbscan_eps >= 0.0:
        ap.error("--dbscan-eps must be >= 0")
    if a.dbscan and a.dbscan_min_samples is not None and a.dbscan_min_samples < 1:
        ap.error("--dbscan-min-samples must be >= 1")
    if a.dbscan and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--dbscan runs in one process (no torch.distributed launch)")
    if bool(a.diffusion_map) != (a.diffusion_epsilon is not None) or bool(a.diffusion_map) != (
            a.n_eigenvectors is not None):
        ap.error("--diffusion-map OUT.npy, --diffusion-epsilon E and --n-eigenvectors K go together")
    if a.diffusion_map and not (a.diffusion_epsilon > 0.0 and 1 <= a.n_eigenvectors <= 39):
        ap.error("--diffusion-epsilon must be > 0 and --n-eigenvectors in 1..39")
    if a.diffusion_map and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--diffusion-map runs in one process (no torch.distributed launch)")
    if bool(a.cross_rmsd) != bool(a.cross_with):
        ap.error("--cross-rmsd OUT.npy and --cross-with TRAJ go together")
    if a.cross_rmsd and a.synthetic:
        ap.error("--cross-rmsd needs --topology/--trajectory")
    if a.cross_rmsd and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--cross-rmsd runs in one process (no torch.distributed launch)")
    if a.covariance and a.merge == "scatter":
        ap.error("--covariance needs --merge root or all")
    if a.exact and (a.align != "none" or a.merge == "scatter"):
        ap.error("--exact needs --align none and --merge root or all")

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    from rmsf_amd import RMSF, parallel
    from rmsf_amd.engine import Engine
    from rmsf_amd.pipeline import run_pipeline
    from rmsf_amd.sources import DeviceSource, FrameList
    from rmsf_amd.synth import generate, motion_table

    align = None if a.align == "none" else a.align
    rank, size = parallel.world()
    root = None if a.merge == "all" else 0
    cov_kw = {"covariance": True} if a.covariance else {}
    cov = None
    dm_input, dm_kw = None, {}   # what --dist-matrix reads: the RMSF run's own input
    cross_b = None               # what --cross-with names, read as the input is
    rdf_sel_b = None             # what --rdf-select-b selects
    if a.synthetic:
        n_atoms, n_frames = a.synthetic
        eng = Engine()
        b0, b1 = parallel.blocks(n_frames, size)[rank]
        print("Process:%3d --> Frames: %10d -- %10d" % (rank, b0, b1), flush=True)
        motion = motion_table(a.seed + 1, n_frames) if align else None
        shard = generate(eng, n_atoms, b0, max(b1 - b0, 1), seed=a.seed, motion=motion)[: b1 - b0]
        res = run_pipeline(eng, DeviceSource(shard, offset=b0, n_traj=n_frames), FrameList(n_frames),
                           align=align, ref_frame=a.ref_frame, merge_root=root, merge_scatter=a.merge == "scatter",
                           exact=a.exact, merge_order=a.merge_order, **cov_kw)
        rmsf = None if res.rmsf is None else res.rmsf.cpu().numpy()   # None on the non-root ranks
        if a.covariance and res.comoment is not None:
            cov = res.covariance.cpu().numpy()
        dm_input = shard
    else:
        if not (a.topology and a.trajectory):
            ap.error("--topology/--trajectory (MDAnalysis) or --synthetic is required")
        try:
            import MDAnalysis as mda
        except ImportError:
            mda = None
        if mda is not None:
            u = mda.Universe(a.topology, a.trajectory)
            ag = u.select_atoms(a.select)
            results = RMSF(ag, align=align, ref_frame=a.ref_frame, verbose=True, merge_root=root,
                           merge_scatter=a.merge == "scatter", exact=a.exact,
                           merge_order=a.merge_order, **cov_kw).run().results
            rmsf, cov = results.rmsf, (results.covariance if a.covariance else None)
            dm_input = ag
            if a.cross_with:
                cross_b = mda.Universe(a.topology, a.cross_with).select_atoms(a.select)
        else:
            # native fallback: GRO or PSF topology + selection subset; XTC, DCD (or
            # multi-frame GRO) trajectory.  PSF masses (GRO: masses guessed from
            # the atom names, as MDAnalysis' GROParser does) feed the
            # mass-weighted centre of mass RMSF.py uses (RMSF.py:84,94,117,127).
            from rmsf_amd.topology import GroTopology, PsfTopology

            ext = a.topology.lower().rsplit(".", 1)[-1]
            if ext not in ("gro", "psf"):
                ap.error("without MDAnalysis only .gro and .psf topologies are read natively")
            top = GroTopology(a.topology) if ext == "gro" else PsfTopology(a.topology)
            sel = top.select(a.select)
            masses = None if top.masses is None else top.masses[sel]
            traj = (a.trajectory if a.trajectory.lower().endswith((".xtc", ".dcd"))
                    else GroTopology(a.trajectory).frames)
            results = RMSF(traj, select=sel, align=align, masses=masses, ref_frame=a.ref_frame,
                           verbose=True, merge_root=root, merge_scatter=a.merge == "scatter", exact=a.exact,
                           merge_order=a.merge_order, **cov_kw).run().results
            rmsf, cov = results.rmsf, (results.covariance if a.covariance else None)
            dm_input, dm_kw = traj, {"select": sel, "weights": masses}
            if a.rdf_select_b:
                rdf_sel_b = top.select(a.rdf_select_b)
            if a.cross_with:
                cross_b = (a.cross_with if a.cross_with.lower().endswith((".xtc", ".dcd"))
                           else GroTopology(a.cross_with).frames)
    if a.dist_matrix:
        from rmsf_amd import DistanceMatrix
        dm = DistanceMatrix(dm_input, superposition=align is not None, **dm_kw).run().results
        print(f"RMSD matrix over {dm.n_frames} frames: max {dm.dist_matrix.max():.6f} A", flush=True)
        np.save(a.dist_matrix, dm.dist_matrix)
    if a.cluster:
        from rmsf_amd import Cluster
        cl = Cluster(dm_input, cutoff=a.cluster_cutoff, superposition=align is not None,
                     matrix=a.cluster_matrix or "auto", **dm_kw).run().results
        print(f"GROMOS clusters at {a.cluster_cutoff} A over {cl.n_frames} frames: {cl.n_clusters}, the largest of "
              f"{int(cl.sizes[0]) if cl.n_clusters else 0} frames (neighbour bits from "
              f"{'the stored f64 matrix' if cl.matrix_form == 'f64' else 'the pair kernel, no matrix stored'})",
              flush=True)
        np.save(a.cluster, cl.labels)
    if a.dbscan:
        from rmsf_amd import DBSCAN
        db = DBSCAN(dm_input, eps=a.dbscan_eps, min_samples=5 if a.dbscan_min_samples is None else a.dbscan_min_samples,
                    superposition=align is not None, matrix=a.cluster_matrix or "auto", **dm_kw).run().results
        print(f"DBSCAN clusters at {a.dbscan_eps} A, {db.n_rounds} rounds, over {db.n_frames} frames: {db.n_clusters}, "
              f"{len(db.core_sample_indices)} core frames, {db.n_noise} noise (neighbour bits from "
              f"{'the stored f64 matrix' if db.matrix_form == 'f64' else 'the pair kernel, no matrix stored'})",
              flush=True)
        np.save(a.dbscan, db.labels)
    if a.diffusion_map:
        from rmsf_amd import DiffusionMap, DistanceMatrix
        dmap = DiffusionMap(DistanceMatrix(dm_input, superposition=align is not None, **dm_kw),
                            epsilon=a.diffusion_epsilon, n_eigenvectors=a.n_eigenvectors, solver="device").run()
        emb = dmap.transform(a.n_eigenvectors, 1.0)
        print(f"diffusion map of {emb.shape[0]} frames at epsilon {a.diffusion_epsilon} A^2: eigenvalues "
              f"{np.array2string(dmap.results.eigenvalues[1:], precision=6)} after the constant mode, "
              f"{dmap.results.solver_info['n_iter']} iterations", flush=True)
        np.save(a.diffusion_map, emb)
    if a.cross_rmsd:
        from rmsf_amd import CrossDistanceMatrix
        cm = CrossDistanceMatrix(dm_input, cross_b, superposition=align is not None, **dm_kw).run().results
        print(f"cross RMSD matrix, {cm.n_frames} x {cm.n_frames_b} frames: max {cm.dist_matrix.max():.6f} A, "
              f"largest distance to the nearest frame of --cross-with {cm.nearest_dist.max():.6f} A", flush=True)
        np.save(a.cross_rmsd, cm.dist_matrix)
    if a.pca_transform:
        from rmsf_amd import PCA
        pca_kw = {"select": dm_kw["select"], "masses": dm_kw["weights"]} if dm_kw else {}
        pca = PCA(dm_input, align=align, ref_frame=a.ref_frame, n_components=a.n_components,
                  solver=a.pca_solver, **pca_kw).run()
        proj = pca.transform()
        print(f"PCA projection of {proj.shape[0]} frames on {proj.shape[1]} components: the first holds "
              f"{pca.results.cumulated_variance[0]:.4f} of the variance", flush=True)
        np.save(a.pca_transform, proj)
    if a.contact_map or a.contacts:
        from rmsf_amd import ContactMap, Contacts
        ct_kw = {"select": dm_kw["select"]} if dm_kw else {}
        radius = 4.5 if a.contact_radius is None else a.contact_radius
        if a.contact_map:
            cm = ContactMap(dm_input, radius=radius, **ct_kw).run().results
            print(f"contact map at {radius} A over {cm.n_frames} frames: {cm.counts.shape[0]} atoms, "
                  f"{int((cm.counts > 0).sum())} ordered pairs in contact in some frame", flush=True)
            np.save(a.contact_map, cm.counts)
        if a.contacts:
            ct = Contacts(dm_input, radius=radius, method=a.contacts_method or "hard_cut", **ct_kw).run().results
            print(f"native contacts at {radius} A: {len(ct.pairs)} pairs in the first frame, Q from "
                  f"{ct.q.min():.4f} to {ct.q.max():.4f} over {ct.n_frames} frames", flush=True)
            np.save(a.contacts, ct.timeseries)
    if a.rdf:
        from rmsf_amd import InterRDF
        if a.rdf_select_b and rdf_sel_b is None:
            raise SystemExit("--rdf-select-b is read through the native topology reader only (no MDAnalysis group)")
        rdf_kw = {"select": dm_kw["select"]} if dm_kw else {}
        if rdf_box == "file" and not isinstance(dm_input, str):
            raise SystemExit("--rdf-box file reads the boxes through the native .xtc reader only")
        rd = InterRDF(dm_input, select_b=rdf_sel_b, nbins=75 if a.rdf_nbins is None else a.rdf_nbins,
                      range=tuple(a.rdf_range or (0.0, 15.0)), norm="density" if rdf_box is None else "rdf",
                      box=rdf_box, **rdf_kw).run().results
        print(f"radial distribution function over {rd.n_frames} frames, {len(rd.bins)} bins on "
              f"[{rd.edges[0]}, {rd.edges[-1]}] A: {int(rd.count_int.sum())} pair distances in range, the largest "
              f"value {np.nanmax(rd.rdf):.4f} at {rd.bins[int(np.nanargmax(rd.rdf))]:.3f} A", flush=True)
        np.savez(a.rdf, bins=rd.bins, edges=rd.edges, count=rd.count, rdf=rd.rdf, volume=rd.volume)
    if a.msd:
        from rmsf_amd import EinsteinMSD
        msd_kw = {"select": dm_kw["select"]} if dm_kw else {}
        if msd_box == "file" and not isinstance(dm_input, str):
            raise SystemExit("--msd-box file reads the boxes through the native .xtc reader only")
        ms = EinsteinMSD(dm_input, msd_type=a.msd_type or "xyz", max_lag=a.msd_max_lag,
                         unwrap=None if msd_box is None else "nojump", box=msd_box,
                         dt=1.0 if a.msd_dt is None else a.msd_dt, **msd_kw).run().results
        print(f"mean squared displacement ({a.msd_type or 'xyz'}) of {ms.n_particles} atoms over {ms.n_frames} "
              f"frames, {len(ms.timeseries)} lags: {ms.timeseries[-1]:.6f} A^2 at the largest"
              + ("" if msd_box is None else ", unwrapped (nojump)"), flush=True)
        np.savez(a.msd, delta_t_values=ms.delta_t_values, timeseries=ms.timeseries,
                 msds_by_particle=ms.msds_by_particle)
    if a.tica:
        from rmsf_amd import TICA
        tica_kw = {"select": dm_kw["select"], "masses": dm_kw["weights"]} if dm_kw else {}
        tr = TICA(dm_input, a.tica_lag, align=align, ref_frame=a.ref_frame, n_components=a.n_components,
                  **tica_kw).run().results
        print(f"TICA at lag {tr.lag} over {tr.n_pairs} pairs of {tr.n_frames} frames, rank {tr.rank}: eigenvalues "
              f"{np.array2string(tr.eigenvalues[:5], precision=6)}, timescales "
              f"{np.array2string(tr.timescales[:5], precision=2)} frames", flush=True)
        np.savez(a.tica, eigenvalues=tr.eigenvalues, timescales=tr.timescales, components=tr.components, mean=tr.mean)
    if rank == 0:
        print(f"RMSF over {len(rmsf)} atoms: mean {rmsf.mean():.6f} A, max {rmsf.max():.6f} A", flush=True)
        if a.out:
            np.save(a.out, rmsf)
        if a.covariance:
            np.save(a.covariance, cov)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
