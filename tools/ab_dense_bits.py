#!/usr/bin/env python3
"""Bit identity of the dense f64 MFMA kernels and the QCP solver between two
checkouts (a refactor's proof: csrc/dense_f64.h, rmsf_device.h::qcp_lambda).

    python tools/ab_dense_bits.py dump --tree PATH OUT.npz
    python tools/ab_dense_bits.py compare A.npz B.npz

``dump`` imports rmsf_amd from the checkout at PATH (built there), runs seeded
inputs through its ``Engine`` and saves the raw outputs: covariance
(accumulate + finish), the time-lagged co-moment (S after accumulate, M after
finish; dense / gathered, unaligned / aligned on superpose's records, one case
over three calls), pca_backproject (overwriting and accumulating), pairwise
RMSD (centres + rmsd, cutoff 0), its neighbour
bits and counts (pairwise_adjacency within the median distance), the cross RMSD
matrix (centres per side + cross_rmsd, cutoff 0), pca_project, qcp_batch, and
the transform records of superpose and superpose_seq.
``compare`` demands the same arrays with the same uint64 views; exit status 1
on any difference.  One process per dump: two checkouts' packages cannot share
an interpreter.
"""
import argparse
import itertools
import os
import sys

import numpy as np

COV_SHAPES = [(5, 3), (17, 5), (214, 67), (341, 300), (500, 40)]                  # (n_sel, n_frames)
PW_SHAPES = [(2, 3), (17, 33), (33, 31), (50, 214), (5, 5000), (500, 40)]         # (n_frames, n_sel)
ADJ_SHAPES = PW_SHAPES + [(130, 20), (300, 50)]                                   # (n_frames, n_sel)
CROSS_SHAPES = [(1, 1, 3), (17, 33, 33), (33, 5, 31), (3, 5, 5000), (50, 40, 214), (528, 130, 40)]  # (n_a, n_b, n_sel)
# tests/test_gpu_pca_project.py::ENGINE_SHAPES as (n_sel, n_frames, k)
PROJ_SHAPES = [(1, 1, 1), (5, 3, 2), (16, 16, 16), (17, 17, 17), (17, 33, 51), (214, 67, 10), (341, 300, 7),
               (5000, 5, 3)]
# (n_sel, n_frames, lag, pairs a call): one pair range, the tile edge either side of 16 atoms, a tail stage,
# split-K with a fold (whole, and over three calls), and at 25 tiles a side the direct path
LAG_SHAPES = [(5, 3, 1, None), (16, 33, 1, None), (17, 40, 7, None), (214, 67, 10, None), (341, 300, 5, None),
              (341, 300, 31, 128), (400, 45, 3, None)]
# tests/test_gpu_pca_backproject.py::ENGINE_SHAPES as (n_sel, n_frames, cols)
BPROJ_SHAPES = [(1, 1, 1), (5, 3, 2), (16, 32, 16), (17, 33, 17), (33, 31, 33), (214, 67, 48), (341, 300, 7),
                (5, 5000, 3), (5000, 5, 48)]
SUPERPOSE_SHAPE = (214, 67)                                                       # (n_sel, n_frames)


def trajectory(n_atoms, n_frames):
    """f32 [F, n_atoms, 3]: a 100 A box, 2 A of motion, a drift per frame."""
    rng = np.random.default_rng(7 * n_atoms + n_frames)
    x = rng.uniform(0.0, 100.0, size=(1, n_atoms, 3)) + 2.0 * rng.normal(size=(n_frames, n_atoms, 3))
    return np.ascontiguousarray(x + rng.uniform(-5.0, 5.0, size=(n_frames, 1, 3)), dtype=np.float32)


def selection(n_sel, gathered):
    """(n_atoms of the frame, sel): dense, or every 3rd of 3 n_sel atoms."""
    return (3 * n_sel, np.arange(1, 3 * n_sel, 3)) if gathered else (n_sel, None)


def dump(tree, out_path):
    tree = os.path.abspath(tree)
    sys.path[:0] = [tree, os.path.join(tree, "mdanalysis-mpi_amd")]
    import torch

    import rmsf_amd
    from rmsf_amd._lib import RMSF_XFORM_DOUBLES
    from rmsf_amd.engine import Engine
    assert os.path.abspath(rmsf_amd.__file__).startswith(tree + os.sep), rmsf_amd.__file__
    if not torch.cuda.is_available():
        raise SystemExit("ab_dense_bits dump needs a HIP device")
    eng = Engine(torch.device("cuda", 0))
    dev = eng.device
    out = {}

    def case(n_sel, n_frames, gathered):
        n_atoms, sel = selection(n_sel, gathered)
        x = torch.tensor(trajectory(n_atoms, n_frames), device=dev)
        return x, eng.sel_tensor(sel)

    def records(x, sel_dev, n_sel, n_frames):
        """The frames' transform records on frame 0 (the frame-parallel superposition)."""
        ref, info = eng.reference_setup(n_sel, frame_ptr=x.data_ptr(), sel=sel_dev)
        xf = eng.zeros(n_frames, RMSF_XFORM_DOUBLES)
        work = eng.empty(eng.workspace_bytes(n_sel, n_frames) // 8 + 2)
        eng.superpose(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, None, ref, info, xf, work)
        return xf, info

    for (n_sel, n_frames), gathered, aligned in itertools.product(COV_SHAPES, (False, True), (False, True)):
        x, sel_dev = case(n_sel, n_frames, gathered)
        xf, info = records(x, sel_dev, n_sel, n_frames) if aligned else (None, None)
        n = 3 * n_sel
        rows = x[0] if sel_dev is None else x[0][sel_dev.long()]
        shift = rows.reshape(-1).double().contiguous()
        cov, t1 = eng.zeros(n, n), eng.zeros(n)
        need = eng.covariance_workspace_bytes(n_sel, n_frames)
        work = eng.empty(need // 8) if need else None
        eng.covariance_accumulate(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, xf, info, shift, cov, t1, work)
        key = f"cov_{n_sel}x{n_frames}_g{int(gathered)}_a{int(aligned)}"
        out[key + "_t1"] = t1.cpu().numpy()
        eng.covariance_finish(cov, t1, n, n_frames)
        out[key] = cov.cpu().numpy()

    for (n_frames, n_sel), gathered, weighted, superpose in itertools.product(PW_SHAPES, (False, True),
                                                                               (False, True), (True, False)):
        x, sel_dev = case(n_sel, n_frames, gathered)
        w = np.random.default_rng(n_sel).uniform(1.0, 16.0, size=n_sel) if weighted else None
        w_dev = None if w is None else torch.tensor(w, device=dev)
        centre, g = eng.pairwise_centres(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, w_dev, superpose)
        need = eng.pairwise_workspace_bytes(n_frames, n_sel)
        work = eng.empty(need // 8) if need else None
        d = torch.full((n_frames, n_frames), float("nan"), dtype=torch.float64, device=dev)
        eng.pairwise_rmsd(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, w_dev,
                          float(n_sel) if w is None else float(w.sum()), centre, g, d, superpose=superpose,
                          cutoff=0.0, work=work)
        key = f"pw_{n_frames}x{n_sel}_g{int(gathered)}_w{int(weighted)}_s{int(superpose)}"
        out[key + "_centre"], out[key + "_g"], out[key] = centre.cpu().numpy(), g.cpu().numpy(), d.cpu().numpy()

    # the neighbour bits of the same cases (and two shapes more) within the median off-diagonal distance
    for (n_frames, n_sel), gathered, weighted, superpose in itertools.product(ADJ_SHAPES, (False, True),
                                                                               (False, True), (True, False)):
        x, sel_dev = case(n_sel, n_frames, gathered)
        w = np.random.default_rng(n_sel).uniform(1.0, 16.0, size=n_sel) if weighted else None
        w_dev = None if w is None else torch.tensor(w, device=dev)
        w_total = float(n_sel) if w is None else float(w.sum())
        centre, g = eng.pairwise_centres(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, w_dev, superpose)
        need = eng.pairwise_workspace_bytes(n_frames, n_sel)
        work = eng.empty(need // 8) if need else None
        tag = f"{n_frames}x{n_sel}_g{int(gathered)}_w{int(weighted)}_s{int(superpose)}"
        d = out.get("pw_" + tag)
        if d is None:  # a shape without a pw_ array: the same matrix, for the radius alone
            d = eng.empty(n_frames, n_frames)
            eng.pairwise_rmsd(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, w_dev, w_total, centre, g, d,
                              superpose=superpose, cutoff=0.0, work=work)
            d = d.cpu().numpy()
        radius = float(np.median(d[~np.eye(n_frames, dtype=bool)]))
        adj = torch.full((n_frames, eng.adjacency_words(n_frames)), -1, dtype=torch.int64, device=dev)
        count = torch.full((n_frames,), -1, dtype=torch.int32, device=dev)
        eng.pairwise_adjacency(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, w_dev, w_total, centre, g, adj,
                               count, radius, superpose=superpose, zero_cutoff=0.0, work=work)
        out["adj_" + tag], out["adj_" + tag + "_count"] = adj.cpu().numpy(), count.cpu().numpy().astype(np.int64)
        out["adj_" + tag + "_radius"] = np.asarray([radius])

    for (n_a, n_b, n_sel), (ga_, gb_), weighted, superpose in itertools.product(
            CROSS_SHAPES, ((False, False), (True, False), (False, True), (True, True)), (False, True), (True, False)):
        # one seeded trajectory, A its first n_a frames and B the rest, as selected rows: each side dense, or
        # scattered over 3 n_sel atoms and gathered back
        rows = trajectory(n_sel, n_a + n_b)

        def side(xs, gathered):
            n_atoms, sel = selection(n_sel, gathered)
            full = np.zeros((len(xs), n_atoms, 3), dtype=np.float32)
            full[:, slice(None) if sel is None else sel] = xs
            return torch.tensor(full, device=dev), eng.sel_tensor(sel)

        (xa, sel_a), (xb, sel_b) = side(rows[:n_a], ga_), side(rows[n_a:], gb_)
        w = np.random.default_rng(n_sel).uniform(1.0, 16.0, size=n_sel) if weighted else None
        w_dev = None if w is None else torch.tensor(w, device=dev)
        ca, g_a = eng.pairwise_centres(xa.data_ptr(), xa.stride(0), n_a, n_sel, sel_a, w_dev, superpose)
        if superpose:
            cb, g_b = eng.pairwise_centres(xb.data_ptr(), xb.stride(0), n_b, n_sel, sel_b, w_dev, True)
        else:  # one common origin, A's frame 0's centre: what CrossDistanceMatrix.run does
            cb, g_b = eng.pairwise_centres_about(xb.data_ptr(), xb.stride(0), n_b, n_sel, sel_b, w_dev, ca)
        need = eng.cross_workspace_bytes(n_a, n_b, n_sel)
        work = eng.empty(need // 8) if need else None
        d = torch.full((n_a, n_b), float("nan"), dtype=torch.float64, device=dev)
        eng.cross_rmsd(xa.data_ptr(), xa.stride(0), n_a, sel_a, ca, g_a, xb.data_ptr(), xb.stride(0), n_b, sel_b,
                       cb, g_b, n_sel, w_dev, float(n_sel) if w is None else float(w.sum()), d, superpose=superpose,
                       cutoff=0.0, work=work)
        key = f"cross_{n_a}x{n_b}x{n_sel}_ga{int(ga_)}_gb{int(gb_)}_w{int(weighted)}_s{int(superpose)}"
        out[key] = d.cpu().numpy()
        out[key + "_centre_a"], out[key + "_g_a"] = ca.cpu().numpy(), g_a.cpu().numpy()
        out[key + "_centre_b"], out[key + "_g_b"] = cb.cpu().numpy(), g_b.cpu().numpy()

    for (n_sel, n_frames, k), gathered, aligned in itertools.product(PROJ_SHAPES, (False, True), (False, True)):
        x, sel_dev = case(n_sel, n_frames, gathered)
        xf, info = records(x, sel_dev, n_sel, n_frames) if aligned else (None, None)
        rng = np.random.default_rng(11 * n_sel + k)
        v = torch.tensor(np.linalg.qr(rng.normal(size=(3 * n_sel, k)))[0].copy(), device=dev)
        xs = x if sel_dev is None else x.index_select(1, sel_dev.long())
        mean = xs.double().mean(dim=0).reshape(-1).contiguous()
        need = eng.pca_project_workspace_bytes(n_frames, n_sel, k)
        work = eng.empty(need // 8) if need else None
        proj = torch.full((n_frames, k), float("nan"), dtype=torch.float64, device=dev)
        eng.pca_project(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, xf, info, mean, v, k, proj, work)
        out[f"proj_{n_sel}x{n_frames}x{k}_g{int(gathered)}_a{int(aligned)}"] = proj.cpu().numpy()

    # the time-lagged co-moment: S before the finish, M after (t = operand A's T1 plus operand B's, what TICA gives it)
    for (n_sel, n_frames, lag, batch), gathered, aligned in itertools.product(LAG_SHAPES, (False, True),
                                                                                (False, True)):
        x, sel_dev = case(n_sel, n_frames, gathered)
        xf, info = records(x, sel_dev, n_sel, n_frames) if aligned else (None, None)
        n, n_pairs = 3 * n_sel, n_frames - lag
        rows = x[0] if sel_dev is None else x[0][sel_dev.long()]
        shift = rows.reshape(-1).double().contiguous()
        s, cov, t = eng.zeros(n, n), eng.zeros(n, n), eng.zeros(n)
        for k in range(0, n_pairs, batch or n_pairs):      # with a batch: several calls, offset pointers
            nb = min(batch or n_pairs, n_pairs - k)
            need = max(eng.lagged_comoment_workspace_bytes(n_sel, nb), eng.covariance_workspace_bytes(n_sel, nb))
            work = eng.empty(need // 8) if need else None
            a, b = x.data_ptr() + 4 * k * x.stride(0), x.data_ptr() + 4 * (k + lag) * x.stride(0)
            xa = None if xf is None else xf[k:k + nb]
            xb = None if xf is None else xf[k + lag:k + lag + nb]
            eng.lagged_comoment_accumulate(a, x.stride(0), b, x.stride(0), nb, n_sel, sel_dev, xa, xb, info, shift, s,
                                           work)
            eng.covariance_accumulate(a, x.stride(0), nb, n_sel, sel_dev, xa, info, shift, cov, t, work)
            eng.covariance_accumulate(b, x.stride(0), nb, n_sel, sel_dev, xb, info, shift, cov, t, work)
        key = f"lag_{n_sel}x{n_frames}_l{lag}_b{batch or 0}_g{int(gathered)}_a{int(aligned)}"
        out[key + "_s"], out[key + "_t"] = s.cpu().numpy(), t.cpu().numpy()
        eng.lagged_comoment_finish(s, t, n, 2 * n_pairs)
        out[key] = s.cpu().numpy()

    # pca_backproject, overwriting and accumulating onto a seeded Y
    for (n_sel, n_frames, cols), gathered, aligned in itertools.product(BPROJ_SHAPES, (False, True), (False, True)):
        x, sel_dev = case(n_sel, n_frames, gathered)
        xf, info = records(x, sel_dev, n_sel, n_frames) if aligned else (None, None)
        rng = np.random.default_rng(13 * n_sel + cols)
        p = torch.tensor(rng.normal(size=(n_frames, cols)), device=dev)
        y0 = torch.tensor(rng.normal(size=(3 * n_sel, cols)), device=dev)
        xs = x if sel_dev is None else x.index_select(1, sel_dev.long())
        mean = xs.double().mean(dim=0).reshape(-1).contiguous()
        need = eng.pca_backproject_workspace_bytes(n_frames, n_sel, cols)
        work = eng.empty(need // 8) if need else None
        for accumulate in (False, True):
            y = y0.clone()
            eng.pca_backproject(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, xf, info, mean, p, cols, y,
                                accumulate, work)
            out[f"bproj_{n_sel}x{n_frames}x{cols}_g{int(gathered)}_a{int(aligned)}_acc{int(accumulate)}"] = \
                y.cpu().numpy()

    # qcp_batch: tests/golden/qcp_kat.npz's pair, then seeded 50-atom pairs
    kat = np.load(os.path.join(tree, "tests", "golden", "qcp_kat.npz"))
    rng = np.random.default_rng(5)
    pairs = [(kat["ref"], kat["mob"])]
    for _ in range(255):
        ref = 10.0 * rng.normal(size=(50, 3))
        pairs.append((ref, ref @ np.linalg.qr(rng.normal(size=(3, 3)))[0] + 0.5 * rng.normal(size=(50, 3))))
    a9, e0, cnt = [], [], []
    for ref, mob in pairs:
        ref, mob = ref - ref.mean(0), mob - mob.mean(0)
        a9.append((mob.T @ ref).reshape(9))
        e0.append(0.5 * ((ref * ref).sum() + (mob * mob).sum()))
        cnt.append(float(len(ref)))
    rot, rmsd = eng.qcp_batch(torch.tensor(np.asarray(a9), device=dev), torch.tensor(np.asarray(e0), device=dev),
                              torch.tensor(np.asarray(cnt), device=dev))
    out["qcp_rot"], out["qcp_rmsd"] = rot.cpu().numpy(), rmsd.cpu().numpy()

    n_sel, n_frames = SUPERPOSE_SHAPE
    for gathered in (False, True):
        x, sel_dev = case(n_sel, n_frames, gathered)
        out[f"superpose_g{int(gathered)}"] = records(x, sel_dev, n_sel, n_frames)[0].cpu().numpy()
        _, ref, info = eng.reference_setup_seq(n_sel, float(n_sel), frame_ptr=x.data_ptr(), sel=sel_dev)
        xf = eng.zeros(n_frames, RMSF_XFORM_DOUBLES)
        eng.superpose_seq(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, None, float(n_sel), ref, info, xf)
        out[f"superpose_seq_g{int(gathered)}"] = xf.cpu().numpy()

    torch.cuda.synchronize()
    np.savez(out_path, **out)
    print(f"{len(out)} arrays from {tree} -> {out_path}")
    return 0


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or not np.array_equal(x.view(np.uint64), y.view(np.uint64)):
            n = int((x.view(np.uint64) != y.view(np.uint64)).sum()) if x.shape == y.shape else -1
            print(f"DIFFERENT {k}: {n} of {x.size} elements")
            bad.append(k)
    print(f"{len(a.files)} arrays in {path_a}, {len(b.files)} in {path_b}: "
          + ("no difference" if not bad else f"{len(bad)} differ or are missing: {bad}"))
    return 1 if bad else 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("--tree", required=True, help="the checkout whose rmsf_amd (and built library) to run")
    d.add_argument("out")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    a = ap.parse_args(argv)
    return dump(a.tree, a.out) if a.cmd == "dump" else compare(a.a, a.b)


if __name__ == "__main__":
    sys.exit(main())
