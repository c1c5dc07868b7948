"""GPU tier: ``PCA(solver="matrix_free")`` and its operator
``rmsf_amd.eigen.TrajectoryOps`` -- M Q = D^T (D Q) / (F - ddof) from the
trajectory (csrc/pca_project.hip, csrc/pca_backproject.hip), no [3n, 3n]
matrix -- against the matrix ``RMSF(covariance=True)`` forms from the same
input, against ``solver="host"``, and, at a size whose matrix cannot exist,
against the dual (F x F) solution in numpy.

Data: the planted-mode recipe of tests/test_gpu_pca_project.py, restated.

Bounds (derived, not measured), with eps = 2^-52, e = tol + 8 (3n + F) eps
(tests/test_pca_eig_host.py::check_pairs' bounds; the factored product has two
contractions, of lengths 3n and F) and l_1 the largest eigenvalue:
  * one product: ``8 (3n + F) eps (|M| @ |q|)`` per element, plus the effect
    of the mean's last bits.  The matrix side centres exactly (C - T1 T1^T /
    N); the operator subtracts the Welford mean m' = m + delta from every
    frame, D' = D - 1 delta^T.  D^T 1 = 0 for the exact mean, so D'^T D' =
    D^T D + F delta delta^T: the first-order terms vanish and what is left is
    ``F / (F - 1) |delta|_i sum_j |delta|_j |q|_jc`` with |delta|_i <= F eps
    max_f |x_i(f)| (F Welford updates, each rounding at the size of the
    coordinate).
  * values ``|l - l_ref| <= e l_1``; vectors ``|v - s v_ref|_2 <= 2 e l_1 /
    gap_i``; orthonormality ``64 n eps``;
  * cumulated variance ``(k + 1) e``: k values within e l_1 <= e trace, and
    the two traces (the Welford sums, the matrix's diagonal) within e of each
    other;
  * ``rmsip >= 1 - 1e-9``;
  * ``transform()`` after the two solvers: ``|d(f)|_2 |v - v_ref|_2`` (the
    vector bound above) plus the projection kernel's f64 bound, twice.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODE_SIGMA = (2.0, 1.4, 1.0)   # A per atom, the three planted modes
NOISE = 0.3
EPS = 2.0 ** -52
TOL = 1e-10


@pytest.fixture(autouse=True)
def release_hbm():
    """Every test hands its HBM back (tensors kept alive by the reference
    cycle of a ``pytest.raises`` record included): the suite's large-memory
    tests measure the free HBM, in whatever order the files run."""
    yield
    import gc

    import torch
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def make_traj(n_atoms: int, n_frames: int, seed: int = 0) -> np.ndarray:
    """f32 [F, n_atoms, 3]: base + sum_k a_k(f) mode_k + noise, then a random
    rotation about the centroid and a translation per frame."""
    rng = np.random.default_rng(1000 * seed + 7 * n_atoms + n_frames)
    base = rng.uniform(0.0, 100.0, size=(n_atoms, 3))
    modes = rng.normal(size=(3, n_atoms, 3))
    modes /= np.sqrt((modes ** 2).sum(axis=(1, 2), keepdims=True) / n_atoms)   # unit displacement per atom
    amp = rng.normal(size=(n_frames, 3)) * np.asarray(MODE_SIGMA)
    x = base + np.einsum("fk,kac->fac", amp, modes) + NOISE * rng.normal(size=(n_frames, n_atoms, 3))
    q = rng.normal(size=(n_frames, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, a, b, c = q.T
    rot = np.stack([np.stack([1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)], -1),
                    np.stack([2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)], -1),
                    np.stack([2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)], -1)], -2)
    cen = x.mean(axis=1, keepdims=True)
    x = np.einsum("fac,fcd->fad", x - cen, rot) + cen + rng.uniform(-5.0, 5.0, size=(n_frames, 1, 3))
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def selection(n_sel: int, gathered: bool):
    """(n_atoms of the frame, sel): dense, or every 3rd of 3 n_sel atoms."""
    return (3 * n_sel, np.arange(1, 3 * n_sel, 3)) if gathered else (n_sel, None)


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint64)


def gaps(w_ref, idx):
    out = []
    for i in idx:
        d = np.abs(w_ref - w_ref[i])
        d[i] = np.inf
        out.append(d.min())
    return np.asarray(out)


def check_pairs(n, n_frames, w_ref, v_ref, vals, vecs, k, what):
    """tests/test_pca_eig_host.py::check_pairs with e = tol + 8 (n + F) eps.
    ``w_ref``: every reference eigenvalue the gaps need, descending."""
    e = (TOL + 8.0 * (n + n_frames) * EPS) * w_ref[0]
    assert vals.shape == (k,) and vecs.shape == (n, k) and vals.dtype == vecs.dtype == np.float64
    dv = np.abs(vals - w_ref[:k])
    print(f"{what}: max |dl| / bound = {dv.max() / e:.3e}")
    assert np.all(dv <= e)
    g = gaps(w_ref, range(k))
    for i in range(k):
        s = 1.0 if vecs[:, i] @ v_ref[:, i] >= 0.0 else -1.0
        d = np.linalg.norm(vecs[:, i] - s * v_ref[:, i])
        print(f"{what}: vector {i}: |dv| / bound = {d * g[i] / (2.0 * e):.3e}")
        assert d <= 2.0 * e / g[i]
    assert np.abs(vecs.T @ vecs - np.eye(k)).max() <= 64.0 * n * EPS
    j = np.argmax(np.abs(vecs), axis=0)
    assert np.all(vecs[j, np.arange(k)] > 0.0)


# ---- 1. one product against the matrix -----------------------------------------
@pytest.mark.parametrize("b", [16, 48])
@pytest.mark.parametrize("align", [None, "average"])
def test_symm_against_the_matrix(align, b):
    import torch

    from rmsf_amd import RMSF
    from rmsf_amd.eigen import DeviceOps, TrajectoryOps
    from rmsf_amd.engine import Engine
    n_sel, n_frames = 214, 300
    n = 3 * n_sel
    traj = make_traj(n_sel, n_frames)
    x = torch.tensor(traj, device="cuda:0")
    rm = RMSF(x, align=align, exact=False, covariance=True)
    rm._comoment_stays_in_hbm = True
    r = rm.run().results
    eng = Engine(torch.device("cuda", 0))
    cov = rm._comoment_hbm
    eng.divide(cov.view(-1), float(n_frames - 1), cov.view(-1))
    q = np.random.default_rng(b).standard_normal((n, b))
    dense = DeviceOps(cov, eng)
    want = dense.get(dense.symm(dense.put(q)))
    last = rm._last_run
    ops = TrajectoryOps(last["source"], last["frames"], r.mean, n_frames - 1, masses=last["masses"],
                        aligned=align is not None, exact=last["exact"], ref=last["ref"], refinfo=last["refinfo"],
                        engine=eng)
    assert ops.n == n
    q_d = ops.put(q)
    got = ops.get(ops.symm(q_d))
    m = np.abs(cov.cpu().numpy())
    # max_f |x_i(f)|: the stored floats, or, aligned, 300 A for every coordinate (the reference's centre is
    # within 110 A of the origin, no atom further than the 100 A box's diagonal from it)
    delta = n_frames * EPS * (np.abs(traj.astype(np.float64)).max(axis=0).reshape(-1) if align is None
                              else np.full(n, 300.0))
    bound = 8.0 * (n + n_frames) * EPS * (m @ np.abs(q)) \
        + n_frames / (n_frames - 1.0) * delta[:, None] * (delta @ np.abs(q))[None, :]
    ratio = np.abs(got - want) / bound
    print(f"symm {align} b={b}: max |dY| = {np.abs(got - want).max():.3e}, max |dY| / bound = {ratio.max():.3e}")
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= bound)
    # a second product reads the records of the first: the same bits
    assert np.array_equal(bits(ops.get(ops.symm(q_d))), bits(got))


# ---- 2. the solver against solver="host" ------------------------------------------
# (n_sel, F, align, input, gathered, exact)
CASES = [(17, 40, None, "hbm", False, False), (17, 40, "average", "hbm", False, False),
         (17, 40, "frame0", "hbm", False, False), (214, 300, None, "hbm", False, False),
         (214, 300, "average", "hbm", False, False), (214, 300, "frame0", "hbm", False, False),
         (214, 300, "average", "host64", False, False), (214, 300, "average", "hbm", True, False),
         (214, 300, "average", "hbm", False, True)]


def pca_input(n_sel, n_frames, kind, gathered):
    import torch
    n_atoms, sel = selection(n_sel, gathered)
    traj = make_traj(n_atoms, n_frames)
    if kind == "hbm":
        return torch.tensor(traj, device="cuda:0"), sel, {}
    return np.array(traj), sel, {"batch_frames": 64}


@pytest.mark.parametrize("n_sel,n_frames,align,kind,gathered,exact", CASES)
def test_matrix_free_against_host(n_sel, n_frames, align, kind, gathered, exact):
    from rmsf_amd import PCA, rmsip
    n, k = 3 * n_sel, 3
    what = f"{n_sel}x{n_frames} {align} {kind} gathered={gathered} exact={exact}"
    x, sel, kw = pca_input(n_sel, n_frames, kind, gathered)
    kw = dict(select=sel, align=align, exact=exact, **kw)
    host = PCA(x, **kw).run()
    free = PCA(x, n_components=k, solver="matrix_free", **kw).run()
    r, h = free.results, host.results
    assert r.covariance is None
    assert r.solver_info["converged"] and r.solver_info["block"] == 16
    print(f"{what}: {r.solver_info['n_iter']} iterations, max residual {r.solver_info['residuals'].max():.3e}")
    assert r.n_frames == n_frames
    assert np.array_equal(bits(r.mean), bits(h.mean)) and np.array_equal(bits(r.rmsf), bits(h.rmsf))
    check_pairs(n, n_frames, h.variance, h.p_components, r.variance, r.p_components, k, what)
    e = TOL + 8.0 * (n + n_frames) * EPS
    dc = np.abs(r.cumulated_variance - h.cumulated_variance[:k])
    print(f"{what}: max |d cumulated| / bound = {dc.max() / ((k + 1) * e):.3e}")
    assert np.all(dc <= (k + 1) * e)
    s = rmsip(r.p_components, h.p_components[:, :k])
    print(f"{what}: 1 - rmsip = {1.0 - s:.3e}")
    assert s >= 1.0 - 1e-9
    # the same call twice: the same bits
    again = PCA(x, n_components=k, solver="matrix_free", **kw).run().results
    assert np.array_equal(bits(again.variance), bits(r.variance))
    assert np.array_equal(bits(again.p_components), bits(r.p_components))
    assert again.solver_info["n_iter"] == r.solver_info["n_iter"]
    # transform() after either solver
    full = host.transform()
    sign = np.sign(np.einsum("ic,ic->c", r.p_components, h.p_components[:, :k]))   # (eigh fixes no sign)
    got, want = free.transform(), full[:, :k] * sign[None, :]
    assert got.shape == (n_frames, k)
    dnorm = np.linalg.norm(full, axis=1)     # |d(f)|_2: the full basis is orthonormal
    g = gaps(h.variance, range(k))
    dv = 2.0 * e * h.variance[0] / g
    # (the kernel's 8 n eps (|d| @ |v|) <= 8 n eps |d|_2 |v|_2 = 8 n eps |d|_2, once per solver)
    bound = dnorm[:, None] * dv[None, :] + 2.0 * 8.0 * n * EPS * dnorm[:, None]
    ratio = np.abs(got - want) / bound
    print(f"{what}: transform max |dP| / bound = {ratio.max():.3e}")
    assert np.all(np.abs(got - want) <= bound)


# ---- 3. the size the matrix cannot have ---------------------------------------------
def test_sixty_thousand_atoms():
    """60,000 atoms x 8 frames: a 5.8 MB trajectory whose covariance would be
    259 GB.  The modes against the dual solution: eigh of the 8 x 8 matrix
    D D^T / (F - 1), v = D^T u / |D^T u|."""
    import torch

    from rmsf_amd import PCA
    n_sel, n_frames, k = 60_000, 8, 3
    n = 3 * n_sel
    traj = make_traj(n_sel, n_frames)
    x = torch.tensor(traj, device="cuda:0")
    with pytest.raises(MemoryError):
        PCA(x, align=None, n_components=k, solver="device").run()
    p = PCA(x, align=None, n_components=k, solver="matrix_free").run()
    r = p.results
    assert r.covariance is None and r.solver_info["converged"]
    assert r.solver_info["rank"] == n_frames - 1
    xs = traj.reshape(n_frames, n).astype(np.float64)
    d = xs - xs.mean(axis=0)
    w, u = np.linalg.eigh(d @ d.T / (n_frames - 1.0))
    w, u = w[::-1].copy(), u[:, ::-1]
    v = d.T @ u[:, :n_frames - 1]
    v /= np.linalg.norm(v, axis=0)
    w_ref = np.concatenate([w[:n_frames - 1], [0.0]])      # the other 3n - 7 eigenvalues are zero
    check_pairs(n, n_frames, w_ref, v, r.variance, r.p_components, k, "60,000 atoms")
    e = TOL + 8.0 * (n + n_frames) * EPS
    cum = np.cumsum(w[:k]) / w[:n_frames - 1].sum()
    assert np.all(np.abs(r.cumulated_variance - cum) <= (k + 1) * e)
    assert p.transform().shape == (n_frames, k)


# ---- 4. refusals ----------------------------------------------------------------------
def test_refusals():
    import torch

    from rmsf_amd import PCA, PCAConvergenceError
    x = torch.tensor(make_traj(17, 40), device="cuda:0")
    kw = dict(n_components=3, solver="matrix_free")
    with pytest.raises(NotImplementedError, match="one device per process"):
        PCA(x, gpus=2, **kw).run()
    with pytest.raises(NotImplementedError, match="one device per process"):
        PCA([x], **kw).run()
    soa = x.permute(0, 2, 1).contiguous()
    with pytest.raises(NotImplementedError, match="planes"):
        PCA(soa, layout="soa", align=None, **kw).run()
    with pytest.raises(PCAConvergenceError, match="rank 0") as ei:
        PCA(x[:1].contiguous(), align=None, **kw).run()
    assert ei.value.info["rank"] == 0 and not ei.value.info["converged"]
    with pytest.raises(PCAConvergenceError, match="rank 2"):        # F - ddof = 2 < k
        PCA(x[:3].contiguous(), align=None, **kw).run()
