"""CPU tier: the matrix-free PCA solver without a device -- the driver of
rmsf_amd/eigen.py over the factored operator ``FactorOps`` (symm(q) =
d.T @ (d @ q) / denom, the numpy twin of ``TrajectoryOps``) against
``numpy.linalg.eigh`` of the matrix it never forms; the host-only workspace
function and the argument checks of csrc/pca_backproject.hip; the argument
checks of ``PCA(solver="matrix_free")``; ``rmsip`` and ``cumulative_overlap``.

Bounds (derived, not measured): those of tests/test_pca_eig_host.py::
check_pairs, restated with e = tol + 8 (3n + F) 2^-52 -- the factored product
has two contractions, of lengths 3n (d @ q) and F (d.T @ .), where the matrix
product has one of length 3n:
  * values: ``|l - l_ref| <= e l_1``;
  * vectors: ``|v - s v_ref|_2 <= 2 e l_1 / gap_i`` (Davis-Kahan);
  * orthonormality: ``|V^T V - I| <= 64 n 2^-52`` elementwise.
"""
import ctypes

import numpy as np
import pytest

TOL = 1e-10
EPS = 2.0 ** -52
MODE_SIGMA = (2.0, 1.4, 1.0)   # A per atom, the three planted modes
NOISE = 0.3


def planted_deviations(n_atoms: int, n_frames: int, seed: int = 0) -> np.ndarray:
    """f64 [F, 3 n_atoms]: the centred coordinates of the planted-mode recipe
    of tests/test_gpu_pca_project.py (base + three collective modes + 0.3 A
    noise, rounded to f32), without its rigid motion."""
    rng = np.random.default_rng(1000 * seed + 7 * n_atoms + n_frames)
    base = rng.uniform(0.0, 100.0, size=(n_atoms, 3))
    modes = rng.normal(size=(3, n_atoms, 3))
    modes /= np.sqrt((modes ** 2).sum(axis=(1, 2), keepdims=True) / n_atoms)
    amp = rng.normal(size=(n_frames, 3)) * np.asarray(MODE_SIGMA)
    x = base + np.einsum("fk,kac->fac", amp, modes) + NOISE * rng.normal(size=(n_frames, n_atoms, 3))
    x = x.astype(np.float32).astype(np.float64).reshape(n_frames, -1)
    return x - x.mean(axis=0)


def gaps(w_ref, idx):
    out = []
    for i in idx:
        d = np.abs(w_ref - w_ref[i])
        d[i] = np.inf
        out.append(d.min())
    return np.asarray(out)


def check_pairs(n, n_frames, w_ref, v_ref, vals, vecs, k, tol=TOL):
    e = (tol + 8.0 * (n + n_frames) * EPS) * w_ref[0]
    assert vals.shape == (k,) and vecs.shape == (n, k) and vals.dtype == vecs.dtype == np.float64
    dv = np.abs(vals - w_ref[:k])
    print(f"n={n} F={n_frames} k={k}: max |dl| / bound = {dv.max() / e:.3e}")
    assert np.all(dv <= e)
    g = gaps(w_ref, range(k))
    for i in range(k):
        s = 1.0 if vecs[:, i] @ v_ref[:, i] >= 0.0 else -1.0
        d = np.linalg.norm(vecs[:, i] - s * v_ref[:, i])
        assert d <= 2.0 * e / g[i], f"vector {i}: |dv| / bound = {d * g[i] / (2.0 * e):.3e}"
    orth = np.abs(vecs.T @ vecs - np.eye(k)).max()
    assert orth <= 64.0 * n * EPS, orth
    j = np.argmax(np.abs(vecs), axis=0)
    assert np.all(vecs[j, np.arange(k)] > 0.0)


# ---- 1. the iteration on the factored operator --------------------------------
@pytest.mark.parametrize("n_atoms,n_frames", [(20, 100), (214, 300)])
def test_factor_ops_against_eigh(n_atoms, n_frames):
    from rmsf_amd.eigen import FactorOps, top_eigenpairs
    d = planted_deviations(n_atoms, n_frames)
    n = 3 * n_atoms
    assert d.shape == (n_frames, n)
    w, v = np.linalg.eigh(d.T @ d / (n_frames - 1))
    ops = FactorOps(d, n_frames - 1)
    assert ops.n == n
    vals, vecs, info = top_eigenpairs(None, 3, ops=ops)
    print(f"{info['n_iter']} iterations, max residual {info['residuals'].max():.3e}")
    assert info["converged"] and info["block"] == 16 and np.all(info["residuals"] <= TOL)
    check_pairs(n, n_frames, w[::-1].copy(), v[:, ::-1].copy(), vals, vecs, 3)
    # the same call again: the same bits
    vals2, vecs2, _ = top_eigenpairs(None, 3, ops=FactorOps(d, n_frames - 1))
    assert np.array_equal(vals, vals2) and np.array_equal(vecs, vecs2)


def test_factor_ops_rank():
    from rmsf_amd import PCAConvergenceError
    from rmsf_amd.eigen import FactorOps, top_eigenpairs
    d = planted_deviations(20, 3)         # F - 1 = 2 < k = 3
    with pytest.raises(PCAConvergenceError, match="rank 2") as ei:
        top_eigenpairs(None, 3, ops=FactorOps(d, 2))
    assert ei.value.info["rank"] == 2 and not ei.value.info["converged"]
    d = planted_deviations(20, 8)         # k = 3 <= F - 1 = 7 < b = 16
    w, v = np.linalg.eigh(d.T @ d / 7.0)
    vals, vecs, info = top_eigenpairs(None, 3, ops=FactorOps(d, 7))
    assert info["converged"] and info["rank"] == 7 and info["block"] == 16
    check_pairs(60, 8, w[::-1].copy(), v[:, ::-1].copy(), vals, vecs, 3)


def test_factor_ops_arguments():
    from rmsf_amd.eigen import FactorOps
    with pytest.raises(ValueError):
        FactorOps(np.zeros(5), 1)
    with pytest.raises(ValueError, match="denom"):
        FactorOps(np.zeros((5, 6)), 0)


# ---- 2. the library's host-only side --------------------------------------------
def _lib():
    from rmsf_amd import _lib
    return _lib.load()


def test_backproject_workspace_bytes():
    ws = _lib().rmsf_pca_backproject_workspace_bytes
    assert ws(256, 100000, 48) == 0                 # many atom tiles: one frame range
    split = ws(5000, 5, 3)                          # one atom tile, 157 stages: frame ranges
    assert split > 0 and split % (8 * 15 * 3) == 0
    assert ws(20000, 214, 16) > 0 and ws(20000, 214, 16) % (8 * 642 * 16) == 0
    for zero in [(0, 5, 3), (5000, 0, 3), (5000, 5, 0)]:
        assert ws(*zero) == 0
    assert ws(5000, 5, 3) == split and ws(5000, 5, 3) == split


def test_backproject_argument_checks_touch_no_device():
    """Every RMSF_EINVAL case returns before any launch: the pointers here are
    host addresses no kernel could read, and no device need exist."""
    from rmsf_amd._lib import RMSF_EINVAL
    lib = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(xyz=p, fstride=15, n_frames=4, n_sel=5, sel=None, xform=None, refinfo=None, mean=p, p=p, ldp=4,
              n_cols=4, y=p, ldy=4, accumulate=0, work=None, work_bytes=0, stream=None)
    bad = [dict(xyz=None), dict(mean=None), dict(p=None), dict(y=None), dict(n_cols=0), dict(n_cols=49, ldp=64, ldy=64),
           dict(ldp=3), dict(ldy=3), dict(xform=p), dict(refinfo=p), dict(n_sel=0), dict(n_frames=-1),
           # a split plan (5,000 frames of 5 atoms) with no workspace, and with one too small
           dict(n_frames=5000, n_cols=3), dict(n_frames=5000, n_cols=3, work=p, work_bytes=8)]
    assert lib.rmsf_pca_backproject_workspace_bytes(5000, 5, 3) > 8
    for change in bad:
        rc = lib.rmsf_pca_backproject(*{**ok, **change}.values())
        assert rc == RMSF_EINVAL, change
        assert b"rmsf_pca_backproject" in lib.rmsf_last_error()
    assert not any(buf)


# ---- 3. PCA(solver="matrix_free") arguments ---------------------------------------
def test_pca_matrix_free_arguments():
    from rmsf_amd import PCA
    x = np.zeros((4, 5, 3), np.float32)
    with pytest.raises(ValueError, match="n_components"):
        PCA(x, solver="matrix_free")
    for bad in (0, 41):
        with pytest.raises(ValueError, match='solver="host"'):
            PCA(x, solver="matrix_free", n_components=bad)
    with pytest.raises(ValueError, match="solver"):
        PCA(x, solver="matrixfree", n_components=3)
    p = PCA(x, solver="matrix_free", n_components=3)
    assert p.solver == "matrix_free" and not p._rmsf.covariance and p._rmsf._keep_last_run
    assert PCA(x)._rmsf.covariance and not PCA(x)._rmsf._keep_last_run


# ---- 4. rmsip and cumulative_overlap ----------------------------------------------
def test_rmsip_and_cumulative_overlap():
    from rmsf_amd import cumulative_overlap, rmsip
    q, _ = np.linalg.qr(np.random.default_rng(4).standard_normal((60, 12)))
    a, b = q[:, :5], q[:, 5:10]
    assert abs(rmsip(a, a) - 1.0) <= 16 * EPS
    # the same subspace in another basis
    rot, _ = np.linalg.qr(np.random.default_rng(5).standard_normal((5, 5)))
    assert abs(rmsip(a, a @ rot) - 1.0) <= 64 * EPS
    assert rmsip(a, b) <= 64 * EPS                      # orthogonal subspaces
    assert abs(rmsip(q, q, n_components=3) - 1.0) <= 16 * EPS
    assert abs(rmsip(a, q[:, :10]) - 1.0) <= 16 * EPS   # a inside the larger span: sum over j of all of a_i
    # by hand: two vectors at 60 degrees in a plane
    u = np.array([[1.0], [0.0]])
    w = np.array([[0.5], [np.sqrt(0.75)]])
    assert abs(rmsip(u, w) - 0.5) <= 4 * EPS
    inside = (a @ np.array([0.3, -1.2, 0.5, 2.0, 0.1]))[:, None]
    assert abs(cumulative_overlap(inside, a) - 1.0) <= 64 * EPS
    assert abs(cumulative_overlap(a, a, 2) - 1.0) <= 64 * EPS
    assert cumulative_overlap(a, b, 0) <= 64 * EPS
    assert abs(cumulative_overlap(inside, a, 0, n_components=2)
               - np.sqrt(0.3 ** 2 + 1.2 ** 2) / np.linalg.norm([0.3, -1.2, 0.5, 2.0, 0.1])) <= 64 * EPS
    for f in (rmsip, cumulative_overlap):
        with pytest.raises(ValueError):
            f(a, q[:59, :5])
        with pytest.raises(ValueError):
            f(a[:, 0], a)
        with pytest.raises(ValueError):
            f(a, a, n_components=6) if f is rmsip else f(a, a, 0, n_components=6)
    with pytest.raises(ValueError):
        cumulative_overlap(a, a, 5)
