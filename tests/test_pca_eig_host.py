"""CPU tier: the device eigen-solver's driver (rmsf_amd/eigen.py) over its
numpy ``ops`` -- the iteration, the stopping rule and the breakdown paths --
against ``numpy.linalg.eigh``; the argument checks of ``PCA(solver=...)`` that
need no library; the host-only workspace functions of csrc/eigen_block.hip.

Bounds (derived, not measured), with e = tol + 8 n 2^-52 and l_1 the largest
eigenvalue:
  * values: ``|l - l_ref| <= e l_1``.  The solver stops at residuals
    |M v - l v| <= tol l_1, and an eigenvalue of a symmetric matrix lies
    within the residual of each Ritz value; 8 n 2^-52 l_1 is the rounding of
    the reference and of the products.
  * vectors: ``|v - s v_ref|_2 <= 2 e l_1 / gap_i``, s = sign(v . v_ref),
    gap_i the distance from l_ref,i to the nearest other reference eigenvalue
    (Davis-Kahan: sin(angle) <= residual / gap; the 2 covers the gap being
    taken between reference values and the chord against the sine).  The
    difference is measured directly: sqrt(1 - dot^2) floors at 5e-8.
  * orthonormality: ``|V^T V - I| <= 64 n 2^-52`` elementwise.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

TOL = 1e-10
EPS = 2.0 ** -52


def power_law(n, seed=1):
    """M = U diag(100 (1 + i)^-2) U^T, symmetrised; (M, descending values, vectors)."""
    return designed(100.0 * (1.0 + np.arange(n)) ** -2.0, seed)


def designed(lam, seed=1):
    lam = np.asarray(lam, dtype=np.float64)
    n = lam.size
    u, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))
    m = (u * lam[None, :]) @ u.T
    m = 0.5 * (m + m.T)
    w, v = np.linalg.eigh(m)
    return m, w[::-1].copy(), v[:, ::-1].copy()


def gaps(w_ref, idx):
    """Distance from each w_ref[idx] to the nearest other reference value."""
    out = []
    for i in idx:
        d = np.abs(w_ref - w_ref[i])
        d[i] = np.inf
        out.append(d.min())
    return np.asarray(out)


def check_pairs(m, w_ref, v_ref, vals, vecs, k, tol=TOL, skip=()):
    """The three bounds of the module docstring; ``skip``: indices whose
    vectors are checked elsewhere (a degenerate cluster)."""
    n = m.shape[0]
    e = (tol + 8.0 * n * EPS) * w_ref[0]
    assert vals.shape == (k,) and vecs.shape == (n, k) and vals.dtype == vecs.dtype == np.float64
    dv = np.abs(vals - w_ref[:k])
    print(f"n={n} k={k}: max |dl| / bound = {dv.max() / e:.3e}")
    assert np.all(dv <= e)
    g = gaps(w_ref, range(k))
    for i in range(k):
        if i in skip:
            continue
        s = 1.0 if vecs[:, i] @ v_ref[:, i] >= 0.0 else -1.0
        d = np.linalg.norm(vecs[:, i] - s * v_ref[:, i])
        assert d <= 2.0 * e / g[i], f"vector {i}: |dv| / bound = {d * g[i] / (2.0 * e):.3e}"
    orth = np.abs(vecs.T @ vecs - np.eye(k)).max()
    assert orth <= 64.0 * n * EPS, orth
    check_signs(vecs)


def check_signs(vecs):
    j = np.argmax(np.abs(vecs), axis=0)
    assert np.all(vecs[j, np.arange(vecs.shape[1])] > 0.0)


def comoment_of_few_frames():
    """51 x 51, rank 9: the co-moment of 10 frames of 17 atoms."""
    x = np.random.default_rng(3).standard_normal((10, 51))
    d = x - x.mean(axis=0)
    return d.T @ d


@pytest.mark.parametrize("n,k,block", [(48, 3, 16), (51, 5, 16), (99, 20, 32), (642, 10, 32), (642, 40, 48)])
def test_power_law_against_eigh(n, k, block):
    from rmsf_amd.eigen import NumpyOps, block_width, top_eigenpairs
    assert block_width(n, k) == block
    m, w_ref, v_ref = power_law(n)
    vals, vecs, info = top_eigenpairs(m, k, ops=NumpyOps(m))
    print(f"n={n} k={k}: {info['n_iter']} iterations, max residual {info['residuals'].max():.3e}")
    assert info["converged"] and 1 <= info["n_iter"] <= 300 and info["block"] == block
    assert info["residuals"].shape == (k,) and np.all(info["residuals"] <= TOL)
    assert info["rank"] == block
    check_pairs(m, w_ref, v_ref, vals, vecs, k)


@pytest.mark.parametrize("k", [3, 9])
def test_rank_deficient_converges(k):
    from rmsf_amd.eigen import top_eigenpairs
    m = comoment_of_few_frames()
    w, v = np.linalg.eigh(m)
    vals, vecs, info = top_eigenpairs(m, k, block=16)
    assert info["converged"] and info["rank"] == 9 and info["block"] == 16 and info["n_iter"] <= 3
    check_pairs(m, w[::-1].copy(), v[:, ::-1].copy(), vals, vecs, k)


def test_rank_deficient_raises_past_the_rank():
    from rmsf_amd import PCAConvergenceError
    from rmsf_amd.eigen import top_eigenpairs
    with pytest.raises(PCAConvergenceError, match="asked for 10 components, the matrix has rank 9") as ei:
        top_eigenpairs(comoment_of_few_frames(), 10, block=16)
    assert ei.value.info["rank"] == 9 and not ei.value.info["converged"]
    assert 'solver="host"' in str(ei.value)
    assert isinstance(ei.value, RuntimeError)


def test_zero_matrix_raises():
    from rmsf_amd.eigen import PCAConvergenceError, top_eigenpairs
    with pytest.raises(PCAConvergenceError, match="rank 0") as ei:
        top_eigenpairs(np.zeros((51, 51)), 3)
    assert ei.value.info["rank"] == 0


def test_matrix_smaller_than_a_tile():
    from rmsf_amd.eigen import block_width, top_eigenpairs
    m, w_ref, v_ref = designed([9.0, 4.0, 2.0, 1.0, 0.5, 0.1], seed=2)
    assert block_width(6, 2) == 6
    vals, vecs, info = top_eigenpairs(m, 2)
    assert info["converged"] and info["n_iter"] == 1 and info["block"] == 6
    check_pairs(m, w_ref, v_ref, vals, vecs, 2)
    with pytest.raises(ValueError, match='solver="host"'):
        top_eigenpairs(m, 7)


def degenerate_case(n=60):
    lam = np.concatenate([[100.0, 50.0, 50.0, 10.0], 1.0 / (1.0 + np.arange(n - 4))])
    return designed(lam, seed=4)


def check_degenerate_pair(m, w_ref, v_ref, vals, vecs, tol=TOL):
    """Values and the simple vectors by the bounds; the pair (1, 2) as a
    subspace: |P - P_ref|_2 within the vector bound with the gap taken from
    the cluster to its neighbours."""
    n = m.shape[0]
    check_pairs(m, w_ref, v_ref, vals, vecs, 4, tol, skip=(1, 2))
    e = (tol + 8.0 * n * EPS) * w_ref[0]
    gap = min(w_ref[0] - w_ref[1], w_ref[2] - w_ref[3])
    p = vecs[:, 1:3] @ vecs[:, 1:3].T
    p_ref = v_ref[:, 1:3] @ v_ref[:, 1:3].T
    d = np.linalg.norm(p - p_ref, 2)
    assert d <= 2.0 * e / gap, d * gap / (2.0 * e)


def test_degenerate_pair_inside_the_top_k():
    from rmsf_amd.eigen import top_eigenpairs
    m, w_ref, v_ref = degenerate_case()
    vals, vecs, info = top_eigenpairs(m, 4)
    assert info["converged"]
    check_degenerate_pair(m, w_ref, v_ref, vals, vecs)


def test_max_iter_reached():
    from rmsf_amd.eigen import PCAConvergenceError, top_eigenpairs
    m, _, _ = power_law(99)
    with pytest.raises(PCAConvergenceError, match="max_iter") as ei:
        top_eigenpairs(m, 20, max_iter=1)
    info = ei.value.info
    assert info["converged"] is False and info["n_iter"] == 1
    assert 'solver="host"' in str(ei.value) and "flat tail" in str(ei.value)


def test_same_call_same_bits():
    from rmsf_amd.eigen import top_eigenpairs
    m, _, _ = power_law(99)
    a = top_eigenpairs(m, 20)
    b = top_eigenpairs(m, 20)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    assert a[2]["n_iter"] == b[2]["n_iter"]
    check_signs(a[1])
    c = top_eigenpairs(m, 20, seed=1)
    assert c[2]["converged"]


def test_sign_rule_takes_the_first_on_ties():
    from rmsf_amd.eigen import fix_signs
    v = np.array([[-0.5, 0.5], [0.5, -0.5], [0.1, 0.7]])
    out = fix_signs(v)
    assert np.array_equal(out[:, 0], [0.5, -0.5, -0.1]) and np.array_equal(out[:, 1], v[:, 1])


def test_argument_checks_need_no_library(monkeypatch):
    """ValueError from the host checks alone: loading the library is made an
    error for the duration."""
    from rmsf_amd import PCA, _lib
    from rmsf_amd.eigen import top_eigenpairs

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the argument check")
    monkeypatch.setattr(_lib, "load", no_load)
    x = np.zeros((4, 20, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="solver"):
        PCA(x, solver="gpu", n_components=3)
    with pytest.raises(ValueError, match='solver="host"'):
        PCA(x, solver="device", n_components=41)
    with pytest.raises(ValueError, match="n_components"):
        PCA(x, solver="device")
    with pytest.raises(ValueError, match='solver="host"'):
        top_eigenpairs(np.eye(100), 41)
    p = PCA(x, solver="device", n_components=3, tol=1e-9, max_iter=50, seed=2)
    assert (p.solver, p.tol, p.max_iter, p.seed) == ("device", 1e-9, 50, 2)
    assert PCA(x).solver == "host"


def test_workspace_functions():
    from rmsf_amd import _lib
    lib = _lib.load()
    symm, gram = lib.rmsf_symm_block_workspace_bytes, lib.rmsf_block_gram_workspace_bytes
    # degenerate shapes (and blocks no kernel takes) ask for nothing
    assert symm(0, 16) == 0 and symm(642, 0) == 0 and symm(642, 49) == 0
    assert gram(0, 16, 16) == 0 and gram(642, 0, 16) == 0 and gram(642, 16, 0) == 0 and gram(642, 49, 1) == 0
    # one range: no workspace
    assert symm(51, 16) == 0 and gram(51, 16, 16) == 0 and symm(1, 1) == 0
    # a split plan: n_ks partials of the result
    for n in (642, 2000):
        for c in (1, 16, 17, 33, 48):
            need = symm(n, c)
            assert need > 0 and need % (n * c * 8) == 0 and need // (n * c * 8) > 1
    need = gram(642, 48, 48)
    assert need > 0 and need % (48 * 48 * 8) == 0
    shapes = [(642, 48), (10023, 48), (10023, 16), (2000, 33), (48, 48), (1, 1)]
    first = [symm(*s) for s in shapes] + [gram(n, c, c) for n, c in shapes]
    for _ in range(3):
        assert [symm(*s) for s in shapes] + [gram(n, c, c) for n, c in shapes] == first


def test_symbols_in_header_and_binding():
    from rmsf_amd import _lib
    with open(os.path.join(ROOT, "include", "rmsf_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in ("rmsf_symm_block_workspace_bytes", "rmsf_symm_block", "rmsf_block_gram_workspace_bytes",
                 "rmsf_block_gram", "rmsf_block_update"):
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "symmetric in its bits" in header
