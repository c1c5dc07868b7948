"""CPU tier of ``DiffusionMap(solver="device")``: what it refuses before a
device is touched, the library's two new entry points, the driver over
``ScaledOps`` (the numpy twin of the device operator) against the host path's
``eigh``, and the default ``solver="host"`` against a literal restatement of
its formulae.

The planted cases are those of tests/test_gpu_diffusion.py (tests/diffusion_cases.py);
what that file needs of them is asserted here, on the CPU: the driver
converges with k = 3 in under 50 iterations, and the first four eigenvalues
(and the fifth) are at least 1e-3 apart."""
import numpy as np
import pytest

import diffusion_cases as C

NEW_SYMBOLS = ("rmsf_diffusion_kernel", "rmsf_block_scale_rows")


def test_library_exports_the_diffusion_entry_points():
    from rmsf_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.rmsf_abi_version() == _lib.ABI_VERSION == 4        # additive: the version stays


def test_launchers_refuse_bad_arguments_without_a_device():
    """The argument checks come before any launch: RMSF_EINVAL and a message,
    with pointers that are never followed."""
    from rmsf_amd import _lib
    lib = _lib.load()
    p, q = 4096, 8192                                             # stand-ins for device addresses
    for args in [(None, 8, 8, 1.0, q, None), (p, 8, 8, 1.0, None, None), (p, 8, 0, 1.0, q, None),
                 (p, 7, 8, 1.0, q, None), (p, 8, 8, 0.0, q, None), (p, 8, 8, -1.0, q, None),
                 (p, 8, 8, float("inf"), q, None), (p, 8, 8, float("nan"), q, None)]:
        assert lib.rmsf_diffusion_kernel(*args) == _lib.RMSF_EINVAL, args
        assert b"rmsf_diffusion_kernel" in lib.rmsf_last_error()
    for args in [(None, p, 8, 8, 8, q, 8, None), (p, None, 8, 8, 8, q, 8, None), (p, p, 8, 8, 8, None, 8, None),
                 (p, p, 8, 0, 8, q, 8, None), (p, p, 8, 8, 0, q, 8, None), (p, p, 49, 8, 49, q, 49, None),
                 (p, p, 7, 8, 8, q, 8, None), (p, p, 8, 8, 8, q, 7, None)]:
        assert lib.rmsf_block_scale_rows(*args) == _lib.RMSF_EINVAL, args
        assert b"rmsf_block_scale_rows" in lib.rmsf_last_error()


def test_device_solver_arguments_are_checked_before_a_device_is_touched():
    from rmsf_amd import DiffusionMap
    d = C.numpy_distances("states", 130)
    for kw in (dict(solver="device"),                              # k missing
               dict(solver="device", n_eigenvectors=0),
               dict(solver="device", n_eigenvectors=40),
               dict(solver="cuda", n_eigenvectors=3),              # unknown solver
               dict(solver="device", n_eigenvectors=3, max_iter=0)):
        with pytest.raises(ValueError):
            DiffusionMap(d, epsilon=2.0, **kw)
    with pytest.raises(ValueError):
        DiffusionMap(d, epsilon=float("inf"), solver="device", n_eigenvectors=3)
    for k in (1, 39):
        dm = DiffusionMap(d, 2.0, n_eigenvectors=k, solver="device", tol=1e-9, max_iter=10, seed=1, device=None)
        assert dm.n_eigenvectors == k and dm.solver == "device"
    assert DiffusionMap(d).solver == "host"
    with pytest.raises(TypeError):                                 # the new parameters are keyword-only
        DiffusionMap(d, 2.0, 3)


@pytest.mark.parametrize("kind,n", C.CASES)
def test_driver_over_scaled_ops_reproduces_eigh(kind, n):
    from rmsf_amd.eigen import ScaledOps, top_eigenpairs
    d = C.numpy_distances(kind, n)
    eps = C.epsilon_of(kind, d)
    w, right, sym, rs, v = C.host_formulae(d, eps)
    gaps = -np.diff(w[:C.K + 2])
    print(f"{kind} {n}: eigenvalues {w[:C.K + 2]}, least gap {gaps.min():.3e}")
    assert gaps.min() >= 1e-3                                      # what the eigenvector comparisons on the device need
    kern = np.exp(-(d * d) / eps)
    ops = ScaledOps(kern, rs)
    q = np.random.default_rng(0).standard_normal((n, 5))
    np.testing.assert_allclose(ops.symm(q), sym @ q, rtol=0, atol=64 * n * 2.0 ** -52 * np.abs(q).max())
    lam, vec, info = top_eigenpairs(None, C.K + 1, ops=ops)
    print(f"{kind} {n}: {info['n_iter']} iterations, max |dlambda| {np.abs(lam - w[:C.K + 1]).max():.3e}")
    assert info["converged"] and info["n_iter"] < 50
    assert np.abs(lam - w[:C.K + 1]).max() <= 1e-9
    assert np.linalg.norm(sym @ vec - vec * lam, axis=0).max() <= 1e-9     # the conjugate residual |S v - l v|
    for i in range(C.K + 1):                                       # Davis-Kahan, the gap from the host spectrum
        gap = min(gaps[i], gaps[i - 1]) if i else gaps[0]
        assert np.linalg.norm(C.aligned(vec, v[:, :C.K + 1])[:, i] - v[:, i]) <= 1e-9 / gap
    with pytest.raises(ValueError):
        ScaledOps(kern, rs[:-1])


def test_host_solver_is_today_s_formulae_bit_for_bit():
    from rmsf_amd import DiffusionMap
    d = C.numpy_distances("states", 130)
    eps = C.epsilon_of("states", d)
    w, right = C.host_formulae(d, eps)[:2]
    for kw in ({}, dict(solver="host"), dict(solver="host", n_eigenvectors=3, tol=1.0, max_iter=1, seed=9)):
        dm = DiffusionMap(d, epsilon=eps, **kw).run()
        r = dm.results
        assert r.eigenvalues.shape == (130,) and r.eigenvectors.shape == (130, 130) and r.n_frames == 130
        assert np.array_equal(r.eigenvalues.view(np.uint64), w.view(np.uint64))
        assert np.array_equal(r.eigenvectors.view(np.uint64), right.view(np.uint64))
        assert "solver_info" not in r
        assert np.array_equal(dm.transform(2, 1.0), right[:, 1:3] * w[1:3] ** 1.0)
    with pytest.raises(ValueError, match="1..129"):
        dm.transform(130, 1.0)
