"""CPU tier of TICA: the lagged co-moment entry points of the library, their
host-only plan and argument checks, and the pure-numpy generalised
eigen-solve ``tica_from_comoments`` against ``scipy.linalg.eigh(C_lag, C0)``.

``make_lagged_traj`` is the generator of this file and of
tests/test_gpu_tica.py: tests/test_gpu_covariance.py's construction (base
positions in a 100 A box, planted collective modes of unit displacement per
atom, 0.3 A noise, a random rigid motion per frame, f32) with amplitudes that
are correlated in time -- three AR(1) modes and a rotating pair (cos wt,
sin wt), which makes S - S^T a tenth of the signal and more, so a transposed
lagged matrix cannot pass.
"""
import ctypes
import functools

import numpy as np
import pytest

NEW_SYMBOLS = ("rmsf_lagged_comoment_workspace_bytes", "rmsf_lagged_comoment_accumulate",
               "rmsf_lagged_comoment_finish")

AR_PHI = (0.98, 0.9, 0.6)      # the three AR(1) modes' one-step autocorrelation
AR_SIGMA = (2.0, 1.4, 1.0)     # ... and stationary amplitude, A per atom
# the rotating pair (modes 4 and 5: cos wt, sin wt).  A pair of equal strength has one double eigenvalue, cos(w lag);
# the second member is kept near the noise so that the pair splits and the third eigenvalue stands clear of the fourth
ROT_SIGMA = (2.0, 0.12)
ROT_OMEGA = 2.0 * np.pi / 29.0
NOISE = 0.3


@functools.lru_cache(maxsize=None)
def make_lagged_traj(n_atoms: int, n_frames: int, seed: int = 0, rigid: bool = True) -> np.ndarray:
    """f32 [F, n_atoms, 3]: base + sum_k a_k(t) mode_k + noise, then (``rigid``)
    a random rotation about the centroid and a translation per frame."""
    rng = np.random.default_rng(1000 * seed + 7 * n_atoms + n_frames + 5)
    base = rng.uniform(0.0, 100.0, size=(n_atoms, 3))
    modes = rng.normal(size=(5, n_atoms, 3))
    modes /= np.sqrt((modes ** 2).sum(axis=(1, 2), keepdims=True) / n_atoms)   # unit displacement per atom
    phi, sigma = np.asarray(AR_PHI), np.asarray(AR_SIGMA)
    amp = np.empty((n_frames, 5))
    a = rng.normal(size=3) * sigma                                              # the stationary distribution
    for t in range(n_frames):
        amp[t, :3] = a
        a = phi * a + np.sqrt(1.0 - phi * phi) * sigma * rng.normal(size=3)
    phase = ROT_OMEGA * np.arange(n_frames) + rng.uniform(0.0, 2.0 * np.pi)
    amp[:, 3], amp[:, 4] = ROT_SIGMA[0] * np.cos(phase), ROT_SIGMA[1] * np.sin(phase)
    x = base + np.einsum("fk,kac->fac", amp, modes) + NOISE * rng.normal(size=(n_frames, n_atoms, 3))
    if rigid:
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


def reversible_comoments(x: np.ndarray, lag: int):
    """The estimator of rmsf_amd/tica.py's docstring in numpy f64, on frames
    x [F, n, 3] as they are: ``(M0, M_lag, mu [3n])`` with M = 2N C."""
    d = x.reshape(len(x), -1).astype(np.float64)
    shift = d[0].copy()
    d = d - shift
    n_pairs = len(d) - lag
    a, b = d[:n_pairs], d[lag:]
    t = a.sum(axis=0) + b.sum(axis=0)
    tt = np.outer(t, t) / (2.0 * n_pairs)
    m0 = a.T @ a + b.T @ b - tt
    s = a.T @ b
    return m0, s + s.T - tt, shift + t / (2.0 * n_pairs)


def test_library_exports_the_lagged_entry_points():
    from rmsf_amd import TICA, _lib, tica_from_comoments  # noqa: F401  (the public names exist)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    from rmsf_amd.engine import Engine
    for name in ("lagged_comoment_workspace_bytes", "lagged_comoment_accumulate", "lagged_comoment_finish"):
        assert callable(getattr(Engine, name))


def test_workspace_bytes_on_the_host():
    """0 = the results go straight to d_s: no size, enough tiles of the full
    square to fill the device, or one stage of pairs."""
    from rmsf_amd import _lib
    wb = _lib.load().rmsf_lagged_comoment_workspace_bytes
    assert wb(0, 10) == 0 and wb(-1, 10) == 0 and wb(10, 0) == 0 and wb(10, -3) == 0
    assert wb(214, 1) == 0 and wb(214, 32) == 0           # one stage of 32 pairs: no split-K
    assert wb(214, 33) > 0 and wb(214, 33) % 8 == 0
    assert wb(214, 19990) > 0 and wb(214, 19990) % 8 == 0
    assert wb(214, 19990) == wb(214, 19990)               # a function of the sizes alone
    # 23 x 23 = 529 tiles are over the 512 workgroups the plan aims at; 22 x 22 = 484 leave one range
    assert wb(368, 39) == 0 and wb(368, 100000) == 0
    assert wb(352, 100000) == 0 and wb(3341, 4086) == 0
    # split-K partials: whole 48 x 48 tiles of the full square, nothing else
    for n_sel, n_pairs in ((214, 35), (214, 19990), (33, 33), (17, 33), (1, 5000)):
        n_tiles = -(-n_sel // 16)
        assert wb(n_sel, n_pairs) % (8 * n_tiles * n_tiles * 48 * 48) == 0, (n_sel, n_pairs)
        n_ks = wb(n_sel, n_pairs) // (8 * n_tiles * n_tiles * 48 * 48)
        assert 2 <= n_ks <= min(-(-n_pairs // 32), 512 // (n_tiles * n_tiles))
    # the covariance plan is its own and has not moved
    assert _lib.load().rmsf_covariance_workspace_bytes(214, 67) == 5822208


def test_argument_checks_come_before_any_launch():
    from rmsf_amd import _lib
    lib = _lib.load()
    acc, fin, err = lib.rmsf_lagged_comoment_accumulate, lib.rmsf_lagged_comoment_finish, lib.rmsf_last_error
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fail first

    def call(xa=one, sa=3, xb=one, sb=3, n_pairs=1, n_sel=1, sel=None, fa=None, fb=None, info=None, shift=one, s=one,
             ld=3, work=None, wbytes=0):
        return acc(xa, sa, xb, sb, n_pairs, n_sel, sel, fa, fb, info, shift, s, ld, work, wbytes, None)

    for bad in (dict(xa=None), dict(xb=None), dict(shift=None), dict(s=None), dict(n_sel=0), dict(n_pairs=-1),
                dict(n_sel=2, ld=5), dict(sa=-1), dict(sb=-1)):
        assert call(**bad) == _lib.RMSF_EINVAL, bad
        assert b"rmsf_lagged_comoment_accumulate" in err(), bad
    # records: both operands' and the reference record, or none of the three
    for bad in (dict(fa=one), dict(fb=one), dict(fa=one, fb=one), dict(info=one), dict(fa=one, info=one),
                dict(fb=one, info=one)):
        assert call(**bad) == _lib.RMSF_EINVAL, bad
        assert b"rmsf_lagged_comoment_accumulate" in err() and b"go together" in err(), bad
    # a workspace that is missing or too small
    need = lib.rmsf_lagged_comoment_workspace_bytes(214, 35)
    assert need > 0
    for kw in (dict(), dict(work=one, wbytes=need - 8)):
        assert call(n_pairs=35, n_sel=214, sa=642, sb=642, ld=642, **kw) == _lib.RMSF_ENOMEM
        assert b"rmsf_lagged_comoment_accumulate" in err() and b"workspace" in err()
    assert call(n_pairs=0) == _lib.RMSF_OK                  # nothing to do, nothing launched
    assert call(n_pairs=0, s=None) == _lib.RMSF_EINVAL       # ... but the arguments are still checked
    for args in ((None, 3, one, 3, 2), (one, 3, None, 3, 2), (one, 2, one, 3, 2), (one, 3, one, 0, 2)):
        assert fin(*args, None) == _lib.RMSF_EINVAL, args
        assert b"rmsf_lagged_comoment_finish" in err()
    assert fin(one, 3, one, 3, 0, None) == _lib.RMSF_EEMPTY
    assert b"rmsf_lagged_comoment_finish" in err()


# ---- tica_from_comoments ----------------------------------------------------
LAG = 5


@functools.lru_cache(maxsize=None)
def full_rank_problem():
    """36 coordinates, 600 frames of the generator, unaligned and without the
    rigid motion, lag 5: (M0, M_lag, N)."""
    x = make_lagged_traj(12, 600, rigid=False)
    m0, mt, _ = reversible_comoments(x, LAG)
    return m0, mt, len(x) - LAG


def test_the_generator_is_not_time_reversible():
    """S - S^T is of the order of the signal: what makes a transposed lagged
    matrix fail the GPU tier's bounds."""
    x = make_lagged_traj(12, 600, rigid=False)
    d = x.reshape(600, -1).astype(np.float64)
    d -= d.mean(axis=0)
    s = d[:-LAG].T @ d[LAG:]
    assert np.abs(s - s.T).max() >= 0.1 * np.abs(s).max()


def test_tica_from_comoments_matches_scipy_on_a_full_rank_problem():
    import scipy.linalg

    from rmsf_amd import tica_from_comoments
    m0, mt, n_pairs = full_rank_problem()
    c0, ct = m0 / (2.0 * n_pairs), mt / (2.0 * n_pairs)
    s = np.linalg.eigvalsh(c0)
    assert s[-1] / s[0] < 1e4, "cond(C0): the eigenvalues' error is ~1e-12 then"
    w_ref, v_ref = scipy.linalg.eigh(ct, c0)
    w_ref, v_ref = w_ref[::-1], v_ref[:, ::-1]
    w, ts, v, kv, rank = tica_from_comoments(m0, mt, n_pairs, LAG)
    assert rank == 36 and w.shape == (36,) and v.shape == (36, 36) and ts.shape == (36,) and kv.shape == (36,)
    assert np.all(np.diff(w) <= 0)
    print(f"max |lambda - scipy| = {np.abs(w - w_ref).max():.3e}, lambda[:6] = {w[:6]}")
    assert np.abs(w - w_ref).max() <= 1e-9
    np.testing.assert_allclose(v.T @ c0 @ v, np.eye(36), atol=1e-9)          # V^T C0 V = I
    cross = np.abs(v[:, :3].T @ c0 @ v_ref[:, :3])
    assert np.abs(cross - np.eye(3)).max() <= 1e-7
    j = np.argmax(np.abs(v), axis=0)
    assert np.all(v[j, np.arange(36)] > 0)                                  # eigen.fix_signs
    # truncation of the output keeps the leading ones and the share of the whole
    w3, ts3, v3, kv3, rank3 = tica_from_comoments(m0, mt, n_pairs, LAG, n_components=3)
    assert rank3 == 36 and v3.shape == (36, 3)
    np.testing.assert_array_equal(w3, w[:3])
    np.testing.assert_array_equal(v3, v[:, :3])
    np.testing.assert_array_equal(kv3, kv[:3])
    assert kv3[-1] < 1.0 and kv[-1] == pytest.approx(1.0, abs=1e-14)


def test_truncation_handles_the_null_directions():
    """Six directions projected out of both matrices, as the optimal fit's
    constraints do: rank = 3n - 6 and the eigenvalues are scipy's on the
    reduced basis."""
    import scipy.linalg

    from rmsf_amd import tica_from_comoments
    m0, mt, n_pairs = full_rank_problem()
    rng = np.random.default_rng(3)
    q, _ = np.linalg.qr(rng.normal(size=(36, 36)))
    null, basis = q[:, :6], q[:, 6:]
    p = np.eye(36) - null @ null.T
    w, _, v, _, rank = tica_from_comoments(p @ m0 @ p, p @ mt @ p, n_pairs, LAG)
    assert rank == 30 and w.shape == (30,) and v.shape == (36, 30)
    w_ref = scipy.linalg.eigh(basis.T @ mt @ basis, basis.T @ m0 @ basis, eigvals_only=True)[::-1]
    print(f"reduced basis: max |lambda - scipy| = {np.abs(w - w_ref).max():.3e}")
    assert np.abs(w - w_ref).max() <= 1e-9
    assert np.abs(null.T @ v).max() <= 1e-9                  # the components stay out of the null space
    with pytest.raises(ValueError, match="rank"):
        tica_from_comoments(p @ m0 @ p, p @ mt @ p, n_pairs, LAG, n_components=31)
    tica_from_comoments(p @ m0 @ p, p @ mt @ p, n_pairs, LAG, n_components=30)


def test_timescales_kinetic_variance_and_refusals():
    from rmsf_amd import TICA, tica_from_comoments
    # C0 = I / 2N-free: M0 = 2N I, M_lag = 2N diag(lambda)
    lam = np.array([1.0, 0.9, 0.5, 0.0, -0.25, -1.5])
    n_pairs, lag = 50, 7
    w, ts, v, kv, rank = tica_from_comoments(2 * n_pairs * np.eye(6), 2 * n_pairs * np.diag(lam), n_pairs, lag)
    order = np.argsort(lam)[::-1]
    np.testing.assert_allclose(w, lam[order], atol=1e-15)
    assert rank == 6
    expect = np.array([np.inf, -lag / np.log(0.9), -lag / np.log(0.5), np.nan, -lag / np.log(0.25), np.inf])
    np.testing.assert_allclose(ts, expect, rtol=1e-12)       # (nan == nan and inf == inf here)
    l2 = lam[order] ** 2
    np.testing.assert_allclose(kv, np.cumsum(l2) / l2.sum(), rtol=1e-14)
    np.testing.assert_allclose(np.abs(v), np.eye(6)[:, order], atol=1e-15)
    eye = np.eye(4)
    for bad in (dict(n_pairs=0), dict(lag=0), dict(n_components=0), dict(n_components=5), dict(epsilon=0.0),
                dict(epsilon=1.0)):
        kw = dict(n_pairs=10, lag=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            tica_from_comoments(eye, eye, **kw)
    with pytest.raises(ValueError):
        tica_from_comoments(np.zeros((3, 4)), np.zeros((3, 4)), 10, 1)
    with pytest.raises(ValueError):
        tica_from_comoments(eye, np.eye(5), 10, 1)
    # the estimator's own refusals that need no device
    x = np.zeros((6, 5, 3), np.float32)
    for lag_bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="lag"):
            TICA(x, lag_bad)
    with pytest.raises(ValueError, match="n_components"):
        TICA(x, 1, n_components=0)
    with pytest.raises(NotImplementedError, match="TICA"):
        TICA(x, 1, gpus=2).run()
    with pytest.raises(NotImplementedError, match="TICA"):
        TICA([x, x], 1).run()
