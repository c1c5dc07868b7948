"""GPU tier: the block products of the device eigen-solver
(csrc/eigen_block.hip, f64 MFMA), ``top_eigenpairs`` over them, and
``PCA(solver="device")`` end to end, against numpy f64.

Bounds (derived, not measured):
  * kernels, per element: ``8 * K * 2^-52 * (|A| @ |B|)`` with K the length
    of the contraction -- the f64 dot-product error bound (K terms, unit
    roundoff 2^-53 doubled), times 8 for the kernel's summation order (4 waves,
    MFMA k-steps, split-K fold), the form tests/test_gpu_pca_project.py uses;
    ``rmsf_block_update`` adds one rounding of ``alpha A + (B T)``.
  * eigenpairs: those of tests/test_pca_eig_host.py, restated in
    ``check_pairs``: with e = tol + 8 n 2^-52, ``|l - l_ref| <= e l_1``,
    ``|v - s v_ref|_2 <= 2 e l_1 / gap_i`` and ``|V^T V - I| <= 64 n 2^-52``.
  * ``cumulated_variance``: ``k tol + 64 n 2^-52`` -- k values each within
    tol of the total, and the rounding of two n-term sums.

Trajectories: the planted-mode recipe of tests/test_gpu_pca_project.py,
restated -- base positions in a 100 A box, three collective modes of 2.0, 1.4
and 1.0 A plus 0.3 A noise, a random rigid motion per frame, f32.  Three
components are asked for: the gap behind the third mode is wide.
"""
import functools

import numpy as np
import pytest

import conftest  # noqa: F401  (import paths)

pytestmark = pytest.mark.gpu

TOL = 1e-10
EPS = 2.0 ** -52
SENTINEL = -7.25e77
NS = [1, 6, 47, 48, 49, 51, 642, 2000]


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint64)


def engine():
    import torch

    from rmsf_amd.engine import Engine
    return Engine(torch.device("cuda", 0))


def padded(a: np.ndarray, pad_cols: int, fill: float, pad_rows: int = 0):
    """``a`` in the top left corner of a wider (and longer) HBM tensor full of ``fill``."""
    import torch
    t = torch.full((a.shape[0] + pad_rows, a.shape[1] + pad_cols), fill, dtype=torch.float64, device="cuda:0")
    t[:a.shape[0], :a.shape[1]] = torch.tensor(a, device="cuda:0")
    return t


def assert_within(got, want, bound, what):
    ratio = np.abs(got - want) / np.maximum(bound, np.finfo(np.float64).tiny)
    print(f"{what}: max |d| / bound = {ratio.max():.3e}")
    assert np.all(np.isfinite(got)), f"{what}: non-finite result"
    assert np.all(np.abs(got - want) <= bound), f"{what}: max |d| / bound = {ratio.max():.3e}"


# ---- 1. the kernels against numpy, through Engine ----------------------------
@functools.lru_cache(maxsize=None)
def symmetric(n: int) -> np.ndarray:
    a = np.random.default_rng(n).standard_normal((n, n))
    m = a + a.T
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def block(n: int, cols: int, seed: int = 0) -> np.ndarray:
    b = np.random.default_rng(1000 * seed + 7 * n + cols).standard_normal((n, cols))
    b.setflags(write=False)
    return b


def scratch(eng, need):
    return eng.empty(need // 8) if need else None


@pytest.mark.parametrize("cols", [1, 16, 17, 33, 48])
@pytest.mark.parametrize("n", NS)
def test_symm_block(n, cols):
    import torch
    eng = engine()
    m, q = symmetric(n), block(n, cols)
    need = eng.symm_block_workspace_bytes(n, cols)
    if n >= 642:   # more than one k-range: the fold launch is exercised
        assert need > 0 and need // (8 * n * cols) > 1
    md, qd = padded(m, 3, float("nan")), padded(q, 5, float("nan"))
    outs = []
    for _ in range(2):
        y = padded(np.zeros((n, cols)), 4, SENTINEL, pad_rows=2)
        y[:n, :cols] = SENTINEL
        eng.symm_block(md, n, qd, cols, y, scratch(eng, need))
        torch.cuda.synchronize()
        outs.append(y.cpu().numpy())
    got = outs[0]
    assert_within(got[:n, :cols], m @ q, 8.0 * n * EPS * (np.abs(m) @ np.abs(q)), f"symm {n}x{cols}")
    assert np.all(got[:n, cols:] == SENTINEL) and np.all(got[n:] == SENTINEL), "the padding of Y was written"
    assert np.array_equal(bits(outs[0]), bits(outs[1]))


@pytest.mark.parametrize("na,nb", [(16, 16), (17, 33), (48, 48), (3, 48)])
@pytest.mark.parametrize("n", NS)
def test_block_gram(n, na, nb):
    import torch
    eng = engine()
    a, b = block(n, na, 1), block(n, nb, 2)
    need = eng.block_gram_workspace_bytes(n, na, nb)
    if n >= 642:
        assert need > 0
    ad, bd = padded(a, 2, float("nan")), padded(b, 7, float("nan"))
    outs = []
    for _ in range(2):
        g = padded(np.full((na, nb), SENTINEL), 3, SENTINEL, pad_rows=1)
        eng.block_gram(ad, na, bd, nb, n, g, scratch(eng, need))
        torch.cuda.synchronize()
        outs.append(g.cpu().numpy())
    got = outs[0]
    assert_within(got[:na, :nb], a.T @ b, 8.0 * n * EPS * (np.abs(a).T @ np.abs(b)), f"gram {n}: {na}x{nb}")
    assert np.all(got[:na, nb:] == SENTINEL) and np.all(got[na:] == SENTINEL), "the padding of G was written"
    assert np.array_equal(bits(outs[0]), bits(outs[1]))


@pytest.mark.parametrize("n", [51, 642])
def test_gram_is_symmetrised_by_the_driver(n):
    """The driver relies on no symmetry of rmsf_block_gram's bits: every
    b x b product goes through ``sym``.  What it hands to ``eigh`` is
    symmetric in its bits and within the kernel's bound."""
    import torch

    from rmsf_amd.eigen import DeviceOps, sym
    a = block(n, 48, 3)
    ops = DeviceOps(torch.tensor(symmetric(n), device="cuda:0"))
    g = sym(ops.gram(ops.put(a), ops.put(a)))
    assert np.array_equal(bits(g), bits(g.T.copy()))
    assert_within(g, a.T @ a, 8.0 * n * EPS * (np.abs(a).T @ np.abs(a)), f"sym(gram) {n}")


@pytest.mark.parametrize("with_a", [False, True], ids=["BT", "aA+BT"])
@pytest.mark.parametrize("n,nb,nc", [(1, 1, 1), (6, 6, 2), (51, 16, 16), (642, 48, 40), (2000, 33, 17), (99, 3, 48)])
def test_block_update(n, nb, nc, with_a):
    import torch
    eng = engine()
    b, t = block(n, nb, 4), np.random.default_rng(nb + nc).standard_normal((nb, nc))
    a = block(n, nc, 5) if with_a else None
    alpha = -1.75 if with_a else 0.0
    bd, td = padded(b, 3, float("nan")), padded(t, 2, float("nan"))
    ad = padded(a, 6, float("nan")) if with_a else None
    c = padded(np.full((n, nc), SENTINEL), 4, SENTINEL, pad_rows=2)
    eng.block_update(alpha, ad, bd, nb, td, n, nc, c)
    torch.cuda.synchronize()
    got = c.cpu().numpy()
    bt = b @ t
    want = alpha * a + bt if with_a else bt
    bound = 8.0 * nb * EPS * (np.abs(b) @ np.abs(t))
    if with_a:
        bound = bound + EPS * np.abs(want)   # one rounding of the add
    assert_within(got[:n, :nc], want, bound, f"update {n}: {nb}x{nc}")
    assert np.all(got[:n, nc:] == SENTINEL) and np.all(got[n:] == SENTINEL), "the padding of C was written"
    if with_a:   # C may be A itself
        eng.block_update(alpha, ad, bd, nb, td, n, nc, ad)
        torch.cuda.synchronize()
        assert np.array_equal(bits(ad.cpu().numpy()[:n, :nc]), bits(got[:n, :nc]))


def test_kernel_argument_checks():
    import torch

    from rmsf_amd._lib import RMSF_EINVAL, RmsfError
    eng = engine()
    m, q, y, g, t = eng.zeros(64, 64), eng.zeros(64, 48), eng.zeros(64, 48), eng.zeros(48, 48), eng.zeros(48, 48)
    wide = eng.zeros(64, 64)
    mp, qp, yp, gp, tp, st = m.data_ptr(), q.data_ptr(), y.data_ptr(), g.data_ptr(), t.data_ptr(), eng.stream
    for args in [(None, 64, 64, qp, 48, 16, yp, 48, None, 0, st), (mp, 64, 64, None, 48, 16, yp, 48, None, 0, st),
                 (mp, 64, 64, qp, 48, 16, None, 48, None, 0, st), (mp, 63, 64, qp, 48, 16, yp, 48, None, 0, st),
                 (mp, 64, 64, qp, 15, 16, yp, 48, None, 0, st), (mp, 64, 64, qp, 48, 16, yp, 15, None, 0, st),
                 (mp, 64, 64, wide.data_ptr(), 64, 49, wide.data_ptr(), 64, None, 0, st)]:
        assert eng.lib.rmsf_symm_block(*args) == RMSF_EINVAL, args
        assert b"rmsf_symm_block" in eng.lib.rmsf_last_error()
    for args in [(None, 48, 16, qp, 48, 16, 64, gp, 48, None, 0, st), (qp, 48, 16, None, 48, 16, 64, gp, 48, None, 0, st),
                 (qp, 48, 16, yp, 48, 16, 64, None, 48, None, 0, st), (qp, 15, 16, yp, 48, 16, 64, gp, 48, None, 0, st),
                 (qp, 48, 16, yp, 48, 16, 64, gp, 15, None, 0, st),
                 (wide.data_ptr(), 64, 49, yp, 48, 16, 64, gp, 48, None, 0, st)]:
        assert eng.lib.rmsf_block_gram(*args) == RMSF_EINVAL, args
        assert b"rmsf_block_gram" in eng.lib.rmsf_last_error()
    for args in [(1.0, None, 0, None, 48, 16, tp, 48, 64, 16, yp, 48, st), (1.0, None, 0, qp, 48, 16, None, 48, 64, 16, yp, 48, st),
                 (1.0, None, 0, qp, 48, 16, tp, 48, 64, 16, None, 48, st), (1.0, None, 0, qp, 15, 16, tp, 48, 64, 16, yp, 48, st),
                 (1.0, None, 0, qp, 48, 16, tp, 15, 64, 16, yp, 48, st), (1.0, None, 0, qp, 48, 16, tp, 48, 64, 16, yp, 15, st),
                 (1.0, None, 0, qp, 48, 16, tp, 48, 64, 16, qp, 48, st),
                 (1.0, None, 0, qp, 48, 16, wide.data_ptr(), 64, 64, 49, wide.data_ptr(), 64, st)]:
        assert eng.lib.rmsf_block_update(*args) == RMSF_EINVAL, args
        assert b"rmsf_block_update" in eng.lib.rmsf_last_error()
    # split plans with too small a workspace
    assert eng.symm_block_workspace_bytes(642, 48) > 0 and eng.block_gram_workspace_bytes(642, 48, 48) > 0
    big, qb = eng.zeros(642, 642), eng.zeros(642, 48)
    with pytest.raises(RmsfError, match="workspace"):
        eng.symm_block(big, 642, qb, 48, eng.zeros(642, 48), eng.zeros(2))
    with pytest.raises(RmsfError, match="workspace"):
        eng.block_gram(qb, 48, qb, 48, 642, g, None)
    torch.cuda.synchronize()
    assert float(y.abs().sum()) == 0.0 and float(g.abs().sum()) == 0.0


# ---- 2. top_eigenpairs over the device ops -----------------------------------
def designed(lam, seed=1):
    """M = U diag(lam) U^T, symmetrised; (M, descending values, vectors)."""
    lam = np.asarray(lam, dtype=np.float64)
    n = lam.size
    u, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))
    m = (u * lam[None, :]) @ u.T
    m = 0.5 * (m + m.T)
    w, v = np.linalg.eigh(m)
    return m, w[::-1].copy(), v[:, ::-1].copy()


@functools.lru_cache(maxsize=None)
def power_law(n):
    return designed(100.0 * (1.0 + np.arange(n)) ** -2.0)


def gaps(w_all, k):
    """Distance from each of the first k of ``w_all`` to its nearest other value."""
    out = np.empty(k)
    for i in range(k):
        d = np.abs(w_all - w_all[i])
        d[i] = np.inf
        out[i] = d.min()
    return out


def check_pairs(n, w_ref, v_ref, vals, vecs, k, gap, tol=TOL, skip=(), what=""):
    """The bounds of the module docstring against the reference's first k
    pairs; ``gap`` [k]; ``skip``: vectors checked elsewhere."""
    e = (tol + 8.0 * n * EPS) * w_ref[0]
    assert vals.shape == (k,) and vecs.shape == (n, k) and vals.dtype == vecs.dtype == np.float64
    dv = np.abs(vals - w_ref[:k])
    print(f"{what} n={n} k={k}: max |dl| / bound = {dv.max() / e:.3e}")
    assert np.all(dv <= e)
    worst = 0.0
    for i in range(k):
        if i in skip:
            continue
        s = 1.0 if vecs[:, i] @ v_ref[:, i] >= 0.0 else -1.0
        d = np.linalg.norm(vecs[:, i] - s * v_ref[:, i])
        worst = max(worst, d * gap[i] / (2.0 * e))
        assert d <= 2.0 * e / gap[i], f"vector {i}: |dv| / bound = {d * gap[i] / (2.0 * e):.3e}"
    print(f"{what} n={n} k={k}: max |dv| / bound = {worst:.3e}")
    assert np.abs(vecs.T @ vecs - np.eye(k)).max() <= 64.0 * n * EPS
    j = np.argmax(np.abs(vecs), axis=0)
    assert np.all(vecs[j, np.arange(k)] > 0.0), "the sign rule"


def device_solve(m, k, **kw):
    import torch

    from rmsf_amd.eigen import top_eigenpairs
    out = top_eigenpairs(torch.tensor(m, device="cuda:0"), k, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n,k,block", [(48, 3, 16), (51, 5, 16), (99, 20, 32), (642, 10, 32), (642, 40, 48)])
def test_top_eigenpairs_power_law(n, k, block):
    from rmsf_amd.eigen import top_eigenpairs
    m, w_ref, v_ref = power_law(n)
    vals, vecs, info = device_solve(m, k)
    print(f"n={n} k={k}: {info['n_iter']} iterations, max residual {info['residuals'].max():.3e}")
    assert info["converged"] and info["block"] == block and info["rank"] == block
    assert np.all(info["residuals"] <= TOL)
    check_pairs(n, w_ref, v_ref, vals, vecs, k, gaps(w_ref, k), what="device")
    # the numpy ops on the same case: the same iteration up to rounding
    vals_h, vecs_h, info_h = top_eigenpairs(m, k)
    assert abs(info["n_iter"] - info_h["n_iter"]) <= 1
    check_pairs(n, vals_h, vecs_h, vals, vecs, k, gaps(w_ref, k), what="device vs numpy ops")
    again = device_solve(m, k)
    assert np.array_equal(bits(again[0]), bits(vals)) and np.array_equal(bits(again[1]), bits(vecs))
    assert again[2]["n_iter"] == info["n_iter"]


def test_top_eigenpairs_rank_deficient():
    from rmsf_amd import PCAConvergenceError
    x = np.random.default_rng(3).standard_normal((10, 51))
    d = x - x.mean(axis=0)
    m = d.T @ d
    m = 0.5 * (m + m.T)
    w, v = np.linalg.eigh(m)
    w, v = w[::-1].copy(), v[:, ::-1].copy()
    for k in (3, 9):
        vals, vecs, info = device_solve(m, k, block=16)
        assert info["converged"] and info["rank"] == 9 and info["n_iter"] <= 3
        check_pairs(51, w, v, vals, vecs, k, gaps(w, k), what="rank 9")
    with pytest.raises(PCAConvergenceError, match="rank 9") as ei:
        device_solve(m, 10, block=16)
    assert ei.value.info["rank"] == 9
    with pytest.raises(PCAConvergenceError, match="rank 0"):
        device_solve(np.zeros((51, 51)), 3)


def test_top_eigenpairs_smaller_than_a_tile():
    m, w_ref, v_ref = designed([9.0, 4.0, 2.0, 1.0, 0.5, 0.1], seed=2)
    vals, vecs, info = device_solve(m, 2)
    assert info["converged"] and info["n_iter"] == 1 and info["block"] == 6
    check_pairs(6, w_ref, v_ref, vals, vecs, 2, gaps(w_ref, 2), what="n=6")


def test_top_eigenpairs_degenerate_pair():
    n = 60
    m, w_ref, v_ref = designed(np.concatenate([[100.0, 50.0, 50.0, 10.0], 1.0 / (1.0 + np.arange(n - 4))]), seed=4)
    vals, vecs, info = device_solve(m, 4)
    assert info["converged"]
    check_pairs(n, w_ref, v_ref, vals, vecs, 4, gaps(w_ref, 4), skip=(1, 2), what="degenerate")
    e = (TOL + 8.0 * n * EPS) * w_ref[0]
    gap = min(w_ref[0] - w_ref[1], w_ref[2] - w_ref[3])
    p, p_ref = vecs[:, 1:3] @ vecs[:, 1:3].T, v_ref[:, 1:3] @ v_ref[:, 1:3].T
    assert np.linalg.norm(p - p_ref, 2) <= 2.0 * e / gap


# ---- 3. PCA(solver="device") end to end --------------------------------------
MODE_SIGMA = (2.0, 1.4, 1.0)   # A per atom, the three planted modes
NOISE = 0.3


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


# (n_sel, F, gathered, align, exact)
PCA_SHAPES = [(17, 40, False, None, None), (50, 300, True, "average", False), (214, 600, False, "average", True)]
K = 3


@functools.lru_cache(maxsize=None)
def run_pca(n_sel, n_frames, gathered, align, exact, solver, n_components):
    import torch

    from rmsf_amd import PCA
    n_atoms, sel = selection(n_sel, gathered)
    x = torch.tensor(make_traj(n_atoms, n_frames), device="cuda:0")
    kw = {} if solver is None else {"solver": solver}
    return PCA(x, select=sel, align=align, exact=exact, n_components=n_components, **kw).run()


@pytest.mark.parametrize("n_sel,n_frames,gathered,align,exact", PCA_SHAPES)
def test_pca_device_against_host(n_sel, n_frames, gathered, align, exact):
    import torch
    dev = run_pca(n_sel, n_frames, gathered, align, exact, "device", K)
    host = run_pca(n_sel, n_frames, gathered, align, exact, "host", None)
    n = 3 * n_sel
    d, h = dev.results, host.results
    info = d.solver_info
    print(f"{n_sel} x {n_frames}: {info['n_iter']} iterations, block {info['block']}, "
          f"l_17 / l_3 = {h.variance[16] / h.variance[2]:.4f}")
    assert info["converged"] and info["block"] == 16 and np.all(info["residuals"] <= TOL)
    # types
    assert isinstance(d.covariance, torch.Tensor) and d.covariance.device.type == "cuda"
    assert d.covariance.shape == (n, n) and d.covariance.dtype == torch.float64
    for a in (d.p_components, d.variance, d.cumulated_variance):
        assert isinstance(a, np.ndarray) and a.dtype == np.float64
    assert d.p_components.shape == (n, K) and d.variance.shape == (K,) and d.cumulated_variance.shape == (K,)
    assert "comoment" not in dev._rmsf.results or dev._rmsf.results.get("comoment") is None
    # the matrix: the host run's, element by element
    cov = d.covariance.cpu().numpy()
    assert np.all(np.abs(cov - h.covariance) <= EPS * np.abs(h.covariance))
    # eigenpairs, the host run as the reference
    check_pairs(n, h.variance, h.p_components, d.variance, d.p_components, K, gaps(h.variance, K), what="PCA")
    lim = K * TOL + 64.0 * n * EPS
    assert np.all(np.abs(d.cumulated_variance - h.cumulated_variance[:K]) <= lim)
    assert np.array_equal(bits(d.mean), bits(h.mean)) and np.array_equal(bits(d.rmsf), bits(h.rmsf))
    assert d.n_frames == h.n_frames == n_frames


def f64_bound(d: np.ndarray, v: np.ndarray) -> np.ndarray:
    return 8.0 * d.shape[1] * 2.0 ** -52 * (np.abs(d) @ np.abs(v))


@functools.lru_cache(maxsize=None)
def oracle_aligned(n_sel, n_frames, gathered):
    """(frames aligned by the oracle on the average structure, f32 [F, n_sel,
    3]; max |aligned x|), as tests/test_gpu_pca_project.py aligns them."""
    from oracle import rmsf_oracle as O
    n_atoms, sel = selection(n_sel, gathered)
    traj = make_traj(n_atoms, n_frames)
    sel = np.arange(n_atoms) if sel is None else sel
    average = O.rmsf_script(traj, sel, None, size=1, align="average")["average"]
    ref_com, ref = O.centred_reference(average, None)
    out = np.empty((n_frames, len(sel), 3), np.float32)
    for f in range(n_frames):
        p = traj[f][sel].astype(np.float32, copy=True)
        out[f] = O.align_frame_(p, None, ref, ref_com)
    return out, float(np.abs(out).max())


@pytest.mark.parametrize("n_sel,n_frames,gathered,align,exact", PCA_SHAPES)
def test_transform_after_the_device_solve(n_sel, n_frames, gathered, align, exact):
    """transform() takes the device solve's host components unchanged: the
    projection equals d @ p_components in numpy within the projection
    kernel's f64 bound (plus, frame-parallel aligned, its 4 u |V_c|_1 term for
    one f32 flip at each rounding point of the superposition)."""
    p = run_pca(n_sel, n_frames, gathered, align, exact, "device", K)
    proj = p.transform()
    assert proj.shape == (n_frames, K) and proj.dtype == np.float64
    v = p.results.p_components
    if align is None:
        n_atoms, sel = selection(n_sel, gathered)
        x = make_traj(n_atoms, n_frames)
        aligned, xmax = (x if sel is None else x[:, sel]), 0.0
    else:
        aligned, xmax = oracle_aligned(n_sel, n_frames, gathered)
    d = aligned.reshape(n_frames, -1).astype(np.float64) - p.results.mean.reshape(-1)
    bound = f64_bound(d, v)
    if align is not None and not exact:
        bound = bound + 4.0 * float(np.spacing(np.float32(xmax))) * np.abs(v).sum(axis=0)[None, :]
    assert_within(proj, d @ v, bound, f"transform {n_sel}x{n_frames}")


def test_one_frame_raises_a_convergence_error():
    import torch

    from rmsf_amd import PCA, PCAConvergenceError
    x = torch.tensor(make_traj(17, 40)[:1], device="cuda:0")
    with pytest.raises(PCAConvergenceError, match="rank 0") as ei:
        PCA(x, align=None, solver="device", n_components=K).run()
    assert ei.value.info["rank"] == 0 and not ei.value.info["converged"]
    # ddof = 0 divides by one frame: the all-zero matrix reaches the solver
    with pytest.raises(PCAConvergenceError, match="rank 0"):
        PCA(x, align=None, solver="device", n_components=K, ddof=0).run()
    torch.cuda.synchronize()


def test_too_many_components_for_the_selection():
    import torch

    from rmsf_amd import PCA
    x = torch.tensor(make_traj(17, 40)[:, :2], device="cuda:0")   # 3n = 6
    with pytest.raises(ValueError, match='solver="host"'):
        PCA(x, align=None, solver="device", n_components=7).run()


def test_cli_pca_solver(tmp_path):
    """The script: --pca-solver device writes the projection on the device
    solve's components; without --pca-transform or --n-components it is an
    argument error, not silently ignored."""
    import subprocess
    import sys

    from conftest import PKG, ROOT
    out = str(tmp_path / "proj.npy")
    base = [sys.executable, f"{PKG}/rmsf_mi355x.py", "--synthetic", "64", "40", "--align", "average"]
    r = subprocess.run(base + ["--pca-transform", out, "--n-components", "3", "--pca-solver", "device"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    proj = np.load(out)
    assert proj.shape == (40, 3) and proj.dtype == np.float64 and np.all(np.isfinite(proj))
    var = (proj * proj).sum(axis=0) / 39.0
    assert var[0] >= var[1] >= var[2] > 0.0
    for args, word in ((["--pca-solver", "device", "--n-components", "3"], "--pca-transform"),
                       (["--pca-solver", "device", "--pca-transform", out], "--n-components")):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 2 and word in r.stderr, r.stderr


@pytest.mark.parametrize("n_sel,n_frames,gathered,align,exact", PCA_SHAPES[:2])
def test_host_solver_is_the_earlier_path(n_sel, n_frames, gathered, align, exact):
    """solver="host", given or defaulted: the types and bits of
    pca_from_comoment on RMSF(covariance=True)'s matrix."""
    import torch

    from rmsf_amd import RMSF
    from rmsf_amd.pca import pca_from_comoment
    n_atoms, sel = selection(n_sel, gathered)
    x = torch.tensor(make_traj(n_atoms, n_frames), device="cuda:0")
    r = RMSF(x, select=sel, align=align, exact=exact, covariance=True).run().results
    assert isinstance(r.comoment, np.ndarray) and isinstance(r.covariance, np.ndarray)
    want = pca_from_comoment(r.comoment, n_frames, 1, K)
    for solver in (None, "host"):
        h = run_pca(n_sel, n_frames, gathered, align, exact, solver, K).results
        for got, ref in zip((h.p_components, h.variance, h.cumulated_variance), want):
            assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(ref))
        assert isinstance(h.covariance, np.ndarray)
        assert np.array_equal(bits(h.covariance), bits(r.comoment / float(n_frames - 1)))
        assert "solver_info" not in h
