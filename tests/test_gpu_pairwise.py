"""GPU tier: the all-pairs RMSD matrix (csrc/pairwise.hip, the f64 MFMA
contraction over atoms with the QCP Newton epilogue) and ``DistanceMatrix``,
against a numpy f64 reference that does not use QCP:

  * superposition on: weighted centring, ``H = (w d_j)^T d_i``, an SVD with
    the determinant sign (as ``oracle.rmsf_oracle.kabsch``), ``d^2 = (G_i +
    G_j - 2 (s0 + s1 +- s2)) / sum w``;
  * superposition off: the direct ``sum w |x_i - x_j|^2 / sum w``.

Data: the generator of tests/test_gpu_covariance.py (planted modes, noise, a
random rigid motion per frame, f32), with the last frame overwritten by a
copy of frame 0, so the data holds one duplicate pair.

Bound (derived, not measured): ``|d^2_gpu - d^2_ref| <= 1e-12 S_ij``, ``S_ij =
(G_i + G_j) / (2 sum w)`` with G about each frame's own weighted centre.  The
f64 Gram sums err by at most n 2^-53 S (1e-13 at 1,000 atoms); Newton's last
step below 1e-11 lambda leaves an error of the order of that step squared.
Every pair is compared except the diagonal and the duplicate pair, which the
cutoff rule sets to exactly 0.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODE_SIGMA = (2.0, 1.4, 1.0)   # A per atom, the three planted modes
NOISE = 0.3
STAGE = 32                     # atoms the kernel stages at a time (kKA of csrc/pairwise.hip)
BOUND = 1e-12


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


@functools.lru_cache(maxsize=None)
def data(n_frames: int, n_sel: int, gathered: bool) -> np.ndarray:
    """The trajectory of a case: the generator's, frame F-1 := frame 0."""
    n_atoms, _ = selection(n_sel, gathered)
    x = make_traj(n_atoms, n_frames).copy()
    x[n_frames - 1] = x[0]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def weights_of(n_sel: int):
    w = np.random.default_rng(n_sel).uniform(1.0, 16.0, size=n_sel)
    w.setflags(write=False)
    return w


def reference_sq(x: np.ndarray, w, superpose: bool):
    """(d^2 [F, F], S [F, F]) of the selected rows x f32 [F, n, 3] in numpy
    f64; no QCP."""
    x = x.astype(np.float64)
    n_frames, n = x.shape[:2]
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    wt = w.sum()
    d = x - (w[None, :, None] * x).sum(axis=1, keepdims=True) / wt
    g = (w[None, :, None] * d * d).sum(axis=(1, 2))
    s_scale = (g[:, None] + g[None, :]) / (2.0 * wt)
    if not superpose:
        sq = np.empty((n_frames, n_frames))
        for i in range(n_frames):
            diff = x - x[i]
            sq[i] = (w[None, :, None] * diff * diff).sum(axis=(1, 2)) / wt
        return sq, s_scale
    # H[i, j] = (w d_j)^T d_i, the 3 x 3 matrix of every pair
    h = np.einsum("jac,iad->ijcd", w[None, :, None] * d, d)
    u, s, vt = np.linalg.svd(h)
    sign = np.sign(np.linalg.det(u @ vt))
    tr = s[..., 0] + s[..., 1] + sign * s[..., 2]
    return (g[:, None] + g[None, :] - 2.0 * tr) / wt, s_scale


@functools.lru_cache(maxsize=None)
def reference(n_frames: int, n_sel: int, gathered: bool, weighted: bool, superpose: bool):
    _, sel = selection(n_sel, gathered)
    x = data(n_frames, n_sel, gathered)
    sq, s = reference_sq(x if sel is None else x[:, sel], weights_of(n_sel) if weighted else None, superpose)
    sq.setflags(write=False)
    s.setflags(write=False)
    return sq, s


def check(m: np.ndarray, sq_ref: np.ndarray, s_scale: np.ndarray, dup, label: str) -> float:
    """Symmetric in its bits, zero diagonal, the duplicate pair exactly 0,
    every other pair inside the bound; returns the largest ratio."""
    n = len(m)
    assert m.shape == (n, n) and m.dtype == np.float64
    assert np.array_equal(m.view(np.uint64), np.ascontiguousarray(m.T).view(np.uint64)), "D != D.T"
    assert not m.diagonal().any(), "the diagonal is exactly zero"
    skip = np.eye(n, dtype=bool)
    if dup is not None:
        a, b = dup
        assert m[a, b] == 0.0 and m[b, a] == 0.0, f"the duplicate pair is not exactly zero: {m[a, b]!r}"
        skip[a, b] = skip[b, a] = True
    keep = ~skip
    assert keep.sum() == n * n - n - (2 if dup is not None else 0)   # no other pair is left out
    # the test's own data: everything compared is a real distance, far above the cutoff
    d_ref = np.sqrt(np.abs(sq_ref))
    assert np.all(d_ref[keep] > 0.1), f"{label}: a non-duplicate reference distance <= 0.1 A"
    ratio = np.abs(m * m - sq_ref) / (BOUND * s_scale)
    worst = float(ratio[keep].max()) if keep.any() else 0.0
    print(f"{label}: max |d2 - d2_ref| / (1e-12 S) = {worst:.3e}")
    assert worst <= 1.0, f"{label}: ratio {worst}"
    return worst


def engine_matrix(n_frames, n_sel, gathered, weighted, superpose, cutoff=1e-5):
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    _, sel = selection(n_sel, gathered)
    x = torch.tensor(data(n_frames, n_sel, gathered), device="cuda:0")
    sel_dev = eng.sel_tensor(sel)
    w = weights_of(n_sel) if weighted else None
    w_dev = None if w is None else torch.tensor(w, device="cuda:0")
    w_total = float(n_sel) if w is None else float(w.sum())
    centre, g = eng.pairwise_centres(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, w_dev, superpose)
    need = eng.pairwise_workspace_bytes(n_frames, n_sel)
    work = eng.empty(need // 8) if need else None
    out = torch.full((n_frames, n_frames), float("nan"), dtype=torch.float64, device="cuda:0")
    eng.pairwise_rmsd(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, w_dev, w_total, centre, g, out,
                      superpose=superpose, cutoff=cutoff, work=work)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def public_matrix(n_frames, n_sel, gathered, weighted, superpose, host=False, run_kw=None, **kw):
    import torch

    from rmsf_amd import DistanceMatrix
    _, sel = selection(n_sel, gathered)
    x = data(n_frames, n_sel, gathered)
    inp = x if host else torch.tensor(x, device="cuda:0")
    dm = DistanceMatrix(inp, select=sel, weights=weights_of(n_sel) if weighted else None, superposition=superpose,
                        **kw).run(**(run_kw or {}))
    return dm.results


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. every shape, engine level and through DistanceMatrix ---------------------
SHAPES = [(2, 3), (15, 4), (16, 17), (17, 33), (33, 31), (50, 214),      # tile edges
          (5, 5000),                                                      # split-K
          (9, STAGE - 1), (9, STAGE), (9, STAGE + 1)]                     # atom-stage edges


@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
@pytest.mark.parametrize("n_frames,n_sel", SHAPES)
def test_matrix_against_reference(n_frames, n_sel, gathered, superpose):
    sq_ref, s = reference(n_frames, n_sel, gathered, False, superpose)
    dup = (0, n_frames - 1)
    label = f"({n_frames} x {n_sel}) gathered={gathered} superpose={superpose}"
    m = engine_matrix(n_frames, n_sel, gathered, False, superpose)
    assert not np.isnan(m).any(), "an element was never written"
    check(m, sq_ref, s, dup, "engine " + label)
    r = public_matrix(n_frames, n_sel, gathered, False, superpose)
    assert r.n_frames == n_frames
    np.testing.assert_array_equal(r.frames, np.arange(n_frames))
    assert same_bits(r.dist_matrix, m), "DistanceMatrix and the engine differ in their bits"


@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
@pytest.mark.parametrize("n_frames,n_sel", [(17, 33), (50, 214)])
def test_weighted_matrix(n_frames, n_sel, gathered, superpose):
    sq_ref, s = reference(n_frames, n_sel, gathered, True, superpose)
    label = f"weighted ({n_frames} x {n_sel}) gathered={gathered} superpose={superpose}"
    m = engine_matrix(n_frames, n_sel, gathered, True, superpose)
    check(m, sq_ref, s, (0, n_frames - 1), "engine " + label)
    r = public_matrix(n_frames, n_sel, gathered, True, superpose)
    assert same_bits(r.dist_matrix, m), "DistanceMatrix and the engine differ in their bits"
    # the weights matter: the unweighted matrix is another one
    assert not same_bits(m, engine_matrix(n_frames, n_sel, gathered, False, superpose))


# ---- 2. frame lists: a dense copy (scattered) and a strided read in place ----------
@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
@pytest.mark.parametrize("run_kw,rows", [(dict(frames=list(range(10)) + list(range(20, 30))),
                                          np.r_[0:10, 20:30]),
                                         (dict(step=3), np.arange(0, 33, 3))], ids=["frames", "step3"])
def test_frame_lists_host_and_device_inputs(run_kw, rows, superpose):
    n_frames, n_sel, gathered = 33, 31, True
    _, sel = selection(n_sel, gathered)
    x = data(n_frames, n_sel, gathered)
    sq_ref, s = reference_sq(x[rows][:, sel], None, superpose)
    dev = public_matrix(n_frames, n_sel, gathered, False, superpose, run_kw=run_kw)
    host = public_matrix(n_frames, n_sel, gathered, False, superpose, host=True, run_kw=run_kw)
    np.testing.assert_array_equal(dev.frames, rows)
    np.testing.assert_array_equal(host.frames, rows)
    assert dev.n_frames == host.n_frames == len(rows)
    dup = None   # frame 32, the copy of frame 0, is in neither list
    check(dev.dist_matrix, sq_ref, s, dup, f"{run_kw} superpose={superpose} (HIP tensor)")
    assert same_bits(dev.dist_matrix, host.dist_matrix), "host and HIP inputs differ in their bits"


def test_host_input_in_batches_and_whole():
    """A host array streamed in batches of 7 frames lands in the same dense
    buffer as one batch: the same bits."""
    a = public_matrix(50, 214, False, False, True, host=True)
    b = public_matrix(50, 214, False, False, True, host=True, batch_frames=7)
    c = public_matrix(50, 214, False, False, True)
    assert same_bits(a.dist_matrix, b.dist_matrix) and same_bits(a.dist_matrix, c.dist_matrix)


# ---- 3. determinism -------------------------------------------------------------
@pytest.mark.parametrize("n_frames,n_sel", [(50, 214), (5, 5000)])
def test_two_runs_are_identical_in_bits(n_frames, n_sel):
    a = engine_matrix(n_frames, n_sel, False, False, True)
    b = engine_matrix(n_frames, n_sel, False, False, True)
    assert a is not b and same_bits(a, b)


# ---- 4. the cutoff --------------------------------------------------------------
@pytest.mark.parametrize("superpose", [True, False], ids=["superpose", "plain"])
@pytest.mark.parametrize("n_frames,n_sel", [(17, 33), (5, 5000)])
def test_cutoff_zero_leaves_the_duplicate_raw(n_frames, n_sel, superpose):
    raw = engine_matrix(n_frames, n_sel, False, False, superpose, cutoff=0.0)
    cut = engine_matrix(n_frames, n_sel, False, False, superpose)
    a, b = 0, n_frames - 1
    print(f"({n_frames} x {n_sel}) superpose={superpose}: raw duplicate distance {raw[a, b]:.3e} A")
    assert 0.0 <= raw[a, b] < 1e-5 and raw[a, b] == raw[b, a]
    assert cut[a, b] == 0.0
    raw[a, b] = raw[b, a] = 0.0
    assert same_bits(raw, cut), "the cutoff moved another element"
    r = public_matrix(n_frames, n_sel, False, False, superpose, cutoff=0.0)
    assert 0.0 <= r.dist_matrix[a, b] < 1e-5


# ---- 5. DiffusionMap from a DistanceMatrix --------------------------------------------
def test_diffusion_map_runs_the_distance_matrix():
    import torch

    from rmsf_amd import DiffusionMap, DistanceMatrix
    x = torch.tensor(data(50, 214, False), device="cuda:0")
    dm = DiffusionMap(DistanceMatrix(x), epsilon=4.0).run()
    w = dm.results.eigenvalues
    assert w.shape == (50,) and abs(w[0] - 1.0) <= 1e-12 and np.all(np.diff(w) <= 0)
    assert dm.transform(2, 1).shape == (50, 2)


# ---- the matrix must fit --------------------------------------------------------
def test_matrix_over_half_the_free_hbm_is_refused():
    """200,000 frames: a 320 GB f64 matrix -- a MemoryError stating the bytes,
    before any launch (7.2 MB of zero frames is all that is allocated)."""
    import torch

    from rmsf_amd import DistanceMatrix
    x = torch.zeros((200_000, 3, 3), dtype=torch.float32, device="cuda:0")
    with pytest.raises(MemoryError, match=str(8 * 200_000 ** 2)):
        DistanceMatrix(x).run()
