"""GPU tier: the PCA projection kernel (csrc/pca_project.hip, f64 MFMA) and
``PCA.transform``, against numpy f64 on raw frames (engine level) or on
frames aligned by the oracle's ``align_frame_``.

Data: the recipe of tests/test_gpu_covariance.py -- base positions in a 100 A
box, three planted collective modes plus 0.3 A noise, a random rigid motion
per frame, f32.

Bounds (derived, not measured):
  * the f64 term, per element ``8 * 3n * 2^-52 * (|d| @ |V|)[f, c]``: the
    f64 dot-product error bound (3n terms, unit roundoff 2^-53 doubled), times
    8 for the kernel's summation order (4 waves, MFMA k-steps, split-K fold);
    two numpy summation orders differ by at most 0.0022 of it on these shapes.
  * aligned, per element ``4 u ||V_c||_1`` on top, u = spacing(f32(max
    |aligned x|)): one f32 flip of size u at each rounding point of
    RMSF.py:99-101 in every coordinate (the frame-parallel rotation may differ
    from the oracle's in its last bits).  About 1e-3 A; a wrong frame, atom or
    record moves a projection by about 1 A.  With exact=True the aligned
    coordinates are the oracle's bit for bit and the f64 term alone holds.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

MODE_SIGMA = (2.0, 1.4, 1.0)   # A per atom, the three planted modes
NOISE = 0.3
SENTINEL = -7.25e77


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


def f64_bound(d: np.ndarray, v: np.ndarray) -> np.ndarray:
    return 8.0 * d.shape[1] * 2.0 ** -52 * (np.abs(d) @ np.abs(v))


def assert_within(got, want, bound, what):
    ratio = np.abs(got - want) / np.maximum(bound, np.finfo(np.float64).tiny)
    print(f"{what}: max |dP| = {np.abs(got - want).max():.3e}, max |dP| / bound = {ratio.max():.3e}")
    assert np.all(np.isfinite(got)), f"{what}: non-finite projection"
    assert np.all(np.abs(got - want) <= bound), f"{what}: max |dP| / bound = {ratio.max():.3e}"


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. engine level, no alignment, against numpy --------------------------
# (n_sel, F, k, batch, every `skip`-th frame of a skip * F frame tensor)
ENGINE_SHAPES = [(1, 1, 1, None, 1), (5, 3, 2, None, 1), (16, 16, 16, None, 1), (17, 17, 17, None, 1),
                 (17, 33, 51, None, 1), (214, 67, 10, None, 1), (341, 300, 7, 128, 2), (5000, 5, 3, None, 1)]


@functools.lru_cache(maxsize=None)
def engine_case(n_sel, n_frames, k, gathered, skip):
    """(stored frames, sel, mean [3n], V [3n, k], the numpy projection, its
    f64 bound) -- computed once per shape."""
    n_atoms, sel = selection(n_sel, gathered)
    stored = make_traj(n_atoms, skip * n_frames)
    x = stored[::skip]
    xs = (x if sel is None else x[:, sel]).reshape(n_frames, -1).astype(np.float64)
    mean = xs.mean(axis=0)
    rng = np.random.default_rng(11 * n_sel + k)
    v, _ = np.linalg.qr(rng.normal(size=(3 * n_sel, k)))
    d = xs - mean
    return stored, sel, mean, np.ascontiguousarray(v), d @ v, f64_bound(d, v)


def engine_project(eng, stored, sel, mean, v, n_frames, batch, skip, pad_c=5, pad_o=4, pad_rows=3):
    """The kernel over the case, batch by batch: d_comp rows ``pad_c`` wider
    than k (NaN there: never read), d_out ``pad_o`` wider and ``pad_rows``
    longer, prefilled with a sentinel."""
    import torch
    n_sel, k = len(mean) // 3, v.shape[1]
    x = torch.tensor(stored, device="cuda:0")
    fstride = skip * x.stride(0)
    comp = torch.full((3 * n_sel, k + pad_c), float("nan"), dtype=torch.float64, device="cuda:0")
    comp[:, :k] = torch.tensor(v, device="cuda:0")
    out = torch.full((n_frames + pad_rows, k + pad_o), SENTINEL, dtype=torch.float64, device="cuda:0")
    mean_d = torch.tensor(mean, device="cuda:0")
    sel_d = eng.sel_tensor(sel)
    bf = batch or n_frames
    for f0 in range(0, n_frames, bf):
        n = min(bf, n_frames - f0)
        need = eng.pca_project_workspace_bytes(n, n_sel, k)
        work = eng.empty(need // 8) if need else None
        eng.pca_project(x.data_ptr() + 4 * f0 * fstride, fstride, n, n_sel, sel_d, None, None, mean_d, comp, k,
                        out[f0:f0 + n], work)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
@pytest.mark.parametrize("n_sel,n_frames,k,batch,skip", ENGINE_SHAPES)
def test_engine_projection_unaligned(n_sel, n_frames, k, batch, skip, gathered):
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    stored, sel, mean, v, want, bound = engine_case(n_sel, n_frames, k, gathered, skip)
    if n_sel == 5000:   # the split-K plan: the fold launch is exercised
        assert eng.pca_project_workspace_bytes(n_frames, n_sel, k) > 0
    out = engine_project(eng, stored, sel, mean, v, n_frames, batch, skip)
    assert_within(out[:n_frames, :k], want, bound, f"engine {n_sel}x{n_frames}x{k}")
    assert np.all(out[:n_frames, k:] == SENTINEL), "padding columns of d_out were written"
    assert np.all(out[n_frames:] == SENTINEL), "rows past the batch were written"


def test_engine_argument_checks():
    import torch

    from rmsf_amd._lib import RMSF_EINVAL, RmsfError
    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    x = torch.zeros((4, 5, 3), dtype=torch.float32, device="cuda:0")
    mean, comp, out = eng.zeros(15), eng.zeros(15, 4), eng.zeros(4, 4)
    xf, info = eng.zeros(4, 16), eng.zeros(2064)
    p, m, c, o = x.data_ptr(), mean.data_ptr(), comp.data_ptr(), out.data_ptr()
    st = eng.stream
    bad = [
        (None, 15, 4, 5, None, None, None, m, c, 4, 4, o, 4, None, 0, st),      # NULL d_xyz
        (p, 15, 4, 5, None, None, None, None, c, 4, 4, o, 4, None, 0, st),      # NULL d_mean
        (p, 15, 4, 5, None, None, None, m, None, 4, 4, o, 4, None, 0, st),      # NULL d_comp
        (p, 15, 4, 5, None, None, None, m, c, 4, 4, None, 4, None, 0, st),      # NULL d_out
        (p, 15, 4, 5, None, None, None, m, c, 4, 0, o, 4, None, 0, st),         # n_comp < 1
        (p, 15, 4, 5, None, None, None, m, c, 3, 4, o, 4, None, 0, st),         # ldc < n_comp
        (p, 15, 4, 5, None, None, None, m, c, 4, 4, o, 3, None, 0, st),         # ldo < n_comp
        (p, 15, 4, 5, None, xf.data_ptr(), None, m, c, 4, 4, o, 4, None, 0, st),    # d_xform alone
        (p, 15, 4, 5, None, None, info.data_ptr(), m, c, 4, 4, o, 4, None, 0, st),  # d_refinfo alone
    ]
    for args in bad:
        rc = eng.lib.rmsf_pca_project(*args)
        assert rc == RMSF_EINVAL, args
        assert b"rmsf_pca_project" in eng.lib.rmsf_last_error()
    # a split plan with too small a workspace
    assert eng.pca_project_workspace_bytes(5, 5000, 3) > 0
    big = torch.zeros((5, 5000, 3), dtype=torch.float32, device="cuda:0")
    with pytest.raises(RmsfError, match="workspace"):
        eng.pca_project(big.data_ptr(), 15000, 5, 5000, None, None, None, eng.zeros(15000), eng.zeros(15000, 3), 3,
                        eng.zeros(5, 3), eng.zeros(2))
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0


# ---- 2. aligned, through PCA.transform -------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_aligned(n_sel, n_frames, gathered, align, target_seed=0):
    """(aligned f32 [F, n_sel, 3], max |aligned x|): the frames of trajectory
    ``target_seed`` aligned by the oracle on the reference of trajectory 0 --
    its frame 0 (RMSF.py:80-87), or its average structure (RMSF.py:89-118,
    from rmsf_script) -- used as tests/test_gpu_covariance.py::ref_aligned
    uses the oracle."""
    from oracle import rmsf_oracle as O
    n_atoms, sel = selection(n_sel, gathered)
    traj = make_traj(n_atoms, n_frames)
    sel = np.arange(n_atoms) if sel is None else sel
    if align == "average":
        average = O.rmsf_script(traj, sel, None, size=1, align="average")["average"]
        ref_com, ref = O.centred_reference(average, None)
    else:
        ref_com, ref = O.centred_reference(traj[0][sel], None)
    target = make_traj(n_atoms, n_frames, target_seed)
    out = np.empty((n_frames, len(sel), 3), np.float32)
    for f in range(n_frames):
        p = target[f][sel].astype(np.float32, copy=True)
        out[f] = O.align_frame_(p, None, ref, ref_com)
    return out, float(np.abs(out).max())


@functools.lru_cache(maxsize=None)
def run_pca(n_sel, n_frames, gathered, align, exact, batch, n_components):
    import torch

    from rmsf_amd import PCA
    n_atoms, sel = selection(n_sel, gathered)
    x = torch.tensor(make_traj(n_atoms, n_frames), device="cuda:0")
    return PCA(x, select=sel, align=align, exact=exact, batch_frames=batch, n_components=n_components).run()


def reference_projection(p, aligned, xmax, exact, k=None):
    """(projection of the oracle-aligned frames on the GPU's own mean and
    components, its elementwise bound)."""
    v = p.results.p_components if k is None else p.results.p_components[:, :k]
    d = aligned.reshape(len(aligned), -1).astype(np.float64) - p.results.mean.reshape(-1)
    bound = f64_bound(d, v)
    if not exact:
        u = float(np.spacing(np.float32(xmax)))
        bound = bound + 4.0 * u * np.abs(v).sum(axis=0)[None, :]
    return d @ v, bound


ALIGNED_SHAPES = [(17, 5, False, None, None), (214, 67, False, None, 10), (341, 300, True, 128, 10)]


@pytest.mark.parametrize("exact", [False, True], ids=["frame-parallel", "exact"])
@pytest.mark.parametrize("align", ["frame0", "average"])
@pytest.mark.parametrize("n_sel,n_frames,gathered,batch,n_comp", ALIGNED_SHAPES)
def test_transform_aligned(n_sel, n_frames, gathered, batch, n_comp, align, exact):
    p = run_pca(n_sel, n_frames, gathered, align, exact, batch, n_comp)
    proj = p.transform()
    k = 3 * n_sel if n_comp is None else n_comp
    assert proj.shape == (n_frames, k) and proj.dtype == np.float64
    aligned, xmax = oracle_aligned(n_sel, n_frames, gathered, align)
    want, bound = reference_projection(p, aligned, xmax, exact)
    assert_within(proj, want, bound, f"transform {n_sel}x{n_frames} {align} exact={exact}")


# ---- 3. identities on the PCA's own trajectory -----------------------------
def check_identities(p, proj, extra=None):
    """Column means vanish and proj^T proj / (F - ddof) = diag(variance).
    ``extra`` [k]: a per-column perturbation of the projections allowed on top
    (the aligned term), propagated to both identities."""
    var = p.results.variance
    n_frames = proj.shape[0]
    e = np.zeros(proj.shape[1]) if extra is None else extra
    means = np.abs(proj.mean(axis=0))
    lim = 1e-9 * np.sqrt(var[0]) + e
    print(f"identities: max |column mean| / bound = {(means / lim).max():.3e}")
    assert np.all(means <= lim)
    s = proj.T @ proj / (n_frames - p.ddof)
    a = np.abs(proj).sum(axis=0)
    lim2 = 1e-8 * var[0] + (np.outer(a, e) + np.outer(e, a) + n_frames * np.outer(e, e)) / (n_frames - p.ddof)
    dev = np.abs(s - np.diag(var))
    print(f"identities: max |P^T P / (F - ddof) - diag(variance)| / bound = {(dev / lim2).max():.3e}")
    assert np.all(dev <= lim2)


def test_identities_unaligned():
    p = run_pca(214, 300, False, None, False, None, None)
    proj = p.transform()
    assert proj.shape == (300, 642)
    check_identities(p, proj)


def test_identities_aligned_average_exact():
    p = run_pca(214, 300, False, "average", True, None, None)
    proj = p.transform()
    _, xmax = oracle_aligned(214, 300, False, "average")
    u = float(np.spacing(np.float32(xmax)))
    check_identities(p, proj, 4.0 * u * np.abs(p.results.p_components).sum(axis=0))


# ---- 4. another trajectory --------------------------------------------------
@pytest.mark.parametrize("exact", [False, True], ids=["frame-parallel", "exact"])
@pytest.mark.parametrize("align", ["frame0", "average"])
def test_transform_other_trajectory(align, exact):
    import torch
    p = run_pca(214, 67, False, align, exact, None, 10)
    other = torch.tensor(make_traj(214, 67, 1), device="cuda:0")
    proj = p.transform(other, n_components=3)
    assert proj.shape == (67, 3)
    aligned, xmax = oracle_aligned(214, 67, False, align, 1)
    want, bound = reference_projection(p, aligned, xmax, exact, 3)
    assert_within(proj, want, bound, f"transform(other) {align} exact={exact}")
    # a frame range of it (another batch size: the frame-parallel sums may round differently)
    part = p.transform(other, n_components=3, start=5, stop=60, step=5)
    assert_within(part, want[5:60:5], bound[5:60:5], f"transform(other, 5:60:5) {align} exact={exact}")
    if exact:
        assert np.array_equal(bits(part), bits(proj[5:60:5]))
    with pytest.raises(ValueError, match="atoms"):
        p.transform(torch.zeros((4, 213, 3), dtype=torch.float32, device="cuda:0"))


# ---- 5. inputs ----------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True], ids=["frame-parallel", "exact"])
def test_transform_inputs_same_bits(tmp_path, exact):
    import torch

    from rmsf_amd import PCA
    from rmsf_amd.xtc import XTCFile, write_xtc
    traj = make_traj(214, 67)
    kw = dict(align="average", exact=exact, n_components=10)
    dev = PCA(torch.tensor(traj, device="cuda:0"), **kw).run().transform()
    host = PCA(np.array(traj), **kw).run().transform()
    assert np.array_equal(bits(host), bits(dev)), "a host array and the HBM tensor of the same floats differ"
    path = str(tmp_path / "t.xtc")
    write_xtc(path, traj)
    decoded = XTCFile(path).read()
    assert decoded.shape == traj.shape
    from_file = PCA(path, **kw).run().transform()
    from_tensor = PCA(torch.tensor(decoded, device="cuda:0"), **kw).run().transform()
    assert np.array_equal(bits(from_file), bits(from_tensor)), "the XTC file and the tensor of its floats differ"
    # another input handed to a finished PCA: the same frames as a host array and as a file
    p = PCA(torch.tensor(decoded, device="cuda:0"), **kw).run()
    assert np.array_equal(bits(p.transform(path)), bits(from_tensor))
    assert np.array_equal(bits(p.transform(decoded)), bits(from_tensor))


# ---- 6. determinism ---------------------------------------------------------------
def test_transform_deterministic():
    import torch
    for args in [(214, 67, False, "average", False, None, 10), (341, 300, True, "frame0", False, 128, 10)]:
        p = run_pca(*args)
        a, b = p.transform(), p.transform()
        assert np.array_equal(bits(a), bits(b))
        t = p.transform(as_tensor=True)
        assert isinstance(t, torch.Tensor) and t.device.type == "cuda"
        assert np.array_equal(bits(t.cpu().numpy()), bits(a))


def test_transform_deterministic_split_k():
    """The split-K shape through transform(): 5,000 atoms x 5 frames.  The
    eigen-decomposition of a 15,000^2 matrix takes minutes, so the results are
    filled in by hand (orthonormal columns, the frames' mean) on an unaligned
    PCA, which transform() then projects from the PCA's own input."""
    import torch

    from rmsf_amd import PCA
    from rmsf_amd.engine import Engine
    stored, sel, mean, v, want, bound = engine_case(5000, 5, 3, False, 1)
    assert Engine(torch.device("cuda", 0)).pca_project_workspace_bytes(5, 5000, 3) > 0
    p = PCA(torch.tensor(stored, device="cuda:0"), align=None)
    p.results.p_components, p.results.mean = v, mean.reshape(-1, 3)
    a, b = p.transform(), p.transform()
    assert np.array_equal(bits(a), bits(b))
    assert_within(a, want, bound, "transform split-K")


# ---- 7. refusals ------------------------------------------------------------------
def test_transform_refusals():
    import torch

    from rmsf_amd import PCA
    from rmsf_amd.sources import DeviceSource
    p = run_pca(17, 5, False, "average", False, None, None)
    k = p.results.p_components.shape[1]
    for bad in (0, k + 1):
        with pytest.raises(ValueError, match="n_components"):
            p.transform(n_components=bad)
    x = torch.tensor(make_traj(17, 5), device="cuda:0")
    with pytest.raises(NotImplementedError):
        PCA(x, gpus=2).run()
    q = PCA(x, gpus=2)
    q.results.update(p.results)
    with pytest.raises(NotImplementedError, match="one device per process"):
        q.transform()
    with pytest.raises(NotImplementedError, match="one device per process"):
        p.transform([x])
    soa = x.permute(0, 2, 1).contiguous()
    with pytest.raises(NotImplementedError, match="planes"):
        p.transform(DeviceSource(soa, layout="soa"))
    q = PCA(soa, layout="soa", align=None)
    q.results.update(p.results)
    with pytest.raises(NotImplementedError, match="planes"):
        q.transform()


def test_projection_over_half_the_free_hbm_is_refused():
    """3 x 10^9 frames of 3 atoms (one zero frame, expanded with a frame
    stride of 0: 36 bytes are all that is allocated) on 9 components: a 216 GB
    projection -- a MemoryError stating the bytes, before any launch."""
    import torch

    from rmsf_amd import PCA
    rng = np.random.default_rng(5)
    small = torch.tensor(rng.normal(size=(8, 3, 3)).astype(np.float32), device="cuda:0")
    p = PCA(small, align=None).run()
    n_frames = 3_000_000_000
    big = torch.zeros((1, 3, 3), dtype=torch.float32, device="cuda:0").expand(n_frames, 3, 3)
    with pytest.raises(MemoryError, match=str(8 * n_frames * 9)):
        p.transform(big)


# ---- 8. the script ----------------------------------------------------------------
def test_cli_pca_transform(tmp_path):
    out = str(tmp_path / "proj.npy")
    r = subprocess.run([sys.executable, f"{PKG}/rmsf_mi355x.py", "--synthetic", "64", "40", "--align", "average",
                        "--pca-transform", out, "--n-components", "3"], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    proj = np.load(out)
    assert proj.shape == (40, 3) and proj.dtype == np.float64
    # identity 3 from the projections alone: centred columns, uncorrelated, variances descending.  Aligned
    # term: 4 u ||V_c||_1 with u = spacing(f32(256)) (the synthetic box is 100 A) and ||V_c||_1 <= sqrt(3 n).
    e = 4.0 * float(np.spacing(np.float32(255.0))) * np.sqrt(3 * 64)
    s = proj.T @ proj / 39.0
    var = s.diagonal()
    assert var[0] >= var[1] >= var[2] > 0.0
    assert np.all(np.abs(proj.mean(axis=0)) <= 1e-9 * np.sqrt(var[0]) + e)
    a = np.abs(proj).sum(axis=0)
    lim = 1e-8 * var[0] + (2.0 * a.max() * e + 40 * e * e) / 39.0
    off = np.abs(s - np.diag(var))
    assert np.all(off <= lim), (off.max(), lim)
    r = subprocess.run([sys.executable, f"{PKG}/rmsf_mi355x.py", "--synthetic", "64", "40", "--merge", "scatter",
                        "--pca-transform", out], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2 and "--pca-transform" in r.stderr
