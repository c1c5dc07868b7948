"""GPU tier: the PCA back-projection kernel (csrc/pca_backproject.hip, f64
MFMA), the adjoint of csrc/pca_project.hip: Y = D^T P, against numpy f64 on
raw frames, against the projection kernel through the adjoint identity
<P, D Q> = <D^T P, Q> on superposed frames, and against numpy on frames
aligned by the oracle's ``align_frame_``.

Data: the planted-mode recipe of tests/test_gpu_pca_project.py, restated --
base positions in a 100 A box, three collective modes plus 0.3 A noise, a
random rigid motion per frame, f32.

Bounds (derived, not measured):
  * the f64 term, per element ``8 F 2^-52 (|d|^T @ |p|)[i, c]``: the f64
    dot-product error bound (F terms, unit roundoff 2^-53 doubled), times 8
    for the kernel's summation order (4 waves, MFMA k-steps, split-K fold,
    batches).  The kernel's d = f64(x) - mean is numpy's own subtraction.
  * ``accumulate`` onto a prefilled Y: one more rounding, 2^-53 |prefill +
    product|, on top.
  * the adjoint identity: both kernels read the same d (the same
    ``apply_xform``, the same records), so no f32 term enters; the two f64
    bounds, each contracted with the other side's magnitudes, plus numpy's own
    rounding of the two inner products.  |d| in the bound is restated from the
    records in numpy and widened by one f32 spacing u (numpy's dot may round
    the rotation's last f32 bit the other way).
  * aligned against the oracle, per element ``4 u sum_f |P[f, c]|`` on top of
    the f64 term, u = spacing(f32(max |aligned x|)): tests/
    test_gpu_pca_project.py's term, one f32 flip at each rounding point of
    RMSF.py:99-101 in every coordinate of every frame.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODE_SIGMA = (2.0, 1.4, 1.0)   # A per atom, the three planted modes
NOISE = 0.3
SENTINEL = -7.25e77
EPS = 2.0 ** -52


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


def f64_bound(d: np.ndarray, p: np.ndarray) -> np.ndarray:
    return 8.0 * d.shape[0] * EPS * (np.abs(d).T @ np.abs(p))


def assert_within(got, want, bound, what):
    ratio = np.abs(got - want) / np.maximum(bound, np.finfo(np.float64).tiny)
    print(f"{what}: max |dY| = {np.abs(got - want).max():.3e}, max |dY| / bound = {ratio.max():.3e}")
    assert np.all(np.isfinite(got)), f"{what}: non-finite result"
    assert np.all(np.abs(got - want) <= bound), f"{what}: max |dY| / bound = {ratio.max():.3e}"


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. engine level, no alignment, against numpy --------------------------
# (n_sel, F, cols, batch, every `skip`-th frame of a skip * F frame tensor)
ENGINE_SHAPES = [(1, 1, 1, None, 1), (5, 3, 2, None, 1), (16, 32, 16, None, 1), (17, 33, 17, None, 1),
                 (33, 31, 33, None, 1), (214, 67, 48, None, 1), (341, 300, 7, 128, 2), (5, 5000, 3, None, 1),
                 (5000, 5, 48, None, 1)]


@functools.lru_cache(maxsize=None)
def engine_case(n_sel, n_frames, cols, gathered, skip):
    """(stored frames, sel, mean [3n], P [F, cols], numpy's d.T @ P, its f64
    bound) -- computed once per shape."""
    n_atoms, sel = selection(n_sel, gathered)
    stored = make_traj(n_atoms, skip * n_frames)
    x = stored[::skip]
    xs = (x if sel is None else x[:, sel]).reshape(n_frames, -1).astype(np.float64)
    mean = xs.mean(axis=0)
    p = np.random.default_rng(13 * n_sel + cols).normal(size=(n_frames, cols))
    d = xs - mean
    want, bound = d.T @ p, f64_bound(d, p)
    for a in (mean, p, want, bound):
        a.setflags(write=False)
    return stored, sel, mean, p, want, bound


def engine_backproject(eng, stored, sel, mean, p, batch, skip, prefill=None, pad_p=5, pad_y=4, pad_rows=3):
    """The kernel over the case, batch by batch (``accumulate`` from the
    second on, or from the first onto ``prefill``): d_p rows ``pad_p`` wider
    than cols (NaN there: never read), d_y ``pad_y`` wider and ``pad_rows``
    longer, a sentinel there."""
    import torch
    n_frames, cols = p.shape
    n_sel = len(mean) // 3
    x = torch.tensor(stored, device="cuda:0")
    fstride = skip * x.stride(0)
    p_d = torch.full((n_frames, cols + pad_p), float("nan"), dtype=torch.float64, device="cuda:0")
    p_d[:, :cols] = torch.tensor(p, device="cuda:0")
    y = torch.full((3 * n_sel + pad_rows, cols + pad_y), SENTINEL, dtype=torch.float64, device="cuda:0")
    if prefill is not None:
        y[:3 * n_sel, :cols] = torch.tensor(prefill, device="cuda:0")
    mean_d = torch.tensor(mean, device="cuda:0")
    sel_d = eng.sel_tensor(sel)
    bf = batch or n_frames
    for f0 in range(0, n_frames, bf):
        n = min(bf, n_frames - f0)
        need = eng.pca_backproject_workspace_bytes(n, n_sel, cols)
        work = eng.empty(need // 8) if need else None
        eng.pca_backproject(x.data_ptr() + 4 * f0 * fstride, fstride, n, n_sel, sel_d, None, None, mean_d,
                            p_d[f0:f0 + n], cols, y, f0 > 0 or prefill is not None, work)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
@pytest.mark.parametrize("n_sel,n_frames,cols,batch,skip", ENGINE_SHAPES)
def test_engine_backprojection_unaligned(n_sel, n_frames, cols, batch, skip, gathered):
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    stored, sel, mean, p, want, bound = engine_case(n_sel, n_frames, cols, gathered, skip)
    if n_frames == 5000:   # the split-K plan: the fold launch is exercised
        assert eng.pca_backproject_workspace_bytes(n_frames, n_sel, cols) > 0
    if n_sel == 5000:      # many tiles: one frame range
        assert eng.pca_backproject_workspace_bytes(n_frames, n_sel, cols) == 0
    n = 3 * n_sel
    what = f"engine {n_sel}x{n_frames}x{cols}"
    y = engine_backproject(eng, stored, sel, mean, p, batch, skip)
    assert_within(y[:n, :cols], want, bound, what)
    assert np.all(y[:n, cols:] == SENTINEL), "padding columns of d_y were written"
    assert np.all(y[n:] == SENTINEL), "rows past 3 n_sel were written"
    # the same call again: the same bits
    again = engine_backproject(eng, stored, sel, mean, p, batch, skip)
    assert np.array_equal(bits(again), bits(y))
    # accumulate = 1 from the first batch on, onto a prefilled Y
    prefill = np.random.default_rng(n_sel + cols).normal(size=(n, cols)) * (1.0 + np.abs(want))
    acc = engine_backproject(eng, stored, sel, mean, p, batch, skip, prefill=prefill)
    assert_within(acc[:n, :cols], prefill + want, bound + 2.0 ** -53 * np.abs(prefill + want), what + " accumulate")
    assert np.all(acc[:n, cols:] == SENTINEL) and np.all(acc[n:] == SENTINEL)


def test_engine_argument_checks():
    import torch

    from rmsf_amd._lib import RMSF_EINVAL, RmsfError
    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    x = torch.zeros((4, 5, 3), dtype=torch.float32, device="cuda:0")
    mean, pm, y = eng.zeros(15), eng.zeros(4, 64), eng.zeros(15, 64)
    xf, info = eng.zeros(4, 16), eng.zeros(2064)
    p, m, c, o = x.data_ptr(), mean.data_ptr(), pm.data_ptr(), y.data_ptr()
    st = eng.stream
    bad = [
        (None, 15, 4, 5, None, None, None, m, c, 64, 4, o, 64, 0, None, 0, st),     # NULL d_xyz
        (p, 15, 4, 5, None, None, None, None, c, 64, 4, o, 64, 0, None, 0, st),     # NULL d_mean
        (p, 15, 4, 5, None, None, None, m, None, 64, 4, o, 64, 0, None, 0, st),     # NULL d_p
        (p, 15, 4, 5, None, None, None, m, c, 64, 4, None, 64, 0, None, 0, st),     # NULL d_y
        (p, 15, 4, 5, None, None, None, m, c, 64, 0, o, 64, 0, None, 0, st),        # n_cols < 1
        (p, 15, 4, 5, None, None, None, m, c, 64, 49, o, 64, 0, None, 0, st),       # n_cols > 48
        (p, 15, 4, 5, None, None, None, m, c, 3, 4, o, 64, 0, None, 0, st),         # ldp < n_cols
        (p, 15, 4, 5, None, None, None, m, c, 64, 4, o, 3, 0, None, 0, st),         # ldy < n_cols
        (p, 15, 4, 5, None, xf.data_ptr(), None, m, c, 64, 4, o, 64, 0, None, 0, st),    # d_xform alone
        (p, 15, 4, 5, None, None, info.data_ptr(), m, c, 64, 4, o, 64, 0, None, 0, st),  # d_refinfo alone
    ]
    for args in bad:
        rc = eng.lib.rmsf_pca_backproject(*args)
        assert rc == RMSF_EINVAL, args
        assert b"rmsf_pca_backproject" in eng.lib.rmsf_last_error()
    # a split plan with too small a workspace
    assert eng.pca_backproject_workspace_bytes(5000, 5, 3) > 16
    big = torch.zeros((5000, 5, 3), dtype=torch.float32, device="cuda:0")
    with pytest.raises(RmsfError, match="workspace"):
        eng.pca_backproject(big.data_ptr(), 15, 5000, 5, None, None, None, eng.zeros(15), eng.zeros(5000, 3), 3,
                            eng.zeros(15, 3), False, eng.zeros(2))
    with pytest.raises(ValueError, match="buffer sizes"):
        eng.pca_backproject(p, 15, 4, 5, None, None, None, mean, pm, 4, eng.zeros(14, 4))
    torch.cuda.synchronize()
    assert float(y.abs().sum()) == 0.0


# ---- 2. adjointness with transform records -----------------------------------
def superposed(eng, x, sel_d, n_sel, n_frames):
    """(records [F, 16], refinfo) of the frame-parallel superposition on frame 0."""
    from rmsf_amd.pipeline import Superposer
    from rmsf_amd.sources import Batch
    ref, info = eng.reference_setup(n_sel, frame_ptr=x.data_ptr(), sel=sel_d)
    sup = Superposer(eng, n_sel, n_frames, None)
    return sup.run(Batch(x.data_ptr(), x.stride(0), n_frames, sel_d), ref, info), info


def numpy_xform(xs, rec, ref_com):
    """apply_xform restated: f32 after the shift, after the rotation, after
    the reference's centre (numpy's dot for the FMA chain)."""
    out = np.empty(xs.shape, np.float32)
    for f in range(len(xs)):
        p = (xs[f].astype(np.float64) - rec[f, 9:12]).astype(np.float32)
        r = (p.astype(np.float64) @ rec[f, :9].reshape(3, 3)).astype(np.float32)
        out[f] = (r.astype(np.float64) + ref_com).astype(np.float32)
    return out


@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
@pytest.mark.parametrize("n_sel,n_frames,cols", [(17, 33, 17), (214, 67, 48)])
def test_adjoint_of_the_projection(n_sel, n_frames, cols, gathered):
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    n_atoms, sel = selection(n_sel, gathered)
    traj = make_traj(n_atoms, n_frames)
    x = torch.tensor(traj, device="cuda:0")
    sel_d = eng.sel_tensor(sel)
    xf, info = superposed(eng, x, sel_d, n_sel, n_frames)
    n = 3 * n_sel
    rng = np.random.default_rng(n_sel)
    q, p = rng.normal(size=(n, cols)), rng.normal(size=(n_frames, cols))
    rec, ref_com = xf.cpu().numpy(), info.cpu().numpy()[:3]
    al = numpy_xform(traj if sel is None else traj[:, sel], rec, ref_com)
    mean = al.reshape(n_frames, n).astype(np.float64).mean(axis=0)
    mean_d, q_d, p_d = (torch.tensor(a, device="cuda:0") for a in (mean, q, p))

    def both(records, sel_t):
        proj, back = eng.empty(n_frames, cols), eng.empty(n, cols)
        need = eng.pca_project_workspace_bytes(n_frames, n_sel, cols)
        eng.pca_project(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_t, records, info, mean_d, q_d, cols, proj,
                        eng.empty(need // 8) if need else None)
        need = eng.pca_backproject_workspace_bytes(n_frames, n_sel, cols)
        eng.pca_backproject(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_t, records, info, mean_d, p_d, cols,
                            back, False, eng.empty(need // 8) if need else None)
        torch.cuda.synchronize()
        return proj.cpu().numpy(), back.cpu().numpy()

    proj, back = both(xf, sel_d)
    lhs, rhs = float((p * proj).sum()), float((back * q).sum())
    u = float(np.spacing(np.float32(np.abs(al).max())))
    d = np.abs(al.reshape(n_frames, n).astype(np.float64) - mean) + u
    bound = (8.0 * n * EPS * float((np.abs(p) * (d @ np.abs(q))).sum())          # the projection's, against |P|
             + 8.0 * n_frames * EPS * float(((d.T @ np.abs(p)) * np.abs(q)).sum())  # the back-projection's, against |Q|
             + cols * (n + n_frames) * 2.0 ** -53 * float((np.abs(p) * (d @ np.abs(q))).sum()))  # numpy's two sums
    print(f"adjoint {n_sel}x{n_frames}x{cols}: <P, DQ> = {lhs:.6e}, |diff| / bound = {abs(lhs - rhs) / bound:.3e}")
    assert abs(lhs - rhs) <= bound
    # and the back-projection itself, against numpy on the restated aligned frames, at the f32 term
    dd = al.reshape(n_frames, n).astype(np.float64) - mean
    assert_within(back, dd.T @ p, f64_bound(dd, p) + 4.0 * u * np.abs(p).sum(axis=0)[None, :], "aligned, restated")
    # a wrong record (the frames' records shifted by one) moves the identity's two sides apart by order 1
    wrong = torch.roll(xf, 1, 0).contiguous()
    _, back_wrong = both(wrong, sel_d)
    assert abs(lhs - float((back_wrong * q).sum())) > 1e6 * bound


# ---- 3. aligned, against the oracle -------------------------------------------
def test_backprojection_aligned_against_the_oracle():
    """214 atoms x 67 frames, align="average": the superposition of a PCA
    run's last sweep (its reference, ``Superposer``), the back-projection of a
    random P, against numpy on the frames the oracle aligned."""
    import torch

    from oracle import rmsf_oracle as O
    from rmsf_amd import PCA
    from rmsf_amd.engine import Engine
    from rmsf_amd.pipeline import Superposer
    from rmsf_amd.sources import Batch
    n_sel, n_frames, cols = 214, 67, 10
    traj = make_traj(n_sel, n_frames)
    sel = np.arange(n_sel)
    average = O.rmsf_script(traj, sel, None, size=1, align="average")["average"]
    ref_com, ref = O.centred_reference(average, None)
    aligned = np.empty((n_frames, n_sel, 3), np.float32)
    for f in range(n_frames):
        aligned[f] = O.align_frame_(traj[f].astype(np.float32, copy=True), None, ref, ref_com)
    x = torch.tensor(traj, device="cuda:0")
    pca = PCA(x, align="average", exact=False, n_components=3).run()
    last = pca._rmsf._last_run
    eng = Engine(torch.device("cuda", 0))
    xf = Superposer(eng, n_sel, n_frames, None).run(Batch(x.data_ptr(), x.stride(0), n_frames, None), last["ref"],
                                                    last["refinfo"])
    mean = pca.results.mean.reshape(-1)
    p = np.random.default_rng(3).normal(size=(n_frames, cols))
    y = eng.empty(3 * n_sel, cols)
    need = eng.pca_backproject_workspace_bytes(n_frames, n_sel, cols)
    eng.pca_backproject(x.data_ptr(), x.stride(0), n_frames, n_sel, None, xf, last["refinfo"],
                        torch.tensor(mean, device="cuda:0"), torch.tensor(p, device="cuda:0"), cols, y, False,
                        eng.empty(need // 8) if need else None)
    torch.cuda.synchronize()
    d = aligned.reshape(n_frames, -1).astype(np.float64) - mean
    u = float(np.spacing(np.float32(np.abs(aligned).max())))
    assert_within(y.cpu().numpy(), d.T @ p, f64_bound(d, p) + 4.0 * u * np.abs(p).sum(axis=0)[None, :],
                  "aligned, oracle")
