"""GPU tier: the positional co-moment matrix (csrc/covariance.hip, the f64
MFMA kernel) and PCA, against a numpy f64 two-pass reference
(``d = x - x.mean(0); d.T @ d``) on raw frames (align=None) or on frames
aligned by the oracle's ``align_frame_``.

Data: base positions in a 100 A box, three planted collective modes plus
0.3 A noise, a random rigid motion per frame, f32 -- so the off-diagonals
carry signal and the matrix is far from symmetric under a block transpose.

Bounds (derived, not measured):
  * unaligned, ``max |M_gpu - M_ref| <= 1e-9 max_k M_ref[k, k]``: f64
    summation error is at most F 2^-53 sum |d_i d_j|, ~1e-13 of that scale at
    these sizes; a dropped frame or a misplaced row moves elements by >= 1/F.
  * aligned, per element ``|dM_ij| <= 2 u sqrt(F) (sqrt(M_ii) + sqrt(M_jj))
    + 4 u^2 F + 1e-9 sqrt(M_ii M_jj)``, u = spacing(f32(max |aligned x|)): the
    Cauchy-Schwarz bound for one f32 rounding flip of size u in every frame
    of both coordinates, doubled (the frame-parallel rotation may differ from
    the oracle's in its last bits).
"""
import functools
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

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


def two_pass(x: np.ndarray) -> np.ndarray:
    d = x.reshape(len(x), -1).astype(np.float64)
    d = d - d.mean(axis=0)
    return d.T @ d


@functools.lru_cache(maxsize=None)
def ref_unaligned(n_sel: int, n_frames: int, gathered: bool) -> np.ndarray:
    n_atoms, sel = selection(n_sel, gathered)
    x = make_traj(n_atoms, n_frames)
    return two_pass(x if sel is None else x[:, sel])


@functools.lru_cache(maxsize=None)
def ref_aligned(n_sel: int, n_frames: int, gathered: bool, align: str):
    """(M_ref, max |aligned x|) of the oracle-aligned frames (RMSF.py:94-101;
    the average of RMSF.py:89-111 from rmsf_script for align="average")."""
    from oracle import rmsf_oracle as O
    n_atoms, sel = selection(n_sel, gathered)
    traj = make_traj(n_atoms, n_frames)
    sel = np.arange(n_atoms) if sel is None else sel
    if align == "average":
        average = O.rmsf_script(traj, sel, None, size=1, align="average")["average"]
        ref_com, ref = O.centred_reference(average, None)
    else:
        ref_com, ref = O.centred_reference(traj[0][sel], None)
    out = np.empty((n_frames, len(sel), 3), np.float32)
    for f in range(n_frames):
        p = traj[f][sel].astype(np.float32, copy=True)
        out[f] = O.align_frame_(p, None, ref, ref_com)
    return two_pass(out), float(np.abs(out).max())


def aligned_bound(m_ref: np.ndarray, xmax: float, n_frames: int) -> np.ndarray:
    u = float(np.spacing(np.float32(xmax)))
    s = np.sqrt(m_ref.diagonal())
    return (2 * u * np.sqrt(n_frames) * (s[:, None] + s[None, :]) + 4 * u * u * n_frames
            + 1e-9 * np.sqrt(np.outer(m_ref.diagonal(), m_ref.diagonal())))


def assert_symmetric_bits(m: np.ndarray) -> None:
    assert np.array_equal(m.view(np.uint64), np.ascontiguousarray(m.T).view(np.uint64)), "M != M.T"


@functools.lru_cache(maxsize=None)
def run_rmsf(n_sel: int, n_frames: int, gathered: bool, align, exact, batch_frames=None, rep: int = 0):
    """One RMSF(..., covariance=True) run on cuda:0 (cached; ``rep``
    distinguishes repeated runs)."""
    import torch

    from rmsf_amd import RMSF
    n_atoms, sel = selection(n_sel, gathered)
    x = torch.tensor(make_traj(n_atoms, n_frames), device="cuda:0")
    r = RMSF(x, select=sel, align=align, exact=exact, batch_frames=batch_frames, covariance=True).run().results
    assert r.get("covariance") is not None and r.get("comoment") is not None, "covariance=True returned no matrix"
    return r


# ---- 1. engine level, no alignment -----------------------------------------
# (500, 40): 528 tile pairs and two stages -- k_comoment_tiles straight to d_cov over more than one stage
ENGINE_SHAPES = [(1, 1, None), (5, 3, None), (16, 4, None), (17, 5, None), (214, 67, None), (341, 300, 128),
                 (500, 40, None)]


@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
@pytest.mark.parametrize("n_sel,n_frames,batch", ENGINE_SHAPES)
def test_engine_comoment_unaligned(n_sel, n_frames, batch, gathered):
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    n_atoms, sel = selection(n_sel, gathered)
    traj = make_traj(n_atoms, n_frames)
    x = torch.tensor(traj, device="cuda:0")
    sel_dev = eng.sel_tensor(sel)
    first = traj[0] if sel is None else traj[0][sel]
    shift = torch.tensor(first.reshape(-1).astype(np.float64), device="cuda:0")
    n = 3 * n_sel
    cov, t1 = eng.zeros(n, n), eng.zeros(n)
    bf = batch or n_frames
    for k in range(0, n_frames, bf):
        nb = min(bf, n_frames - k)
        need = eng.covariance_workspace_bytes(n_sel, nb)
        work = eng.empty(need // 8) if need else None
        eng.covariance_accumulate(x.data_ptr() + 4 * k * x.stride(0), x.stride(0), nb, n_sel, sel_dev, None, None,
                                  shift, cov, t1, work)
    eng.covariance_finish(cov, t1, n, n_frames)
    torch.cuda.synchronize()
    m = cov.cpu().numpy()
    m_ref = ref_unaligned(n_sel, n_frames, gathered)
    scale = m_ref.diagonal().max()
    err = np.abs(m - m_ref).max()
    print(f"unaligned ({n_sel}, {n_frames}) gathered={gathered}: max |dM| = {err:.3e}, scale {scale:.3e}")
    assert_symmetric_bits(m)
    if n_frames == 1:
        assert not m.any(), "one frame: the co-moment is exactly zero"
    assert err <= 1e-9 * scale
    # the same through the public interface (its shift: the first frame's rows)
    r = run_rmsf(n_sel, n_frames, gathered, None, None, batch)
    assert r.comoment.shape == (n, n) and r.comoment.dtype == np.float64
    assert_symmetric_bits(r.comoment)
    assert np.abs(r.comoment - m_ref).max() <= 1e-9 * scale
    np.testing.assert_array_equal(r.covariance, r.comoment / n_frames)
    if n_frames == 1:
        assert not r.comoment.any()


# ---- 2. aligned -------------------------------------------------------------
ALIGNED_CASES = [(17, 5, None, False), (214, 67, None, False), (341, 300, 128, False), (341, 300, 128, True)]


@pytest.mark.parametrize("exact", [False, True], ids=["parallel", "exact"])
@pytest.mark.parametrize("align", ["frame0", "average"])
@pytest.mark.parametrize("n_sel,n_frames,batch,gathered", ALIGNED_CASES)
def test_comoment_aligned(n_sel, n_frames, batch, gathered, align, exact):
    r = run_rmsf(n_sel, n_frames, gathered, align, exact, batch)
    m = r.comoment
    assert m.shape == (3 * n_sel, 3 * n_sel)
    assert_symmetric_bits(m)
    # (a) the diagonal is the Welford sweep's sum of squares: the same
    # aligned bits through two kernels
    diag, ss = m.diagonal(), r.sumsquares.ravel()
    da = np.abs(diag - ss).max()
    # (b) against the oracle-aligned two-pass reference, per element
    m_ref, xmax = ref_aligned(n_sel, n_frames, gathered, align)
    bound = aligned_bound(m_ref, xmax, n_frames)
    ratio = (np.abs(m - m_ref) / bound).max()
    print(f"aligned ({n_sel}, {n_frames}) {align} exact={exact} gathered={gathered}: "
          f"max |diag - sumsquares| = {da:.3e} (scale {diag.max():.3e}), max |dM| / bound = {ratio:.3e}")
    assert da <= 1e-9 * diag.max()
    assert ratio <= 1.0
    # the docstring's identity: the diagonal, summed per atom, is rmsf**2
    np.testing.assert_allclose(r.covariance.diagonal().reshape(n_sel, 3).sum(1), r.rmsf ** 2, rtol=1e-9, atol=0)


# ---- 3. determinism ---------------------------------------------------------
@pytest.mark.parametrize("align", ["average"])
def test_comoment_is_deterministic(align):
    a = run_rmsf(214, 67, False, align, False, None, rep=0).comoment
    b = run_rmsf(214, 67, False, align, False, None, rep=1).comoment
    assert a is not b
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 4. ranks ---------------------------------------------------------------
def _rank_worker(rank, size, init, q, align, root):
    sys.path[:0] = [ROOT, PKG, ROOT + "/tests"]
    import torch
    import torch.distributed as dist

    from conftest import init_gloo
    init_gloo(init, rank, size)
    try:
        from rmsf_amd import RMSF
        x = torch.tensor(make_traj(214, 67), device="cuda:0")
        r = RMSF(x, align=align, exact=False, merge_root=root, covariance=True).run().results
        q.put((rank, r.get("comoment", "missing"), r.n_local))
    except Exception as e:  # noqa: BLE001  (surface the failure to the parent)
        q.put((rank, repr(e), -1))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("size,align,root", [(2, None, None), (2, "average", None), (3, None, None),
                                             (3, "average", 0)])
def test_comoment_over_ranks(size, align, root):
    from conftest import spawn_ranks
    out = spawn_ranks(_rank_worker, size, lambda r, init, q: (r, size, init, q, align, root), timeout=100)
    for rank, m, n_local in out:
        assert n_local >= 0, m
    assert sorted(o[2] for o in out) == sorted([67 // size] * (size - 1) + [67 - (size - 1) * (67 // size)])
    one = run_rmsf(214, 67, False, align, False, None).comoment
    if align is None:
        bound = 1e-9 * one.diagonal().max()
    else:
        bound = aligned_bound(one, ref_aligned(214, 67, False, align)[1], 67)
    for rank, m, _ in out:
        if root is not None and rank != root:
            assert m is None, f"rank {rank} is not the merge root"
            continue
        assert isinstance(m, np.ndarray), m
        assert_symmetric_bits(m)
        print(f"{size} ranks, {align}: rank {rank} max |dM| / bound = {(np.abs(m - one) / bound).max():.3e}")
        assert np.all(np.abs(m - one) <= bound)


# ---- 5. PCA end to end ------------------------------------------------------
def test_pca_end_to_end():
    import torch

    from rmsf_amd import PCA
    n_sel, n_frames = 214, 300
    x = torch.tensor(make_traj(n_sel, n_frames), device="cuda:0")
    p = PCA(x, align="average", exact=False).run()
    res = p.results
    m_ref, _ = ref_aligned(n_sel, n_frames, False, "average")
    w, v = np.linalg.eigh(m_ref / (n_frames - 1))
    w, v = w[::-1], v[:, ::-1]
    assert res.p_components.shape == (3 * n_sel, 3 * n_sel) and res.variance.shape == (3 * n_sel,)
    assert res.cumulated_variance[-1] == pytest.approx(1.0, abs=1e-12)
    assert res.covariance.shape == (3 * n_sel, 3 * n_sel) and res.rmsf.shape == (n_sel,) and res.mean.shape == (n_sel, 3)
    rel = np.abs(res.variance[:3] - w[:3]) / w[:3]
    cos = np.abs(np.einsum("ik,ik->k", res.p_components[:, :3], v[:, :3]))
    print(f"PCA (214, 300): variance {res.variance[:3]}, rel err {rel}, 1 - |cos| {1 - cos}")
    assert w[2] > 10 * w[3], "the three planted modes stand clear of the noise"
    assert np.all(rel <= 1e-6)
    assert np.all(cos >= 1 - 1e-6)
    k3 = PCA(x, align="average", exact=False, n_components=3, ddof=0).run().results
    assert k3.p_components.shape == (3 * n_sel, 3) and k3.variance.shape == (3,)
    np.testing.assert_allclose(k3.variance * n_frames, res.variance[:3] * (n_frames - 1), rtol=1e-12)


# ---- 6. covariance=False ----------------------------------------------------
def test_covariance_off_returns_no_matrix():
    import torch

    from rmsf_amd import RMSF
    x = torch.tensor(make_traj(17, 5), device="cuda:0")
    for kw in ({}, dict(covariance=False)):
        r = RMSF(x, align="average", **kw).run().results
        assert "covariance" not in r and "comoment" not in r
    on = run_rmsf(17, 5, False, "average", None)
    np.testing.assert_array_equal(on.rmsf, r.rmsf)    # the statistics do not move with the option


# ---- the matrix must fit ----------------------------------------------------
def test_matrix_over_half_the_free_hbm_is_refused():
    """200k atoms: a 600,000^2 f64 matrix, 2.9 TB -- a MemoryError stating the
    bytes, before any launch (two 2.4 MB frames are all that is allocated)."""
    import torch

    from rmsf_amd import RMSF
    x = torch.zeros((2, 200_000, 3), dtype=torch.float32, device="cuda:0")
    for align in (None, "average"):
        with pytest.raises(MemoryError, match=str(8 * 600_000 ** 2)):
            RMSF(x, align=align, covariance=True).run()
