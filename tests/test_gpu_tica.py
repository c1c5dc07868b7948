"""GPU tier of TICA: the lagged co-moment kernel (csrc/covariance.hip's tile
body over the full square of tiles), its finish, and ``TICA`` end to end, against
the reversible estimator restated in numpy f64 (tests/test_tica_host.py::
reversible_comoments) on raw frames or on frames aligned by the oracle's
``align_frame_``.  Data: tests/test_tica_host.py::make_lagged_traj.

Bounds:
  * unaligned S, ``max |S - S_ref| <= 1e-9 max_k sum_t d_k^2`` -- the derived
    bound of tests/test_gpu_covariance.py: f64 summation error is ~1e-13 of
    that scale, a dropped pair moves an element by >= 1/N of it.
  * finish: 1 ulp per element of ``(S + S^T) - T T^T / m`` as numpy rounds it.
  * aligned matrices: tests/test_gpu_covariance.py::aligned_bound with F -> 2N
    and the diagonal of the reference's 2N C0, applied to 2N C0 and to 2N C_lag
    (Cauchy-Schwarz for one f32 flip in every frame of both coordinates: both
    matrices are sums of 2N such products of the same deviations).
  * spectrum: measured against the reference alone, see
    ``test_spectrum_end_to_end``.
  * transform: tests/test_gpu_pca_project.py's bound.
"""
import functools

import numpy as np
import pytest

from test_gpu_covariance import aligned_bound, assert_symmetric_bits, selection
from test_gpu_pca_project import assert_within, bits, f64_bound
from test_tica_host import make_lagged_traj, reversible_comoments

pytestmark = pytest.mark.gpu


# ---- 1. engine level, no alignment -----------------------------------------
# (n_sel, F, lag, batch of pairs)
ENGINE_SHAPES = [(1, 2, 1, None), (5, 3, 2, None), (16, 33, 1, None), (17, 40, 7, None), (33, 65, 32, None),
                 (33, 40, 37, None), (214, 67, 32, None), (341, 300, 31, 128), (368, 40, 1, None)]


def engine_lagged(eng, x, sel_dev, shift, n_sel, n_frames, lag, batch):
    n, n_pairs = 3 * n_sel, n_frames - lag
    s = eng.zeros(n, n)
    nb_max = batch or n_pairs
    for k in range(0, n_pairs, nb_max):
        nb = min(nb_max, n_pairs - k)
        need = eng.lagged_comoment_workspace_bytes(n_sel, nb)
        work = eng.empty(need // 8) if need else None
        a = x.data_ptr() + 4 * k * x.stride(0)
        eng.lagged_comoment_accumulate(a, x.stride(0), a + 4 * lag * x.stride(0), x.stride(0), nb, n_sel, sel_dev,
                                       None, None, None, shift, s, work)
    return s


@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
@pytest.mark.parametrize("n_sel,n_frames,lag,batch", ENGINE_SHAPES)
def test_engine_lagged_comoment_unaligned(n_sel, n_frames, lag, batch, gathered):
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    n_atoms, sel = selection(n_sel, gathered)
    traj = make_lagged_traj(n_atoms, n_frames)
    x = torch.tensor(traj, device="cuda:0")
    sel_dev = eng.sel_tensor(sel)
    rows = traj if sel is None else traj[:, sel]
    d = rows.reshape(n_frames, -1).astype(np.float64)
    d = d - d[0]
    shift = torch.tensor(rows[0].reshape(-1).astype(np.float64), device="cuda:0")
    n_pairs = n_frames - lag
    s_ref = d[:n_pairs].T @ d[lag:]
    scale = (d * d).sum(axis=0).max()
    s = engine_lagged(eng, x, sel_dev, shift, n_sel, n_frames, lag, batch)
    torch.cuda.synchronize()
    got = s.cpu().numpy()
    err = np.abs(got - s_ref).max()
    asym = np.abs(s_ref - s_ref.T).max()
    print(f"lagged ({n_sel}, {n_frames}, lag {lag}) gathered={gathered}: max |dS| = {err:.3e}, scale {scale:.3e}, "
          f"max |S - S^T| of the reference {asym:.3e}")
    assert err <= 1e-9 * scale
    # the same bits from a second identical run
    again = engine_lagged(eng, x, sel_dev, shift, n_sel, n_frames, lag, batch).cpu().numpy()
    assert np.array_equal(bits(again), bits(got))


# (n_sel, F): one tile; two tiles a side with an atom in the second; three tiles with a ragged stage
SAME_OPERAND_SHAPES = [(5, 3), (17, 32), (33, 20)]


@pytest.mark.parametrize("aligned", [False, True], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("gathered", [False, True], ids=["dense", "gathered"])
@pytest.mark.parametrize("n_sel,n_frames", SAME_OPERAND_SHAPES)
def test_lagged_with_one_operand_twice_is_the_covariance_kernel(n_sel, n_frames, gathered, aligned):
    """The two instantiations of the co-moment tile body against each other:
    with B = A (pointer, stride, records) the time-lagged kernel stages the
    doubles the positional kernel stages, contracts them in the same MFMA order
    and sums the waves alike, so at F <= 32 -- one stage, one frame range in
    both plans -- S equals C bit for bit on the tile pairs J >= I that the
    positional kernel writes, and S is symmetric in its bits."""
    import torch

    from rmsf_amd.engine import Engine
    from test_gpu_pca_backproject import superposed
    eng = Engine(torch.device("cuda", 0))
    assert eng.covariance_workspace_bytes(n_sel, n_frames) == 0
    assert eng.lagged_comoment_workspace_bytes(n_sel, n_frames) == 0
    n_atoms, sel = selection(n_sel, gathered)
    x = torch.tensor(make_lagged_traj(n_atoms, n_frames), device="cuda:0")
    sel_dev = eng.sel_tensor(sel)
    xf, info = superposed(eng, x, sel_dev, n_sel, n_frames) if aligned else (None, None)
    rows = x[0] if sel_dev is None else x[0][sel_dev.long()]
    shift = rows.reshape(-1).double().contiguous()
    n = 3 * n_sel
    s, c, t1 = eng.zeros(n, n), eng.zeros(n, n), eng.zeros(n)
    eng.lagged_comoment_accumulate(x.data_ptr(), x.stride(0), x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev,
                                   xf, xf, info, shift, s)
    eng.covariance_accumulate(x.data_ptr(), x.stride(0), n_frames, n_sel, sel_dev, xf, info, shift, c, t1)
    torch.cuda.synchronize()
    s, c = s.cpu().numpy(), c.cpu().numpy()
    tile = np.arange(n) // 48
    written = tile[None, :] >= tile[:, None]                # whole 48 x 48 tile pairs J >= I
    assert np.any(s != 0.0)
    differ = int((bits(s)[written] != bits(c)[written]).sum())
    print(f"B = A ({n_sel}, {n_frames}) gathered={gathered} aligned={aligned}: {differ} of {int(written.sum())} "
          f"elements differ")
    assert differ == 0
    assert_symmetric_bits(s)


# ---- 2. finish --------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 32, 33, 97])
def test_finish_is_symmetric_and_numpy_within_an_ulp(n):
    import torch

    from rmsf_amd.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    rng = np.random.default_rng(n)
    s = rng.normal(size=(n, n)) * 10.0 ** rng.uniform(-3, 3, size=(n, n))
    t = rng.normal(size=n) * 30.0
    m = 2 * 37
    want = (s + s.T) - np.outer(t, t) / float(m)
    ld = n + 5                                              # rows wider than the matrix: the padding is not touched
    buf = torch.full((n, ld), -7.25e77, dtype=torch.float64, device="cuda:0")
    buf[:, :n] = torch.tensor(s, device="cuda:0")
    eng.lagged_comoment_finish(buf, torch.tensor(t, device="cuda:0"), n, m)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    got = np.ascontiguousarray(out[:, :n])
    assert np.all(out[:, n:] == -7.25e77)
    assert_symmetric_bits(got)
    ulps = np.abs(got - want) / np.spacing(np.abs(want))
    print(f"finish n = {n}: max error {ulps.max():.2f} ulp")
    assert np.all(ulps <= 1.0)


# ---- 3. aligned matrices ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_aligned(n_sel: int, n_frames: int, gathered: bool, align: str):
    """(aligned f32 [F, n_sel, 3], max |aligned x|) of the generator's frames,
    by the oracle as tests/test_gpu_covariance.py::ref_aligned uses it."""
    from oracle import rmsf_oracle as O
    n_atoms, sel = selection(n_sel, gathered)
    traj = make_lagged_traj(n_atoms, n_frames)
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
    out.setflags(write=False)
    return out, float(np.abs(out).max())


@functools.lru_cache(maxsize=None)
def run_tica(n_sel, n_frames, lag, gathered, align, exact=False, n_components=None, where="hbm", batch=None,
             transforms=False):
    import torch

    from rmsf_amd import TICA
    n_atoms, sel = selection(n_sel, gathered)
    traj = make_lagged_traj(n_atoms, n_frames)
    x = torch.tensor(traj, device="cuda:0") if where == "hbm" else np.array(traj)
    return TICA(x, lag, select=sel, align=align, exact=exact, n_components=n_components, keep_matrices=True,
                batch_frames=batch, collect_transforms=transforms).run()


ALIGNED_CASES = [(12, 600, 5, False, False), (12, 600, 5, True, False), (40, 300, 7, False, False),
                 (40, 300, 7, True, False), (40, 300, 7, False, True)]


@pytest.mark.parametrize("align", ["frame0", "average"])
@pytest.mark.parametrize("n_sel,n_frames,lag,gathered,exact", ALIGNED_CASES)
def test_matrices_aligned(n_sel, n_frames, lag, gathered, exact, align):
    r = run_tica(n_sel, n_frames, lag, gathered, align, exact).results
    n_pairs = n_frames - lag
    assert (r.n_frames, r.n_pairs, r.lag) == (n_frames, n_pairs, lag)
    assert r.cov0.shape == r.cov_lag.shape == (3 * n_sel, 3 * n_sel) and r.mean.shape == (n_sel, 3)
    assert_symmetric_bits(r.cov0)
    assert_symmetric_bits(r.cov_lag)
    aligned, xmax = oracle_aligned(n_sel, n_frames, gathered, align)
    m0_ref, mt_ref, mu_ref = reversible_comoments(aligned, lag)
    bound = aligned_bound(m0_ref, xmax, 2 * n_pairs)
    r0 = (np.abs(2 * n_pairs * r.cov0 - m0_ref) / bound).max()
    rt = (np.abs(2 * n_pairs * r.cov_lag - mt_ref) / bound).max()
    du = np.abs(r.mean.reshape(-1) - mu_ref).max()
    print(f"aligned ({n_sel}, {n_frames}, lag {lag}) {align} exact={exact} gathered={gathered}: max |dM0| / bound = "
          f"{r0:.3e}, max |dM_lag| / bound = {rt:.3e}, max |d mu| = {du:.3e}")
    assert r0 <= 1.0 and rt <= 1.0
    assert du <= 2.0 * float(np.spacing(np.float32(xmax)))
    assert r.rank == 3 * n_sel - 6


# ---- 4. the spectrum, end to end --------------------------------------------
def restated_tica(x, lag, epsilon=1e-6):
    """The estimator and its truncated solve, restated: (lambda, V, C0, the
    whole spectrum of C0)."""
    m0, mt, _ = reversible_comoments(x, lag)
    n2 = 2.0 * (len(x) - lag)
    c0, ct = m0 / n2, mt / n2
    s, u = np.linalg.eigh(c0)
    keep = s > epsilon * s.max()
    el = u[:, keep] / np.sqrt(s[keep])
    w, v = np.linalg.eigh(el.T @ ct @ el)
    return w[::-1], (el @ v)[:, ::-1], c0, s


def flipped(x, seed):
    """Every coordinate moved to its f32 neighbour above or below, at random."""
    rng = np.random.default_rng(seed)
    up = rng.integers(0, 2, size=x.shape).astype(bool)
    return np.where(up, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))).astype(np.float32)


SPECTRUM_FACTOR = 10.0


def test_spectrum_end_to_end():
    """(12 atoms, 600 frames, lag 5, align="average"): the first three
    eigenvalues and |V^T C0 V_ref| = I for the first three components against
    the restatement on the oracle-aligned frames.

    The tolerance is measured here, against the reference alone: the
    restatement is run on the oracle-aligned frames and on those frames with
    every coordinate moved by one f32 ulp up or down at random, 8 seeds; the
    tolerance is SPECTRUM_FACTOR = 10 times the largest change seen -- 10,
    because the device's rotation may differ from the oracle's in its last
    bits in every frame, a coherent change of the frame's coordinates, where
    the probe moves each coordinate independently.  Measured with the
    committed generator: largest change of the three eigenvalues 4.7e-07
    (tolerance 4.7e-06), of |V^T C0 V_ref| - I 6.9e-07 (tolerance 6.9e-06);
    the test prints both.  The noise bulk under the planted modes moves by
    ~1e-6 and is not compared."""
    n_sel, n_frames, lag, eps = 12, 600, 5, 1e-6
    aligned, _ = oracle_aligned(n_sel, n_frames, False, "average")
    w_ref, v_ref, c0_ref, s0 = restated_tica(aligned, lag, eps)
    # conditions on the reference, not measurements
    gaps = -np.diff(w_ref[:4])
    print(f"reference eigenvalues {w_ref[:5]}, spectrum of C0 / max: kept >= {s0[s0 > eps * s0.max()].min() / s0.max():.3e}, "
          f"dropped <= {np.abs(s0[s0 <= eps * s0.max()]).max() / s0.max():.3e}")
    assert np.all(gaps >= 0.1), "the three planted eigenvalues stand 0.1 apart from each other and from the fourth"
    assert not np.any((s0 > 1e-2 * eps * s0.max()) & (s0 < 1e2 * eps * s0.max())), "rank cannot move by rounding"
    assert int((s0 > eps * s0.max()).sum()) == 3 * n_sel - 6
    dw, dv = 0.0, 0.0
    for seed in range(8):
        w, v, _, _ = restated_tica(flipped(aligned, seed), lag, eps)
        dw = max(dw, np.abs(w[:3] - w_ref[:3]).max())
        dv = max(dv, np.abs(np.abs(v[:, :3].T @ c0_ref @ v_ref[:, :3]) - np.eye(3)).max())
    tol_w, tol_v = SPECTRUM_FACTOR * dw, SPECTRUM_FACTOR * dv
    print(f"one-ulp probe, 8 seeds: largest change of lambda[:3] {dw:.3e}, of |V^T C0 V_ref| - I {dv:.3e}")
    t = run_tica(n_sel, n_frames, lag, False, "average")
    r = t.results
    assert r.rank == 3 * n_sel - 6 and r.eigenvalues.shape == (30,) and r.components.shape == (36, 30)
    err_w = np.abs(r.eigenvalues[:3] - w_ref[:3]).max()
    err_v = np.abs(np.abs(r.components[:, :3].T @ c0_ref @ v_ref[:, :3]) - np.eye(3)).max()
    print(f"device: eigenvalues {r.eigenvalues[:4]}, max |d lambda| = {err_w:.3e} (tolerance {tol_w:.3e}), "
          f"max ||V^T C0 V_ref| - I| = {err_v:.3e} (tolerance {tol_v:.3e})")
    assert err_w <= tol_w
    assert err_v <= tol_v
    np.testing.assert_allclose(r.timescales[:3], -lag / np.log(np.abs(r.eigenvalues[:3])), rtol=1e-12)
    assert np.all(np.diff(r.kinetic_variance) >= 0) and r.kinetic_variance[-1] == pytest.approx(1.0, abs=1e-12)


# ---- 5. transform -----------------------------------------------------------
@pytest.mark.parametrize("align,gathered", [("average", False), ("frame0", True), (None, False)])
def test_transform(align, gathered):
    from oracle import rmsf_oracle as O
    n_sel, n_frames, lag = 40, 300, 7
    t = run_tica(n_sel, n_frames, lag, gathered, align, n_components=5, transforms=align is not None)
    r = t.results
    proj = t.transform()
    assert proj.shape == (n_frames, 5) and proj.dtype == np.float64
    n_atoms, sel = selection(n_sel, gathered)
    traj = make_lagged_traj(n_atoms, n_frames)
    rows = np.array(traj if sel is None else traj[:, sel])
    extra = 0.0
    if align is not None:
        # the frames as the device's own records place them (RMSF.py:99-101 with the device's R and COM)
        rec = t._rmsf.results.transforms
        ref_com = t._rmsf._last_run["refinfo"][:3].cpu().numpy()
        for f in range(n_frames):
            O.apply_transform_(rows[f], rec[f, :9].reshape(3, 3), rec[f, 9:12], ref_com)
        u = float(np.spacing(np.float32(np.abs(rows).max())))
        extra = 4.0 * u * np.abs(r.components).sum(axis=0)
    d = rows.reshape(n_frames, -1).astype(np.float64) - r.mean.reshape(-1)
    assert_within(proj, d @ r.components, f64_bound(d, r.components) + extra, f"TICA.transform {align}")
    # the invariant: symmetrised variance 1 and symmetrised autocorrelation lambda at the lag
    n_pairs = n_frames - lag
    a, b = proj[:n_pairs], proj[lag:]
    var = ((a * a).sum(axis=0) + (b * b).sum(axis=0)) / (2.0 * n_pairs)
    acf = (a * b).sum(axis=0) / n_pairs
    mean = (a.sum(axis=0) + b.sum(axis=0)) / (2.0 * n_pairs)
    print(f"invariant {align}: max |mean| = {np.abs(mean).max():.3e}, max |var - 1| = {np.abs(var - 1).max():.3e}, "
          f"max |acf - lambda| = {np.abs(acf - r.eigenvalues).max():.3e}")
    assert np.abs(var - 1.0).max() <= 1e-9
    assert np.abs(acf - r.eigenvalues).max() <= 1e-9
    # a host copy of the same frames: the bits of the HBM input's projection
    assert np.array_equal(bits(t.transform(np.array(traj))), bits(proj))
    assert np.array_equal(bits(t.transform(n_components=2)), bits(proj[:, :2]))


# ---- 6. sources -------------------------------------------------------------
def test_sources_give_the_same_bits():
    """The frame-parallel superposition's sums round with the batch size, so
    each pair of runs is given one batching; the lagged matrix itself is
    contracted over all pairs at once, whatever the batches were."""
    import torch

    from rmsf_amd import TICA
    n_sel, n_frames, lag = 40, 300, 7
    traj = make_lagged_traj(n_sel, n_frames)
    kw = dict(align="frame0", keep_matrices=True, n_components=3)
    # a host array streamed in batches of 64: pairs straddle the batches
    dev = run_tica(n_sel, n_frames, lag, False, "frame0", batch=64).results
    host = TICA(np.array(traj), lag, batch_frames=64, **kw).run().results
    assert np.array_equal(bits(host.cov_lag), bits(dev.cov_lag))
    assert np.array_equal(bits(host.cov0), bits(dev.cov0))
    # an explicit scattered frame list, against the HBM tensor of those frames
    rng = np.random.default_rng(11)
    idx = np.concatenate([[0], np.sort(rng.choice(np.arange(1, n_frames), size=149, replace=False))])
    assert len(set(np.diff(idx))) > 1
    x = torch.tensor(traj, device="cuda:0")
    packed_x = torch.tensor(traj[idx], device="cuda:0")
    listed = TICA(x, lag, **kw).run(frames=idx).results
    packed = TICA(packed_x, lag, **kw).run().results
    assert listed.n_frames == 150 and listed.n_pairs == 150 - lag
    assert np.array_equal(bits(listed.cov_lag), bits(packed.cov_lag))
    assert np.array_equal(bits(listed.cov0), bits(packed.cov0))
    host_listed = TICA(np.array(traj), lag, batch_frames=64, **kw).run(frames=idx).results
    packed64 = TICA(packed_x, lag, batch_frames=64, **kw).run().results
    assert np.array_equal(bits(host_listed.cov_lag), bits(packed64.cov_lag))
    # a strided range of an HBM tensor is read in place
    strided = TICA(x, lag, **kw).run(step=2).results
    halved = TICA(torch.tensor(traj[::2], device="cuda:0"), lag, **kw).run().results
    assert np.array_equal(bits(strided.cov_lag), bits(halved.cov_lag))


def test_refusals():
    import torch

    from rmsf_amd import TICA
    x = torch.tensor(make_lagged_traj(12, 600), device="cuda:0")
    for lag in (600, 601, 5000):
        with pytest.raises(ValueError, match="lag"):
            TICA(x, lag).run()
    with pytest.raises(ValueError, match="lag"):
        TICA(x, 5).run(stop=5)
    with pytest.raises(NotImplementedError, match='layout="fac"'):
        TICA(x.permute(0, 2, 1).contiguous(), 5, layout="soa").run()
    with pytest.raises(NotImplementedError, match="TICA"):
        TICA(x, 5, gpus=[0]).run()
    with pytest.raises(ValueError, match="rank"):
        TICA(x, 5, n_components=31).run()
    with pytest.raises(ValueError, match="components"):
        TICA(x, 5).transform()


def test_matrices_over_half_the_free_hbm_are_refused():
    """200k atoms: two 600,000^2 f64 matrices, 5.8 TB -- a MemoryError stating
    the bytes, before any launch (four 2.4 MB frames are all that is allocated)."""
    import torch

    from rmsf_amd import TICA
    x = torch.zeros((4, 200_000, 3), dtype=torch.float32, device="cuda:0")
    with pytest.raises(MemoryError, match=str(2 * 8 * 600_000 ** 2)):
        TICA(x, 1).run()
    with pytest.raises(MemoryError, match=str(2 * 8 * 600_000 ** 2 + 12 * 200_000 * 3)):
        TICA(x, 1).run(frames=[0, 1, 3])                       # not one run of frames: a resident copy on top


# ---- 7. the command line -----------------------------------------------------
def test_cli_tica(tmp_path):
    import subprocess
    import sys

    from conftest import PKG, ROOT
    out = str(tmp_path / "tica.npz")
    r = subprocess.run([sys.executable, f"{PKG}/rmsf_mi355x.py", "--synthetic", "64", "80", "--align", "average",
                        "--tica", out, "--tica-lag", "3", "--n-components", "4"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    assert sorted(z.files) == ["components", "eigenvalues", "mean", "timescales"]
    assert z["eigenvalues"].shape == (4,) and z["timescales"].shape == (4,)
    assert z["components"].shape == (192, 4) and z["mean"].shape == (64, 3)
    assert np.all(np.diff(z["eigenvalues"]) <= 0) and np.all(np.abs(z["eigenvalues"]) <= 1.0 + 1e-9)
    r = subprocess.run([sys.executable, f"{PKG}/rmsf_mi355x.py", "--synthetic", "64", "80", "--tica", out],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2 and "--tica-lag" in r.stderr
