"""GPU tier of the mean squared displacement (csrc/msd.hip): ``rmsf_msd_planes``
and ``rmsf_msd_lags`` through ``Engine``, and ``EinsteinMSD`` end to end, against
the numpy restatement of the definition in tests/test_msd_host.py.

The planes are compared bit for bit; ``msd`` is held to (N + 8) 2^-53 relative of
``math.fsum`` of the restated terms divided exactly (N = F - tau) and the particle
mean to (n + 8) 2^-53 of ``fsum`` over the device's own per-particle values.
Every device call runs twice into poison-filled buffers wider than the result:
the same bytes both times, the poison intact.

The shapes stand on the launcher's own plan (``rmsf_msd_plan``): the lag block
LB, the origin chunk C and the smallest frame count it splits, not on a
workload."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from test_contacts_host import jittered
from test_msd_host import (LINEAR_PER_LAG_SQ, MASKS, POISON, assert_mean_within, assert_msd_within, host_lags,
                           host_planes, linear_motion, msd_bound, plan, planes_reference, same_bits, terms,
                           wrapped_walk)

pytestmark = pytest.mark.gpu

N_MAX = 65                             # the most atoms a case follows
N_TRAJ_ATOMS = 70                      # ... out of a frame's
ATOMS = (1, 3, N_MAX)


@functools.lru_cache(maxsize=None)
def engine():
    import torch

    from rmsf_amd.engine import Engine
    return Engine(torch.device("cuda", 0))


def edges():
    lb, c, _ = plan(3, 100, 100)
    return lb, c


def frame_counts():
    lb, c = edges()
    return sorted({1, 2, lb - 1, lb, lb + 1, lb + c + 1, 2 * max(lb, c) + 3} - {0})


def lag_counts(n_frames):
    lb, _ = edges()
    return sorted(k for k in {1, 2, lb, lb + 1, n_frames} if k <= n_frames)


@functools.lru_cache(maxsize=None)
def first_split_frames():
    """The smallest F <= 4096 whose plan at one atom and all lags splits the origins."""
    for f in range(1, 4097):
        if plan(1, f, f)[2] > 1:
            return f
    return None


@functools.lru_cache(maxsize=None)
def rows():
    """The atoms followed, out of order, out of a frame's N_TRAJ_ATOMS."""
    r = np.random.default_rng(21).permutation(N_TRAJ_ATOMS)[:N_MAX]
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def on_device(n_frames, seed=0):
    import torch
    x, boxes = wrapped_walk(N_TRAJ_ATOMS, n_frames, seed=seed)
    return x, boxes, torch.tensor(x, device="cuda:0")


@functools.lru_cache(maxsize=None)
def exact_msd(n_frames, periodic, mask, seed=0):
    """(planes f64 [N_MAX, 3, F] by the restatement, fsum of the restated terms
    f64 [F, N_MAX]): computed once a case, shared, read only."""
    x, boxes = wrapped_walk(N_TRAJ_ATOMS, n_frames, seed=seed)
    u = planes_reference(x, rows(), boxes if periodic else None)
    s = np.empty((n_frames, N_MAX))
    for tau in range(n_frames):
        t = terms(u, tau, mask)
        s[tau] = [math.fsum(row) for row in t]
    u.setflags(write=False)
    s.setflags(write=False)
    return u, s


def assert_within(got, sums, n_frames):
    """``got`` [n_lags, n] against the shared fsum values of its atoms, divided exactly."""
    n_lags, n = got.shape
    for tau in range(n_lags):
        count = n_frames - tau
        for a in range(n):
            ref = Fraction(float(sums[tau, a])) / count
            assert abs(Fraction(float(got[tau, a])) - ref) <= msd_bound(count) * ref, (tau, a, n_frames)


def device_planes(x_dev, idx, box, n_atoms=None, fstride=None):
    """Engine.msd_planes twice into a poison-filled buffer with a row to spare
    and ld from rmsf_msd_plane_ld: the same bytes, zeros from F to ld, the
    poison row intact.  (the tensor [n_sel + 1, 3, ld] in HBM, n_sel, F)"""
    import torch
    n_frames = x_dev.shape[0]
    n_atoms = x_dev.shape[1] if n_atoms is None else n_atoms
    n_sel = n_atoms if idx is None else len(idx)
    ld = engine().msd_plane_ld(n_frames)
    assert ld >= n_frames
    if box is not None:
        box = np.broadcast_to(np.asarray(box, dtype=np.float64), (n_frames, 3))
    runs, keep = [], None
    for _ in range(2):
        out = torch.full((n_sel + 1, 3, ld), POISON, dtype=torch.float64, device="cuda:0")
        got = engine().msd_planes(x_dev.data_ptr(), x_dev.stride(0) if fstride is None else fstride, n_frames, n_atoms,
                                  idx, n_sel, box=box, out=out)
        torch.cuda.synchronize()
        assert got.shape == (n_sel, 3, n_frames) and got.data_ptr() == out.data_ptr()
        runs.append(out.cpu().numpy())
        keep = out
    assert runs[0].tobytes() == runs[1].tobytes()
    assert (runs[0][n_sel] == POISON).all() and (runs[0][:n_sel, :, n_frames:] == 0.0).all()
    return keep, runs[0][:n_sel, :, :n_frames].copy()


def device_lags(planes_buf, n_sel, n_frames, n_lags, mask, pad=3, mean=True):
    """Engine.msd_lags twice into poison-filled buffers with ld_out > n and a
    lag to spare: the same bytes, the poison intact.  (msd [n_lags, n], mean)"""
    import torch
    planes = planes_buf[:n_sel, :, :n_frames]
    runs = []
    for _ in range(2):
        out = torch.full((n_lags + 1, n_sel + pad), POISON, dtype=torch.float64, device="cuda:0")
        m = torch.full((n_lags + 2,), POISON, dtype=torch.float64, device="cuda:0") if mean else False
        got, got_mean = engine().msd_lags(planes, n_frames, n_lags, mask, out=out, mean=m)
        torch.cuda.synchronize()
        assert got.shape == (n_lags, n_sel) and got.data_ptr() == out.data_ptr()
        assert (got_mean is None) == (not mean)
        runs.append((out.cpu().numpy(), m.cpu().numpy() if mean else None))
    (a, ma), (b, mb) = runs
    assert a.tobytes() == b.tobytes() and (not mean or ma.tobytes() == mb.tobytes())
    assert (a[:, n_sel:] == POISON).all() and (a[n_lags] == POISON).all()
    assert not mean or (ma[n_lags:] == POISON).all()
    return a[:n_lags, :n_sel].copy(), ma[:n_lags].copy() if mean else None


def test_the_plan_is_not_trivial():
    lb, c = edges()
    frames = frame_counts()
    assert lb > 1 and c > 1 and len(frames) == 7
    assert frames[-1] > 2 * c and frames[-1] > 2 * lb                   # three chunks of origins, a ragged last one
    assert max(lag_counts(frames[-1])) > 2 * lb and frames[-1] % lb     # lag blocks, and a partial last one
    assert plan(1, 1, 1)[2] == 1
    f = first_split_frames()
    assert f is not None and plan(1, f, f)[2] > 1 and plan(1, f - 1, f - 1)[2] == 1
    assert plan(1, 4 * c + 5, 4 * c + 5)[2] > 2
    assert plan(4096, 4096, 4096)[:2] == (lb, c) and plan(4096, 4096, 4096)[2] == 1   # the edges do not move
    assert engine().msd_plan(214, 20000, 2001) == plan(214, 20000, 2001)


@pytest.mark.parametrize("periodic", [False, True], ids=["free", "nojump"])
@pytest.mark.parametrize("n_frames", frame_counts())
def test_planes_and_lags_at_the_plan_edges(n_frames, periodic):
    x, boxes, x_dev = on_device(n_frames)
    box = boxes if periodic else None
    u_ref, sums = exact_msd(n_frames, periodic, 7)
    for n in ATOMS:
        idx = rows()[:n]
        buf, u = device_planes(x_dev, idx, box)
        assert same_bits(u, u_ref[:n])                                  # the restatement, bit for bit
        if n == 3:
            assert same_bits(u, host_planes(x, idx, box))
        for n_lags in lag_counts(n_frames):
            got, mean = device_lags(buf, n, n_frames, n_lags, 7)
            assert_within(got, sums, n_frames)
            assert_mean_within(mean, got)
            assert (got[0] == 0.0).all() and mean[0] == 0.0
    # dense rows: no index array at all
    buf, u = device_planes(x_dev, None, box)
    assert same_bits(u[rows()], u_ref)
    got, _ = device_lags(buf, N_TRAJ_ATOMS, n_frames, min(n_frames, 2), 7, mean=False)
    assert_within(got[:, rows()], sums, n_frames)


@pytest.mark.parametrize("periodic", [False, True], ids=["free", "nojump"])
def test_every_mask(periodic):
    lb, c = edges()
    n_frames = lb + c + 1
    x, boxes, x_dev = on_device(n_frames)
    idx = rows()[:3]
    buf, u = device_planes(x_dev, idx, boxes if periodic else None)
    for name, mask in MASKS.items():
        got, mean = device_lags(buf, 3, n_frames, n_frames, mask)
        assert_msd_within(got, u, n_frames, mask)
        assert_mean_within(mean, got)
        want, _ = host_lags(u, n_frames, mask)                          # another order of the same terms
        assert np.allclose(got, want, rtol=1e-12, atol=0), name


@pytest.mark.parametrize("periodic", [False, True], ids=["free", "nojump"])
def test_origins_split_over_workgroups_and_folded(periodic):
    _, c = edges()
    f = first_split_frames()
    assert f is not None                                                # a split plan exists at F <= 4096
    for n_frames, n in ((f, 1), (4 * c + 5, 1), (4 * c + 5, 3)):
        assert plan(n, n_frames, n_frames)[2] > 1
        x, boxes, x_dev = on_device(n_frames, seed=1)
        u_ref, sums = exact_msd(n_frames, periodic, 7, seed=1)
        buf, u = device_planes(x_dev, rows()[:n], boxes if periodic else None)
        assert same_bits(u, u_ref[:n])
        got, mean = device_lags(buf, n, n_frames, n_frames, 7)
        assert_within(got, sums, n_frames)
        assert_mean_within(mean, got)
    # fewer lags and another mask on the same planes
    n_frames = 4 * c + 5
    got, _ = device_lags(buf, 3, n_frames, 70, 5)
    assert_msd_within(got, u, 70, 5)


def test_gathered_in_place_from_a_wider_tensor():
    """Frames a stride past 3 n_atoms apart, NaN between them, rows picked by a
    repeated index."""
    import torch
    lb, _ = edges()
    n_frames = lb + 1
    x, boxes, _ = on_device(n_frames)
    wide = torch.full((n_frames, N_TRAJ_ATOMS * 3 + 7), float("nan"), dtype=torch.float32, device="cuda:0")
    wide[:, :N_TRAJ_ATOMS * 3] = torch.tensor(x.reshape(n_frames, -1), device="cuda:0")
    idx = np.concatenate([rows()[:20], [5, 5, 69, 0]])
    for box in (None, boxes):
        buf, u = device_planes(wide, idx, box, n_atoms=N_TRAJ_ATOMS, fstride=wide.stride(0))
        assert same_bits(u, planes_reference(x, idx, box)) and np.isfinite(u).all()
        got, mean = device_lags(buf, len(idx), n_frames, n_frames, 7)
        assert_msd_within(got, u, n_frames, 7)
        assert same_bits(got[:, 20], got[:, 21])                        # the same atom twice: the same column


def test_linear_motion_is_exact_on_the_device():
    import torch
    _, c = edges()
    x = linear_motion()
    buf, u = device_planes(torch.tensor(x, device="cuda:0"), None, None)
    tau = np.arange(200, dtype=np.float64)
    for name, mask in MASKS.items():
        got, mean = device_lags(buf, 3, 200, 200, mask)
        want = tau * tau * LINEAR_PER_LAG_SQ[name]
        assert (got == want[:, None]).all() and (mean == want).all(), name
    # split origins, wrapped into a box of edge 8 and put back
    n_frames = 2 * c + 88
    assert plan(1, n_frames, n_frames)[2] > 1
    x = linear_motion(1, n_frames).astype(np.float64)
    wrapped = (x - 8.0 * np.floor(x / 8.0)).astype(np.float32)
    buf, u = device_planes(torch.tensor(wrapped, device="cuda:0"), None, (8.0, 8.0, 8.0))
    got, mean = device_lags(buf, 1, n_frames, n_frames, 7)
    tau = np.arange(n_frames, dtype=np.float64)
    assert (got[:, 0] == tau * tau * 0.375).all() and (mean == tau * tau * 0.375).all()


def test_a_nan_reaches_the_lags_that_use_its_frame():
    import torch
    lb, c = edges()
    n_frames, n, j, k = lb + c + 1, 5, 2, 100
    x = jittered(n, n_frames)
    bad = x.copy()
    bad[k, j, 1] = np.nan
    buf, _ = device_planes(torch.tensor(x, device="cuda:0"), None, None)
    clean, clean_mean = device_lags(buf, n, n_frames, n_frames, 7)
    buf, ub = device_planes(torch.tensor(bad, device="cuda:0"), None, None)
    got, mean = device_lags(buf, n, n_frames, n_frames, 7)
    hit = np.arange(n_frames) <= max(k, n_frames - 1 - k)
    assert hit.sum() < n_frames and np.isnan(got[hit, j]).all()          # NaN exactly for tau <= max(k, F - 1 - k)
    assert not np.isnan(got[~hit, j]).any() and same_bits(got[~hit, j], clean[~hit, j])
    others = np.arange(n) != j
    assert same_bits(got[:, others], clean[:, others]) and not np.isnan(clean).any()
    assert np.array_equal(np.isnan(mean), hit) and same_bits(mean[~hit], clean_mean[~hit])
    # under nojump the chain is NaN from k on: every lag of that atom, and no other
    boxes = np.broadcast_to(np.array([30.0, 31.0, 32.0]), (n_frames, 3))
    buf, ub = device_planes(torch.tensor(bad, device="cuda:0"), None, boxes)
    assert same_bits(ub, planes_reference(bad, None, boxes)) and np.isnan(ub[j, 1, k:]).all()
    assert np.isnan(ub).sum() == n_frames - k
    got, _ = device_lags(buf, n, n_frames, n_frames, 7)
    assert np.isnan(got[:, j]).all() and not np.isnan(got[:, others]).any()
    got_xz, _ = device_lags(buf, n, n_frames, n_frames, MASKS["xz"])      # y is not in the expression
    assert not np.isnan(got_xz).any()


def engine_msd(x, idx, box, n_lags, mask):
    import torch
    buf, u = device_planes(torch.tensor(np.ascontiguousarray(x), device="cuda:0"), idx, box)
    return device_lags(buf, len(idx), len(x), n_lags, mask) + (u,)


def test_einstein_msd_from_hbm_and_from_the_host():
    from rmsf_amd import EinsteinMSD
    n_traj = 90
    x, boxes, x_dev = on_device(n_traj)
    sel = rows()[:20]
    # a wider HBM tensor, a selection, step=2: read in place
    a = EinsteinMSD(x_dev, select=sel, dt=0.5)
    r = a.run(step=2).results
    msd, mean, u = engine_msd(x[::2], sel, None, 45, 7)
    assert r.n_frames == 45 and r.n_particles == 20 and r.dim_fac == 3 and np.array_equal(r.frames, np.arange(0, 90, 2))
    assert r.timeseries.tobytes() == mean.tobytes() and r.msds_by_particle.tobytes() == msd.tobytes()
    assert r.msds_by_particle.shape == (45, 20) and np.array_equal(r.delta_t_values, np.arange(45) * 0.5)
    assert_msd_within(r.msds_by_particle, u, 45, 7)
    # a host array, nojump with a box a trajectory frame, a mask, max_lag, an explicit frame list
    frames = np.arange(3, 80, 3)
    h = EinsteinMSD(np.asarray(x), select=sel, msd_type="xz", max_lag=11, unwrap="nojump", box=boxes)
    r = h.run(frames=frames).results
    msd, mean, u = engine_msd(x[frames], sel, boxes[frames], 12, MASKS["xz"])
    assert r.timeseries.tobytes() == mean.tobytes() and r.msds_by_particle.tobytes() == msd.tobytes()
    assert r.dim_fac == 2 and r.timeseries.shape == (12,) and np.array_equal(r.frames, frames)
    assert_msd_within(r.msds_by_particle, planes_reference(x[frames], sel, boxes[frames]), 12, MASKS["xz"])
    d = h.diffusion_coefficient(1, 12)                                  # the walk does diffuse once it is unwrapped
    assert d > 0 and h.results.D == d
    # by_particle=False: the same timeseries, no matrix
    q = EinsteinMSD(np.asarray(x), select=sel, msd_type="xz", max_lag=11, unwrap="nojump", box=boxes,
                    by_particle=False).run(frames=frames).results
    assert q.msds_by_particle is None and q.timeseries.tobytes() == mean.tobytes()
    # every atom, one [6] box
    e = EinsteinMSD(x_dev, unwrap="nojump", box=(24.0, 23.0, 22.0, 90.0, 90.0, 90.0), max_lag=0).run().results
    assert e.msds_by_particle.shape == (1, N_TRAJ_ATOMS) and not e.msds_by_particle.any() and e.timeseries[0] == 0.0
    with pytest.raises(ValueError, match="rows"):
        EinsteinMSD(x_dev, unwrap="nojump", box=boxes[:7]).run()
    with pytest.raises(ValueError, match="max_lag"):
        EinsteinMSD(x_dev, max_lag=90).run()
    with pytest.raises(ValueError, match="no frames"):
        EinsteinMSD(x_dev).run(frames=[])


def test_einstein_msd_from_an_xtc_with_its_own_boxes(tmp_path):
    from rmsf_amd import EinsteinMSD
    from rmsf_amd.xtc import XTCFile, write_xtc
    x, boxes, _ = on_device(40)
    path = str(tmp_path / "msd.xtc")
    segments = (slice(0, 13), slice(13, 14), slice(14, 40))
    for k, fr in enumerate(segments):                                  # a box a segment: the writer takes one a call
        seg_box = boxes[fr.start]
        wrapped = (x[fr].astype(np.float64) % seg_box).astype(np.float32)
        write_xtc(path, wrapped, box=np.diag(seg_box), append=k > 0)
    with XTCFile(path) as fh:
        stored, file_boxes = fh.read(), fh.boxes()                     # the coordinates as the file rounds them
    assert stored.shape == x.shape and file_boxes.shape == (40, 3)
    sel = rows()[:30]
    r = EinsteinMSD(path, select=sel, unwrap="nojump", box="file", dt=2.0).run(start=1).results
    msd, mean, u = engine_msd(stored[1:], sel, file_boxes[1:], 39, 7)
    assert r.n_frames == 39 and r.timeseries.tobytes() == mean.tobytes()
    assert r.msds_by_particle.tobytes() == msd.tobytes() and np.array_equal(r.delta_t_values, np.arange(39) * 2.0)
    assert same_bits(u, planes_reference(stored[1:], sel, file_boxes[1:]))
    assert_msd_within(r.msds_by_particle, u, 39, 7)
    assert r.timeseries[-1] > 0
    with pytest.raises(ValueError, match="max_lag"):
        EinsteinMSD(path, max_lag=40).run()
