"""CPU tier of the mean squared displacement (csrc/msd.hip): the ``_host`` entries
-- the definition in plain C++ -- against a numpy restatement of it, the
argument checks (which come before any launch), what ``EinsteinMSD`` refuses
without a device, ``diffusion_coefficient`` and the command line's errors.

The definition (include/rmsf_hip.h): f32 coordinates widened; free ``u(k) =
x(k)``; nojump ``u(0) = x(0)``, ``u(k) = u(k-1) + (d - L * rint(d * (1.0 / L)))``
with ``d = x(k) - x(k-1)`` and the box of frame k; the term ``(dx*dx + dy*dy) +
dz*dz`` of ``dc = u_c(t+tau) - u_c(t)`` with the coordinates the mask leaves out
left out; ``msd(a, tau) = S / (F - tau)``.  numpy evaluates the planes to the same
bits; the sums are held to (N + 8) 2^-53 relative of ``math.fsum`` of the
restated terms divided exactly, N = F - tau: any order of N terms that are not
negative is within (N - 1) 2^-53 of their sum, and the division rounds once.

The GPU tier (tests/test_gpu_msd.py) takes its inputs and references from here."""
import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from test_contacts_host import i32, jittered, ptr
from test_rdf_host import box6, frame_boxes

POISON = -7.0
MASKS = {"x": 1, "y": 2, "xy": 3, "z": 4, "xz": 5, "yz": 6, "xyz": 7}
NEW_SYMBOLS = ("rmsf_msd_plane_ld", "rmsf_msd_plan", "rmsf_msd_workspace_bytes", "rmsf_msd_planes", "rmsf_msd_lags",
               "rmsf_msd_planes_host", "rmsf_msd_lags_host")


# ---- the restatement ---------------------------------------------------------------------
def planes_reference(x, idx, box=None):
    """f64 [n_sel, 3, F] by the definition; ``box`` [3] or [F, 3] or None."""
    x = np.asarray(x)
    rows = np.arange(x.shape[1]) if idx is None else np.asarray(idx)
    xs = x[:, rows].astype(np.float64)                                   # [F, n, 3]
    if box is not None:
        b6 = box6(box, len(x))
        u = np.empty_like(xs)
        u[0] = xs[0]
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(1, len(x)):
                d = xs[k] - xs[k - 1]
                step = d - b6[k, None, :3] * np.rint(d * b6[k, None, 3:])
                u[k] = u[k - 1] + step
        xs = u
    return np.ascontiguousarray(xs.transpose(1, 2, 0))


def terms(u, tau, mask):
    """f64 [n, F - tau]: the terms of every atom at one lag, as the definition writes them."""
    n_frames = u.shape[2]
    with np.errstate(invalid="ignore", over="ignore"):
        d = u[:, :, tau:] - u[:, :, :n_frames - tau]
        t = None
        for c in range(3):
            if (mask >> c) & 1:
                sq = d[:, c] * d[:, c]
                t = sq if t is None else t + sq
    return t


def msd_bound(n_terms):
    return Fraction(n_terms + 8, 2 ** 53)


def assert_msd_within(got, u, n_lags, mask):
    """``got`` [n_lags, n] against math.fsum of the restated terms divided
    exactly; a sum with a non-finite term must be NaN (the terms are never
    +-inf alone: inf - inf)."""
    n, _, n_frames = u.shape
    assert got.shape == (n_lags, n)
    worst = Fraction(0)
    for tau in range(n_lags):
        t = terms(u, tau, mask)
        count = n_frames - tau
        for a in range(n):
            if not np.isfinite(t[a]).all():
                assert np.isnan(got[tau, a]), (tau, a, mask)
                continue
            ref = Fraction(math.fsum(t[a])) / count
            err = abs(Fraction(float(got[tau, a])) - ref)
            assert err <= msd_bound(count) * ref, (tau, a, mask, float(got[tau, a]), float(ref))
            if ref:
                worst = max(worst, err / ref / msd_bound(count))
    return float(worst)


def assert_mean_within(mean, msd):
    """``mean`` [n_lags] against fsum over the per-particle values it was summed from."""
    n_lags, n = msd.shape
    assert mean.shape == (n_lags,)
    for tau in range(n_lags):
        if np.isnan(msd[tau]).any():
            assert np.isnan(mean[tau]), tau
            continue
        ref = Fraction(math.fsum(msd[tau])) / n
        assert abs(Fraction(float(mean[tau])) - ref) <= Fraction(n + 8, 2 ** 53) * ref, tau


def same_bits(a, b):
    """Equal bit for bit where neither is NaN, and NaN in the same places."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64),
                                                                              b[~nb].view(np.uint64))


# ---- the library's host entries ----------------------------------------------------------
def host_planes(x, idx, box=None, pad=5):
    """rmsf_msd_planes_host into a poison-filled buffer; f64 [n_sel, 3, F]."""
    from rmsf_amd import _lib
    x = np.ascontiguousarray(x)
    n_frames, n_atoms = x.shape[:2]
    idx = i32(idx)
    n_sel = n_atoms if idx is None else len(idx)
    ld = n_frames + pad
    b6 = box6(box, n_frames)
    out = np.full((n_sel + 1, 3, ld), POISON)
    _lib.call("rmsf_msd_planes_host", x.ctypes.data, 3 * n_atoms, n_frames, n_atoms, ptr(idx), n_sel, ptr(b6),
              out.ctypes.data, ld)
    assert (out[:n_sel, :, n_frames:] == 0.0).all() and (out[n_sel] == POISON).all()
    return out[:n_sel, :, :n_frames].copy()


def host_lags(u, n_lags, mask, pad=3, mean=True):
    """rmsf_msd_lags_host on planes [n, 3, F]; (msd [n_lags, n], mean [n_lags] or None)."""
    from rmsf_amd import _lib
    u = np.ascontiguousarray(u)
    n, _, n_frames = u.shape
    out = np.full((n_lags + 1, n + pad), POISON)
    m = np.full(n_lags + 1, POISON) if mean else None
    _lib.call("rmsf_msd_lags_host", u.ctypes.data, n_frames, n, n_frames, n_lags, mask, out.ctypes.data, n + pad,
              ptr(m))
    assert (out[:, n:] == POISON).all() and (out[n_lags] == POISON).all() and (m is None or m[n_lags] == POISON)
    return out[:n_lags, :n].copy(), None if m is None else m[:n_lags].copy()


# ---- inputs ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wrapped_walk(n_atoms, n_frames, seed=0, lo=20.0):
    """(x f32 [F, n, 3] wrapped into its boxes, boxes f64 [F, 3], another every
    frame): a random walk with steps of a few A, so atoms cross the faces.
    Read only."""
    rng = np.random.default_rng(100 * seed + n_atoms + 7 * n_frames)
    boxes = frame_boxes(n_frames, lo=lo, seed=seed + 3)
    walk = rng.uniform(0.0, lo, (1, n_atoms, 3)) + np.cumsum(rng.normal(0.0, 2.5, (n_frames, n_atoms, 3)), axis=0)
    x = (walk - boxes[:, None, :] * np.floor(walk / boxes[:, None, :])).astype(np.float32)
    x.setflags(write=False)
    boxes.setflags(write=False)
    return x, boxes


def linear_motion(n_atoms=3, n_frames=200):
    """Atoms at k * 0.25 * (1, 2, -1) past an integer offset of their own: every
    number in the sum is a small multiple of 1/16, so every order is exact."""
    k = np.arange(n_frames, dtype=np.float64)[:, None, None]
    off = np.arange(n_atoms, dtype=np.float64)[None, :, None] * np.array([1.0, -2.0, 3.0])
    return (k * 0.25 * np.array([1.0, 2.0, -1.0]) + off).astype(np.float32)


LINEAR_PER_LAG_SQ = {"x": 0.0625, "y": 0.25, "z": 0.0625, "xy": 0.3125, "yz": 0.3125, "xz": 0.125, "xyz": 0.375}


def plan(n_sel, n_frames, n_lags):
    """(lag_block, origin_chunk, n_splits): host only."""
    from rmsf_amd import _lib
    v = [ctypes.c_int32(0) for _ in range(3)]
    _lib.call("rmsf_msd_plan", n_sel, n_frames, n_lags, *(ctypes.byref(t) for t in v))
    return tuple(t.value for t in v)


# ---- tests -------------------------------------------------------------------------------
def test_abi_and_export():
    from rmsf_amd import EinsteinMSD, _lib        # (the import fails without the feature)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert EinsteinMSD.__name__ == "EinsteinMSD"
    for f in (1, 15, 16, 17, 4096, 20000):
        assert lib.rmsf_msd_plane_ld(f) >= f
    assert lib.rmsf_msd_plane_ld(0) == 0


def test_plan_is_host_only_and_checked():
    from rmsf_amd import _lib
    lib = _lib.load()
    lb, chunk, splits = plan(214, 20000, 2001)
    assert lb >= 1 and chunk >= 1 and splits == 1                      # atoms times lag blocks fill the chip
    assert plan(1, 1, 1)[2] == 1
    assert plan(1, 4096, 4096)[2] > 1                                  # one atom: the origins are split
    assert plan(1, 4096, 4096)[:2] == (lb, chunk)
    v = [ctypes.c_int32(0) for _ in range(3)]
    refs = [ctypes.byref(t) for t in v]
    for bad in ((0, 5, 5), (5, 0, 1), (5, 5, 0), (5, 5, 6), (-1, 5, 5)):
        assert lib.rmsf_msd_plan(*bad, *refs) == _lib.RMSF_EINVAL
        assert b"rmsf_msd_plan" in lib.rmsf_last_error()
    assert lib.rmsf_msd_plan(5, 5, 5, None, refs[1], refs[2]) == _lib.RMSF_EINVAL
    assert lib.rmsf_msd_workspace_bytes(214, 20000, 2001) == 0
    assert lib.rmsf_msd_workspace_bytes(1, 4096, 4096) >= 8 * plan(1, 4096, 4096)[2] * 4096


@pytest.mark.parametrize("periodic", [False, True], ids=["free", "nojump"])
def test_planes_equal_the_restatement_bit_for_bit(periodic):
    x, boxes = wrapped_walk(23, 41)
    box = boxes if periodic else None
    want = planes_reference(x, None, box)
    assert same_bits(host_planes(x, None, box), want)
    rng = np.random.default_rng(3)
    idx = np.concatenate([rng.permutation(23)[:11], [4, 4, 22, 0]])      # out of order; repeated
    got = host_planes(x, idx, box)
    assert same_bits(got, planes_reference(x, idx, box)) and same_bits(got, want[idx])
    if periodic:                                                         # atoms did cross faces, and were put back
        assert (np.abs(want - x.transpose(1, 2, 0)) > 10.0).mean() > 0.1
        assert np.abs(np.diff(want, axis=2)).max() < 0.5 * 24.0
    # one frame: nothing to unwrap
    assert same_bits(host_planes(x[:1], None, None if box is None else box[:1]), x[:1].transpose(1, 2, 0))


@pytest.mark.parametrize("periodic", [False, True], ids=["free", "nojump"])
def test_non_finite_coordinates_poison_their_own_chain(periodic):
    clean, boxes = wrapped_walk(9, 30, seed=1)
    bad = clean.copy()
    bad[11, 4, 1], bad[17, 6, 2] = np.nan, np.inf
    box = boxes if periodic else None
    got, ok = host_planes(bad, None, box), host_planes(clean, None, box)
    assert same_bits(got, planes_reference(bad, None, box))
    touched = np.zeros(got.shape, dtype=bool)
    if periodic:                                                         # NaN from the frame on
        touched[4, 1, 11:], touched[6, 2, 17:] = True, True
        assert np.isnan(got[touched]).all()
    else:                                                                # that frame alone, as stored
        touched[4, 1, 11], touched[6, 2, 17] = True, True
        assert np.isnan(got[4, 1, 11]) and got[6, 2, 17] == np.inf
    assert same_bits(got[~touched], ok[~touched])


@pytest.mark.parametrize("periodic", [False, True], ids=["free", "nojump"])
def test_msd_within_the_bound_for_every_atom_lag_and_mask(periodic):
    x, boxes = wrapped_walk(6, 70, seed=2)
    u = host_planes(x, None, boxes if periodic else None)
    for name, mask in MASKS.items():
        for n_lags in (70, 17):
            got, mean = host_lags(u, n_lags, mask)
            assert_msd_within(got, u, n_lags, mask)
            assert_mean_within(mean, got)
            assert (got[0] == 0.0).all() and mean[0] == 0.0             # lag 0: exactly 0.0
        assert same_bits(host_lags(u, 70, mask, mean=False)[0], host_lags(u, 70, mask)[0])
    # the masks are told apart, and add up as they should to rounding
    full, x_only, yz = (host_lags(u, 70, MASKS[m])[0] for m in ("xyz", "x", "yz"))
    assert np.allclose(full, x_only + yz, rtol=1e-12, atol=0) and (x_only[1:] > 0).all() and (yz[1:] > x_only[1:]).any()


def test_a_nan_reaches_the_lags_that_use_its_frame():
    x = jittered(5, 40)
    bad = x.copy()
    j, k = 2, 13
    bad[k, j, 0] = np.nan
    u, ub = host_planes(x, None), host_planes(bad, None)
    clean, clean_mean = host_lags(u, 40, 7)
    got, mean = host_lags(ub, 40, 7)
    assert_msd_within(got, ub, 40, 7)
    hit = np.arange(40) <= max(k, 39 - k)
    assert np.isnan(got[hit, j]).all() and same_bits(got[~hit, j], clean[~hit, j])
    others = np.arange(5) != j
    assert same_bits(got[:, others], clean[:, others])
    assert np.array_equal(np.isnan(mean), hit) and same_bits(mean[~hit], clean_mean[~hit])


def test_linear_motion_is_exact_for_every_mask():
    x = linear_motion()
    u = host_planes(x, None)
    tau = np.arange(200, dtype=np.float64)
    for name, mask in MASKS.items():
        got, mean = host_lags(u, 200, mask)
        want = tau * tau * LINEAR_PER_LAG_SQ[name]
        assert (got == want[:, None]).all(), name
        assert (mean == want).all(), name
        assert got[0].tolist() == [0.0] * 3
    # the same walk wrapped into a box of edge 8 and put back by nojump: the same numbers
    wrapped = (x.astype(np.float64) - 8.0 * np.floor(x.astype(np.float64) / 8.0)).astype(np.float32)
    assert np.abs(wrapped - x).max() >= 8.0
    uw = host_planes(wrapped, None, (8.0, 8.0, 8.0))
    assert (host_lags(uw, 200, 7)[0] == (tau * tau * 0.375)[:, None]).all()


def test_nojump_follows_a_wrapped_walk():
    """Constant box L, steps under L / 2: the chain stays within F * L * 2^-23 of
    the true walk less the image offset of frame 0 -- a step costs two f32
    roundings at magnitude <= L (2 * L * 2^-24), and the f64 adds nothing
    that shows."""
    L, n_frames, n = 30.0, 400, 12
    rng = np.random.default_rng(8)
    walk = rng.uniform(-50.0, 50.0, (1, n, 3)) + np.cumsum(rng.uniform(-0.4 * L, 0.4 * L, (n_frames, n, 3)), axis=0)
    wrapped64 = walk - L * np.floor(walk / L)
    x = wrapped64.astype(np.float32)
    u = host_planes(x, None, (L, L, L))
    want = (walk - (walk[0] - wrapped64[0])[None]).transpose(1, 2, 0)
    assert np.abs(walk[-1] - walk[0]).max() > 3 * L                      # it did leave the box
    assert np.abs(u - want).max() <= n_frames * L * 2.0 ** -23
    assert np.abs(x.transpose(1, 2, 0) - want).max() > L                 # ... and the stored coordinates do not follow it


def test_argument_checks_come_before_any_launch():
    """No device is touched: the pointers are host arrays, and every call is
    refused on its arguments, by the device entries and by the host entries."""
    from rmsf_amd import _lib
    lib = _lib.load()
    x = np.zeros((4, 6, 3), np.float32)
    planes = np.zeros((6, 3, 16))
    out = np.zeros((4, 8))
    mean = np.zeros(4)
    work = np.zeros(4096)
    good_box = box6((10.0, 12.0, 14.0), 4)

    def run_planes(entry, xyz=x, fstride=18, n_frames=4, n_atoms=6, idx=None, n_sel=6, box=None, d_box="same",
                   dst=planes, ld=16):
        idx = i32(idx)
        if entry == "rmsf_msd_planes":
            return lib.rmsf_msd_planes(ptr(xyz), fstride, n_frames, n_atoms, ptr(idx), ptr(idx), n_sel,
                                       ptr(box) if isinstance(d_box, str) else ptr(d_box), ptr(box), ptr(dst), ld, None)
        return lib.rmsf_msd_planes_host(ptr(xyz), fstride, n_frames, n_atoms, ptr(idx), n_sel, ptr(box), ptr(dst), ld)

    def bad_box(f, k, v, inv=None):
        b = good_box.copy()
        b[f, k] = v
        b[f, 3 + k] = (1.0 / v if v else np.inf) if inv is None else inv
        return b

    bad = [dict(box=bad_box(1, 2, 0.0)), dict(box=bad_box(0, 0, -10.0)), dict(box=bad_box(3, 1, np.inf, 0.0)),
           dict(box=bad_box(0, 1, np.nan)), dict(box=bad_box(1, 0, 10.0, np.nextafter(0.1, 1.0))),
           dict(idx=[0, 6, 2], n_sel=3), dict(idx=[0, -1], n_sel=2), dict(ld=3), dict(n_frames=0), dict(n_sel=0),
           dict(n_atoms=0), dict(fstride=17), dict(xyz=None), dict(dst=None), dict(n_sel=7),
           dict(n_frames=2 ** 31)]
    for entry in ("rmsf_msd_planes", "rmsf_msd_planes_host"):
        for kw in bad:
            assert run_planes(entry, **kw) == _lib.RMSF_EINVAL, (entry, kw)
            assert entry.encode() in lib.rmsf_last_error(), (entry, kw)
    # exactly one of the two copies of the boxes
    assert run_planes("rmsf_msd_planes", box=good_box, d_box=None) == _lib.RMSF_EINVAL
    assert lib.rmsf_msd_planes(ptr(x), 18, 4, 6, None, None, 6, ptr(good_box), None, ptr(planes), 16,
                               None) == _lib.RMSF_EINVAL
    assert run_planes("rmsf_msd_planes_host", box=good_box) == _lib.RMSF_OK
    assert run_planes("rmsf_msd_planes_host", ld=4) == _lib.RMSF_OK

    def run_lags(entry, src=planes, ld=16, n_sel=6, n_frames=4, n_lags=4, mask=7, dst=out, ld_out=8, wk=work,
                 wk_bytes=work.nbytes):
        if entry == "rmsf_msd_lags":
            return lib.rmsf_msd_lags(ptr(src), ld, n_sel, n_frames, n_lags, mask, ptr(dst), ld_out, ptr(mean), ptr(wk),
                                     wk_bytes, None)
        return lib.rmsf_msd_lags_host(ptr(src), ld, n_sel, n_frames, n_lags, mask, ptr(dst), ld_out, ptr(mean))

    bad = [dict(n_lags=0), dict(n_lags=5), dict(n_lags=-1), dict(mask=0), dict(mask=8), dict(mask=-1), dict(ld=3),
           dict(ld_out=5), dict(src=None), dict(dst=None), dict(n_sel=0), dict(n_frames=0), dict(n_frames=2 ** 31)]
    for entry in ("rmsf_msd_lags", "rmsf_msd_lags_host"):
        for kw in bad:
            assert run_lags(entry, **kw) == _lib.RMSF_EINVAL, (entry, kw)
            assert entry.encode() in lib.rmsf_last_error(), (entry, kw)
    # a split plan without its workspace
    big = dict(n_sel=1, n_frames=4096, n_lags=4096, ld=4096, ld_out=8)
    assert plan(1, 4096, 4096)[2] > 1
    assert run_lags("rmsf_msd_lags", wk=None, wk_bytes=0, **big) == _lib.RMSF_EINVAL
    assert run_lags("rmsf_msd_lags", wk_bytes=8, **big) == _lib.RMSF_EINVAL
    assert b"workspace" in lib.rmsf_last_error()
    assert run_lags("rmsf_msd_lags_host") == _lib.RMSF_OK


def test_einstein_msd_refusals_need_no_device(monkeypatch):
    import torch

    from rmsf_amd import EinsteinMSD, parallel
    from rmsf_amd.sources import DeviceSource
    x = np.zeros((5, 10, 3), np.float32)
    # what ContactMap refuses, under this class's own name: gpus=, shards, HBM-resident planes, more than one rank
    with pytest.raises(NotImplementedError, match="EinsteinMSD runs on one device"):
        EinsteinMSD(x, gpus=2).run()
    with pytest.raises(NotImplementedError, match="EinsteinMSD runs on one device"):
        EinsteinMSD([x, x]).run()
    planes = object.__new__(DeviceSource)                              # HBM-resident [F, 3, n_atoms]; no tensor needed
    planes.layout, planes.n_sel = "soa", 10
    with pytest.raises(NotImplementedError, match="EinsteinMSD reads"):
        EinsteinMSD(planes).run()
    with pytest.raises(NotImplementedError, match="EinsteinMSD reads"):
        EinsteinMSD(planes, unwrap="nojump", box=(40.0, 40.0, 40.0)).run()
    with monkeypatch.context() as m:
        m.setattr(parallel, "world", lambda: (0, 2))
        with pytest.raises(NotImplementedError, match="EinsteinMSD runs on one device.*more than one rank"):
            EinsteinMSD(x).run()
        with pytest.raises(NotImplementedError, match="more than one rank"):
            EinsteinMSD(x, max_lag=9).run()                              # ... before the run's length is looked at
    EinsteinMSD(x)
    EinsteinMSD(x, unwrap="nojump", box=(40.0, 40.0, 40.0, 90.0, 90.0, 90.0), max_lag=0, msd_type="xz")
    for kw in (dict(msd_type="zx"), dict(msd_type="xyzz"), dict(msd_type=None), dict(max_lag=-1), dict(max_lag=1.5),
               dict(unwrap="wrap"), dict(unwrap=True), dict(dt=np.inf), dict(layout="aos")):
        with pytest.raises(ValueError):
            EinsteinMSD(x, **kw)
    with pytest.raises(ValueError, match="unwrap"):
        EinsteinMSD(x, box=(40.0, 40.0, 40.0))                           # a box without unwrap
    with pytest.raises(ValueError, match="needs a box"):
        EinsteinMSD(x, unwrap="nojump")                                  # unwrap without a box
    with pytest.raises(NotImplementedError, match="orthorhombic"):
        EinsteinMSD(x, unwrap="nojump", box=(40.0, 40.0, 40.0, 90.0, 90.0, 60.0))
    with pytest.raises(ValueError, match="file"):
        EinsteinMSD(x, unwrap="nojump", box="file")
    with pytest.raises(ValueError, match="file"):
        EinsteinMSD("traj.dcd", unwrap="nojump", box="file")
    with pytest.raises(ValueError):
        EinsteinMSD(x, unwrap="nojump", box="xtc")
    for bad in ((40.0, 0.0, 40.0), (40.0, -1.0, 40.0), (40.0, np.nan, 40.0), (40.0, 40.0), np.zeros((3, 4))):
        with pytest.raises(ValueError):
            EinsteinMSD(x, unwrap="nojump", box=bad)
    with pytest.raises(ValueError):
        EinsteinMSD(x, select=[])
    with pytest.raises(NotImplementedError):
        EinsteinMSD(x, gpus=2).run()
    with pytest.raises(NotImplementedError):
        EinsteinMSD([x, x]).run()
    with pytest.raises(TypeError):
        EinsteinMSD(x, fft=True)                                         # there is no FFT route
    # the run's own length: known for an array before any device is asked for
    with pytest.raises(ValueError, match="no frames"):
        EinsteinMSD(x).run(frames=[])
    with pytest.raises(ValueError, match="no frames"):
        EinsteinMSD(torch.zeros(5, 10, 3)).run(start=5)
    with pytest.raises(ValueError, match="max_lag"):
        EinsteinMSD(x, max_lag=5).run()
    with pytest.raises(ValueError, match="max_lag"):
        EinsteinMSD(x, max_lag=3).run(step=2)                            # three frames: lags 0..2


def test_diffusion_coefficient_is_the_closed_form_slope():
    from rmsf_amd import EinsteinMSD
    for msd_type, dt in (("xyz", 1.0), ("xy", 0.002), ("z", 10.0)):
        m = EinsteinMSD(np.zeros((2, 1, 3), np.float32), msd_type=msd_type, dt=dt)
        with pytest.raises(RuntimeError):
            m.diffusion_coefficient()
        t = np.arange(500) * dt
        m.n_frames = 500
        m.results.delta_t_values = t
        m.results.timeseries = 2.0 * m.dim_fac * 0.25 * t
        assert m.dim_fac == len(msd_type)
        for window in ((None, None), (50, 400), (498, 500)):
            got = m.diffusion_coefficient(*window)
            assert abs(got - 0.25) <= 1e-12 * 0.25 and m.results.D == got
        # an offset does not move the slope; a window of one lag has none
        m.results.timeseries = m.results.timeseries + 3.0
        assert abs(m.diffusion_coefficient(10, 300) - 0.25) <= 1e-12 * 0.25
        for window in ((5, 6), (7, 7), (-1, 10), (0, 501), (400, 300)):
            with pytest.raises(ValueError):
                m.diffusion_coefficient(*window)


def test_cli_refuses_msd_under_a_distributed_launch(capsys, monkeypatch):
    import rmsf_mi355x
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as exc:
        rmsf_mi355x.main(["--synthetic", "50", "8", "--msd", "o.npz"])
    assert exc.value.code == 2
    assert "--msd runs in one process" in capsys.readouterr().err


def test_cli_refuses_bad_msd_options(capsys):
    import rmsf_mi355x
    for argv in (["--synthetic", "50", "8", "--msd-type", "xy"],
                 ["--synthetic", "50", "8", "--msd-max-lag", "3"],
                 ["--synthetic", "50", "8", "--msd-dt", "2.0"],
                 ["--synthetic", "50", "8", "--msd-box", "20", "20", "20"],
                 ["--synthetic", "50", "8", "--msd", "o.npz", "--msd-type", "zz"],
                 ["--synthetic", "50", "8", "--msd", "o.npz", "--msd-max-lag", "-1"],
                 ["--synthetic", "50", "8", "--msd", "o.npz", "--msd-max-lag", "8"],
                 ["--synthetic", "50", "8", "--msd", "o.npz", "--msd-dt", "inf"],
                 ["--synthetic", "50", "8", "--msd", "o.npz", "--msd-box", "file"],
                 ["--synthetic", "50", "8", "--msd", "o.npz", "--msd-box", "20", "20"],
                 ["--synthetic", "50", "8", "--msd", "o.npz", "--msd-box", "20", "0", "20"],
                 ["--synthetic", "50", "8", "--msd", "o.npz", "--msd-box", "20", "x", "20"]):
        with pytest.raises(SystemExit) as exc:
            rmsf_mi355x.main(argv)
        assert exc.value.code == 2, argv
        assert "--msd" in capsys.readouterr().err
