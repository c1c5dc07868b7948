"""CPU tier of the contact kernels (csrc/contacts.hip): the library's entry
points, their argument checks (which come before any launch),
``contact_threshold_sq``, ``rmsf_contact_counts_host`` and
``rmsf_contact_fraction_host`` -- the definition in plain C++ -- against a numpy
restatement of it, what ``ContactMap`` and ``Contacts`` refuse without a
device, and the script's option errors.

The definition (include/rmsf_hip.h): f32 coordinates, ``dx = (double)xa -
(double)xb`` and so for y and z, ``d2 = (dx*dx + dy*dy) + dz*dz`` with no FMA,
``d = sqrt(d2)``, in contact iff ``d <= radius``, a NaN never.  numpy evaluates
that expression to the same bits, so counts, ``n_contacts`` and the hard-cut q
are compared for equality.  soft_cut is compared with the restatement summed by
``math.fsum`` within ``(P + 8) 2^-53`` relative: the argument of the
exponential has numpy's bits, the exponential is within the 4 ulp the project
bounds it by, two correctly rounded operations make a term, P - 1 additions of
non-negative terms the sum, and one division q.

The GPU tier (tests/test_gpu_contacts.py) takes its inputs and references
from here."""
import ctypes
import functools
import math

import numpy as np
import pytest

SOFT = dict(beta=5.0, lambda_constant=1.8)
METHOD = {"hard_cut": 0, "radius_cut": 1, "soft_cut": 2}


# ---- inputs ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def jittered(n_atoms, n_frames, seed=0):
    """Base positions uniform in a 20 A box, 1 A noise a frame: at radius 6 a
    fifth of the pairs touch in some frames and not in others.  Read only."""
    rng = np.random.default_rng(1000 * seed + 7 * n_atoms + n_frames)
    x = (rng.uniform(0.0, 20.0, (n_atoms, 3))[None] + rng.normal(0.0, 1.0, (n_frames, n_atoms, 3))).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def lattice(n_frames=3, side=5):
    """The side^3 integer lattice, its atoms in another order every frame: at
    radius 3.0 many distances equal the radius exactly.  Read only."""
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(5)
    x = np.stack([g] + [g[rng.permutation(len(g))] for _ in range(n_frames - 1)])
    x.setflags(write=False)
    return x


NAN_AT, INF_AT = (3, 5, 1), (7, 11, 0)        # (frame, atom, coordinate)


@functools.lru_cache(maxsize=None)
def poisoned(n_atoms=130, n_frames=12):
    """(clean, the same with one NaN and one Inf coordinate).  Read only."""
    clean = jittered(n_atoms, n_frames, seed=3)
    bad = clean.copy()
    bad[NAN_AT], bad[INF_AT] = np.nan, np.inf
    bad.setflags(write=False)
    return clean, bad


# ---- the restatement ---------------------------------------------------------------------
def distances(x, ia, ib):
    """f64 [F, n_a, n_b] by the definition."""
    a = x[:, ia].astype(np.float64)[:, :, None, :]
    b = x[:, ib].astype(np.float64)[:, None, :, :]
    with np.errstate(invalid="ignore", over="ignore"):
        d = a - b
        return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def counts_reference(x, ia, ib, radius):
    with np.errstate(invalid="ignore"):
        return (distances(x, ia, ib) <= radius).sum(axis=0).astype(np.int64)


def pair_distance(x, ra, rb):
    """f64 [F, P] of the pairs of rows (ra[p], rb[p])."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[:, ra].astype(np.float64) - x[:, rb].astype(np.float64)
        return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def fraction_reference(x, ra, rb, r0, radius, method, beta=5.0, lambda_constant=1.8):
    """(q f64 [F], n_contacts int64 [F]); soft_cut's sum by math.fsum."""
    d = pair_distance(x, ra, rb)
    with np.errstate(invalid="ignore"):
        n = (d <= radius).sum(axis=1).astype(np.int64)
    if method != "soft_cut":
        return n / float(len(ra)), n
    with np.errstate(over="ignore"):
        terms = 1.0 / (1.0 + np.exp(beta * (d - lambda_constant * np.asarray(r0)[None])))
    return np.array([math.fsum(t) / len(ra) for t in terms]), n


def soft_bound(n_pairs):
    return (n_pairs + 8) * 2.0 ** -53


def natives(x0, ia, ib, radius):
    """(rows a, rows b, r0) of the pairs in contact in the frame x0, row-major."""
    d = distances(x0[None], ia, ib)[0]
    with np.errstate(invalid="ignore"):
        i, j = np.nonzero(d <= radius)
    return np.asarray(ia)[i], np.asarray(ib)[j], d[i, j]


# ---- the library's host entries ----------------------------------------------------------
def i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def ptr(a):
    return None if a is None else a.ctypes.data


def host_counts(x, ia, ib, radius, pad=3):
    from rmsf_amd import _lib
    x = np.ascontiguousarray(x)
    n_frames, n_atoms = x.shape[:2]
    ia, ib = i32(ia), i32(ib)
    n_a, n_b = (n_atoms if ia is None else len(ia)), (n_atoms if ib is None else len(ib))
    out = np.full((n_a, n_b + pad), -7, dtype=np.int32)
    _lib.call("rmsf_contact_counts_host", x.ctypes.data, 3 * n_atoms, n_frames, n_atoms, ptr(ia), n_a, ptr(ib), n_b,
              float(radius), out.ctypes.data, n_b + pad)
    assert (out[:, n_b:] == -7).all()                                  # nothing written past n_b
    return out[:, :n_b].astype(np.int64)


def host_fraction(x, ra, rb, r0, radius, method, beta=5.0, lambda_constant=1.8, rows=None):
    from rmsf_amd import _lib
    x = np.ascontiguousarray(x)
    n_frames, n_atoms = x.shape[:2]
    ra, rb, rows = i32(ra), i32(rb), i32(rows)
    r0 = None if r0 is None else np.ascontiguousarray(r0, dtype=np.float64)
    q, n = np.full(n_frames, -1.0), np.full(n_frames, -1, dtype=np.int32)
    _lib.call("rmsf_contact_fraction_host", x.ctypes.data, 3 * n_atoms, n_frames, n_atoms,
              n_atoms if rows is None else len(rows), ptr(rows), ra.ctypes.data, rb.ctypes.data, ptr(r0), len(ra),
              float(radius), METHOD[method], float(beta), float(lambda_constant), q.ctypes.data, n.ctypes.data)
    return q, n.astype(np.int64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- tests -------------------------------------------------------------------------------
NEW_SYMBOLS = ("rmsf_contact_threshold_sq", "rmsf_contact_counts_plan", "rmsf_contact_counts_workspace_bytes",
               "rmsf_contact_counts", "rmsf_contact_counts_host", "rmsf_contact_fraction",
               "rmsf_contact_fraction_host")


def test_abi():
    from rmsf_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.rmsf_abi_version() == 4 == _lib.ABI_VERSION


def test_plan_is_host_only_and_checked():
    from rmsf_amd import _lib
    lib = _lib.load()
    v = [ctypes.c_int32(-1) for _ in range(4)]
    refs = [ctypes.byref(t) for t in v]
    assert lib.rmsf_contact_counts_plan(214, 214, 20000, 1, *refs) == _lib.RMSF_OK
    tile_a, tile_b, chunk, splits = (t.value for t in v)
    assert tile_a >= 1 and tile_b >= 1 and chunk >= 1
    assert splits > 1                                                  # few tiles: the frames are split
    assert lib.rmsf_contact_counts_plan(3341, 3341, 4096, 1, *refs) == _lib.RMSF_OK and v[3].value >= 1
    assert lib.rmsf_contact_counts_plan(1, 1, 1, 0, *refs) == _lib.RMSF_OK and v[3].value == 1
    for bad in ((0, 5, 5, 0), (5, 0, 5, 0), (5, 5, 0, 0), (5, 6, 5, 1)):
        assert lib.rmsf_contact_counts_plan(*bad, *refs) == _lib.RMSF_EINVAL
        assert b"rmsf_contact_counts_plan" in lib.rmsf_last_error()
    assert lib.rmsf_contact_counts_workspace_bytes(214, 214, 20000, 1) % 8 == 0


def test_argument_checks_come_before_any_launch():
    """No device is touched: the pointers are host arrays, and every call is
    refused on its arguments."""
    from rmsf_amd import _lib
    lib = _lib.load()
    x = np.zeros((2, 5, 3), np.float32)
    out = np.zeros((5, 5), np.int32)
    idx, far = i32([0, 1, 2]), i32([0, 5, 2])
    q, n = np.zeros(2), np.zeros(2, np.int32)
    r0 = np.ones(3)

    def counts(radius=4.5, h_a=None, n_a=5, entry="rmsf_contact_counts"):
        args = [x.ctypes.data, 15, 2, 5, ptr(idx) if h_a is not None else None]
        if entry == "rmsf_contact_counts":
            return lib.rmsf_contact_counts(*args, ptr(h_a), n_a, None, None, 5, 0, radius, out.ctypes.data, 5, None, 0,
                                           None)
        return lib.rmsf_contact_counts_host(x.ctypes.data, 15, 2, 5, ptr(h_a), n_a, None, 5, radius, out.ctypes.data, 5)

    def fraction(p=3, pa=idx, radius=4.5, method=0, entry="rmsf_contact_fraction", rows=None):
        if entry == "rmsf_contact_fraction":
            return lib.rmsf_contact_fraction(x.ctypes.data, 15, 2, 5, 5 if rows is None else len(rows), ptr(rows),
                                             ptr(rows), idx.ctypes.data, idx.ctypes.data, pa.ctypes.data,
                                             idx.ctypes.data, r0.ctypes.data, p, radius, method, 5.0, 1.8,
                                             q.ctypes.data, n.ctypes.data, None)
        return lib.rmsf_contact_fraction_host(x.ctypes.data, 15, 2, 5, 5 if rows is None else len(rows), ptr(rows),
                                              pa.ctypes.data, idx.ctypes.data, r0.ctypes.data, p, radius, method, 5.0,
                                              1.8, q.ctypes.data, n.ctypes.data)

    for entry in ("rmsf_contact_counts", "rmsf_contact_counts_host"):
        for radius in (0.0, -1.0, float("nan"), float("inf")):
            assert counts(radius=radius, entry=entry) == _lib.RMSF_EINVAL
            assert b"radius" in lib.rmsf_last_error()
        assert counts(h_a=far, n_a=3, entry=entry) == _lib.RMSF_EINVAL
        assert b"out of range" in lib.rmsf_last_error() and entry.encode() in lib.rmsf_last_error()
        assert counts(n_a=0, entry=entry) == _lib.RMSF_EINVAL
        assert counts(n_a=6, entry=entry) == _lib.RMSF_EINVAL           # more dense rows than atoms
    for entry in ("rmsf_contact_fraction", "rmsf_contact_fraction_host"):
        for p in (0, -1):
            assert fraction(p=p, entry=entry) == _lib.RMSF_EINVAL
            assert b"at least one pair" in lib.rmsf_last_error()
        for radius in (0.0, -1.0, float("nan"), float("inf")):
            assert fraction(radius=radius, entry=entry) == _lib.RMSF_EINVAL
            assert b"radius" in lib.rmsf_last_error()
        assert fraction(pa=far, entry=entry) == _lib.RMSF_EINVAL
        assert b"out of range" in lib.rmsf_last_error()
        assert fraction(rows=far, entry=entry) == _lib.RMSF_EINVAL      # a staged row past the frame's atoms
        assert fraction(rows=i32([0, 1]), entry=entry) == _lib.RMSF_EINVAL   # a pair past the staged rows
        assert fraction(method=3, entry=entry) == _lib.RMSF_EINVAL
        assert b"method" in lib.rmsf_last_error()
    assert not out.any() and not q.any() and not n.any()
    assert math.isnan(lib.rmsf_contact_threshold_sq(-1.0)) and math.isnan(lib.rmsf_contact_threshold_sq(float("inf")))


def test_contact_threshold_sq():
    from rmsf_amd import contact_threshold_sq
    radii = [1.5, 4.5, 5.0, 8.0, 3.0, 6.0, 1e-3, 1e6] + list(np.random.default_rng(2).uniform(0.05, 40.0, 2000))
    for r in radii:
        t = contact_threshold_sq(r)
        assert math.sqrt(t) <= r < math.sqrt(np.nextafter(t, np.inf)), r
        assert abs(t - r * r) <= np.spacing(r * r), r                   # within an ulp of r * r
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            contact_threshold_sq(bad)


def threshold_counts(x, radius):
    from rmsf_amd import contact_threshold_sq
    d = x.astype(np.float64)[:, :, None, :] - x.astype(np.float64)[:, None, :, :]
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        return (d2 <= contact_threshold_sq(radius)).sum(axis=0).astype(np.int64)


def test_counts_host_on_jittered_points():
    x, radius = jittered(130, 70), 6.0
    rows = np.arange(130)
    ref = counts_reference(x, rows, rows, radius)
    mixed = ((ref > 0) & (ref < 70)).mean()
    assert 0.15 < mixed < 0.30 and (ref == 70).any() and (ref == 0).mean() > 0.5   # the comparison decides
    assert np.array_equal(threshold_counts(x, radius), ref)            # the two forms of the predicate agree
    assert np.array_equal(host_counts(x, None, None, radius), ref)
    ia, ib = np.arange(3, 130, 3), np.array([129, 0, 7, 7, 64])         # index arrays, a repeated row
    assert np.array_equal(host_counts(x, ia, ib, radius), ref[np.ix_(ia, ib)])


def test_counts_host_on_lattice_ties():
    x, radius = lattice(), 3.0
    rows = np.arange(125)
    d = distances(x[:1], rows, rows)[0]
    assert (d == radius).sum() == 1164                                  # <=, not <
    ref = counts_reference(x, rows, rows, radius)
    assert np.array_equal(host_counts(x, None, None, radius), ref)
    assert np.array_equal(threshold_counts(x, radius), ref)
    assert ref.sum() > counts_reference(x, rows, rows, np.nextafter(radius, 0.0)).sum()


def assert_poison_is_local(got_bad, got_clean, clean, radius):
    """All-atom square counts: the NaN's and the Inf's atoms lose their pairs
    in their frame, themselves included, and nothing else changes."""
    rows = np.arange(clean.shape[1])
    want = got_clean.copy()
    for frame, atom, _ in (NAN_AT, INF_AT):
        c = counts_reference(clean[frame:frame + 1], rows, rows, radius)
        want[atom, :] -= c[atom, :]
        want[:, atom] -= c[:, atom]
        want[atom, atom] += c[atom, atom]
        assert c[atom].sum() > 1 and got_bad[atom, atom] == clean.shape[0] - 1
    assert np.array_equal(got_bad, want)


def test_counts_host_with_nan_and_inf():
    clean, bad = poisoned()
    rows = np.arange(clean.shape[1])
    got = host_counts(bad, None, None, 6.0)
    assert np.array_equal(got, counts_reference(bad, rows, rows, 6.0))
    assert_poison_is_local(got, host_counts(clean, None, None, 6.0), clean, 6.0)


@pytest.mark.parametrize("kind", ["jittered", "lattice", "poisoned"])
def test_fraction_host(kind):
    x, radius = {"jittered": (jittered(130, 70), 6.0), "lattice": (lattice(), 3.0), "poisoned": (poisoned()[1], 6.0)}[kind]
    rows = np.arange(x.shape[1])
    ra, rb, r0 = natives(x[0], rows, rows, radius)
    assert len(ra) > x.shape[1]
    for method in ("hard_cut", "radius_cut", "soft_cut"):
        q_ref, n_ref = fraction_reference(x, ra, rb, r0, radius, method, **SOFT)
        q, n = host_fraction(x, ra, rb, r0, radius, method, **SOFT)
        assert np.array_equal(n, n_ref)
        if method == "soft_cut":
            ok = np.isfinite(q_ref)
            assert (np.abs(q[ok] - q_ref[ok]) <= soft_bound(len(ra)) * q_ref[ok]).all()
            assert np.array_equal(np.isnan(q), np.isnan(q_ref))
        else:
            assert np.array_equal(bits(q), bits(q_ref))
            assert q[0] == 1.0 and n[0] == len(ra)                      # the reference frame
    # through a list of staged rows: the same pairs, named by their positions in it
    staged = np.array([9, 4, 77, 30, 12])
    pa, pb = np.array([0, 1, 2, 4, 4]), np.array([1, 2, 3, 0, 4])
    q, n = host_fraction(x, pa, pb, None, radius, "hard_cut", rows=staged)
    q_ref, n_ref = fraction_reference(x, staged[pa], staged[pb], None, radius, "hard_cut")
    assert np.array_equal(n, n_ref) and np.array_equal(bits(q), bits(q_ref))


def test_python_natives_are_the_restatement():
    from rmsf_amd.contacts import native_pairs, pair_distances
    x = jittered(130, 70)
    ia, ib = np.arange(0, 60), np.arange(40, 130)
    pairs, r0 = native_pairs(x[0, ia], x[0, ib], 6.0)
    ra, rb, r0_ref = natives(x[0], ia, ib, 6.0)
    assert np.array_equal(ia[pairs[:, 0]], ra) and np.array_equal(ib[pairs[:, 1]], rb)
    assert np.array_equal(bits(r0), bits(r0_ref))
    assert np.array_equal(bits(pair_distances(x[:, ia], x[:, ib])), bits(distances(x, ia, ib)))


def test_refusals_without_a_device(monkeypatch):
    from rmsf_amd import ContactMap, Contacts, parallel
    from rmsf_amd.sources import DeviceSource
    x = np.zeros((6, 5, 3), np.float32)
    planes = object.__new__(DeviceSource)                              # HBM-resident [F, 3, n_atoms]; no tensor needed
    planes.layout, planes.n_sel = "soa", 5
    for cls in (ContactMap, Contacts):
        name = cls.__name__
        with pytest.raises(NotImplementedError, match=f"{name} runs on one device"):
            cls(x, gpus=2).run()
        with pytest.raises(NotImplementedError, match=f"{name} runs on one device"):
            cls([x, x]).run()
        with pytest.raises(NotImplementedError, match=f"{name} reads"):
            cls(planes).run()
        for radius in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="radius"):
                cls(x, radius=radius)
        with pytest.raises(ValueError, match="layout"):
            cls(x, layout="rows")
        with pytest.raises(ValueError, match="no atoms"):
            cls(x, select=[])
        with pytest.raises(IndexError, match="negative"):
            cls(x, select=[0, -1])
        with pytest.raises(TypeError, match="integer"):
            cls(x, select_b=[0.5])
    with pytest.raises(ValueError, match="method"):
        Contacts(x, method="q1q2")
    with pytest.raises(ValueError, match="reference"):
        Contacts(x, reference=np.zeros((5, 2)))
    with pytest.raises(ValueError, match="one length"):
        Contacts(x, pairs=([0, 1], [1]))
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    for cls in (ContactMap, Contacts):
        with pytest.raises(NotImplementedError, match="more than one rank"):
            cls(x).run()


def test_zero_native_pairs():
    """Two atoms 100 A apart: no native pair at 4.5 A, and Q would be 0 / 0.
    The native search is on the host; nothing reaches a device."""
    from rmsf_amd import Contacts
    ref = np.array([[0, 0, 0], [100, 0, 0]], np.float32)
    c = Contacts(np.zeros((3, 2, 3), np.float32), select=[0], select_b=[1], reference=ref)
    with pytest.raises(ValueError, match="no pair"):
        c._native(ref, np.array([0]), np.array([1]))
    pairs, r0 = Contacts(np.zeros((3, 2, 3), np.float32), radius=150.0, select=[0], select_b=[1])._native(
        ref, np.array([0]), np.array([1]))
    assert pairs.tolist() == [[0, 0]] and r0.tolist() == [100.0]


def test_script_contact_options():
    """rmsf_mi355x.py --contact-map / --contacts / --contact-radius / --contacts-method: refused before any device work."""
    import os
    import subprocess
    import sys

    from conftest import ROOT
    script = f"{ROOT}/mdanalysis-mpi_amd/rmsf_mi355x.py"
    cases = ((["--contact-radius", "4.5"], "needs --contact-map or --contacts", {}),
             (["--contact-map", "x.npy", "--contact-radius", "0"], "positive and finite", {}),
             (["--contacts", "x.npy", "--contact-radius", "nan"], "positive and finite", {}),
             (["--contacts-method", "soft_cut"], "needs --contacts", {}),
             (["--contact-map", "x.npy", "--contacts-method", "soft_cut"], "needs --contacts", {}),
             (["--contacts", "x.npy", "--contacts-method", "q1q2"], "invalid choice", {}),
             (["--contact-map", "x.npy"], "one process", {"WORLD_SIZE": "2"}),
             (["--contacts", "x.npy"], "one process", {"WORLD_SIZE": "2"}))
    for extra, msg, env in cases:
        r = subprocess.run([sys.executable, script, "--synthetic", "10", "5", *extra], capture_output=True, text=True,
                           timeout=120, env={**os.environ, **env})
        assert r.returncode == 2 and msg in r.stderr, (extra, r.stderr[-500:])
