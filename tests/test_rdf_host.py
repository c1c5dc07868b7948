"""CPU tier of the radial distribution function (csrc/rdf.hip): ``rmsf_rdf_edges``,
the argument checks (which come before any launch) and ``rmsf_rdf_counts_host``
-- the definition in plain C++ -- against a numpy restatement of it and against
``numpy.histogram``, for equality; what ``InterRDF`` refuses without a device;
``XTCFile.boxes``.

The definition (include/rmsf_hip.h): f32 coordinates, ``dx = (double)xa -
(double)xb`` and so for y and z; with a box ``dx = dx - Lx * rint(dx * ix)``,
``ix = 1.0 / Lx``; ``d2 = (dx*dx + dy*dy) + dz*dz`` with no FMA, ``d =
sqrt(d2)``; edges ``numpy.linspace(rmin, rmax, nbins + 1)``; bin k iff ``e_k <=
d < e_(k+1)``, the last bin also ``d == rmax``, a NaN in no bin.  numpy
evaluates every step to the same bits, so counts are compared for equality.

The GPU tier (tests/test_gpu_rdf.py) takes its inputs and references from
here."""
import ctypes
import functools

import numpy as np
import pytest

from test_contacts_host import i32, jittered, lattice, poisoned, ptr, NAN_AT, INF_AT

POISON = -7


# ---- the restatement ---------------------------------------------------------------------
def box6(box, n_frames):
    """f64 [F, 6] = Lx, Ly, Lz, 1/Lx, 1/Ly, 1/Lz from [3] or [F, 3]; None stays None."""
    if box is None:
        return None
    b = np.broadcast_to(np.asarray(box, dtype=np.float64), (n_frames, 3))
    return np.ascontiguousarray(np.concatenate([b, 1.0 / b], axis=1))


def image_distances(x, ia, ib, box=None):
    """f64 [F, n_a, n_b] by the definition; ``box`` [3] or [F, 3] or None."""
    a = x[:, ia].astype(np.float64)[:, :, None, :]
    b = x[:, ib].astype(np.float64)[:, None, :, :]
    with np.errstate(invalid="ignore", over="ignore"):
        d = a - b
        if box is not None:
            b6 = box6(box, len(x))
            L, iL = b6[:, None, None, :3], b6[:, None, None, 3:]
            d = d - L * np.rint(d * iL)
        return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def kept(n_a, n_b, symmetric=False, excl=None):
    """bool [n_a, n_b]: the pairs that are counted."""
    i, j = np.arange(n_a)[:, None], np.arange(n_b)[None, :]
    keep = np.ones((n_a, n_b), dtype=bool)
    if symmetric:
        keep &= i != j
    if excl is not None:
        keep &= (i // excl[0]) != (j // excl[1])
    return keep


def bin_index(d, rng, nbins):
    """int64, the shape of d: the bin of every distance by the definition, -1 for none."""
    e = np.linspace(rng[0], rng[1], nbins + 1)
    with np.errstate(invalid="ignore"):
        k = np.searchsorted(e, d, side="right") - 1          # e_k <= d < e_(k+1); a NaN sorts past the end
        k = np.where(d == e[-1], nbins - 1, k)
        return np.where((d >= e[0]) & (d <= e[-1]), k, -1).astype(np.int64)


def count_bins(k, nbins):
    return np.bincount(k.ravel() + 1, minlength=nbins + 1)[1:nbins + 1].astype(np.int64)


def reference(x, ia, ib, box, rng, nbins, symmetric=False, excl=None, check_numpy=True):
    """int64 [nbins] by the restatement; and numpy.histogram agrees."""
    d = image_distances(x, ia, ib, box)[:, kept(len(ia), len(ib), symmetric, excl)]
    got = count_bins(bin_index(d, rng, nbins), nbins)
    if check_numpy:
        with np.errstate(invalid="ignore"):
            h = np.histogram(d[np.isfinite(d)], bins=nbins, range=rng)[0]
        assert np.array_equal(got, h)
    return got


# ---- the library's host entry ------------------------------------------------------------
def host_rdf(x, ia, ib, box, rng, nbins, symmetric=False, excl=None, pad=3):
    from rmsf_amd import _lib
    x = np.ascontiguousarray(x)
    n_frames, n_atoms = x.shape[:2]
    ia = i32(ia)
    ib = ia if symmetric else i32(ib)
    n_a, n_b = (n_atoms if ia is None else len(ia)), (n_atoms if ib is None else len(ib))
    b6 = box6(box, n_frames)
    ea, eb = (0, 0) if excl is None else excl
    out = np.full(nbins + pad, POISON, dtype=np.int64)
    _lib.call("rmsf_rdf_counts_host", x.ctypes.data, 3 * n_atoms, n_frames, n_atoms, ptr(ia), n_a, ptr(ib), n_b,
              int(symmetric), ea, eb, ptr(b6), float(rng[0]), float(rng[1]), nbins, out.ctypes.data)
    assert (out[nbins:] == POISON).all()                      # nothing written past nbins
    return out[:nbins].copy()


def edges_and_thresholds(rng, nbins):
    from rmsf_amd import _lib
    e, t = np.empty(nbins + 1), np.empty(nbins + 1)
    _lib.call("rmsf_rdf_edges", float(rng[0]), float(rng[1]), nbins, e.ctypes.data, t.ctypes.data)
    return e, t


# ---- inputs ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cube(m, n_frames=1):
    """The m^3 integer lattice.  Read only."""
    return lattice(n_frames, m)


@functools.lru_cache(maxsize=None)
def uniform(n_atoms, n_frames, box, seed):
    """Uniform points in [0, L) of a box.  Read only."""
    rng = np.random.default_rng(seed)
    x = (rng.random((n_frames, n_atoms, 3)) * np.asarray(box)).astype(np.float32)
    x = np.minimum(x, np.nextafter(np.asarray(box, dtype=np.float32), np.float32(0)))   # f32 rounding up to L
    x.setflags(write=False)
    return x


def frame_boxes(n_frames, lo=20.0, seed=2):
    """f64 [F, 3]: another box every frame, edges in [lo, lo + 4)."""
    return lo + 4.0 * np.random.default_rng(seed).random((n_frames, 3))


LATTICE_CASES = [((0.0, 4.0), 4), ((0.5, 4.0), 7), ((0.0, 3.0), 75), ((1.0, 4.0), 1)]
LATTICE_BOXES = [None, (8.0, 8.0, 8.0), (10.0, 8.0, 9.0)]
NEW_SYMBOLS = ("rmsf_rdf_edges", "rmsf_rdf_counts_plan", "rmsf_rdf_counts_workspace_bytes", "rmsf_rdf_counts",
               "rmsf_rdf_counts_host", "rmsf_xtc_boxes")


# ---- tests -------------------------------------------------------------------------------
def test_abi():
    from rmsf_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


@pytest.mark.parametrize("rng, nbins", LATTICE_CASES + [((0.0, 15.0), 75), ((0.0, 15.0), 2048), ((0.3, 7.7), 999),
                                                        ((2.0, 1.0e6), 13)])
def test_edges_are_linspace_and_thresholds_are_tight(rng, nbins):
    e, t = edges_and_thresholds(rng, nbins)
    assert e.tobytes() == np.linspace(rng[0], rng[1], nbins + 1).tobytes()
    below = np.nextafter(t, -np.inf)
    # an inner edge: T_k is the smallest double whose root is >= e_k
    assert (np.sqrt(t[:-1]) >= e[:-1]).all()
    inner = e[:-1] > 0
    assert (np.sqrt(below[:-1][inner]) < e[:-1][inner]).all()
    assert (t[:-1][~inner] == 0).all()                        # e_0 = 0: every d2 >= 0 is at or past it
    # the closed last edge: T_nbins is the first double above the largest whose root is <= rmax
    assert np.sqrt(t[-1]) > e[-1] and np.sqrt(below[-1]) <= e[-1]
    assert (np.diff(t) > 0).all()


def test_plan_is_host_only_and_checked():
    from rmsf_amd import _lib
    lib = _lib.load()
    v = [ctypes.c_int32(-1) for _ in range(4)]
    refs = [ctypes.byref(t) for t in v]
    assert lib.rmsf_rdf_counts_plan(214, 214, 20000, 1, *refs) == _lib.RMSF_OK
    tile_a, tile_b, chunk, splits = (t.value for t in v)
    assert tile_a >= 1 and tile_b >= 1 and chunk >= 1 and splits > 1
    assert lib.rmsf_rdf_counts_plan(1, 1, 1, 0, *refs) == _lib.RMSF_OK and v[3].value == 1
    # a run so long that one workgroup's int32 counters could wrap is split even when the tiles are many:
    # 2 * tile_a * tile_b a frame into one counter at the most
    n_frames = 2 ** 31 - 1
    assert lib.rmsf_rdf_counts_plan(4096, 4096, n_frames, 1, *refs) == _lib.RMSF_OK
    per_split = -(-n_frames // v[3].value)
    assert 2 * tile_a * tile_b * (per_split + chunk) < 2 ** 31
    for bad in ((0, 5, 5, 0), (5, 0, 5, 0), (5, 5, 0, 0), (5, 6, 5, 1)):
        assert lib.rmsf_rdf_counts_plan(*bad, *refs) == _lib.RMSF_EINVAL
        assert b"rmsf_rdf_counts_plan" in lib.rmsf_last_error()
    assert lib.rmsf_rdf_counts_workspace_bytes(75) >= 8 * 76


def test_argument_checks_come_before_any_launch():
    """No device is touched: the pointers are host arrays, and every call is
    refused on its arguments, by the device entry and by the host entry."""
    from rmsf_amd import _lib
    lib = _lib.load()
    x = np.zeros((2, 6, 3), np.float32)
    out = np.zeros(8, np.int64)
    work = np.zeros(4096, np.float64)
    good_box = box6((10.0, 12.0, 14.0), 2)

    def run(entry, idx_a=None, n_a=6, idx_b=None, n_b=6, symmetric=0, excl=(0, 0), box=None, rng=(0.0, 4.0), nbins=4):
        ia, ib = i32(idx_a), i32(idx_b)
        if entry == "rmsf_rdf_counts":
            return lib.rmsf_rdf_counts(x.ctypes.data, 18, 2, 6, ptr(ia), ptr(ia), n_a, ptr(ib), ptr(ib), n_b, symmetric,
                                       excl[0], excl[1], ptr(box), ptr(box), rng[0], rng[1], nbins, out.ctypes.data,
                                       work.ctypes.data, work.nbytes, None)
        return lib.rmsf_rdf_counts_host(x.ctypes.data, 18, 2, 6, ptr(ia), n_a, ptr(ib), n_b, symmetric, excl[0],
                                        excl[1], ptr(box), rng[0], rng[1], nbins, out.ctypes.data)

    def bad_box(f, k, v, inv=None):
        b = good_box.copy()
        b[f, k] = v
        b[f, 3 + k] = (1.0 / v if v else np.inf) if inv is None else inv
        return b

    bad = [dict(nbins=0), dict(nbins=2049), dict(nbins=-1),
           dict(rng=(-0.5, 4.0)), dict(rng=(4.0, 4.0)), dict(rng=(5.0, 4.0)), dict(rng=(0.0, np.inf)),
           dict(rng=(np.nan, 4.0)), dict(rng=(0.0, np.nan)),
           dict(box=bad_box(1, 2, 0.0)), dict(box=bad_box(0, 0, -10.0)), dict(box=bad_box(1, 1, np.inf, 0.0)),
           dict(box=bad_box(0, 1, np.nan)),
           dict(box=bad_box(1, 0, 10.0, np.nextafter(0.1, 1.0))),           # not 1.0 / L
           dict(box=bad_box(1, 0, 7.9)),                                     # rmax 4.0 > 7.9 / 2, in the second frame only
           dict(idx_a=[0, 6, 2], n_a=3), dict(idx_b=[0, -1], n_b=2),
           dict(symmetric=1, n_a=6, n_b=5),
           dict(excl=(4, 3)), dict(excl=(3, 4)), dict(excl=(3, 0)), dict(excl=(-2, -2))]
    for entry in ("rmsf_rdf_counts", "rmsf_rdf_counts_host"):
        for kw in bad:
            assert run(entry, **kw) == _lib.RMSF_EINVAL, (entry, kw)
            assert entry.encode() in lib.rmsf_last_error(), (entry, kw)
    # rmax == L / 2 exactly is allowed, and the host entry takes the good arguments
    assert run("rmsf_rdf_counts_host", box=box6((8.0, 8.0, 9.0), 2)) == _lib.RMSF_OK
    assert run("rmsf_rdf_counts_host", excl=(3, 2), box=good_box) == _lib.RMSF_OK
    assert lib.rmsf_rdf_edges(0.0, 4.0, 0, None, None) == _lib.RMSF_EINVAL
    assert lib.rmsf_rdf_edges(1.0, 1.0, 4, None, None) == _lib.RMSF_EINVAL
    assert lib.rmsf_rdf_edges(0.0, 4.0, 4, None, None) == _lib.RMSF_OK


@pytest.mark.parametrize("box", LATTICE_BOXES)
@pytest.mark.parametrize("rng, nbins", LATTICE_CASES)
def test_lattice_distances_on_the_edges(box, rng, nbins):
    x = lattice(3, 5)
    rows = np.arange(x.shape[1])
    d = image_distances(x, rows, rows, box)
    e = np.linspace(rng[0], rng[1], nbins + 1)
    assert np.isin(d, e).sum() >= 700                                   # hundreds of distances sit on an edge
    ref = reference(x, rows, rows, box, rng, nbins)
    assert np.array_equal(host_rdf(x, None, None, box, rng, nbins), ref)
    assert np.array_equal(host_rdf(x, rows, rows, box, rng, nbins), ref)


def test_every_atom_of_a_periodic_lattice_has_the_same_environment():
    """m^3 lattice in a box of edge m, rmax = m / 2: the ties dx = +-L/2 land
    the same way for every atom."""
    m = 6
    x, box, rng, nbins = cube(m), (float(m),) * 3, (0.0, 3.0), 12
    rows = np.arange(m ** 3)
    k = bin_index(image_distances(x, rows, rows, box)[0], rng, nbins)
    per_atom = np.stack([count_bins(row, nbins) for row in k])
    assert (per_atom == per_atom[0]).all() and per_atom[0].sum() > 100
    assert per_atom[0, -1] > 0                                          # d == rmax lands in the last bin
    for i in (0, 17, m ** 3 - 1):
        assert np.array_equal(host_rdf(x, [i], rows, box, rng, nbins), per_atom[0])
    assert np.array_equal(host_rdf(x, None, None, box, rng, nbins), m ** 3 * per_atom[0])


KD_CASES = [((20.0, 22.0, 25.0), 3), ((30.0, 30.0, 30.0), 1)]


@pytest.mark.parametrize("box, seed", KD_CASES)
def test_minimum_image_against_a_periodic_kd_tree(box, seed):
    """An independent minimum image: scipy's periodic k-d tree counts the
    pairs within each edge.  It computes the distance another way, so the two
    agree only where no distance is within rounding of an edge: the gap is
    asserted, a seed that loses it fails here and not in the comparison."""
    spatial = pytest.importorskip("scipy.spatial")
    rng, nbins = (0.0, 10.0), 30
    x = uniform(120, 1, box, seed)
    rows = np.arange(120)
    d = image_distances(x, rows, rows, box)[0]
    e = np.linspace(rng[0], rng[1], nbins + 1)
    off = d[~np.eye(120, dtype=bool)]
    assert np.abs(off[:, None] - e[None, :]).min() >= 1e-6
    tree = spatial.cKDTree(x[0].astype(np.float64), boxsize=np.asarray(box))
    within = tree.count_neighbors(tree, e)                              # ordered pairs with d <= e_k, self pairs included
    want = np.diff(within).astype(np.int64)
    want[0] += within[0] - 120                                          # e_0 = 0 takes only the self pairs
    got = host_rdf(x, rows, None, box, rng, nbins, symmetric=True)
    assert np.array_equal(got, want)
    assert np.array_equal(reference(x, rows, rows, box, rng, nbins, symmetric=True), want)
    # the image matters: in free space the same points give another histogram
    assert not np.array_equal(host_rdf(x, rows, None, None, rng, nbins, symmetric=True), want)


def test_a_different_box_every_frame():
    x = jittered(90, 7)
    boxes = frame_boxes(7)
    rows_a, rows_b = np.arange(0, 60), np.arange(40, 90)
    rng, nbins = (0.5, 9.0), 40
    ref = reference(x, rows_a, rows_b, boxes, rng, nbins)
    assert np.array_equal(host_rdf(x, rows_a, rows_b, boxes, rng, nbins), ref)
    per_frame = sum(reference(x[f:f + 1], rows_a, rows_b, boxes[f], rng, nbins) for f in range(7))
    assert np.array_equal(per_frame, ref)
    assert not np.array_equal(reference(x, rows_a, rows_b, boxes[0], rng, nbins), ref)   # the boxes are told apart


@pytest.mark.parametrize("box", [None, (24.0, 23.0, 22.0)])
def test_a_non_finite_coordinate_loses_only_its_own_pairs(box):
    clean, bad = poisoned()
    n = clean.shape[1]
    rows = np.arange(n)
    rng, nbins = (0.0, 9.0), 30
    got = host_rdf(bad, None, None, box, rng, nbins)
    assert np.array_equal(got, reference(bad, rows, rows, box, rng, nbins))
    # what is missing is exactly the pairs of the two atoms in their frames
    lost = np.zeros(nbins, dtype=np.int64)
    for f, atom, _ in (NAN_AT, INF_AT):
        row = bin_index(image_distances(clean[f:f + 1], [atom], rows, box)[0, 0], rng, nbins)
        lost += 2 * count_bins(row, nbins)                             # as a row and as a column ...
        lost[row[atom]] -= 1                                           # ... its self pair once
    assert np.array_equal(host_rdf(clean, None, None, box, rng, nbins) - got, lost) and lost.sum() > 0


@pytest.mark.parametrize("box", [None, (21.0, 22.0, 23.0)])
def test_symmetric_route_and_exclusion_blocks(box):
    x = jittered(66, 5)
    rng, nbins = (0.0, 9.5), 25
    rows = np.random.default_rng(4).permutation(66)[:60]
    full = host_rdf(x, rows, rows, box, rng, nbins)
    sym = host_rdf(x, rows, None, box, rng, nbins, symmetric=True)
    self_pairs = np.zeros(nbins, dtype=np.int64)
    self_pairs[0] = 60 * 5                                              # d = 0 in every frame
    assert np.array_equal(sym, full - self_pairs) and (sym % 2 == 0).all()
    assert np.array_equal(sym, reference(x, rows, rows, box, rng, nbins, symmetric=True))
    for excl in ((3, 3), (1, 2)):
        rows_b = rows[:60] if excl[1] == 3 else np.concatenate([rows, rows[::-1]])
        ref = reference(x, rows, rows_b, box, rng, nbins, excl=excl)
        assert np.array_equal(host_rdf(x, rows, rows_b, box, rng, nbins, excl=excl), ref)
        assert ref.sum() < reference(x, rows, rows_b, box, rng, nbins).sum()
    assert np.array_equal(host_rdf(x, rows, None, box, rng, nbins, symmetric=True, excl=(3, 3)),
                          reference(x, rows, rows, box, rng, nbins, symmetric=True, excl=(3, 3)))


def test_normalisation_of_an_ideal_gas():
    """Uniform points in a periodic box: g(r) = 1 in expectation.  A bin's
    count c is twice a Poisson number of unordered pairs, so its relative
    standard deviation is sqrt(2 / c): 4.5 % at the emptiest bin used (c >
    1,000), and each bin is held to five of its own."""
    from rmsf_amd.rdf import normalise
    box, n, n_frames = (30.0, 30.0, 30.0), 600, 4
    x = uniform(n, n_frames, box, 9)
    rng, nbins = (0.0, 15.0), 30
    count = host_rdf(x, None, None, box, rng, nbins, symmetric=True)
    e = np.linspace(*rng, nbins + 1)
    g = normalise(count, e, n_frames, "rdf", n, n, 27000.0, symmetric=True)
    used = count > 1000
    assert used.sum() >= 20
    margin = 5.0 * np.sqrt(2.0 / count[used])
    assert margin.max() <= 5.0 * np.sqrt(2.0 / 1000.0)
    assert (np.abs(g[used] - 1.0) <= margin).all(), np.abs(g[used] - 1.0).max()
    assert np.abs(g[count > 20000] - 1.0).max() < 0.05                  # the full bins: within a few percent
    # the formula, written out once more
    shell = 4.0 / 3.0 * np.pi * np.diff(e ** 3)
    assert np.allclose(g, count / (n_frames * shell * (n * n - n) / 27000.0), rtol=1e-14, atol=0)
    dens = normalise(count, e, n_frames, "density", n, n, 27000.0, symmetric=True)
    assert np.allclose(dens, count / (n_frames * shell), rtol=1e-14, atol=0)
    assert np.array_equal(normalise(count, e, n_frames, "none", n, n, 27000.0), count / n_frames)
    ex = normalise(count, e, n_frames, "rdf", n, n, 27000.0, exclusion_block=(3, 3))
    assert np.allclose(ex, count / (n_frames * shell * (n * n - 9 * (n // 3)) / 27000.0), rtol=1e-14, atol=0)
    assert np.isnan(normalise(np.zeros(nbins), e, 0, "rdf", n, n, 27000.0)).all()


def test_interrdf_refusals_need_no_device():
    from rmsf_amd import InterRDF
    x = np.zeros((3, 10, 3), np.float32)
    with pytest.raises(ValueError, match="norm='rdf' needs a box"):
        InterRDF(x)
    InterRDF(x, norm="density")
    InterRDF(x, norm="none")
    with pytest.raises(ValueError, match="norm"):
        InterRDF(x, norm="g", box=(40.0, 40.0, 40.0))
    with pytest.raises(ValueError, match="file"):
        InterRDF(x, box="file")
    with pytest.raises(ValueError, match="file"):
        InterRDF("traj.dcd", box="file")
    with pytest.raises(ValueError):
        InterRDF(x, box="xtc")
    with pytest.raises(NotImplementedError, match="orthorhombic"):
        InterRDF(x, box=(40.0, 40.0, 40.0, 90.0, 90.0, 60.0))
    with pytest.raises(NotImplementedError, match="orthorhombic"):
        InterRDF(x, box=np.array([[40.0, 40.0, 40.0, 90.0, 90.0, 90.0]] * 2 + [[40.0, 40.0, 40.0, 90.0, 80.0, 90.0]]))
    InterRDF(x, box=(40.0, 40.0, 40.0, 90.0, 90.0, 90.0))
    for bad in ((40.0, 0.0, 40.0), (40.0, -1.0, 40.0), (40.0, np.nan, 40.0), (40.0, np.inf, 40.0), (40.0, 40.0),
                np.zeros((3, 4))):
        with pytest.raises(ValueError):
            InterRDF(x, box=bad)
    with pytest.raises(ValueError, match="half"):
        InterRDF(x, box=(40.0, 29.9, 40.0))                             # the default range ends at 15
    InterRDF(x, box=(40.0, 30.0, 40.0))
    for kw in (dict(nbins=0), dict(nbins=2049), dict(nbins=7.5), dict(range=(-1.0, 5.0)), dict(range=(5.0, 5.0)),
               dict(range=(0.0, np.inf)), dict(range=(0.0,)), dict(exclusion_block=(0, 1)), dict(exclusion_block=3)):
        with pytest.raises(ValueError):
            InterRDF(x, norm="none", **kw)
    with pytest.raises(NotImplementedError):
        InterRDF(x, norm="none", gpus=2).run()


def test_xtc_boxes_round_trip(tmp_path):
    from rmsf_amd.xtc import XTCFile, write_xtc
    x = uniform(20, 5, (20.0, 20.0, 20.0), 1)
    boxes = np.array([[20.0, 22.0, 25.0], [20.5, 22.25, 24.0], [21.3, 22.7, 23.9]])
    path = str(tmp_path / "boxes.xtc")
    frames_of = [slice(0, 2), slice(2, 3), slice(3, 5)]
    for k, (b, fr) in enumerate(zip(boxes, frames_of)):
        write_xtc(path, x[fr], box=np.diag(b), append=k > 0)
    with XTCFile(path) as fh:
        got = fh.boxes()
        raw = fh.frame_info(2)[2]
    # the file holds f32 nm (the writer's f32 product); boxes() widens that and multiplies by 10.0 in f64
    nm = np.float32(boxes.astype(np.float32) * np.float32(0.1))
    want = np.repeat(nm.astype(np.float64) * 10.0, [2, 1, 2], axis=0)
    assert got.dtype == np.float64 and got.shape == (5, 3) and got.tobytes() == want.tobytes()
    assert np.abs(got - np.repeat(boxes, [2, 1, 2], axis=0)).max() < 1e-5
    assert raw.dtype == np.float32 and np.array_equal(np.diag(raw), nm[1])      # frame_info: as it was
    tri = np.diag(boxes[0])
    tri[1, 0] = 3.0
    write_xtc(path, x[:2], box=tri)
    with XTCFile(path) as fh, pytest.raises(NotImplementedError, match="triclinic"):
        fh.boxes()
    write_xtc(path, x[:2])
    with XTCFile(path) as fh, pytest.raises(ValueError, match="no box"):
        fh.boxes()


def test_cli_refuses_bad_rdf_options(capsys):
    import rmsf_mi355x
    for argv in (["--synthetic", "50", "8", "--rdf-nbins", "10"],
                 ["--synthetic", "50", "8", "--rdf", "o.npz", "--rdf-nbins", "0"],
                 ["--synthetic", "50", "8", "--rdf", "o.npz", "--rdf-range", "3", "2"],
                 ["--synthetic", "50", "8", "--rdf", "o.npz", "--rdf-box", "file"],
                 ["--synthetic", "50", "8", "--rdf", "o.npz", "--rdf-box", "20", "20"],
                 ["--synthetic", "50", "8", "--rdf", "o.npz", "--rdf-box", "20", "20", "20"],
                 ["--synthetic", "50", "8", "--rdf", "o.npz", "--rdf-select-b", "name OW"]):
        with pytest.raises(SystemExit) as exc:
            rmsf_mi355x.main(argv)
        assert exc.value.code == 2, argv
        assert "--rdf" in capsys.readouterr().err
