"""GPU tier of the radial distribution function (csrc/rdf.hip): ``rmsf_rdf_counts``
through ``Engine`` and ``InterRDF`` end to end, against the numpy restatement of
the definition in tests/test_rdf_host.py and the library's ``_host`` entry.

Everything is integers after one comparison: counts are compared for equality,
twice (the same bytes both times), in a poison-filled buffer longer than nbins.

The shapes stand on the launcher's own plan (``rmsf_rdf_counts_plan``): tile
edges T, frame chunk C and a frame count it splits, not on a workload."""
import functools

import numpy as np
import pytest

from test_contacts_host import jittered, lattice, poisoned
from test_rdf_host import (LATTICE_BOXES, LATTICE_CASES, POISON, bin_index, count_bins, cube, frame_boxes, host_rdf,
                           image_distances, kept, reference)

pytestmark = pytest.mark.gpu

RANGE = (0.5, 9.0)                     # the jittered atoms: distances below, inside and above
ALL_BINS = (1, 2, 75, 2048)


@functools.lru_cache(maxsize=None)
def engine():
    import torch

    from rmsf_amd.engine import Engine
    return Engine(torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def plan(n_a, n_b, n_frames, symmetric=False):
    """(tile_a, tile_b, frame_chunk, n_splits): host only, so the cases can be listed without a device."""
    import ctypes

    from rmsf_amd import _lib
    v = [ctypes.c_int32(0) for _ in range(4)]
    _lib.call("rmsf_rdf_counts_plan", n_a, n_b, n_frames, int(symmetric), *(ctypes.byref(t) for t in v))
    return tuple(t.value for t in v)


@functools.lru_cache(maxsize=None)
def on_device(kind, *args):
    import torch
    x = {"jittered": jittered, "lattice": lattice, "cube": cube, "poisoned": lambda *a: poisoned(*a)[1]}[kind](*args)
    return x, torch.tensor(x, device="cuda:0")


def device_rdf(x_dev, ia, ib, box, rng, nbins, symmetric=False, excl=None, pad=5, n_atoms=None, fstride=None):
    """Engine.rdf_counts into a poison-filled int64 buffer of nbins + pad,
    twice: the same bytes, the poison past nbins intact.  int64 [nbins]."""
    import torch
    n_frames = x_dev.shape[0]
    n_atoms = x_dev.shape[1] if n_atoms is None else n_atoms
    n_a = n_atoms if ia is None else len(ia)
    n_b = n_a if symmetric else (n_atoms if ib is None else len(ib))
    if box is not None:
        box = np.broadcast_to(np.asarray(box, dtype=np.float64), (n_frames, 3))
    runs = []
    for _ in range(2):
        out = torch.full((nbins + pad,), POISON, dtype=torch.int64, device="cuda:0")
        got = engine().rdf_counts(x_dev.data_ptr(), x_dev.stride(0) if fstride is None else fstride, n_frames, n_atoms,
                                  ia, n_a, ib, n_b, rng[0], rng[1], nbins, symmetric=symmetric, exclusion_block=excl,
                                  box=box, out=out)
        torch.cuda.synchronize()
        assert got.shape == (nbins,) and got.data_ptr() == out.data_ptr()
        runs.append(out.cpu().numpy())
    assert runs[0].tobytes() == runs[1].tobytes()                      # a second run: the same bytes
    assert (runs[0][nbins:] == POISON).all()                           # nothing written past nbins
    assert (runs[0][:nbins] >= 0).all()                                # every bin written
    return runs[0][:nbins].copy()


def edges():
    tile_a, tile_b, chunk, _ = plan(200, 200, 64)
    return tile_a, tile_b, chunk


def sizes(t):
    return sorted({1, t - 1, t, t + 1, 2 * t + 2} - {0})


def frame_counts():
    c = edges()[2]
    return sorted({1, c - 1, c, c + 1} - {0}) + [2 * c + 3]           # the last: several splits, a ragged tail


def test_the_plan_is_not_trivial():
    ta, tb, c = edges()
    assert max(sizes(ta)) > 2 * ta and max(sizes(tb)) > 2 * tb          # two tiles a side and a partial third
    split = frame_counts()[-1]
    for sym in (False, True):
        n_splits = plan(max(sizes(ta)), max(sizes(ta)) if sym else max(sizes(tb)), split, sym)[3]
        assert n_splits > 1 and (split % c or split % n_splits)
    assert plan(1, 1, 1)[3] == 1 and c > 1
    assert plan(3341, 3341, 4096, True)[:3] == (ta, tb, c)               # the plan's edges do not move with the shape
    assert engine().rdf_counts_plan(3341, 3341, 4096, True) == plan(3341, 3341, 4096, True)


@functools.lru_cache(maxsize=None)
def pair_bins(n, n_frames, periodic, nbins):
    """int64 [F, n, n]: the bin of every pair of the jittered atoms, computed once a case."""
    x = jittered(n, n_frames)
    rows = np.arange(n)
    k = bin_index(image_distances(x, rows, rows, frame_boxes(n_frames) if periodic else None), RANGE, nbins)
    k.setflags(write=False)
    return k


def subset_counts(k, ia, ib, nbins, symmetric=False, excl=None):
    return count_bins(k[:, ia][:, :, ib][:, kept(len(ia), len(ib), symmetric, excl)], nbins)


@pytest.mark.parametrize("periodic", [False, True], ids=["free", "periodic"])
@pytest.mark.parametrize("n_frames", frame_counts())
def test_counts_at_the_plan_edges(n_frames, periodic):
    ta, tb, _ = edges()
    n = max(sizes(ta) + sizes(tb))
    x, x_dev = on_device("jittered", n, n_frames)
    box = frame_boxes(n_frames) if periodic else None                  # another box every frame
    rows = np.arange(n)
    for nbins in ALL_BINS:
        k = pair_bins(n, n_frames, periodic, nbins)
        full = subset_counts(k, rows, rows, nbins)
        if nbins == 75:
            assert np.array_equal(host_rdf(x, None, None, box, RANGE, nbins), full)
            assert np.array_equal(reference(x, rows, rows, box, RANGE, nbins), full)
            assert (full > 0).sum() > 60 and (k < 0).mean() > 0.1       # bins in use, and pairs out of range
        for n_a in sizes(ta):
            ia = np.arange(n_a)
            for n_b in sizes(tb):
                ib = np.arange(n - n_b, n)                              # the other end: A is not B
                got = device_rdf(x_dev, ia, ib, box, RANGE, nbins)
                assert np.array_equal(got, subset_counts(k, ia, ib, nbins)), (nbins, n_a, n_b)
            sym = device_rdf(x_dev, ia, None, box, RANGE, nbins, symmetric=True)
            assert np.array_equal(sym, subset_counts(k, ia, ia, nbins, symmetric=True)), (nbins, n_a)
        # dense rows: no index array at all
        assert np.array_equal(device_rdf(x_dev, None, None, box, RANGE, nbins), full)
        assert np.array_equal(device_rdf(x_dev, None, None, box, RANGE, nbins, symmetric=True),
                              subset_counts(k, rows, rows, nbins, symmetric=True))


@pytest.mark.parametrize("periodic", [False, True], ids=["free", "periodic"])
def test_many_splits_permuted_repeated_rows_and_exclusion_blocks(periodic):
    _, _, c = edges()
    n_frames = 40 * c + 5
    x, x_dev = on_device("jittered", 70, n_frames)
    assert plan(70, 70, n_frames)[3] > 1
    box = frame_boxes(n_frames) if periodic else None
    rng = np.random.default_rng(11)
    ia, ib = rng.permutation(70)[:48], rng.integers(0, 70, 66)         # out of order; repeated
    k = pair_bins(70, n_frames, periodic, 75)
    assert np.array_equal(device_rdf(x_dev, ia, ib, box, RANGE, 75), subset_counts(k, ia, ib, 75))
    for excl in ((3, 3), (1, 2), (48, 66)):
        want = subset_counts(k, ia, ib, 75, excl=excl)
        assert np.array_equal(device_rdf(x_dev, ia, ib, box, RANGE, 75, excl=excl), want), excl
        assert np.array_equal(host_rdf(x, ia, ib, box, RANGE, 75, excl=excl), want), excl
    assert device_rdf(x_dev, ia, ib, box, RANGE, 75, excl=(48, 66)).sum() == 0     # one block: every pair excluded
    want = subset_counts(k, ia, ia, 75, symmetric=True, excl=(3, 3))
    assert np.array_equal(device_rdf(x_dev, ia, None, box, RANGE, 75, symmetric=True, excl=(3, 3)), want)


def test_gathered_in_place_from_a_wider_tensor_and_from_a_host_array():
    """The frames of a wider HBM tensor read where they lie (a frame stride
    past 3 n_atoms, rows picked by the index arrays), and ``InterRDF`` on the
    same data from the host."""
    import torch

    from rmsf_amd import InterRDF
    n_frames = frame_counts()[-1]
    x, _ = on_device("jittered", 130, n_frames)
    wide = torch.full((n_frames, 130 * 3 + 7), float("nan"), dtype=torch.float32, device="cuda:0")
    wide[:, :390] = torch.tensor(x.reshape(n_frames, -1), device="cuda:0")
    box = frame_boxes(n_frames)
    ia, ib = np.arange(3, 130, 2), np.arange(0, 130, 3)
    k = pair_bins(130, n_frames, True, 75)
    got = device_rdf(wide, ia, ib, box, RANGE, 75, n_atoms=130, fstride=wide.stride(0))
    assert np.array_equal(got, subset_counts(k, ia, ib, 75))
    r = InterRDF(np.asarray(x), select=ia, select_b=ib, nbins=75, range=RANGE, box=box).run().results
    assert np.array_equal(r.count_int, got)


@pytest.mark.parametrize("box", LATTICE_BOXES, ids=["free", "cubic", "ortho"])
def test_lattice_ties(box):
    x, x_dev = on_device("lattice", 3, 5)
    rows = np.arange(x.shape[1])
    for rng, nbins in LATTICE_CASES:
        want = reference(x, rows, rows, box, rng, nbins)
        assert np.array_equal(device_rdf(x_dev, None, None, box, rng, nbins), want), (rng, nbins)
        sym = device_rdf(x_dev, None, None, box, rng, nbins, symmetric=True)
        assert np.array_equal(sym, reference(x, rows, rows, box, rng, nbins, symmetric=True)), (rng, nbins)
    m = 6                                                               # rmax = L / 2: the ties of the image step
    x, x_dev = on_device("cube", m)
    rows = np.arange(m ** 3)
    want = reference(x, rows, rows, (6.0,) * 3, (0.0, 3.0), 12)
    assert want[-1] > 0 and np.array_equal(device_rdf(x_dev, None, None, (6.0,) * 3, (0.0, 3.0), 12), want)
    one = device_rdf(x_dev, np.array([17]), rows, (6.0,) * 3, (0.0, 3.0), 12)
    assert np.array_equal(one * m ** 3, want)                           # every atom: the same environment


@pytest.mark.parametrize("box", [None, (24.0, 23.0, 22.0)], ids=["free", "periodic"])
def test_non_finite_coordinates(box):
    x, x_dev = on_device("poisoned")
    rows = np.arange(x.shape[1])
    for nbins in (30, 2048):
        want = reference(x, rows, rows, box, (0.0, 9.0), nbins)
        assert np.array_equal(device_rdf(x_dev, None, None, box, (0.0, 9.0), nbins), want)
        assert np.array_equal(host_rdf(x, None, None, box, (0.0, 9.0), nbins), want)


def test_one_bin_past_two_to_the_32():
    """2,048 atoms against themselves over 1,100 frames, every distance in
    the one bin: 2048 * 2047 * 1100 = 4,611,481,600 > 2^32, the LDS counters
    flushed before any can wrap."""
    import torch
    n, n_frames = 2048, 1100
    g = torch.Generator(device="cuda:0").manual_seed(5)
    x = torch.rand((n_frames, n, 3), generator=g, device="cuda:0", dtype=torch.float32) * 40.0
    want = n * (n - 1) * n_frames
    assert want == 4_611_481_600 and want > 2 ** 32
    got = device_rdf(x, None, None, None, (0.0, 100.0), 1, symmetric=True)
    assert got.tolist() == [want]


def _expected_rdf(count, edges, n_frames, n_pairs, volume):
    norm = n_frames * (4 / 3 * np.pi * np.diff(np.power(edges, 3)))
    return count / (norm * (n_pairs / volume))


def test_interrdf_from_hbm_with_box_arrays():
    from rmsf_amd import InterRDF
    n_traj = 30
    x, x_dev = on_device("jittered", 130, n_traj)
    boxes = frame_boxes(n_traj)
    ia, ib = np.arange(0, 90), np.arange(60, 130)
    frames = np.arange(2, 30, 3)
    a = InterRDF(x_dev, select=ia, select_b=ib, nbins=40, range=RANGE, box=boxes)
    r = a.run(frames=frames).results
    want = reference(x[frames], ia, ib, boxes[frames], RANGE, 40)
    assert np.array_equal(r.count_int, want) and r.count.dtype == np.float64 and np.array_equal(r.count, want)
    assert r.n_frames == len(frames) and np.array_equal(r.frames, frames)
    e = np.linspace(*RANGE, 41)
    assert r.edges.tobytes() == e.tobytes() and np.array_equal(r.bins, 0.5 * (e[:-1] + e[1:]))
    volume = (boxes[frames, 0] * boxes[frames, 1] * boxes[frames, 2]).sum() / len(frames)
    assert r.volume == volume
    assert r.rdf.tobytes() == _expected_rdf(r.count, e, len(frames), 90 * 70, volume).tobytes()
    assert np.array_equal(a.get_cdf(), np.cumsum(r.count) / (90 * len(frames)))
    # the symmetric route, a constant [6] box, an exclusion block
    s = InterRDF(x_dev, select=ia, nbins=40, range=RANGE, box=(24.0, 23.0, 22.0, 90.0, 90.0, 90.0),
                 exclusion_block=(3, 3)).run().results
    want = reference(x, ia, ia, (24.0, 23.0, 22.0), RANGE, 40, symmetric=True, excl=(3, 3))
    assert np.array_equal(s.count_int, want)
    assert s.rdf.tobytes() == _expected_rdf(s.count, e, n_traj, 90 * 90 - 9 * 30, 24.0 * 23.0 * 22.0).tobytes()
    # free space: density, and no frames
    d = InterRDF(x_dev, select=ia, select_b=ib, nbins=40, range=RANGE, norm="density").run(step=2).results
    want = reference(x[::2], ia, ib, None, RANGE, 40)
    assert np.array_equal(d.count_int, want) and np.isnan(d.volume)
    assert d.rdf.tobytes() == (d.count / (15 * (4 / 3 * np.pi * np.diff(np.power(e, 3))))).tobytes()
    z = InterRDF(x_dev, nbins=40, range=RANGE, box=boxes).run(frames=[]).results
    assert z.n_frames == 0 and not z.count_int.any() and np.isnan(z.rdf).all()
    # a frame of the run whose box is too small for the range: refused before any launch
    small = boxes.copy()
    small[5, 1] = 2.0 * RANGE[1] - 0.01
    with pytest.raises(ValueError, match="half"):
        InterRDF(x_dev, nbins=40, range=RANGE, box=small).run()
    InterRDF(x_dev, nbins=40, range=RANGE, box=small).run(frames=[0, 1, 6])       # ... not when the frame is left out
    with pytest.raises(ValueError, match="rows"):
        InterRDF(x_dev, nbins=40, range=RANGE, box=boxes[:7]).run()
    with pytest.raises(ValueError, match="divide"):
        InterRDF(x_dev, select=ia, nbins=40, range=RANGE, norm="none", exclusion_block=(4, 4)).run()


def test_interrdf_from_an_xtc_with_its_own_boxes(tmp_path):
    from rmsf_amd import InterRDF
    from rmsf_amd.xtc import XTCFile, write_xtc
    x = jittered(100, 12)
    boxes = np.array([[22.0, 23.0, 24.0], [22.5, 23.25, 24.75], [21.9, 22.1, 23.3]])
    path = str(tmp_path / "rdf.xtc")
    for k, fr in enumerate((slice(0, 5), slice(5, 6), slice(6, 12))):
        write_xtc(path, x[fr], box=np.diag(boxes[k]), append=k > 0)
    with XTCFile(path) as fh:
        stored, file_boxes = fh.read(), fh.boxes()                     # the coordinates as the file rounds them
    assert file_boxes.shape == (12, 3) and np.abs(file_boxes[5] - boxes[1]).max() < 1e-5
    sel = np.arange(5, 95)
    r = InterRDF(path, select=sel, nbins=50, range=(0.0, 10.0), box="file").run(start=1).results
    want = reference(stored[1:], sel, sel, file_boxes[1:], (0.0, 10.0), 50, symmetric=True)
    assert np.array_equal(r.count_int, want) and want.sum() > 0
    volume = (file_boxes[1:, 0] * file_boxes[1:, 1] * file_boxes[1:, 2]).sum() / 11
    e = np.linspace(0.0, 10.0, 51)
    assert r.rdf.tobytes() == _expected_rdf(r.count, e, 11, 90 * 90 - 90, volume).tobytes()
