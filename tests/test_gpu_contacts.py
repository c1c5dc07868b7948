"""GPU tier of the contact kernels (csrc/contacts.hip): ``rmsf_contact_counts``
and ``rmsf_contact_fraction`` through ``Engine``, and ``ContactMap`` and
``Contacts`` end to end, against the numpy restatement of the definition in
tests/test_contacts_host.py and against the library's ``_host`` entries.

After one comparison everything is integers: counts, ``n_contacts`` and the
hard-cut q are compared for equality.  soft_cut is within the derived bound
``(P + 8) 2^-53`` relative of the restatement summed by ``math.fsum`` (see
test_contacts_host.py) and bit-identical on a second run.

The shapes stand on the launcher's own plan (``rmsf_contact_counts_plan``):
tile edges T, frame chunk C and a frame count it splits, not on a workload."""
import functools

import numpy as np
import pytest

from test_contacts_host import (SOFT, assert_poison_is_local, bits, counts_reference, fraction_reference, host_counts,
                                host_fraction, jittered, lattice, natives, poisoned, soft_bound)

pytestmark = pytest.mark.gpu

POISON = -7
RADIUS = 6.0
METHOD = {"hard_cut": 0, "radius_cut": 1, "soft_cut": 2}


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
    _lib.call("rmsf_contact_counts_plan", n_a, n_b, n_frames, int(symmetric), *(ctypes.byref(t) for t in v))
    return tuple(t.value for t in v)


@functools.lru_cache(maxsize=None)
def on_device(kind, *args):
    import torch
    x = {"jittered": jittered, "lattice": lattice, "poisoned": lambda *a: poisoned(*a)[1],
         "clean": lambda *a: poisoned(*a)[0]}[kind](*args)
    return x, torch.tensor(x, device="cuda:0")


def device_counts(x_dev, ia, ib, radius, symmetric=False, pad=3):
    """Engine.contact_counts into a poison-filled [n_a, n_b + pad] buffer,
    twice: the same bytes, the poison past n_b intact.  int64 [n_a, n_b]."""
    import torch
    n_frames, n_atoms = x_dev.shape[:2]
    n_a = n_atoms if ia is None else len(ia)
    n_b = n_a if symmetric else (n_atoms if ib is None else len(ib))
    runs = []
    for _ in range(2):
        out = torch.full((n_a, n_b + pad), POISON, dtype=torch.int32, device="cuda:0")
        got = engine().contact_counts(x_dev.data_ptr(), x_dev.stride(0), n_frames, n_atoms, ia, n_a, ib, n_b, radius,
                                      symmetric=symmetric, out=out)
        torch.cuda.synchronize()
        assert got.shape == (n_a, n_b) and got.data_ptr() == out.data_ptr()
        runs.append(out.cpu().numpy())
    assert runs[0].tobytes() == runs[1].tobytes()                      # a second run: the same bytes
    assert (runs[0][:, n_b:] == POISON).all()                          # nothing written past n_b
    assert (runs[0][:, :n_b] >= 0).all() and (runs[0][:, :n_b] <= n_frames).all()   # every entry written
    return runs[0][:, :n_b].astype(np.int64)


def edges():
    tile_a, tile_b, chunk, _ = plan(200, 200, 64)
    return tile_a, tile_b, chunk


def sizes(t):
    return sorted({1, t - 1, t, t + 1, 2 * t + 2} - {0})


def frame_counts():
    c = edges()[2]
    split = 2 * c + 3                                                  # more than one split, the last a partial chunk
    return sorted({1, c - 1, c, c + 1} - {0}) + [split]


def test_the_plan_is_not_trivial():
    """The cases below stand on real edges: more than one tile a side, more
    than one split with a ragged end, symmetric and rectangular runs."""
    ta, tb, c = edges()
    assert max(sizes(ta)) > ta and max(sizes(tb)) > tb                  # two tiles a side and a partial third
    split = frame_counts()[-1]
    for sym in (False, True):
        n_splits = plan(max(sizes(ta)), max(sizes(ta)) if sym else max(sizes(tb)), split, sym)[3]
        assert n_splits > 1 and (split % c or split % n_splits)
        assert plan(1, 1, split, sym)[3] > 1
    assert plan(1, 1, 1)[3] == 1 and c > 1
    assert plan(3341, 3341, 4096, True)[:3] == (ta, tb, c)               # the plan's edges do not move with the shape
    assert engine().contact_counts_plan(3341, 3341, 4096, True) == plan(3341, 3341, 4096, True)


@pytest.mark.parametrize("n_frames", frame_counts())
def test_counts_at_the_plan_edges(n_frames):
    ta, tb, _ = edges()
    n = max(sizes(ta) + sizes(tb))
    x, x_dev = on_device("jittered", n, n_frames)
    rows = np.arange(n)
    ref = counts_reference(x, rows, rows, RADIUS)
    assert np.array_equal(host_counts(x, None, None, RADIUS), ref)
    if n_frames > 2:
        assert ((ref > 0) & (ref < n_frames)).mean() > 0.1              # the comparison decides
    for n_a in sizes(ta):
        ia = np.arange(n_a)
        for n_b in sizes(tb):
            ib = np.arange(n - n_b, n)                                  # the other end: A is not B
            got = device_counts(x_dev, ia, ib, RADIUS)
            assert np.array_equal(got, ref[np.ix_(ia, ib)]), (n_a, n_b)
        sym = device_counts(x_dev, ia, None, RADIUS, symmetric=True)
        assert np.array_equal(sym, ref[np.ix_(ia, ia)]), n_a
        assert np.array_equal(sym, device_counts(x_dev, ia, ia, RADIUS)), n_a   # the rectangular route on A = B
    # dense rows: no index array at all
    assert np.array_equal(device_counts(x_dev, None, None, RADIUS), ref)
    assert np.array_equal(device_counts(x_dev, None, None, RADIUS, symmetric=True), ref)


def test_counts_many_splits_and_a_permuted_selection():
    """A run long enough that every split has several chunks, rows out of order
    and repeated."""
    _, _, c = edges()
    n_frames = 40 * c + 5
    x, x_dev = on_device("jittered", 70, n_frames)
    assert plan(70, 70, n_frames)[3] > 1
    rng = np.random.default_rng(11)
    ia, ib = rng.permutation(70)[:50], rng.integers(0, 70, 66)
    ref = counts_reference(x, np.arange(70), np.arange(70), RADIUS)
    assert np.array_equal(device_counts(x_dev, ia, ib, RADIUS), ref[np.ix_(ia, ib)])
    assert np.array_equal(device_counts(x_dev, ia, None, RADIUS, symmetric=True), ref[np.ix_(ia, ia)])


def test_counts_lattice_ties():
    x, x_dev = on_device("lattice")
    rows = np.arange(x.shape[1])
    ref = counts_reference(x, rows, rows, 3.0)
    assert np.array_equal(device_counts(x_dev, None, None, 3.0, symmetric=True), ref)
    assert np.array_equal(device_counts(x_dev, None, None, 3.0), ref)
    below = device_counts(x_dev, None, None, float(np.nextafter(3.0, 0.0)))
    assert np.array_equal(below, counts_reference(x, rows, rows, np.nextafter(3.0, 0.0))) and below.sum() < ref.sum()


def test_counts_with_nan_and_inf():
    (clean, clean_dev), (bad, bad_dev) = on_device("clean"), on_device("poisoned")
    rows = np.arange(clean.shape[1])
    for sym in (False, True):
        got = device_counts(bad_dev, None, None, RADIUS, symmetric=sym)
        assert np.array_equal(got, counts_reference(bad, rows, rows, RADIUS))
        assert np.array_equal(got, host_counts(bad, None, None, RADIUS))
        assert_poison_is_local(got, device_counts(clean_dev, None, None, RADIUS, symmetric=sym), clean, RADIUS)


# ---- selections and residency ------------------------------------------------------------
def test_contact_map_selections_and_residency():
    import torch

    from rmsf_amd import ContactMap
    x, x_dev = on_device("jittered", 300, 24)
    rng = np.random.default_rng(4)
    sel_a = np.sort(rng.permutation(300)[:40])
    sel_b = np.concatenate([sel_a[:15], rng.permutation(300)[:55]])     # overlapping, unsorted, 70 atoms
    ref = counts_reference(x, sel_a, sel_b, RADIUS)
    ref_step = counts_reference(x[1:23:2], sel_a, sel_b, RADIUS)
    runs = {"HBM in place": x_dev, "host array": np.array(x), "host tensor": torch.tensor(x)}
    for name, inp in runs.items():
        r = ContactMap(inp, radius=RADIUS, select=sel_a, select_b=sel_b).run().results
        assert r.counts.dtype == np.int64 and np.array_equal(r.counts, ref), name
        assert r.n_frames == 24 and np.array_equal(r.frames, np.arange(24))
        assert np.array_equal(r.frequency, ref / 24.0)
        r = ContactMap(inp, radius=RADIUS, select=sel_a, select_b=sel_b).run(1, 23, 2).results
        assert np.array_equal(r.counts, ref_step) and np.array_equal(r.frames, np.arange(1, 23, 2)), name
    # a scattered frame list: the dense copy even from HBM
    frames = [0, 1, 5, 6, 17]
    r = ContactMap(x_dev, radius=RADIUS, select=sel_a, select_b=sel_b).run(frames=frames).results
    assert np.array_equal(r.counts, counts_reference(x[frames], sel_a, sel_b, RADIUS))
    # one selection against itself, every atom, a prefix of the atoms, a wide tensor's leading atoms
    sym = ContactMap(x_dev, radius=RADIUS, select=sel_b).run().results.counts
    assert np.array_equal(sym, counts_reference(x, sel_b, sel_b, RADIUS)) and np.array_equal(sym, sym.T)
    every = ContactMap(x_dev, radius=RADIUS).run().results.counts
    assert np.array_equal(every, counts_reference(x, np.arange(300), np.arange(300), RADIUS))
    dense = ContactMap(x_dev[:, :70].contiguous(), radius=RADIUS).run().results.counts
    assert np.array_equal(dense, every[:70, :70])
    assert np.array_equal(ContactMap(x_dev, radius=RADIUS, select=np.arange(70)).run().results.counts, dense)
    assert np.array_equal(ContactMap(x_dev, radius=RADIUS, select_b=sel_a).run().results.counts, every[:, sel_a])
    with pytest.raises(IndexError):
        ContactMap(x_dev, select=[0, 300]).run()
    empty = ContactMap(x_dev, select=sel_a).run(5, 5).results
    assert empty.n_frames == 0 and not empty.counts.any() and np.isnan(empty.frequency).all()


# ---- the fraction kernel -----------------------------------------------------------------
def device_fraction(x_dev, ra, rb, r0, radius, method, rows=None):
    """Engine.contact_fraction, twice: (q, n_contacts int64) and the same bytes."""
    import torch
    n_frames, n_atoms = x_dev.shape[:2]
    runs = []
    for _ in range(2):
        q, n = engine().contact_fraction(x_dev.data_ptr(), x_dev.stride(0), n_frames, n_atoms, rows,
                                         n_atoms if rows is None else len(rows), ra, rb, r0, radius, METHOD[method],
                                         **SOFT)
        torch.cuda.synchronize()
        runs.append((q.cpu().numpy(), n.cpu().numpy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    return runs[0][0], runs[0][1].astype(np.int64)


def check_fraction(x, x_dev, ra, rb, r0, radius, rows=None, reference_frame=True):
    pa, pb = (ra, rb) if rows is None else (np.asarray(rows)[ra], np.asarray(rows)[rb])
    for method in ("hard_cut", "radius_cut", "soft_cut"):
        q_ref, n_ref = fraction_reference(x, pa, pb, r0, radius, method, **SOFT)
        q, n = device_fraction(x_dev, ra, rb, r0, radius, method, rows=rows)
        assert np.array_equal(n, n_ref), method
        if method == "soft_cut":
            assert (np.abs(q - q_ref) <= soft_bound(len(ra)) * q_ref).all(), np.abs(q / q_ref - 1).max()
        else:
            assert np.array_equal(bits(q), bits(q_ref)), method
            q_host, n_host = host_fraction(x, ra, rb, r0, radius, method, rows=rows)
            assert np.array_equal(bits(q), bits(q_host)) and np.array_equal(n, n_host)
            if reference_frame:
                assert q[0] == 1.0 and n[0] == len(ra)


@pytest.mark.parametrize("n_frames", [1, 2, 65])
@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 257, 1000, 1025])
def test_fraction(n_pairs, n_frames):
    """1025 pairs: past the wave-a-frame path, the workgroup a frame."""
    x, x_dev = on_device("jittered", 130, 65)
    rows = np.arange(130)
    ra, rb, r0 = natives(x[0], rows, rows, RADIUS)
    assert len(ra) >= 1025
    keep = np.linspace(0, len(ra) - 1, n_pairs).astype(np.int64) if n_pairs > 1 else np.array([len(ra) // 2])
    check_fraction(x[:n_frames], x_dev[:n_frames], ra[keep], rb[keep], r0[keep], RADIUS)


def test_fraction_paths_by_the_staged_rows():
    """The three kernels: four frames' rows in LDS, one frame's, and rows too
    many for LDS read from where they lie -- dense and through an index array."""
    x, x_dev = on_device("jittered", 5200, 5)
    near = np.arange(0, 5200, 40)
    ra, rb, r0 = natives(x[0], near, near, RADIUS)
    assert len(ra) > 1024
    check_fraction(x, x_dev, ra, rb, r0, RADIUS)                        # 5,200 dense rows: not staged
    rows = np.arange(5199, -1, -1)                                     # ... through an index array
    check_fraction(x, x_dev, 5199 - ra, 5199 - rb, r0, RADIUS, rows=rows)
    rows = np.arange(1500) * 3                                         # 1,500 rows: one frame in LDS, not four
    inside = (ra % 3 == 0) & (rb % 3 == 0) & (ra < 4500) & (rb < 4500)
    assert 20 < inside.sum() <= 1024                                   # (few pairs, and still not four frames)
    check_fraction(x, x_dev, ra[inside] // 3, rb[inside] // 3, r0[inside], RADIUS, rows=rows)
    rows = near[::-1].copy()                                           # 130 rows: four frames in LDS
    pos = {int(r): k for k, r in enumerate(rows)}
    few = np.arange(0, len(ra), 3)
    assert len(few) <= 1024
    check_fraction(x, x_dev, np.array([pos[int(r)] for r in ra[few]]), np.array([pos[int(r)] for r in rb[few]]),
                   r0[few], RADIUS, rows=rows, reference_frame=True)


def test_fraction_on_lattice_ties_and_non_finite_frames():
    x, x_dev = on_device("lattice")
    rows = np.arange(x.shape[1])
    ra, rb, r0 = natives(x[0], rows, rows, 3.0)
    check_fraction(x, x_dev, ra, rb, r0, 3.0)
    (clean, _), (bad, bad_dev) = on_device("clean"), on_device("poisoned")
    rows = np.arange(bad.shape[1])
    ra, rb, r0 = natives(bad[0], rows, rows, RADIUS)
    for method in ("hard_cut", "soft_cut"):
        q, n = device_fraction(bad_dev, ra, rb, r0, RADIUS, method)
        q_ref, n_ref = fraction_reference(bad, ra, rb, r0, RADIUS, method, **SOFT)
        assert np.array_equal(n, n_ref)
        n_clean = fraction_reference(clean, ra, rb, r0, RADIUS, method, **SOFT)[1]
        differ = np.nonzero(n != n_clean)[0]
        assert set(differ) == {3, 7} and (n[differ] < n_clean[differ]).all()   # the two frames with a bad coordinate
        if method == "hard_cut":
            assert np.array_equal(bits(q), bits(q_ref))
        else:
            # a bad atom's pair with itself is a native one and its distance NaN (inf - inf): the formula as
            # written makes those two frames' soft q NaN, as numpy's
            assert np.isnan(q[[3, 7]]).all() and np.isnan(q_ref[[3, 7]]).all()
            ok = ~np.isin(np.arange(len(q)), (3, 7))
            assert (np.abs(q[ok] - q_ref[ok]) <= soft_bound(len(ra)) * q_ref[ok]).all()


# ---- the two classes ---------------------------------------------------------------------
def test_contacts_and_contact_map_agree():
    """ContactMap's counts at the native pairs are the frames in which
    Contacts counts that pair, and their sum is n_contacts' sum."""
    from rmsf_amd import ContactMap, Contacts
    x, x_dev = on_device("jittered", 130, 65)
    sel_a, sel_b = np.arange(0, 80), np.arange(50, 130)
    c = Contacts(x_dev, select=sel_a, select_b=sel_b, radius=RADIUS).run().results
    m = ContactMap(x_dev, select=sel_a, select_b=sel_b, radius=RADIUS).run().results
    at_pairs = m.counts[c.pairs[:, 0], c.pairs[:, 1]]
    assert len(c.pairs) > 100 and c.n_contacts.sum() == at_pairs.sum()
    for p in np.linspace(0, len(c.pairs) - 1, 12).astype(int):
        i, j = c.pairs[p]
        one = Contacts(x_dev, select=sel_a, select_b=sel_b, radius=RADIUS, pairs=([i], [j])).run().results
        assert one.n_contacts.sum() == at_pairs[p] and one.r0[0] == c.r0[p]
        assert set(one.n_contacts) <= {0, 1} and np.array_equal(one.q, one.n_contacts.astype(np.float64))


def contacts_reference(x, sel_a, sel_b, radius, method, frames, reference=0):
    ref = x[reference] if isinstance(reference, int) else reference
    ra, rb, r0 = natives(ref, sel_a, sel_b, radius)
    q, n = fraction_reference(x[frames], ra, rb, r0, radius, method, **SOFT)
    pos_a = {int(a): k for k, a in enumerate(sel_a)}
    pos_b = {int(b): k for k, b in enumerate(sel_b)}
    pairs = np.array([[pos_a[int(a)], pos_b[int(b)]] for a, b in zip(ra, rb)], dtype=np.int64)
    return q, n, pairs, r0


def assert_contacts(r, want, frames, method):
    q, n, pairs, r0 = want
    assert np.array_equal(r.pairs, pairs) and r.pairs.dtype == np.int64
    assert np.array_equal(bits(r.r0), bits(r0))
    assert np.array_equal(r.n_contacts, n) and r.n_contacts.dtype == np.int64
    if method == "soft_cut":
        assert (np.abs(r.q - q) <= soft_bound(len(pairs)) * q).all()
    else:
        assert np.array_equal(bits(r.q), bits(q))
    assert r.timeseries.shape == (len(frames), 2) and np.array_equal(r.timeseries[:, 0], np.asarray(frames, float))
    assert np.array_equal(bits(r.timeseries[:, 1]), bits(r.q)) and r.n_frames == len(frames)


def test_contacts_and_contact_map_end_to_end(tmp_path):
    """From a host array, an HBM tensor and an .xtc file, against the
    restatement on the decoded coordinates."""
    import torch

    from rmsf_amd import ContactMap, Contacts
    from rmsf_amd.xtc import XTCFile, write_xtc
    path = str(tmp_path / "traj.xtc")
    write_xtc(path, jittered(300, 24))
    with XTCFile(path) as f:
        x = f.read()
    assert x.shape == (24, 300, 3) and x.dtype == np.float32
    rng = np.random.default_rng(8)
    sel_a, sel_b = np.sort(rng.permutation(300)[:60]), rng.permutation(300)[:90]
    inputs = {"host array": x, "HBM tensor": torch.tensor(x, device="cuda:0"), "xtc": path}
    every, stepped = list(range(24)), list(range(2, 20, 3))
    want_map = counts_reference(x, sel_a, sel_b, RADIUS)
    for name, inp in inputs.items():
        kw = {"batch_frames": 7} if name != "HBM tensor" else {}
        m = ContactMap(inp, radius=RADIUS, select=sel_a, select_b=sel_b, **kw).run().results
        assert np.array_equal(m.counts, want_map) and m.n_frames == 24, name
        for method in ("hard_cut", "radius_cut", "soft_cut"):
            r = Contacts(inp, select=sel_a, select_b=sel_b, radius=RADIUS, method=method, **SOFT, **kw).run().results
            assert_contacts(r, contacts_reference(x, sel_a, sel_b, RADIUS, method, every), every, method)
            if method != "soft_cut":
                assert r.q[0] == 1.0                                    # the reference frame
        r = Contacts(inp, select=sel_a, select_b=sel_b, radius=RADIUS, reference=5, **kw).run(2, 20, 3).results
        assert_contacts(r, contacts_reference(x, sel_a, sel_b, RADIUS, "hard_cut", stepped, reference=5), stepped,
                        "hard_cut")
        assert r.q[1] == 1.0                                            # frame 5 is the second of the run
        # the reference as an array of every atom; one selection against itself
        r = Contacts(inp, select=sel_a, radius=RADIUS, reference=x[3], **kw).run().results
        assert_contacts(r, contacts_reference(x, sel_a, sel_a, RADIUS, "hard_cut", every, reference=3), every,
                        "hard_cut")
    hbm = inputs["HBM tensor"]
    with pytest.raises(ValueError, match="no pair"):
        Contacts(hbm, select=[0], select_b=[1], radius=1e-3).run()
    with pytest.raises(ValueError, match="reference has"):
        Contacts(hbm, select=sel_a, reference=x[0, :100]).run()
    with pytest.raises(IndexError, match="pairs index"):
        Contacts(hbm, select=sel_a, pairs=([0], [60])).run()


def test_script_writes_the_map_and_q(tmp_path):
    """rmsf_mi355x.py --synthetic --contact-map --contacts: the files hold what the classes give."""
    import os
    import subprocess
    import sys

    from conftest import ROOT
    out_map, out_q = str(tmp_path / "map.npy"), str(tmp_path / "q.npy")
    r = subprocess.run([sys.executable, f"{ROOT}/mdanalysis-mpi_amd/rmsf_mi355x.py", "--synthetic", "90", "20",
                        "--align", "none", "--contact-map", out_map, "--contacts", out_q, "--contact-radius", "8",
                        "--contacts-method", "soft_cut"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ))
    assert r.returncode == 0, r.stderr[-800:]
    counts, ts = np.load(out_map), np.load(out_q)
    assert counts.shape == (90, 90) and counts.dtype == np.int64 and np.array_equal(counts, counts.T)
    assert (np.diag(counts) == 20).all() and ts.shape == (20, 2) and np.array_equal(ts[:, 0], np.arange(20.0))
    assert (ts[:, 1] > 0).all() and (ts[:, 1] <= 1).all()
    assert "contact map at 8.0 A over 20 frames" in r.stdout and "native contacts at 8.0 A" in r.stdout
