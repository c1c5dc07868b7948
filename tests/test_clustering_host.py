"""CPU tier of the GROMOS clustering: the library's new entry points, their
argument checks (which come before any launch), ``rmsf_cluster_gromos_host``
-- the definition in plain C++ -- against a numpy restatement of it, and what
``Cluster`` refuses without a device.

Everything after the threshold is integers: every comparison is exact."""
import ctypes

import numpy as np
import pytest

NEW_SYMBOLS = ("rmsf_adjacency_words", "rmsf_adjacency_pack", "rmsf_cluster_gromos_workspace_bytes",
               "rmsf_cluster_gromos", "rmsf_cluster_gromos_host")
CUT = 2.0


# ---- the reference: include/rmsf_hip.h's definition, restated in numpy -----------
def adjacency(d, cut):
    """bool [F, F]: d <= cut (a NaN compares false), the diagonal forced."""
    with np.errstate(invalid="ignore"):
        adj = np.asarray(d) <= cut
    adj[np.arange(len(adj)), np.arange(len(adj))] = True
    return adj


def gromos_reference(d, cut):
    """(labels, centres, sizes, tied): the clusters, and of each pick whether
    another active frame had the centre's count."""
    adj = adjacency(d, cut)
    n = len(adj)
    counts = adj.sum(1).astype(np.int64)
    active = np.ones(n, dtype=bool)
    labels = np.full(n, -1, dtype=np.int64)
    centres, sizes, tied = [], [], []
    while active.any():
        masked = np.where(active, counts, -1)
        c = int(np.argmax(masked))                       # the first maximum: the lowest index
        tied.append(int((masked == masked[c]).sum()) > 1)
        mem = adj[c] & active
        labels[mem] = len(centres)
        centres.append(c)
        sizes.append(int(mem.sum()))
        active &= ~mem
        counts -= adj[:, mem].sum(1)
    return labels, np.array(centres, dtype=np.int64), np.array(sizes, dtype=np.int64), np.array(tied)


def pack_reference(d, cut, ldw=None, poison=0):
    """(uint64 [F, ldw], int32 [F]): the bit rows and their counts; words past
    the last of a row hold ``poison``."""
    adj = adjacency(d, cut)
    n = len(adj)
    nw = (n + 63) // 64
    bits = np.zeros((n, 64 * nw), dtype=bool)
    bits[:, :n] = adj
    words = np.packbits(bits, axis=1, bitorder="little").view("<u8")
    out = np.full((n, nw if ldw is None else ldw), poison, dtype=np.uint64)
    out[:, :nw] = words
    return out, adj.sum(1).astype(np.int32)


# ---- matrices ---------------------------------------------------------------------
def points(n, k=6, seed=None):
    """Euclidean distances of n points in the plane: k centres uniform in [0,
    10 sqrt k]^2 with populations ~ 1 / (1 + index), unit normal noise, and one
    point in ten replaced by a uniform outlier in [-5, 10 sqrt k + 5]^2."""
    rng = np.random.default_rng(n if seed is None else seed)
    side = 10.0 * np.sqrt(k)
    centres = rng.uniform(0.0, side, size=(k, 2))
    w = 1.0 / (1.0 + np.arange(k))
    member = rng.choice(k, size=n, p=w / w.sum())
    x = centres[member] + rng.normal(size=(n, 2))
    out = rng.permutation(n)[: n // 10]
    x[out] = rng.uniform(-5.0, side + 5.0, size=(len(out), 2))
    return np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))


def lattice(n, seed=None, m=7):
    """L1 distances of n integer points in [0, m)^2: entries equal to the
    cutoff, duplicated frames (d = 0), tied counts."""
    rng = np.random.default_rng(n if seed is None else seed)
    x = rng.integers(0, m, size=(n, 2))
    return np.abs(x[:, None, :] - x[None, :, :]).sum(-1).astype(np.float64)


def host_cluster(d, cut, n=None, ld=None):
    """rmsf_cluster_gromos_host on d[:n, :ld-strided]."""
    from rmsf_amd import _lib
    d = np.ascontiguousarray(d, dtype=np.float64)
    n = d.shape[0] if n is None else n
    ld = d.shape[1] if ld is None else ld
    label, centre, size = (np.full(n, -7, dtype=np.int32) for _ in range(3))
    k = ctypes.c_int32(-1)
    _lib.call("rmsf_cluster_gromos_host", d.ctypes.data, n, ld, float(cut), label.ctypes.data, centre.ctypes.data,
              size.ctypes.data, ctypes.byref(k))
    return label.astype(np.int64), centre[:k.value].astype(np.int64), size[:k.value].astype(np.int64)


def assert_same(got, ref):
    for g, r, what in zip(got, ref, ("labels", "centres", "sizes")):
        assert g.shape == r.shape and np.array_equal(g, r), what


def assert_consequences(labels, centres, sizes):
    """What the definition implies, whatever the matrix."""
    assert np.all(np.diff(sizes) <= 0) and sizes.sum() == len(labels) and sizes.min() >= 1
    assert np.array_equal(np.bincount(labels, minlength=len(sizes)), sizes)
    assert np.array_equal(labels[centres], np.arange(len(centres)))
    ones = np.flatnonzero(sizes == 1)
    assert np.all(np.diff(centres[ones]) > 0)            # singletons in index order


# ---- the symbols and the two size functions ------------------------------------------
def test_library_exports_the_clustering_entry_points():
    import rmsf_amd
    from rmsf_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "Cluster" in rmsf_amd.__all__ and hasattr(rmsf_amd, "Cluster")


def test_words_and_workspace_are_functions_of_n():
    from rmsf_amd import _lib
    lib = _lib.load()
    words, wb = lib.rmsf_adjacency_words, lib.rmsf_cluster_gromos_workspace_bytes
    for n in (0, -1, -(2 ** 40)):
        assert words(n) == 0 and wb(n) == 0, n
    for n in (1, 2, 63, 64, 65, 128, 129, 4097, 100_000, 2 ** 31 - 1):
        assert words(n) == (n + 63) // 64 == words(n), n
        # at least: the working counts, the active and the member words
        assert wb(n) == wb(n) and wb(n) >= 4 * n + 16 * words(n), n
        assert wb(n) % 8 == 0
    assert wb(100_000) < 2 * 1024 * 1024                  # O(n): the bit matrix is not in it


def test_argument_checks_come_before_any_launch():
    from rmsf_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fail first
    E, M = _lib.RMSF_EINVAL, _lib.RMSF_ENOMEM
    nan, big = float("nan"), 2 ** 31

    def pack(m=one, n=100, ld=100, cutoff=1.0, adj=one, ldw=2, count=one):
        return lib.rmsf_adjacency_pack(m, n, ld, cutoff, adj, ldw, count, None)

    for kw in (dict(m=None), dict(adj=None), dict(count=None), dict(ld=99), dict(ldw=1), dict(n=0), dict(n=-5),
               dict(n=big, ld=big, ldw=big), dict(cutoff=-1e-300), dict(cutoff=-1.0), dict(cutoff=nan)):
        assert pack(**kw) == E, kw
        assert b"rmsf_adjacency_pack" in lib.rmsf_last_error(), kw

    need = lib.rmsf_cluster_gromos_workspace_bytes(100)
    kcl = ctypes.c_int32(0)

    def loop(adj=one, n=100, ldw=2, count=one, label=one, centre=one, size=one, k=ctypes.byref(kcl), work=one,
             work_bytes=need):
        return lib.rmsf_cluster_gromos(adj, n, ldw, count, label, centre, size, k, work, work_bytes, None)

    for kw in (dict(adj=None), dict(count=None), dict(label=None), dict(centre=None), dict(size=None), dict(k=None),
               dict(ldw=1), dict(n=0), dict(n=-1), dict(n=big, ldw=big)):
        assert loop(**kw) == E, kw
        assert b"rmsf_cluster_gromos" in lib.rmsf_last_error(), kw
    for kw in (dict(work=None), dict(work_bytes=need - 1), dict(work_bytes=0)):
        assert loop(**kw) == M, kw
        assert b"rmsf_cluster_gromos" in lib.rmsf_last_error() and b"workspace" in lib.rmsf_last_error(), kw

    def host(m=one, n=100, ld=100, cutoff=1.0, label=one, centre=one, size=one, k=ctypes.byref(kcl)):
        return lib.rmsf_cluster_gromos_host(m, n, ld, cutoff, label, centre, size, k)

    for kw in (dict(m=None), dict(label=None), dict(centre=None), dict(size=None), dict(k=None), dict(ld=99),
               dict(n=0), dict(n=-1), dict(n=big, ld=big), dict(cutoff=-1.0), dict(cutoff=nan)):
        assert host(**kw) == E, kw
        assert b"rmsf_cluster_gromos_host" in lib.rmsf_last_error(), kw


# ---- rmsf_cluster_gromos_host against the reference ------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 1000])
def test_host_points(n):
    d = points(n)
    ref = gromos_reference(d, CUT)
    if n >= 63:  # the general loop and the singleton tail are both exercised
        assert (ref[2] >= 2).sum() >= 3 and (ref[2] == 1).sum() >= 1
    got = host_cluster(d, CUT)
    assert_same(got, ref)
    assert_consequences(*got)


@pytest.mark.parametrize("n", [65, 300, 1000])
def test_host_lattice(n):
    d = lattice(n)
    ref = gromos_reference(d, CUT)
    assert ref[3].any() and (d == CUT).sum() > 0 and len(ref[1]) >= 2   # tied picks, entries equal to the cutoff
    got = host_cluster(d, CUT)
    assert_same(got, ref)
    assert_consequences(*got)


def test_host_cutoff_zero_and_above_everything():
    d = points(130)
    assert d[~np.eye(130, dtype=bool)].min() > 0.0        # distinct points
    labels, centres, sizes = host_cluster(d, 0.0)
    assert np.array_equal(labels, np.arange(130)) and np.array_equal(centres, np.arange(130))
    assert np.array_equal(sizes, np.ones(130, dtype=np.int64))
    assert_same((labels, centres, sizes), gromos_reference(d, 0.0))
    for cut in (float(d.max()) + 1.0, float("inf")):
        labels, centres, sizes = host_cluster(d, cut)
        assert not labels.any() and centres.tolist() == [0] and sizes.tolist() == [130]
        assert_same((labels, centres, sizes), gromos_reference(d, cut))


def nan_case(n=130, q=37):
    """(d with frame q's row, column and diagonal NaN, the matrix without q)."""
    d = points(n)
    keep = np.arange(n) != q
    small = d[np.ix_(keep, keep)].copy()
    d = d.copy()
    d[q, :] = np.nan
    d[:, q] = np.nan
    return d, small, q, keep


def assert_nan_frame_alone(got, small_ref, q, keep):
    labels, centres, sizes = got
    lq = labels[q]
    assert sizes[lq] == 1 and centres[lq] == q and (labels == lq).sum() == 1
    rest = labels[keep]
    rest = rest - (rest > lq)                             # renumbered without q's cluster
    assert np.array_equal(rest, small_ref[0])
    assert np.array_equal(np.delete(sizes, lq), small_ref[2])
    c = np.delete(centres, lq)
    assert np.array_equal(c - (c > q), small_ref[1])


def test_host_nan_row_and_column():
    d, small, q, keep = nan_case()
    ref_small = gromos_reference(small, CUT)
    assert (ref_small[2] >= 2).sum() >= 3 and (ref_small[2] == 1).sum() >= 1
    got = host_cluster(d, CUT)
    assert_same(got, gromos_reference(d, CUT))
    assert_nan_frame_alone(got, ref_small, q, keep)


def test_host_padded_matrix():
    n = 130
    d = points(n)
    padded = np.zeros((n, n + 3))                        # the padding would be everybody's neighbour
    padded[:, :n] = d
    ref = gromos_reference(d, CUT)
    assert (ref[2] >= 2).sum() >= 3
    assert_same(host_cluster(padded, CUT, n=n, ld=n + 3), ref)


def test_pack_reference_bit_order():
    """The reference of the pack (used by the GPU tier): bit j & 63 of word j // 64."""
    d = np.full((70, 70), 9.0)
    d[3, 5] = d[3, 64] = d[3, 69] = 1.0
    words, counts = pack_reference(d, CUT, ldw=3, poison=2 ** 64 - 1)
    assert words[3, 0] == (1 << 3) | (1 << 5) and words[3, 1] == (1 << 0) | (1 << 5) and words[3, 2] == 2 ** 64 - 1
    assert counts[3] == 4 and counts[0] == 1 and words[69, 1] == 1 << 5 and words[69, 0] == 0


# ---- Cluster: what is decided without a device ----------------------------------------
def test_cluster_refusals_without_a_device():
    from rmsf_amd import Cluster
    from rmsf_amd.sources import DeviceSource
    x = np.zeros((6, 5, 3), np.float32)
    d = lattice(20)
    with pytest.raises(TypeError):
        Cluster(d)                                        # cutoff is required
    with pytest.raises(TypeError):
        Cluster(d, 1.5)                                   # and keyword-only
    for bad in (-1.0, -1e-300, float("nan")):
        with pytest.raises(ValueError, match="cutoff"):
            Cluster(d, cutoff=bad)
    with pytest.raises(ValueError, match="method"):
        Cluster(d, cutoff=1.0, method="dbscan")
    with pytest.raises(ValueError, match="square"):
        Cluster(np.zeros((4, 5)), cutoff=1.0)
    with pytest.raises(ValueError, match="layout"):
        Cluster(x, cutoff=1.0, layout="aos")
    lop = d.copy()
    lop[2, 7], lop[7, 2] = 1.0, 3.0                       # neighbours one way only
    with pytest.raises(ValueError, match="not symmetric"):
        Cluster(lop, cutoff=2.0).run()
    with pytest.raises(NotImplementedError, match="one device"):
        Cluster(x, cutoff=1.0, gpus=2).run()
    with pytest.raises(NotImplementedError, match="one device"):
        Cluster([x, x], cutoff=1.0).run()
    planes = object.__new__(DeviceSource)                 # HBM-resident [F, 3, n_atoms]; no tensor needed
    planes.layout, planes.n_sel = "soa", 5
    with pytest.raises(NotImplementedError, match='layout="fac"'):
        Cluster(planes, cutoff=1.0).run()
    with pytest.raises(ValueError, match="at least 3"):
        Cluster(x, cutoff=1.0, select=[0, 4]).run()       # DistanceMatrix's own refusals, in its words
    with pytest.raises(ValueError, match="weights"):
        Cluster(x, cutoff=1.0, weights=np.ones(4)).run()


def test_script_cluster_options_go_together():
    """rmsf_mi355x.py --cluster / --cluster-cutoff: refused alone, before any device work."""
    import subprocess
    import sys

    from conftest import ROOT
    script = f"{ROOT}/mdanalysis-mpi_amd/rmsf_mi355x.py"
    for extra, msg in ((["--cluster", "x.npy"], "go together"), (["--cluster-cutoff", "1.5"], "go together"),
                       (["--cluster", "x.npy", "--cluster-cutoff", "-1"], ">= 0")):
        r = subprocess.run([sys.executable, script, "--synthetic", "10", "5", *extra], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and msg in r.stderr, (extra, r.stderr[-500:])
