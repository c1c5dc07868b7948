"""CPU tier of DBSCAN (csrc/dbscan.hip): the library's entry points, their
argument checks (which come before any launch), ``rmsf_cluster_dbscan_host``
-- the definition in plain C++ -- against a numpy restatement of it and
against scikit-learn where that is installed, what ``DBSCAN`` refuses without
a device, and the script's option errors.

The definition (include/rmsf_hip.h): ``adj = d <= eps`` with the diagonal set
and a NaN never a neighbour, ``core = count >= min_samples``, the clusters are
the connected components of adj on core x core numbered by their lowest core
index, a non-core row takes the lowest id among its core neighbours' clusters,
every other row is -1.  Everything after the threshold is integers: every
comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest

from test_clustering_host import CUT, adjacency, lattice, nan_case, points

NEW_SYMBOLS = ("rmsf_cluster_dbscan_workspace_bytes", "rmsf_cluster_dbscan", "rmsf_cluster_dbscan_host")
SIZES = [1, 2, 63, 64, 65, 130, 1000]
MIN_SAMPLES = [1, 2, 4, 8]


# ---- the reference: the definition, restated in numpy --------------------------------
def dbscan_reference(d, eps, min_samples):
    """(labels int64 [n], core rows int64, n_clusters, rounds): plain
    min-propagation to a fixpoint -- every core row takes the lowest label among
    its core neighbours (itself among them), all rows at once, until a round
    changes nothing; ``rounds`` counts that last round too."""
    adj = adjacency(d, eps)
    n = len(adj)
    core = adj.sum(1) >= min_samples
    rows, cols = np.nonzero(adj & core[:, None] & core[None, :])      # row-major: each core row's run of columns
    core_rows = np.flatnonzero(core)
    starts = np.searchsorted(rows, core_rows)                          # (every core row has its diagonal)
    low = np.arange(n, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        new = low.copy()
        if len(core_rows):
            new[core_rows] = np.minimum.reduceat(low[cols], starts)
        if np.array_equal(new, low):
            break
        low = new
    roots = np.flatnonzero(core & (low == np.arange(n)))               # each cluster's lowest core index
    labels = np.full(n, -1, dtype=np.int64)
    labels[core] = np.searchsorted(roots, low[core])
    near = adj & core[None, :]
    border = ~core & near.any(1)
    labels[border] = np.where(near[border], labels[None, :], n).min(1)
    return labels, core_rows.astype(np.int64), len(roots), rounds


# ---- matrices ---------------------------------------------------------------------
def chain(n, shuffled):
    """|x_i - x_j| with x a permutation of 0..n-1: a path at eps = 1."""
    x = np.random.default_rng(n).permutation(n) if shuffled else np.arange(n)
    return np.abs(x[:, None] - x[None, :]).astype(np.float64)


def touching(n, gap=4.0):
    """Euclidean distances of n points in five unit blobs `gap` apart on a line:
    neighbouring blobs' fringes meet, so border rows see several clusters."""
    rng = np.random.default_rng(n)
    member = rng.integers(0, 5, n)
    x = np.stack([gap * member, np.zeros(n)], 1) + rng.normal(size=(n, 2))
    return np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))


TOUCHING = {130: (1.0, 6), 1000: (0.6, 6)}                             # n -> (eps, min_samples)
CHAIN_EPS, CHAIN_M = 1.0, 3


@functools.lru_cache(maxsize=None)
def matrix(kind: str, n: int):
    """(matrix, eps) of a named case; computed once, read-only."""
    if kind == "points":
        d, eps = points(n), CUT
    elif kind == "lattice":
        d, eps = lattice(n), CUT
    elif kind in ("chain", "chain_shuffled"):
        d, eps = chain(n, kind == "chain_shuffled"), CHAIN_EPS
    elif kind == "touching":
        d, eps = touching(n), TOUCHING[n][0]
    elif kind == "zero":
        d, eps = points(n), 0.0
    elif kind == "inf":
        d, eps = points(n), float("inf")
    elif kind == "nan":
        d, eps = nan_case(n)[0], CUT
    d.setflags(write=False)
    return d, eps


@functools.lru_cache(maxsize=None)
def reference(kind: str, n: int, m: int):
    """The restatement's (labels, core rows, n_clusters, rounds) of a named case; read-only."""
    d, eps = matrix(kind, n)
    ref = dbscan_reference(d, eps, m)
    ref[0].setflags(write=False)
    ref[1].setflags(write=False)
    return ref


def core_rows_of(words, n):
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n]).astype(
        np.int64)


def host_dbscan(d, eps, m, n=None, ld=None):
    """rmsf_cluster_dbscan_host on d[:n, :ld-strided] -> (labels int64, core rows int64, n_clusters)."""
    from rmsf_amd import _lib
    d = np.ascontiguousarray(d, dtype=np.float64)
    n = d.shape[0] if n is None else n
    ld = d.shape[1] if ld is None else ld
    label = np.full(n, -7, dtype=np.int32)
    core = np.full((n + 63) // 64, 2 ** 64 - 1, dtype=np.uint64)
    k = ctypes.c_int32(-1)
    _lib.call("rmsf_cluster_dbscan_host", d.ctypes.data, n, ld, float(eps), int(m), label.ctypes.data,
              core.ctypes.data, ctypes.byref(k))
    if n % 64:
        assert not int(core[-1]) >> (n % 64)                           # bits at or past n are zero
    return label.astype(np.int64), core_rows_of(core, n), k.value


def assert_same(got, ref):
    for g, r, what in zip(got[:2], ref[:2], ("labels", "core rows")):
        assert g.shape == r.shape and np.array_equal(g, r), what
    assert got[2] == ref[2], "n_clusters"


def assert_consequences(d, eps, m, labels, core_rows, n_clusters):
    """What the definition implies, whatever the matrix."""
    adj = adjacency(d, eps)
    n = len(adj)
    core = np.zeros(n, dtype=bool)
    core[core_rows] = True
    assert np.array_equal(core, adj.sum(1) >= m)
    assert labels.min() >= -1 and labels.max() == n_clusters - 1
    assert (labels[core] >= 0).all()
    firsts = [np.flatnonzero(core & (labels == k))[0] for k in range(n_clusters)]
    assert np.all(np.diff(firsts) > 0)                                 # numbered by the lowest core index
    i, j = np.nonzero(adj & core[:, None] & core[None, :])
    assert np.array_equal(labels[i], labels[j])                        # core neighbours share a cluster
    noise = labels < 0
    assert not (adj[noise] & core[None, :]).any()                      # noise has no core neighbour


# ---- the symbols and the size function ------------------------------------------------
def test_library_exports_the_dbscan_entry_points():
    import rmsf_amd
    from rmsf_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "DBSCAN" in rmsf_amd.__all__ and hasattr(rmsf_amd, "DBSCAN")


def test_workspace_is_a_function_of_n():
    from rmsf_amd import _lib
    wb = _lib.load().rmsf_cluster_dbscan_workspace_bytes
    for n in (0, -1, -(2 ** 40), 2 ** 31):
        assert wb(n) == 0, n
    for n in (1, 2, 63, 64, 65, 128, 129, 4097, 100_000, 2 ** 31 - 1):
        assert wb(n) == wb(n) and wb(n) >= 8 * n, n                    # at least: two parent arrays
        assert wb(n) % 8 == 0
        assert wb(n) <= 64 * n + 4096, n                               # O(n): the bit matrix is not in it
    assert wb(100_000) < 2 * 1024 * 1024


def test_argument_checks_come_before_any_launch():
    from rmsf_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fail first
    E, M = _lib.RMSF_EINVAL, _lib.RMSF_ENOMEM
    nan, big = float("nan"), 2 ** 31
    need = lib.rmsf_cluster_dbscan_workspace_bytes(100)
    kcl, rounds = ctypes.c_int32(0), ctypes.c_int32(0)

    def loop(adj=one, n=100, ldw=2, count=one, m=5, label=one, core=one, k=ctypes.byref(kcl),
             r=ctypes.byref(rounds), work=one, work_bytes=need):
        return lib.rmsf_cluster_dbscan(adj, n, ldw, count, m, label, core, k, r, work, work_bytes, None)

    for kw in (dict(adj=None), dict(count=None), dict(label=None), dict(core=None), dict(k=None), dict(r=None),
               dict(ldw=1), dict(n=0), dict(n=-1), dict(n=big, ldw=big), dict(m=0), dict(m=-3)):
        assert loop(**kw) == E, kw
        assert b"rmsf_cluster_dbscan" in lib.rmsf_last_error(), kw
    for kw in (dict(work=None), dict(work_bytes=need - 1), dict(work_bytes=0)):
        assert loop(**kw) == M, kw
        assert b"rmsf_cluster_dbscan" in lib.rmsf_last_error() and b"workspace" in lib.rmsf_last_error(), kw

    def host(m_=one, n=100, ld=100, cutoff=1.0, m=5, label=one, core=one, k=ctypes.byref(kcl)):
        return lib.rmsf_cluster_dbscan_host(m_, n, ld, cutoff, m, label, core, k)

    for kw in (dict(m_=None), dict(label=None), dict(core=None), dict(k=None), dict(ld=99), dict(n=0), dict(n=-1),
               dict(n=big, ld=big), dict(m=0), dict(m=-1), dict(cutoff=-1.0), dict(cutoff=-1e-300), dict(cutoff=nan)):
        assert host(**kw) == E, kw
        assert b"rmsf_cluster_dbscan_host" in lib.rmsf_last_error(), kw


# ---- the restatement itself -----------------------------------------------------------
def test_reference_on_a_hand_made_matrix():
    """{0, 1, 2, 9} and {5, 6, 7, 8} are cliques of core rows, 4 is noise, and 3 is a border row of both:
    its lowest-indexed core neighbour, 5, is in cluster 1, and its label is 0."""
    d = np.full((10, 10), 9.0)
    np.fill_diagonal(d, 0.0)
    for clique in ((0, 1, 2, 9), (5, 6, 7, 8)):
        for i in clique:
            for j in clique:
                d[i, j] = min(d[i, j], 1.0)
    d[3, 5] = d[5, 3] = d[3, 9] = d[9, 3] = 1.0
    labels, core_rows, k, rounds = dbscan_reference(d, 1.0, 4)
    assert labels.tolist() == [0, 0, 0, 0, -1, 1, 1, 1, 1, 0] and core_rows.tolist() == [0, 1, 2, 5, 6, 7, 8, 9]
    assert k == 2 and rounds == 2                                      # one round that changes, one that does not
    assert_same(host_dbscan(d, 1.0, 4), (labels, core_rows, k))


# ---- rmsf_cluster_dbscan_host against the restatement ------------------------------------
@pytest.mark.parametrize("m", MIN_SAMPLES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["points", "lattice"])
def test_host_points_and_lattice(kind, n, m):
    d, eps = matrix(kind, n)
    ref = reference(kind, n, m)
    if kind == "lattice" and n >= 63:
        assert (d == eps).sum() > 0                                    # entries equal to the cutoff
    got = host_dbscan(d, eps, m)
    assert_same(got, ref)
    assert_consequences(d, eps, m, *got)


def test_points_130_has_clusters_border_and_noise():
    labels, core_rows, k, _ = reference("points", 130, 4)
    core = np.zeros(130, dtype=bool)
    core[core_rows] = True
    assert k == 6 and int((~core & (labels >= 0)).sum()) == 5 and int((labels < 0).sum()) == 13


@pytest.mark.parametrize("n", [130, 1000])
@pytest.mark.parametrize("kind", ["chain", "chain_shuffled"])
def test_host_chain(kind, n):
    d, eps = matrix(kind, n)
    labels, core_rows, k, rounds = ref = reference(kind, n, CHAIN_M)
    ends = np.flatnonzero(adjacency(d, eps).sum(1) == 2)               # the two ends have one neighbour and themselves
    assert len(ends) == 2 and k == 1 and not labels.any() and len(core_rows) == n - 2
    assert sorted(set(range(n)) - set(core_rows.tolist())) == sorted(ends.tolist())   # two border ends
    if kind == "chain":
        assert rounds == n - 2                                         # the diameter of the core path, and one more
    got = host_dbscan(d, eps, CHAIN_M)
    assert_same(got, ref)
    assert_consequences(d, eps, CHAIN_M, *got)


def test_shuffled_chain_of_1000_takes_756_rounds():
    assert reference("chain_shuffled", 1000, CHAIN_M)[3] == 756


def contested_border_rows(d, eps, m, labels, core_rows):
    """(border rows with core neighbours in more than one cluster, those of
    them whose lowest-indexed core neighbour's cluster is not their label)."""
    adj = adjacency(d, eps)
    core = np.zeros(len(adj), dtype=bool)
    core[core_rows] = True
    several, fooled = [], []
    for i in np.flatnonzero(~core & (labels >= 0)):
        nb = np.flatnonzero(adj[i] & core)
        if len(set(labels[nb])) > 1:
            several.append(i)
            assert labels[i] == labels[nb].min()
            if labels[nb[0]] != labels[i]:
                fooled.append(i)
    return several, fooled


@pytest.mark.parametrize("n,several,fooled", [(130, 3, 2), (1000, 5, 4)])
def test_host_touching(n, several, fooled):
    eps, m = TOUCHING[n]
    d, _ = matrix("touching", n)
    ref = reference("touching", n, m)
    s, f = contested_border_rows(d, eps, m, ref[0], ref[1])
    assert len(s) >= 2 and len(f) >= 1 and (len(s), len(f)) == (several, fooled)
    got = host_dbscan(d, eps, m)
    assert_same(got, ref)
    assert_consequences(d, eps, m, *got)


def test_host_eps_zero_and_above_everything():
    n = 130
    d, _ = matrix("zero", n)
    assert d[~np.eye(n, dtype=bool)].min() > 0.0                       # distinct points
    for m in (2, 4):
        labels, core_rows, k = got = host_dbscan(d, 0.0, m)
        assert (labels == -1).all() and len(core_rows) == 0 and k == 0  # all noise
        assert_same(got, reference("zero", n, m))
    labels, core_rows, k = got = host_dbscan(d, 0.0, 1)
    assert np.array_equal(labels, np.arange(n)) and np.array_equal(core_rows, np.arange(n)) and k == n
    assert_same(got, reference("zero", n, 1))
    for eps in (float(d.max()) + 1.0, float("inf")):
        for m in (1, 8, n):
            labels, core_rows, k = got = host_dbscan(d, eps, m)
            assert not labels.any() and len(core_rows) == n and k == 1
            assert_same(got, dbscan_reference(d, eps, m))
    labels, core_rows, k = host_dbscan(d, float("inf"), n + 1)          # nobody has n + 1 neighbours
    assert (labels == -1).all() and len(core_rows) == 0 and k == 0


def assert_nan_frame(labels, core_rows, k, small_ref, q, keep, m):
    """Frame q (a NaN row and column) is noise for m >= 2 and a cluster of
    its own for m = 1; the others are labelled as without it, renumbered."""
    rest = labels[keep]
    if m >= 2:
        assert labels[q] == -1 and q not in core_rows and k == small_ref[2]
    else:
        lq = labels[q]
        assert lq >= 0 and (labels == lq).sum() == 1 and q in core_rows and k == small_ref[2] + 1
        rest = rest - (rest > lq)
    assert np.array_equal(rest, small_ref[0])
    c = core_rows[core_rows != q]
    assert np.array_equal(c - (c > q), small_ref[1])


@pytest.mark.parametrize("m", [1, 2, 4])
def test_host_nan_row_and_column(m):
    d, eps = matrix("nan", 130)
    _, small, q, keep = nan_case(130)
    small_ref = dbscan_reference(small, eps, m)
    assert small_ref[2] >= 3
    got = host_dbscan(d, eps, m)
    assert_same(got, reference("nan", 130, m))
    assert_nan_frame(*got, small_ref, q, keep, m)


def test_host_padded_matrix():
    n = 130
    d, eps = matrix("points", n)
    padded = np.zeros((n, n + 3))                                      # the padding would be everybody's neighbour
    padded[:, :n] = d
    assert_same(host_dbscan(padded, eps, 4, n=n, ld=n + 3), reference("points", n, 4))


# ---- the same finite cases against scikit-learn ---------------------------------------
SKLEARN_CASES = ([(kind, n, m) for kind in ("points", "lattice") for n in SIZES for m in MIN_SAMPLES]
                 + [(kind, n, CHAIN_M) for kind in ("chain", "chain_shuffled") for n in (130, 1000)]
                 + [("touching", n, TOUCHING[n][1]) for n in TOUCHING])


@pytest.mark.parametrize("kind,n,m", SKLEARN_CASES)
def test_host_against_scikit_learn(kind, n, m):
    cluster = pytest.importorskip("sklearn.cluster")
    d, eps = matrix(kind, n)
    sk = cluster.DBSCAN(eps=eps, min_samples=m, metric="precomputed").fit(np.array(d))
    labels, core_rows, k = host_dbscan(d, eps, m)
    assert np.array_equal(labels, sk.labels_) and np.array_equal(core_rows, sk.core_sample_indices_)
    assert k == (sk.labels_.max() + 1 if len(sk.labels_) else 0)
    ref = reference(kind, n, m)
    assert np.array_equal(ref[0], sk.labels_) and np.array_equal(ref[1], sk.core_sample_indices_)


# ---- DBSCAN: what is decided without a device ------------------------------------------
def test_dbscan_refusals_without_a_device():
    from rmsf_amd import DBSCAN
    from rmsf_amd.distances import DistanceMatrix
    from rmsf_amd.sources import DeviceSource
    x = np.zeros((6, 5, 3), np.float32)
    d = lattice(20)
    with pytest.raises(TypeError):
        DBSCAN(d)                                                      # eps is required
    with pytest.raises(TypeError):
        DBSCAN(d, 1.5)                                                 # and keyword-only
    for bad in (-1.0, -1e-300, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            DBSCAN(d, eps=bad)
    for bad in (0, -1, 2.5, True, "3", None):
        with pytest.raises(ValueError, match="min_samples"):
            DBSCAN(d, eps=1.0, min_samples=bad)
    assert DBSCAN(d, eps=1.0).min_samples == 5 and DBSCAN(d, eps=1.0, min_samples=np.int64(3)).min_samples == 3
    with pytest.raises(ValueError, match="square"):
        DBSCAN(np.zeros((4, 5)), eps=1.0)
    with pytest.raises(ValueError, match="layout"):
        DBSCAN(x, eps=1.0, layout="aos")
    with pytest.raises(ValueError, match="matrix must be"):
        DBSCAN(x, eps=1.0, matrix="f32")
    for kw, inp in ((dict(keep_matrix=True), x), ({}, d), ({}, DistanceMatrix(x))):
        with pytest.raises(ValueError, match='matrix="bits"'):
            DBSCAN(inp, eps=1.0, matrix="bits", **kw)
    lop = d.copy()
    lop[2, 7], lop[7, 2] = 1.0, 3.0                                    # neighbours one way only
    with pytest.raises(ValueError, match="not symmetric"):
        DBSCAN(lop, eps=2.0).run()
    with pytest.raises(NotImplementedError, match="DBSCAN runs on one device"):
        DBSCAN(x, eps=1.0, gpus=2).run()
    with pytest.raises(NotImplementedError, match="DBSCAN runs on one device"):
        DBSCAN([x, x], eps=1.0).run()
    planes = object.__new__(DeviceSource)                              # HBM-resident [F, 3, n_atoms]; no tensor needed
    planes.layout, planes.n_sel = "soa", 5
    with pytest.raises(NotImplementedError, match='layout="fac"'):
        DBSCAN(planes, eps=1.0).run()
    with pytest.raises(ValueError, match="at least 3"):
        DBSCAN(x, eps=1.0, select=[0, 4]).run()                        # DistanceMatrix's own refusals, in its words
    with pytest.raises(ValueError, match="weights"):
        DBSCAN(x, eps=1.0, weights=np.ones(4)).run()


def test_dbscan_refuses_a_distributed_world(monkeypatch):
    from rmsf_amd import DBSCAN, parallel
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="more than one rank"):
        DBSCAN(lattice(20), eps=1.0).run()


def test_cluster_names_itself_in_its_refusals():
    """The helper the two classes share speaks for whichever called it."""
    from rmsf_amd import Cluster
    with pytest.raises(NotImplementedError, match="Cluster runs on one device"):
        Cluster(np.zeros((6, 5, 3), np.float32), cutoff=1.0, gpus=2).run()


def test_script_dbscan_options():
    """rmsf_mi355x.py --dbscan / --dbscan-eps / --dbscan-min-samples: refused before any device work."""
    import os
    import subprocess
    import sys

    from conftest import ROOT
    script = f"{ROOT}/mdanalysis-mpi_amd/rmsf_mi355x.py"
    cases = ((["--dbscan", "x.npy"], "go together", {}),
             (["--dbscan-eps", "1.5"], "go together", {}),
             (["--dbscan", "x.npy", "--dbscan-eps", "-1"], ">= 0", {}),
             (["--dbscan", "x.npy", "--dbscan-eps", "1.5", "--dbscan-min-samples", "0"], ">= 1", {}),
             (["--dbscan-min-samples", "3"], "needs --dbscan", {}),
             (["--dbscan", "x.npy", "--dbscan-eps", "1.5"], "one process", {"WORLD_SIZE": "2"}))
    for extra, msg, env in cases:
        r = subprocess.run([sys.executable, script, "--synthetic", "10", "5", *extra], capture_output=True, text=True,
                           timeout=120, env={**os.environ, **env})
        assert r.returncode == 2 and msg in r.stderr, (extra, r.stderr[-500:])
