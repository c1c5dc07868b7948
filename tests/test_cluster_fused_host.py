"""CPU tier of the fused neighbour bits (``Cluster(matrix=...)``,
``rmsf_pairwise_adjacency``, ``rmsf_adjacency_count``): what is decided
without a device -- the keyword's refusals in ``__init__``, the two symbols,
their argument checks (which come before any launch) and the script's flag."""
import ctypes
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_abi import HEADER, declared_functions
from test_clustering_host import lattice

NEW_SYMBOLS = ("rmsf_pairwise_adjacency", "rmsf_adjacency_count")


def test_matrix_keyword_is_checked_in_init():
    from rmsf_amd import Cluster, DistanceMatrix
    x = np.zeros((6, 5, 3), np.float32)
    d = lattice(20)
    with pytest.raises(ValueError, match="matrix"):
        Cluster(x, cutoff=1.0, matrix="nope")
    with pytest.raises(ValueError, match="keep_matrix"):
        Cluster(x, cutoff=1.0, matrix="bits", keep_matrix=True)
    with pytest.raises(ValueError, match="distance matrix"):
        Cluster(d, cutoff=1.0, matrix="bits")
    with pytest.raises(ValueError, match="distance matrix"):
        Cluster(DistanceMatrix(x), cutoff=1.0, matrix="bits")
    # what "auto" becomes where a matrix is asked for or given, and what stays open until the device is known
    assert Cluster(x, cutoff=1.0).matrix == "auto" and Cluster(x, cutoff=1.0, matrix="bits").matrix == "bits"
    assert Cluster(x, cutoff=1.0, matrix="f64").matrix == "f64"
    assert Cluster(x, cutoff=1.0, keep_matrix=True).matrix == "f64"
    assert Cluster(d, cutoff=1.0).matrix == "f64" and Cluster(DistanceMatrix(x), cutoff=1.0).matrix == "f64"


def test_library_declares_and_exports_the_two_entry_points():
    from rmsf_amd import _lib
    lib = _lib.load()
    declared = declared_functions()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(re.findall(rf"\bint\s+{name}\s*\(", src)) == 1, name
    # the argument counts of the header's prototypes and of the ctypes table agree
    for name in NEW_SYMBOLS:
        proto = re.search(rf"\b{name}\s*\(([^)]*)\)", src).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_argument_checks_come_before_any_launch():
    from rmsf_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fail first
    E, M = _lib.RMSF_EINVAL, _lib.RMSF_ENOMEM
    nan, big = float("nan"), 2 ** 31

    def count(adj=one, n=100, ldw=2, cnt=one):
        return lib.rmsf_adjacency_count(adj, n, ldw, cnt, None)

    for kw in (dict(adj=None), dict(cnt=None), dict(ldw=1), dict(n=0), dict(n=-5), dict(n=big, ldw=big)):
        assert count(**kw) == E, kw
        assert b"rmsf_adjacency_count" in lib.rmsf_last_error(), kw

    def fused(xyz=one, fstride=30, n=100, n_sel=10, w_total=10.0, centre=one, g=one, zero_cutoff=1e-5, cutoff=1.0,
              adj=one, ldw=2, work=None, work_bytes=0):
        return lib.rmsf_pairwise_adjacency(xyz, fstride, n, n_sel, None, None, w_total, centre, g, 1, zero_cutoff,
                                           cutoff, adj, ldw, None, work, work_bytes, None)

    for kw in (dict(xyz=None), dict(centre=None), dict(g=None), dict(adj=None), dict(n_sel=0), dict(n=-1),
               dict(fstride=-1), dict(w_total=0.0), dict(w_total=nan), dict(ldw=1), dict(cutoff=nan),
               dict(cutoff=-1.0), dict(cutoff=-1e-300)):
        assert fused(**kw) == E, kw
        assert b"rmsf_pairwise_adjacency" in lib.rmsf_last_error(), kw
    # a plan of more tile pairs than a grid's x extent takes: 65,537 tiles a side
    n_big = 16 * 65537
    assert fused(n=n_big, ldw=(n_big + 63) // 64) == E
    assert b"rmsf_pairwise_adjacency" in lib.rmsf_last_error() and b"too many frames" in lib.rmsf_last_error()
    # split-K shapes need the workspace of rmsf_pairwise_workspace_bytes
    need = lib.rmsf_pairwise_workspace_bytes(5, 5000)
    assert need > 0
    for kw in (dict(work=None, work_bytes=need), dict(work=one, work_bytes=need - 1), dict(work=one, work_bytes=0)):
        assert fused(n=5, n_sel=5000, w_total=5000.0, ldw=1, **kw) == M, kw
        assert b"rmsf_pairwise_adjacency" in lib.rmsf_last_error() and b"workspace" in lib.rmsf_last_error(), kw
    assert fused(n=0, ldw=0) == _lib.RMSF_OK               # no frames: nothing to do, nothing launched


def test_script_cluster_matrix_needs_cluster():
    script = f"{ROOT}/mdanalysis-mpi_amd/rmsf_mi355x.py"
    r = subprocess.run([sys.executable, script, "--synthetic", "10", "5", "--cluster-matrix", "bits"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "needs --cluster" in r.stderr, r.stderr[-500:]
    r = subprocess.run([sys.executable, script, "--synthetic", "10", "5", "--cluster", "x.npy", "--cluster-cutoff",
                        "1.5", "--cluster-matrix", "f32"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "invalid choice" in r.stderr, r.stderr[-500:]
