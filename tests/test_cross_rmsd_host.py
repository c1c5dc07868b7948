"""CPU tier of the cross RMSD matrix: the library's new entry points, the
plan behind ``rmsf_cross_workspace_bytes``, the argument checks that come
before any launch, what ``CrossDistanceMatrix`` refuses without a device, and
the numpy-only ``hausdorff`` / ``discrete_frechet``."""
import ctypes

import numpy as np
import pytest

NEW_SYMBOLS = ("rmsf_cross_workspace_bytes", "rmsf_cross_rmsd", "rmsf_row_argmin")
TILE_BYTES = 8 * 9 * 256       # one tile pair's nine A_ij entries of 16 x 16 frame pairs, f64
TF, KA, TARGET = 16, 32, 512   # kTF, kKA, kTargetGroups of csrc/pairwise.hip


def test_library_exports_the_cross_entry_points():
    from rmsf_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    import rmsf_amd
    for name in ("CrossDistanceMatrix", "hausdorff", "discrete_frechet"):
        assert name in rmsf_amd.__all__ and hasattr(rmsf_amd, name)


def plan(n_a, n_b, n_sel):
    """(tile pairs, n_ks) by split_k's formula (csrc/dense_f64.h) with
    min_stages = 1, restated."""
    pairs = -(-n_a // TF) * -(-n_b // TF)
    stages = max(1, -(-n_sel // KA))
    ks = max(1, min(stages, TARGET // pairs))
    per = -(-stages // ks)
    return pairs, -(-stages // per)


def test_workspace_bytes():
    from rmsf_amd import _lib
    wb = _lib.load().rmsf_cross_workspace_bytes
    for bad in ((0, 5, 100), (5, 0, 100), (5, 5, 0), (-1, 5, 100), (5, -3, 100), (5, 5, -1)):
        assert wb(*bad) == 0, bad
    # more than 256 tile pairs leave no room to split; one stage of atoms has nothing to split
    assert wb(16 * 257, 16, 5000) == 0 and wb(16 * 16 + 1, 16 * 16 + 1, 5000) == 0
    assert wb(16 * 256, 16, 5000) > 0
    assert wb(3, 5, 32) == 0 and wb(3, 5, 3) == 0 and wb(3, 5, 33) > 0
    for shape in ((3, 5, 5000), (17, 33, 33)):
        assert wb(*shape) > 0 and wb(*shape) % TILE_BYTES == 0, shape
    for shape in ((3, 5, 5000), (17, 33, 33), (33, 5, 31), (528, 130, 40), (256, 16, 100_000), (4096, 64, 214),
                  (20_000, 64, 214), (1, 50, 214), (50, 1, 214), (9, 20, 33), (4096, 16, 5000), (4097, 16, 5000)):
        pairs, n_ks = plan(*shape)
        assert wb(*shape) == (TILE_BYTES * pairs * n_ks if n_ks > 1 else 0), shape
        assert wb(*shape) == wb(*shape), shape                 # a function of the sizes alone
    assert plan(3, 5, 5000) == (1, 157) and plan(17, 33, 33) == (6, 2) and plan(528, 130, 40) == (297, 1)


def test_argument_checks_come_before_any_launch():
    from rmsf_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fail first
    E, M = _lib.RMSF_EINVAL, _lib.RMSF_ENOMEM

    def cross(a=one, stride_a=9, n_a=4, centre_a=one, g_a=one, b=one, stride_b=9, n_b=5, centre_b=one, g_b=one,
              n_sel=3, w_total=3.0, out=one, ld=5, work=None, work_bytes=0):
        return lib.rmsf_cross_rmsd(a, stride_a, n_a, None, centre_a, g_a, b, stride_b, n_b, None, centre_b, g_b,
                                   n_sel, None, w_total, 1, 0.0, out, ld, work, work_bytes, None)

    for kw in (dict(a=None), dict(centre_a=None), dict(g_a=None), dict(b=None), dict(centre_b=None), dict(g_b=None),
               dict(out=None), dict(ld=4), dict(n_sel=0), dict(w_total=0.0), dict(w_total=-1.0),
               dict(stride_a=-1), dict(stride_b=-1)):
        assert cross(**kw) == E, kw
        assert b"rmsf_cross_rmsd" in lib.rmsf_last_error(), kw
    # 3 x 5 frames of 5,000 atoms need a workspace: none given, then one too small
    need = lib.rmsf_cross_workspace_bytes(3, 5, 5000)
    big = dict(n_a=3, n_b=5, n_sel=5000, stride_a=15000, stride_b=15000)
    assert cross(**big) == M
    assert b"rmsf_cross_rmsd" in lib.rmsf_last_error() and b"workspace" in lib.rmsf_last_error()
    assert cross(**big, work=one, work_bytes=need - 8) == M
    assert cross(n_a=0) == _lib.RMSF_OK and cross(n_b=0) == _lib.RMSF_OK   # nothing to do, nothing launched
    # more tile pairs than one launch takes
    assert cross(n_a=2 ** 31, n_b=2 ** 31, ld=2 ** 31) == E

    def argmin(m=one, n_rows=4, n_cols=5, ld=5, idx=one, val=one):
        return lib.rmsf_row_argmin(m, n_rows, n_cols, ld, idx, val, None)

    for kw in (dict(m=None), dict(idx=None, val=None), dict(n_cols=0), dict(ld=4), dict(n_rows=-1)):
        assert argmin(**kw) == E, kw
        assert b"rmsf_row_argmin" in lib.rmsf_last_error(), kw
    assert argmin(n_rows=0) == _lib.RMSF_OK

    def about(xyz=one, n_sel=3, centre0=one, centre=one, g=one, fstride=9):
        return lib.rmsf_pairwise_centres_about(xyz, fstride, 4, n_sel, None, None, centre0, centre, g, None)

    for kw in (dict(xyz=None), dict(centre0=None), dict(centre=None), dict(g=None), dict(n_sel=0), dict(fstride=-1)):
        assert about(**kw) == E, kw
        assert b"rmsf_pairwise_centres_about" in lib.rmsf_last_error(), kw


def test_cross_distance_matrix_refusals_without_a_device():
    from rmsf_amd import CrossDistanceMatrix
    from rmsf_amd.sources import DeviceSource
    x = np.zeros((6, 5, 3), np.float32)
    y = np.zeros((4, 8, 3), np.float32)
    with pytest.raises(NotImplementedError, match="one device"):
        CrossDistanceMatrix(x, x, gpus=2).run()
    with pytest.raises(NotImplementedError, match="one device"):
        CrossDistanceMatrix([x, x], x).run()
    with pytest.raises(NotImplementedError, match="one device"):
        CrossDistanceMatrix(x, (x, x)).run()
    with pytest.raises(ValueError, match="same length"):
        CrossDistanceMatrix(x, y).run()                                          # 5 atoms against 8
    with pytest.raises(ValueError, match="same length"):
        CrossDistanceMatrix(x, y, select=[0, 1, 2], select_b=[0, 1, 2, 3]).run()
    with pytest.raises(ValueError, match="at least 3"):
        CrossDistanceMatrix(x, y, select=[0, 4]).run()                           # select_b defaults to select
    with pytest.raises(ValueError, match="at least 3"):
        CrossDistanceMatrix(x[:, :2], x[0, :2]).run()                            # a 2-D array is one frame
    with pytest.raises(ValueError, match="weights"):
        CrossDistanceMatrix(x, x, weights=np.ones(4)).run()                      # wrong length
    with pytest.raises(ValueError, match="weights"):
        CrossDistanceMatrix(x, y, select=[0, 1, 2], select_b=[5, 6, 7], weights=np.ones(5)).run()
    for bad in ([1.0, 2.0, 0.0, 1.0, 1.0], [1.0, -2.0, 1.0, 1.0, 1.0], [1.0, np.nan, 1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="positive"):
            CrossDistanceMatrix(x, x, weights=bad).run()
    with pytest.raises(ValueError, match="mass"):
        CrossDistanceMatrix(x, x, weights="mass").run()                          # an array has no masses
    with pytest.raises(ValueError, match="weights"):
        CrossDistanceMatrix(x, x, weights="charge").run()
    planes = object.__new__(DeviceSource)                    # HBM-resident [F, 3, n_atoms]; no tensor needed
    planes.layout, planes.n_sel = "soa", 5
    for a, b in ((planes, x), (x, planes)):
        with pytest.raises(NotImplementedError, match='layout="fac"'):
            CrossDistanceMatrix(a, b).run()
    with pytest.raises(ValueError, match="layout"):
        CrossDistanceMatrix(x, x, layout="aos")
    with pytest.raises(ValueError, match="layout"):
        CrossDistanceMatrix(x, x, layout_b="aos")


def test_script_cross_options_go_together():
    """rmsf_mi355x.py --cross-rmsd / --cross-with: refused alone, and with
    --synthetic, before any device work."""
    import subprocess
    import sys

    from conftest import ROOT
    script = f"{ROOT}/mdanalysis-mpi_amd/rmsf_mi355x.py"
    for extra, msg in ((["--cross-rmsd", "x.npy"], "go together"), (["--cross-with", "b.xtc"], "go together"),
                       (["--cross-rmsd", "x.npy", "--cross-with", "b.xtc"], "--cross-rmsd needs --topology")):
        r = subprocess.run([sys.executable, script, "--synthetic", "10", "5", *extra], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and msg in r.stderr, (extra, r.stderr[-500:])


# ---- hausdorff / discrete_frechet ------------------------------------------------
def hausdorff_loops(d):
    n, m = d.shape
    h = -np.inf
    for i in range(n):
        h = max(h, min(d[i, j] for j in range(m)))
    for j in range(m):
        h = max(h, min(d[i, j] for i in range(n)))
    return h


def frechet_loops(d):
    """Eiter and Mannila's coupling recurrence, entry by entry."""
    n, m = d.shape
    c = np.empty((n, m))
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                c[i, j] = d[0, 0]
            elif i == 0:
                c[i, j] = max(c[0, j - 1], d[0, j])
            elif j == 0:
                c[i, j] = max(c[i - 1, 0], d[i, 0])
            else:
                c[i, j] = max(d[i, j], min(c[i - 1, j], c[i - 1, j - 1], c[i, j - 1]))
    return c[n - 1, m - 1]


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 9), (40, 33)])
def test_path_metrics_against_double_loops(shape):
    """Both only select and compare entries of d: exact equality."""
    from rmsf_amd import discrete_frechet, hausdorff
    for seed in range(3):
        d = np.random.default_rng(100 * seed + shape[0] + 7 * shape[1]).uniform(0.0, 10.0, size=shape)
        assert hausdorff(d) == hausdorff_loops(d)
        assert discrete_frechet(d) == frechet_loops(d)
        assert hausdorff(d.T) == hausdorff(d) and discrete_frechet(d.T) == discrete_frechet(d)
        assert discrete_frechet(d) >= hausdorff(d)       # a coupling visits every frame of both paths


def test_path_metrics_known_answers():
    from rmsf_amd import discrete_frechet, hausdorff
    # points on a line, P = (0, 1, 2) and Q = (0, 2): d[i, j] = |P_i - Q_j|.  P's middle point is 1 from
    # either point of Q, every other point has a partner at 0: Hausdorff 1; and the walk has to pair it: Frechet 1
    p, q = np.array([0.0, 1.0, 2.0]), np.array([0.0, 2.0])
    d = np.abs(p[:, None] - q[None, :])
    assert hausdorff(d) == 1.0 and discrete_frechet(d) == 1.0
    # the same points of Q walked backwards: every frame still has a partner within 1 (Hausdorff 1), but the
    # walks start at opposite ends: the first pair alone is 2 apart (Frechet 2)
    d = np.abs(p[:, None] - q[::-1][None, :])
    assert hausdorff(d) == 1.0 and discrete_frechet(d) == 2.0
    assert hausdorff([[3.5]]) == 3.5 and discrete_frechet([[3.5]]) == 3.5
    for f in (hausdorff, discrete_frechet):
        with pytest.raises(ValueError):
            f(np.zeros((0, 4)))
        with pytest.raises(ValueError):
            f(np.zeros(4))
