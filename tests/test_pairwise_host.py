"""CPU tier of the all-pairs RMSD matrix: the library's new entry points and
their argument checks, what ``DistanceMatrix`` refuses without a device, and
the pure-numpy ``DiffusionMap``."""
import ctypes

import numpy as np
import pytest

NEW_SYMBOLS = ("rmsf_pairwise_centres", "rmsf_pairwise_workspace_bytes", "rmsf_pairwise_rmsd")


def test_library_exports_the_pairwise_entry_points():
    from rmsf_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    import rmsf_amd
    for name in ("DistanceMatrix", "DiffusionMap"):
        assert name in rmsf_amd.__all__ and hasattr(rmsf_amd, name)


def test_workspace_bytes():
    """0 = the epilogue runs in the contraction kernel: enough tile pairs, or
    one atom range.  Split-K partials are whole tile pairs of 9 x 256 doubles."""
    from rmsf_amd import _lib
    wb = _lib.load().rmsf_pairwise_workspace_bytes
    assert wb(0, 10) == 0 and wb(10, 0) == 0 and wb(-1, 5) == 0
    assert wb(5, 5000) > 0 and wb(5, 5000) % 8 == 0       # few frames, many atoms: split-K
    assert wb(5, 5000) == wb(5, 5000)                     # a function of the sizes alone
    assert wb(5, 5000) % (8 * 9 * 256) == 0               # one tile pair per atom range
    assert wb(5, 3) == 0                                  # one stage of atoms: nothing to split
    assert wb(4096, 214) == 0 and wb(4096, 3341) == 0     # 32,896 tile pairs fill the device
    assert wb(256, 100_000) > 0 and wb(256, 100_000) % (8 * 9 * 256 * 136) == 0


# rmsf_pairwise_workspace_bytes(n_frames, n_sel), recorded before the plan
# arithmetic moved into csrc/dense_f64.h: the GPU tests' and
# tools/bench_pairwise.py's shapes, then the tile edges x the stage edges.
PLAN_BYTES = [
    (2, 3, 0), (15, 4, 0), (16, 17, 0), (17, 33, 110592), (33, 31, 0), (50, 214, 1290240), (5, 5000, 2893824),
    (9, 31, 0), (9, 32, 0), (9, 33, 36864), (20, 31, 0), (11, 31, 0), (500, 40, 0), (4096, 214, 0), (4096, 3341, 0),
    (256, 100000, 7520256), (1, 1, 0), (1, 31, 0), (1, 32, 0), (1, 33, 36864), (1, 511, 294912), (1, 512, 294912),
    (1, 513, 313344), (1, 5000, 2893824), (1, 100000, 8239104), (15, 1, 0), (15, 31, 0), (15, 32, 0), (15, 33, 36864),
    (15, 511, 294912), (15, 512, 294912), (15, 513, 313344), (15, 5000, 2893824), (15, 100000, 8239104), (16, 1, 0),
    (16, 31, 0), (16, 32, 0), (16, 33, 36864), (16, 511, 294912), (16, 512, 294912), (16, 513, 313344),
    (16, 5000, 2893824), (16, 100000, 8239104), (17, 1, 0), (17, 31, 0), (17, 32, 0), (17, 511, 884736),
    (17, 512, 884736), (17, 513, 940032), (17, 5000, 8681472), (17, 100000, 9123840), (31, 1, 0), (31, 31, 0),
    (31, 32, 0), (31, 33, 110592), (31, 511, 884736), (31, 512, 884736), (31, 513, 940032), (31, 5000, 8681472),
    (31, 100000, 9123840), (32, 1, 0), (32, 31, 0), (32, 32, 0), (32, 33, 110592), (32, 511, 884736),
    (32, 512, 884736), (32, 513, 940032), (32, 5000, 8681472), (32, 100000, 9123840), (33, 1, 0), (33, 32, 0),
    (33, 33, 221184), (33, 511, 1769472), (33, 512, 1769472), (33, 513, 1880064), (33, 5000, 8736768),
    (33, 100000, 9400320), (496, 1, 0), (496, 31, 0), (496, 32, 0), (496, 33, 0), (496, 511, 0), (496, 512, 0),
    (496, 513, 0), (496, 5000, 0), (496, 100000, 0), (497, 1, 0), (497, 31, 0), (497, 32, 0), (497, 33, 0),
    (497, 511, 0), (497, 512, 0), (497, 513, 0), (497, 5000, 0), (497, 100000, 0), (512, 1, 0), (512, 31, 0),
    (512, 32, 0), (512, 33, 0), (512, 511, 0), (512, 512, 0), (512, 513, 0), (512, 5000, 0), (512, 100000, 0),
    (513, 1, 0), (513, 31, 0), (513, 32, 0), (513, 33, 0), (513, 511, 0), (513, 512, 0), (513, 513, 0),
    (513, 5000, 0), (513, 100000, 0),
]


def test_workspace_bytes_are_the_recorded_plan():
    from rmsf_amd import _lib
    wb = _lib.load().rmsf_pairwise_workspace_bytes
    assert [(n_frames, n_sel, wb(n_frames, n_sel)) for n_frames, n_sel, _ in PLAN_BYTES] == PLAN_BYTES


def test_argument_checks_come_before_any_launch():
    from rmsf_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fail first
    E, M = _lib.RMSF_EINVAL, _lib.RMSF_ENOMEM

    def rmsd(xyz=one, fstride=9, n_frames=4, n_sel=3, centre=one, g=one, out=one, ld=4, w_total=3.0, work=None,
             work_bytes=0):
        return lib.rmsf_pairwise_rmsd(xyz, fstride, n_frames, n_sel, None, None, w_total, centre, g, 1, 0.0, out, ld,
                                      work, work_bytes, None)

    for kw in (dict(xyz=None), dict(centre=None), dict(g=None), dict(out=None), dict(ld=3), dict(n_sel=0),
               dict(w_total=0.0), dict(fstride=-1)):
        assert rmsd(**kw) == E, kw
        assert b"rmsf_pairwise_rmsd" in lib.rmsf_last_error(), kw
    # 5 frames x 5,000 atoms needs a workspace: none given, then one too small
    need = lib.rmsf_pairwise_workspace_bytes(5, 5000)
    assert rmsd(n_frames=5, n_sel=5000, ld=5, fstride=15000) == M
    assert b"rmsf_pairwise_rmsd" in lib.rmsf_last_error() and b"workspace" in lib.rmsf_last_error()
    assert rmsd(n_frames=5, n_sel=5000, ld=5, fstride=15000, work=one, work_bytes=need - 8) == M
    assert rmsd(n_frames=0) == _lib.RMSF_OK               # nothing to do, nothing launched

    def centres(xyz=one, n_sel=3, centre=one, g=one, fstride=9):
        return lib.rmsf_pairwise_centres(xyz, fstride, 4, n_sel, None, None, 1, centre, g, None)

    for kw in (dict(xyz=None), dict(centre=None), dict(g=None), dict(n_sel=0), dict(fstride=-1)):
        assert centres(**kw) == E, kw
        assert b"rmsf_pairwise_centres" in lib.rmsf_last_error(), kw


def test_distance_matrix_refusals_without_a_device():
    """n_sel < 3 and bad weights: ValueError; gpus= or shards, HBM planes:
    NotImplementedError -- all before any launch (no engine is made)."""
    from rmsf_amd import DistanceMatrix
    from rmsf_amd.sources import DeviceSource
    x = np.zeros((6, 5, 3), np.float32)
    with pytest.raises(ValueError, match="at least 3"):
        DistanceMatrix(x[:, :2]).run()
    with pytest.raises(ValueError, match="at least 3"):
        DistanceMatrix(x, select=[0, 4]).run()
    with pytest.raises(ValueError, match="weights"):
        DistanceMatrix(x, weights=np.ones(4)).run()                    # wrong length
    with pytest.raises(ValueError, match="weights"):
        DistanceMatrix(x, select=[0, 1, 2], weights=np.ones(5)).run()  # the selection's length counts
    for bad in ([1.0, 2.0, 0.0, 1.0, 1.0], [1.0, -2.0, 1.0, 1.0, 1.0], [1.0, np.nan, 1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="positive"):
            DistanceMatrix(x, weights=bad).run()
    with pytest.raises(ValueError, match="mass"):
        DistanceMatrix(x, weights="mass").run()                        # an array has no masses
    with pytest.raises(ValueError, match="weights"):
        DistanceMatrix(x, weights="charge").run()
    with pytest.raises(NotImplementedError, match="one device"):
        DistanceMatrix(x, gpus=2).run()
    with pytest.raises(NotImplementedError, match="one device"):
        DistanceMatrix([x, x]).run()
    planes = object.__new__(DeviceSource)                    # HBM-resident [F, 3, n_atoms]; no tensor needed
    planes.layout, planes.n_sel = "soa", 5
    with pytest.raises(NotImplementedError, match='layout="fac"'):
        DistanceMatrix(planes).run()
    with pytest.raises(ValueError, match="layout"):
        DistanceMatrix(x, layout="aos")


def _random_distances(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 4))
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    d = 0.5 * (d + d.T)
    np.fill_diagonal(d, 0.0)
    return d


def test_diffusion_map_on_a_random_symmetric_matrix():
    from rmsf_amd import DiffusionMap
    n, eps = 40, 2.5
    d = _random_distances(n, 3)
    dm = DiffusionMap(d, epsilon=eps).run()
    w, v = dm.results.eigenvalues, dm.results.eigenvectors
    assert w.shape == (n,) and v.shape == (n, n) and dm.results.n_frames == n
    assert abs(w[0] - 1.0) <= 1e-12                                   # the leading eigenvalue
    assert np.abs(v[:, 0] - v[:, 0].mean()).max() <= 1e-12 * abs(v[:, 0].mean())   # its eigenvector is constant
    assert np.all(np.diff(w) <= 0) and w.max() <= 1 + 1e-12 and w.min() >= -1 - 1e-12
    # the eigenpairs reconstruct the transition matrix P = D^-1 K: the columns
    # of v are P's right eigenvectors, the rows of v^-1 its left ones
    k = np.exp(-d * d / eps)
    p = k / k.sum(axis=1, keepdims=True)
    assert np.abs(v @ np.diag(w) @ np.linalg.inv(v) - p).max() <= 1e-10
    assert np.abs(p @ v - v * w).max() <= 1e-10
    # transform: the eigenvectors after the constant one, scaled by lambda^time
    t0 = dm.transform(3, 0)
    assert t0.shape == (n, 3)
    np.testing.assert_array_equal(t0, v[:, 1:4])
    np.testing.assert_allclose(dm.transform(3, 2), v[:, 1:4] * w[1:4] ** 2, rtol=1e-15)
    np.testing.assert_allclose(dm.transform(2, 1), t0[:, :2] * w[1:3], rtol=1e-15)
    for bad in (0, n):
        with pytest.raises(ValueError):
            dm.transform(bad, 1)
    with pytest.raises(ValueError):
        DiffusionMap(d, epsilon=0.0)
    with pytest.raises(ValueError):
        DiffusionMap(np.zeros((3, 4))).run()
    # epsilon scales the kernel: a wider one mixes faster (a smaller gap to 1)
    assert DiffusionMap(d, epsilon=10 * eps).run().results.eigenvalues[1] != w[1]
