"""CPU tier of the positional covariance / PCA feature: the library's new
entry points, the pure-numpy eigen-decomposition, and the argument refusals
that need no device."""
import ctypes

import numpy as np
import pytest

NEW_SYMBOLS = ("rmsf_covariance_workspace_bytes", "rmsf_covariance_accumulate", "rmsf_covariance_finish")


def test_library_exports_the_covariance_entry_points():
    from rmsf_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def test_workspace_bytes_and_argument_checks_on_the_host():
    """Host-only parts of the ABI: the workspace bound (0 = results go
    straight to d_cov: enough tile pairs, or one frame range) and the
    argument checks, which come before any launch."""
    from rmsf_amd import _lib
    lib = _lib.load()
    wb = lib.rmsf_covariance_workspace_bytes
    assert wb(0, 10) == 0 and wb(10, 0) == 0
    assert wb(214, 1) == 0                      # one stage of frames: no split-K
    assert wb(214, 20000) > 0 and wb(214, 20000) % 8 == 0
    assert wb(214, 20000) == wb(214, 20000)     # a function of the sizes alone
    assert wb(3341, 4000) == 0                  # 21,945 tile pairs fill the device
    # split-K partials: whole 48 x 48 tiles plus a T1 row per tile
    n_tiles = -(-214 // 16)
    per_range = n_tiles * (n_tiles + 1) // 2 * 48 * 48 + n_tiles * 48
    assert wb(214, 20000) % (8 * per_range) == 0
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fail first
    rc = lib.rmsf_covariance_accumulate(None, 0, 1, 1, None, None, None, one, one, 3, one, None, 0, None)
    assert rc == _lib.RMSF_EINVAL and b"rmsf_covariance_accumulate" in lib.rmsf_last_error()
    rc = lib.rmsf_covariance_accumulate(one, 3, 1, 1, None, one, None, one, one, 3, one, None, 0, None)
    assert rc == _lib.RMSF_EINVAL and b"go together" in lib.rmsf_last_error()
    rc = lib.rmsf_covariance_accumulate(one, 3, 1, 2, None, None, None, one, one, 5, one, None, 0, None)
    assert rc == _lib.RMSF_EINVAL                # ld < 3 n_sel
    rc = lib.rmsf_covariance_accumulate(one, 642, 20000, 214, None, None, None, one, one, 642, one, None, 0, None)
    assert rc == _lib.RMSF_ENOMEM and b"workspace" in lib.rmsf_last_error()
    assert lib.rmsf_covariance_finish(None, 3, one, 3, 1, None) == _lib.RMSF_EINVAL
    assert lib.rmsf_covariance_finish(one, 2, one, 3, 1, None) == _lib.RMSF_EINVAL
    assert lib.rmsf_covariance_finish(one, 3, one, 3, 0, None) == _lib.RMSF_EEMPTY


# rmsf_covariance_workspace_bytes(n_sel, n_frames), recorded before the plan
# arithmetic moved into csrc/dense_f64.h: the GPU tests' and
# tools/bench_covariance.py's shapes, then the tile edges x the stage edges.
PLAN_BYTES = [
    (1, 1, 0), (5, 3, 0), (16, 4, 0), (17, 5, 0), (214, 67, 5822208), (341, 300, 9343488), (341, 128, 9343488),
    (341, 44, 9343488), (500, 40, 0), (214, 300, 7762944), (214, 20000, 7762944), (3341, 4000, 0), (1, 31, 0),
    (1, 32, 0), (1, 33, 37632), (1, 511, 301056), (1, 512, 301056), (1, 513, 319872), (1, 5000, 2954112),
    (1, 100000, 8410752), (15, 1, 0), (15, 31, 0), (15, 32, 0), (15, 33, 37632), (15, 511, 301056), (15, 512, 301056),
    (15, 513, 319872), (15, 5000, 2954112), (15, 100000, 8410752), (16, 1, 0), (16, 31, 0), (16, 32, 0),
    (16, 33, 37632), (16, 511, 301056), (16, 512, 301056), (16, 513, 319872), (16, 5000, 2954112),
    (16, 100000, 8410752), (17, 1, 0), (17, 31, 0), (17, 32, 0), (17, 33, 112128), (17, 511, 897024),
    (17, 512, 897024), (17, 513, 953088), (17, 5000, 8802048), (17, 100000, 9250560), (31, 1, 0), (31, 31, 0),
    (31, 32, 0), (31, 33, 112128), (31, 511, 897024), (31, 512, 897024), (31, 513, 953088), (31, 5000, 8802048),
    (31, 100000, 9250560), (32, 1, 0), (32, 31, 0), (32, 32, 0), (32, 33, 112128), (32, 511, 897024),
    (32, 512, 897024), (32, 513, 953088), (32, 5000, 8802048), (32, 100000, 9250560), (33, 1, 0), (33, 31, 0),
    (33, 32, 0), (33, 33, 223488), (33, 511, 1787904), (33, 512, 1787904), (33, 513, 1899648), (33, 5000, 8827776),
    (33, 100000, 9498240), (496, 1, 0), (496, 31, 0), (496, 32, 0), (496, 33, 0), (496, 511, 0), (496, 512, 0),
    (496, 513, 0), (496, 5000, 0), (496, 100000, 0), (497, 1, 0), (497, 31, 0), (497, 32, 0), (497, 33, 0),
    (497, 511, 0), (497, 512, 0), (497, 513, 0), (497, 5000, 0), (497, 100000, 0), (512, 1, 0), (512, 31, 0),
    (512, 32, 0), (512, 33, 0), (512, 511, 0), (512, 512, 0), (512, 513, 0), (512, 5000, 0), (512, 100000, 0),
    (513, 1, 0), (513, 31, 0), (513, 32, 0), (513, 33, 0), (513, 511, 0), (513, 512, 0), (513, 513, 0),
    (513, 5000, 0), (513, 100000, 0),
]


def test_workspace_bytes_are_the_recorded_plan():
    from rmsf_amd import _lib
    wb = _lib.load().rmsf_covariance_workspace_bytes
    assert [(n_sel, n_frames, wb(n_sel, n_frames)) for n_sel, n_frames, _ in PLAN_BYTES] == PLAN_BYTES


def _pair_to_tiles():
    from rmsf_amd import _lib
    fn = _lib.load().rmsf_internal_pair_to_tiles
    fn.restype = None
    fn.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    i, j = ctypes.c_int64(), ctypes.c_int64()

    def mapped(p, n_tiles):
        i.value = j.value = -1
        fn(p, n_tiles, ctypes.byref(i), ctypes.byref(j))
        return i.value, j.value
    return mapped


@pytest.mark.parametrize("n_tiles", [1, 2, 3, 22, 209, 256])
def test_pair_to_tiles_is_the_upper_triangle_in_row_order(n_tiles):
    """The tile mapping of k_comoment_tiles, k_comoment_fold, k_pw_tiles and
    k_pw_fold (csrc/dense_f64.h), on the host: a wrong (I, J) there is an out-of-bounds
    store."""
    mapped = _pair_to_tiles()
    p = 0
    for i in range(n_tiles):
        for j in range(i, n_tiles):
            assert mapped(p, n_tiles) == (i, j), p
            p += 1
    assert p == n_tiles * (n_tiles + 1) // 2


def test_pair_to_tiles_at_the_largest_grid():
    """65,535 tiles a side: the most that n_pairs <= INT32_MAX admits.  The
    first and the last pair of every row, where the square root's rounding
    would show."""
    mapped = _pair_to_tiles()
    n = 65535
    assert n * (n + 1) // 2 <= 2 ** 31 - 1 < (n + 1) * (n + 2) // 2
    for i in range(n):
        first = i * n - i * (i - 1) // 2
        assert mapped(first, n) == (i, i), i
        assert mapped(first + n - i - 1, n) == (i, n - 1), i


def _random_psd(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 2 * n)) * rng.uniform(0.1, 3.0, size=(n, 1))
    return a @ a.T


def test_pca_from_comoment_matches_eigh():
    from rmsf_amd import pca_from_comoment
    n, n_frames = 30, 57
    m = _random_psd(n, 0)
    w_ref, v_ref = np.linalg.eigh(m / (n_frames - 1))
    w_ref, v_ref = w_ref[::-1], v_ref[:, ::-1]
    comp, var, cum = pca_from_comoment(m, n_frames)
    assert comp.shape == (n, n) and var.shape == (n,) and cum.shape == (n,)
    assert np.all(np.diff(var) <= 0)                        # descending variance
    np.testing.assert_allclose(var, w_ref, rtol=1e-12, atol=0)
    for k in range(n):                                      # columns, sign free
        assert abs(abs(comp[:, k] @ v_ref[:, k]) - 1.0) < 1e-9
    np.testing.assert_allclose(comp.T @ comp, np.eye(n), atol=1e-12)
    assert cum[-1] == pytest.approx(1.0, abs=1e-14)
    np.testing.assert_allclose(cum, np.cumsum(w_ref) / w_ref.sum(), rtol=1e-12)
    # ddof scales the eigenvalues only
    _, var0, cum0 = pca_from_comoment(m, n_frames, ddof=0)
    np.testing.assert_allclose(var0 * n_frames, var * (n_frames - 1), rtol=1e-12)
    np.testing.assert_allclose(cum0, cum, rtol=1e-12)
    # truncation keeps the leading components and the share of the whole
    comp3, var3, cum3 = pca_from_comoment(m, n_frames, n_components=3)
    assert comp3.shape == (n, 3)
    np.testing.assert_array_equal(var3, var[:3])
    np.testing.assert_array_equal(cum3, cum[:3])
    np.testing.assert_array_equal(comp3, comp[:, :3])
    assert cum3[-1] < 1.0
    for bad in (dict(n_components=0), dict(n_components=n + 1), dict(ddof=n_frames)):
        with pytest.raises(ValueError):
            pca_from_comoment(m, n_frames, **bad)
    with pytest.raises(ValueError):
        pca_from_comoment(np.zeros((3, 4)), 10)


def test_covariance_refusals_without_a_device():
    """n_splits / merge_scatter / merge_slabs > 1 with covariance: ValueError;
    HBM planes read in place: NotImplementedError naming layout="fac";
    gpus= or a list of shards: NotImplementedError -- all before any launch
    (no device is touched: the engine argument is never used)."""
    from rmsf_amd import PCA, RMSF
    from rmsf_amd.pipeline import check_covariance_args, run_pipeline
    from rmsf_amd.sources import DeviceSource, FrameList

    class Src:
        n_sel = 4

    for kw in (dict(n_splits=2), dict(merge_scatter=True), dict(merge_slabs=2)):
        with pytest.raises(ValueError, match="covariance"):
            run_pipeline(None, Src(), FrameList(10), covariance=True, **kw)
        with pytest.raises(ValueError, match="covariance"):
            check_covariance_args(Src(), **kw)
    check_covariance_args(Src())                             # the default merge passes
    check_covariance_args(Src(), merge_slabs=1)
    planes = object.__new__(DeviceSource)                    # HBM-resident [F, 3, n_atoms]; no tensor needed
    planes.layout = "soa"
    with pytest.raises(NotImplementedError, match='layout="fac"'):
        run_pipeline(None, planes, FrameList(10), covariance=True)
    x = np.zeros((6, 5, 3), np.float32)
    with pytest.raises(NotImplementedError, match="covariance"):
        RMSF(x, covariance=True, gpus=2).run()
    with pytest.raises(NotImplementedError, match="covariance"):
        RMSF([x, x], covariance=True).run()
    with pytest.raises(NotImplementedError, match="covariance"):
        PCA(x, gpus=[0, 1]).run()
    for kw in (dict(n_splits=2), dict(merge_scatter=True)):
        with pytest.raises(ValueError, match="covariance"):
            RMSF(x, covariance=True, **kw).run()
