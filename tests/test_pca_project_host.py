"""CPU tier: what PCA.transform and its kernel's plan decide on the host --
the split-K workspace size (rmsf_pca_project_workspace_bytes, host-only
integer arithmetic), ``cosine_content``, and the argument checks of
``PCA.transform`` that need no device.
"""
import numpy as np
import pytest

import conftest  # noqa: F401  (import paths)


def _lib():
    from rmsf_amd import _lib
    return _lib.load()


def test_workspace_bytes_plan():
    lib = _lib()
    ws = lib.rmsf_pca_project_workspace_bytes
    # many frame tiles, a small selection: no coordinate split, no workspace
    assert ws(4096, 214, 10) == 0
    # one frame tile, 5,000 atoms: the coordinates are split (the GPU tests'
    # split-K case relies on it) -- n_ks partials of [F, k] doubles
    need = ws(5, 5000, 3)
    assert need > 0 and need % (5 * 3 * 8) == 0
    # degenerate shapes ask for nothing
    assert ws(0, 214, 10) == 0 and ws(16, 0, 10) == 0 and ws(16, 214, 0) == 0


def test_workspace_bytes_deterministic():
    ws = _lib().rmsf_pca_project_workspace_bytes
    shapes = [(5, 5000, 3), (256, 100_000, 48), (4096, 3341, 10), (1, 1, 1), (20_000, 214, 48), (33, 17, 51)]
    first = [ws(*s) for s in shapes]
    for _ in range(3):
        assert [ws(*s) for s in shapes] == first


# rmsf_pca_project_workspace_bytes(n_frames, n_sel, n_comp), recorded before
# the plan arithmetic moved into csrc/dense_f64.h: the GPU tests' and
# tools/bench_pca_project.py's shapes, then the tile edges x the stage edges
# at 3 and 49 components (one panel, two).
PLAN_BYTES = [
    (1, 1, 1, 0), (3, 5, 2, 0), (16, 16, 16, 0), (17, 17, 17, 0), (33, 17, 51, 0), (67, 214, 10, 0), (300, 341, 7, 0),
    (128, 341, 7, 0), (44, 341, 7, 0), (5, 5000, 3, 1080), (5, 17, 51, 0), (67, 214, 642, 0), (300, 341, 10, 0),
    (20000, 214, 10, 0), (20000, 214, 48, 0), (4096, 3341, 10, 1310720), (4096, 3341, 48, 6291456),
    (256, 100000, 10, 1310720), (256, 100000, 48, 6291456), (1, 1, 3, 0), (1, 1, 49, 0), (1, 31, 3, 0),
    (1, 31, 49, 0), (1, 32, 3, 0), (1, 32, 49, 0), (1, 33, 3, 0), (1, 33, 49, 0), (1, 511, 3, 0), (1, 511, 49, 0),
    (1, 512, 3, 0), (1, 512, 49, 0), (1, 513, 3, 0), (1, 513, 49, 0), (1, 5000, 3, 216), (1, 5000, 49, 3528),
    (1, 100000, 3, 4416), (1, 100000, 49, 72128), (15, 1, 3, 0), (15, 1, 49, 0), (15, 31, 3, 0), (15, 31, 49, 0),
    (15, 32, 3, 0), (15, 32, 49, 0), (15, 33, 3, 0), (15, 33, 49, 0), (15, 511, 3, 0), (15, 511, 49, 0),
    (15, 512, 3, 0), (15, 512, 49, 0), (15, 513, 3, 0), (15, 513, 49, 0), (15, 5000, 3, 3240), (15, 5000, 49, 52920),
    (15, 100000, 3, 66240), (15, 100000, 49, 1081920), (16, 1, 3, 0), (16, 1, 49, 0), (16, 31, 3, 0), (16, 31, 49, 0),
    (16, 32, 3, 0), (16, 32, 49, 0), (16, 33, 3, 0), (16, 33, 49, 0), (16, 511, 3, 0), (16, 511, 49, 0),
    (16, 512, 3, 0), (16, 512, 49, 0), (16, 513, 3, 0), (16, 513, 49, 0), (16, 5000, 3, 3456), (16, 5000, 49, 56448),
    (16, 100000, 3, 70656), (16, 100000, 49, 1154048), (17, 1, 3, 0), (17, 1, 49, 0), (17, 31, 3, 0), (17, 31, 49, 0),
    (17, 32, 3, 0), (17, 32, 49, 0), (17, 33, 3, 0), (17, 33, 49, 0), (17, 511, 3, 0), (17, 511, 49, 0),
    (17, 512, 3, 0), (17, 512, 49, 0), (17, 513, 3, 0), (17, 513, 49, 0), (17, 5000, 3, 3672), (17, 5000, 49, 59976),
    (17, 100000, 3, 75072), (17, 100000, 49, 1226176), (31, 1, 3, 0), (31, 1, 49, 0), (31, 31, 3, 0), (31, 31, 49, 0),
    (31, 32, 3, 0), (31, 32, 49, 0), (31, 33, 3, 0), (31, 33, 49, 0), (31, 511, 3, 0), (31, 511, 49, 0),
    (31, 512, 3, 0), (31, 512, 49, 0), (31, 513, 3, 0), (31, 513, 49, 0), (31, 5000, 3, 6696), (31, 5000, 49, 109368),
    (31, 100000, 3, 136896), (31, 100000, 49, 2235968), (32, 1, 3, 0), (32, 1, 49, 0), (32, 31, 3, 0),
    (32, 31, 49, 0), (32, 32, 3, 0), (32, 32, 49, 0), (32, 33, 3, 0), (32, 33, 49, 0), (32, 511, 3, 0),
    (32, 511, 49, 0), (32, 512, 3, 0), (32, 512, 49, 0), (32, 513, 3, 0), (32, 513, 49, 0), (32, 5000, 3, 6912),
    (32, 5000, 49, 112896), (32, 100000, 3, 141312), (32, 100000, 49, 2308096), (33, 1, 3, 0), (33, 1, 49, 0),
    (33, 31, 3, 0), (33, 31, 49, 0), (33, 32, 3, 0), (33, 32, 49, 0), (33, 33, 3, 0), (33, 33, 49, 0),
    (33, 511, 3, 0), (33, 511, 49, 0), (33, 512, 3, 0), (33, 512, 49, 0), (33, 513, 3, 0), (33, 513, 49, 0),
    (33, 5000, 3, 7128), (33, 5000, 49, 116424), (33, 100000, 3, 145728), (33, 100000, 49, 2134440), (496, 1, 3, 0),
    (496, 1, 49, 0), (496, 31, 3, 0), (496, 31, 49, 0), (496, 32, 3, 0), (496, 32, 49, 0), (496, 33, 3, 0),
    (496, 33, 49, 0), (496, 511, 3, 0), (496, 511, 49, 0), (496, 512, 3, 0), (496, 512, 49, 0), (496, 513, 3, 0),
    (496, 513, 49, 0), (496, 5000, 3, 107136), (496, 5000, 49, 1749888), (496, 100000, 3, 392832),
    (496, 100000, 49, 3110912), (497, 1, 3, 0), (497, 1, 49, 0), (497, 31, 3, 0), (497, 31, 49, 0), (497, 32, 3, 0),
    (497, 32, 49, 0), (497, 33, 3, 0), (497, 33, 49, 0), (497, 511, 3, 0), (497, 511, 49, 0), (497, 512, 3, 0),
    (497, 512, 49, 0), (497, 513, 3, 0), (497, 513, 49, 0), (497, 5000, 3, 107352), (497, 5000, 49, 1753416),
    (497, 100000, 3, 381696), (497, 100000, 49, 3117184), (512, 1, 3, 0), (512, 1, 49, 0), (512, 31, 3, 0),
    (512, 31, 49, 0), (512, 32, 3, 0), (512, 32, 49, 0), (512, 33, 3, 0), (512, 33, 49, 0), (512, 511, 3, 0),
    (512, 511, 49, 0), (512, 512, 3, 0), (512, 512, 49, 0), (512, 513, 3, 0), (512, 513, 49, 0),
    (512, 5000, 3, 110592), (512, 5000, 49, 1806336), (512, 100000, 3, 393216), (512, 100000, 49, 3211264),
    (513, 1, 3, 0), (513, 1, 49, 0), (513, 31, 3, 0), (513, 31, 49, 0), (513, 32, 3, 0), (513, 32, 49, 0),
    (513, 33, 3, 0), (513, 33, 49, 0), (513, 511, 3, 0), (513, 511, 49, 0), (513, 512, 3, 0), (513, 512, 49, 0),
    (513, 513, 3, 0), (513, 513, 49, 0), (513, 5000, 3, 110808), (513, 5000, 49, 1809864), (513, 100000, 3, 381672),
    (513, 100000, 49, 3016440),
]


def test_workspace_bytes_are_the_recorded_plan():
    ws = _lib().rmsf_pca_project_workspace_bytes
    assert [(f, n, k, ws(f, n, k)) for f, n, k, _ in PLAN_BYTES] == PLAN_BYTES


@pytest.mark.parametrize("i", [0, 1, 4])
def test_cosine_content_of_a_cosine(i):
    from rmsf_amd import cosine_content
    from rmsf_amd.pca import cosine_content as cc2
    assert cosine_content is cc2
    n = 1001
    t = np.arange(n)
    big_t = n - 1
    space = np.stack([np.cos(np.pi * (k + 1) * t / big_t) for k in range(6)], axis=1)
    assert abs(cosine_content(space, i) - 1.0) < 1e-3
    # the neighbouring index's cosine in column i: orthogonal over [0, T]
    other = space.copy()
    other[:, i] = space[:, i + 1]
    assert cosine_content(other, i) < 1e-3


def test_cosine_content_even_sample_count_and_bounds():
    from rmsf_amd import cosine_content
    n = 1000   # an odd number of intervals: the 3/8 panel closes Simpson's rule
    t = np.arange(n)
    space = np.cos(np.pi * t / (n - 1))[:, None]
    assert abs(cosine_content(space, 0) - 1.0) < 1e-3
    with pytest.raises(ValueError):
        cosine_content(space, 1)
    with pytest.raises(ValueError):
        cosine_content(space[:, 0], 0)


def test_transform_before_run_raises():
    from rmsf_amd import PCA
    p = PCA(np.zeros((4, 5, 3), dtype=np.float32), align=None)
    with pytest.raises(ValueError, match="run"):
        p.transform()


def _hand_filled(n_sel=5, n_frames=12, k=4, align="average"):
    from rmsf_amd import PCA
    from rmsf_amd.pca import pca_from_comoment
    rng = np.random.default_rng(3)
    x = rng.normal(size=(n_frames, 3 * n_sel))
    d = x - x.mean(0)
    p = PCA(np.zeros((n_frames, n_sel, 3), dtype=np.float32), align=align)
    r = p.results
    r.p_components, r.variance, r.cumulated_variance = pca_from_comoment(d.T @ d, n_frames, 1, k)
    r.mean = x.mean(0).reshape(n_sel, 3)
    r.n_frames = n_frames
    return p


@pytest.mark.parametrize("bad", [0, -1, 5, 100])
def test_transform_n_components_bounds(bad):
    p = _hand_filled(k=4)
    with pytest.raises(ValueError, match="n_components"):
        p.transform(n_components=bad)


def test_transform_of_hand_filled_results_needs_a_run():
    """In bounds, the hand-filled PCA still has no superposition to repeat:
    ValueError, not a device error."""
    p = _hand_filled(k=4)
    with pytest.raises(ValueError, match="run"):
        p.transform(n_components=2)


def test_transform_refuses_gpus_and_shards_without_a_device():
    from rmsf_amd import PCA
    q = _hand_filled()
    for p in (PCA(np.zeros((4, 5, 3), dtype=np.float32), align=None, gpus=2),
              PCA([np.zeros((4, 5, 3), dtype=np.float32)], align=None)):
        p.results.update(q.results)
        with pytest.raises(NotImplementedError, match="one device per process"):
            p.transform()
