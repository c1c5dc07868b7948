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
