"""The planted trajectories of the diffusion-map tests (tests/test_diffusion_host.py
on the CPU, tests/test_gpu_diffusion.py on the device), their RMSD matrix in
numpy and the host path's formulae restated.

Two kinds, 40 atoms, f32, each frame under a random rotation about its centroid
and a translation (the generator of tests/test_gpu_clustering.py):

  * "states": four conformations, a base structure plus each state's own
    displacement of 1.0 / 1.6 / 2.2 / 2.8 A per atom (unequal, so that the three
    slow modes that tell the states apart are not degenerate), 0.3 A noise;
    populations 40 / 30 / 20 / 10 per cent, shuffled.
  * "path": a curved path, base + 3 A (cos(pi s) u1 + sin(pi s) u2) with s
    uniform in [0, 1] along the frames and 0.2 A noise -- the spectrum of a
    one-dimensional diffusion, with gaps between its first modes.

``EPS_FACTOR``: epsilon as a multiple of the median squared distance of the
case's matrix (the diagonal included).
"""
import functools

import numpy as np

N_ATOMS = 40
K = 3                              # diffusion coordinates the end-to-end tests ask for
CASES = [("states", 130), ("path", 130), ("states", 353), ("path", 353)]
EPS_FACTOR = {"states": 1.0, "path": 0.25}
STATE_SIGMA = (1.0, 1.6, 2.2, 2.8)
STATE_NOISE, PATH_RADIUS, PATH_NOISE = 0.3, 3.0, 0.2


def _unit(d: np.ndarray) -> np.ndarray:
    """Displacement fields scaled to 1 A per atom (rms)."""
    return d / np.sqrt((d ** 2).sum(axis=(-2, -1), keepdims=True) / d.shape[-2])


@functools.lru_cache(maxsize=None)
def planted(kind: str, n_frames: int) -> np.ndarray:
    """f32 [n_frames, N_ATOMS, 3], read-only."""
    rng = np.random.default_rng(1000 * n_frames + 7 * N_ATOMS + len(kind))
    base = rng.uniform(0.0, 100.0, size=(N_ATOMS, 3))
    if kind == "states":
        disp = _unit(rng.normal(size=(4, N_ATOMS, 3))) * np.asarray(STATE_SIGMA)[:, None, None]
        counts = np.floor(np.array([0.4, 0.3, 0.2, 0.1]) * n_frames).astype(int)
        counts[0] += n_frames - counts.sum()
        state = rng.permutation(np.repeat(np.arange(4), counts))
        x = base + disp[state] + STATE_NOISE * rng.normal(size=(n_frames, N_ATOMS, 3))
    elif kind == "path":
        u = _unit(rng.normal(size=(2, N_ATOMS, 3)))
        s = np.pi * np.arange(n_frames) / (n_frames - 1)
        x = (base + PATH_RADIUS * (np.cos(s)[:, None, None] * u[0] + np.sin(s)[:, None, None] * u[1])
             + PATH_NOISE * rng.normal(size=(n_frames, N_ATOMS, 3)))
    else:
        raise ValueError(kind)
    q = rng.normal(size=(n_frames, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, a, b, c = q.T
    rot = np.stack([np.stack([1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)], -1),
                    np.stack([2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)], -1),
                    np.stack([2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)], -1)], -2)
    cen = x.mean(axis=1, keepdims=True)
    x = np.einsum("fac,fcd->fad", x - cen, rot) + cen + rng.uniform(-5.0, 5.0, size=(n_frames, 1, 3))
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def numpy_distances(kind: str, n_frames: int) -> np.ndarray:
    """The minimal RMSD of every pair of ``planted``'s frames in numpy f64
    (Kabsch by SVD, no QCP): symmetric in its bits, zero diagonal, read-only."""
    x = planted(kind, n_frames).astype(np.float64)
    d = x - x.mean(axis=1, keepdims=True)
    g = (d * d).sum(axis=(1, 2))
    h = np.einsum("jac,iad->ijcd", d, d)
    u, s, vt = np.linalg.svd(h)
    tr = s[..., 0] + s[..., 1] + np.sign(np.linalg.det(u @ vt)) * s[..., 2]
    sq = np.maximum(g[:, None] + g[None, :] - 2.0 * tr, 0.0) / N_ATOMS
    m = np.sqrt(0.5 * (sq + sq.T))
    np.fill_diagonal(m, 0.0)
    m.setflags(write=False)
    return m


def epsilon_of(kind: str, d: np.ndarray) -> float:
    return float(EPS_FACTOR[kind] * np.median(d * d))


def host_formulae(d: np.ndarray, epsilon: float):
    """``DiffusionMap(solver="host")`` restated literally: (eigenvalues [F]
    descending, right eigenvectors [F, F], the conjugate matrix D^-1/2 K D^-1/2,
    t = rowsum^-1/2, the conjugate's own orthonormal eigenvectors)."""
    k = np.exp(-(d * d) / epsilon)
    rs = 1.0 / np.sqrt(k.sum(axis=1))
    sym = k * rs[:, None] * rs[None, :]
    sym = 0.5 * (sym + sym.T)
    w, v = np.linalg.eigh(sym)
    order = np.argsort(w, kind="stable")[::-1]
    w, v = w[order], v[:, order]
    right = v * rs[:, None]
    if right.shape[0] and right[:, 0].sum() < 0:
        right[:, 0] = -right[:, 0]
    return w, np.ascontiguousarray(right), sym, rs, v


def aligned(v: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """The columns of ``v`` with the signs that bring each nearest ``ref``'s."""
    s = np.sign((v * ref).sum(axis=0))
    s[s == 0] = 1.0
    return v * s
