"""Frames at which the largest root of the QCP quartic is double, triple or
nearly so -- the data of tests/test_gpu_pairwise_degenerate.py (GPU tier) and
tests/test_pair_lambda_host.py (CPU tier).  Not a test module.

With s0 >= s1 >= s2 the singular values of a pair's 3 x 3 matrix A and sigma
the sign of its determinant, the 4 x 4 key matrix has the eigenvalues s0 + s1
+ sigma s2, s0 - s1 - sigma s2, -s0 + s1 - sigma s2, -s0 - s1 + sigma s2; the
two largest differ by 2 (s1 + sigma s2).  That gap closes when

  * A has rank 1 -- either frame has its atoms on a line (``L``, ``Ls``,
    ``C5``, ``C3``, ``C1``; every frame of two atoms) -- or rank 0 (``COL``, all
    atoms at one point);
  * s1 = s2 and sigma = -1: ``S`` has s0 = s1 = s2 (the vertices of nested
    cubes) and ``I0`` .. ``I2`` are its point reflection, rotated, with noise
    0, 1e-6, 1e-4 and 1e-2 A -- a triple root at no noise;
  * s2 = 0: ``P``, ``PR``, ``PM`` are planar (a double root exactly).

``G``, ``mG`` (= -G), ``G2``, ``G3`` are generic; ``Z0``, ``Z1`` all zero.
Every frame but those two is rotated where its name says so and translated by
a few A.  Frames are generated in f64 and cast to f32; the references work
from the f32 values.

The weights are multiples of 1/4 and the collapsed frame's point is dyadic, so
that its weighted centre is that point exactly and its G exactly 0, on the
device and in numpy alike; within one cube they take two values, one per
inscribed tetrahedron, which keeps s0 = s1 = s2 of ``S`` under weights.

The point-like frames (``COL``, ``Z0``, ``Z1``) have G = 0, so for a pair of
them the bound 1e-12 (G_i + G_j) / (2 sum w) is 0: the distance has to be
exact.  Superposed it is 0.  Without superposition it is the distance of the
two points, computed about frame 0's centre: ``Z0`` is frame 0 (the origin)
and the collapsed frames sit at 1.25 (2, -1, 2) and 0.75 (2, -1, 2), whose
lengths (3.75, 2.25) and distance (1.5) are dyadic, so every sum, the square
root and its square are exact.
"""
import functools

import numpy as np

ORDER = {
    # 16 frames in the first tile, 4 in the second: (S, I6), (L, C3), (Z0, Z1) meet
    # in the off-diagonal tile, (S, I0), (S, I4), (L, Ls), (L, C5) in a diagonal one
    20: ("Z0", "G", "L", "I0", "C5", "P", "mG", "I2", "Ls", "PM", "S", "C1", "G2", "PR", "I4", "COL",
         "I6", "C3", "Z1", "G3"),
    # one frame in the second tile: (S, I4) meets there
    17: ("Z0", "G", "L", "I0", "C5", "P", "mG", "I2", "Ls", "PM", "S", "C1", "Z1", "I6", "C3", "COL",
         "I4"),
    5: ("Z0", "L", "G", "COL", "S"),
}
# (family, first frame, the frames it is paired with): gap of the two largest
# eigenvalues of the key matrix < 1e-4 of the largest
FLAGGED = (("inverted eps=0", "S", ("I0",)), ("inverted eps=1e-6", "S", ("I6",)),
           ("inverted eps=1e-4", "S", ("I4",)), ("collinear", "L", ("Ls", "C5", "C3", "C1")),
           ("collapsed", "COL", ("G", "S", "P")))
CUBE = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
CUBE_SIZES = (4.0, 1.5, 2.25, 3.0, 5.5)


def rotation(rng) -> np.ndarray:
    q = rng.normal(size=4)
    w, a, b, c = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)],
                     [2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)],
                     [2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)]])


@functools.lru_cache(maxsize=None)
def weights_of(n_sel: int) -> np.ndarray:
    """Multiples of 1/4 in [1, 16]; in a cube of ``S`` one value per tetrahedron."""
    rng = np.random.default_rng(100 + n_sel)
    if n_sel % 8:
        w = rng.integers(4, 65, size=n_sel) / 4.0
    else:
        even = CUBE.prod(axis=1) > 0
        w = np.concatenate([np.where(even, *(rng.integers(4, 65, size=2) / 4.0)) for _ in range(n_sel // 8)])
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def frames_by_name(n_sel: int, seed: int) -> dict:
    """name -> f64 [n_sel, 3]; n_sel = 8 or 40 (S needs whole cubes)."""
    assert n_sel % 8 == 0 and n_sel // 8 <= len(CUBE_SIZES)
    rng = np.random.default_rng(7000 + 10 * n_sel + seed)
    noise = lambda: rng.normal(size=(n_sel, 3))                       # noqa: E731
    shift = lambda: rng.uniform(-5.0, 5.0, size=(1, 3))               # noqa: E731
    g = rng.uniform(-8.0, 8.0, size=(n_sel, 3))
    s = np.concatenate([r * CUBE for r in CUBE_SIZES[:n_sel // 8]])
    line = rng.uniform(-15.0, 15.0, size=(n_sel, 1)) * (np.array([[2.0, -1.0, 0.5]]) / np.sqrt(5.25))
    p = np.concatenate([rng.uniform(-8.0, 8.0, size=(n_sel, 2)), np.zeros((n_sel, 1))], axis=1)
    out = {"G": g + shift(), "mG": -g + shift(), "S": s + shift(), "L": line + shift(), "P": p + shift(),
           "G2": rng.uniform(-8.0, 8.0, size=(n_sel, 3)) + shift(),
           "G3": rng.uniform(-8.0, 8.0, size=(n_sel, 3)) + shift()}
    for name, eps in (("I0", 0.0), ("I6", 1e-6), ("I4", 1e-4), ("I2", 1e-2)):
        out[name] = -(s + eps * noise()) @ rotation(rng) + shift()
    out["Ls"] = 1.05 * line @ rotation(rng) + shift()
    for name, eps in (("C5", 1e-5), ("C3", 1e-3), ("C1", 1e-1)):
        out[name] = (line + eps * noise()) @ rotation(rng) + shift()
    out["PR"] = p @ rotation(rng) + shift()
    out["PM"] = (p * np.array([[-1.0, 1.0, 1.0]])) @ rotation(rng) + shift()
    out["COL"] = np.tile((0.75 if seed else 1.25) * np.array([[2.0, -1.0, 2.0]]), (n_sel, 1))
    out["Z0"] = out["Z1"] = np.zeros((n_sel, 3))
    return out


@functools.lru_cache(maxsize=None)
def zoo(n_frames: int, n_sel: int, gathered: bool, seed: int = 0) -> np.ndarray:
    """f32 [n_frames, n_atoms, 3]: the frames of ORDER[n_frames]; gathered:
    in rows 1, 4, 7, ... of 3 n_sel atoms, random rows between them."""
    f = frames_by_name(n_sel, seed)
    x = np.stack([f[name] for name in ORDER[n_frames]])
    if gathered:
        wide = np.random.default_rng(seed).uniform(-50.0, 50.0, size=(n_frames, 3 * n_sel, 3))
        wide[:, 1::3] = x
        x = wide
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def few_atoms(n_frames: int, n_sel: int, gathered: bool) -> np.ndarray:
    """f32 [n_frames, n_atoms, 3] of 1 or 2 selected atoms: every pair of
    frames is degenerate (rank 1, or rank 0)."""
    rng = np.random.default_rng(40 + n_sel)
    x = rng.uniform(-10.0, 10.0, size=(n_frames, 3 * n_sel if gathered else n_sel, 3)).astype(np.float32)
    x.setflags(write=False)
    return x


def selection(n_sel: int, gathered: bool):
    return np.arange(1, 3 * n_sel, 3) if gathered else None


def index_of(n_frames: int, name: str) -> int:
    return ORDER[n_frames].index(name)


def pair_inputs(xa: np.ndarray, xb: np.ndarray, w=None):
    """(A [F_a, F_b, 9], E0 [F_a, F_b], sum w) of the selected rows xa [F_a, n,
    3], xb [F_b, n, 3] in numpy f64, as the kernels define them: A_ij = sum_a
    w_a d_i,a d_j,a^T about each frame's weighted centre, E0 = (G_i + G_j) / 2."""
    xa, xb = xa.astype(np.float64), xb.astype(np.float64)
    n = xa.shape[1]
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    wt = w.sum()
    wc = w[None, :, None]
    da = xa - (wc * xa).sum(axis=1, keepdims=True) / wt
    db = xb - (wc * xb).sum(axis=1, keepdims=True) / wt
    ga, gb = (wc * da * da).sum(axis=(1, 2)), (wc * db * db).sum(axis=(1, 2))
    a = np.einsum("iac,jad->ijcd", wc * da, db).reshape(len(xa), len(xb), 9)
    return a, 0.5 * (ga[:, None] + gb[None, :]), wt


def key_eigenvalues(a: np.ndarray) -> np.ndarray:
    """The eigenvalues, ascending, of the key matrix of A [..., 9]."""
    sxx, sxy, sxz, syx, syy, syz, szx, szy, szz = np.moveaxis(np.asarray(a, dtype=np.float64), -1, 0)
    k = np.array([[sxx + syy + szz, syz - szy, szx - sxz, sxy - syx],
                  [syz - szy, sxx - syy - szz, sxy + syx, szx + sxz],
                  [szx - sxz, sxy + syx, -sxx + syy - szz, syz + szy],
                  [sxy - syx, szx + sxz, syz + szy, -sxx - syy + szz]])
    return np.linalg.eigvalsh(np.moveaxis(k, (0, 1), (-2, -1)))


def assert_degenerate(a: np.ndarray, label: str) -> None:
    """The two largest eigenvalues of the key matrix of every A [..., 9]
    differ by at most 1e-4 of the largest."""
    ev = key_eigenvalues(a)
    gap, top = ev[..., 3] - ev[..., 2], ev[..., 3]
    assert np.all(gap <= 1e-4 * top), f"{label}: not degenerate: gap / largest = {np.max(gap / top):.3e}"


def svd_sq(a: np.ndarray, e0: np.ndarray, wt: float) -> np.ndarray:
    """d^2 = 2 (E0 - (s0 + s1 + sigma s2)) / sum w from the SVD of A [..., 9]."""
    u, s, vt = np.linalg.svd(np.asarray(a, dtype=np.float64).reshape(a.shape[:-1] + (3, 3)))
    sign = np.sign(np.linalg.det(u @ vt))
    return 2.0 * (e0 - (s[..., 0] + s[..., 1] + sign * s[..., 2])) / wt
