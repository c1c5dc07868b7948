"""``top_eigenpairs`` -- the first k eigenpairs of a symmetric positive
semi-definite f64 matrix by blocked subspace iteration with Rayleigh-Ritz.

The matrix is touched through three block products only,

    symm(Q)               Y = M Q              [n, b]   the n^2-sized one
    gram(A, B)            A^T B                [b, b]   on the host
    update(alpha, A, B, T)  alpha A + B T      [n, .]   T a host [b, .] matrix

so the same driver runs over ``DeviceOps`` (csrc/eigen_block.hip on the f64
matrix cores, the matrix and every block in HBM) and over ``NumpyOps`` (the
whole iteration, its stopping rule and its breakdown paths on the CPU).  The
b x b steps -- ``numpy.linalg.eigh`` of a Gram matrix or of the projected
matrix -- run on the host: a few stream synchronisations per iteration.

One iteration, from an orthonormal block Q:

    Y = M Q;  H = sym(Q^T Y);  H = S diag(L) S^T, L descending  (Rayleigh-Ritz)
    W = Y - Q H;  |r_i|^2 = s_i^T (W^T W) s_i                   (explicit residuals)
    stop when max_{i<k} |r_i| <= tol L_1
    Q = orth(Y)

``s_i^T (Y^T Y) s_i - L_i^2`` is the same number on paper and cancels at
sqrt(eps) L_1; it is not used.  ``orth`` is two passes of SVQB (Stathopoulos &
Wu, SIAM J. Sci. Comput. 23:2165, 2002): G = Y^T Y scaled to unit diagonal,
``eigh``, the directions with d <= b 2^-52 d_max dropped (zero columns), so a
rank-deficient matrix -- fewer frames than b -- loses columns where a
Cholesky-QR would break down.  The count kept is the numerical rank.
"""
from __future__ import annotations

import numpy as np

MAX_BLOCK = 48       # columns of a block: three tiles of the f64 MFMA (csrc/eigen_block.hip)
MAX_COMPONENTS = 40  # k + 8 guard vectors, rounded up to whole tiles, must fit a block
EPS = 2.0 ** -52


class PCAConvergenceError(RuntimeError):
    """The device eigen-solver gave up: the matrix has fewer than k
    significant directions, or ``max_iter`` was reached.  ``info`` is the
    solver's record at that point."""

    def __init__(self, message: str, info: dict):
        super().__init__(message)
        self.info = info


def block_width(n: int, k: int) -> int:
    """b = min(n, 16 ceil((k + 8) / 16), 48): k and 8 guard vectors in whole
    MFMA tiles.  ValueError for a k no block holds (k > 40, or k > n)."""
    n, k = int(n), int(k)
    if n < 1:
        raise ValueError(f"the matrix must have at least one row, got {n}")
    if k < 1:
        raise ValueError(f"n_components must be at least 1, got {k}")
    if k > MAX_COMPONENTS or k > n:
        raise ValueError(f"the device eigen-solver computes at most min({MAX_COMPONENTS}, n = {n}) components, got "
                         f'{k}; use solver="host" for more')
    return min(n, 16 * ((k + 8 + 15) // 16), MAX_BLOCK)


def sym(g: np.ndarray) -> np.ndarray:
    """(G + G^T) / 2: the driver symmetrises every b x b product itself and
    relies on no symmetry of ``gram``'s bits."""
    return 0.5 * (g + g.T)


class NumpyOps:
    """The three block products in numpy: blocks are host arrays."""

    def __init__(self, matrix):
        m = np.asarray(matrix, dtype=np.float64)
        if m.ndim != 2 or m.shape[0] != m.shape[1]:
            raise ValueError("matrix must be square")
        self.m, self.n = m, m.shape[0]

    def put(self, x: np.ndarray):
        return np.array(x, dtype=np.float64)

    def get(self, x) -> np.ndarray:
        return np.array(x)

    def symm(self, q):
        return self.m @ q

    def gram(self, a, b) -> np.ndarray:
        return a.T @ b

    def update(self, alpha: float, a, b, t: np.ndarray):
        bt = b @ t
        return bt if a is None else alpha * a + bt


class DeviceOps:
    """The three block products on the device (Engine.symm_block,
    block_gram, block_update): ``matrix`` is an HBM f64 tensor [n, n],
    symmetric in its bits; blocks are HBM tensors, Gram matrices come back as
    host arrays (one synchronisation each)."""

    def __init__(self, matrix, engine=None):
        import torch

        from .engine import Engine
        if not isinstance(matrix, torch.Tensor) or matrix.device.type != "cuda" or matrix.dtype != torch.float64 \
                or matrix.dim() != 2 or matrix.shape[0] != matrix.shape[1] or matrix.stride(1) != 1:
            raise ValueError("matrix must be a square f64 HIP tensor with contiguous rows")
        self.eng = engine or Engine(matrix.device)
        self.m, self.n = matrix, int(matrix.shape[0])
        self._work = None

    def _scratch(self, need: int):
        if not need:
            return None
        if self._work is None or need > self._work.numel() * 8:
            self._work = self.eng.empty((need + 7) // 8)
        return self._work

    def put(self, x: np.ndarray):
        import torch
        return torch.as_tensor(np.array(x, dtype=np.float64, order="C")).to(self.eng.device)

    def get(self, x) -> np.ndarray:
        return x.cpu().numpy()

    def symm(self, q):
        b = int(q.shape[1])
        y = self.eng.empty(self.n, b)
        self.eng.symm_block(self.m, self.n, q, b, y, self._scratch(self.eng.symm_block_workspace_bytes(self.n, b)))
        return y

    def gram(self, a, b) -> np.ndarray:
        na, nb = int(a.shape[1]), int(b.shape[1])
        g = self.eng.empty(na, nb)
        self.eng.block_gram(a, na, b, nb, self.n, g,
                            self._scratch(self.eng.block_gram_workspace_bytes(self.n, na, nb)))
        return g.cpu().numpy()

    def update(self, alpha: float, a, b, t: np.ndarray):
        nb, nc = t.shape
        c = self.eng.empty(self.n, nc)
        self.eng.block_update(alpha, a, b, nb, self.put(t), self.n, nc, c)
        return c


def svqb_transform(g: np.ndarray):
    """(T [b, b], rank) of one SVQB pass: with G = Y^T Y, Y T has ``rank``
    orthonormal columns followed by zero columns.  G is scaled to unit
    diagonal (D), ``eigh`` gives d and V, the directions with d > b 2^-52
    d_max are kept, strongest first: T = D^-1 V d_kept^-1/2."""
    b = g.shape[0]
    if not np.all(np.isfinite(g)):
        raise ValueError("the matrix has non-finite entries")
    g = sym(g)
    t = np.zeros((b, b))
    diag = np.diagonal(g)
    live = diag > 0.0
    if not live.any():
        return t, 0
    s = np.zeros(b)
    s[live] = 1.0 / np.sqrt(diag[live])
    d, v = np.linalg.eigh(g * s[:, None] * s[None, :])
    keep = np.nonzero(d > b * EPS * d.max())[0][::-1]
    t[:, :keep.size] = s[:, None] * v[:, keep] / np.sqrt(d[keep])[None, :]
    return t, int(keep.size)


def _orthonormalise(ops, y):
    """Two SVQB passes; (Q, numerical rank of y)."""
    t, rank = svqb_transform(ops.gram(y, y))
    q = ops.update(0.0, None, y, t)
    t, _ = svqb_transform(ops.gram(q, q))
    return ops.update(0.0, None, q, t), rank


def fix_signs(v: np.ndarray) -> np.ndarray:
    """Each column's component of largest magnitude (the first on ties) made
    positive."""
    v = np.array(v, dtype=np.float64)
    if v.size:
        j = np.argmax(np.abs(v), axis=0)
        neg = v[j, np.arange(v.shape[1])] < 0.0
        v[:, neg] = -v[:, neg]
    return v


def top_eigenpairs(matrix, k: int, *, block: int | None = None, tol: float = 1e-10, max_iter: int = 300,
                   seed: int = 0, ops=None):
    """``(values [k], vectors [n, k], info)``: the k largest eigenvalues of
    the symmetric positive semi-definite ``matrix``, descending, and their
    orthonormal eigenvectors (columns, signs fixed by ``fix_signs``), host
    f64.  ``matrix``: an HBM f64 tensor symmetric in its bits (``DeviceOps``)
    or a host array (``NumpyOps``); ``ops`` overrides the choice.

    ``block``: the block width (default ``block_width(n, k)``; k <= 40).
    ``tol``: stop when every one of the k residuals |M v - l v| is at most
    ``tol`` times the largest eigenvalue.  The f64 floor of that ratio is of
    order n 2^-53, so the default 1e-10 is attainable at every size that fits
    HBM.  ``seed``: of the Gaussian start block
    ``numpy.random.default_rng(seed).standard_normal((n, b))``; the solve is
    deterministic.

    ``info``: ``n_iter`` (products with the matrix), ``residuals`` [k]
    (relative to the largest eigenvalue), ``rank`` (the numerical rank of the
    last M Q, at most the block width), ``block``, ``converged``.

    ValueError for a k no block holds, before any device work;
    ``PCAConvergenceError`` (carrying ``info``) when the matrix has fewer than
    k significant directions -- the all-zero matrix included -- or when
    ``max_iter`` is reached."""
    k = int(k)
    if ops is None:
        n = int(matrix.shape[0])
        b = block_width(n, k) if block is None else int(block)
        ops = NumpyOps(matrix) if isinstance(matrix, np.ndarray) else DeviceOps(matrix)
    else:
        n = int(ops.n)
        b = block_width(n, k) if block is None else int(block)
    if not k <= b <= min(n, MAX_BLOCK):
        raise ValueError(f"block must be in {k}..{min(n, MAX_BLOCK)}, got {b}")
    if int(max_iter) < 1:
        raise ValueError(f"max_iter must be at least 1, got {max_iter}")

    info = {"n_iter": 0, "residuals": np.full(k, np.inf), "rank": 0, "block": b, "converged": False}
    q, _ = _orthonormalise(ops, ops.put(np.random.default_rng(seed).standard_normal((n, b))))
    for it in range(1, int(max_iter) + 1):
        y = ops.symm(q)
        h = sym(ops.gram(q, y))
        lam, s = np.linalg.eigh(h)
        lam, s = lam[::-1], s[:, ::-1]
        w = ops.update(1.0, y, q, -h)
        gw = sym(ops.gram(w, w))
        res = np.sqrt(np.maximum(np.einsum("ji,jl,li->i", s[:, :k], gw, s[:, :k]), 0.0))
        t, rank = svqb_transform(ops.gram(y, y))
        info.update(n_iter=it, rank=rank)
        if rank < k:
            raise PCAConvergenceError(
                f"asked for {k} components, the matrix has rank {rank}: ask for fewer, or use solver=\"host\" for "
                "the full decomposition", info)
        info["residuals"] = res / lam[0]
        if res.max() <= tol * lam[0]:
            info["converged"] = True
            break
        q = ops.update(0.0, None, y, t)
        t, _ = svqb_transform(ops.gram(q, q))
        q = ops.update(0.0, None, q, t)
    if not info["converged"]:
        raise PCAConvergenceError(
            f"no convergence in max_iter = {max_iter} iterations: the largest of the {k} residuals is "
            f"{info['residuals'].max():.3e} of the largest eigenvalue, tol = {tol:.3e}.  The likely cause is a "
            f"flat tail of the spectrum around component {k}: raise max_iter, ask for fewer components, or use "
            'solver="host"', info)
    vectors = fix_signs(ops.get(ops.update(0.0, None, q, np.ascontiguousarray(s[:, :k]))))
    return lam[:k].copy(), vectors, info
