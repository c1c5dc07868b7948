"""``top_eigenpairs`` -- the first k eigenpairs of a symmetric positive
semi-definite f64 matrix by blocked subspace iteration with Rayleigh-Ritz.

The matrix is touched through three block products only,

    symm(Q)               Y = M Q              [n, b]   the n^2-sized one
    gram(A, B)            A^T B                [b, b]   on the host
    update(alpha, A, B, T)  alpha A + B T      [n, .]   T a host [b, .] matrix

so the same driver runs over ``DeviceOps`` (csrc/eigen_block.hip on the f64
matrix cores, the matrix and every block in HBM) and over ``NumpyOps`` (the
whole iteration, its stopping rule and its breakdown paths on the CPU).
``TrajectoryOps`` overrides ``symm`` alone: M Q = D^T (D Q) / denom from the
trajectory's frames (csrc/pca_project.hip and csrc/pca_backproject.hip), so no
n x n matrix exists at all; ``FactorOps`` is its numpy twin.  ``KernelOps``
does the same for M = diag(t) K diag(t) with K in HBM (csrc/diffusion.hip's
row scaling around ``DeviceOps``' product; ``DiffusionMap(solver="device")``),
and ``ScaledOps`` is its numpy twin.  The
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


class FactorOps(NumpyOps):
    """The numpy twin of ``TrajectoryOps``: the matrix D^T D / denom through
    its factor ``d`` [F, n] alone, ``symm(q) = d.T @ (d @ q) / denom``.  The
    n x n matrix is never formed."""

    def __init__(self, d, denom: float):
        d = np.asarray(d, dtype=np.float64)
        if d.ndim != 2:
            raise ValueError("d must be [n_frames, n]")
        if not float(denom) > 0.0:
            raise ValueError(f"denom must be positive, got {denom}")
        self.d, self.denom, self.n = d, float(denom), d.shape[1]

    def symm(self, q):
        return self.d.T @ (self.d @ q) / self.denom


class ScaledOps(NumpyOps):
    """The numpy twin of ``KernelOps``: the matrix diag(t) K diag(t) through
    K and t alone, ``symm(q) = t * (K @ (t * q))``.  The scaled matrix is
    never formed."""

    def __init__(self, matrix, t):
        super().__init__(matrix)
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        if t.size != self.n:
            raise ValueError(f"t must have {self.n} entries, got {t.size}")
        self.t = t

    def symm(self, q):
        return self.t[:, None] * (self.m @ (self.t[:, None] * q))


class KernelOps(DeviceOps):
    """A diagonally scaled matrix as an operator:

        symm(Q) = diag(t) K (diag(t) Q)

    with K [n, n] (symmetric in its bits) and t [n], both f64 in HBM: one
    ``block_scale_rows``, ``DeviceOps``' product with K, a second
    ``block_scale_rows`` in place.  diag(t) K diag(t) is never written.
    With K a diffusion kernel and t = rowsum^-1/2 that is the symmetric
    conjugate of the transition matrix (``DiffusionMap(solver="device")``).
    ``put``, ``get``, ``gram`` and ``update`` are ``DeviceOps``' own."""

    def __init__(self, matrix, t, engine=None):
        import torch
        super().__init__(matrix, engine)
        if not isinstance(t, torch.Tensor) or t.device != matrix.device or t.dtype != torch.float64 \
                or t.dim() != 1 or t.shape[0] != self.n or not t.is_contiguous():
            raise ValueError(f"t must be a contiguous f64 HIP tensor [{self.n}] on the matrix's device")
        self.t = t

    def symm(self, q):
        b = int(q.shape[1])
        tq = self.eng.empty(self.n, b)
        self.eng.block_scale_rows(self.t, q, self.n, b, tq)
        y = super().symm(tq)
        self.eng.block_scale_rows(self.t, y, self.n, b, y)
        return y


_TRAJ_ONE_DEVICE = "the matrix-free product runs on one device per process: not "
_TRAJ_PLANES = ('the matrix-free product reads (frame, atom, xyz) rows; HBM-resident coordinate planes are not '
                'supported -- pass the trajectory with layout="fac"')


class TrajectoryOps(DeviceOps):
    """The covariance as an operator on the trajectory, with no [n, n] matrix
    anywhere (n = 3 n_sel):

        symm(Q) = D^T (D Q) / denom,   D[f, i] = x_i(f) - mean[i]

    where x(f) is frame f's selected coordinates, superposed exactly as the
    run's last sweep superposed them when ``aligned`` -- the rows
    ``PCA.transform`` projects.  D Q is csrc/pca_project.hip, its adjoint
    csrc/pca_backproject.hip, both on the f64 matrix cores, batch by batch in
    the source's order; ``put``, ``get``, ``gram`` and ``update`` are
    ``DeviceOps``' own and need only n.

    ``source``, ``frames``: the frame source and ``FrameList`` of the run
    (``RMSF._last_run``), with its ``masses``, device ``ref`` / ``refinfo``
    and ``exact``.  ``mean``: f64 [n] (host or HBM), ``denom``: n_frames -
    ddof.  ``batch_frames`` bounds a batch, and with it the scratch P_b
    [batch, b]; default: every frame at once for a source that yields them so
    -- 8 b F bytes, under the trajectory's own 12 n_sel F from 32 atoms on.

    With ``aligned`` every frame's transform record is computed once, on the
    first product, into an HBM [F, RMSF_XFORM_DOUBLES] tensor -- by
    ``Superposer.run`` on the frame-parallel path, ``superpose_seq`` when the
    run was exact, as ``PCA.transform`` computes them -- and later products
    read the records: an iteration costs two reads of a batch, not four.

    One device per process: HBM-resident ``layout="soa"`` planes and a
    ``torch.distributed`` world of more than one rank are NotImplementedError
    before any launch."""

    def __init__(self, source, frames, mean, denom: float, *, masses=None, aligned: bool = False, exact: bool = False,
                 ref=None, refinfo=None, batch_frames: int | None = None, engine=None, device=None):
        import torch

        from . import parallel
        from .engine import Engine
        from .sources import DeviceSource
        if isinstance(source, (list, tuple)):
            raise NotImplementedError(_TRAJ_ONE_DEVICE + "with gpus= or a list of shards")
        if isinstance(source, DeviceSource) and source.layout == "soa":
            raise NotImplementedError(_TRAJ_PLANES)
        if parallel.world()[1] > 1:
            raise NotImplementedError(_TRAJ_ONE_DEVICE + "under torch.distributed with more than one rank")
        if not float(denom) > 0.0:
            raise ValueError(f"denom must be positive, got {denom}")
        if aligned and (ref is None or refinfo is None):
            raise ValueError("an aligned product needs the run's device reference (ref, refinfo)")
        self.eng = engine or Engine(device)
        self.src, self.frames = source, frames
        self.n_sel, self.n = int(source.n_sel), 3 * int(source.n_sel)
        self.n_frames = len(frames)
        self.denom = float(denom)
        self.aligned, self.exact = bool(aligned), bool(exact)
        self.ref, self.refinfo, self.masses = ref, refinfo, masses
        self.max_batch = max(1, min(int(batch_frames or self.n_frames or 1), max(1, self.n_frames)))
        if isinstance(mean, torch.Tensor):
            mean = mean.detach().cpu().numpy()
        m = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        if m.size != self.n:
            raise ValueError(f"mean must have {self.n} entries, got {m.size}")
        with torch.cuda.device(self.eng.device):
            self.mean = torch.as_tensor(m).to(self.eng.device)
        self._work = self._p = self._records = None

    def _batches(self):
        return self.src.batches(self.frames, 0, self.n_frames, self.max_batch, self.eng.stream)

    def _superpose_all(self):
        """Every frame's transform record, once: [F, RMSF_XFORM_DOUBLES]."""
        import torch

        from ._lib import RMSF_XFORM_DOUBLES
        from .pipeline import Superposer
        eng, n_sel = self.eng, self.n_sel
        rec = eng.empty(max(1, self.n_frames), RMSF_XFORM_DOUBLES)
        m_dev, mass_total, sup = None, float(n_sel), None
        if self.masses is not None:
            m_np = np.ascontiguousarray(self.masses, dtype=np.float64)
            mass_total = float(m_np.sum())  # numpy's own sum, as the exact run's (pipeline._run_exact)
            m_dev = torch.as_tensor(m_np).to(eng.device)
        if not self.exact:
            sup = Superposer(eng, n_sel, self.max_batch, m_dev)
        done = 0
        for b in self._batches():
            if b.pstride:
                raise NotImplementedError(_TRAJ_PLANES)
            x = rec[done:done + b.n_frames]
            if self.exact:
                eng.superpose_seq(b.ptr, b.fstride, b.n_frames, n_sel, b.sel, m_dev, mass_total, self.ref,
                                  self.refinfo, x)
            else:
                x.copy_(sup.run(b, self.ref, self.refinfo))
            done += b.n_frames
            b.done()
        if done != self.n_frames:
            raise RuntimeError(f"the source yielded {done} of {self.n_frames} frames")
        return rec

    def symm(self, q):
        import torch

        eng, n_sel = self.eng, self.n_sel
        b_cols = int(q.shape[1])
        with torch.cuda.device(eng.device):
            if self.aligned and self._records is None:
                self._records = self._superpose_all()
            if self._p is None or self._p.shape[1] < b_cols:
                self._p = eng.empty(self.max_batch, max(b_cols, MAX_BLOCK))
            y = eng.empty(self.n, b_cols)
            done = 0
            for i, b in enumerate(self._batches()):
                if b.pstride:
                    raise NotImplementedError(_TRAJ_PLANES)
                x = self._records[done:done + b.n_frames] if self.aligned else None
                info = self.refinfo if self.aligned else None
                need = max(eng.pca_project_workspace_bytes(b.n_frames, n_sel, b_cols),
                           eng.pca_backproject_workspace_bytes(b.n_frames, n_sel, b_cols))
                work = self._scratch(need)  # the two launches follow each other on one stream
                eng.pca_project(b.ptr, b.fstride, b.n_frames, n_sel, b.sel, x, info, self.mean, q, b_cols, self._p,
                                work)
                eng.pca_backproject(b.ptr, b.fstride, b.n_frames, n_sel, b.sel, x, info, self.mean, self._p, b_cols,
                                    y, i > 0, work)
                done += b.n_frames
                b.done()
            if done != self.n_frames:
                raise RuntimeError(f"the source yielded {done} of {self.n_frames} frames")
            if done == 0:
                y.zero_()
            flat = y.view(-1)
            eng.divide(flat, self.denom, flat)
        return y


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
