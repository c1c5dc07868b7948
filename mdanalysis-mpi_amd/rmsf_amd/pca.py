"""``PCA`` -- the principal components of the positional covariance, named as
``MDAnalysis.analysis.pca.PCA`` names them.

The workflow RMSF.py restates (AverageStructure -> AlignTraj -> rms.RMSF) is
also the preamble of ``pca.PCA``: the covariance of the aligned coordinates,
of which the RMSF is the diagonal.  ``RMSF(..., covariance=True)`` forms that
matrix on the device (csrc/covariance.hip, the f64 matrix cores) from the
very coordinates the Welford sweep reads; the eigen-decomposition of the
[3n, 3n] f64 matrix is ``numpy.linalg.eigh`` on the host, or, with
``solver="device"``, the first modes by subspace iteration on the matrix where
it lies (rmsf_amd/eigen.py over csrc/eigen_block.hip), or, with
``solver="matrix_free"``, the same iteration over the trajectory itself with
no matrix formed at all (csrc/pca_project.hip and csrc/pca_backproject.hip).
``rmsip`` and ``cumulative_overlap`` compare two sets of modes.

``PCA.transform()`` projects a trajectory on the components, on the device
(csrc/pca_project.hip, the f64 matrix cores again): every frame is superposed
as the run's last sweep superposed it -- the same kernels, masses and
reference -- and the deviations from ``results.mean`` are contracted with the
components, batch by batch, with no aligned copy of the trajectory anywhere.
``cosine_content`` is the usual convergence measure of such a projection.

MDAnalysis is not a dependency and is absent where this was written: the
semantics of ``transform`` and ``cosine_content`` are restated from its
published documentation, not verified against it.
"""
from __future__ import annotations

import numpy as np

from .eigen import MAX_COMPONENTS, PCAConvergenceError
from .rms import RMSF, Results


def pca_from_comoment(comoment, n_frames: int, ddof: int = 1, n_components: int | None = None):
    """Principal components of the centred co-moment matrix
    ``sum_f (x_f - mean)(x_f - mean)^T`` of ``n_frames`` frames.

    Returns ``(p_components [3n, k], variance [k], cumulated_variance [k])``:
    the eigenvectors (columns) and eigenvalues of ``comoment / (n_frames -
    ddof)`` by descending eigenvalue, and the running share of the total
    variance (of all 3n components, so the full set ends at 1).  Pure numpy
    (``numpy.linalg.eigh`` on the f64 matrix)."""
    m = np.asarray(comoment, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("comoment must be a square matrix")
    if n_frames - ddof <= 0:
        raise ValueError(f"n_frames - ddof must be positive, got {n_frames} - {ddof}")
    k = m.shape[0] if n_components is None else int(n_components)
    if not 1 <= k <= m.shape[0]:
        raise ValueError(f"n_components must be in 1..{m.shape[0]}, got {n_components}")
    w, v = np.linalg.eigh(m / float(n_frames - ddof))
    order = np.argsort(w, kind="stable")[::-1]
    w, v = w[order], v[:, order]
    cumulated = np.cumsum(w) / w.sum()
    return np.ascontiguousarray(v[:, :k]), w[:k].copy(), cumulated[:k].copy()


def _simpson(y: np.ndarray) -> float:
    """Simpson's rule over samples one unit apart: the composite 1/3 rule,
    closed with one 3/8 panel when the number of intervals is odd (the
    trapezoid for two samples)."""
    y = np.asarray(y, dtype=np.float64)
    n = y.size - 1  # intervals
    if n < 1:
        return 0.0
    if n == 1:
        return 0.5 * (y[0] + y[1])
    tail = 0.0
    if n % 2:
        tail = 3.0 / 8.0 * (y[-4] + 3.0 * y[-3] + 3.0 * y[-2] + y[-1])
        y = y[:-3]
        if y.size < 3:
            return tail
    return float((y[0] + 4.0 * y[1:-1:2].sum() + 2.0 * y[2:-1:2].sum() + y[-1]) / 3.0 + tail)


def cosine_content(pca_space, i: int) -> float:
    """The cosine content of column ``i`` of a ``PCA.transform`` output
    [n_frames, k]:

        2 / T  (int_0^T cos(pi (i + 1) t / T) p_i(t) dt)^2 / int_0^T p_i(t)^2 dt

    with t the frame number and T = n_frames - 1 the length of the
    trajectory, both integrals by Simpson's rule (numpy only).  1 for a
    projection that is exactly the half-period cosine of its index -- the
    signature of random diffusion, i.e. of an unconverged simulation -- and
    near 0 for a converged one (B. Hess, Phys Rev E 65:031910, 2002).
    Restated from MDAnalysis' documentation of
    ``MDAnalysis.analysis.pca.cosine_content``, not verified against it."""
    p = np.asarray(pca_space, dtype=np.float64)
    if p.ndim != 2:
        raise ValueError("pca_space must be [n_frames, n_components]")
    if not 0 <= int(i) < p.shape[1]:
        raise ValueError(f"i must be in 0..{p.shape[1] - 1}, got {i}")
    if p.shape[0] < 2:
        raise ValueError("cosine_content needs at least 2 frames")
    col = p[:, int(i)]
    big_t = float(p.shape[0] - 1)
    cos = np.cos(np.pi * (int(i) + 1) * np.arange(p.shape[0]) / big_t)
    return float(2.0 / big_t * _simpson(cos * col) ** 2 / _simpson(col * col))


def _mode_sets(a, b, n_components):
    """The first columns of two sets of modes [n, ka], [n, kb] over the same
    coordinates, as f64."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim != 2 or b.ndim != 2:
        raise ValueError("modes must be [n_coordinates, n_components] (columns, as results.p_components)")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"the two sets of modes span {a.shape[0]} and {b.shape[0]} coordinates")
    if n_components is None:
        ka, kb = a.shape[1], b.shape[1]
    elif isinstance(n_components, (tuple, list)):
        ka, kb = (int(n) for n in n_components)
    else:
        ka = kb = int(n_components)
    if not (1 <= ka <= a.shape[1] and 1 <= kb <= b.shape[1]):
        raise ValueError(f"n_components must be in 1..{a.shape[1]} and 1..{b.shape[1]}, got {n_components}")
    return a[:, :ka], b[:, :kb]


def rmsip(a, b, n_components=None) -> float:
    """The root mean square inner product of two sets of modes, columns of
    ``a`` [n, ka] and ``b`` [n, kb] (``results.p_components`` of two runs):

        sqrt(sum_ij (a_i . b_j)^2 / ka)

    over the first ``n_components`` columns of each (an int, a pair, default
    all).  1 when orthonormal sets span the same subspace, 0 when the two are
    orthogonal (Amadei et al., Proteins 36:419, 1999).  Host numpy.  Restated
    from MDAnalysis' documentation of ``MDAnalysis.analysis.pca.rmsip``, not
    verified against it."""
    a, b = _mode_sets(a, b, n_components)
    dot = a.T @ b
    return float(np.sqrt((dot * dot).sum() / a.shape[1]))


def cumulative_overlap(a, b, i: int = 0, n_components=None) -> float:
    """How well the modes ``b`` [n, kb] (columns; the first ``n_components``,
    default all) span column ``i`` of ``a`` [n, ka]:

        sqrt(sum_j (a_i . b_j)^2 / (|a_i|^2 |b_j|^2))

    1 for a vector inside the span of orthogonal modes, 0 for one orthogonal
    to all of them.  Host numpy.  Restated from MDAnalysis' documentation of
    ``MDAnalysis.analysis.pca.cumulative_overlap``, not verified against it."""
    a, b = _mode_sets(a, b, None)
    if n_components is not None:
        if not 1 <= int(n_components) <= b.shape[1]:
            raise ValueError(f"n_components must be in 1..{b.shape[1]}, got {n_components}")
        b = b[:, :int(n_components)]
    if not 0 <= int(i) < a.shape[1]:
        raise ValueError(f"i must be in 0..{a.shape[1] - 1}, got {i}")
    vec = a[:, int(i)]
    norms = np.sqrt((vec * vec).sum()) * np.sqrt((b * b).sum(axis=0))
    if not np.all(norms > 0.0):
        raise ValueError("cumulative_overlap of a zero vector")
    o = np.abs(vec @ b) / norms
    return float(np.sqrt((o * o).sum()))


_ONE_DEVICE = "PCA.transform runs on one device per process: not "
_PLANES = ('PCA.transform reads (frame, atom, xyz) rows; HBM-resident coordinate planes are not supported -- pass '
           'the trajectory with layout="fac"')


def check_projection_memory(eng, n_frames: int, n_comp: int) -> None:
    """MemoryError if the [F, k] f64 projection is over half the free HBM."""
    import torch

    need = 8 * n_frames * n_comp
    free = torch.cuda.mem_get_info(eng.device)[0]
    if need > free // 2:
        raise MemoryError(f"PCA.transform: the [{n_frames}, {n_comp}] f64 projection needs {need} bytes, over half "
                          f"of the {free} bytes of free HBM")


def refuse_one_device(rmsf, atomgroup, what: str = "PCA.transform") -> None:
    """What reads the trajectory of ``rmsf`` (an ``RMSF``) or ``atomgroup`` on
    one device per process -- ``PCA.transform``, ``PCA(solver="matrix_free")``,
    ``TICA`` (``what``) -- refuses, before any launch."""
    import torch

    from . import parallel
    from .sources import DeviceSource

    one_device = _ONE_DEVICE.replace("PCA.transform", what)
    r = rmsf
    for x in (r._input, atomgroup):
        if isinstance(x, (list, tuple)):
            raise NotImplementedError(one_device + "with gpus= or a list of shards")
    if r.gpus is not None:
        raise NotImplementedError(one_device + "with gpus= or a list of shards")
    x = r._input if atomgroup is None else atomgroup
    if (isinstance(x, DeviceSource) and x.layout == "soa") or (
            isinstance(x, torch.Tensor) and x.device.type == "cuda" and r.layout == "soa"):
        raise NotImplementedError(_PLANES.replace("PCA.transform", what))
    if parallel.world()[1] > 1:
        raise NotImplementedError(one_device + "under torch.distributed with more than one rank")


def project_on_components(rmsf, comps, mean, what: str, atomgroup=None, n_components: int | None = None,
                          start=None, stop=None, step=None, frames=None, as_tensor: bool = False):
    """``PCA.transform``'s path, for any [3n, k] set of columns ``comps`` and
    any ``mean`` [n, 3] over the selection of ``rmsf`` (the ``RMSF`` whose run
    supplied the superposition): see ``PCA.transform``.  ``what`` names the
    caller in the messages."""
    if comps is None:
        raise ValueError(f"{what} needs the components: call run() first (the non-root ranks of a "
                         "reduce-to-root merge hold none)")
    k_total = int(comps.shape[1])
    k = k_total if n_components is None else int(n_components)
    if not 1 <= k <= k_total:
        raise ValueError(f"n_components must be in 1..{k_total}, got {n_components}")
    refuse_one_device(rmsf, atomgroup, what)
    r = rmsf
    last = r._last_run
    if last is None:
        # results filled in by hand (components kept from an earlier run): without alignment there is
        # no superposition to repeat, and the PCA's own input can be projected
        if r.align is not None:
            raise ValueError(f"{what} needs the superposition of run(): these results were not computed "
                             "by run() on this object")
        last = {"source": None, "frames": None, "masses": None, "device": r.device, "exact": False,
                "ref": None, "refinfo": None}

    import torch

    from ._lib import RMSF_XFORM_DOUBLES
    from .engine import Engine
    from .pipeline import Superposer
    from .rms import make_source
    from .sources import DeviceSource, FrameList

    eng = Engine(last["device"])
    with torch.cuda.device(eng.device):
        if atomgroup is None and last["source"] is None:
            atomgroup = r._input
        if atomgroup is None:
            src = last["source"]
            same = start is None and stop is None and step is None and frames is None
            fl = last["frames"] if same else FrameList(src.n_traj, start, stop, step, frames=frames)
        else:
            src, _ = make_source(atomgroup, select=r.select, masses=r.masses, align=None,
                                 batch_frames=r.batch_frames, layout=r.layout, group_masses=False)
            fl = FrameList(src.n_traj, start, stop, step, frames=frames)
        if isinstance(src, DeviceSource) and src.layout == "soa":
            raise NotImplementedError(_PLANES.replace("PCA.transform", what))
        n_sel = src.n_sel
        if 3 * n_sel != comps.shape[0]:
            raise ValueError(f"the input selects {n_sel} atoms, the components were computed for "
                             f"{comps.shape[0] // 3}")
        n_frames = len(fl)
        check_projection_memory(eng, n_frames, k)
        out = eng.empty(n_frames, k)
        if n_frames == 0:
            return out if as_tensor else out.cpu().numpy()
        mean = torch.as_tensor(np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)).to(eng.device)
        comp = torch.as_tensor(np.ascontiguousarray(comps, dtype=np.float64)).to(eng.device)
        max_batch = max(1, min(r.batch_frames or n_frames, n_frames))
        aligned = r.align is not None
        exact = bool(last["exact"])
        ref, info = last["ref"], last["refinfo"]
        m_dev, mass_total, sup, xf = None, float(n_sel), None, None
        if aligned:
            masses = last["masses"]
            if masses is not None:
                m_np = np.ascontiguousarray(masses, dtype=np.float64)
                mass_total = float(m_np.sum())  # numpy's own sum, as the exact run's (pipeline._run_exact)
                m_dev = torch.as_tensor(m_np).to(eng.device)
            if exact:
                xf = eng.empty(max_batch, RMSF_XFORM_DOUBLES)
            else:
                sup = Superposer(eng, n_sel, max_batch, m_dev)
        work, done = None, 0
        for b in src.batches(fl, 0, n_frames, max_batch, eng.stream):
            if b.pstride:
                raise NotImplementedError(_PLANES.replace("PCA.transform", what))
            x = None
            if aligned and exact:
                x = xf[:b.n_frames]
                eng.superpose_seq(b.ptr, b.fstride, b.n_frames, n_sel, b.sel, m_dev, mass_total, ref, info, x)
            elif aligned:
                x = sup.run(b, ref, info)
            need = eng.pca_project_workspace_bytes(b.n_frames, n_sel, k)
            if need and (work is None or need > work.numel() * 8):  # not monotone in the batch size
                work = eng.empty((need + 7) // 8)
            eng.pca_project(b.ptr, b.fstride, b.n_frames, n_sel, b.sel, x, info if x is not None else None,
                            mean, comp, k, out[done:done + b.n_frames], work if need else None)
            done += b.n_frames
            b.done()
        if done != n_frames:
            raise RuntimeError(f"the source yielded {done} of {n_frames} frames")
        torch.cuda.current_stream(eng.device).synchronize()
        return out if as_tensor else out.cpu().numpy()


class PCA:
    """Principal component analysis of a trajectory's selected coordinates.

    ``PCA(atomgroup, select=..., align="average").run()`` runs
    ``RMSF(..., covariance=True)`` (every other keyword goes to ``RMSF``) and
    fills, as ``MDAnalysis.analysis.pca.PCA`` does:

    ``results.p_components``  [3n, k] eigenvectors of the covariance (columns),
    ``results.variance``      [k] their eigenvalues, descending,
    ``results.cumulated_variance``  [k] running share of the total variance,

    and ``results.mean`` [n, 3], ``results.rmsf`` [n], ``results.covariance``
    [3n, 3n] (co-moment / (n_frames - ddof), as ``pca.PCA`` divides; ddof=1)
    and ``results.n_frames``.  Coordinate order 3 a + c over the selection's
    order.  Under ``torch.distributed`` with ``merge_root`` the other ranks'
    results are None.

    ``transform()`` then gives the projection of the trajectory (or of
    another one) on the components, f64 [n_frames, k].

    ``solver="host"`` (the default) is ``numpy.linalg.eigh`` of the whole
    matrix on the host.  ``solver="device"`` keeps the matrix in HBM and finds
    the first ``n_components`` (required, 1..40) modes there by blocked
    subspace iteration (``rmsf_amd.eigen.top_eigenpairs``; ``tol``,
    ``max_iter`` and ``seed`` are its keywords).  Then ``results.covariance``
    is the HBM ``torch.Tensor`` [3n, 3n] -- ``.cpu()`` is the caller's call --
    while ``results.p_components`` and ``results.variance`` are host numpy as
    with ``"host"`` (each component's largest entry positive),
    ``results.cumulated_variance`` divides by the trace of the device matrix,
    and ``results.solver_info`` is the solver's record (``n_iter``,
    ``residuals``, ``rank``, ``block``, ``converged``).  A matrix with fewer
    than ``n_components`` significant directions (a one-frame run) or an
    iteration that does not converge raises ``PCAConvergenceError``.  Every
    rank that holds the matrix runs the same deterministic solve.

    ``solver="matrix_free"`` runs the same iteration with no [3n, 3n] matrix
    anywhere: ``RMSF`` without the covariance gives the mean, and the product
    M Q = D^T (D Q) / (n_frames - ddof) is taken from the trajectory itself
    (``rmsf_amd.eigen.TrajectoryOps``: csrc/pca_project.hip and its adjoint
    csrc/pca_backproject.hip, two reads of the frames per iteration, O(3n b)
    memory), so the selection may be as large as the trajectory that fits --
    the covariance's memory check is never asked.  ``n_components`` (1..40),
    ``tol``, ``max_iter``, ``seed``, ``results.p_components``, ``variance`` and
    ``solver_info`` are as with ``"device"``; ``results.covariance`` is None,
    and ``cumulated_variance`` divides by the trace taken from the Welford
    sums, ``results.sumsquares.sum() / (n_frames - ddof)``.  Fewer than
    ``n_components`` directions (n_frames - ddof < n_components) raise
    ``PCAConvergenceError``.  One device per process, as ``transform()``:
    ``gpus=``, lists of shards, HBM-resident ``layout="soa"`` planes and more
    than one ``torch.distributed`` rank are NotImplementedError before any
    launch.  ``transform()`` works after it as after the other solvers.
    """

    def __init__(self, atomgroup, select=None, align="average", n_components: int | None = None, ddof: int = 1,
                 solver: str = "host", tol: float = 1e-10, max_iter: int = 300, seed: int = 0, **rmsf_kwargs):
        if solver not in ("host", "device", "matrix_free"):
            raise ValueError(f'solver must be "host", "device" or "matrix_free", got {solver!r}')
        if solver != "host":
            if n_components is None:
                raise ValueError(f'solver="{solver}" computes the first n_components modes: give n_components (a '
                                 'full decomposition is solver="host"\'s job)')
            if not 1 <= int(n_components) <= MAX_COMPONENTS:
                raise ValueError(f'solver="{solver}" computes 1..{MAX_COMPONENTS} components, got {n_components}; '
                                 'use solver="host" for more')
        rmsf_kwargs.pop("covariance", None)
        self.n_components = n_components
        self.ddof = int(ddof)
        self.solver, self.tol, self.max_iter, self.seed = solver, float(tol), int(max_iter), int(seed)
        self._rmsf = RMSF(atomgroup, select=select, align=align, covariance=solver != "matrix_free", **rmsf_kwargs)
        self._rmsf._comoment_stays_in_hbm = solver == "device"
        self._rmsf._keep_last_run = solver == "matrix_free"
        self.results = Results()

    def _run_device(self, start, stop, step, frames, **kwargs):
        """``run()`` with ``solver="device"``: the finished co-moment stays
        in HBM, is divided in place and handed to ``top_eigenpairs``."""
        from .eigen import block_width, top_eigenpairs
        from .engine import Engine

        rm = self._rmsf
        r = rm.run(start, stop, step, frames=frames, **kwargs).results
        out = self.results
        out.n_frames = r.n_frames
        out.mean, out.rmsf = r.mean, r.rmsf
        cov, rm._comoment_hbm = rm._comoment_hbm, None
        if cov is None:  # a non-root rank of a reduce-to-root merge
            out.covariance = out.p_components = out.variance = out.cumulated_variance = out.solver_info = None
            return self
        k = int(self.n_components)
        if r.n_frames - self.ddof <= 0:  # one frame: the co-moment is exactly zero and there is nothing to divide by
            info = {"n_iter": 0, "residuals": np.full(k, np.inf), "rank": 0, "block": 0, "converged": False}
            out.solver_info = info
            raise PCAConvergenceError(f"asked for {k} components, the matrix has rank 0: {r.n_frames} frame(s) with "
                                      f"ddof = {self.ddof} leave no covariance", info)
        block_width(cov.shape[0], k)  # ValueError for k > 3n, before any launch
        import torch

        eng = Engine(cov.device)
        with torch.cuda.device(eng.device):
            flat = cov.view(-1)
            eng.divide(flat, float(r.n_frames - self.ddof), flat)  # x / d element by element, in place
            out.covariance = cov
            trace = float(cov.diagonal().cpu().numpy().sum())
            out.variance, out.p_components, out.solver_info = top_eigenpairs(
                cov, k, tol=self.tol, max_iter=self.max_iter, seed=self.seed)
        out.cumulated_variance = np.cumsum(out.variance) / trace
        self.n_frames = r.n_frames
        return self

    def _run_matrix_free(self, start, stop, step, frames, **kwargs):
        """``run()`` with ``solver="matrix_free"``: ``RMSF`` without the
        covariance for the mean, the RMSF and the last sweep's reference, then
        ``top_eigenpairs`` over ``TrajectoryOps``.  No [3n, 3n] matrix is
        formed and ``check_covariance_memory`` is never asked."""
        from .eigen import TrajectoryOps, block_width, top_eigenpairs

        self._refuse_transform(None, 'PCA(solver="matrix_free")')  # before any launch
        rm = self._rmsf
        r = rm.run(start, stop, step, frames=frames, **kwargs).results
        out = self.results
        out.n_frames = r.n_frames
        out.mean, out.rmsf = r.mean, r.rmsf
        out.covariance = None
        k = int(self.n_components)
        denom = r.n_frames - self.ddof
        if denom <= 0:  # one frame: every deviation is zero and there is nothing to divide by
            info = {"n_iter": 0, "residuals": np.full(k, np.inf), "rank": 0, "block": 0, "converged": False}
            out.solver_info = info
            raise PCAConvergenceError(f"asked for {k} components, the matrix has rank 0: {r.n_frames} frame(s) with "
                                      f"ddof = {self.ddof} leave no covariance", info)
        block_width(r.mean.size, k)  # ValueError for k > 3n, before any launch
        last = rm._last_run
        import torch

        with torch.cuda.device(last["device"]):
            ops = TrajectoryOps(last["source"], last["frames"], r.mean, float(denom), masses=last["masses"],
                                aligned=rm.align is not None, exact=last["exact"], ref=last["ref"],
                                refinfo=last["refinfo"], batch_frames=rm.batch_frames, device=last["device"])
            out.variance, out.p_components, out.solver_info = top_eigenpairs(
                None, k, tol=self.tol, max_iter=self.max_iter, seed=self.seed, ops=ops)
        # the matrix's trace from the Welford sums: sum_i sum_f d_i(f)^2 / (F - ddof)
        trace = float(np.asarray(r.sumsquares, dtype=np.float64).sum()) / float(denom)
        out.cumulated_variance = np.cumsum(out.variance) / trace
        self.n_frames = r.n_frames
        return self

    def run(self, start=None, stop=None, step=None, frames=None, **kwargs):
        if self.solver == "device":
            return self._run_device(start, stop, step, frames, **kwargs)
        if self.solver == "matrix_free":
            return self._run_matrix_free(start, stop, step, frames, **kwargs)
        r = self._rmsf.run(start, stop, step, frames=frames, **kwargs).results
        out = self.results
        out.n_frames = r.n_frames
        out.mean, out.rmsf = r.mean, r.rmsf
        if r.comoment is None:  # a non-root rank of a reduce-to-root merge
            out.covariance = out.p_components = out.variance = out.cumulated_variance = None
            return self
        out.p_components, out.variance, out.cumulated_variance = pca_from_comoment(
            r.comoment, r.n_frames, self.ddof, self.n_components)
        out.covariance = r.comoment / float(r.n_frames - self.ddof)
        self.n_frames = r.n_frames
        return self

    def _refuse_transform(self, atomgroup, what: str = "PCA.transform") -> None:
        """What ``transform`` -- and ``solver="matrix_free"``, which reads the
        trajectory the same way (``what``) -- refuses, before any launch."""
        refuse_one_device(self._rmsf, atomgroup, what)

    def transform(self, atomgroup=None, n_components: int | None = None, start=None, stop=None, step=None,
                  frames=None, as_tensor: bool = False):
        """The projection of a trajectory on the first ``n_components``
        components (default: all that ``run()`` computed): host f64
        [n_frames, n_components], or the HBM tensor with ``as_tensor=True``.

            proj[f, c] = sum_i (x_i(f) - results.mean_i) results.p_components[i, c]

        ``atomgroup=None``: the input ``run()`` read, and its frame list
        unless ``start``/``stop``/``step``/``frames`` give another.  Any other
        input takes what ``RMSF`` takes, with the PCA's ``select``, ``masses``
        and ``layout``, and must select as many atoms (ValueError).

        With ``align`` set, each frame x(f) is superposed exactly as the run's
        last sweep superposed it: the same masses, the same device reference
        (the all-reduced average, or frame ``ref_frame`` of the run's
        trajectory), the same entry points -- rmsf_superpose on the
        frame-parallel path, rmsf_superpose_sequential when the run was exact
        -- and the same f32 transform inside the projection kernel, so the
        trajectory ``run()`` read is projected from the very bits its
        covariance was formed from.  Frames stream through in batches of
        ``batch_frames``; a dense HBM tensor is read in place.  ``run()``'s
        source stays alive on the PCA for this (a host input's staged frames
        in HBM included).  Results filled in by hand (components kept from
        an earlier session) can be projected on without a ``run()`` only for
        ``align=None``: there is no superposition to repeat.

        One device per process: ``gpus=``, lists of shards, HBM-resident
        ``layout="soa"`` planes and a ``torch.distributed`` world of more than
        one rank are NotImplementedError; a projection over half the free HBM
        is a MemoryError."""
        return project_on_components(self._rmsf, self.results.get("p_components"), self.results.get("mean"),
                                     "PCA.transform", atomgroup, n_components, start, stop, step, frames, as_tensor)
