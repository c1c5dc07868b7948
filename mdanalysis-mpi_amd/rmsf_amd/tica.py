"""``TICA`` -- time-lagged independent component analysis: the slowest
motions of a trajectory's selected coordinates (Perez-Hernandez et al.,
J. Chem. Phys. 139:015102, 2013; Schwantes & Pande, J. Chem. Theory Comput.
9:2000, 2013), the first step of a Markov-model pipeline.

PCA diagonalises the covariance of the (aligned) coordinates; TICA asks which
of their combinations decorrelate slowest, which needs the covariance of the
frames with the frames ``lag`` positions later as well.  With N = F - lag
pairs, d(t) the deviations from a shift near the data, and the reversible
(symmetrised) estimator:

    T  = sum_{t<N} d(t) + sum_{t>=lag} d(t)                 mu = shift + T / 2N
    M0 = sum_{t<N} d d^T + sum_{t>=lag} d d^T - T T^T / 2N  C0 = M0 / 2N
    Mt = S + S^T - T T^T / 2N,  S = sum_{t<N} d(t) d(t+lag)^T   Ct = Mt / 2N
    Ct v = lambda C0 v

M0 and T are two calls of the covariance kernel (csrc/covariance.hip), one
per window, into one matrix; S is that file's tile body again, the same
contraction on the f64 matrix cores with its operands ``lag`` frames apart, and all three
read the superposed coordinates the Welford sweep read, with no aligned copy
of the trajectory.  The generalised eigenproblem is solved on the host
(``tica_from_comoments``, numpy); ``TICA.transform`` is ``PCA.transform``'s
projection (csrc/pca_project.hip) with mu and the components.

Not here: the non-reversible (Koopman) estimator, a device-side generalised
eigen-solve, several lags in one pass, multi-device and multi-rank runs.
"""
from __future__ import annotations

import numpy as np

from .eigen import fix_signs
from .pca import project_on_components, refuse_one_device
from .rms import RMSF, Results


def tica_from_comoments(m0, m_lag, n_pairs: int, lag: int, n_components: int | None = None, epsilon: float = 1e-6):
    """The TICA modes of the symmetrised co-moment matrices ``m0`` = 2N C0
    and ``m_lag`` = 2N C_lag of ``n_pairs`` = N frame pairs ``lag`` apart.

    Returns ``(eigenvalues [k], timescales [k], components [3n, k],
    kinetic_variance [k], rank)``.  ``eigh(C0)`` first: the eigenvalues
    ``> epsilon * max`` are kept (their count is ``rank``) -- a superposed
    trajectory has exactly six null directions in C0, the linear constraints
    of the optimal fit, and this truncation is what handles them.  With L = U
    Lambda^-1/2 on the kept directions, ``eigh`` of the symmetrised L^T C_lag
    L gives the eigenvalues, descending, and ``components = L W`` with V^T C0
    V = I, each column's largest entry positive (``eigen.fix_signs``).
    ``timescales = -lag / ln |lambda|`` in frames of the list, ``inf`` where
    ``|lambda| >= 1`` and ``nan`` where ``lambda = 0``;
    ``kinetic_variance = cumsum(lambda^2) / sum`` over all ``rank`` of them.
    ``n_components`` (default: ``rank``) over ``rank`` is a ValueError.  Pure
    numpy."""
    m0 = np.asarray(m0, dtype=np.float64)
    mt = np.asarray(m_lag, dtype=np.float64)
    if m0.ndim != 2 or m0.shape[0] != m0.shape[1] or mt.shape != m0.shape:
        raise ValueError("m0 and m_lag must be square matrices of one shape")
    if int(n_pairs) < 1:
        raise ValueError(f"n_pairs must be positive, got {n_pairs}")
    if int(lag) < 1:
        raise ValueError(f"lag must be at least 1, got {lag}")
    if not 0.0 < float(epsilon) < 1.0:
        raise ValueError(f"epsilon must be in (0, 1), got {epsilon}")
    if n_components is not None and int(n_components) < 1:
        raise ValueError(f"n_components must be at least 1, got {n_components}")
    if not (np.all(np.isfinite(m0)) and np.all(np.isfinite(mt))):
        raise ValueError("the matrices have non-finite entries")
    denom = 2.0 * float(n_pairs)
    c0 = 0.5 * (m0 + m0.T) / denom
    ct = 0.5 * (mt + mt.T) / denom
    s, u = np.linalg.eigh(c0)
    s, u = s[::-1], u[:, ::-1]
    keep = s > float(epsilon) * s[0] if s[0] > 0.0 else np.zeros(s.shape, bool)
    rank = int(keep.sum())
    k = rank if n_components is None else int(n_components)
    if k > rank:
        raise ValueError(f"n_components = {k} is over the rank {rank} of C0 (epsilon = {epsilon})")
    if rank == 0:
        raise ValueError("C0 is zero: no direction to keep")
    el = u[:, keep] / np.sqrt(s[keep])
    a = el.T @ ct @ el
    w, v = np.linalg.eigh(0.5 * (a + a.T))
    order = np.argsort(w, kind="stable")[::-1]
    w, v = w[order], v[:, order]
    comps = fix_signs(el @ v[:, :k])
    with np.errstate(divide="ignore", invalid="ignore"):
        ts = -float(lag) / np.log(np.abs(w))
    ts = np.where(np.abs(w) >= 1.0, np.inf, ts)
    ts = np.where(w == 0.0, np.nan, ts)
    total = float((w * w).sum())
    kv = np.cumsum(w * w) / total if total > 0.0 else np.full(w.shape, np.nan)
    return w[:k].copy(), ts[:k].copy(), np.ascontiguousarray(comps), kv[:k].copy(), rank


def check_tica_memory(eng, n_sel: int, n_frames: int, resident_copy: bool) -> None:
    """MemoryError if the two [3n, 3n] f64 matrices plus the resident f32
    copy of the frames (when one is made) are over half the free HBM."""
    import torch

    n = 3 * n_sel
    need = 2 * 8 * n * n + (12 * n_sel * n_frames if resident_copy else 0)
    free = torch.cuda.mem_get_info(eng.device)[0]
    if need > free // 2:
        raise MemoryError(f"TICA: two [{n}, {n}] f64 matrices"
                          + (f" and the resident [{n_frames}, {n_sel}, 3] f32 frames" if resident_copy else "")
                          + f" need {need} bytes, over half of the {free} bytes of free HBM")


def _in_place(src, fl):
    """(first frame, step) when ``src`` is a dense HBM ``fac`` tensor and the
    list ``fl`` one arithmetic run of its frames, else None."""
    from .sources import DeviceSource
    if not isinstance(src, DeviceSource) or src.layout != "fac" or len(fl) < 1:
        return None
    runs = list(fl.runs(0, len(fl), len(fl)))
    if len(runs) != 1:
        return None
    first, step, n = runs[0]
    if not (src.holds(first) and src.holds(first + step * (n - 1))):
        return None
    return first, step


class TICA:
    """Time-lagged independent component analysis of a trajectory's selected
    coordinates, with the reversible estimator of the module's docstring.

    ``TICA(atomgroup, lag, select=..., align="average").run()`` runs ``RMSF``
    (every other keyword goes to it) for the reference, the masses and the
    exactness of the superposition, computes every frame's transform record
    once as that run's last sweep did, and fills

    ``results.eigenvalues``       [k] lambda, descending: the autocorrelation
                                  of each component at the lag,
    ``results.timescales``        [k] -lag / ln |lambda|, in list positions,
    ``results.components``        [3n, k] columns v with V^T C0 V = I,
    ``results.kinetic_variance``  [k] running share of sum lambda^2,

    and ``results.mean`` [n, 3] (mu, the mean over both windows),
    ``results.rank`` (directions of C0 kept: 3n - 6 for a superposed
    trajectory), ``results.n_frames``, ``results.n_pairs``, ``results.lag``;
    with ``keep_matrices=True`` also ``results.cov0`` and ``results.cov_lag``,
    host f64 [3n, 3n].  Coordinate order 3 a + c over the selection's order.

    ``lag`` counts positions in the run's frame list: pair t is the list's
    frames t and t + lag.  It is a time lag only for a uniform list (a
    ``start``/``stop``/``step`` range, or evenly spaced ``frames``).

    A dense HBM tensor (``layout="fac"``, a range of frames) is read in
    place.  Any other source -- host arrays, XTC and DCD files, AtomGroups,
    scattered frame lists -- is streamed once into a resident dense f32 [F,
    n_sel, 3] copy in list order: a pair may straddle any batch boundary, so
    the batches cannot be contracted one at a time.  The two matrices and
    that copy over half the free HBM are a MemoryError.

    ``transform()`` projects a trajectory on the components as
    ``PCA.transform`` does.  One device per process: ``gpus=``, lists of
    shards, HBM-resident ``layout="soa"`` planes and more than one
    ``torch.distributed`` rank are NotImplementedError before any launch;
    ``lag < 1`` or ``lag >= n_frames`` is a ValueError."""

    def __init__(self, atomgroup, lag: int, select=None, align="average", n_components: int | None = None,
                 epsilon: float = 1e-6, keep_matrices: bool = False, **rmsf_kwargs):
        if int(lag) != lag or int(lag) < 1:
            raise ValueError(f"lag must be an integer of at least 1, got {lag!r}")
        if n_components is not None and int(n_components) < 1:
            raise ValueError(f"n_components must be at least 1, got {n_components}")
        if not 0.0 < float(epsilon) < 1.0:
            raise ValueError(f"epsilon must be in (0, 1), got {epsilon}")
        rmsf_kwargs.pop("covariance", None)
        self.lag = int(lag)
        self.n_components = None if n_components is None else int(n_components)
        self.epsilon = float(epsilon)
        self.keep_matrices = bool(keep_matrices)
        self._rmsf = RMSF(atomgroup, select=select, align=align, **rmsf_kwargs)
        self._rmsf._keep_last_run = True
        self.results = Results()

    def run(self, start=None, stop=None, step=None, frames=None, **kwargs):
        import torch

        from .engine import Engine
        from .eigen import TrajectoryOps
        from .pipeline import _covariance_shift
        from .sources import DeviceSource, FrameList

        rm = self._rmsf
        refuse_one_device(rm, None, "TICA")  # before any launch
        # The frame source is made here and handed to RMSF as its input, so the
        # length of the list and the selection's size are known -- and the lag
        # and the memory checked -- before anything is launched.
        eng = Engine(rm.device)
        with torch.cuda.device(eng.device):
            src, masses = rm._make_source(eng)
            fl = FrameList(src.n_traj, start, stop, step, frames=frames)
            n_frames, lag = len(fl), self.lag
            if lag >= n_frames:
                raise ValueError(f"lag = {lag} leaves no pair of frames: the run has {n_frames} frame(s)")
            n_pairs = n_frames - lag
            n_sel = int(src.n_sel)
            n = 3 * n_sel
            place = _in_place(src, fl)
            check_tica_memory(eng, n_sel, n_frames, place is None)
        rm._input, rm.masses = src, masses
        r = rm.run(start, stop, step, frames=frames, **kwargs).results
        last = rm._last_run
        aligned = rm.align is not None
        with torch.cuda.device(eng.device):
            if place is None:
                # every frame of the list, selected, once: [F, n_sel, 3] f32 in list order
                copy = eng.empty(n_frames, n_sel, 3, dtype=torch.float32)
                max_batch = max(1, min(int(rm.batch_frames or n_frames), n_frames))
                rows = torch.arange(max_batch, dtype=torch.int64, device=eng.device)
                done = 0
                for b in src.batches(fl, 0, n_frames, max_batch, eng.stream):
                    if b.pstride:
                        raise NotImplementedError("TICA reads (frame, atom, xyz) rows; coordinate planes are not "
                                                  'supported -- pass the trajectory with layout="fac"')
                    eng.gather_frames(b.ptr, b.fstride, rows, b.n_frames, n_sel, b.sel, copy[done:done + b.n_frames])
                    done += b.n_frames
                    b.done()
                if done != n_frames:
                    raise RuntimeError(f"the source yielded {done} of {n_frames} frames")
                dense, dense_fl = DeviceSource(copy), FrameList(n_frames)
                ptr, fstride, sel = copy.data_ptr(), 3 * n_sel, None
            else:
                dense, dense_fl = src, fl
                ptr, fstride, sel = src._ptr(place[0]), src.fstride * place[1], src.sel_dev
            records = None
            if aligned:
                # every frame's transform record, once, by the entry points of the run's last sweep
                ops = TrajectoryOps(dense, dense_fl, np.zeros(n), 1.0, masses=last["masses"], aligned=True,
                                    exact=last["exact"], ref=last["ref"], refinfo=last["refinfo"],
                                    batch_frames=rm.batch_frames, engine=eng)
                records = ops._superpose_all()
            info = last["refinfo"] if aligned else None
            average = None
            if rm.align == "average":
                average = torch.as_tensor(np.ascontiguousarray(r.average, dtype=np.float64)).to(eng.device)
            shift = _covariance_shift(eng, src, fl, rm.align, average, last["ref"], last["refinfo"]).contiguous()
            b_ptr = ptr + 4 * lag * fstride
            xa = None if records is None else records[:n_pairs]
            xb = None if records is None else records[lag:]
            # M0 and T: the covariance kernel over the two windows, into one matrix
            cov0, t = eng.zeros(n, n), eng.zeros(n)
            need = max(eng.covariance_workspace_bytes(n_sel, n_pairs),
                       eng.lagged_comoment_workspace_bytes(n_sel, n_pairs))
            work = eng.empty((need + 7) // 8) if need else None
            eng.covariance_accumulate(ptr, fstride, n_pairs, n_sel, sel, xa, info, shift, cov0, t, work)
            eng.covariance_accumulate(b_ptr, fstride, n_pairs, n_sel, sel, xb, info, shift, cov0, t, work)
            eng.covariance_finish(cov0, t, n, 2 * n_pairs)
            # S, then M_lag = S + S^T - T T^T / 2N
            cov_lag = eng.zeros(n, n)
            eng.lagged_comoment_accumulate(ptr, fstride, b_ptr, fstride, n_pairs, n_sel, sel, xa, xb, info, shift,
                                           cov_lag, work)
            eng.lagged_comoment_finish(cov_lag, t, n, 2 * n_pairs)
            torch.cuda.current_stream(eng.device).synchronize()
            m0, mt = cov0.cpu().numpy(), cov_lag.cpu().numpy()
            mean = shift.cpu().numpy() + t.cpu().numpy() / (2.0 * n_pairs)
            del cov0, cov_lag, records
        out = self.results
        out.n_frames, out.n_pairs, out.lag = n_frames, n_pairs, lag
        out.mean = mean.reshape(n_sel, 3)
        if self.keep_matrices:
            out.cov0, out.cov_lag = m0 / (2.0 * n_pairs), mt / (2.0 * n_pairs)
        out.eigenvalues, out.timescales, out.components, out.kinetic_variance, out.rank = tica_from_comoments(
            m0, mt, n_pairs, lag, self.n_components, self.epsilon)
        self.n_frames = n_frames
        return self

    def transform(self, atomgroup=None, n_components: int | None = None, start=None, stop=None, step=None,
                  frames=None, as_tensor: bool = False):
        """The projection of a trajectory on the first ``n_components``
        components (default: all that ``run()`` kept), f64 [n_frames, k]:

            proj[f, c] = sum_i (x_i(f) - results.mean_i) results.components[i, c]

        ``PCA.transform``'s path and rules: each frame is superposed as the
        run's last sweep superposed it and contracted on the f64 matrix cores
        (csrc/pca_project.hip); ``atomgroup=None`` is the input ``run()`` read.
        Over the run's own frames each column has symmetrised variance 1 and
        symmetrised autocorrelation ``results.eigenvalues[c]`` at the lag."""
        return project_on_components(self._rmsf, self.results.get("components"), self.results.get("mean"),
                                     "TICA.transform", atomgroup, n_components, start, stop, step, frames, as_tensor)
