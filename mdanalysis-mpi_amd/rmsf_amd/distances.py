"""``DistanceMatrix`` and ``DiffusionMap`` -- the frame-by-frame view of a
trajectory, named as ``MDAnalysis.analysis.diffusionmap`` names them.

``DistanceMatrix(ag).run().results.dist_matrix`` is the F x F matrix of RMSDs
between every pair of frames ("2D RMSD").  On the CPU that is F^2 / 2 QCP
superpositions; here it is the covariance kernel turned on its side
(csrc/pairwise.hip): the 3 x 3 inner product of frames i and j is one block of
the Gram matrix X W X^T, contracted over the atoms on the f64 matrix cores,
and each pair's RMSD comes from the QCP quartic's largest root in the same
kernel -- no rotation, no 9 F^2 intermediate, every pair once.

``DiffusionMap`` is the eigen-decomposition of the diffusion kernel of that
matrix, on the host (numpy only, like ``pca_from_comoment``).

MDAnalysis is not a dependency and is absent where this was written: its
semantics (``DistanceMatrix``'s metric and cutoff, ``rms.rmsd``'s weights,
``DiffusionMap``'s kernel and ``transform``) are restated from its published
documentation, not verified against it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import parallel
from .engine import Engine
from .rms import Results, make_source
from .sources import DeviceSource, FrameList

_PW_PLANES = ('DistanceMatrix reads (frame, atom, xyz) rows; HBM-resident coordinate planes are not supported -- '
              'pass the trajectory with layout="fac"')
MAX_GATHER = 65535  # frames one rmsf_gather_frames launch takes


def check_pairwise_memory(eng: Engine, n_frames: int, dense_bytes: int = 0) -> None:
    """MemoryError if the [F, F] f64 result plus the dense copy of the
    selected rows (when one is made) is over half the free HBM."""
    need = 8 * n_frames * n_frames
    free = torch.cuda.mem_get_info(eng.device)[0]
    if need + dense_bytes > free // 2:
        raise MemoryError(f"DistanceMatrix: the [{n_frames}, {n_frames}] f64 matrix needs {need} bytes"
                          + (f" and the dense copy of the selected rows {dense_bytes} bytes" if dense_bytes else "")
                          + f", over half of the {free} bytes of free HBM")


def _check_weights(weights, n_sel: int):
    """None, or the f64 [n_sel] weights -- ValueError for a wrong length or a
    weight that is not positive (and finite)."""
    if weights is None:
        return None
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w.size != n_sel:
        raise ValueError(f"weights must have one entry per selected atom ({n_sel}), got {w.size}")
    if not np.all(np.isfinite(w)) or not np.all(w > 0.0):
        raise ValueError("weights must be positive and finite")
    return w


def _check_n_sel(n_sel: int) -> None:
    if n_sel < 3:
        raise ValueError(f"DistanceMatrix needs at least 3 selected atoms, got {n_sel}: the superposition of fewer "
                         "is degenerate")


class DistanceMatrix:
    """All-pairs RMSD matrix of a trajectory's frames, ``results.dist_matrix``
    (host f64 [F, F], symmetric in its bits, zero diagonal).

    Parameters
    ----------
    atomgroup : MDAnalysis AtomGroup | np.ndarray | torch.Tensor | path | frame source
        The inputs of ``RMSF``: a float32 trajectory [F, n_atoms, 3] on the
        host or in HBM, an ``.xtc`` / ``.dcd`` path, an AtomGroup.
    select : array of int, optional
        Atom indices (array and file inputs); default all atoms.
    weights : None | "mass" | array [n_sel]
        As in ``MDAnalysis.analysis.rms.rmsd`` (restated, not verified): the
        weighted centre, the weighted inner product, divided by the sum of
        the weights.  "mass": the AtomGroup's masses.
    superposition : bool
        True (the default here): the minimal RMSD over rotations and
        translations of each pair -- aligned analysis without a pre-pass is
        what this project is for.  False: the plain RMSD of the coordinates as
        they are, no centring, the trajectory assumed pre-aligned --
        ``MDAnalysis.analysis.diffusionmap.DistanceMatrix``'s default metric
        (``rms.rmsd`` with ``superposition=False``; restated, not verified).
    cutoff : float
        Distances <= cutoff are stored as 0 (upstream's 1e-5).
    layout : "fac" | "soa"
        Host arrays may be [F, 3, n_atoms] planes (interleaved by the
        stager); HBM-resident planes are refused (NotImplementedError).
    batch_frames : int, optional
        Frames per staged batch of a streamed input.

    One device per process: ``gpus=`` and a ``torch.distributed`` world of
    more than one rank are NotImplementedError.

    ``run(start, stop, step)`` or ``run(frames=...)`` as ``RMSF.run``;
    ``results.frames`` are the trajectory indices of the rows, ascending, and
    ``results.n_frames`` their count.

    Residency: a dense HBM tensor whose frame list is one run (a constant
    step) is read in place, its selection gathered in the kernel; everything
    else -- host arrays, files, AtomGroups, scattered frame lists -- is copied
    once into a dense [F, n_sel, 3] f32 buffer, batch by batch.  A result
    plus dense copy over half the free HBM is a MemoryError.
    """

    def __init__(self, atomgroup, *, select=None, weights=None, superposition: bool = True, cutoff: float = 1e-5,
                 layout: str = "fac", device=None, batch_frames: int | None = None, gpus=None):
        if layout not in ("fac", "soa"):
            raise ValueError(f"layout must be 'fac' or 'soa', got {layout!r}")
        self._input = atomgroup
        self.select = select
        self.weights = weights
        self.superposition = bool(superposition)
        self.cutoff = float(cutoff)
        self.layout = layout
        self.device = device
        self.batch_frames = batch_frames
        self.gpus = gpus
        self.results = Results()
        self.n_frames = None

    # -- what can be refused without a device ------------------------------
    def _n_sel_hint(self):
        """The selection's size where the input shows it without a source."""
        x = self._input
        if hasattr(x, "n_sel"):
            return int(x.n_sel)
        if self.select is not None:
            return int(np.asarray(self.select).reshape(-1).size)
        if isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim == 3:
            return int(x.shape[2] if self.layout == "soa" else x.shape[1])
        if hasattr(x, "universe") and hasattr(x, "n_atoms"):
            return int(x.n_atoms)
        return None

    def _refuse(self) -> None:
        x = self._input
        if self.gpus is not None or isinstance(x, (list, tuple)):
            raise NotImplementedError("DistanceMatrix runs on one device per process: not with gpus= or a list of "
                                      "shards")
        if (isinstance(x, DeviceSource) and x.layout == "soa") or (
                isinstance(x, torch.Tensor) and x.device.type == "cuda" and self.layout == "soa"):
            raise NotImplementedError(_PW_PLANES)
        if isinstance(self.weights, str):
            if self.weights != "mass":
                raise ValueError(f'weights must be None, "mass" or an array, got {self.weights!r}')
            if not hasattr(x, "masses"):
                raise ValueError('weights="mass" needs an AtomGroup; pass the masses as an array')
        n_sel = self._n_sel_hint()
        if n_sel is not None:
            _check_n_sel(n_sel)
            if self.weights is not None and not isinstance(self.weights, str):
                _check_weights(self.weights, n_sel)
        if parallel.world()[1] > 1:
            raise NotImplementedError("DistanceMatrix runs on one device per process: not under torch.distributed "
                                      "with more than one rank")

    # -- the frames, dense in HBM -------------------------------------------
    def _resident(self, eng: Engine, src, fl: FrameList):
        """(keep-alive, ptr, frame stride, device selection) of the frames at
        a constant stride."""
        n_frames, n_sel = len(fl), src.n_sel
        if isinstance(src, DeviceSource) and src.layout == "fac":
            runs = list(fl.runs(0, n_frames, n_frames))
            if len(runs) == 1:  # read in place
                first, step, n = runs[0]
                for f in (first, first + step * (n - 1)):
                    if not src.holds(f):
                        raise IndexError(f"frame {f} is not resident in this HBM tensor")
                check_pairwise_memory(eng, n_frames)
                return src.traj, src._ptr(first), src.fstride * step, src.sel_dev
        dense_bytes = 12 * n_frames * n_sel
        check_pairwise_memory(eng, n_frames, dense_bytes)
        dense = torch.empty((n_frames, n_sel, 3), dtype=torch.float32, device=eng.device)
        nb = max(1, min(self.batch_frames or n_frames, MAX_GATHER))
        rows = torch.arange(min(nb, n_frames), dtype=torch.int64, device=eng.device)
        done = 0
        for b in src.batches(fl, 0, n_frames, nb, eng.stream):
            if b.pstride:
                raise NotImplementedError(_PW_PLANES)
            eng.gather_frames(b.ptr, b.fstride, rows, b.n_frames, n_sel, b.sel, dense[done:done + b.n_frames])
            b.done()
            done += b.n_frames
        if done != n_frames:
            raise RuntimeError(f"the source yielded {done} of {n_frames} frames")
        return dense, dense.data_ptr(), 3 * n_sel, None

    def run(self, start=None, stop=None, step=None, frames=None, **kwargs):
        self._refuse()
        eng = Engine(self.device)
        with torch.cuda.device(eng.device):
            src, masses = make_source(self._input, select=self.select, align=None, batch_frames=self.batch_frames,
                                      layout=self.layout, group_masses=isinstance(self.weights, str))
            n_sel = src.n_sel
            _check_n_sel(n_sel)
            w = _check_weights(masses if isinstance(self.weights, str) else self.weights, n_sel)
            fl = FrameList(src.n_traj, start, stop, step, frames=frames)
            n_frames = len(fl)
            r = self.results
            r.frames = (np.asarray(fl.idx, dtype=np.int64).copy() if fl.idx is not None
                        else np.arange(fl.r.start, fl.r.stop, fl.r.step, dtype=np.int64))
            r.n_frames = self.n_frames = n_frames
            if n_frames == 0:
                r.dist_matrix = np.zeros((0, 0))
                return self
            keep, ptr, fstride, sel = self._resident(eng, src, fl)
            w_dev = None if w is None else torch.tensor(w, device=eng.device)
            w_total = float(n_sel) if w is None else float(w.sum())
            centre, g = eng.pairwise_centres(ptr, fstride, n_frames, n_sel, sel, w_dev, self.superposition)
            need = eng.pairwise_workspace_bytes(n_frames, n_sel)
            work = eng.empty(need // 8) if need else None
            out = eng.empty(n_frames, n_frames)
            eng.pairwise_rmsd(ptr, fstride, n_frames, n_sel, sel, w_dev, w_total, centre, g, out,
                              superpose=self.superposition, cutoff=self.cutoff, work=work)
            torch.cuda.current_stream(eng.device).synchronize()
            r.dist_matrix = out.cpu().numpy()
            del keep
        return self

    @property
    def dist_matrix(self):
        return self.results.dist_matrix


class DiffusionMap:
    """Diffusion map of a trajectory's frames, mirroring
    ``MDAnalysis.analysis.diffusionmap.DiffusionMap`` (restated, not
    verified): the kernel ``K = exp(-d^2 / epsilon)`` of the distance matrix,
    row-normalised to the transition matrix ``P = D^-1 K`` (D = K's row sums),
    and its eigenpairs.

    ``DiffusionMap(dist, epsilon=1.0).run()``; ``dist`` is a ``DistanceMatrix``
    (run here if it has not been) or an [F, F] array.  ``results.eigenvalues``
    [F] descending, the first equal to 1; ``results.eigenvectors`` [F, F], the
    right eigenvectors of P as columns (the first constant).  P is solved
    through its symmetric conjugate ``D^-1/2 K D^-1/2`` with
    ``numpy.linalg.eigh``, so the spectrum is real: P's right eigenvectors
    are ``D^-1/2`` times the conjugate's.  Host only, numpy only.
    """

    def __init__(self, dist, epsilon: float = 1.0):
        if not float(epsilon) > 0.0:
            raise ValueError(f"epsilon must be positive, got {epsilon}")
        self._dist = dist
        self.epsilon = float(epsilon)
        self.results = Results()

    def run(self, start=None, stop=None, step=None, frames=None):
        d = self._dist
        if isinstance(d, DistanceMatrix):
            if d.results.get("dist_matrix") is None:
                d.run(start, stop, step, frames=frames)
            d = d.results.dist_matrix
        d = np.asarray(d, dtype=np.float64)
        if d.ndim != 2 or d.shape[0] != d.shape[1]:
            raise ValueError("the distance matrix must be square")
        k = np.exp(-(d * d) / self.epsilon)
        rs = 1.0 / np.sqrt(k.sum(axis=1))
        sym = k * rs[:, None] * rs[None, :]
        sym = 0.5 * (sym + sym.T)
        w, v = np.linalg.eigh(sym)
        order = np.argsort(w, kind="stable")[::-1]
        w, v = w[order], v[:, order]
        right = v * rs[:, None]
        if right.shape[0] and right[:, 0].sum() < 0:  # the constant vector, positive
            right[:, 0] = -right[:, 0]
        self.results.eigenvalues = w
        self.results.eigenvectors = np.ascontiguousarray(right)
        self.results.n_frames = d.shape[0]
        return self

    def transform(self, n_eigenvectors: int, time: float):
        """The diffusion-space embedding [F, n_eigenvectors]: the
        eigenvectors after the constant one, each scaled by its eigenvalue to
        the power ``time`` (as upstream's ``transform``)."""
        if "eigenvalues" not in self.results:
            self.run()
        w, v = self.results.eigenvalues, self.results.eigenvectors
        n = int(n_eigenvectors)
        if not 1 <= n <= len(w) - 1:
            raise ValueError(f"n_eigenvectors must be in 1..{len(w) - 1}, got {n_eigenvectors}")
        return v[:, 1:n + 1] * (w[1:n + 1] ** time)
