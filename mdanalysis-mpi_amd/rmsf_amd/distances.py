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
matrix: on the host (numpy only, like ``pca_from_comoment``), or, with
``solver="device"``, its first modes with the matrix kept in HBM
(csrc/diffusion.hip and the block solver of ``rmsf_amd.eigen``).

``CrossDistanceMatrix(a, b).run().results.dist_matrix`` is the rectangular
F_a x F_b matrix of the RMSDs of every frame of one trajectory to every frame
of another (or to a set of reference structures), by the same contraction
over the whole tile rectangle with a second operand of its own;
``results.nearest`` names each frame's nearest reference.  ``hausdorff`` and
``discrete_frechet`` are the path-similarity distances of such a matrix, on
the host, named as ``MDAnalysis.analysis.psa`` names them.

MDAnalysis is not a dependency and is absent where this was written: its
semantics (``DistanceMatrix``'s metric and cutoff, ``rms.rmsd``'s weights,
``DiffusionMap``'s kernel and ``transform``, ``psa``'s two distances) are
restated from its published documentation, not verified against it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import parallel
from .eigen import MAX_COMPONENTS, KernelOps, block_width, top_eigenpairs
from .engine import Engine
from .rms import Results, make_source
from .sources import DeviceSource, FrameList

_PW_PLANES = ('DistanceMatrix reads (frame, atom, xyz) rows; HBM-resident coordinate planes are not supported -- '
              'pass the trajectory with layout="fac"')
MAX_GATHER = 65535  # frames one rmsf_gather_frames launch takes


def check_pairwise_memory(eng: Engine, n_frames: int, dense_bytes: int = 0, bits: bool = False,
                          matrix: bool = True) -> None:
    """MemoryError if the [F, F] f64 result plus the dense copy of the
    selected rows (when one is made) is over half the free HBM.  ``bits``
    (``Cluster``): plus the F^2 / 8 bytes of the neighbour bits.  ``matrix``
    False, the bits-only form (``Cluster(matrix="bits")``, where no f64 matrix
    is stored): the neighbour bits and the dense copy alone.  The split-K
    workspace is in neither form: it exists only up to 352 frames (256 tile
    pairs) and is at most 512 tile pairs' partials, 9.4 MB whatever the
    atoms -- the other half of the free HBM is there for such."""
    free = torch.cuda.mem_get_info(eng.device)[0]
    bit_bytes = 8 * n_frames * ((n_frames + 63) // 64) if bits or not matrix else 0
    if not matrix:
        if bit_bytes + dense_bytes > free // 2:
            raise MemoryError(f"Cluster: the neighbour bits of {n_frames} frames need {bit_bytes} bytes"
                              + (f" and the dense copy of the selected rows {dense_bytes} bytes" if dense_bytes else "")
                              + f", over half of the {free} bytes of free HBM")
        return
    need = 8 * n_frames * n_frames
    if need + dense_bytes + bit_bytes > free // 2:
        raise MemoryError(f"DistanceMatrix: the [{n_frames}, {n_frames}] f64 matrix needs {need} bytes"
                          + (f", its neighbour bits {bit_bytes} bytes" if bit_bytes else "")
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


def _n_sel_hint(x, select, layout: str):
    """The selection's size where the input shows it without a source."""
    if hasattr(x, "n_sel"):
        return int(x.n_sel)
    if select is not None:
        return int(np.asarray(select).reshape(-1).size)
    if isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim == 3:
        return int(x.shape[2] if layout == "soa" else x.shape[1])
    if hasattr(x, "universe") and hasattr(x, "n_atoms"):
        return int(x.n_atoms)
    return None


def _in_place_run(src, fl: FrameList):
    """(first, step) where the frames of ``fl`` can be read where they lie: a
    dense HBM tensor and a frame list of one run; None otherwise."""
    n_frames = len(fl)
    if isinstance(src, DeviceSource) and src.layout == "fac":
        runs = list(fl.runs(0, n_frames, n_frames))
        if len(runs) == 1:
            first, step, n = runs[0]
            for f in (first, first + step * (n - 1)):
                if not src.holds(f):
                    raise IndexError(f"frame {f} is not resident in this HBM tensor")
            return first, step
    return None


def resident_frames(eng: Engine, src, fl: FrameList, batch_frames, check):
    """(keep-alive, ptr, frame stride, device selection) of the frames of
    ``fl`` at a constant stride: read in place (see ``_in_place_run``), or
    copied once into a dense [F, n_sel, 3] f32 buffer, batch by batch.
    ``check(dense_bytes)`` runs before anything is allocated (the callers'
    MemoryError).  The residency rule of ``DistanceMatrix`` and of either side
    of ``CrossDistanceMatrix``."""
    n_frames, n_sel = len(fl), src.n_sel
    run = _in_place_run(src, fl)
    if run is not None:
        first, step = run
        check(0)
        return src.traj, src._ptr(first), src.fstride * step, src.sel_dev
    check(12 * n_frames * n_sel)
    dense = torch.empty((n_frames, n_sel, 3), dtype=torch.float32, device=eng.device)
    nb = max(1, min(batch_frames or n_frames, MAX_GATHER))
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
        self.matrix_form = None  # set by _adjacency_hbm

    # -- what can be refused without a device ------------------------------
    def _n_sel_hint(self):
        return _n_sel_hint(self._input, self.select, self.layout)

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

    def _pairs_hbm(self, eng: Engine, start, stop, step, frames, check):
        """What the matrix and the neighbour bits share: the source, the frame
        list (``results.frames`` / ``n_frames`` are set), the frames' residency,
        their centres and the split-K workspace.  ``check(n_frames,
        dense_bytes)`` runs before anything is allocated.  Returns
        (the arguments of ``Engine.pairwise_rmsd`` up to ``g``, work, what
        the kernels read), or None with no frames."""
        src, masses = make_source(self._input, select=self.select, align=None, batch_frames=self.batch_frames,
                                  layout=self.layout, group_masses=isinstance(self.weights, str))
        n_sel = src.n_sel
        _check_n_sel(n_sel)
        w = _check_weights(masses if isinstance(self.weights, str) else self.weights, n_sel)
        fl = FrameList(src.n_traj, start, stop, step, frames=frames)
        n_frames = len(fl)
        r = self.results
        r.frames = _frame_rows(fl)
        r.n_frames = self.n_frames = n_frames
        if n_frames == 0:
            return None
        keep, ptr, fstride, sel = resident_frames(eng, src, fl, self.batch_frames,
                                                  lambda dense_bytes: check(n_frames, dense_bytes))
        w_dev = None if w is None else torch.tensor(w, device=eng.device)
        w_total = float(n_sel) if w is None else float(w.sum())
        centre, g = eng.pairwise_centres(ptr, fstride, n_frames, n_sel, sel, w_dev, self.superposition)
        need = eng.pairwise_workspace_bytes(n_frames, n_sel)
        work = eng.empty(need // 8) if need else None
        return (ptr, fstride, n_frames, n_sel, sel, w_dev, w_total, centre, g), work, (src, keep, w_dev, centre, g, work)

    def _matrix_hbm(self, eng: Engine, start=None, stop=None, step=None, frames=None, bits: bool = False):
        """The device part of ``run``: ``results.frames`` / ``n_frames`` are
        set and (the [F, F] f64 matrix as an HBM tensor, what its kernels read)
        is returned, the kernels enqueued on the current stream and not waited
        for: the caller holds the second until it has synchronised.  (None,
        None) with no frames.  ``bits``: the memory check also counts a bit
        matrix (``Cluster``).  Call it under ``torch.cuda.device(eng.device)``."""
        pairs = self._pairs_hbm(eng, start, stop, step, frames,
                                lambda n, dense: check_pairwise_memory(eng, n, dense, bits=bits))
        if pairs is None:
            return None, None
        args, work, keep = pairs
        return self._store_matrix(eng, args, work), keep

    def _store_matrix(self, eng: Engine, args, work) -> torch.Tensor:
        n_frames = args[2]
        out = eng.empty(n_frames, n_frames)
        eng.pairwise_rmsd(*args, out, superpose=self.superposition, cutoff=self.cutoff, work=work)
        return out

    def _adjacency_hbm(self, eng: Engine, cutoff: float, start=None, stop=None, step=None, frames=None,
                       matrix: str = "bits"):
        """``_matrix_hbm`` for the neighbour bits within ``cutoff`` alone:
        (uint64 words as int64 [F, words], int32 [F] row counts, what the
        kernels read), enqueued and not waited for; (None, None, None) with no
        frames.  ``matrix`` "bits": the pair kernel's epilogue writes the bits
        and no f64 matrix is stored (``Engine.pairwise_adjacency``); the memory
        check is ``check_pairwise_memory``'s bits-only form.  "auto": where
        the stored matrix passes that check as it stands, the matrix is
        stored, packed and freed, as ``_matrix_hbm`` and
        ``Engine.adjacency_pack`` do; the bits alone otherwise.
        ``self.matrix_form`` is "f64" or "bits", whichever ran."""
        form = [matrix]

        def check(n, dense):
            if form[0] == "auto":
                try:
                    check_pairwise_memory(eng, n, dense, bits=True)
                    form[0] = "f64"
                    return
                except MemoryError:
                    form[0] = "bits"
            check_pairwise_memory(eng, n, dense, matrix=False)

        pairs = self._pairs_hbm(eng, start, stop, step, frames, check)
        if pairs is None:
            return None, None, None
        args, work, keep = pairs
        self.matrix_form = form[0]
        if form[0] == "f64":
            adj, count = eng.adjacency_pack(self._store_matrix(eng, args, work), cutoff)
            return adj, count, keep
        n_frames = args[2]
        adj = torch.empty((n_frames, eng.adjacency_words(n_frames)), dtype=torch.int64, device=eng.device)
        count = torch.empty(n_frames, dtype=torch.int32, device=eng.device)
        eng.pairwise_adjacency(*args, adj, count, cutoff, superpose=self.superposition, zero_cutoff=self.cutoff,
                               work=work)
        return adj, count, keep

    def run(self, start=None, stop=None, step=None, frames=None, **kwargs):
        self._refuse()
        eng = Engine(self.device)
        with torch.cuda.device(eng.device):
            out, keep = self._matrix_hbm(eng, start, stop, step, frames)
            if out is None:
                self.results.dist_matrix = np.zeros((0, 0))
                return self
            torch.cuda.current_stream(eng.device).synchronize()
            self.results.dist_matrix = out.cpu().numpy()
            del keep
        return self

    @property
    def dist_matrix(self):
        return self.results.dist_matrix


def _frame_rows(fl: FrameList) -> np.ndarray:
    return (np.asarray(fl.idx, dtype=np.int64).copy() if fl.idx is not None
            else np.arange(fl.r.start, fl.r.stop, fl.r.step, dtype=np.int64))


def _one_frame(x):
    """A 2-D array ([n_atoms, 3], or [3, n_atoms] planes) is one frame."""
    if isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim == 2:
        return x[None]
    return x


class CrossDistanceMatrix:
    """The rectangular RMSD matrix of two trajectories,
    ``results.dist_matrix[i, j] = RMSD(A_i, B_j)`` (host f64 [F_a, F_b]): the
    RMSD of every frame to a set of reference structures, the 2-D RMSD plot
    between two runs, the input of ``hausdorff`` and ``discrete_frechet``.
    Only the F_a x F_b pairs asked for are computed (csrc/pairwise.hip,
    ``k_pw_tiles`` over the tile rectangle), each once.

    Parameters
    ----------
    a, b : as ``DistanceMatrix``'s input, independently of each other (an HBM
        tensor read in place against a host array or an ``.xtc`` path, ...).
        A 2-D [n_atoms, 3] array is one frame.
    select, select_b : array of int, optional
        The atoms of A and of B (``select_b`` defaults to ``select``); atom k
        of one is paired with atom k of the other, so both must have the same
        length, at least 3.  The frames of A and B may differ in size.
    weights : None | "mass" | array [n_sel]
        One weight per selected atom, shared by both sides; "mass": the masses
        of A's AtomGroup.
    superposition, cutoff : as ``DistanceMatrix``.
    layout, layout_b : "fac" | "soa"
        As ``DistanceMatrix``'s ``layout``, per side (``layout_b`` defaults to
        ``layout``).

    ``run(start, stop, step, frames=None, frames_b=None)``: the frame
    arguments apply to A; B is used whole, or restricted to ``frames_b``.
    ``results.frames`` / ``results.frames_b`` are the trajectory indices of the
    rows / columns, ``results.n_frames`` / ``results.n_frames_b`` their counts.
    ``results.nearest`` (int64 [F_a]) is the column of each row's least
    distance -- the lowest such column where several are equal, which happens:
    the cutoff writes exact zeros and references can be duplicated -- and
    ``results.nearest_dist`` (f64 [F_a]) that distance; both are found on the
    device before the matrix is copied back (``rmsf_row_argmin``).  A frame
    with a non-finite coordinate makes its row or column NaN and, as for
    ``numpy.argmin``, a NaN counts as the least: every row then names the
    first such reference and its ``nearest_dist`` is NaN.  With no
    frames on either side the matrix is empty, ``nearest`` is -1 and
    ``nearest_dist`` NaN.

    Residency, per side, as ``DistanceMatrix``; a result plus dense copies over
    half the free HBM is a MemoryError before anything is launched.  One
    device per process; HBM-resident planes are refused.
    """

    def __init__(self, a, b, *, select=None, select_b=None, weights=None, superposition: bool = True,
                 cutoff: float = 1e-5, layout: str = "fac", layout_b: str | None = None, device=None,
                 batch_frames: int | None = None, gpus=None):
        layout_b = layout if layout_b is None else layout_b
        for lay in (layout, layout_b):
            if lay not in ("fac", "soa"):
                raise ValueError(f"layout must be 'fac' or 'soa', got {lay!r}")
        self._a, self._b = _one_frame(a), _one_frame(b)
        self.select = select
        self.select_b = select if select_b is None else select_b
        self.weights = weights
        self.superposition = bool(superposition)
        self.cutoff = float(cutoff)
        self.layout, self.layout_b = layout, layout_b
        self.device = device
        self.batch_frames = batch_frames
        self.gpus = gpus
        self.results = Results()
        self.n_frames = self.n_frames_b = None

    def _refuse(self) -> None:
        sides = ((self._a, self.select, self.layout), (self._b, self.select_b, self.layout_b))
        if self.gpus is not None or any(isinstance(x, (list, tuple)) for x, _, _ in sides):
            raise NotImplementedError("CrossDistanceMatrix runs on one device per process: not with gpus= or a list "
                                      "of shards")
        for x, _, lay in sides:
            if (isinstance(x, DeviceSource) and x.layout == "soa") or (
                    isinstance(x, torch.Tensor) and x.device.type == "cuda" and lay == "soa"):
                raise NotImplementedError(_PW_PLANES)
        if isinstance(self.weights, str):
            if self.weights != "mass":
                raise ValueError(f'weights must be None, "mass" or an array, got {self.weights!r}')
            if not hasattr(self._a, "masses"):
                raise ValueError('weights="mass" needs an AtomGroup as A; pass the masses as an array')
        hints = [_n_sel_hint(x, s, lay) for x, s, lay in sides]
        if None not in hints and hints[0] != hints[1]:
            raise ValueError(f"the selections of A and B must have the same length, got {hints[0]} and {hints[1]}")
        for n_sel in hints:
            if n_sel is not None:
                _check_n_sel(n_sel)
                if self.weights is not None and not isinstance(self.weights, str):
                    _check_weights(self.weights, n_sel)
        if parallel.world()[1] > 1:
            raise NotImplementedError("CrossDistanceMatrix runs on one device per process: not under "
                                      "torch.distributed with more than one rank")

    def run(self, start=None, stop=None, step=None, frames=None, frames_b=None, **kwargs):
        self._refuse()
        eng = Engine(self.device)
        with torch.cuda.device(eng.device):
            src_a, masses = make_source(self._a, select=self.select, align=None, batch_frames=self.batch_frames,
                                        layout=self.layout, group_masses=isinstance(self.weights, str))
            src_b, _ = make_source(self._b, select=self.select_b, align=None, batch_frames=self.batch_frames,
                                   layout=self.layout_b, group_masses=False)
            n_sel = src_a.n_sel
            if src_b.n_sel != n_sel:
                raise ValueError(f"the selections of A and B must have the same length, got {n_sel} and "
                                 f"{src_b.n_sel}")
            _check_n_sel(n_sel)
            w = _check_weights(masses if isinstance(self.weights, str) else self.weights, n_sel)
            fl_a = FrameList(src_a.n_traj, start, stop, step, frames=frames)
            fl_b = FrameList(src_b.n_traj, frames=frames_b)
            n_a, n_b = len(fl_a), len(fl_b)
            r = self.results
            r.frames, r.frames_b = _frame_rows(fl_a), _frame_rows(fl_b)
            r.n_frames = self.n_frames = n_a
            r.n_frames_b = self.n_frames_b = n_b
            if n_a == 0 or n_b == 0:
                r.dist_matrix = np.zeros((n_a, n_b))
                r.nearest = np.full(n_a, -1, dtype=np.int64)
                r.nearest_dist = np.full(n_a, np.nan)
                return self
            # the result and both dense copies, before anything is allocated
            dense = sum(0 if _in_place_run(s, fl) is not None else 12 * len(fl) * n_sel
                        for s, fl in ((src_a, fl_a), (src_b, fl_b)))
            need = 8 * n_a * n_b
            free = torch.cuda.mem_get_info(eng.device)[0]
            if need + dense > free // 2:
                raise MemoryError(f"CrossDistanceMatrix: the [{n_a}, {n_b}] f64 matrix needs {need} bytes"
                                  + (f" and the dense copies of the selected rows {dense} bytes" if dense else "")
                                  + f", over half of the {free} bytes of free HBM")
            keep_a, ptr_a, stride_a, sel_a = resident_frames(eng, src_a, fl_a, self.batch_frames, lambda _: None)
            keep_b, ptr_b, stride_b, sel_b = resident_frames(eng, src_b, fl_b, self.batch_frames, lambda _: None)
            w_dev = None if w is None else torch.tensor(w, device=eng.device)
            w_total = float(n_sel) if w is None else float(w.sum())
            if self.superposition:
                centre_a, g_a = eng.pairwise_centres(ptr_a, stride_a, n_a, n_sel, sel_a, w_dev, True)
                centre_b, g_b = eng.pairwise_centres(ptr_b, stride_b, n_b, n_sel, sel_b, w_dev, True)
            else:  # one common shift: the centre of A's first frame
                centre_a, g_a = eng.pairwise_centres(ptr_a, stride_a, n_a, n_sel, sel_a, w_dev, False)
                centre_b, g_b = eng.pairwise_centres_about(ptr_b, stride_b, n_b, n_sel, sel_b, w_dev, centre_a)
            work_bytes = eng.cross_workspace_bytes(n_a, n_b, n_sel)
            work = eng.empty(work_bytes // 8) if work_bytes else None
            out = eng.empty(n_a, n_b)
            eng.cross_rmsd(ptr_a, stride_a, n_a, sel_a, centre_a, g_a, ptr_b, stride_b, n_b, sel_b, centre_b, g_b,
                           n_sel, w_dev, w_total, out, superpose=self.superposition, cutoff=self.cutoff, work=work)
            idx, val = eng.row_argmin(out)
            torch.cuda.current_stream(eng.device).synchronize()
            r.dist_matrix = out.cpu().numpy()
            r.nearest, r.nearest_dist = idx.cpu().numpy(), val.cpu().numpy()
            del keep_a, keep_b
        return self

    @property
    def dist_matrix(self):
        return self.results.dist_matrix


def _cross_matrix(d) -> np.ndarray:
    d = np.asarray(d, dtype=np.float64)
    if d.ndim != 2 or d.size == 0:
        raise ValueError("a cross distance matrix [F_a, F_b] with at least one frame a side is needed")
    return d


def hausdorff(d) -> float:
    """The Hausdorff distance of two paths from their cross matrix ``d[i, j]``
    (``CrossDistanceMatrix``'s ``dist_matrix``): the largest distance of a
    frame of either path to the nearest frame of the other, ``max(d.min(1)
    .max(), d.min(0).max())``.  Named as ``MDAnalysis.analysis.psa.hausdorff``;
    its semantics are restated from its documentation, not verified against
    it.  Host only, numpy only."""
    d = _cross_matrix(d)
    return float(max(d.min(axis=1).max(), d.min(axis=0).max()))


def discrete_frechet(d) -> float:
    """The discrete Frechet distance of two paths from their cross matrix: the
    last entry of the coupling recurrence ``c[i, j] = max(d[i, j], min(c[i-1,
    j], c[i-1, j-1], c[i, j-1]))`` (Eiter and Mannila 1994), evaluated one
    anti-diagonal at a time -- the entries of an anti-diagonal depend only on
    the two before it, so F_a + F_b - 1 vector steps replace the F_a F_b scalar
    ones.  Only selects and compares entries of ``d``: the result is one of
    them.  Named as ``MDAnalysis.analysis.psa.discrete_frechet``; its semantics
    are restated from its documentation, not verified against it.  Host only,
    numpy only."""
    d = _cross_matrix(d)
    n, m = d.shape
    # c with a border of +inf: row 0 and column 0 stand for "no predecessor";
    # the corner is -inf so that c[1, 1] = d[0, 0]
    c = np.full((n + 1, m + 1), np.inf)
    c[0, 0] = -np.inf
    for k in range(2, n + m + 1):
        i = np.arange(max(1, k - m), min(n, k - 1) + 1)
        j = k - i
        c[i, j] = np.maximum(d[i - 1, j - 1], np.minimum(np.minimum(c[i - 1, j], c[i - 1, j - 1]), c[i, j - 1]))
    return float(c[n, m])


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
    are ``D^-1/2`` times the conjugate's.  ``solver="host"`` (the default) is
    that: host only, numpy only, all F eigenpairs at O(F^3);
    ``n_eigenvectors`` and the solver's parameters are ignored.

    ``solver="device"``: the first ``n_eigenvectors`` = k diffusion
    coordinates (1 <= k <= 39) and the constant mode before them, with the
    matrix in HBM from start to end.  ``dist`` may then be

      * a ``DistanceMatrix`` that has not run -- any trajectory input, wrapped:
        ``DiffusionMap(DistanceMatrix(ca), ...)``.  Its matrix is computed in
        HBM, transformed in place and never copied to the host (its
        ``results.dist_matrix`` stays unset); memory and refusals are
        ``DistanceMatrix``'s own.
      * a ``DistanceMatrix`` that has run, or a host [F, F] array: uploaded.
      * a square f64 HBM tensor: copied, the caller's stays as it is; a copy
        over half the free HBM is a MemoryError.

    A matrix of the caller's must be exactly symmetric, ``d[i, j] == d[j, i]``:
    the device product reads K[j, i] where the formula has K[i, j].  The host
    path symmetrises the conjugate matrix and forgives a rounding's difference;
    here the kernel of such a matrix is compared with its transpose once on
    the device and a difference is a ValueError (pass ``0.5 * (d + d.T)``).

    One pass (csrc/diffusion.hip) turns the distances into K and sums its
    rows; the F row sums come to the host, and one that is not positive and
    finite -- a NaN distance, a user's matrix whose diagonal underflows -- is a
    ValueError.  ``rmsf_amd.eigen.top_eigenpairs`` then runs over
    ``KernelOps``: ``symm(Q) = D^-1/2 K (D^-1/2 Q)``, K read once per
    iteration on the f64 matrix cores, the conjugate never written.
    ``results.eigenvalues`` [k + 1] descending, the first 1 to the solver's
    tolerance; ``results.eigenvectors`` [F, k + 1] host f64, ``D^-1/2`` times
    the conjugate's orthonormal vectors, the constant one positive;
    ``results.solver_info`` the driver's record (``tol``, ``max_iter``,
    ``seed`` are its parameters).  ``PCAConvergenceError`` when it does not
    converge; ValueError for a bad k or solver before any device work, and
    for k + 1 > F as soon as F is known, before the matrix is computed.

    The Gaussian kernel of superposed RMSDs is not guaranteed positive
    semi-definite: minimal RMSD is not a Euclidean distance.  The driver
    returns the largest eigenvalues of the subspace it finds, which for the
    spectra met here are the leading ones; a matrix with a negative eigenvalue
    of large magnitude would draw the iteration towards it.  Modes in a flat
    tail of the spectrum crawl, as they do for ``PCA(solver="device")``: ask
    for fewer, or raise ``max_iter``.
    """

    MAX_EIGENVECTORS = MAX_COMPONENTS - 1  # the constant mode is computed with the others

    def __init__(self, dist, epsilon: float = 1.0, *, n_eigenvectors: int | None = None, solver: str = "host",
                 tol: float = 1e-10, max_iter: int = 300, seed: int = 0, device=None):
        if not float(epsilon) > 0.0:
            raise ValueError(f"epsilon must be positive, got {epsilon}")
        if solver not in ("host", "device"):
            raise ValueError(f'solver must be "host" or "device", got {solver!r}')
        if solver == "device":
            if n_eigenvectors is None:
                raise ValueError('solver="device" needs n_eigenvectors, the number of diffusion coordinates to compute')
            if not 1 <= int(n_eigenvectors) <= self.MAX_EIGENVECTORS:
                raise ValueError(f'solver="device" computes 1..{self.MAX_EIGENVECTORS} diffusion coordinates, got '
                                 f'n_eigenvectors = {n_eigenvectors}; use solver="host" for more')
            if not np.isfinite(float(epsilon)):
                raise ValueError(f"epsilon must be finite, got {epsilon}")
            if int(max_iter) < 1:
                raise ValueError(f"max_iter must be at least 1, got {max_iter}")
        self._dist = dist
        self.epsilon = float(epsilon)
        self.n_eigenvectors = None if n_eigenvectors is None else int(n_eigenvectors)
        self.solver = solver
        self.tol, self.max_iter, self.seed = float(tol), int(max_iter), seed
        self.device = device
        self.results = Results()

    def _check_frames(self, n_frames: int) -> None:
        """``block_width``'s refusal of k + 1 > F, in this class's terms."""
        k = self.n_eigenvectors
        try:
            block_width(n_frames, k + 1)
        except ValueError as e:
            raise ValueError(f"n_eigenvectors = {k} diffusion coordinates and the constant mode are {k + 1} "
                             f"eigenpairs, the matrix has {n_frames} frames: ask for at most "
                             f"{min(n_frames, MAX_COMPONENTS) - 1}") from e

    def _kernel_input_hbm(self, eng: Engine, start, stop, step, frames):
        """(the distances as an f64 [F, F] HBM tensor this run may overwrite,
        what its kernels read -- to be held until the stream has been waited
        for)."""
        d = self._dist
        if isinstance(d, DistanceMatrix) and d.results.get("dist_matrix") is None:
            d._refuse()

            def check(n, dense):  # before anything is allocated or computed
                self._check_frames(n)
                check_pairwise_memory(eng, n, dense)

            pairs = d._pairs_hbm(eng, start, stop, step, frames, check)
            if pairs is None:
                raise ValueError("the distance matrix has no frames")
            args, work, keep = pairs
            return d._store_matrix(eng, args, work), keep
        if isinstance(d, DistanceMatrix):
            d = d.results.dist_matrix
        on_device = isinstance(d, torch.Tensor) and d.device.type == "cuda"
        if on_device:
            if d.dtype != torch.float64:
                raise ValueError(f"an HBM distance matrix must be float64, got {d.dtype}")
        else:
            d = np.ascontiguousarray(d.cpu().numpy() if isinstance(d, torch.Tensor) else d, dtype=np.float64)
        if d.ndim != 2 or d.shape[0] != d.shape[1]:
            raise ValueError("the distance matrix must be square")
        n = int(d.shape[0])
        if n == 0:
            raise ValueError("the distance matrix has no frames")
        self._check_frames(n)
        free = torch.cuda.mem_get_info(eng.device)[0]
        if 8 * n * n > free // 2:
            raise MemoryError(f"DiffusionMap: the copy of the [{n}, {n}] f64 matrix needs {8 * n * n} bytes, over "
                              f"half of the {free} bytes of free HBM")
        if on_device:
            out = eng.empty(n, n)
            out.copy_(d)
            return out, None
        return torch.as_tensor(d).to(eng.device), None

    def _run_device(self, start, stop, step, frames):
        k = self.n_eigenvectors + 1
        eng = Engine(self.device)
        with torch.cuda.device(eng.device):
            kern, keep = self._kernel_input_hbm(eng, start, stop, step, frames)
            n = int(kern.shape[0])
            supplied = keep is None  # a matrix of the caller's, not one computed here
            rowsum = eng.diffusion_kernel(kern, self.epsilon)
            torch.cuda.current_stream(eng.device).synchronize()
            del keep
            rs = rowsum.cpu().numpy()
            if not (np.all(np.isfinite(rs)) and np.all(rs > 0.0)):
                bad = np.nonzero(~(np.isfinite(rs) & (rs > 0.0)))[0]
                raise ValueError(f"the distance matrix has non-finite entries or rows whose kernel sums to zero: "
                                 f"{bad.size} of the {n} row sums of exp(-d^2 / epsilon) are not positive and finite "
                                 f"(the first is row {int(bad[0])})")
            if supplied and not torch.equal(kern, kern.T):
                raise ValueError('solver="device" needs a distance matrix that is exactly symmetric, d[i, j] == '
                                 "d[j, i] (its product reads K[j, i] for K[i, j]); pass 0.5 * (d + d.T), or use "
                                 'solver="host", which symmetrises the conjugate matrix itself')
            t = 1.0 / np.sqrt(rs)
            ops = KernelOps(kern, torch.as_tensor(t).to(eng.device), engine=eng)
            w, v, info = top_eigenpairs(None, k, tol=self.tol, max_iter=self.max_iter, seed=self.seed, ops=ops)
        right = v * t[:, None]
        if right[:, 0].sum() < 0:  # the constant vector, positive
            right[:, 0] = -right[:, 0]
        self.results.eigenvalues = w
        self.results.eigenvectors = np.ascontiguousarray(right)
        self.results.n_frames = n
        self.results.solver_info = info
        return self

    def run(self, start=None, stop=None, step=None, frames=None):
        if self.solver == "device":
            return self._run_device(start, stop, step, frames)
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
            raise ValueError(f"n_eigenvectors must be in 1..{len(w) - 1}, the diffusion coordinates this run computed, "
                             f"got {n_eigenvectors}")
        return v[:, 1:n + 1] * (w[1:n + 1] ** time)
