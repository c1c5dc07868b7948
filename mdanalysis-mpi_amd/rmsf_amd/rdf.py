"""``InterRDF`` -- the radial distribution function g(r) between two selections,
free or under the minimum image of an orthorhombic box, named as
``MDAnalysis.analysis.rdf.InterRDF`` names it.

One rule bins a pair everywhere (csrc/rdf.hip, csrc/pair_image.h,
include/rmsf_hip.h): the coordinates are f32 as stored,
``dx = (double)xa - (double)xb`` and so for y and z; with a box
``dx = dx - Lx * rint(dx * ix)`` where ``ix = 1.0 / Lx`` is formed once a frame
and ``rint`` rounds half to even; ``d2 = (dx*dx + dy*dy) + dz*dz`` with no FMA
and ``d = sqrt(d2)`` correctly rounded.  The edges are
``numpy.linspace(rmin, rmax, nbins + 1)``; bin k holds ``e_k <= d < e_(k+1)``,
the last bin also ``d == rmax``, and a NaN is in no bin -- the counts of
``numpy.histogram(d, bins=nbins, range=(rmin, rmax))``, compared with it for
equality.  The device takes no root a pair: the host turns every edge into a
threshold on ``d2`` (``rdf_edges``).

Nothing of the size [F, n, n] is formed: a workgroup streams the frames of a
64 x 64 tile of pairs through LDS and keeps the histogram in LDS counters.

Only orthorhombic boxes; ``rmax`` may not exceed half the shortest box edge of
any frame of the run (past it the minimum image is not the only image in
range).  No cell lists: every pair of the two selections is visited.

MDAnalysis is not a dependency and is absent where this was written: the
names and the normalisation (``norm``, ``exclusion_block``, ``get_cdf``) are
restated from its published documentation, not verified against it.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from .contacts import _PairAnalysis
from .distances import _frame_rows
from .engine import Engine
from .sources import FrameList

MAX_BINS = 2048
NORMS = ("rdf", "density", "none")


def rdf_edges(rmin: float, rmax: float, nbins: int):
    """(edges f64 [nbins + 1], thresholds_sq f64 [nbins + 1]): the bin edges,
    ``numpy.linspace(rmin, rmax, nbins + 1)``'s bits, and the same bins as
    thresholds on the squared distance -- bin k is ``T_k <= d2 < T_(k+1)``
    (rmsf_rdf_edges; host only)."""
    rmin, rmax, nbins = _check_range((rmin, rmax), nbins)
    e, t = np.empty(nbins + 1), np.empty(nbins + 1)
    _lib.call("rmsf_rdf_edges", rmin, rmax, nbins, e.ctypes.data, t.ctypes.data)
    return e, t


def _check_range(rng, nbins):
    try:
        rmin, rmax = (float(v) for v in rng)
    except (TypeError, ValueError):
        raise ValueError(f"range must be (rmin, rmax), got {rng!r}") from None
    if not (np.isfinite(rmin) and np.isfinite(rmax) and 0.0 <= rmin < rmax):
        raise ValueError(f"range needs 0 <= rmin < rmax, both finite, got {rng!r}")
    if int(nbins) != nbins or not 1 <= int(nbins) <= MAX_BINS:
        raise ValueError(f"nbins must be an integer in 1..{MAX_BINS}, got {nbins!r}")
    return rmin, rmax, int(nbins)


def _box_edges(box, what: str) -> np.ndarray:
    """f64 [..., 3] from [..., 3] or [..., 6] (edges and angles, 90 degrees
    only): positive and finite."""
    b = np.asarray(box, dtype=np.float64)
    if b.ndim not in (1, 2) or b.shape[-1] not in (3, 6):
        raise ValueError(f"{what} must be [3], [6], [n_frames, 3] or [n_frames, 6], got shape {b.shape}")
    if b.shape[-1] == 6:
        if (b[..., 3:] != 90.0).any():
            raise NotImplementedError(f"{what}: only orthorhombic boxes are supported (angles of 90 degrees)")
        b = b[..., :3]
    if not (np.isfinite(b) & (b > 0.0)).all():
        raise ValueError(f"{what}: every box edge must be positive and finite")
    return np.ascontiguousarray(b)


def _box_argument(box, traj):
    """A ``box=`` argument checked: None, ``"file"`` (``traj`` must be an
    ``.xtc`` path) or the edges f64 [3] / [n_traj, 3]."""
    if isinstance(box, str):
        if box != "file":
            raise ValueError(f"box must be None, an array or 'file', got {box!r}")
        is_path = isinstance(traj, (str, bytes)) or hasattr(traj, "__fspath__")
        if not (is_path and str(os.fspath(traj)).lower().endswith(".xtc")):
            raise ValueError("box='file' reads the boxes of an .xtc path; pass the boxes as an array for any "
                             "other input")
        return box
    return None if box is None else _box_edges(box, "box")


def _run_boxes(box, traj, n_traj: int, frames: np.ndarray):
    """f64 [len(frames), 3] for the run's frames from a checked ``box=``
    argument; None in free space."""
    if box is None:
        return None
    if isinstance(box, str):
        from .xtc import XTCFile
        with XTCFile(os.fspath(traj)) as fh:
            box = fh.boxes()
    if box.ndim == 1:
        return np.broadcast_to(box, (len(frames), 3)).copy()
    if box.shape[0] != n_traj:
        raise ValueError(f"box has {box.shape[0]} rows, the trajectory {n_traj} frames")
    return np.ascontiguousarray(box[frames])


class InterRDF(_PairAnalysis):
    """The radial distribution function of ``select_b`` around ``select``,
    mirroring ``MDAnalysis.analysis.rdf.InterRDF`` (restated, not verified).

    Parameters
    ----------
    traj : as ``ContactMap``'s input -- a float32 trajectory [F, n_atoms, 3] on
        the host or in HBM, an ``.xtc`` / ``.dcd`` path, an AtomGroup, a frame
        source.
    select, select_b : array of int, optional
        The two groups of atoms.  ``select=None`` is every atom;
        ``select_b=None`` is ``select`` against itself by the symmetric route:
        the ordered pairs i != j, an atom never paired with itself.
    nbins : int, 1..2048.  range : (rmin, rmax), ``0 <= rmin < rmax``.
    norm : "rdf" | "density" | "none"
        ``rdf`` divides the counts by the frames, the shell volumes and the
        pair density ``N / volume``; ``density`` by the frames and the shell
        volumes; ``none`` by the frames.  ``rdf`` needs a box (ValueError
        without one: there is no volume).
    exclusion_block : (a, b), optional
        The pair (i, j) is skipped when ``i // a == j // b`` (positions in the
        two selections): atoms of one molecule.  Each must divide its side.
    box : None | array | "file"
        ``None``: free space.  ``[3]`` (or ``[6]`` with 90 degree angles): one
        box for every frame.  ``[n_traj, 3]`` / ``[n_traj, 6]``: one box a
        trajectory frame, indexed by the run's frames.  ``"file"``: the boxes
        of an ``.xtc`` path (``XTCFile.boxes``); ValueError for any other
        input.  Triclinic boxes are NotImplementedError.
    layout, device, batch_frames : as ``ContactMap``.

    ``run(start, stop, step)`` or ``run(frames=...)``.  ``results.edges`` f64
    [nbins + 1], ``results.bins`` the bin centres, ``results.count`` f64 (as
    upstream) and ``results.count_int`` int64, ``results.rdf``,
    ``results.volume`` (the mean box volume; NaN in free space),
    ``results.frames`` / ``n_frames``.  With no frames the counts are zero and
    ``rdf`` NaN.  ``rmax`` over half the shortest box edge of a frame of the
    run is a ValueError before any launch.  Residency, memory and refusals
    are ``ContactMap``'s.
    """

    _name = "InterRDF"

    def __init__(self, traj, select=None, select_b=None, nbins=75, range=(0.0, 15.0), norm="rdf",
                 exclusion_block=None, box=None, layout="fac", device=None, batch_frames=None, gpus=None):
        self.rmin, self.rmax, self.nbins = _check_range(range, nbins)
        super().__init__(traj, radius=self.rmax, select=select, select_b=select_b, layout=layout, device=device,
                         batch_frames=batch_frames, gpus=gpus)
        if norm not in NORMS:
            raise ValueError(f"norm must be one of {NORMS}, got {norm!r}")
        self.norm = norm
        if exclusion_block is not None:
            try:
                ea, eb = (int(v) for v in exclusion_block)
            except (TypeError, ValueError):
                raise ValueError(f"exclusion_block must be two integers, got {exclusion_block!r}") from None
            if ea < 1 or eb < 1:
                raise ValueError(f"exclusion_block must be positive, got {exclusion_block!r}")
            exclusion_block = (ea, eb)
        self.exclusion_block = exclusion_block
        box = _box_argument(box, traj)
        if box is None:
            if norm == "rdf":
                raise ValueError("norm='rdf' needs a box: free space has no volume (use norm='density' or 'none')")
        elif not isinstance(box, str) and box.ndim == 1 and self.rmax > 0.5 * box.min():
            # (a box a frame: run() knows which frames)
            raise ValueError(f"range ends at {self.rmax}, over half the shortest box edge ({box.min()}): the "
                             "minimum image is not the only image in range")
        self.box = box

    def _boxes(self, n_traj: int, frames: np.ndarray):
        """f64 [len(frames), 3] for the run's frames; None in free space."""
        return _run_boxes(self.box, self._input, n_traj, frames)

    def run(self, start=None, stop=None, step=None, frames=None):
        self._refuse()
        eng = Engine(self.device)
        r = self.results
        r.edges, _ = rdf_edges(self.rmin, self.rmax, self.nbins)
        r.bins = 0.5 * (r.edges[:-1] + r.edges[1:])
        with torch.cuda.device(eng.device):
            src, pos_a, pos_b, _ = self._source()
            fl = FrameList(src.n_traj, start, stop, step, frames=frames)
            r.frames = _frame_rows(fl)
            r.n_frames = self.n_frames = len(fl)
            n_a, n_b = self._sides(src, pos_a, pos_b)
            self.n_a, self.n_b = n_a, n_b
            ex = self.exclusion_block
            if ex is not None:
                if n_a % ex[0] or n_b % ex[1]:
                    raise ValueError(f"exclusion_block {ex} does not divide the selections ({n_a} and {n_b} atoms)")
                if self.symmetric and ex[0] != ex[1]:
                    raise ValueError(f"exclusion_block {ex} must be square when select_b is None")
            boxes = self._boxes(src.n_traj, np.asarray(r.frames, dtype=np.int64))
            if boxes is not None and len(boxes) and self.rmax > 0.5 * boxes.min():
                raise ValueError(f"range ends at {self.rmax}, over half the shortest box edge of the run "
                                 f"({boxes.min()}): the minimum image is not the only image in range")
            r.volume = float("nan") if boxes is None or not len(boxes) else float(
                (boxes[:, 0] * boxes[:, 1] * boxes[:, 2]).sum() / len(boxes))
            if len(fl) == 0:
                r.count_int = np.zeros(self.nbins, dtype=np.int64)
            else:
                fr = self._open(eng, src, fl, 8 * self.nbins)
                counts = eng.rdf_counts(fr.ptr, fr.fstride, len(fl), fr.n_atoms, fr.rows(pos_a), n_a,
                                        None if self.symmetric else fr.rows(pos_b), n_b, self.rmin, self.rmax,
                                        self.nbins, symmetric=self.symmetric, exclusion_block=ex, box=boxes)
                torch.cuda.current_stream(eng.device).synchronize()
                r.count_int = counts.cpu().numpy()
                del fr
        r.count = r.count_int.astype(np.float64)
        r.rdf = normalise(r.count, r.edges, r.n_frames, self.norm, n_a, n_b, r.volume, self.symmetric, ex)
        return self

    def get_cdf(self) -> np.ndarray:
        """The cumulative count around an atom of ``select``, a frame:
        ``cumsum(count) / (n_a * n_frames)``, stored as ``results.cdf``."""
        if self.n_frames is None:
            raise RuntimeError("call run() first")
        with np.errstate(invalid="ignore", divide="ignore"):
            self.results.cdf = np.cumsum(self.results.count) / (self.n_a * self.n_frames)
        return self.results.cdf


def normalise(count, edges, n_frames, norm, n_a, n_b, volume, symmetric=False, exclusion_block=None) -> np.ndarray:
    """``count / norm`` on the host in f64, upstream's formula written out:
    ``norm = n_frames``; for "rdf" and "density" ``norm *= 4/3 pi diff(edges^3)``;
    for "rdf" also ``norm *= N / volume`` with N = n_a n_b less the pairs never
    counted -- ``excl_a excl_b (n_a / excl_a)`` of an exclusion block, else the
    n_a self pairs of the symmetric route.  No frames: NaN."""
    count = np.asarray(count, dtype=np.float64)
    if n_frames == 0:
        return np.full(count.shape, np.nan)
    nrm = n_frames
    if norm in ("rdf", "density"):
        vols = np.power(edges, 3)
        nrm = nrm * (4 / 3 * np.pi * np.diff(vols))
    if norm == "rdf":
        n_pairs = n_a * n_b
        if exclusion_block is not None:
            n_pairs -= exclusion_block[0] * exclusion_block[1] * (n_a // exclusion_block[0])
        elif symmetric:
            n_pairs -= n_a
        nrm = nrm * (n_pairs / volume)
    with np.errstate(invalid="ignore", divide="ignore"):
        return count / nrm
