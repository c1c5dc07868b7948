"""``Cluster`` -- conformational clustering of a trajectory's frames from their
all-pairs RMSD matrix, on the device.

The method is the GROMOS algorithm (Daura et al. 1999; ``gmx cluster -method
gromos``): frames within ``cutoff`` of each other are neighbours, the frame
with the most neighbours and its neighbours form the first cluster and leave,
and so on until no frame is left.  After the one threshold it is all integers
(csrc/clustering.hip): the F x F f64 matrix is packed into F^2 / 8 bytes of
neighbour bits where it lies in HBM and never crosses to the host, and the
result is the same on every run.  Where that matrix does not fit
(``matrix="bits"``, and "auto" then) the pair kernel writes the bits itself
and the matrix is never stored (csrc/pairwise.hip, ``pair_epilogue``).

The definition, shared with ``rmsf_cluster_gromos_host`` (include/rmsf_hip.h):
``adj(i, j) = (d[i, j] <= cutoff)``, the diagonal always set, a NaN never a
neighbour; the centre is the active frame with the most active neighbours,
the lowest index among equals.

``DBSCAN`` -- density clustering (Ester et al. 1996) of the same neighbour
bits, as ``sklearn.cluster.DBSCAN(metric="precomputed")`` defines it
(csrc/dbscan.hip): a frame with at least ``min_samples`` frames within ``eps``
(itself included) is a core frame, the clusters are the connected components
of the core frames, a non-core frame within ``eps`` of a core frame joins the
lowest-numbered of its core neighbours' clusters, and every other frame is
noise.  Both classes take the same inputs and make their bits by the same
routes (``_NeighbourBits``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import parallel
from .distances import _PW_PLANES, DistanceMatrix
from .engine import Engine
from .rms import Results
from .sources import DeviceSource

_ONE_DEVICE = " runs on one device per process: not "
_ASYMMETRIC = "the neighbour relation (d <= cutoff) of the distance matrix is not symmetric"


class _NeighbourBits:
    """What ``Cluster`` and ``DBSCAN`` share: the inputs they take, what they
    refuse without a device, and the way from an input to its neighbour bits
    ``d <= self.cutoff`` in HBM."""

    def _setup(self, x, cutoff: float, select, weights, superposition, zero_cutoff, layout, device, batch_frames,
               keep_matrix, matrix, gpus) -> None:
        if matrix not in ("auto", "f64", "bits"):
            raise ValueError(f"matrix must be 'auto', 'f64' or 'bits', got {matrix!r}")
        if layout not in ("fac", "soa"):
            raise ValueError(f"layout must be 'fac' or 'soa', got {layout!r}")
        if isinstance(x, torch.Tensor) and x.ndim == 2 and x.device.type == "cpu":
            x = x.numpy()
        self._input = x
        self.cutoff = cutoff
        self.device = device
        self.keep_matrix = bool(keep_matrix)
        self.gpus = gpus
        self.layout = layout
        self._dm = None
        given = isinstance(x, DistanceMatrix) or self._is_matrix(x)
        if matrix == "bits" and (keep_matrix or given):
            raise ValueError('matrix="bits" stores no f64 matrix: not with '
                             + ("keep_matrix=True" if keep_matrix else "a distance matrix as the input")
                             + ' (use matrix="f64" or "auto")')
        # a matrix that is asked for, or given, is a stored one
        self.matrix = "f64" if matrix == "auto" and (keep_matrix or given) else matrix
        if isinstance(x, DistanceMatrix):
            self._dm = x
        elif not self._is_matrix(x):
            self._dm = DistanceMatrix(x, select=select, weights=weights, superposition=superposition,
                                      cutoff=zero_cutoff, layout=layout, device=device, batch_frames=batch_frames)
        elif x.shape[0] != x.shape[1]:
            raise ValueError(f"the distance matrix must be square, got {tuple(x.shape)}")
        self.results = Results()
        self.n_frames = None

    @staticmethod
    def _is_matrix(x) -> bool:
        """A 2-D array is a distance matrix (a trajectory has three axes)."""
        return isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim == 2

    # -- what can be refused without a device ------------------------------
    def _refuse(self) -> None:
        x = self._input
        one_device = type(self).__name__ + _ONE_DEVICE
        if self.gpus is not None or isinstance(x, (list, tuple)):
            raise NotImplementedError(one_device + "with gpus= or a list of shards")
        if (isinstance(x, DeviceSource) and x.layout == "soa") or (
                isinstance(x, torch.Tensor) and x.ndim == 3 and x.device.type == "cuda" and self.layout == "soa"):
            raise NotImplementedError(_PW_PLANES)
        if self._dm is not None and self._dm is not x:
            self._dm._refuse()
        if isinstance(x, np.ndarray) and x.ndim == 2 and x.size:
            # a host matrix shows an asymmetric neighbour relation before any device is touched
            nb = np.asarray(x, dtype=np.float64) <= self.cutoff
            if not np.array_equal(nb, nb.T):
                raise ValueError(_ASYMMETRIC)
        if parallel.world()[1] > 1:
            raise NotImplementedError(one_device + "under torch.distributed with more than one rank")

    def _engine(self, start, stop, step, frames) -> Engine:
        """The engine of the run; a ``DistanceMatrix`` given and not yet run is run first."""
        x, dm = self._input, self._dm
        if dm is x and dm.results.get("dist_matrix") is None:
            dm.run(start, stop, step, frames=frames)
        return Engine(self.device if dm is not x else dm.device)

    def _neighbour_bits(self, eng: Engine, start, stop, step, frames):
        """(adj, count, rows, form, host, keep): the neighbour bits of the input
        within ``self.cutoff`` and their row counts in HBM, the frame of each
        row, "f64" or "bits" (whichever made them), the host copy of the f64
        matrix where one exists anyway or ``keep_matrix`` asks for it, and what
        the matrix kernels read, to be held until the caller has synchronised.
        ``adj`` is None with no frames.  Call it under
        ``torch.cuda.device(eng.device)``."""
        x, dm = self._input, self._dm
        host = None  # a host copy of the matrix that exists anyway
        keep = None  # what the matrix kernels read, held until the loop has synchronised
        d = adj = count = None
        form = "f64"
        if dm is x:
            host = dm.results.dist_matrix
            rows = dm.results.frames
            d = torch.as_tensor(host, device=eng.device) if host.size else None
        elif dm is not None and self.matrix == "f64":
            d, keep = dm._matrix_hbm(eng, start, stop, step, frames, bits=True)
            rows = dm.results.frames
        elif dm is not None:
            adj, count, keep = dm._adjacency_hbm(eng, self.cutoff, start, stop, step, frames, matrix=self.matrix)
            rows, form = dm.results.frames, dm.matrix_form
        else:
            if isinstance(x, np.ndarray):
                host = np.ascontiguousarray(x, dtype=np.float64)
                d = torch.as_tensor(host, device=eng.device) if host.size else None
            else:
                if x.numel() and (x.device.type != "cuda" or x.dtype != torch.float64):
                    raise ValueError("a distance matrix given as a tensor must be f64 in HBM")
                d = x.to(eng.device) if x.numel() else None
                if d is not None and d.stride(1) != 1:
                    d = d.contiguous()
                if d is not None and not bool(torch.equal(d <= self.cutoff, (d <= self.cutoff).T)):
                    raise ValueError(_ASYMMETRIC)
            rows = np.arange(x.shape[0], dtype=np.int64)
        if d is not None:
            adj, count = eng.adjacency_pack(d, self.cutoff)
            if self.keep_matrix and host is None:
                host = d.cpu().numpy()
            del d  # the f64 matrix is not needed past the pack
        return adj, count, rows, form, host, keep


class Cluster(_NeighbourBits):
    """GROMOS clusters of a trajectory's frames (or of a distance matrix).

    Parameters
    ----------
    x : trajectory | DistanceMatrix | [F, F] matrix
        A trajectory as ``DistanceMatrix`` takes it (host or HBM float32 [F,
        n_atoms, 3], an ``.xtc`` / ``.dcd`` path, an AtomGroup, a frame
        source): its RMSD matrix is computed in HBM by the calls
        ``DistanceMatrix.run`` makes, packed, clustered and freed.  Or a
        ``DistanceMatrix`` (run here if it has not been), a square host array,
        or a square f64 HBM tensor: a symmetric distance matrix of any origin.
    cutoff : float, required, >= 0
        The cluster radius (A): frames i and j are neighbours when ``d[i, j]
        <= cutoff``.
    method : "gromos"
    select, weights, superposition, layout, device, batch_frames :
        As ``DistanceMatrix`` (trajectory input only).
    zero_cutoff : float
        ``DistanceMatrix``'s ``cutoff``: distances <= it are stored as 0.
    keep_matrix : bool
        True: ``results.dist_matrix`` is the host copy of the f64 matrix.
        False (the default): the matrix is not copied to the host.
    matrix : "auto" | "f64" | "bits"
        How a trajectory's neighbour bits are made.  "f64": the F x F f64
        matrix is stored in HBM (8 F^2 bytes), packed and freed.  "bits": the
        pair kernel's epilogue writes the bits themselves
        (``rmsf_pairwise_adjacency``) -- the same words, F^2 / 8 bytes and no
        matrix, which is what fits at 10^5 - 10^6 frames; not with
        ``keep_matrix=True`` or a matrix as the input (ValueError).  "auto"
        (the default): "f64" wherever that fits in half the free HBM, or a
        matrix is asked for or given; "bits" where it does not; MemoryError
        only if the bits do not fit either.

    ``run(start, stop, step)`` or ``run(frames=...)`` as ``DistanceMatrix.run``
    (trajectory and ``DistanceMatrix`` inputs).  Results:

    ``results.labels``   int64 [F]: the cluster of each row; clusters are
                         numbered as found, so the largest is 0.
    ``results.centres``  int64 [n_clusters]: the row of each cluster's centre;
                         ``results.frames[centres]`` are trajectory frames.
    ``results.sizes``    int64 [n_clusters], non-increasing.
    ``results.n_neighbours``  int64 [F]: the frames within ``cutoff`` of each
                         row, itself included (the bit rows' counts).
    ``results.matrix_form``  "f64" or "bits", whichever ran.
    ``results.n_clusters``, ``results.frames``, ``results.n_frames``.

    A supplied matrix must be square and its neighbour relation ``d <=
    cutoff`` symmetric (ValueError).  No frames: empty results.  One device
    per process: ``gpus=``, lists of shards, a ``torch.distributed`` world of
    more than one rank and HBM-resident coordinate planes are
    NotImplementedError.
    """

    def __init__(self, x, *, cutoff: float, method: str = "gromos", select=None, weights=None,
                 superposition: bool = True, zero_cutoff: float = 1e-5, layout: str = "fac", device=None,
                 batch_frames: int | None = None, keep_matrix: bool = False, matrix: str = "auto", gpus=None):
        if method != "gromos":
            raise ValueError(f"method must be 'gromos', got {method!r}")
        cutoff = float(cutoff)
        if not cutoff >= 0.0:
            raise ValueError(f"cutoff must be >= 0, got {cutoff}")
        self.method = method
        self._setup(x, cutoff, select, weights, superposition, zero_cutoff, layout, device, batch_frames, keep_matrix,
                    matrix, gpus)

    def _empty(self, n_frames_rows=None):
        r = self.results
        r.labels = np.zeros(0, dtype=np.int64)
        r.centres = np.zeros(0, dtype=np.int64)
        r.sizes = np.zeros(0, dtype=np.int64)
        r.n_neighbours = np.zeros(0, dtype=np.int64)
        r.matrix_form = None  # nothing ran
        r.n_clusters = 0
        r.n_frames = self.n_frames = 0
        r.frames = np.zeros(0, dtype=np.int64) if n_frames_rows is None else n_frames_rows
        r.dist_matrix = np.zeros((0, 0)) if self.keep_matrix else None
        return self

    def run(self, start=None, stop=None, step=None, frames=None, **kwargs):
        self._refuse()
        r = self.results
        eng = self._engine(start, stop, step, frames)
        with torch.cuda.device(eng.device):
            adj, count, rows, form, host, keep = self._neighbour_bits(eng, start, stop, step, frames)
            if adj is None:
                return self._empty(rows)
            n = adj.shape[0]
            label, centre, size = eng.cluster_gromos(adj, count)
            del keep
            r.labels = label.cpu().numpy().astype(np.int64)
            r.centres = centre.cpu().numpy().astype(np.int64)
            r.sizes = size.cpu().numpy().astype(np.int64)
            r.n_neighbours = count.cpu().numpy().astype(np.int64)
            r.n_clusters = int(r.centres.size)
            r.frames = np.asarray(rows, dtype=np.int64)
            r.n_frames = self.n_frames = n
            r.matrix_form = form
            r.dist_matrix = host if self.keep_matrix else None
        return self


class DBSCAN(_NeighbourBits):
    """DBSCAN clusters of a trajectory's frames (or of a distance matrix), as
    ``sklearn.cluster.DBSCAN(eps, min_samples, metric="precomputed")`` defines
    them on the RMSD matrix, on the device (csrc/dbscan.hip).

    Parameters
    ----------
    x : trajectory | DistanceMatrix | [F, F] matrix
        As ``Cluster``.
    eps : float, required, >= 0
        Frames i and j are neighbours when ``d[i, j] <= eps`` (A).
    min_samples : int >= 1
        A frame with at least this many frames within ``eps``, itself
        included, is a core frame.  1: every frame is one, and the clusters
        are single linkage cut at ``eps`` (``gmx cluster -method linkage``).
    select, weights, superposition, zero_cutoff, layout, device, batch_frames,
    keep_matrix, matrix :
        As ``Cluster``: the neighbour bits are ``Cluster``'s, by the same routes.

    ``run(start, stop, step)`` or ``run(frames=...)`` as ``Cluster.run``.
    The definition needs no visiting order: the clusters are the connected
    components of the neighbour relation among the core frames, numbered by
    their lowest core frame; a non-core frame with a core neighbour (a border
    frame) takes the lowest-numbered of its core neighbours' clusters; every
    other frame is noise.  On a finite matrix this is scikit-learn's result,
    ``labels_`` and ``core_sample_indices_`` alike.  A frame with a non-finite
    coordinate has no neighbour but itself: noise for ``min_samples >= 2``.
    Results:

    ``results.labels``   int64 [F]: the cluster of each row, -1 for noise.
    ``results.core_sample_indices``  int64, ascending: the core rows.
    ``results.sizes``    int64 [n_clusters], in label order.
    ``results.n_noise``  the rows labelled -1.
    ``results.n_neighbours``  int64 [F]: the frames within ``eps`` of each row,
                         itself included.
    ``results.n_rounds`` the rounds the component loop took, the one that
                         changed nothing included.
    ``results.matrix_form``  "f64" or "bits", whichever ran.
    ``results.n_clusters``, ``results.frames``, ``results.n_frames``, and
    ``results.dist_matrix`` with ``keep_matrix=True``.

    The refusals are ``Cluster``'s.  No frames: empty results.
    """

    def __init__(self, x, *, eps: float, min_samples: int = 5, select=None, weights=None, superposition: bool = True,
                 zero_cutoff: float = 1e-5, layout: str = "fac", device=None, batch_frames: int | None = None,
                 keep_matrix: bool = False, matrix: str = "auto", gpus=None):
        eps = float(eps)
        if not eps >= 0.0:
            raise ValueError(f"eps must be >= 0, got {eps}")
        if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or min_samples < 1:
            raise ValueError(f"min_samples must be an integer >= 1, got {min_samples!r}")
        self.eps = eps
        self.min_samples = int(min_samples)
        self._setup(x, eps, select, weights, superposition, zero_cutoff, layout, device, batch_frames, keep_matrix,
                    matrix, gpus)

    def _empty(self, rows=None):
        r = self.results
        r.labels = np.zeros(0, dtype=np.int64)
        r.core_sample_indices = np.zeros(0, dtype=np.int64)
        r.sizes = np.zeros(0, dtype=np.int64)
        r.n_neighbours = np.zeros(0, dtype=np.int64)
        r.matrix_form = None  # nothing ran
        r.n_clusters = r.n_noise = r.n_rounds = 0
        r.n_frames = self.n_frames = 0
        r.frames = np.zeros(0, dtype=np.int64) if rows is None else rows
        r.dist_matrix = np.zeros((0, 0)) if self.keep_matrix else None
        return self

    def run(self, start=None, stop=None, step=None, frames=None, **kwargs):
        self._refuse()
        r = self.results
        eng = self._engine(start, stop, step, frames)
        with torch.cuda.device(eng.device):
            adj, count, rows, form, host, keep = self._neighbour_bits(eng, start, stop, step, frames)
            if adj is None:
                return self._empty(rows)
            n = adj.shape[0]
            label, core, n_clusters, n_rounds = eng.cluster_dbscan(adj, count, self.min_samples)
            del keep
            r.labels = label.cpu().numpy().astype(np.int64)
            bits = np.unpackbits(core.cpu().numpy().view(np.uint8), bitorder="little")[:n]
            r.core_sample_indices = np.flatnonzero(bits).astype(np.int64)
            r.n_clusters = int(n_clusters)
            r.sizes = np.bincount(r.labels[r.labels >= 0], minlength=r.n_clusters).astype(np.int64)
            r.n_noise = int((r.labels < 0).sum())
            r.n_neighbours = count.cpu().numpy().astype(np.int64)
            r.n_rounds = int(n_rounds)
            r.frames = np.asarray(rows, dtype=np.int64)
            r.n_frames = self.n_frames = n
            r.matrix_form = form
            r.dist_matrix = host if self.keep_matrix else None
        return self
