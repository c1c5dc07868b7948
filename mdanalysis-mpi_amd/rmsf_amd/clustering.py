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
"""
from __future__ import annotations

import numpy as np
import torch

from . import parallel
from .distances import _PW_PLANES, DistanceMatrix
from .engine import Engine
from .rms import Results
from .sources import DeviceSource

_ONE_DEVICE = "Cluster runs on one device per process: not "
_ASYMMETRIC = "the neighbour relation (d <= cutoff) of the distance matrix is not symmetric"


class Cluster:
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
        if matrix not in ("auto", "f64", "bits"):
            raise ValueError(f"matrix must be 'auto', 'f64' or 'bits', got {matrix!r}")
        cutoff = float(cutoff)
        if not cutoff >= 0.0:
            raise ValueError(f"cutoff must be >= 0, got {cutoff}")
        if layout not in ("fac", "soa"):
            raise ValueError(f"layout must be 'fac' or 'soa', got {layout!r}")
        if isinstance(x, torch.Tensor) and x.ndim == 2 and x.device.type == "cpu":
            x = x.numpy()
        self._input = x
        self.cutoff = cutoff
        self.method = method
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
        if self.gpus is not None or isinstance(x, (list, tuple)):
            raise NotImplementedError(_ONE_DEVICE + "with gpus= or a list of shards")
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
            raise NotImplementedError(_ONE_DEVICE + "under torch.distributed with more than one rank")

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
        x, dm, r = self._input, self._dm, self.results
        host = None  # a host copy of the matrix that exists anyway
        keep = None  # what the matrix kernels read, held until the loop has synchronised
        d = adj = count = None
        form = "f64"
        if dm is x and dm.results.get("dist_matrix") is None:
            dm.run(start, stop, step, frames=frames)
        eng = Engine(self.device if dm is not x else dm.device)
        with torch.cuda.device(eng.device):
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
            if d is None and adj is None:
                return self._empty(rows)
            if adj is None:
                adj, count = eng.adjacency_pack(d, self.cutoff)
                if self.keep_matrix and host is None:
                    host = d.cpu().numpy()
                del d  # the f64 matrix is not needed past the pack
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
