"""``PCA`` -- the principal components of the positional covariance, named as
``MDAnalysis.analysis.pca.PCA`` names them.

The workflow RMSF.py restates (AverageStructure -> AlignTraj -> rms.RMSF) is
also the preamble of ``pca.PCA``: the covariance of the aligned coordinates,
of which the RMSF is the diagonal.  ``RMSF(..., covariance=True)`` forms that
matrix on the device (csrc/covariance.hip, the f64 matrix cores) from the
very coordinates the Welford sweep reads; the eigen-decomposition of the
[3n, 3n] f64 matrix is ``numpy.linalg.eigh`` on the host.

``transform()`` -- the projection of a trajectory on the components -- is not
part of this module.
"""
from __future__ import annotations

import numpy as np

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
    """

    def __init__(self, atomgroup, select=None, align="average", n_components: int | None = None, ddof: int = 1,
                 **rmsf_kwargs):
        rmsf_kwargs.pop("covariance", None)
        self.n_components = n_components
        self.ddof = int(ddof)
        self._rmsf = RMSF(atomgroup, select=select, align=align, covariance=True, **rmsf_kwargs)
        self.results = Results()

    def run(self, start=None, stop=None, step=None, frames=None, **kwargs):
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
