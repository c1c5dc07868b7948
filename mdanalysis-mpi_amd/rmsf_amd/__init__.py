"""rmsf_amd -- MI355X-native frame-parallel RMSF (drop-in for the hot path of
i2nico/MDAnalysis-MPI ``RMSF.py``).

Public surface (mirrors the reference's names):
  * ``RMSF(atomgroup, align=...).run(start, stop, step).results.rmsf``
  * ``second_order_moments`` / ``get_rotation_matrix`` / ``CalcRMSDRotationalMatrix``
    (device-backed versions of RMSF.py:36-51 and MDAnalysis.lib.qcprot)
  * ``blocks`` -- the RMSF.py:65-69 frame decomposition
  * ``PCA`` / ``pca_from_comoment`` -- the modes of the positional covariance
    (``RMSF(..., covariance=True)``), named as MDAnalysis.analysis.pca.PCA names them;
    ``PCA.transform`` projects a trajectory on them on the device, ``cosine_content``
    measures such a projection's convergence; ``PCA(solver="device")`` finds the first modes
    on the device (``rmsf_amd.eigen.top_eigenpairs``) and raises ``PCAConvergenceError`` when it cannot;
    ``PCA(solver="matrix_free")`` finds them from the trajectory with no [3n, 3n] matrix at all;
    ``rmsip`` / ``cumulative_overlap`` compare two sets of modes
  * ``DistanceMatrix`` / ``DiffusionMap`` -- the all-pairs RMSD matrix of the frames and
    its diffusion map, named as MDAnalysis.analysis.diffusionmap names them;
    ``DiffusionMap(DistanceMatrix(traj), epsilon, n_eigenvectors=k, solver="device")`` finds the first k
    diffusion coordinates with the matrix and its kernel kept in HBM (``rmsf_amd.eigen.KernelOps``)
  * ``CrossDistanceMatrix`` -- the rectangular RMSD matrix of every frame of one trajectory to
    every frame of another (or to a set of references) and each frame's nearest reference;
    ``hausdorff`` / ``discrete_frechet`` -- the path distances of such a matrix, named as
    MDAnalysis.analysis.psa names them
  * ``Cluster`` -- GROMOS clustering (Daura et al. 1999) of the frames from their RMSD matrix,
    which is thresholded into neighbour bits and clustered in HBM without crossing to the host:
    ``Cluster(traj, cutoff=1.5).run().results.labels`` / ``.centres`` / ``.sizes``
  * ``DBSCAN`` -- density clustering of the same neighbour bits, named as sklearn.cluster.DBSCAN
    names it and equal to it with ``metric="precomputed"``: core frames, their connected components,
    border frames and noise (-1), all in HBM:
    ``DBSCAN(traj, eps=1.5, min_samples=5).run().results.labels`` / ``.core_sample_indices``
  * ``TICA`` / ``tica_from_comoments`` -- the slowest modes of the trajectory from the covariance and the
    time-lagged covariance of the (aligned) coordinates, the latter on the f64 matrix cores with its two
    operands ``lag`` frames apart: ``TICA(traj, lag=10).run().results.timescales`` / ``.components``;
    ``TICA.transform`` projects on them as ``PCA.transform`` does
  * ``Contacts`` / ``ContactMap`` -- distances between atoms within a frame: the fraction of native
    contacts Q(t), named as MDAnalysis.analysis.contacts.Contacts names it, and the count of frames in
    which each pair of two selections touches; ``contact_threshold_sq`` is the squared cutoff the device
    compares against.  No periodic boundary conditions
  * ``InterRDF`` -- the radial distribution function g(r) of two selections, named as
    MDAnalysis.analysis.rdf.InterRDF names it, free or under the minimum image of per-frame orthorhombic
    boxes (arrays, or an ``.xtc`` file's own): ``InterRDF(traj, box=(30, 30, 30)).run().results.rdf``;
    ``rdf_edges`` gives the bin edges and the squared thresholds the device compares against
  * ``EinsteinMSD`` -- the mean squared displacement of every atom at every lag and its mean over the
    atoms, named as MDAnalysis.analysis.msd.EinsteinMSD names it, by the windowed sum on the f64 vector
    units, with the "nojump" unwrap of a wrapped trajectory under per-frame orthorhombic boxes:
    ``EinsteinMSD(traj, unwrap="nojump", box="file").run().results.timeseries``;
    ``diffusion_coefficient`` fits the slope
"""
from ._lib import RmsfEmptyError, RmsfError, load as load_library
from .parallel import blocks
from .qcprot import CalcRMSDRotationalMatrix, get_rotation_matrix
from .moments import second_order_moments
from .rms import RMSF, Results
from .eigen import PCAConvergenceError
from .pca import PCA, cosine_content, cumulative_overlap, pca_from_comoment, rmsip
from .distances import CrossDistanceMatrix, DiffusionMap, DistanceMatrix, discrete_frechet, hausdorff
from .clustering import DBSCAN, Cluster
from .tica import TICA, tica_from_comoments
from .contacts import ContactMap, Contacts, contact_threshold_sq
from .rdf import InterRDF, rdf_edges
from .msd import EinsteinMSD

__all__ = [
    "EinsteinMSD",
    "InterRDF",
    "rdf_edges",
    "ContactMap",
    "Contacts",
    "contact_threshold_sq",
    "TICA",
    "tica_from_comoments",
    "RMSF",
    "Results",
    "PCA",
    "pca_from_comoment",
    "cosine_content",
    "rmsip",
    "cumulative_overlap",
    "PCAConvergenceError",
    "DistanceMatrix",
    "DiffusionMap",
    "CrossDistanceMatrix",
    "hausdorff",
    "discrete_frechet",
    "Cluster",
    "DBSCAN",
    "blocks",
    "second_order_moments",
    "get_rotation_matrix",
    "CalcRMSDRotationalMatrix",
    "RmsfError",
    "RmsfEmptyError",
    "load_library",
]
