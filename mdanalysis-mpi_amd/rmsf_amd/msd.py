"""``EinsteinMSD`` -- the mean squared displacement of every atom at every lag
and its mean over the atoms, named as ``MDAnalysis.analysis.msd.EinsteinMSD``
names it, with the "nojump" unwrap of a trajectory that was wrapped into its
box.

One rule everywhere (csrc/msd.hip, csrc/pair_image.h, include/rmsf_hip.h), all
f64 with no FMA.  Frames are positions k = 0..F-1 in the run's frame list and
a lag counts positions, as in ``TICA``: it is a time lag only for a uniform
list.  The coordinates are f32 as stored, widened.  ``unwrap="nojump"``:
``u(0) = x(0)``, ``u(k) = u(k-1) + image(x(k) - x(k-1))`` with ``image(d) = d -
L * rint(d * (1.0 / L))`` under the box of frame k -- one in-order add chain an
atom-coordinate.  The term of atom a, origin t and lag tau is ``(dx*dx + dy*dy)
+ dz*dz`` with ``dc = u_c(t+tau) - u_c(t)``, the coordinates ``msd_type`` leaves
out left out of the expression; ``msd(a, tau)`` is the sum over the F - tau
origins, in a fixed order, divided once by ``F - tau``: within (F - tau + 8)
2^-53 relative of the exact value and the same bytes every run.
``timeseries(tau)`` is the mean over the atoms, summed on the device in a
fixed order.

The sum is the windowed one, O(F * n_lags) an atom: there is no FFT route
(``fft=`` does not exist here).  Only orthorhombic boxes.

MDAnalysis is not a dependency and is absent where this was written: the
names (``msd_type``, ``timeseries``, ``msds_by_particle``, ``delta_t_values``,
``dim_fac``) are restated from its published documentation, not verified
against it.
"""
from __future__ import annotations

import numpy as np
import torch

from .contacts import _PairAnalysis
from .distances import _frame_rows
from .engine import Engine
from .rdf import _box_argument, _run_boxes
from .sources import FrameList

# msd_type -> the mask of rmsf_msd_lags: bit 0 x, bit 1 y, bit 2 z
MSD_TYPES = {"x": 1, "y": 2, "xy": 3, "z": 4, "xz": 5, "yz": 6, "xyz": 7}


class EinsteinMSD(_PairAnalysis):
    """The mean squared displacement by the Einstein relation, mirroring
    ``MDAnalysis.analysis.msd.EinsteinMSD`` (restated, not verified).

    Parameters
    ----------
    traj : as ``ContactMap``'s input -- a float32 trajectory [F, n_atoms, 3] on
        the host or in HBM, an ``.xtc`` / ``.dcd`` path, an AtomGroup, a frame
        source.
    select : array of int, optional
        The atoms followed, in the order given; None is every atom.
    msd_type : "xyz" | "xy" | "yz" | "xz" | "x" | "y" | "z"
        The coordinates of the displacement; ``dim_fac`` is their number.
    max_lag : int, optional
        The largest lag, in positions of the run's frame list; None is F - 1.
        ``max_lag >= F`` is a ValueError.
    unwrap : None | "nojump"
        ``"nojump"`` undoes the wrapping of the trajectory into its box before
        anything is summed, and needs ``box``.
    box : None | array | "file"
        As ``InterRDF``'s: ``[3]`` (or ``[6]`` with 90 degree angles) for one
        box, ``[n_traj, 3]`` / ``[n_traj, 6]`` for one a trajectory frame,
        ``"file"`` for the boxes of an ``.xtc`` path.  Triclinic boxes are
        NotImplementedError; a box without ``unwrap``, and ``unwrap`` without
        a box, are ValueError.
    dt : float
        The time between two positions of the frame list, for
        ``delta_t_values`` alone.
    by_particle : bool
        False skips the copy of the [n_lags, n] matrix to the host.
    layout, device, batch_frames : as ``ContactMap``.

    ``run(start, stop, step)`` or ``run(frames=...)``.  ``results.timeseries``
    f64 [n_lags], ``results.msds_by_particle`` f64 [n_lags, n] (None with
    ``by_particle=False``), ``results.delta_t_values = arange(n_lags) * dt``,
    ``results.n_frames``, ``results.n_particles``, ``results.dim_fac``,
    ``results.frames``.  A run with no frames is a ValueError.

    Residency and refusals are ``ContactMap``'s: a dense HBM tensor with a
    one-run frame list is read in place through its selection, anything else
    is copied once.  The f64 planes (24 n ld bytes) plus the result (8 n_lags
    n, the mean's 8 n_lags and the workspace of a split plan,
    ``rmsf_msd_workspace_bytes``) plus that copy over half the free HBM is a
    MemoryError before anything is allocated.  One device per process;
    ``gpus=``, lists of shards, a world of more than one rank and HBM-resident
    planes are NotImplementedError.
    """

    _name = "EinsteinMSD"

    def __init__(self, traj, select=None, msd_type="xyz", max_lag=None, unwrap=None, box=None, dt=1.0,
                 by_particle=True, layout="fac", device=None, batch_frames=None, gpus=None):
        super().__init__(traj, radius=None, select=select, layout=layout, device=device, batch_frames=batch_frames,
                         gpus=gpus)
        if msd_type not in MSD_TYPES:
            raise ValueError(f"msd_type must be one of {sorted(MSD_TYPES)}, got {msd_type!r}")
        self.msd_type = msd_type
        self.dim_fac = len(msd_type)
        if max_lag is not None:
            if isinstance(max_lag, bool) or int(max_lag) != max_lag or max_lag < 0:
                raise ValueError(f"max_lag must be a non-negative integer, got {max_lag!r}")
            max_lag = int(max_lag)
        self.max_lag = max_lag
        if unwrap not in (None, "nojump"):
            raise ValueError(f"unwrap must be None or 'nojump', got {unwrap!r}")
        self.unwrap = unwrap
        box = _box_argument(box, traj)
        if unwrap is None and box is not None:
            raise ValueError("a box is used by unwrap='nojump' alone: without unwrap the coordinates are taken as "
                             "stored")
        if unwrap is not None and box is None:
            raise ValueError("unwrap='nojump' needs a box (an array of edges, or 'file' for an .xtc path)")
        self.box = box
        self.dt = float(dt)
        if not np.isfinite(self.dt):
            raise ValueError(f"dt must be finite, got {dt!r}")
        self.by_particle = bool(by_particle)

    def _n_lags(self, n_frames: int) -> int:
        if n_frames == 0:
            raise ValueError("EinsteinMSD: the run has no frames")
        if self.max_lag is not None and self.max_lag >= n_frames:
            raise ValueError(f"max_lag must be below the number of frames ({n_frames}), got {self.max_lag}")
        return n_frames if self.max_lag is None else self.max_lag + 1

    def run(self, start=None, stop=None, step=None, frames=None):
        self._refuse()
        x = self._input
        if isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim == 3:  # an array's run is known before any device is
            self._n_lags(len(FrameList(x.shape[0], start, stop, step, frames=frames)))
        eng = Engine(self.device)
        r = self.results
        with torch.cuda.device(eng.device):
            src, pos, _, _ = self._source()
            fl = FrameList(src.n_traj, start, stop, step, frames=frames)
            n_frames = len(fl)
            n_lags = self._n_lags(n_frames)
            r.frames = _frame_rows(fl)
            r.n_frames = self.n_frames = n_frames
            n = self._sides(src, pos, None)[0]
            r.n_particles, r.dim_fac = n, self.dim_fac
            r.delta_t_values = np.arange(n_lags) * self.dt
            boxes = _run_boxes(self.box, self._input, src.n_traj, np.asarray(r.frames, dtype=np.int64))
            ld = eng.msd_plane_ld(n_frames)
            work = int(eng.lib.rmsf_msd_workspace_bytes(n, n_frames, n_lags))  # (0 unless the origins are split)
            fr = self._open(eng, src, fl, 24 * n * ld + 8 * n_lags * n + 8 * n_lags + work)
            planes = eng.msd_planes(fr.ptr, fr.fstride, n_frames, fr.n_atoms, fr.rows(pos), n, box=boxes)
            msd, mean = eng.msd_lags(planes, n_frames, n_lags, MSD_TYPES[self.msd_type])
            torch.cuda.current_stream(eng.device).synchronize()
            r.timeseries = mean.cpu().numpy()
            r.msds_by_particle = msd.cpu().numpy() if self.by_particle else None
            del fr, planes, msd
        return self

    def diffusion_coefficient(self, start_lag=None, stop_lag=None) -> float:
        """The self-diffusion coefficient ``D = slope / (2 dim_fac)``, where
        slope is the least-squares slope of ``timeseries`` against
        ``delta_t_values`` over the lags ``start_lag <= tau < stop_lag``
        (defaults: every lag), in closed form on the host in f64; stored as
        ``results.D``.  The window is the caller's to choose: the ballistic
        start and the noisy tail of the curve do not belong in it."""
        if self.n_frames is None:
            raise RuntimeError("call run() first")
        t = np.asarray(self.results.delta_t_values, dtype=np.float64)
        y = np.asarray(self.results.timeseries, dtype=np.float64)
        lo = 0 if start_lag is None else int(start_lag)
        hi = len(t) if stop_lag is None else int(stop_lag)
        if not 0 <= lo < hi <= len(t) or hi - lo < 2:
            raise ValueError(f"the fit needs 0 <= start_lag < stop_lag <= {len(t)} and two lags at the least, got "
                             f"{start_lag!r}, {stop_lag!r}")
        t, y = t[lo:hi], y[lo:hi]
        tc, yc = t - t.mean(), y - y.mean()
        den = float((tc * tc).sum())
        if den == 0.0:
            raise ValueError("the fit needs lags at different times (dt is 0)")
        self.results.D = float((tc * yc).sum()) / den / (2.0 * self.dim_fac)
        return self.results.D
