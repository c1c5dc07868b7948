"""``Contacts`` and ``ContactMap`` -- distances between atoms within a frame:
the fraction of native contacts Q(t) along a trajectory, named as
``MDAnalysis.analysis.contacts.Contacts`` names it, and the contact count /
frequency map of two selections.

One rule decides a contact everywhere (csrc/contacts.hip, include/rmsf_hip.h):
the coordinates are f32 as stored, ``dx = (double)xa - (double)xb`` and so for
y and z, ``d2 = (dx*dx + dy*dy) + dz*dz`` with no FMA, ``d = sqrt(d2)``
correctly rounded, and a pair is in contact iff ``d <= radius``.  A NaN is
never a contact: an atom with a non-finite coordinate in a frame loses its
pairs in that frame and nothing else changes.  numpy evaluates the same
expression to the same bits, so counts are compared with it for equality.

No periodic boundary conditions are applied: these classes take no box (only
``InterRDF`` does), and a pair across a periodic image is as far apart as its
stored coordinates say.

Contacts are invariant under superposition, so nothing is aligned.  Nothing of
the size [F, n, n] is ever formed: the count kernel keeps a tile of integer
counters in registers and streams the frames through LDS.

MDAnalysis is not a dependency and is absent where this was written: the
methods' names and semantics (``hard_cut``, ``radius_cut``, ``soft_cut`` and its
``beta`` / ``lambda_constant``, ``timeseries``) are restated from its published
documentation, not verified against it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, parallel
from .distances import _PW_PLANES, _frame_rows, _in_place_run, resident_frames
from .engine import Engine
from .rms import Results, make_source
from .sources import DeviceSource, FrameList

METHODS = {"hard_cut": _lib.RMSF_CONTACT_HARD_CUT, "radius_cut": _lib.RMSF_CONTACT_RADIUS_CUT,
           "soft_cut": _lib.RMSF_CONTACT_SOFT_CUT}


def _check_radius(radius) -> float:
    r = float(radius)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"radius must be positive and finite, got {radius!r}")
    return r


def contact_threshold_sq(radius: float) -> float:
    """The largest f64 ``t`` with ``sqrt(t) <= radius``: ``radius * radius``
    moved by ``nextafter`` where its rounding fell on the wrong side.  The
    correctly rounded square root is monotone, so ``d2 <= t`` is exactly
    ``sqrt(d2) <= radius`` -- what the device compares, with no root a pair
    (rmsf_contact_threshold_sq; host only)."""
    return float(_lib.load().rmsf_contact_threshold_sq(_check_radius(radius)))


def pair_distances(xa: np.ndarray, xb: np.ndarray) -> np.ndarray:
    """f64 [..., n_a, n_b] distances of f32 rows ``xa`` [..., n_a, 3] and
    ``xb`` [..., n_b, 3] by the rule above, on the host."""
    a = np.asarray(xa, dtype=np.float32).astype(np.float64)[..., :, None, :]
    b = np.asarray(xb, dtype=np.float32).astype(np.float64)[..., None, :, :]
    d = a - b
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def native_pairs(ref_a: np.ndarray, ref_b: np.ndarray, radius: float):
    """(pairs int64 [P, 2], r0 f64 [P]): the pairs (i, j) of rows of the
    reference coordinates ``ref_a`` [n_a, 3] and ``ref_b`` [n_b, 3] in contact
    at ``radius``, in row-major order, and their reference distances."""
    d = pair_distances(ref_a, ref_b)
    with np.errstate(invalid="ignore"):
        i, j = np.nonzero(d <= _check_radius(radius))
    return np.stack([i, j], axis=1).astype(np.int64), d[i, j]


def _selection(sel, what: str):
    if sel is None:
        return None
    s = np.asarray(sel)
    if s.size and not np.issubdtype(s.dtype, np.integer):
        raise TypeError(f"{what} must be integer atom indices, got dtype {s.dtype}")
    s = s.astype(np.int64).reshape(-1)
    if s.size == 0:
        raise ValueError(f"{what} selects no atoms")
    if s.min() < 0:
        raise IndexError(f"{what}: a negative atom index")
    return s


def _is_source(x) -> bool:
    """Inputs that carry their own atoms (``make_source`` ignores ``select``
    for them): a frame source, an AtomGroup."""
    return (hasattr(x, "batches") and hasattr(x, "reference") and hasattr(x, "n_sel")) or (
        hasattr(x, "universe") and hasattr(x, "positions"))


class _Frames:
    """What both classes' kernels read: the frames at a constant stride, and
    ``rows(pos)``, the rows in such a frame of the source's rows ``pos`` (None
    for all of them, in and out)."""

    def __init__(self, keep, ptr, fstride, n_atoms, base):
        self.keep, self.ptr, self.fstride, self.n_atoms, self.base = keep, ptr, fstride, n_atoms, base

    def rows(self, pos):
        if self.base is None:
            return pos
        return self.base if pos is None else self.base[pos]


class _PairAnalysis:
    """The inputs, the refusals and the residency ``ContactMap`` and
    ``Contacts`` share.  One source is built over the sorted union of the two
    selections and each side is an index array into its rows; the kernels
    gather through it, composed with the source's own selection where an HBM
    tensor is read in place."""

    _name = "ContactMap"

    def __init__(self, traj, radius=4.5, select=None, select_b=None, layout="fac", device=None,
                 batch_frames=None, gpus=None):
        if layout not in ("fac", "soa"):
            raise ValueError(f"layout must be 'fac' or 'soa', got {layout!r}")
        self._input = traj
        self.radius = None if radius is None else _check_radius(radius)  # (None: an analysis with no distance)
        self.select = _selection(select, "select")
        self.select_b = _selection(select_b, "select_b")
        self.symmetric = select_b is None
        self.layout = layout
        self.device = device
        self.batch_frames = batch_frames
        self.gpus = gpus
        self.results = Results()
        self.n_frames = None

    def _refuse(self) -> None:
        x = self._input
        if self.gpus is not None or isinstance(x, (list, tuple)):
            raise NotImplementedError(f"{self._name} runs on one device per process: not with gpus= or a list of "
                                      "shards")
        if (isinstance(x, DeviceSource) and x.layout == "soa") or (
                isinstance(x, torch.Tensor) and x.device.type == "cuda" and self.layout == "soa"):
            raise NotImplementedError(_PW_PLANES.replace("DistanceMatrix", self._name))
        if parallel.world()[1] > 1:
            raise NotImplementedError(f"{self._name} runs on one device per process: not under torch.distributed "
                                      "with more than one rank")

    def _source(self):
        """(source, positions of A in its rows, positions of B, the atoms its
        rows are) -- None for all rows in order, and for every atom."""
        x, a, b = self._input, self.select, self.select_b
        if _is_source(x) or a is None:
            src, _ = make_source(x, select=None, align=None, batch_frames=self.batch_frames, layout=self.layout,
                                 group_masses=False)
            for s, what in ((a, "select"), (b, "select_b")):
                if s is not None and s.max() >= src.n_sel:
                    raise IndexError(f"{what}: atom index {int(s.max())} is out of range for {src.n_sel} atoms")
            return src, a, b, None
        union = np.unique(a if b is None else np.concatenate([a, b]))
        src, _ = make_source(x, select=union, align=None, batch_frames=self.batch_frames, layout=self.layout,
                             group_masses=False)

        def pos(s):
            p = np.searchsorted(union, s)
            return None if p.size == union.size and np.array_equal(p, np.arange(union.size)) else p

        return src, pos(a), None if b is None else pos(b), union

    def _sides(self, src, pos_a, pos_b):
        n_a = src.n_sel if pos_a is None else len(pos_a)
        return n_a, n_a if self.symmetric else (src.n_sel if pos_b is None else len(pos_b))

    def _open(self, eng: Engine, src, fl: FrameList, result_bytes: int) -> _Frames:
        """The frames of ``fl`` resident (``resident_frames``' rule);
        MemoryError before anything is allocated when the result and the dense
        copy are over half the free HBM."""
        def check(dense_bytes):
            free = torch.cuda.mem_get_info(eng.device)[0]
            if result_bytes + dense_bytes > free // 2:
                raise MemoryError(f"{self._name}: the result needs {result_bytes} bytes"
                                  + (f" and the dense copy of the selected rows {dense_bytes} bytes" if dense_bytes
                                     else "") + f", over half of the {free} bytes of free HBM")

        in_place = _in_place_run(src, fl) is not None
        keep, ptr, fstride, sel = resident_frames(eng, src, fl, self.batch_frames, check)
        if in_place:  # the kernels gather through the source's own selection
            return _Frames((src, keep), ptr, fstride, src.n_atoms, src.sel_host if sel is not None else None)
        return _Frames((src, keep), ptr, fstride, src.n_sel, None)


class ContactMap(_PairAnalysis):
    """How often each pair of atoms touches: ``results.counts[i, j]`` (int64
    [n_a, n_b]) is the number of frames in which atom i of ``select`` and atom
    j of ``select_b`` are within ``radius`` of each other, and
    ``results.frequency = counts / n_frames``.  The rule is the module's: f64
    differences of the f32 coordinates, ``d <= radius``, a NaN never a
    contact.  No periodic boundary conditions are applied -- there is no
    ``box=`` here yet.

    Parameters
    ----------
    traj : as ``DistanceMatrix``'s input -- a float32 trajectory [F, n_atoms, 3]
        on the host or in HBM, an ``.xtc`` / ``.dcd`` path, an AtomGroup, a
        frame source.
    radius : float
        The contact distance, positive and finite (ValueError otherwise).
    select, select_b : array of int, optional
        The atoms of the rows and of the columns, in the order given (indices
        into the trajectory's atoms; into the group's or the source's own
        atoms for an AtomGroup or a frame source).  ``select=None`` is every
        atom.  ``select_b=None``: the map of ``select`` against itself, by the
        symmetric route -- tiles on or above the diagonal are computed and
        mirrored, so the result is symmetric in its bits; the diagonal is
        computed like any other entry (an atom touches itself in every frame
        in which its coordinates are finite).
    layout, device, batch_frames : as ``DistanceMatrix``.

    ``run(start, stop, step)`` or ``run(frames=...)`` as ``RMSF.run``;
    ``results.frames`` are the trajectory indices counted, ``results.n_frames``
    their number.  With no frames the counts are zero and the frequency NaN.

    One source is read, over the sorted union of the two selections; residency
    is ``DistanceMatrix``'s: a dense HBM tensor with a one-run frame list is
    read in place, the selections gathered in the kernel; anything else is
    copied once into a dense f32 buffer.  The int32 counts plus that copy over
    half the free HBM is a MemoryError.  One device per process; ``gpus=``,
    lists of shards, a world of more than one rank and HBM-resident planes are
    NotImplementedError.
    """

    def run(self, start=None, stop=None, step=None, frames=None):
        self._refuse()
        eng = Engine(self.device)
        r = self.results
        with torch.cuda.device(eng.device):
            src, pos_a, pos_b, _ = self._source()
            fl = FrameList(src.n_traj, start, stop, step, frames=frames)
            r.frames = _frame_rows(fl)
            r.n_frames = self.n_frames = len(fl)
            n_a, n_b = self._sides(src, pos_a, pos_b)
            if len(fl) == 0:
                r.counts = np.zeros((n_a, n_b), dtype=np.int64)
                r.frequency = np.full((n_a, n_b), np.nan)
                return self
            fr = self._open(eng, src, fl, 4 * n_a * n_b)
            counts = eng.contact_counts(fr.ptr, fr.fstride, len(fl), fr.n_atoms, fr.rows(pos_a), n_a,
                                        None if self.symmetric else fr.rows(pos_b), n_b, self.radius,
                                        symmetric=self.symmetric)
            torch.cuda.current_stream(eng.device).synchronize()
            r.counts = counts.cpu().numpy().astype(np.int64)
            del fr
        r.frequency = r.counts / float(r.n_frames)
        return self


class Contacts(_PairAnalysis):
    """The fraction of native contacts Q(t), mirroring
    ``MDAnalysis.analysis.contacts.Contacts`` (restated, not verified).

    The native pairs are the pairs (atom i of ``select``, atom j of
    ``select_b``) in contact at ``radius`` in the reference, found on the host
    by the module's rule and listed in row-major order; ``r0`` are their
    reference distances.  ``select_b=None`` pairs ``select`` with itself, every
    ordered pair (i, j), the diagonal included, as the rule finds them.  For
    each frame, over the P native pairs with distance d:

      ``hard_cut`` / ``radius_cut``  n = #(d <= radius), q = n / P -- one f64
          division, numpy's bits; ``r0`` is not used.
      ``soft_cut``  q = (1 / P) sum 1 / (1 + exp(beta * (d - lambda_constant * r0)))
          summed in a fixed order on the device: the same bits every run, and
          within (P + 8) 2^-53 relative of the exact sum.  ``n_contacts`` is
          still the hard count at ``radius``.  The formula is taken as written:
          a native pair with a non-finite coordinate in a frame has a NaN
          term and makes that frame's soft q NaN, as numpy's would be.

    No periodic boundary conditions are applied -- there is no ``box=`` here yet.

    Parameters
    ----------
    traj, select, select_b, radius, layout, device, batch_frames :
        as ``ContactMap``.
    reference : int | array [n_atoms, 3]
        A frame of the trajectory (default the first), or f32 coordinates of
        all the atoms ``select`` / ``select_b`` index.
    pairs : (i, j), optional
        The pairs to follow instead of the reference's contacts: two equally
        long arrays of positions in ``select`` and in ``select_b``.  ``r0`` is
        still taken from the reference.
    method : "hard_cut" | "radius_cut" | "soft_cut"
    beta, lambda_constant : float
        ``soft_cut``'s parameters (upstream's defaults, 5.0 and 1.8).

    ``run(start, stop, step)`` or ``run(frames=...)``.  ``results.timeseries``
    f64 [F, 2] (frame, q) as upstream; ``results.q`` f64 [F];
    ``results.n_contacts`` int64 [F]; ``results.pairs`` int64 [P, 2], positions
    in the two selections; ``results.r0`` f64 [P]; ``results.frames`` /
    ``n_frames``.  A reference with no native pairs is a ValueError.
    Residency, memory and refusals are ``ContactMap``'s.
    """

    _name = "Contacts"

    def __init__(self, traj, select=None, select_b=None, reference=0, pairs=None, radius=4.5,
                 method="hard_cut", beta=5.0, lambda_constant=1.8, layout="fac", device=None, batch_frames=None,
                 gpus=None):
        super().__init__(traj, radius=radius, select=select, select_b=select_b, layout=layout, device=device,
                         batch_frames=batch_frames, gpus=gpus)
        if method not in METHODS:
            raise ValueError(f"method must be one of {sorted(METHODS)}, got {method!r}")
        self.method = method
        self.beta, self.lambda_constant = float(beta), float(lambda_constant)
        if not (np.isfinite(self.beta) and np.isfinite(self.lambda_constant)):
            raise ValueError("beta and lambda_constant must be finite")
        self.reference = reference
        if pairs is not None:
            i, j = (_selection(p, "pairs") for p in pairs)
            if i.size != j.size:
                raise ValueError(f"pairs must be two arrays of one length, got {i.size} and {j.size}")
            pairs = np.stack([i, j], axis=1)
        self.pairs = pairs
        if not isinstance(reference, (int, np.integer)):
            ref = np.asarray(reference)
            if ref.ndim != 2 or ref.shape[1] != 3:
                raise ValueError(f"reference must be a frame index or an [n_atoms, 3] array, got shape {ref.shape}")

    def _reference_rows(self, eng: Engine, src, atoms) -> np.ndarray:
        """f32 [n_sel, 3]: the reference's coordinates of the source's rows
        (``atoms``: which atoms those are, None for every atom)."""
        ref = self.reference
        if isinstance(ref, (int, np.integer)):
            one = FrameList(src.n_traj, frames=[int(ref)])
            keep, ptr, fstride, sel = resident_frames(eng, src, one, None, lambda _: None)
            out = torch.empty((1, src.n_sel, 3), dtype=torch.float32, device=eng.device)
            eng.gather_frames(ptr, fstride, eng.zero_index(), 1, src.n_sel, sel, out)
            torch.cuda.current_stream(eng.device).synchronize()
            del keep
            return out[0].cpu().numpy()
        ref = np.ascontiguousarray(ref, dtype=np.float32)
        if atoms is not None:
            if atoms.max() >= ref.shape[0]:
                raise ValueError(f"the reference has {ref.shape[0]} atoms, the selections reach atom "
                                 f"{int(atoms.max())}")
            return ref[atoms]
        if ref.shape[0] != src.n_sel:
            raise ValueError(f"the reference has {ref.shape[0]} atoms, the trajectory {src.n_sel}")
        return ref

    def _native(self, ref_rows: np.ndarray, pos_a, pos_b):
        ra = ref_rows if pos_a is None else ref_rows[pos_a]
        rb = ra if self.symmetric else (ref_rows if pos_b is None else ref_rows[pos_b])
        if self.pairs is None:
            pairs, r0 = native_pairs(ra, rb, self.radius)
            if not len(pairs):
                raise ValueError(f"the reference has no pair of the two selections within {self.radius}: Q is 0 / 0")
            return pairs, r0
        pairs = self.pairs
        if pairs[:, 0].max() >= len(ra) or pairs[:, 1].max() >= len(rb):
            raise IndexError(f"pairs index past the selections ({len(ra)} and {len(rb)} atoms)")
        d = ra[pairs[:, 0]].astype(np.float64) - rb[pairs[:, 1]].astype(np.float64)
        return pairs, np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])

    def run(self, start=None, stop=None, step=None, frames=None):
        self._refuse()
        eng = Engine(self.device)
        r = self.results
        with torch.cuda.device(eng.device):
            src, pos_a, pos_b, atoms = self._source()
            fl = FrameList(src.n_traj, start, stop, step, frames=frames)
            n_frames = len(fl)
            r.frames = _frame_rows(fl)
            r.n_frames = self.n_frames = n_frames
            pairs, r0 = self._native(self._reference_rows(eng, src, atoms), pos_a, pos_b)
            r.pairs, r.r0 = pairs, r0
            if n_frames == 0:
                r.q, r.n_contacts = np.zeros(0), np.zeros(0, dtype=np.int64)
                r.timeseries = np.zeros((0, 2))
                return self
            # the pairs as rows of the source; the kernel stages those rows once a frame
            side_b = pos_a if self.symmetric else pos_b
            in_a = pairs[:, 0] if pos_a is None else pos_a[pairs[:, 0]]
            in_b = pairs[:, 1] if side_b is None else side_b[pairs[:, 1]]
            fr = self._open(eng, src, fl, 12 * n_frames)
            q, n = eng.contact_fraction(fr.ptr, fr.fstride, n_frames, fr.n_atoms, fr.rows(None), src.n_sel, in_a, in_b,
                                        r0, self.radius, METHODS[self.method], self.beta, self.lambda_constant)
            torch.cuda.current_stream(eng.device).synchronize()
            r.q = q.cpu().numpy()
            r.n_contacts = n.cpu().numpy().astype(np.int64)
            del fr
        r.timeseries = np.stack([r.frames.astype(np.float64), r.q], axis=1)
        return self
