"""Device engine: thin typed wrappers around the C ABI on torch-allocated HBM.

torch is plumbing here (the caching allocator for HBM buffers, the current
HIP stream, torch.distributed for RCCL); every byte of arithmetic on the hot
path runs in the hand-written HIP kernels of csrc/rmsf_kernels.hip.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import RMSF_MODE_SUM, RMSF_MODE_WELFORD, RMSF_REFINFO_DOUBLES, RMSF_XFORM_DOUBLES, call

F64 = torch.float64
F32 = torch.float32


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


class Engine:
    """Launches the RMSF kernels on one device, on torch's current stream."""

    def __init__(self, device: torch.device | int | str | None = None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("rmsf_amd needs a HIP device (MI355X); none is visible -- no CPU fallback exists")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"rmsf_amd runs on HIP devices only, got {self.device}")
        call("rmsf_set_device", self.device.index if self.device.index is not None else 0)

    # -- helpers -----------------------------------------------------------
    @property
    def stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    @property
    def side_stream(self) -> torch.cuda.Stream:
        """A second stream on the device, for work that must not queue ahead
        of the launching stream's kernels (the merge shift's gather)."""
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(self.device)
        return self._side

    def empty(self, *shape, dtype=F64) -> torch.Tensor:
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def zeros(self, *shape, dtype=F64) -> torch.Tensor:
        return torch.zeros(*shape, dtype=dtype, device=self.device)

    def sel_tensor(self, sel) -> torch.Tensor | None:
        if sel is None:
            return None
        s = torch.as_tensor(np.ascontiguousarray(sel, dtype=np.int32)).to(self.device)
        return s

    # -- kernels -----------------------------------------------------------
    def reference_setup(self, n_sel: int, *, frame_ptr: int | None = None, avg: torch.Tensor | None = None,
                        sel: torch.Tensor | None = None, masses: torch.Tensor | None = None):
        """RMSF.py:80-87 (frame) / 113-118 (average): centred f64 reference + info."""
        ref = self.empty(n_sel, 3)
        info = self.empty(RMSF_REFINFO_DOUBLES)
        call("rmsf_reference_setup", frame_ptr, _ptr(avg), n_sel, _ptr(sel if frame_ptr else None), _ptr(masses),
             ref.data_ptr(), info.data_ptr(), self.stream)
        return ref, info

    def reference_setup_mean(self, total: torch.Tensor, n_frames: float, n_sel: int,
                             masses: torch.Tensor | None = None):
        """RMSF.py:111 + 113-118: the average total / n_frames and the
        reference from it (one launch up to 1,024 selected atoms);
        bit-identical to ``divide`` + ``reference_setup(avg=...)``."""
        avg = self.empty(3 * n_sel)
        ref = self.empty(n_sel, 3)
        info = self.empty(RMSF_REFINFO_DOUBLES)
        call("rmsf_reference_setup_mean", total.data_ptr(), float(n_frames), n_sel, _ptr(masses), avg.data_ptr(),
             ref.data_ptr(), info.data_ptr(), self.stream)
        return avg, ref, info

    def workspace_bytes(self, n_sel: int, n_frames: int) -> int:
        return int(self.lib.rmsf_superpose_workspace_bytes(n_sel, n_frames))

    def superpose(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, masses, ref, refinfo,
                  xform: torch.Tensor, work: torch.Tensor, pstride: int = 0, dense_out: int | None = None,
                  dense_stride: int = 0) -> None:
        """RMSF.py:94-97,127-131 + get_rotation_matrix (RMSF.py:43-51): per-frame COM + QCP.
        ``pstride`` > 0: frames stored as coordinate planes (rmsf_superpose_planes).
        ``dense_out`` (a gathered ``sel``): also write the selected rows to
        that device address, frame f's [n_sel, 3] at f * ``dense_stride``
        floats (0 = 3 n_sel; rmsf_superpose_compact)."""
        if dense_out is not None:
            call("rmsf_superpose_compact", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(masses),
                 ref.data_ptr(), refinfo.data_ptr(), xform.data_ptr(), work.data_ptr(),
                 work.numel() * work.element_size(), dense_out, dense_stride, self.stream)
            return
        if pstride:
            call("rmsf_superpose_planes", xyz_ptr, fstride, pstride, n_frames, n_sel, _ptr(sel), _ptr(masses),
                 ref.data_ptr(), refinfo.data_ptr(), xform.data_ptr(), work.data_ptr(),
                 work.numel() * work.element_size(), self.stream)
            return
        call("rmsf_superpose", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(masses), ref.data_ptr(),
             refinfo.data_ptr(), xform.data_ptr(), work.data_ptr(), work.numel() * work.element_size(), self.stream)

    def splits(self, n_sel: int, n_frames: int, aligned: bool) -> int:
        return int(self.lib.rmsf_accumulate_splits(n_sel, n_frames, int(aligned)))

    def split_counts(self, n_frames: int, n_splits: int) -> list[int]:
        return [int(self.lib.rmsf_split_count(n_frames, n_splits, s)) for s in range(n_splits)]

    def accumulate(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, xform, refinfo, mode: int,
                   n_splits: int, out0: torch.Tensor, out1: torch.Tensor | None) -> None:
        """RMSF.py:99-103 (SUM) / 133-138 (WELFORD) over split frame tiles."""
        call("rmsf_accumulate", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(xform), _ptr(refinfo), mode,
             n_splits, out0.data_ptr(), _ptr(out1), self.stream)

    def balanced_workspace_bytes(self, n_sel: int, n_frames: int, n_groups: int = 0) -> int:
        return int(self.lib.rmsf_accumulate_balanced_workspace_bytes(n_sel, n_frames, n_groups))

    def accumulate_balanced(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, xform, refinfo,
                            mode: int, work: torch.Tensor, n_groups: int = 0, pstride: int = 0) -> None:
        """RMSF.py:99-103 (SUM) / 133-138 (WELFORD) on the balanced grid (one equal
        (lane chunk, frame) range per workgroup); partials go to ``work``.
        ``pstride`` > 0: aligned sweep over coordinate planes read in place."""
        if pstride:
            call("rmsf_accumulate_balanced_planes", xyz_ptr, fstride, pstride, n_frames, n_sel, _ptr(sel),
                 _ptr(xform), _ptr(refinfo), mode, n_groups, work.data_ptr(), work.numel() * work.element_size(),
                 self.stream)
            return
        call("rmsf_accumulate_balanced", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(xform), _ptr(refinfo),
             mode, n_groups, work.data_ptr(), work.numel() * work.element_size(), self.stream)

    def fold_balanced(self, work: torch.Tensor, n_coord: int, mode: int, acc_n: int, acc0: torch.Tensor,
                      acc1: torch.Tensor | None) -> None:
        """Fold the balanced partials in frame order into the running result
        (Chan's merge, RMSF.py:36-41, or a sum)."""
        call("rmsf_fold_balanced", work.data_ptr(), n_coord, mode, acc_n, acc0.data_ptr(), _ptr(acc1), self.stream)

    def fold_balanced_finalize(self, work: torch.Tensor, n_coord: int, acc_n: int, acc0: torch.Tensor,
                               acc1: torch.Tensor, n_total: int, rmsf: torch.Tensor) -> None:
        """fold_balanced (WELFORD) + finalize (RMSF.py:146) in one launch, for
        an atom plan (aligned sweeps, gathered selections, planes)."""
        call("rmsf_fold_balanced_finalize", work.data_ptr(), n_coord, acc_n, acc0.data_ptr(), acc1.data_ptr(),
             n_total, rmsf.data_ptr(), self.stream)

    def fold_balanced_shift(self, work: torch.Tensor, n_coord: int, acc_n: int, acc0: torch.Tensor,
                            acc1: torch.Tensor, shift: torch.Tensor, off3, out: torch.Tensor) -> None:
        """fold_balanced (WELFORD) + chan_shift_pack in one launch: ``out`` =
        the moments about c = shift + off3 that the cross-rank merge sums."""
        if out.numel() < 2 * n_coord or shift.numel() < n_coord:
            raise ValueError("fold_balanced_shift: buffer sizes")
        call("rmsf_fold_balanced_shift", work.data_ptr(), n_coord, acc_n, acc0.data_ptr(), acc1.data_ptr(),
             shift.data_ptr(), int(shift.dtype == torch.float32), _ptr(off3), out.data_ptr(), self.stream)

    def fold_balanced_shift_sliced(self, work: torch.Tensor, n_coord: int, acc_n: int, acc0: torch.Tensor,
                                   acc1: torch.Tensor, shift: torch.Tensor, off3, slice_coords: int,
                                   out: torch.Tensor) -> None:
        """fold_balanced_shift writing the reduce-scatter merge's atom-sliced
        layout: slice r (slice_coords coordinates) as [T1 | T2] at
        out[2 r slice_coords:]."""
        n_slices = -(-n_coord // slice_coords)
        if out.numel() < 2 * slice_coords * n_slices or shift.numel() < n_coord:
            raise ValueError("fold_balanced_shift_sliced: buffer sizes")
        call("rmsf_fold_balanced_shift_sliced", work.data_ptr(), n_coord, acc_n, acc0.data_ptr(), acc1.data_ptr(),
             shift.data_ptr(), int(shift.dtype == torch.float32), _ptr(off3), slice_coords, out.data_ptr(),
             self.stream)

    def balanced_slab_chunks(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int) -> int:
        """Chunks (1024 coordinates each) of the flat balanced plan when it is
        chunk-aligned (atom slabs possible), else 0."""
        c = ctypes.c_int64(0)
        call("rmsf_balanced_slab_chunks", xyz_ptr, fstride, n_frames, n_sel, ctypes.cast(ctypes.pointer(c),
                                                                                        ctypes.c_void_p))
        return int(c.value)

    def accumulate_balanced_slab(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, c0: int, c1: int,
                                 work: torch.Tensor) -> None:
        """The whole flat plan's ranges of chunks [c0, c1) (WELFORD)."""
        call("rmsf_accumulate_balanced_slab", xyz_ptr, fstride, n_frames, n_sel, c0, c1, work.data_ptr(),
             work.numel() * work.element_size(), self.stream)

    def fold_balanced_shift_slab(self, work: torch.Tensor, n_coord: int, acc_n: int, acc0: torch.Tensor,
                                 acc1: torch.Tensor, shift: torch.Tensor, off3, out: torch.Tensor, c0: int,
                                 c1: int) -> None:
        """Fold chunks [c0, c1) and write their [T1 | T2] to ``out``."""
        j0, j1 = 1024 * c0, min(1024 * c1, n_coord)
        if out.numel() < 2 * (j1 - j0) or shift.numel() < n_coord:
            raise ValueError("fold_balanced_shift_slab: buffer sizes")
        call("rmsf_fold_balanced_shift_slab", work.data_ptr(), n_coord, acc_n, acc0.data_ptr(), acc1.data_ptr(),
             shift.data_ptr(), int(shift.dtype == torch.float32), _ptr(off3), out.data_ptr(), c0, c1, self.stream)

    def chan_merge(self, mean_parts: torch.Tensor, m2_parts: torch.Tensor, counts, n_coord: int,
                   mean_out: torch.Tensor, m2_out: torch.Tensor) -> None:
        """second_order_moments (RMSF.py:36-41) folded over the partials in order."""
        c = _lib.i64p(counts)
        call("rmsf_chan_merge", mean_parts.data_ptr(), m2_parts.data_ptr(), ctypes.cast(c, ctypes.c_void_p),
             len(counts), n_coord, mean_out.data_ptr(), m2_out.data_ptr(), self.stream)

    def chan_reduce(self, mean_parts: torch.Tensor, m2_parts: torch.Tensor, counts, n_coord: int,
                    mean_out: torch.Tensor, m2_out: torch.Tensor, order="mpi4py") -> None:
        """RMSF.py:143's comm.reduce of the partials (rank order in the rows)
        with second_order_moments in ``order`` ("mpi4py": mpi4py's default
        binomial tree; "rank": rank order).  The parts are overwritten (the
        schedule's working storage)."""
        c = _lib.i64p(counts)
        call("rmsf_chan_reduce", mean_parts.data_ptr(), m2_parts.data_ptr(), ctypes.cast(c, ctypes.c_void_p),
             len(counts), n_coord, _lib.merge_order(order), mean_out.data_ptr(), m2_out.data_ptr(), self.stream)

    def chan_merge_pair(self, mean1: torch.Tensor, m21: torch.Tensor, n1: int, mean2: torch.Tensor,
                        m22: torch.Tensor, n2: int) -> None:
        """(mean1, m21) = second_order_moments((n1, mean1, m21), (n2, mean2, m22)) in place."""
        n = mean1.numel()
        if m21.numel() != n or mean2.numel() != n or m22.numel() != n:
            raise ValueError("chan_merge_pair: buffer sizes")
        call("rmsf_chan_merge_pair", mean1.data_ptr(), m21.data_ptr(), int(n1), mean2.data_ptr(), m22.data_ptr(),
             int(n2), n, self.stream)

    def sum_splits(self, parts: torch.Tensor, n_parts: int, n: int, out: torch.Tensor) -> None:
        call("rmsf_sum_splits", parts.data_ptr(), n_parts, n, out.data_ptr(), self.stream)

    def divide(self, x: torch.Tensor, divisor: float, out: torch.Tensor) -> None:
        call("rmsf_divide", x.data_ptr(), float(divisor), x.numel(), out.data_ptr(), self.stream)

    def chan_weight(self, mean_k: torch.Tensor, w: float, out: torch.Tensor) -> None:
        call("rmsf_chan_weight", mean_k.data_ptr(), float(w), mean_k.numel(), out.data_ptr(), self.stream)

    def chan_deviation(self, mean_k, m2_k, mean, n_k: float, out) -> None:
        call("rmsf_chan_deviation", mean_k.data_ptr(), m2_k.data_ptr(), mean.data_ptr(), float(n_k), mean_k.numel(),
             out.data_ptr(), self.stream)

    def chan_shift_pack(self, mean_k, m2_k, shift, off3, n_k: float, out) -> None:
        """out[0:n] = n_k (mean_k - c), out[n:2n] = M2_k + n_k (mean_k - c)^2,
        c = shift + off3 (per xyz); shift f64 or f32."""
        n = mean_k.numel()
        if out.numel() < 2 * n or shift.numel() < n:
            raise ValueError("chan_shift_pack: buffer sizes")
        call("rmsf_chan_shift_pack", mean_k.data_ptr(), m2_k.data_ptr(), shift.data_ptr(),
             int(shift.dtype == torch.float32), _ptr(off3), float(n_k), n, out.data_ptr(), self.stream)

    def chan_shift_finish(self, t, shift, off3, n_sel: int, n_frames: int, mean, m2, rmsf) -> None:
        if t.numel() < 6 * n_sel or shift.numel() < 3 * n_sel or mean.numel() < 3 * n_sel or m2.numel() < 3 * n_sel:
            raise ValueError("chan_shift_finish: buffer sizes")
        call("rmsf_chan_shift_finish", t.data_ptr(), shift.data_ptr(), int(shift.dtype == torch.float32), _ptr(off3),
             n_sel, n_frames, mean.data_ptr(), m2.data_ptr(), _ptr(rmsf), self.stream)

    def chan_shift_pack_sliced(self, mean_k, m2_k, shift, off3, n_k: float, slice_coords: int, out) -> None:
        """chan_shift_pack into the atom-sliced layout (see
        fold_balanced_shift_sliced)."""
        n = mean_k.numel()
        if out.numel() < 2 * slice_coords * -(-n // slice_coords) or shift.numel() < n:
            raise ValueError("chan_shift_pack_sliced: buffer sizes")
        call("rmsf_chan_shift_pack_sliced", mean_k.data_ptr(), m2_k.data_ptr(), shift.data_ptr(),
             int(shift.dtype == torch.float32), _ptr(off3), float(n_k), n, slice_coords, out.data_ptr(), self.stream)

    def chan_shift_finish_slice(self, t, slice_coords: int, shift, off3, n_sel: int, n_frames: int, mean, m2,
                                rmsf) -> None:
        """Unpack one reduced slice [T1 | T2] (width slice_coords) for its
        n_sel atoms; shift / mean / m2 / rmsf start at the slice's first atom."""
        if (t.numel() < 2 * slice_coords or 3 * n_sel > slice_coords or shift.numel() < 3 * n_sel
                or mean.numel() < 3 * n_sel or m2.numel() < 3 * n_sel):
            raise ValueError("chan_shift_finish_slice: buffer sizes")
        call("rmsf_chan_shift_finish_slice", t.data_ptr(), slice_coords, shift.data_ptr(),
             int(shift.dtype == torch.float32), _ptr(off3), n_sel, n_frames, mean.data_ptr(), m2.data_ptr(),
             _ptr(rmsf), self.stream)

    def zero_index(self) -> torch.Tensor:
        """A resident int64 [0] (row index for gathering one frame); made once."""
        if getattr(self, "_zero_idx", None) is None:
            self._zero_idx = torch.zeros(1, dtype=torch.int64, device=self.device)
        return self._zero_idx

    def gather_frames(self, base_ptr: int, fstride: int, rows: torch.Tensor, n: int, n_sel: int, sel,
                      out: torch.Tensor) -> None:
        """out[i] = frame base + rows[i]*fstride, selected (rmsf_gather_frames)."""
        if out.dtype != F32 or out.numel() < 3 * n_sel * n or rows.numel() < n:
            raise ValueError("gather_frames: buffer sizes")
        call("rmsf_gather_frames", base_ptr, fstride, rows.data_ptr(), n, n_sel, _ptr(sel), out.data_ptr(),
             self.stream)

    def planes_to_rows(self, x: torch.Tensor, n: int) -> torch.Tensor:
        """f64 [3n] in plane order (x[n], y[n], z[n]) -> a new [3n] in (atom, xyz) order."""
        out = self.empty(3 * n)
        call("rmsf_planes_to_rows", x.data_ptr(), n, out.data_ptr(), self.stream)
        return out

    def welford_sequential(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, k0: int,
                           mean: torch.Tensor, sumsquares: torch.Tensor,
                           work: torch.Tensor | None = None) -> torch.Tensor:
        """RMSF.py:137-138 as written, frame by frame from k = k0 (k0 = 0:
        the state starts at np.zeros): the reference recurrence's own
        (mean, sumsquares), bit for bit.  Unaligned rows; ``sel`` an int32
        device index tensor or None.  Returns the coefficient workspace
        (pass it back to reuse it)."""
        need = int(self.lib.rmsf_welford_sequential_workspace_bytes(n_frames))
        if work is None or work.numel() * work.element_size() < need:
            work = self.empty(max(need, 16) // 8)
        call("rmsf_welford_sequential", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), k0, mean.data_ptr(),
             sumsquares.data_ptr(), work.data_ptr(), work.numel() * work.element_size(), self.stream)
        return work

    # -- exact=True on the aligned path (the reference's summation orders) ---
    def reference_setup_seq(self, n_sel: int, mass_total: float, *, frame_ptr: int | None = None,
                            sel: torch.Tensor | None = None, total: torch.Tensor | None = None,
                            n_frames: float = 1.0, masses: torch.Tensor | None = None, after_centre=None):
        """RMSF.py:84-85 (``frame_ptr``) or RMSF.py:111 + 117-118 (``total``,
        the all-reduced sweep-1 sums, divided by ``n_frames`` as read) with
        the reference's own summation order (rmsf_reference_setup_sequential).
        ``after_centre``: called between the two halves (the centred
        reference, then the record's sums; rmsf_reference_centre_sequential /
        rmsf_reference_sums_sequential, same bits) -- e.g. to record an event
        an InnerProduct on another stream waits for.  Returns (average or
        None, ref, info)."""
        ref = self.empty(n_sel, 3)
        info = self.empty(RMSF_REFINFO_DOUBLES)
        avg = self.empty(3 * n_sel) if total is not None else None
        args = (frame_ptr, _ptr(total), float(n_frames), n_sel, _ptr(sel if frame_ptr else None), _ptr(masses),
                float(mass_total), _ptr(avg), ref.data_ptr(), info.data_ptr(), self.stream)
        if after_centre is None:
            call("rmsf_reference_setup_sequential", *args)
        else:
            call("rmsf_reference_centre_sequential", *args)
            after_centre()
            call("rmsf_reference_sums_sequential", n_sel, float(mass_total), ref.data_ptr(), info.data_ptr(),
                 self.stream)
        return avg, ref, info

    def superpose_seq(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, masses,
                      mass_total: float, ref: torch.Tensor, refinfo: torch.Tensor, xform: torch.Tensor) -> None:
        """RMSF.py:94-97,127-131 + get_rotation_matrix per frame in the
        reference's order (rmsf_superpose_sequential)."""
        call("rmsf_superpose_sequential", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(masses),
             float(mass_total), ref.data_ptr(), refinfo.data_ptr(), xform.data_ptr(), self.stream)

    def frame_com_seq(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, masses,
                      mass_total: float, xform: torch.Tensor) -> None:
        """The first half of superpose_seq: every frame's mobile COM into the
        records' [9..11] (rmsf_frame_com_sequential); no reference needed."""
        call("rmsf_frame_com_sequential", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(masses),
             float(mass_total), xform.data_ptr(), self.stream)

    def superpose_seq_from_com(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel,
                               ref: torch.Tensor, refinfo: torch.Tensor, xform: torch.Tensor) -> None:
        """The second half: InnerProduct + QCP from the COMs in the records
        (rmsf_superpose_sequential_from_com)."""
        call("rmsf_superpose_sequential_from_com", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), ref.data_ptr(),
             refinfo.data_ptr(), xform.data_ptr(), self.stream)

    def inner_product_seq(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, ref: torch.Tensor,
                          xform: torch.Tensor) -> None:
        """superpose_seq_from_com's first part: qcprot's InnerProduct per
        frame against the centred reference (rmsf_inner_product_sequential;
        the record's sums need not be ready)."""
        call("rmsf_inner_product_sequential", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), ref.data_ptr(),
             xform.data_ptr(), self.stream)

    def superpose_seq_qcp(self, n_frames: int, n_sel: int, refinfo: torch.Tensor, xform: torch.Tensor) -> None:
        """Its second part: E0 with the record's G2, and the QCP
        (rmsf_superpose_sequential_qcp)."""
        call("rmsf_superpose_sequential_qcp", n_frames, n_sel, refinfo.data_ptr(), xform.data_ptr(), self.stream)

    def accumulate_seq(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, xform, refinfo,
                       mode: int, k0: int, acc0: torch.Tensor, acc1: torch.Tensor | None,
                       work: torch.Tensor | None = None) -> torch.Tensor | None:
        """RMSF.py:99-103 (SUM) / 133-138 (WELFORD) frame by frame in order
        (rmsf_accumulate_sequential); returns the coefficient workspace."""
        if mode == RMSF_MODE_WELFORD:
            need = int(self.lib.rmsf_welford_sequential_workspace_bytes(n_frames))
            if work is None or work.numel() * work.element_size() < need:
                work = self.empty(max(need, 16) // 8)
        call("rmsf_accumulate_sequential", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(xform),
             _ptr(refinfo), mode, k0, acc0.data_ptr(), _ptr(acc1), _ptr(work),
             0 if work is None else work.numel() * work.element_size(), self.stream)
        return work

    def finalize(self, m2: torch.Tensor, n_sel: int, n_frames: int, out: torch.Tensor) -> None:
        """RMSF.py:146: sqrt(M2.sum(axis=1)/n)."""
        call("rmsf_finalize", m2.data_ptr(), n_sel, n_frames, out.data_ptr(), self.stream)

    # -- positional covariance (csrc/covariance.hip) --------------------------
    def covariance_workspace_bytes(self, n_sel: int, n_frames: int) -> int:
        return int(self.lib.rmsf_covariance_workspace_bytes(n_sel, n_frames))

    def covariance_accumulate(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, xform, refinfo,
                              shift: torch.Tensor, cov: torch.Tensor, t1: torch.Tensor,
                              work: torch.Tensor | None = None) -> None:
        """cov[i, j] += sum_f d_i d_j (blocks holding j >= i), t1[i] += sum_f d_i
        over the batch, d = f64(p) - shift with p the selected rows -- through
        the transform of RMSF.py:99-101 / 133-135 when ``xform`` and
        ``refinfo`` are given -- on the f64 matrix cores
        (rmsf_covariance_accumulate).  ``work``: f64 scratch of at least
        covariance_workspace_bytes(n_sel, n_frames) bytes (None when 0)."""
        n = 3 * n_sel
        if (cov.dtype != F64 or t1.dtype != F64 or shift.dtype != F64 or cov.dim() != 2 or cov.stride(1) != 1
                or cov.shape[0] < n or cov.shape[1] < n or t1.numel() < n or shift.numel() < n):
            raise ValueError("covariance_accumulate: buffer sizes")
        call("rmsf_covariance_accumulate", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(xform), _ptr(refinfo),
             shift.data_ptr(), cov.data_ptr(), cov.stride(0), t1.data_ptr(), _ptr(work),
             0 if work is None else work.numel() * work.element_size(), self.stream)

    def covariance_finish(self, cov: torch.Tensor, t1: torch.Tensor, n_coord: int, n_frames: int) -> None:
        """cov = cov - t1 t1^T / n_frames, the centred co-moment, mirrored
        from the upper triangle to the full symmetric matrix
        (rmsf_covariance_finish)."""
        if cov.dim() != 2 or cov.stride(1) != 1 or cov.shape[0] < n_coord or cov.shape[1] < n_coord \
                or t1.numel() < n_coord:
            raise ValueError("covariance_finish: buffer sizes")
        call("rmsf_covariance_finish", cov.data_ptr(), cov.stride(0), t1.data_ptr(), n_coord, n_frames, self.stream)

    # -- time-lagged co-moment (csrc/covariance.hip) ---------------------------
    def lagged_comoment_workspace_bytes(self, n_sel: int, n_pairs: int) -> int:
        return int(self.lib.rmsf_lagged_comoment_workspace_bytes(n_sel, n_pairs))

    def lagged_comoment_accumulate(self, xyz_a_ptr: int, fstride_a: int, xyz_b_ptr: int, fstride_b: int,
                                   n_pairs: int, n_sel: int, sel, xform_a, xform_b, refinfo, shift: torch.Tensor,
                                   s: torch.Tensor, work: torch.Tensor | None = None) -> None:
        """s[i, j] += sum_q d_i(frame q of A) d_j(frame q of B) over the
        batch's pairs, all of the matrix, d = f64(p) - shift as in
        ``covariance_accumulate`` -- each operand through its own transform
        records when ``xform_a``, ``xform_b`` and ``refinfo`` are given -- on
        the f64 matrix cores (rmsf_lagged_comoment_accumulate).  The caller
        offsets B by the lag.  ``work``: f64 scratch of at least
        lagged_comoment_workspace_bytes(n_sel, n_pairs) bytes (None when 0)."""
        n = 3 * n_sel
        if (s.dtype != F64 or shift.dtype != F64 or s.dim() != 2 or s.stride(1) != 1 or s.shape[0] < n
                or s.shape[1] < n or shift.numel() < n):
            raise ValueError("lagged_comoment_accumulate: buffer sizes")
        call("rmsf_lagged_comoment_accumulate", xyz_a_ptr, fstride_a, xyz_b_ptr, fstride_b, n_pairs, n_sel, _ptr(sel),
             _ptr(xform_a), _ptr(xform_b), _ptr(refinfo), shift.data_ptr(), s.data_ptr(), s.stride(0), _ptr(work),
             0 if work is None else work.numel() * work.element_size(), self.stream)

    def lagged_comoment_finish(self, s: torch.Tensor, t: torch.Tensor, n_coord: int, m: int) -> None:
        """s = s + s^T - t t^T / m in place, symmetric in its bits
        (rmsf_lagged_comoment_finish)."""
        if (s.dtype != F64 or t.dtype != F64 or s.dim() != 2 or s.stride(1) != 1 or s.shape[0] < n_coord
                or s.shape[1] < n_coord or t.numel() < n_coord):
            raise ValueError("lagged_comoment_finish: buffer sizes")
        call("rmsf_lagged_comoment_finish", s.data_ptr(), s.stride(0), t.data_ptr(), n_coord, m, self.stream)

    # -- PCA projection (csrc/pca_project.hip) ---------------------------------
    def pca_project_workspace_bytes(self, n_frames: int, n_sel: int, n_comp: int) -> int:
        return int(self.lib.rmsf_pca_project_workspace_bytes(n_frames, n_sel, n_comp))

    def pca_project(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, xform, refinfo,
                    mean: torch.Tensor, comp: torch.Tensor, n_comp: int, out: torch.Tensor,
                    work: torch.Tensor | None = None) -> None:
        """out[f, c] = sum_i d_i comp[i, c] for c < ``n_comp`` over the batch,
        d = f64(p) - mean with p the selected rows -- through the transform of
        RMSF.py:99-101 / 133-135 when ``xform`` and ``refinfo`` are given --
        on the f64 matrix cores (rmsf_pca_project).  ``comp``: f64 [3 n_sel,
        >= n_comp], ``out``: f64 [>= n_frames, >= n_comp], rows of either may
        be wider (their other columns are not touched).  ``work``: f64 scratch
        of at least pca_project_workspace_bytes(n_frames, n_sel, n_comp)
        bytes (None when 0)."""
        n = 3 * n_sel
        if (mean.dtype != F64 or comp.dtype != F64 or out.dtype != F64 or comp.dim() != 2 or out.dim() != 2
                or comp.stride(1) != 1 or out.stride(1) != 1 or mean.numel() < n or not mean.is_contiguous()
                or comp.shape[0] < n or comp.shape[1] < n_comp or out.shape[0] < n_frames
                or out.shape[1] < n_comp):
            raise ValueError("pca_project: buffer sizes")
        call("rmsf_pca_project", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(xform), _ptr(refinfo),
             mean.data_ptr(), comp.data_ptr(), comp.stride(0), n_comp, out.data_ptr(), out.stride(0), _ptr(work),
             0 if work is None else work.numel() * work.element_size(), self.stream)

    # -- PCA back-projection (csrc/pca_backproject.hip) --------------------------
    def pca_backproject_workspace_bytes(self, n_frames: int, n_sel: int, n_cols: int) -> int:
        return int(self.lib.rmsf_pca_backproject_workspace_bytes(n_frames, n_sel, n_cols))

    def pca_backproject(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, xform, refinfo,
                        mean: torch.Tensor, p: torch.Tensor, n_cols: int, y: torch.Tensor, accumulate: bool = False,
                        work: torch.Tensor | None = None) -> None:
        """y[i, c] (+)= sum_f d_i(f) p[f, c] for c < ``n_cols`` <= 48 over the
        batch, the adjoint of ``pca_project`` with the same d = f64(p) - mean
        (rmsf_pca_backproject).  ``p``: f64 [>= n_frames, >= n_cols], ``y``:
        f64 [>= 3 n_sel, >= n_cols], rows of either may be wider (their other
        columns are not touched).  ``accumulate``: add to ``y`` (a later batch
        of a streamed trajectory) instead of overwriting it.  ``work``: f64
        scratch of at least pca_backproject_workspace_bytes(n_frames, n_sel,
        n_cols) bytes (None when 0)."""
        n = 3 * n_sel
        if (mean.dtype != F64 or p.dtype != F64 or y.dtype != F64 or p.dim() != 2 or y.dim() != 2
                or p.stride(1) != 1 or y.stride(1) != 1 or mean.numel() < n or not mean.is_contiguous()
                or p.shape[0] < n_frames or p.shape[1] < n_cols or y.shape[0] < n or y.shape[1] < n_cols):
            raise ValueError("pca_backproject: buffer sizes")
        call("rmsf_pca_backproject", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(xform), _ptr(refinfo),
             mean.data_ptr(), p.data_ptr(), p.stride(0), n_cols, y.data_ptr(), y.stride(0), int(bool(accumulate)),
             _ptr(work), 0 if work is None else work.numel() * work.element_size(), self.stream)

    # -- block products of the device eigen-solver (csrc/eigen_block.hip) -------
    @staticmethod
    def _is_block(t: torch.Tensor, rows: int, cols: int) -> bool:
        return (t.dtype == F64 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= rows and t.shape[1] >= cols
                and (t.shape[0] == 1 or t.stride(0) >= t.shape[1]))

    def symm_block_workspace_bytes(self, n: int, n_cols: int) -> int:
        return int(self.lib.rmsf_symm_block_workspace_bytes(n, n_cols))

    def symm_block(self, m: torch.Tensor, n: int, q: torch.Tensor, n_cols: int, y: torch.Tensor,
                   work: torch.Tensor | None = None) -> None:
        """y[:n, :n_cols] = m[:n, :n] @ q[:n, :n_cols] on the f64 matrix cores
        (rmsf_symm_block).  ``m`` must be symmetric in its bits (what
        covariance_finish writes).  Rows of any of the three may be wider;
        the other columns are neither read nor written.  ``work``: f64
        scratch of at least symm_block_workspace_bytes(n, n_cols) bytes
        (None when 0)."""
        if not (self._is_block(m, n, n) and self._is_block(q, n, n_cols) and self._is_block(y, n, n_cols)):
            raise ValueError("symm_block: buffer sizes")
        call("rmsf_symm_block", m.data_ptr(), m.stride(0), n, q.data_ptr(), q.stride(0), n_cols, y.data_ptr(),
             y.stride(0), _ptr(work), 0 if work is None else work.numel() * work.element_size(), self.stream)

    def block_gram_workspace_bytes(self, n: int, na: int, nb: int) -> int:
        return int(self.lib.rmsf_block_gram_workspace_bytes(n, na, nb))

    def block_gram(self, a: torch.Tensor, na: int, b: torch.Tensor, nb: int, n: int, g: torch.Tensor,
                   work: torch.Tensor | None = None) -> None:
        """g[:na, :nb] = a[:n, :na].T @ b[:n, :nb] (rmsf_block_gram).
        ``work``: f64 scratch of at least block_gram_workspace_bytes(n, na,
        nb) bytes (None when 0)."""
        if not (self._is_block(a, n, na) and self._is_block(b, n, nb) and self._is_block(g, na, nb)):
            raise ValueError("block_gram: buffer sizes")
        call("rmsf_block_gram", a.data_ptr(), a.stride(0), na, b.data_ptr(), b.stride(0), nb, n, g.data_ptr(),
             g.stride(0), _ptr(work), 0 if work is None else work.numel() * work.element_size(), self.stream)

    def block_update(self, alpha: float, a: torch.Tensor | None, b: torch.Tensor, nb: int, t: torch.Tensor, n: int,
                     nc: int, c: torch.Tensor) -> None:
        """c[:n, :nc] = alpha * a[:n, :nc] + b[:n, :nb] @ t[:nb, :nc], or
        b @ t alone when ``a`` is None (rmsf_block_update).  ``c`` may be
        ``a``; it must not be ``b``."""
        if not (self._is_block(b, n, nb) and self._is_block(t, nb, nc) and self._is_block(c, n, nc)
                and (a is None or self._is_block(a, n, nc))):
            raise ValueError("block_update: buffer sizes")
        call("rmsf_block_update", float(alpha), _ptr(a), 0 if a is None else a.stride(0), b.data_ptr(), b.stride(0),
             nb, t.data_ptr(), t.stride(0), n, nc, c.data_ptr(), c.stride(0), self.stream)

    # -- diffusion kernel of a distance matrix (csrc/diffusion.hip) -------------
    def diffusion_kernel(self, m: torch.Tensor, epsilon: float, n: int | None = None) -> torch.Tensor:
        """``m[:n, :n]`` (f64 distances in HBM) becomes ``exp(-(m * m) /
        epsilon)`` in place; returns the f64 [n] sums of its rows
        (rmsf_diffusion_kernel).  Columns past ``n`` are neither read nor
        written."""
        n = m.shape[0] if n is None else n
        if m.dtype != F64 or m.dim() != 2 or m.stride(1) != 1 or m.shape[0] < n or m.shape[1] < n or n < 1:
            raise ValueError("diffusion_kernel: buffer sizes")
        rowsum = self.empty(n)
        call("rmsf_diffusion_kernel", m.data_ptr(), m.stride(0), n, float(epsilon), rowsum.data_ptr(), self.stream)
        return rowsum

    def block_scale_rows(self, s: torch.Tensor, a: torch.Tensor, n: int, nc: int, c: torch.Tensor) -> None:
        """c[:n, :nc] = s[:n, None] * a[:n, :nc] (rmsf_block_scale_rows).
        ``c`` may be ``a``."""
        if not (self._is_block(a, n, nc) and self._is_block(c, n, nc) and s.dtype == F64 and s.numel() >= n
                and s.is_contiguous()):
            raise ValueError("block_scale_rows: buffer sizes")
        call("rmsf_block_scale_rows", s.data_ptr(), a.data_ptr(), a.stride(0), n, nc, c.data_ptr(), c.stride(0),
             self.stream)

    # -- all-pairs RMSD matrix (csrc/pairwise.hip) ----------------------------
    def pairwise_centres(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, weights,
                         per_frame: bool = True):
        """Every frame's weighted centre [n_frames, 3] and G_f = sum_a w_a
        |x_f,a - c_f|^2 [n_frames] (rmsf_pairwise_centres).  ``per_frame``
        False: frame 0's centre for every frame (the metric without
        superposition; a common shift)."""
        centre, g = self.empty(n_frames, 3), self.empty(n_frames)
        call("rmsf_pairwise_centres", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(weights), int(per_frame),
             centre.data_ptr(), g.data_ptr(), self.stream)
        return centre, g

    def pairwise_workspace_bytes(self, n_frames: int, n_sel: int) -> int:
        return int(self.lib.rmsf_pairwise_workspace_bytes(n_frames, n_sel))

    def pairwise_rmsd(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, weights, w_total: float,
                      centre: torch.Tensor, g: torch.Tensor, out: torch.Tensor, superpose: bool = True,
                      cutoff: float = 0.0, work: torch.Tensor | None = None) -> None:
        """out[i, j] = out[j, i] = the RMSD of frames i and j (minimal over
        rotations when ``superpose``), 0 where <= ``cutoff`` and on the
        diagonal, on the f64 matrix cores (rmsf_pairwise_rmsd).  ``centre``,
        ``g``: pairwise_centres' (per_frame = superpose).  ``work``: f64 scratch
        of at least pairwise_workspace_bytes(n_frames, n_sel) bytes (None when 0)."""
        if (out.dtype != F64 or centre.dtype != F64 or g.dtype != F64 or out.dim() != 2 or out.stride(1) != 1
                or out.shape[0] < n_frames or out.shape[1] < n_frames or centre.numel() < 3 * n_frames
                or g.numel() < n_frames or not centre.is_contiguous()):
            raise ValueError("pairwise_rmsd: buffer sizes")
        call("rmsf_pairwise_rmsd", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(weights), float(w_total),
             centre.data_ptr(), g.data_ptr(), int(bool(superpose)), float(cutoff), out.data_ptr(), out.stride(0),
             _ptr(work), 0 if work is None else work.numel() * work.element_size(), self.stream)

    # -- cross RMSD matrix: frames of A against frames of B (csrc/pairwise.hip) --
    def pairwise_centres_about(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, weights,
                               about: torch.Tensor):
        """pairwise_centres(per_frame=False) about a centre found elsewhere:
        ``about`` (f64, its first three entries) for every frame, and G about
        it (rmsf_pairwise_centres_about) -- the common shift of the second side
        of a cross matrix without superposition."""
        if about.dtype != F64 or about.numel() < 3 or not about.is_contiguous():
            raise ValueError("pairwise_centres_about: buffer sizes")
        centre, g = self.empty(n_frames, 3), self.empty(n_frames)
        call("rmsf_pairwise_centres_about", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(weights),
             about.data_ptr(), centre.data_ptr(), g.data_ptr(), self.stream)
        return centre, g

    def cross_workspace_bytes(self, n_a: int, n_b: int, n_sel: int) -> int:
        return int(self.lib.rmsf_cross_workspace_bytes(n_a, n_b, n_sel))

    def cross_rmsd(self, a_ptr: int, stride_a: int, n_a: int, sel_a, centre_a: torch.Tensor, g_a: torch.Tensor,
                   b_ptr: int, stride_b: int, n_b: int, sel_b, centre_b: torch.Tensor, g_b: torch.Tensor,
                   n_sel: int, weights, w_total: float, out: torch.Tensor, superpose: bool = True,
                   cutoff: float = 0.0, work: torch.Tensor | None = None) -> None:
        """out[i, j] = the RMSD of frame i of A and frame j of B (minimal over
        rotations when ``superpose``), 0 where <= ``cutoff``, on the f64 matrix
        cores (rmsf_cross_rmsd).  ``centre_*``, ``g_*``: pairwise_centres' of
        each side (superposed), or pairwise_centres(per_frame=False) of A and
        pairwise_centres_about(A's centre) of B (plain).  ``work``: f64 scratch
        of at least cross_workspace_bytes(n_a, n_b, n_sel) bytes (None when 0)."""
        sides = ((centre_a, g_a, n_a), (centre_b, g_b, n_b))
        if (out.dtype != F64 or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < n_a or out.shape[1] < n_b
                or any(c.dtype != F64 or g.dtype != F64 or c.numel() < 3 * n or g.numel() < n
                       or not c.is_contiguous() for c, g, n in sides)):
            raise ValueError("cross_rmsd: buffer sizes")
        call("rmsf_cross_rmsd", a_ptr, stride_a, n_a, _ptr(sel_a), centre_a.data_ptr(), g_a.data_ptr(),
             b_ptr, stride_b, n_b, _ptr(sel_b), centre_b.data_ptr(), g_b.data_ptr(), n_sel, _ptr(weights),
             float(w_total), int(bool(superpose)), float(cutoff), out.data_ptr(), out.stride(0),
             _ptr(work), 0 if work is None else work.numel() * work.element_size(), self.stream)

    def row_argmin(self, m: torch.Tensor, n_rows: int | None = None, n_cols: int | None = None):
        """(int64 [n_rows], f64 [n_rows]): of every row of ``m[:n_rows,
        :n_cols]`` the lowest column holding its least entry, and that entry
        (rmsf_row_argmin; numpy.argmin's tie rule, which torch.min does not
        promise)."""
        n_rows = m.shape[0] if n_rows is None else n_rows
        n_cols = m.shape[1] if n_cols is None else n_cols
        if (m.dtype != F64 or m.dim() != 2 or m.stride(1) != 1 or m.shape[0] < n_rows or m.shape[1] < n_cols
                or n_cols < 1):
            raise ValueError("row_argmin: buffer sizes")
        idx = torch.empty(n_rows, dtype=torch.int64, device=self.device)
        val = self.empty(n_rows)
        call("rmsf_row_argmin", m.data_ptr(), n_rows, n_cols, m.stride(0), idx.data_ptr(), val.data_ptr(),
             self.stream)
        return idx, val

    # -- GROMOS clustering of a distance matrix (csrc/clustering.hip) ------------
    def adjacency_words(self, n: int) -> int:
        return int(self.lib.rmsf_adjacency_words(n))

    def adjacency_pack(self, m: torch.Tensor, cutoff: float, n: int | None = None, ldw: int | None = None):
        """(uint64 words as int64 [n, ldw], int32 [n]): the neighbour bits
        ``adj(i, j) = (m[i, j] <= cutoff)``, diagonal set, NaN never a
        neighbour, bit j & 63 of word j // 64, and their row counts
        (rmsf_adjacency_pack).  ``m``: f64 [>= n, >= n] in HBM, read once."""
        n = m.shape[0] if n is None else n
        if m.dtype != F64 or m.dim() != 2 or m.stride(1) != 1 or m.shape[0] < n or m.shape[1] < n or n < 1:
            raise ValueError("adjacency_pack: buffer sizes")
        ldw = self.adjacency_words(n) if ldw is None else ldw
        adj = torch.empty((n, ldw), dtype=torch.int64, device=self.device)
        count = torch.empty(n, dtype=torch.int32, device=self.device)
        call("rmsf_adjacency_pack", m.data_ptr(), n, m.stride(0), float(cutoff), adj.data_ptr(), adj.stride(0),
             count.data_ptr(), self.stream)
        return adj, count

    def _is_adjacency(self, adj: torch.Tensor, n: int) -> bool:
        return (adj.dtype == torch.int64 and adj.dim() == 2 and adj.stride(1) == 1 and adj.shape[0] >= n >= 1
                and adj.shape[1] >= self.adjacency_words(n))

    def pairwise_adjacency(self, xyz_ptr: int, fstride: int, n_frames: int, n_sel: int, sel, weights,
                           w_total: float, centre: torch.Tensor, g: torch.Tensor, adj: torch.Tensor,
                           count: torch.Tensor | None, cutoff: float, superpose: bool = True,
                           zero_cutoff: float = 0.0, work: torch.Tensor | None = None) -> None:
        """adj[:n_frames] (uint64 words as int64 [>= n_frames, ldw]) = the
        neighbour bits that pairwise_rmsd(cutoff=zero_cutoff) followed by
        adjacency_pack(cutoff) would give, word for word, and ``count`` (int32
        [>= n_frames], or None) their row counts, without the f64 matrix
        (rmsf_pairwise_adjacency).  ``centre``, ``g``, ``work``: as
        pairwise_rmsd's."""
        if (centre.dtype != F64 or g.dtype != F64 or centre.numel() < 3 * n_frames or g.numel() < n_frames
                or not centre.is_contiguous() or not self._is_adjacency(adj, n_frames)
                or (count is not None and (count.dtype != torch.int32 or count.numel() < n_frames
                                           or not count.is_contiguous()))):
            raise ValueError("pairwise_adjacency: buffer sizes")
        call("rmsf_pairwise_adjacency", xyz_ptr, fstride, n_frames, n_sel, _ptr(sel), _ptr(weights), float(w_total),
             centre.data_ptr(), g.data_ptr(), int(bool(superpose)), float(zero_cutoff), float(cutoff),
             adj.data_ptr(), adj.stride(0), _ptr(count),
             _ptr(work), 0 if work is None else work.numel() * work.element_size(), self.stream)

    def adjacency_count(self, adj: torch.Tensor, n: int | None = None) -> torch.Tensor:
        """int32 [n]: the set bits of every row of ``adj[:n]``'s
        adjacency_words(n) words (rmsf_adjacency_count)."""
        n = adj.shape[0] if n is None else n
        if not self._is_adjacency(adj, n):
            raise ValueError("adjacency_count: buffer sizes")
        count = torch.empty(n, dtype=torch.int32, device=self.device)
        call("rmsf_adjacency_count", adj.data_ptr(), n, adj.stride(0), count.data_ptr(), self.stream)
        return count

    def cluster_gromos(self, adj: torch.Tensor, count: torch.Tensor):
        """(labels int32 [n], centres int32 [k], sizes int32 [k]) in HBM: the
        GROMOS loop on adjacency_pack's bits and counts (rmsf_cluster_gromos;
        ``count`` is left as it is).  Returns after the loop's last read of
        its state: the stream is idle."""
        n = adj.shape[0]
        if (adj.dtype != torch.int64 or adj.dim() != 2 or adj.stride(1) != 1 or count.dtype != torch.int32
                or count.numel() < n or not count.is_contiguous() or adj.shape[1] < self.adjacency_words(n) or n < 1):
            raise ValueError("cluster_gromos: buffer sizes")
        label, centre, size = (torch.empty(n, dtype=torch.int32, device=self.device) for _ in range(3))
        need = int(self.lib.rmsf_cluster_gromos_workspace_bytes(n))
        work = torch.empty(need // 8, dtype=torch.int64, device=self.device)
        k = ctypes.c_int32(0)
        call("rmsf_cluster_gromos", adj.data_ptr(), n, adj.stride(0), count.data_ptr(), label.data_ptr(),
             centre.data_ptr(), size.data_ptr(), ctypes.byref(k), work.data_ptr(), need, self.stream)
        return label, centre[:k.value], size[:k.value]

    def cluster_dbscan(self, adj: torch.Tensor, count: torch.Tensor, min_samples: int):
        """(labels int32 [n], core bits as int64 [adjacency_words(n)],
        n_clusters, n_rounds): DBSCAN on adjacency_pack's bits and counts
        (rmsf_cluster_dbscan, csrc/dbscan.hip; ``adj`` and ``count`` are left
        as they are).  -1 is noise.  Returns after the last read of its state:
        the stream is idle."""
        n = adj.shape[0]
        if (adj.dtype != torch.int64 or adj.dim() != 2 or adj.stride(1) != 1 or count.dtype != torch.int32
                or count.numel() < n or not count.is_contiguous() or adj.shape[1] < self.adjacency_words(n) or n < 1):
            raise ValueError("cluster_dbscan: buffer sizes")
        if int(min_samples) != min_samples or min_samples < 1:
            raise ValueError(f"cluster_dbscan: min_samples must be an integer >= 1, got {min_samples!r}")
        label = torch.empty(n, dtype=torch.int32, device=self.device)
        core = torch.empty(self.adjacency_words(n), dtype=torch.int64, device=self.device)
        need = int(self.lib.rmsf_cluster_dbscan_workspace_bytes(n))
        work = torch.empty(need // 8, dtype=torch.int64, device=self.device)
        k, rounds = ctypes.c_int32(0), ctypes.c_int32(0)
        call("rmsf_cluster_dbscan", adj.data_ptr(), n, adj.stride(0), count.data_ptr(),
             min(int(min_samples), 2 ** 62), label.data_ptr(), core.data_ptr(), ctypes.byref(k), ctypes.byref(rounds),
             work.data_ptr(), need, self.stream)
        return label, core, k.value, rounds.value

    def contact_counts_plan(self, n_a: int, n_b: int, n_frames: int, symmetric: bool = False):
        """(tile_a, tile_b, frame_chunk, n_splits) of rmsf_contact_counts for
        these sizes (rmsf_contact_counts_plan; host only)."""
        v = [ctypes.c_int32(0) for _ in range(4)]
        call("rmsf_contact_counts_plan", n_a, n_b, n_frames, int(bool(symmetric)), *(ctypes.byref(x) for x in v))
        return tuple(x.value for x in v)

    def _rows(self, rows):
        """(host int32 array, its device copy) of a row-index array; (None,
        None) for None, the dense rows."""
        if rows is None:
            return None, None
        h = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        return h, torch.as_tensor(h).to(self.device)

    def contact_counts(self, xyz_ptr: int, fstride: int, n_frames: int, n_atoms: int, rows_a, n_a: int, rows_b,
                       n_b: int, radius: float, symmetric: bool = False, out: torch.Tensor | None = None):
        """int32 [n_a, n_b] in HBM: the frames in which rows a_i and b_j of
        the frames at xyz_ptr are in contact (rmsf_contact_counts,
        csrc/contacts.hip).  ``rows_a`` / ``rows_b``: host index arrays into a
        frame's n_atoms rows, None = rows 0..n-1; ``symmetric``: B is A and
        ``rows_b`` / ``n_b`` are not used.  ``out``: an int32 tensor of at
        least [n_a, n_b] with unit column stride to write into (columns at or
        past n_b are left as they are).  Enqueued, not waited for."""
        h_a, d_a = self._rows(rows_a)
        if symmetric:
            h_b, d_b, n_b = h_a, d_a, n_a
        else:
            h_b, d_b = self._rows(rows_b)
        if (h_a is not None and h_a.size != n_a) or (h_b is not None and h_b.size != n_b):
            raise ValueError("contact_counts: one row index per atom of a side is needed")
        if out is None:
            out = torch.empty((n_a, n_b), dtype=torch.int32, device=self.device)
        elif (out.dtype != torch.int32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < n_a
              or out.shape[1] < n_b or out.stride(0) < n_b):
            raise ValueError("contact_counts: buffer sizes")
        need = int(self.lib.rmsf_contact_counts_workspace_bytes(n_a, n_b, n_frames, int(bool(symmetric))))
        work = torch.empty(need // 8 + 1, dtype=torch.int64, device=self.device) if need else None
        call("rmsf_contact_counts", xyz_ptr, fstride, n_frames, n_atoms, _ptr(d_a), None if h_a is None else
             h_a.ctypes.data, n_a, _ptr(d_b), None if h_b is None else h_b.ctypes.data, n_b, int(bool(symmetric)),
             float(radius), out.data_ptr(), out.stride(0), _ptr(work), need, self.stream)
        return out[:n_a, :n_b]  # (the index copies are freed into the stream the kernels run on)

    def contact_fraction(self, xyz_ptr: int, fstride: int, n_frames: int, n_atoms: int, rows, n_rows: int, pair_a,
                         pair_b, r0, radius: float, method: int, beta: float = 5.0, lambda_constant: float = 1.8):
        """(q f64 [n_frames], n_contacts int32 [n_frames]) in HBM over the
        pairs (rows[pair_a[p]], rows[pair_b[p]]) of each frame
        (rmsf_contact_fraction).  ``rows``: host indices into a frame's
        n_atoms rows, None = rows 0..n_rows-1; ``pair_a`` / ``pair_b``: host
        positions in ``rows``; ``r0``: f64 [P], read by soft_cut alone.
        Enqueued, not waited for."""
        h_rows, d_rows = self._rows(rows)
        h_pa, d_pa = self._rows(pair_a)
        h_pb, d_pb = self._rows(pair_b)
        if h_pa.size != h_pb.size or (h_rows is not None and h_rows.size != n_rows):
            raise ValueError("contact_fraction: buffer sizes")
        d_r0 = None
        if r0 is not None:
            h_r0 = np.ascontiguousarray(r0, dtype=np.float64).reshape(-1)
            if h_r0.size != h_pa.size:
                raise ValueError("contact_fraction: one r0 per pair is needed")
            d_r0 = torch.as_tensor(h_r0).to(self.device)
        q = self.empty(n_frames)
        n = torch.empty(n_frames, dtype=torch.int32, device=self.device)
        call("rmsf_contact_fraction", xyz_ptr, fstride, n_frames, n_atoms, n_rows, _ptr(d_rows),
             None if h_rows is None else h_rows.ctypes.data, d_pa.data_ptr(), d_pb.data_ptr(), h_pa.ctypes.data,
             h_pb.ctypes.data, _ptr(d_r0), h_pa.size, float(radius), int(method), float(beta),
             float(lambda_constant), q.data_ptr(), n.data_ptr(), self.stream)
        return q, n

    def rdf_counts_plan(self, n_a: int, n_b: int, n_frames: int, symmetric: bool = False):
        """(tile_a, tile_b, frame_chunk, n_splits) of rmsf_rdf_counts for these
        sizes (rmsf_rdf_counts_plan; host only)."""
        v = [ctypes.c_int32(0) for _ in range(4)]
        call("rmsf_rdf_counts_plan", n_a, n_b, n_frames, int(bool(symmetric)), *(ctypes.byref(x) for x in v))
        return tuple(x.value for x in v)

    def rdf_counts(self, xyz_ptr: int, fstride: int, n_frames: int, n_atoms: int, rows_a, n_a: int, rows_b, n_b: int,
                   rmin: float, rmax: float, nbins: int, symmetric: bool = False, exclusion_block=None, box=None,
                   out: torch.Tensor | None = None):
        """int64 [nbins] in HBM: the histogram of the distances of rows a_i and
        b_j of the frames at xyz_ptr (rmsf_rdf_counts, csrc/rdf.hip).
        ``rows_a`` / ``rows_b`` / ``symmetric`` as ``contact_counts``;
        ``exclusion_block``: (excl_a, excl_b) or None; ``box``: host f64
        [n_frames, 3] of box edges, None for free space; ``out``: a contiguous
        int64 tensor of at least nbins to write into (entries at or past nbins
        are left as they are).  Enqueued, not waited for."""
        h_a, d_a = self._rows(rows_a)
        if symmetric:
            h_b, d_b, n_b = h_a, d_a, n_a
        else:
            h_b, d_b = self._rows(rows_b)
        if (h_a is not None and h_a.size != n_a) or (h_b is not None and h_b.size != n_b):
            raise ValueError("rdf_counts: one row index per atom of a side is needed")
        ea, eb = (0, 0) if exclusion_block is None else (int(exclusion_block[0]), int(exclusion_block[1]))
        h_box = d_box = None
        if box is not None:
            edge = np.ascontiguousarray(box, dtype=np.float64)
            if edge.shape != (n_frames, 3):
                raise ValueError(f"rdf_counts: box must be [n_frames, 3], got {edge.shape}")
            with np.errstate(divide="ignore", invalid="ignore"):
                h_box = np.ascontiguousarray(np.concatenate([edge, 1.0 / edge], axis=1))
            d_box = torch.as_tensor(h_box).to(self.device)
        nbins = int(nbins)
        if out is None:
            out = torch.empty(max(nbins, 1), dtype=torch.int64, device=self.device)
        elif out.dtype != torch.int64 or out.dim() != 1 or not out.is_contiguous() or out.shape[0] < nbins:
            raise ValueError("rdf_counts: buffer sizes")
        need = int(self.lib.rmsf_rdf_counts_workspace_bytes(nbins))
        work = torch.empty(need // 8 + 1, dtype=torch.int64, device=self.device)
        call("rmsf_rdf_counts", xyz_ptr, fstride, n_frames, n_atoms, _ptr(d_a), None if h_a is None else
             h_a.ctypes.data, n_a, _ptr(d_b), None if h_b is None else h_b.ctypes.data, n_b, int(bool(symmetric)),
             ea, eb, _ptr(d_box), None if h_box is None else h_box.ctypes.data, float(rmin), float(rmax), nbins,
             out.data_ptr(), work.data_ptr(), need, self.stream)
        return out[:nbins]  # (the index, box and workspace copies are freed into the stream the kernel runs on)

    def msd_plane_ld(self, n_frames: int) -> int:
        """The leading dimension ``msd_planes`` gives its planes
        (rmsf_msd_plane_ld; host only)."""
        ld = int(self.lib.rmsf_msd_plane_ld(int(n_frames)))
        if ld < 1:
            raise ValueError(f"msd_plane_ld: {n_frames} frames are out of range")
        return ld

    def msd_plan(self, n_sel: int, n_frames: int, n_lags: int):
        """(lag_block, origin_chunk, n_splits) of rmsf_msd_lags for these
        sizes (rmsf_msd_plan; host only)."""
        v = [ctypes.c_int32(0) for _ in range(3)]
        call("rmsf_msd_plan", n_sel, n_frames, n_lags, *(ctypes.byref(x) for x in v))
        return tuple(x.value for x in v)

    def msd_planes(self, xyz_ptr: int, fstride: int, n_frames: int, n_atoms: int, rows, n_sel: int, box=None,
                   out: torch.Tensor | None = None):
        """f64 [n_sel, 3, ld] in HBM, of which [:, :, :n_frames] is returned:
        the coordinates of the rows ``rows`` (host indices into a frame's
        n_atoms rows, None = rows 0..n_sel-1) of the frames at xyz_ptr,
        widened and atom-major, unwrapped by the nojump rule where ``box``
        (host f64 [n_frames, 3] of box edges) is given (rmsf_msd_planes,
        csrc/msd.hip).  ``out``: a contiguous f64 tensor [>= n_sel, 3, ld >=
        n_frames] to write into; columns n_frames..ld-1 are zeroed.  Enqueued,
        not waited for."""
        h_idx, d_idx = self._rows(rows)
        if h_idx is not None and h_idx.size != n_sel:
            raise ValueError("msd_planes: one row index per atom is needed")
        h_box = d_box = None
        if box is not None:
            edge = np.ascontiguousarray(box, dtype=np.float64)
            if edge.shape != (n_frames, 3):
                raise ValueError(f"msd_planes: box must be [n_frames, 3], got {edge.shape}")
            with np.errstate(divide="ignore", invalid="ignore"):
                h_box = np.ascontiguousarray(np.concatenate([edge, 1.0 / edge], axis=1))
            d_box = torch.as_tensor(h_box).to(self.device)
        if out is None:
            out = self.empty(n_sel, 3, self.msd_plane_ld(n_frames))
        elif (out.dtype != F64 or out.dim() != 3 or not out.is_contiguous() or out.shape[0] < n_sel
              or out.shape[1] != 3 or out.shape[2] < n_frames):
            raise ValueError("msd_planes: buffer sizes")
        call("rmsf_msd_planes", xyz_ptr, fstride, n_frames, n_atoms, _ptr(d_idx), None if h_idx is None else
             h_idx.ctypes.data, n_sel, _ptr(d_box), None if h_box is None else h_box.ctypes.data, out.data_ptr(),
             out.shape[2], self.stream)
        return out[:n_sel, :, :n_frames]  # (the index and box copies are freed into the stream the kernel runs on)

    def msd_lags(self, planes: torch.Tensor, n_frames: int, n_lags: int, dims_mask: int = 7,
                 out: torch.Tensor | None = None, mean: torch.Tensor | bool = True):
        """(msd f64 [n_lags, n_sel], mean f64 [n_lags] or None) in HBM from
        ``msd_planes``' planes [n_sel, 3, >= n_frames] (unit stride along the
        frames): the mean squared displacement of every atom at the lags
        0..n_lags-1 over the coordinates ``dims_mask`` names (bit 0 x, 1 y, 2
        z) and its mean over the atoms (rmsf_msd_lags).  ``out``: an f64
        tensor of at least [n_lags, n_sel] with unit column stride to write
        into (entries past either bound are left as they are); ``mean``: a
        contiguous f64 tensor of at least n_lags to write into, True to
        allocate one, False to skip the mean.  Enqueued, not waited for."""
        if (planes.dtype != F64 or planes.dim() != 3 or planes.shape[1] != 3 or planes.stride(2) != 1
                or planes.shape[2] < n_frames or planes.stride(1) < n_frames
                or planes.stride(0) != 3 * planes.stride(1)):
            raise ValueError("msd_lags: planes must be f64 [n_sel, 3, ld >= n_frames], rows ld apart")
        n_sel, n_lags = planes.shape[0], int(n_lags)
        if out is None:
            out = self.empty(max(n_lags, 1), n_sel)
        elif (out.dtype != F64 or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < n_lags
              or out.shape[1] < n_sel or out.stride(0) < n_sel):
            raise ValueError("msd_lags: buffer sizes")
        if mean is True:
            mean = self.empty(max(n_lags, 1))
        elif mean is False or mean is None:
            mean = None
        elif mean.dtype != F64 or mean.dim() != 1 or not mean.is_contiguous() or mean.shape[0] < n_lags:
            raise ValueError("msd_lags: buffer sizes")
        need = int(self.lib.rmsf_msd_workspace_bytes(n_sel, n_frames, n_lags))
        work = torch.empty(need // 8, dtype=F64, device=self.device) if need else None
        call("rmsf_msd_lags", planes.data_ptr(), planes.stride(1), n_sel, n_frames, n_lags, int(dims_mask),
             out.data_ptr(), out.stride(0), _ptr(mean), _ptr(work), need, self.stream)
        return out[:n_lags, :n_sel], None if mean is None else mean[:n_lags]

    def qcp_batch(self, A: torch.Tensor, E0: torch.Tensor, N: torch.Tensor):
        n = A.shape[0]
        rot = self.empty(n, 9)
        rmsd = self.empty(n)
        call("rmsf_qcp_batch", A.data_ptr(), E0.data_ptr(), N.data_ptr(), n, rot.data_ptr(), rmsd.data_ptr(),
             self.stream)
        return rot, rmsd

    def synth_frames(self, out: torch.Tensor, n_atoms: int, f0: int, nf: int, seed: int,
                     motion: torch.Tensor | None = None, fstride: int | None = None) -> None:
        fstride = 3 * n_atoms if fstride is None else fstride
        call("rmsf_synth_frames", out.data_ptr(), fstride, n_atoms, f0, nf, ctypes.c_uint64(seed).value,
             _ptr(motion), self.stream)


def block_range(n_frames: int, size: int, rank: int) -> tuple[int, int]:
    """RMSF.py:63-72 through the C ABI (bit-exact integer arithmetic)."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    call("rmsf_block_range", n_frames, size, rank, ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


__all__ = ["Engine", "block_range", "RMSF_MODE_SUM", "RMSF_MODE_WELFORD", "RMSF_XFORM_DOUBLES"]
