/*
 * rmsf_hip.h -- C ABI of the MI355X (gfx950) frame-parallel RMSF path.
 *
 * This is the drop-in boundary for the hot path of i2nico/MDAnalysis-MPI
 * `RMSF.py` (the whole reference is that one file).  The reference has no
 * native FFI of its own: its per-frame loops call numpy, MDAnalysis
 * `lib.qcprot` (Cython) and mpi4py.  Every entry point below replaces one of
 * those call sites; the citation `RMSF.py:N` is /root/reference/RMSF.py line N.
 *
 * Conventions (all entry points):
 *   - Plain pointers and sizes only.  `d_` = device pointer (HBM, caller
 *     owned), `h_` = host pointer.  Coordinates are float32 `fac` layout
 *     (frame, atom, xyz); statistics are float64.
 *   - Every call returns an int status: 0 = ok, < 0 = error (see RMSF_E*).
 *     rmsf_last_error() returns a thread-local message for the last failure.
 *     No C++ exception crosses the ABI.
 *   - Device work is enqueued asynchronously on `stream` (a hipStream_t, NULL
 *     = the legacy default stream).  Nothing synchronises unless stated.
 *   - `sel` (int32 atom indices into a frame) may be NULL, meaning atoms
 *     0..n_sel-1 of each frame (the contiguous fast path).
 *   - `frame_stride` is the distance between consecutive frames in floats
 *     (>= 3*n_atoms of the frame; a multiple of it implements `step`).
 */
#ifndef RMSF_HIP_H
#define RMSF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMSF_ABI_VERSION 4

#define RMSF_OK 0
#define RMSF_EINVAL (-1)   /* bad argument (shape, null pointer, size)      */
#define RMSF_EHIP (-2)     /* HIP runtime error                             */
#define RMSF_ENOMEM (-3)   /* allocation failed / workspace too small       */
#define RMSF_EEMPTY (-4)   /* no frames to reduce (RMSF.py:39 would raise   */
                           /* ZeroDivisionError)                            */

/* accumulate modes for rmsf_accumulate() */
#define RMSF_MODE_WELFORD 0 /* n/mean/M2 per coordinate   (RMSF.py:137-138) */
#define RMSF_MODE_SUM 1     /* f64 sum of positions        (RMSF.py:103)     */

/* Size of one per-frame transform record written by rmsf_superpose():
 * R[9] (row-major, applied as x @ R, RMSF.py:100), mobile COM[3], rmsd, pad[3] */
#define RMSF_XFORM_DOUBLES 16
/* longest frame tile one rmsf_accumulate split may hold (Welford
 * coefficient table); n_splits >= ceil(n_frames / RMSF_MAX_SPLIT_FRAMES)    */
#define RMSF_MAX_SPLIT_FRAMES 4096
/* how a pair's lambda was found (rmsf_pair_lambda_host)                      */
#define RMSF_PAIR_NEWTON 0 /* Newton's iteration, at a simple root            */
#define RMSF_PAIR_JACOBI 1 /* largest eigenvalue of the 4 x 4 key matrix       */
#define RMSF_PAIR_ZERO 2   /* E0 <= 0 (two all-zero frames) or NaN: lambda = E0 */
/* Size of the reference record written by rmsf_reference_setup():
 * [0..15]  ref_com[3], sum_r[3] (= sum of centred ref coords),
 *          G_ref (= sum |r|^2), total mass, n_sel, pad[7]
 * [16..]   scratch for the setup's fixed-order block reductions             */
#define RMSF_REFINFO_DOUBLES 2064

/* ---- library / device helpers (for callers without their own allocator) */
int rmsf_abi_version(void);
const char *rmsf_last_error(void);
int rmsf_device_count(int *n);
int rmsf_set_device(int dev);
int rmsf_malloc(void **d_ptr, size_t bytes);
int rmsf_free(void *d_ptr);
int rmsf_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream);
int rmsf_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream);
/* Strided device->device copy of `height` rows of `width` bytes (pitches in
 * bytes), asynchronous on `stream`: fills the HBM frame cache that lets the
 * second sweep (RMSF.py:124) read the frames the first (RMSF.py:92) staged. */
int rmsf_memcpy2d_d2d(void *d_dst, size_t dpitch, const void *d_src, size_t spitch,
                      size_t width, size_t height, void *stream);
int rmsf_stream_synchronize(void *stream);

/* ---- frame-block decomposition: RMSF.py:63-72 ----------------------------
 * per = n_frames // size; ranks 0..size-2 get [r*per, (r+1)*per); the last
 * rank gets [(size-1)*per, n_frames).  Pure integer, bit-exact.            */
int rmsf_block_range(int64_t n_frames, int size, int rank, int64_t *start,
                     int64_t *stop);

/* ---- reference structure: RMSF.py:80-87 (frame `ref_frame`, float32) and
 * RMSF.py:113-118 (the all-reduced float64 average) -------------------------
 * Exactly one of d_frame (float32 frame, atoms addressed via sel) or d_avg
 * (float64 [n_sel*3], already the selection) is non-NULL.
 * ref_com = sum(m x)/sum(m) in f64 (center_of_mass, RMSF.py:84,117);
 * d_ref[n_sel*3] = x - ref_com (f64, RMSF.py:85,118); d_refinfo as above.  */
int rmsf_reference_setup(const float *d_frame, const double *d_avg,
                         int64_t n_sel, const int32_t *d_sel,
                         const double *d_masses, double *d_ref,
                         double *d_refinfo, void *stream);

/* ---- RMSF.py:111 + 113-118 in one call: the sweep-1 average
 * d_avg[n_sel*3] = d_sum / n_frames (f64) and the reference setup from it, as
 * rmsf_divide() followed by rmsf_reference_setup(NULL, d_avg, ...) would
 * write them, bit for bit.  Up to 1,024 selected atoms this is ONE launch
 * (the division done as the sums are read); otherwise the same launches as
 * the two calls.                                                            */
int rmsf_reference_setup_mean(const double *d_sum, double n_frames,
                              int64_t n_sel, const double *d_masses,
                              double *d_avg, double *d_ref, double *d_refinfo,
                              void *stream);

/* ---- superposition: RMSF.py:94-97,127-131 + get_rotation_matrix RMSF.py:43-51
 * For every frame f of the block: mobile COM (mass-weighted, f64), the 3x3
 * inner product A = sum (x-com) (x) ref and E0 against the centred reference
 * (qcprot InnerProduct), then the QCP rotation (qcprot FastCalcRMSDAndRotation,
 * Theobald 2005 / Liu 2010) -> d_xform[f*RMSF_XFORM_DOUBLES + ...].
 * Two launches: a (frame, atom-chunk) covariance reduction and a per-frame
 * QCP solve.  d_work must hold rmsf_superpose_workspace_bytes() bytes.     */
size_t rmsf_superpose_workspace_bytes(int64_t n_sel, int64_t n_frames);
int rmsf_superpose(const float *d_xyz, int64_t frame_stride, int64_t n_frames,
                   int64_t n_sel, const int32_t *d_sel,
                   const double *d_masses, const double *d_ref,
                   const double *d_refinfo, double *d_xform, void *d_work,
                   size_t work_bytes, void *stream);

/* rmsf_superpose over a gathered selection (d_sel != NULL, rows) that also
 * COMPACTS it: every frame's selected rows, as the covariance pass stages
 * them, go out to d_dense_out + f * dense_stride as [n_sel][3] (f32, an exact
 * copy; dense_stride >= 3 n_sel floats, 0 = 3 n_sel), so the passes after it
 * -- the accumulate of this sweep, and with the whole block kept resident
 * every pass of RMSF.py's second sweep -- read n_sel dense rows (d_sel =
 * NULL, frame_stride = dense_stride) instead of gathering them again from
 * the full frames.  Same records, same bits as rmsf_superpose.  A gathered
 * row read costs every 128-B line holding a selected atom -- at CA-like
 * densities (1 in 10) nearly all of the frame -- so each avoided gather saves
 * up to ~10x the selected bytes ("Sparse selections").   */
int rmsf_superpose_compact(const float *d_xyz, int64_t frame_stride,
                           int64_t n_frames, int64_t n_sel, const int32_t *d_sel,
                           const double *d_masses, const double *d_ref,
                           const double *d_refinfo, double *d_xform,
                           void *d_work, size_t work_bytes, float *d_dense_out,
                           int64_t dense_stride, void *stream);

/* The same for frames stored as coordinate planes (SoA): atom a's x, y and
 * z of frame f at d_xyz + f*frame_stride + a (or d_sel[a]) + {0, 1, 2} *
 * plane_stride floats (frame_stride >= 3*plane_stride).  Same workspace,
 * same records, same arithmetic: the planes are read in place.           */
int rmsf_superpose_planes(const float *d_xyz, int64_t frame_stride,
                          int64_t plane_stride, int64_t n_frames,
                          int64_t n_sel, const int32_t *d_sel,
                          const double *d_masses, const double *d_ref,
                          const double *d_refinfo, double *d_xform,
                          void *d_work, size_t work_bytes, void *stream);

/* ---- streaming accumulator: RMSF.py:99-103 (SUM) and RMSF.py:133-138 (WELFORD)
 * For each frame: if d_xform != NULL apply the f32-faithful transform of
 * RMSF.py:99-101 / 133-135
 *     p = f32(f64(p) - com_f); p = f32(f64(p) @ R_f); p = f32(f64(p) + ref_com)
 * (ref_com from d_refinfo), then x = f64(p) feeds
 *   WELFORD: M2 += k/(k+1) (x-mean)^2 ; mean = (k mean + x)/(k+1)
 *   SUM:     sum += x
 * Frames are cut into n_splits contiguous splits (frame tiles); split s
 * holds frames [n_frames*s/n_splits, n_frames*(s+1)/n_splits) and writes
 * d_out0[s*3*n_sel + j] (mean or sum) and, for WELFORD, d_out1 (M2).
 * n_splits <= 0 picks one (see rmsf_accumulate_splits()).  The partials are
 * folded by rmsf_chan_merge() / rmsf_sum_splits().                          */
int rmsf_accumulate_splits(int64_t n_sel, int64_t n_frames, int aligned);
int rmsf_accumulate(const float *d_xyz, int64_t frame_stride, int64_t n_frames,
                    int64_t n_sel, const int32_t *d_sel,
                    const double *d_xform, const double *d_refinfo, int mode,
                    int n_splits, double *d_out0, double *d_out1,
                    void *stream);

/* split s of rmsf_accumulate() holds this many frames */
int64_t rmsf_split_count(int64_t n_frames, int n_splits, int s);

/* ---- balanced streaming accumulator (the default product path) ------------
 * Same arithmetic as rmsf_accumulate(), different work decomposition: the
 * batch's (256-lane chunk, frame) space is cut into n_groups equal contiguous
 * ranges, one per workgroup (n_groups <= 0: a per-kernel multiple of the
 * CU count -- 3 for the float4 Welford, 2 per atom lane, 32 with the
 * transform -- fewer for small batches), so every workgroup streams the same
 * bytes and no tail wave is left.  The partials and a plan header go to d_work
 * (rmsf_accumulate_balanced_workspace_bytes() bytes, 16-B aligned; the
 * bound covers every layout and mode for these n_sel/n_frames/n_groups).
 * rmsf_fold_balanced() then folds them, in frame order, into a running
 * result that already holds acc_n frames (acc_n = 0: d_acc* are
 * overwritten): Chan's merge (RMSF.py:36-41) into d_acc0 = mean,
 * d_acc1 = M2 for WELFORD; d_acc0 += sum for SUM.  n_coord = 3*n_sel.
 * d_work must not be reused between the two calls.                        */
size_t rmsf_accumulate_balanced_workspace_bytes(int64_t n_sel, int64_t n_frames,
                                                int n_groups);
int rmsf_accumulate_balanced(const float *d_xyz, int64_t frame_stride,
                             int64_t n_frames, int64_t n_sel,
                             const int32_t *d_sel, const double *d_xform,
                             const double *d_refinfo, int mode, int n_groups,
                             void *d_work, size_t work_bytes, void *stream);
int rmsf_fold_balanced(const void *d_work, int64_t n_coord, int mode,
                       int64_t acc_n, double *d_acc0, double *d_acc1,
                       void *stream);
/* rmsf_fold_balanced (WELFORD) of the last batch + the finalise of
 * RMSF.py:146 (d_rmsf[n_sel] over n_total frames), bit-identical to
 * rmsf_fold_balanced + rmsf_finalize, for every plan the accumulate can
 * write.  An atom plan (the aligned sweep, a gathered selection, planes: one
 * atom per lane) finalises inside the fold (one launch); the flat plan of an
 * unaligned contiguous selection (an atom's coordinates span two lanes) is
 * finalised by a second launch.  The plan is read from the workspace's own
 * header on the device (the host keeps no record of workspaces).          */
int rmsf_fold_balanced_finalize(const void *d_work, int64_t n_coord,
                                int64_t acc_n, double *d_acc0, double *d_acc1,
                                int64_t n_total, double *d_rmsf, void *stream);
/* The accumulate (RMSF.py:99-103 / 133-138 with d_xform, else the raw
 * frames) over frames stored as coordinate planes (see
 * rmsf_superpose_planes), read in place, one atom per lane; partials, header
 * and fold as rmsf_accumulate_balanced's.  (Without a selection, the
 * unaligned sweep can also read contiguous planes as rows of 3n floats on
 * the float4 stream and permute its statistics with rmsf_planes_to_rows.)  */
int rmsf_accumulate_balanced_planes(const float *d_xyz, int64_t frame_stride,
                                    int64_t plane_stride, int64_t n_frames,
                                    int64_t n_sel, const int32_t *d_sel,
                                    const double *d_xform,
                                    const double *d_refinfo, int mode,
                                    int n_groups, void *d_work,
                                    size_t work_bytes, void *stream);

/* ---- Chan merge: second_order_moments, RMSF.py:36-41 ------------------------
 * op(S1, S2): T = n1+n2, mu = (n1 mu1 + n2 mu2)/T, M = M1+M2+(n1 n2/T)(mu2-mu1)^2,
 * with RMSF.py's operations in its order (no FP contraction; n1 n2 / T as
 * Python's exact int product and one rounded division, exact for
 * n1 n2 < 2^53), so every value RMSF.py produces is reproduced bit for bit.
 * An empty partial (count 0) is RMSF.py:119-121's (0, zeros, zeros) -- its
 * memory is not read -- and enters op like any other (op((0,0,0), S) is not
 * S bit for bit, as in RMSF.py).  op of two empty partials (T = 0), where
 * RMSF.py:39 raises ZeroDivisionError, is skipped: the result stays empty.
 * RMSF_EEMPTY when every partial is empty.
 *
 * rmsf_chan_merge folds n_parts partials of n_coord coordinates in order:
 * res = part 0, res = op(res, part i) for i = 1..n_parts-1 (mpi4py's naive
 * reduce, RMSF_MERGE_RANK below).  h_counts: host array of n_parts counts. */
int rmsf_chan_merge(const double *d_mean_parts, const double *d_m2_parts,
                    const int64_t *h_counts, int n_parts, int64_t n_coord,
                    double *d_mean, double *d_m2, void *stream);

/* The order RMSF.py:143's comm.reduce(S, root=0, op=second_order_moments)
 * applies op in (mpi4py's lowercase object reduce; upstream, not vendored):
 *   RMSF_MERGE_MPI4PY  mpi4py's default (rc.fast_reduce): a binomial tree,
 *                      for mask = 1, 2, 4, ...: rank r, r % (2 mask) == 0,
 *                      computes op(S_r, S_{r+mask}) -- at 4 ranks
 *                      op(op(S0,S1), op(S2,S3)), at 5 op(op(op(S0,S1),
 *                      op(S2,S3)), S4).  Equal to RANK up to 3 ranks.
 *   RMSF_MERGE_RANK    rc.fast_reduce = False: op folded in rank order.   */
#define RMSF_MERGE_RANK 0
#define RMSF_MERGE_MPI4PY 1
/* The schedule as (dst, src) steps S[dst] = op(S[dst], S[src]), S[0] the
 * result: returns the step count (n_parts - 1) and, when h_dst/h_src are
 * non-NULL, writes up to `capacity` steps.                                   */
int rmsf_chan_reduce_steps(int n_parts, int order, int *h_dst, int *h_src,
                           int capacity);
/* comm.reduce's result over n_parts partials (the ranks' S of RMSF.py:140,
 * in rank order) in the given order, written to d_mean / d_m2.  The parts
 * are the schedule's working storage (each rank's `result`, as in mpi4py)
 * and are overwritten.                                                      */
int rmsf_chan_reduce(double *d_mean_parts, double *d_m2_parts,
                     const int64_t *h_counts, int n_parts, int64_t n_coord,
                     int order, double *d_mean, double *d_m2, void *stream);
/* One step S1 = op(S1, S2) in place (S2 in separate buffers: the partial
 * another rank or device just sent) -- a distributed reduction's building
 * block.  RMSF_EEMPTY when n1 = n2 = 0.                                    */
int rmsf_chan_merge_pair(double *d_mean1, double *d_m21, int64_t n1,
                         const double *d_mean2, const double *d_m22,
                         int64_t n2, int64_t n_coord, void *stream);

/* sum of split partial sums (sweep 1, RMSF.py:103,105) */
int rmsf_sum_splits(const double *d_parts, int n_parts, int64_t n_coord,
                    double *d_sum, void *stream);

/* y = x / divisor  (average structure, RMSF.py:111) */
int rmsf_divide(const double *d_x, double divisor, int64_t n, double *d_y,
                void *stream);

/* Exact k-way Chan across ranks as two all-reduce(SUM) passes (replaces the
 * pickle comm.reduce of RMSF.py:143):
 *   pass 1 input: d_out = w * mean_k            (w = n_k / n)
 *   pass 2 input: d_out = M2_k + n_k (mean_k - mean)^2                      */
int rmsf_chan_weight(const double *d_mean_k, double w, int64_t n,
                     double *d_out, void *stream);
int rmsf_chan_deviation(const double *d_mean_k, const double *d_m2_k,
                        const double *d_mean, double n_k, int64_t n,
                        double *d_out, void *stream);

/* One-collective form of the same merge (RMSF.py:140-143 + 146): moments
 * about a shift c held by every rank (c[j] = shift[j] + off3[j % 3]; shift
 * f64, or f32 when shift_is_f32; off3 may be NULL):
 *   pack:   d_t[0:n] = n_k (mean_k - c),  d_t[n:2n] = M2_k + n_k (mean_k - c)^2
 *   -- one all-reduce(SUM) of d_t[0:2n] over the ranks --
 *   finish: mean = c + T1/n,  M2 = max(T2 - T1^2/n, 0),  rmsf = sqrt(sum M2 / n)
 * (d_rmsf may be NULL; n = 3 n_sel coordinates).                           */
int rmsf_chan_shift_pack(const double *d_mean_k, const double *d_m2_k,
                         const void *d_shift, int shift_is_f32,
                         const double *d_off3, double n_k, int64_t n,
                         double *d_t, void *stream);
int rmsf_chan_shift_finish(const double *d_t, const void *d_shift,
                           int shift_is_f32, const double *d_off3,
                           int64_t n_sel, int64_t n_frames, double *d_mean,
                           double *d_m2, double *d_rmsf, void *stream);

/* rmsf_fold_balanced (WELFORD) and rmsf_chan_shift_pack in ONE launch, for a
 * rank's last batch before the cross-rank merge: the fold as above, then
 * d_t as the pack writes it, with n_k = acc_n + the batch's frames --
 * bit-identical to the two calls (RMSF.py:36-41 + 140-143).                */
int rmsf_fold_balanced_shift(const void *d_work, int64_t n_coord,
                             int64_t acc_n, double *d_acc0, double *d_acc1,
                             const void *d_shift, int shift_is_f32,
                             const double *d_off3, double *d_t, void *stream);

/* The reduce-scatter form of the merge (RMSF.py:140-143 with :146 on each
 * rank's atom slice, then only the RMSF gathered to the root): the same
 * T1/T2 in the ATOM-SLICED layout -- for slice_coords = 3 x atoms per rank,
 * slice r = j / slice_coords holds [T1 | T2] of its slice_coords
 * coordinates at d_t + 2 r slice_coords (T2 slice_coords after T1), so a
 * reduce-scatter of equal chunks gives rank r its slice; coordinates past n
 * in the last slice are not written (the caller zeroes that padding).
 * rmsf_chan_shift_finish_slice unpacks one reduced slice [T1 | T2] of width
 * slice_coords for its n_sel atoms (d_shift, d_mean, d_m2, d_rmsf point at
 * the slice's first atom).  Bit-identical per coordinate to the plain
 * layout's pack and finish.                                                 */
int rmsf_fold_balanced_shift_sliced(const void *d_work, int64_t n_coord,
                                    int64_t acc_n, double *d_acc0,
                                    double *d_acc1, const void *d_shift,
                                    int shift_is_f32, const double *d_off3,
                                    int64_t slice_coords, double *d_t,
                                    void *stream);
int rmsf_chan_shift_pack_sliced(const double *d_mean_k, const double *d_m2_k,
                                const void *d_shift, int shift_is_f32,
                                const double *d_off3, double n_k, int64_t n,
                                int64_t slice_coords, double *d_t,
                                void *stream);
int rmsf_chan_shift_finish_slice(const double *d_t, int64_t slice_coords,
                                 const void *d_shift, int shift_is_f32,
                                 const double *d_off3, int64_t n_sel,
                                 int64_t n_frames, double *d_mean, double *d_m2,
                                 double *d_rmsf, void *stream);

/* Atom slabs of the flat WELFORD plan (no selection, no transform, 16-B
 * aligned float4 columns), so a rank's cross-rank merge can start on the
 * first slab while the next one streams (large n_sel; RMSF.py:140-143).
 * rmsf_balanced_slab_chunks: *h_chunks = the plan's chunk count C (256
 * lanes of 4 coordinates = 1024 coordinates each) when the plan is
 * chunk-aligned, else 0 (no slabs).  rmsf_accumulate_balanced_slab runs
 * the whole plan's ranges of chunks [c0, c1) -- the same segments, so the
 * slab's partials equal the whole launch's -- into the same d_work;
 * rmsf_fold_balanced_shift_slab folds those chunks into d_acc* (global
 * coordinates) and writes the slab's [T1 | T2] (2 (j1 - j0) doubles,
 * j0 = 1024 c0, j1 = min(1024 c1, n_coord)) to d_t.  Bit-identical to the
 * whole-selection calls for every coordinate.  Slab bounds that are a
 * multiple of 3 chunks keep whole atoms together (rmsf_chan_shift_finish
 * per slab).                                                               */
int rmsf_balanced_slab_chunks(const float *d_xyz, int64_t frame_stride,
                              int64_t n_frames, int64_t n_sel,
                              int64_t *h_chunks);
int rmsf_accumulate_balanced_slab(const float *d_xyz, int64_t frame_stride,
                                  int64_t n_frames, int64_t n_sel, int64_t c0,
                                  int64_t c1, void *d_work, size_t work_bytes,
                                  void *stream);
int rmsf_fold_balanced_shift_slab(const void *d_work, int64_t n_coord,
                                  int64_t acc_n, double *d_acc0,
                                  double *d_acc1, const void *d_shift,
                                  int shift_is_f32, const double *d_off3,
                                  double *d_t, int64_t c0, int64_t c1,
                                  void *stream);

/* ---- RMSF.py:137-138 as written: the sequential Welford ---------------------
 * For every selected coordinate (atom d_sel[a], or a, when d_sel is NULL;
 * f32 rows d_xyz[f * frame_stride + 3 atom + c], no transform), the frames
 * f = 0 .. n_frames-1 in order with k = k0 + f:
 *   sumsquares += (k / (k + 1.0)) * (x - mean)**2 ;  mean = (k*mean + x)/(k+1)
 * in numpy's operations and roundings, so d_mean / d_sumsquares (f64
 * [3 n_sel], the running state after k0 frames; k0 = 0: start from zeros,
 * inputs ignored) end as the reference recurrence's own values bit for bit
 * -- a rank's S of RMSF.py:140, which rmsf_chan_merge then combines as
 * RMSF.py:143 does, also bit for bit.  Parallel over coordinates only (one
 * lane per coordinate through every frame; one lane per atom for a d_sel of
 * >= 49,152 atoms -- same bits); rmsf_accumulate_balanced is the
 * reassociated, frame-parallel form (faster, equal to ~1e-13).
 * d_work: rmsf_welford_sequential_workspace_bytes(n_frames) bytes (the
 * per-frame coefficients).  Replaces RMSF.py:120-138's loop for one rank.
 * Domain of the bit-for-bit claim: any float32 coordinates (zeros and
 * infinities included; NaN wherever the reference has NaN, payload bits
 * aside) and any running state they can produce; a caller-made state with
 * |mean| beyond ~1e270 would need the full division sequence.              */
size_t rmsf_welford_sequential_workspace_bytes(int64_t n_frames);
int rmsf_welford_sequential(const float *d_xyz, int64_t frame_stride,
                            int64_t n_frames, int64_t n_sel,
                            const int32_t *d_sel, int64_t k0, double *d_mean,
                            double *d_sumsquares, void *d_work,
                            size_t work_bytes, void *stream);

/* ---- exact=True on the ALIGNED path: RMSF.py:80-146 in the reference's own
 * summation orders -----------------------------------------------------------
 * The frame-parallel kernels above (rmsf_reference_setup, rmsf_superpose,
 * rmsf_accumulate*) reassociate the per-frame sums; their rotations then
 * differ from the script's in the last bits, which now and then flips an
 * f32 rounding point of an aligned coordinate (RMSF.py:99-101) -- a few
 * e-8 A at 100 frames, but up to ~ulp/2 = 2e-6 A at 2 frames.  These three
 * entry points remove every such source: each sum runs atom by atom or
 * frame by frame exactly as the reference runs it, so the transform records,
 * the sweep-1 sums, the average and the Welford state equal the script's
 * bit for bit.  The orders of the absent upstream dependencies are the
 * published ones, restated (oracle/rmsf_oracle.py; upstream, unverified):
 *   AtomGroup.center_of_mass(): einsum('ij,ij->j', x, m[:, None]) / m.sum()
 *     -- a sequential sum over the atoms of f64(x) * m, divided by
 *     mass_total = the caller's numpy ``masses.sum()`` (numpy sums pairwise;
 *     n_sel when d_masses is NULL, i.e. unit masses);
 *   qcprot InnerProduct: one pass over the atoms, A[3a+b] += mob_a ref_b,
 *     G1 += x*x + y*y + z*z per atom, E0 = (G1 + G2) * 0.5.
 *
 * rmsf_reference_setup_sequential: RMSF.py:84-85 (d_frame, f32, atoms via
 * d_sel) or RMSF.py:111 + 117-118 (d_avg = the all-reduced f64 sweep-1 sums,
 * divided by avg_divisor = n_frames as they are read and written to
 * d_avg_out when non-NULL; d_sel must be NULL): ref_com, d_ref = x - ref_com,
 * and the refinfo record (ref_com, sum r, G2 of qcprot's loop, mass_total,
 * n_sel).  Each sum is one wave's in-order add chain (two chain phases,
 * ~0.2 ms each per 100k atoms); below 16,384 atoms one launch, from there
 * the fill and the centring as grid-wide launches around the chains.      */
int rmsf_reference_setup_sequential(const float *d_frame, const double *d_avg,
                                    double avg_divisor, int64_t n_sel,
                                    const int32_t *d_sel, const double *d_masses,
                                    double mass_total, double *d_avg_out,
                                    double *d_ref, double *d_refinfo,
                                    void *stream);
/* The two halves of rmsf_reference_setup_sequential, same bits and the same
 * arguments: rmsf_reference_centre_sequential writes d_ref (centred) and
 * d_refinfo[0..2] (ref_com) -- all an InnerProduct needs;
 * rmsf_reference_sums_sequential writes the rest of the record from the
 * centred d_ref (sum r, G2, mass_total, n_sel).  Only the QCP reads G2, so the
 * sums may run on another stream beside rmsf_inner_product_sequential.    */
int rmsf_reference_centre_sequential(const float *d_frame, const double *d_avg,
                                     double avg_divisor, int64_t n_sel,
                                     const int32_t *d_sel, const double *d_masses,
                                     double mass_total, double *d_avg_out,
                                     double *d_ref, double *d_refinfo,
                                     void *stream);
int rmsf_reference_sums_sequential(int64_t n_sel, double mass_total,
                                   const double *d_ref, double *d_refinfo,
                                   void *stream);
/* rmsf_superpose_sequential: RMSF.py:94-97 / 127-131 + get_rotation_matrix
 * for every frame: mobile COM atom by atom, centred coordinates f64(x) - com,
 * InnerProduct against d_ref (G2 from d_refinfo[6], i.e. a record of
 * rmsf_reference_setup_sequential), QCP -> d_xform[f * RMSF_XFORM_DOUBLES]
 * as rmsf_superpose writes it (COM absolute).  Rows only (frame, atom, xyz).
 * Three launches: the COM (one wave per frame and axis), the InnerProduct
 * (one wave per frame and sum: A[0..8], G1) and the QCP (one lane per
 * frame); d_xform holds the COM and the sums in between.  Each sum is an
 * in-order add chain over the atoms, so the cost grows with n_sel, not the
 * frames: ~0.7 ms per 100k atoms ("Few frames").       */
int rmsf_superpose_sequential(const float *d_xyz, int64_t frame_stride,
                              int64_t n_frames, int64_t n_sel,
                              const int32_t *d_sel, const double *d_masses,
                              double mass_total, const double *d_ref,
                              const double *d_refinfo, double *d_xform,
                              void *stream);
/* The two halves of rmsf_superpose_sequential, same bits:
 * rmsf_frame_com_sequential writes every frame's mobile COM (RMSF.py:94 /
 * 127) to d_xform[f * RMSF_XFORM_DOUBLES + 9..11]; it needs no reference, so
 * it may run on another stream beside rmsf_reference_setup_sequential.
 * rmsf_superpose_sequential_from_com then runs the InnerProduct and the QCP
 * from those COMs (it keeps [9..11] and rewrites the rest of the record).
 * It is in turn rmsf_inner_product_sequential (A[0..8] and G1 into the
 * record's [0..8] and [13]; needs the centred d_ref only) followed by
 * rmsf_superpose_sequential_qcp (E0 = (G1 + d_refinfo[6]) * 0.5 and the QCP:
 * R in [0..8], rmsd in [12], [13..15] zero).                                */
int rmsf_frame_com_sequential(const float *d_xyz, int64_t frame_stride,
                              int64_t n_frames, int64_t n_sel,
                              const int32_t *d_sel, const double *d_masses,
                              double mass_total, double *d_xform, void *stream);
int rmsf_superpose_sequential_from_com(const float *d_xyz, int64_t frame_stride,
                                       int64_t n_frames, int64_t n_sel,
                                       const int32_t *d_sel, const double *d_ref,
                                       const double *d_refinfo, double *d_xform,
                                       void *stream);
int rmsf_inner_product_sequential(const float *d_xyz, int64_t frame_stride,
                                  int64_t n_frames, int64_t n_sel,
                                  const int32_t *d_sel, const double *d_ref,
                                  double *d_xform, void *stream);
int rmsf_superpose_sequential_qcp(int64_t n_frames, int64_t n_sel,
                                  const double *d_refinfo, double *d_xform,
                                  void *stream);
/* rmsf_accumulate_sequential: the frames in order for every selected atom
 * (one lane per atom), k = k0 + f, each frame transformed first when d_xform
 * (+ d_refinfo) is given (RMSF.py:99-101 / 133-135, the same f32-faithful
 * transform as rmsf_accumulate), then
 *   RMSF_MODE_SUM:     d_acc0 += x                          (RMSF.py:103)
 *   RMSF_MODE_WELFORD: rmsf_welford_sequential's recurrence (RMSF.py:137-138)
 *                      on (d_acc0 = mean, d_acc1 = sumsquares)
 * continuing the running state after k0 frames (k0 = 0: from zeros).  The
 * WELFORD mode needs d_work of rmsf_welford_sequential_workspace_bytes
 * (n_frames) bytes; SUM needs none.  Rows only.                            */
int rmsf_accumulate_sequential(const float *d_xyz, int64_t frame_stride,
                               int64_t n_frames, int64_t n_sel,
                               const int32_t *d_sel, const double *d_xform,
                               const double *d_refinfo, int mode, int64_t k0,
                               double *d_acc0, double *d_acc1, void *d_work,
                               size_t work_bytes, void *stream);

/* ---- finalise: RMSF.py:146  rmsf = sqrt(M2.sum(axis=1) / n) ---------------*/
int rmsf_finalize(const double *d_m2, int64_t n_sel, int64_t n_frames,
                  double *d_rmsf, void *stream);

/* ---- positional covariance (the preamble of MDAnalysis.analysis.pca.PCA) --
 * The co-moment matrix of the selected coordinates, of which RMSF.py:146's
 * RMSF is the diagonal, on the f64 matrix cores (v_mfma_f64_16x16x4_f64;
 * csrc/covariance.hip).  Coordinate index i = 3 a + c over the selection's
 * order (atom d_sel[a], or a when d_sel is NULL; rows only).
 * rmsf_covariance_accumulate, for every frame f of the batch:
 *   p = the atom's three floats -- through the transform of RMSF.py:99-101 /
 *       133-135 with the frame's record d_xform[f] and ref_com =
 *       d_refinfo[0..2] when both are given (the same device function the
 *       accumulate runs: the Welford sweep's coordinates bit for bit), the
 *       raw floats when both are NULL;
 *   d = f64(p) - d_shift (f64 [3 n_sel], something near the data);
 *   d_cov[i * ld + j] += sum_f d_i d_j  for every 48 x 48 block that holds an
 *       element with j >= i (the strict lower blocks are not touched);
 *   d_t1[i] += sum_f d_i.
 * The caller zeroes d_cov (ld >= 3 n_sel doubles a row) and d_t1 before the
 * first batch.  Work is cut into (tile pair, frame range) workgroups; with
 * more than one frame range the partials go to d_work
 * (rmsf_covariance_workspace_bytes() bytes, 0 when none is needed and d_work
 * may be NULL) and are summed in frame order by a second launch: no
 * floating-point atomics, the same bits for the same inputs and batching.
 * rmsf_covariance_finish, after the last batch (and after d_cov and d_t1 were
 * summed over the ranks), over n_frames frames in all:
 *   d_cov = d_cov - d_t1 d_t1^T / n_frames, the centred co-moment, read from
 *   the upper triangle and written to both, exactly symmetric.
 * covariance = d_cov / n_frames (numpy.cov: / (n_frames - 1)).              */
size_t rmsf_covariance_workspace_bytes(int64_t n_sel, int64_t n_frames);
int rmsf_covariance_accumulate(const float *d_xyz, int64_t frame_stride,
                               int64_t n_frames, int64_t n_sel,
                               const int32_t *d_sel, const double *d_xform,
                               const double *d_refinfo, const double *d_shift,
                               double *d_cov, int64_t ld, double *d_t1,
                               void *d_work, size_t work_bytes, void *stream);
int rmsf_covariance_finish(double *d_cov, int64_t ld, const double *d_t1,
                           int64_t n_coord, int64_t n_frames, void *stream);

/* ---- time-lagged co-moment (the contraction of TICA) -----------------------
 * The covariance contraction with its two operands apart in time, on the f64
 * matrix cores (csrc/covariance.hip).  Coordinate index i = 3 a + c over the
 * selection's order, p and d as rmsf_covariance_accumulate has them.  Pair q
 * of the batch is frame q of operand A (d_xyz_a, frame_stride_a, records
 * d_xform_a) and frame q of operand B (d_xyz_b, frame_stride_b, d_xform_b);
 * for one resident array the caller passes b = a + lag * stride (and its
 * records lag further on): the kernel never adds a lag itself.
 * rmsf_lagged_comoment_accumulate:
 *   d_s[i * ld + j] += sum_q d_i(frame q of A) d_j(frame q of B)
 * for every i, j < 3 n_sel: all of the matrix, which is not symmetric.  The
 * caller zeroes d_s (ld >= 3 n_sel doubles a row) before the first batch.
 * Work is cut into (48 x 48 tile, pair range) workgroups over the full square
 * of tiles; with more than one pair range the partials go to d_work
 * (rmsf_lagged_comoment_workspace_bytes() bytes, host-only arithmetic, 0 when
 * none is needed and d_work may be NULL) and are summed in range order by a
 * second launch: no floating-point atomics, the same bits for the same
 * inputs and batching.  d_xform_a, d_xform_b and d_refinfo are given
 * together or all NULL (RMSF_EINVAL otherwise, as for a NULL pointer or
 * ld < 3 n_sel; a workspace too small: RMSF_ENOMEM); n_pairs == 0: RMSF_OK.
 * rmsf_lagged_comoment_finish, after the last batch, with d_t[i] = the sum of
 * d_i over both windows' frames (m of them in all):
 *   d_s = d_s + d_s^T - d_t d_t^T / m  in place, each element's sum formed
 *   once and stored to (i, j) and (j, i): exactly symmetric.                */
size_t rmsf_lagged_comoment_workspace_bytes(int64_t n_sel, int64_t n_pairs);
int rmsf_lagged_comoment_accumulate(const float *d_xyz_a,
                                    int64_t frame_stride_a,
                                    const float *d_xyz_b,
                                    int64_t frame_stride_b, int64_t n_pairs,
                                    int64_t n_sel, const int32_t *d_sel,
                                    const double *d_xform_a,
                                    const double *d_xform_b,
                                    const double *d_refinfo,
                                    const double *d_shift, double *d_s,
                                    int64_t ld, void *d_work,
                                    size_t work_bytes, void *stream);
int rmsf_lagged_comoment_finish(double *d_s, int64_t ld, const double *d_t,
                                int64_t n_coord, int64_t m, void *stream);

/* ---- PCA projection (MDAnalysis.analysis.pca.PCA.transform) ----------------
 * The projection of a batch's frames on n_comp components, a tall, skinny
 * product [n_frames x 3 n_sel] . [3 n_sel x n_comp] on the f64 matrix cores
 * (csrc/pca_project.hip).  Coordinate index i = 3 a + c over the selection's
 * order (atom d_sel[a], or a when d_sel is NULL; rows only).  For every frame
 * f of the batch:
 *   p = the atom's three floats -- through the transform of RMSF.py:99-101 /
 *       133-135 with the frame's record d_xform[f] and ref_com =
 *       d_refinfo[0..2] when both are given (the device function the Welford
 *       and covariance sweeps run: their coordinates bit for bit), the raw
 *       floats when both are NULL;
 *   d_i = f64(p_i) - d_mean[i]   (d_mean f64 [3 n_sel]);
 *   d_out[f * ldo + c] = sum_i d_i d_comp[i * ldc + c],  c < n_comp
 *       (d_comp f64 [3 n_sel][ldc >= n_comp], row i = coordinate i; d_out f64
 *       [n_frames][ldo >= n_comp], overwritten; columns >= n_comp of either
 *       are neither read nor written).
 * Work is cut into (16 frames, panel of 48 components, coordinate range)
 * workgroups, so each frame's bytes are read once for n_comp <= 48.  With
 * more than one coordinate range (few frames, many atoms) the partials go to
 * d_work (rmsf_pca_project_workspace_bytes() bytes, 0 when none is needed and
 * d_work may be NULL) and are summed in coordinate order by a second launch:
 * no floating-point atomics.  The plan is a function of (n_frames, n_sel,
 * n_comp) alone: the same bits for the same inputs.
 * rmsf_pca_project_workspace_bytes is host-only arithmetic (no device).
 * Bad arguments (a NULL pointer, n_comp < 1, ldc or ldo < n_comp, one of
 * d_xform and d_refinfo without the other, a workspace too small):
 * RMSF_EINVAL.                                                              */
size_t rmsf_pca_project_workspace_bytes(int64_t n_frames, int64_t n_sel,
                                        int64_t n_comp);
int rmsf_pca_project(const float *d_xyz, int64_t frame_stride,
                     int64_t n_frames, int64_t n_sel, const int32_t *d_sel,
                     const double *d_xform, const double *d_refinfo,
                     const double *d_mean, const double *d_comp, int64_t ldc,
                     int64_t n_comp, double *d_out, int64_t ldo, void *d_work,
                     size_t work_bytes, void *stream);

/* ---- PCA back-projection: the adjoint of the projection --------------------
 * The product that contracts over the frames, [3 n_sel x n_frames] . [n_frames
 * x n_cols] on the f64 matrix cores (csrc/pca_backproject.hip).  With
 * rmsf_pca_project it is the matrix-free covariance product
 * M Q = D^T (D Q) / (F - ddof) of PCA(solver="matrix_free"), which never
 * forms the [3n, 3n] matrix.  Everything not stated here follows
 * rmsf_pca_project: the coordinate index i = 3 a + c, the selection, p (through
 * the same device function as the Welford, covariance and projection sweeps
 * when d_xform and d_refinfo are both given, the raw floats when both are
 * NULL) and d_i(f) = f64(p_i) - d_mean[i].
 *   d_y[i * ldy + c] = (accumulate ? d_y[i * ldy + c] : 0)
 *                      + sum_f d_i(f) d_p[f * ldp + c],  i < 3 n_sel, c < n_cols
 *       (d_p f64 [n_frames][ldp >= n_cols], row f = frame f of the batch; d_y
 *       f64 [3 n_sel][ldy >= n_cols]; 1 <= n_cols <= 48; columns >= n_cols of
 *       either are neither read nor written).  accumulate = 1 is how a
 *       streamed trajectory adds its batches, in batch order.  n_frames = 0
 *       is RMSF_OK and leaves d_y as it is.
 * Work is cut into (16 atoms = 48 coordinates, frame range) workgroups.  With
 * more than one frame range (few atoms, many frames) the partials go to d_work
 * (rmsf_pca_backproject_workspace_bytes() bytes, 0 when none is needed and
 * d_work may be NULL) and are summed in frame-range order by a second launch,
 * from d_y when accumulating and else from the first range's partial (so a
 * sum of negative zeros keeps its sign, as the one-range path's store does):
 * no floating-point atomics.  The plan is a function of (n_frames, n_sel,
 * n_cols) alone: the same bits for the same inputs and batching.
 * rmsf_pca_backproject_workspace_bytes is host-only arithmetic (no device).
 * Bad arguments (a NULL pointer, n_cols < 1 or > 48, ldp or ldy < n_cols, one
 * of d_xform and d_refinfo without the other, a workspace too small):
 * RMSF_EINVAL, before any launch.                                           */
size_t rmsf_pca_backproject_workspace_bytes(int64_t n_frames, int64_t n_sel,
                                            int64_t n_cols);
int rmsf_pca_backproject(const float *d_xyz, int64_t frame_stride,
                         int64_t n_frames, int64_t n_sel, const int32_t *d_sel,
                         const double *d_xform, const double *d_refinfo,
                         const double *d_mean, const double *d_p, int64_t ldp,
                         int64_t n_cols, double *d_y, int64_t ldy,
                         int accumulate, void *d_work, size_t work_bytes,
                         void *stream);

/* ---- block products of a device-side eigen-solver (PCA(solver="device")) ---
 * The three products of a blocked subspace iteration with Rayleigh-Ritz on a
 * symmetric f64 matrix that stays in HBM (csrc/eigen_block.hip; the driver is
 * rmsf_amd/eigen.py).  A block is a tall, skinny f64 matrix of n rows and at
 * most 48 columns; every leading dimension is in doubles, and the columns of
 * a row past the block's width are neither read nor written.
 * rmsf_symm_block:  d_y[r * ldy + c] = sum_k d_m[r * ldm + k] d_q[k * ldq + c]
 *   for r < n, c < n_cols <= 48: Y = M Q on the f64 matrix cores
 *   (v_mfma_f64_16x16x4_f64), M read once (8 n^2 bytes).
 *   PRECONDITION: d_m [n][ldm >= n] is symmetric in its bits, d_m[i][j] ==
 *   d_m[j][i] -- the kernel reads M[k][r] where the formula has M[r][k].
 *   rmsf_covariance_finish writes such a matrix; an element-wise division of
 *   it keeps the property.  Work is cut into (48 rows of Y, range of k)
 *   workgroups; with more than one range the partials go to d_work
 *   (rmsf_symm_block_workspace_bytes() bytes, 0 when none is needed and
 *   d_work may be NULL) and are summed in range order by a second launch.
 * rmsf_block_gram:  d_g[i * ldg + j] = sum_r d_a[r * lda + i] d_b[r * ldb + j]
 *   for i < na <= 48, j < nb <= 48: G = A^T B, contracted over the n rows on
 *   the matrix cores; the rows are cut into ranges over the workgroups, whose
 *   partials go to d_work (rmsf_block_gram_workspace_bytes() bytes, as above)
 *   and are summed in range order.  d_a == d_b is allowed.
 * rmsf_block_update:  d_c[r * ldc + c] = alpha d_a[r * lda + c]
 *   + sum_j d_b[r * ldb + j] d_t[j * ldt + c]  for r < n, c < nc <= 48, j < nb
 *   <= 48: C = alpha A + B T with the small matrix T [nb][ldt >= nc] in HBM,
 *   the nb products summed in order of j.  d_a NULL: C = B T.  d_c may be
 *   d_a; it must not be d_b.
 * No floating-point atomics; every plan is a function of the shape alone
 * (n and the column counts): the same bits for the same inputs.  The
 * *_workspace_bytes functions are host-only arithmetic (no device).  Bad
 * arguments (a NULL pointer other than d_a and an unneeded d_work, a size
 * < 1, a leading dimension smaller than the width it strides, more than 48
 * columns, a workspace too small): RMSF_EINVAL.                              */
size_t rmsf_symm_block_workspace_bytes(int64_t n, int64_t n_cols);
int rmsf_symm_block(const double *d_m, int64_t ldm, int64_t n,
                    const double *d_q, int64_t ldq, int64_t n_cols,
                    double *d_y, int64_t ldy, void *d_work, size_t work_bytes,
                    void *stream);
size_t rmsf_block_gram_workspace_bytes(int64_t n, int64_t na, int64_t nb);
int rmsf_block_gram(const double *d_a, int64_t lda, int64_t na,
                    const double *d_b, int64_t ldb, int64_t nb, int64_t n,
                    double *d_g, int64_t ldg, void *d_work, size_t work_bytes,
                    void *stream);
int rmsf_block_update(double alpha, const double *d_a, int64_t lda,
                      const double *d_b, int64_t ldb, int64_t nb,
                      const double *d_t, int64_t ldt, int64_t n, int64_t nc,
                      double *d_c, int64_t ldc, void *stream);

/* ---- diffusion kernel of a distance matrix (DiffusionMap(solver="device")) --
 * rmsf_diffusion_kernel: in one pass over d_m[n][ld] (f64, ld >= n, in HBM)
 *   every distance d becomes exp(-(d * d) / epsilon) in place, and d_rowsum[r]
 *   receives the sum of row r's n new values (csrc/diffusion.hip): 8 n^2 bytes
 *   read, 8 n^2 written.  The argument is formed as written, with a true f64
 *   division, so it has the bits numpy gives it and only the two exp can
 *   differ.  d = 0 gives exactly 1; d = +-inf, or an argument below exp's
 *   underflow point, exactly 0; a NaN stays NaN and makes its row's sum NaN.
 *   The transform is element-wise: a matrix symmetric in its bits stays so
 *   (rmsf_symm_block's precondition).  Columns n..ld-1 are neither read nor
 *   written.  A row's sum has a fixed order -- each lane's terms in column
 *   order, the 64 lanes by a halving tree, the waves in order -- and no
 *   atomics: the same bits on every run.  Rows that are all 16-byte aligned
 *   (d_m is, and ld is even) are moved 16 bytes a lane, others 8; the two
 *   forms sum in different orders.  n <= INT32_MAX.  A NULL pointer, n < 1,
 *   ld < n, an epsilon that is not positive and finite: RMSF_EINVAL.
 * rmsf_block_scale_rows:  d_c[r * ldc + c] = d_s[r] d_a[r * lda + c] for r < n,
 *   c < nc <= 48: C = diag(s) A for a block of the eigen-solver, one multiply
 *   an element.  d_c may be d_a.  A NULL pointer, a size < 1, more than 48
 *   columns, lda or ldc < nc: RMSF_EINVAL.                                    */
int rmsf_diffusion_kernel(double *d_m, int64_t ld, int64_t n, double epsilon,
                          double *d_rowsum, void *stream);
int rmsf_block_scale_rows(const double *d_s, const double *d_a, int64_t lda,
                          int64_t n, int64_t nc, double *d_c, int64_t ldc,
                          void *stream);

/* ---- all-pairs RMSD matrix (MDAnalysis.analysis.diffusionmap.DistanceMatrix)
 * The n_frames x n_frames matrix of RMSDs between every pair of frames of a
 * batch read at a constant frame_stride, on the f64 matrix cores
 * (csrc/pairwise.hip): the covariance contraction turned on its side -- over
 * the atoms, the frames' coordinates as rows.  For frames i, j
 *   A_ij = sum_a w_a (x_i,a - c_i) (x_j,a - c_j)^T   (qcprot's inner product),
 *   G_f  = sum_a w_a |x_f,a - c_f|^2,  E0 = (G_i + G_j) / 2,
 * atom a = d_sel[a] (or a when d_sel is NULL; rows only), w = d_weights (NULL:
 * unit weights), x = f64 of the atom's three floats.
 * rmsf_pairwise_centres writes every frame's weighted centre c_f
 * (d_centre[n_frames][3]) and G_f (d_g[n_frames]); per_frame = 0 gives every
 * frame the centre of frame 0 -- a common shift for the metric without
 * superposition, which does not depend on it (conditioning only).  Fixed
 * summation order, no floating-point atomics.
 * rmsf_pairwise_rmsd, from those, for every pair j > i:
 *   superpose = 1: lambda = the largest root of the QCP quartic of A_ij by
 *     Newton's iteration from E0 (the coefficients, start and stopping rule of
 *     RMSF.py:48's qcprot, no rotation), d = sqrt(|2 (E0 - lambda)| / w_total)
 *     -- the minimal RMSD of MDAnalysis.analysis.rms.rmsd(superposition=True);
 *   superpose = 0: d = sqrt(|G_i + G_j - 2 tr A_ij| / w_total), the plain RMSD;
 *   d <= cutoff is written as 0; d_out[i * ld + j] = d_out[j * ld + i] = d (one
 *   value, stored twice: symmetric in its bits), the diagonal exactly 0.
 * w_total = sum_a w_a (n_sel without weights), ld >= n_frames doubles a row.
 * Work is cut into (pair of 16-frame tiles J >= I, atom range) workgroups;
 * with more than one atom range (few frames, many atoms) the partial A_ij go
 * to d_work (rmsf_pairwise_workspace_bytes() bytes, 0 when none is needed and
 * d_work may be NULL) and are summed in atom order by a second launch.  The
 * plan is a function of (n_frames, n_sel) alone: the same bits for the same
 * inputs.                                                                    */
int rmsf_pairwise_centres(const float *d_xyz, int64_t frame_stride,
                          int64_t n_frames, int64_t n_sel, const int32_t *d_sel,
                          const double *d_weights, int per_frame,
                          double *d_centre, double *d_g, void *stream);
size_t rmsf_pairwise_workspace_bytes(int64_t n_frames, int64_t n_sel);
int rmsf_pairwise_rmsd(const float *d_xyz, int64_t frame_stride,
                       int64_t n_frames, int64_t n_sel, const int32_t *d_sel,
                       const double *d_weights, double w_total,
                       const double *d_centre, const double *d_g, int superpose,
                       double cutoff, double *d_out, int64_t ld, void *d_work,
                       size_t work_bytes, void *stream);

/* ---- cross RMSD matrix: every frame of A against every frame of B ----------
 * d_out[i * ld + j] = the RMSD of frame i of A (n_a frames at d_a + i *
 * stride_a) and frame j of B (n_b frames at d_b + j * stride_b), ld >= n_b:
 * the contraction, the epilogue and the cutoff of rmsf_pairwise_rmsd over the
 * whole n_a x n_b rectangle, each pair once, one store a pair, nothing
 * mirrored and no diagonal.  Each side has its own selection of n_sel atoms
 * (d_sel_a, d_sel_b; NULL: atoms 0..n_sel-1), stride, centres and G; atom k of
 * one selection is paired with atom k of the other and weighs d_weights[k]
 * (NULL: 1), w_total = their sum.
 * Centres and G of a side: rmsf_pairwise_centres(per_frame = 1) for
 * superpose = 1.  superpose = 0 needs one common shift for both sides (tr A_ij
 * and the G are taken about it): rmsf_pairwise_centres(per_frame = 0) for A,
 * then rmsf_pairwise_centres_about for B with d_about = A's first centre
 * (three doubles in device memory), which gives every frame that centre and G
 * about it.
 * Work is cut into (tile I of A, tile J of B, atom range) workgroups of 16 x
 * 16 frames; with more than one atom range the partials go to d_work
 * (rmsf_cross_workspace_bytes() bytes, 0 when none is needed) and are summed
 * in atom order by a second launch.  The plan is a function of (n_a, n_b,
 * n_sel) alone, there are no floating-point atomics: the same bits for the
 * same inputs.  More than INT32_MAX tile pairs are refused.
 * rmsf_row_argmin: of every row of d_m[n_rows][ld] (n_cols >= 1 entries), the
 * least entry (d_val[n_rows], may be NULL) and the lowest column holding it
 * (d_idx[n_rows], may be NULL) -- strict comparisons in a fixed order, so
 * equal minima (exact zeros below the cutoff, duplicated references) resolve
 * to the first.  A NaN is below every number, as for numpy.argmin: a row
 * that holds one returns its first NaN's column and that NaN.
 * The lambda of a pair (superpose = 1): Newton's iteration on the QCP
 * quartic from E0, as qcprot's; where it has not met its stopping rule or
 * the quartic's slope there is below lambda^3 / 16 -- a double or nearly
 * double largest root: collinear, planar or collapsed frames, reflections of
 * symmetric structures -- the largest eigenvalue of the 4 x 4 key matrix by
 * cyclic Jacobi instead.  d^2 is then
 * within 1e-12 (G_i + G_j) / (2 w_total) of the exact value for every pair.
 * A non-finite coordinate makes its own frame's row and column NaN and
 * changes no other entry.                                                   */
int rmsf_pairwise_centres_about(const float *d_xyz, int64_t frame_stride,
                                int64_t n_frames, int64_t n_sel,
                                const int32_t *d_sel, const double *d_weights,
                                const double *d_about, double *d_centre,
                                double *d_g, void *stream);
size_t rmsf_cross_workspace_bytes(int64_t n_a, int64_t n_b, int64_t n_sel);
int rmsf_cross_rmsd(const float *d_a, int64_t stride_a, int64_t n_a,
                    const int32_t *d_sel_a, const double *d_centre_a,
                    const double *d_g_a, const float *d_b, int64_t stride_b,
                    int64_t n_b, const int32_t *d_sel_b,
                    const double *d_centre_b, const double *d_g_b,
                    int64_t n_sel, const double *d_weights, double w_total,
                    int superpose, double cutoff, double *d_out, int64_t ld,
                    void *d_work, size_t work_bytes, void *stream);
int rmsf_row_argmin(const double *d_m, int64_t n_rows, int64_t n_cols,
                    int64_t ld, int64_t *d_idx, double *d_val, void *stream);

/* The epilogue's lambda on the host, the device's own code (no device is
 * touched): for each of n pairs, h_A[9 k..] (row-major A_ij) and h_E0[k] give
 * h_lambda[k] and, when h_path is not NULL, the RMSF_PAIR_* way it was found
 * in h_path[k].                                                             */
int rmsf_pair_lambda_host(const double *h_A, const double *h_E0, int64_t n,
                          double *h_lambda, int32_t *h_path);

/* ---- GROMOS clustering of a symmetric distance matrix (Daura et al. 1999) ---
 * The definition, the same for the device entries and rmsf_cluster_gromos_host:
 *   adj(i, j) = (d[i, j] <= cutoff) for i != j, and adj(i, i) = 1 whatever the
 *   diagonal holds.  A NaN is never a neighbour (a frame with a non-finite
 *   coordinate has a NaN row and column and ends as a cluster of its own).
 *   count[i] = the number of set bits of row i.  While any frame is active:
 *   the centre is the active frame with the largest count -- among equal
 *   counts the lowest index --, its members adj(centre, .) & active get the
 *   next cluster id (0, 1, ...) and become inactive, and every frame still
 *   active loses |adj(i, .) & members| from its count.  Every step removes at
 *   least its centre, so there are at most n clusters, their sizes do not
 *   increase, and a cluster's size is its centre's count when it was picked.
 *   Integers only after the threshold: the same result on every run.
 * rmsf_adjacency_words(n): the 64-bit words of a row of n bits, (n + 63) / 64
 *   (0 for n <= 0).
 * rmsf_adjacency_pack: d_m[n][ld] f64 (ld >= n; columns >= n are not read, the
 *   matrix is read once) -> d_adj[n][ldw] (ldw >= rmsf_adjacency_words(n)):
 *   bit j & 63 of word j / 64 of row i is adj(i, j); the bits j >= n of the
 *   last word are 0 and the words past it are not touched.  d_count[n] (int32)
 *   receives the rows' counts.  cutoff >= 0 (a NaN is refused).
 * rmsf_cluster_gromos: the loop on d_adj (symmetric, as the pack of a
 *   symmetric matrix is) and d_count (read, not changed: the working copy
 *   lives in d_work, rmsf_cluster_gromos_workspace_bytes(n) bytes, a function
 *   of n alone).  d_label[n]: the cluster of each frame; d_centre / d_size
 *   [n], of which the first *h_n_clusters are written: each cluster's centre
 *   and size (all int32, device).  Two launches a cluster (pick and assign;
 *   decrement, which walks the members' rows: n^2 / 8 bytes over the whole
 *   run), enqueued 32 clusters at a time; once the largest count is 1 the
 *   remaining frames are labelled as singletons in index order by one launch.
 *   After each batch the call reads one state word back -- its only host
 *   synchronisation -- and it returns after the last such read: the stream is
 *   idle and *h_n_clusters (host) is set when it does.
 * rmsf_cluster_gromos_host: the same definition in plain C++ on a host matrix
 *   h_m[n][ld]; touches no device; all outputs are host pointers.
 * rmsf_adjacency_count: d_count[i] = the set bits of the rmsf_adjacency_words(n)
 *   words of row i of d_adj[n][ldw] (words past them are not read): one
 *   wavefront a row, a fixed order, no atomics, the bits read once.
 * rmsf_pairwise_adjacency: the bits rmsf_pairwise_rmsd (cutoff = zero_cutoff)
 *   followed by rmsf_adjacency_pack (cutoff) would give, word for word,
 *   without the n_frames^2 f64 matrix between them: the inputs, the plan, the
 *   workspace (rmsf_pairwise_workspace_bytes) and the distance of every pair
 *   are rmsf_pairwise_rmsd's, and each 16 x 16 tile of pairs stores, in place
 *   of its distances, the 16-bit segments of its rows (and of its mirror's) --
 *   plain 2-byte stores to different quarters of the 64-bit words, no atomics.
 *   Rows >= n_frames and words past rmsf_adjacency_words(n_frames) are not
 *   touched, the bits j >= n_frames of the last word are 0.  d_count may be
 *   NULL; otherwise rmsf_adjacency_count runs after.  cutoff >= 0 (a NaN is
 *   refused), ldw >= rmsf_adjacency_words(n_frames); more than INT32_MAX tile
 *   pairs (n_frames above about 1,048,000) are refused, as everything else is,
 *   before any launch.
 * n must be in 1..INT32_MAX.                                                 */
int64_t rmsf_adjacency_words(int64_t n);
int rmsf_adjacency_pack(const double *d_m, int64_t n, int64_t ld, double cutoff,
                        uint64_t *d_adj, int64_t ldw, int32_t *d_count,
                        void *stream);
size_t rmsf_cluster_gromos_workspace_bytes(int64_t n);
int rmsf_cluster_gromos(const uint64_t *d_adj, int64_t n, int64_t ldw,
                        const int32_t *d_count, int32_t *d_label,
                        int32_t *d_centre, int32_t *d_size,
                        int32_t *h_n_clusters, void *d_work, size_t work_bytes,
                        void *stream);
int rmsf_cluster_gromos_host(const double *h_m, int64_t n, int64_t ld,
                             double cutoff, int32_t *h_label, int32_t *h_centre,
                             int32_t *h_size, int32_t *h_n_clusters);
int rmsf_adjacency_count(const uint64_t *d_adj, int64_t n, int64_t ldw,
                         int32_t *d_count, void *stream);
int rmsf_pairwise_adjacency(const float *d_xyz, int64_t frame_stride,
                            int64_t n_frames, int64_t n_sel,
                            const int32_t *d_sel, const double *d_weights,
                            double w_total, const double *d_centre,
                            const double *d_g, int superpose,
                            double zero_cutoff, double cutoff, uint64_t *d_adj,
                            int64_t ldw, int32_t *d_count, void *d_work,
                            size_t work_bytes, void *stream);

/* ---- DBSCAN on the neighbour bits (Ester et al. 1996) -----------------------
 * scikit-learn's definition (sklearn.cluster.DBSCAN, metric="precomputed"),
 * restated so that it needs no visiting order; the same for the device entry,
 * rmsf_cluster_dbscan_host and the tests' numpy reference:
 *   adj and count are those of the GROMOS section above (diagonal set, a NaN
 *   never a neighbour).  core[i] = (count[i] >= min_samples).  The clusters are
 *   the connected components of adj restricted to core x core; a cluster's id
 *   is the rank of its lowest core index among all clusters' lowest core
 *   indices.  A non-core row with at least one core neighbour is a border row
 *   and takes the lowest cluster id among its core neighbours' clusters (not
 *   the cluster of its lowest-indexed core neighbour).  Every other row is
 *   noise, -1.  min_samples = 1 is single linkage at the cutoff.  Integers
 *   only: the same result on every run.
 * rmsf_cluster_dbscan: on d_adj[n][ldw] (symmetric) and d_count[n], both read
 *   and not changed.  d_label[n] (int32) receives the labels, d_core
 *   [rmsf_adjacency_words(n)] (uint64) the core bits (bits >= n are 0), and the
 *   host words *h_n_clusters and *h_n_rounds the number of clusters and of
 *   rounds.  The components are found by min-hooking with shortcutting (the
 *   FastSV family): a parent array f starts as the identity; a round gives
 *   every core row the minimum grandparent f[f[j]] over its core neighbours j,
 *   hooks it onto the row's parent and onto the row (integer atomicMin into
 *   the next round's array: the minimum of a set, whatever the order) and so
 *   shortcuts f[i] to f[f[i]]; each round reads the core rows once, n^2 / 8
 *   bytes at the most.  Two launches a round, enqueued 4 rounds at a time;
 *   after each batch the call reads one state word back, and it stops after
 *   the first round that changes nothing: *h_n_rounds counts that round too.
 *   More than n + 1 rounds is RMSF_EHIP and no labels (a guard only: after t
 *   rounds f[i] is at most what plain min-propagation has after t, and that
 *   settles within the graph's diameter, below n).
 *   Then the roots' ranks (one workgroup's popcount scan) and the labels, one
 *   wavefront a row.  The stream is idle when the call returns.  d_work:
 *   rmsf_cluster_dbscan_workspace_bytes(n) bytes, a function of n alone, O(n)
 *   (0 for n outside 1..INT32_MAX); NULL or too small is RMSF_ENOMEM.
 * rmsf_cluster_dbscan_host: the same definition in plain C++ on a host matrix
 *   h_m[n][ld] thresholded at cutoff (>= 0; a NaN is refused); touches no
 *   device; h_label[n], h_core[rmsf_adjacency_words(n)] and *h_n_clusters are
 *   host pointers.
 * n in 1..INT32_MAX, min_samples >= 1; every check comes before any launch.  */
size_t rmsf_cluster_dbscan_workspace_bytes(int64_t n);
int rmsf_cluster_dbscan(const uint64_t *d_adj, int64_t n, int64_t ldw,
                        const int32_t *d_count, int64_t min_samples,
                        int32_t *d_label, uint64_t *d_core,
                        int32_t *h_n_clusters, int32_t *h_n_rounds,
                        void *d_work, size_t work_bytes, void *stream);
int rmsf_cluster_dbscan_host(const double *h_m, int64_t n, int64_t ld,
                             double cutoff, int64_t min_samples,
                             int32_t *h_label, uint64_t *h_core,
                             int32_t *h_n_clusters);

/* ---- contacts: distances between atoms within a frame (csrc/contacts.hip) ---
 * One rule everywhere.  Coordinates are f32 as stored;
 *   dx = (double)xa - (double)xb, dy and dz likewise,
 *   d2 = (dx*dx + dy*dy) + dz*dz with no FMA, d = sqrt(d2) correctly rounded,
 * and a pair is in contact iff d <= radius.  A NaN is never a contact, so an
 * atom with a non-finite coordinate in a frame loses its pairs in that frame
 * and nothing else changes.  No periodic images: these entries take no box
 * (the rdf section below does).
 * rmsf_contact_threshold_sq(radius): the largest double t with sqrt(t) <=
 *   radius (NaN unless radius is positive and finite).  sqrt is monotone, so
 *   d2 <= t is the same predicate and the device entries take no root a pair.
 * Frames are d_xyz + f * frame_stride floats, f < n_frames, each holding
 * n_atoms rows of 3 floats (frame_stride >= 3 n_atoms).  An index array names
 * rows of a frame, NULL the rows 0..n-1.  Every index array has a device copy
 * the kernels read and a host copy h_* the call checks against its bound
 * before any launch (NULL: the caller vouches for it).
 * rmsf_contact_counts: d_counts[i][j] (int32 [n_a][ld], ld >= n_b; columns at
 *   or past n_b are not written) = the number of frames in which rows a_i and
 *   b_j are in contact.  symmetric != 0: A is B (n_a == n_b, d_idx_a ==
 *   d_idx_b); only tiles on or above the diagonal are computed, each mirrored,
 *   the diagonal like any other entry.  A workgroup owns a tile of pairs and a
 *   run of frames staged through LDS a chunk at a time; where the tiles are
 *   few the frames are split across workgroups and the splits meet in
 *   d_counts by integer atomicAdd after one zeroing launch -- exact in any
 *   order, the same bytes every run.  rmsf_contact_counts_plan reports what
 *   the launcher chooses: the tile's edges, the frame chunk and the number of
 *   splits (host only).  rmsf_contact_counts_workspace_bytes is what d_work
 *   must hold: 0 as the splits are combined now, d_work may be NULL.
 * rmsf_contact_fraction: pairs p < n_pairs of rows[pair_a[p]] and
 *   rows[pair_b[p]], where d_rows[n_rows] are the frame's rows the pairs use
 *   (staged in LDS once a frame where they fit) and pair_a / pair_b positions
 *   in it.  d_n_contacts[f] (int32) = the pairs in contact at radius in frame
 *   f, and d_q[f] (f64) by method:
 *     RMSF_CONTACT_HARD_CUT, RMSF_CONTACT_RADIUS_CUT  n_contacts / n_pairs,
 *       one f64 division; d_r0 is not read;
 *     RMSF_CONTACT_SOFT_CUT  (sum over p of 1 / (1 + exp(beta * (d -
 *       lambda_constant * r0[p])))) / n_pairs, the argument formed as written;
 *       each lane sums its pairs in order and the lanes are summed by a fixed
 *       tree: the same bits every run.
 * The _host entries are the definition in plain C++ on host pointers (sqrt a
 * pair, soft_cut summed in pair order) and touch no device.
 * RMSF_EINVAL before any launch: n_pairs < 1, an index out of range, a radius
 * that is not positive and finite, an unknown method, a NULL or a size out of
 * range (frames, rows and pairs up to INT32_MAX).                            */
#define RMSF_CONTACT_HARD_CUT 0
#define RMSF_CONTACT_RADIUS_CUT 1
#define RMSF_CONTACT_SOFT_CUT 2
double rmsf_contact_threshold_sq(double radius);
int rmsf_contact_counts_plan(int64_t n_a, int64_t n_b, int64_t n_frames,
                             int symmetric, int32_t *tile_a, int32_t *tile_b,
                             int32_t *frame_chunk, int32_t *n_splits);
size_t rmsf_contact_counts_workspace_bytes(int64_t n_a, int64_t n_b,
                                           int64_t n_frames, int symmetric);
int rmsf_contact_counts(const float *d_xyz, int64_t frame_stride,
                        int64_t n_frames, int64_t n_atoms,
                        const int32_t *d_idx_a, const int32_t *h_idx_a,
                        int64_t n_a, const int32_t *d_idx_b,
                        const int32_t *h_idx_b, int64_t n_b, int symmetric,
                        double radius, int32_t *d_counts, int64_t ld,
                        void *d_work, size_t work_bytes, void *stream);
int rmsf_contact_counts_host(const float *h_xyz, int64_t frame_stride,
                             int64_t n_frames, int64_t n_atoms,
                             const int32_t *h_idx_a, int64_t n_a,
                             const int32_t *h_idx_b, int64_t n_b, double radius,
                             int32_t *h_counts, int64_t ld);
int rmsf_contact_fraction(const float *d_xyz, int64_t frame_stride,
                          int64_t n_frames, int64_t n_atoms, int64_t n_rows,
                          const int32_t *d_rows, const int32_t *h_rows,
                          const int32_t *d_pair_a, const int32_t *d_pair_b,
                          const int32_t *h_pair_a, const int32_t *h_pair_b,
                          const double *d_r0, int64_t n_pairs, double radius,
                          int method, double beta, double lambda_constant,
                          double *d_q, int32_t *d_n_contacts, void *stream);
int rmsf_contact_fraction_host(const float *h_xyz, int64_t frame_stride,
                               int64_t n_frames, int64_t n_atoms,
                               int64_t n_rows, const int32_t *h_rows,
                               const int32_t *h_pair_a, const int32_t *h_pair_b,
                               const double *h_r0, int64_t n_pairs,
                               double radius, int method, double beta,
                               double lambda_constant, double *h_q,
                               int32_t *h_n_contacts);

/* ---- radial distribution function: a histogram of pair distances, free or
 * under the minimum image (csrc/rdf.hip, csrc/pair_image.h) ------------------
 * One rule everywhere.  Coordinates are f32 as stored, no FMA anywhere;
 *   dx = (double)xa - (double)xb, dy and dz likewise,
 *   periodic: dx = dx - Lx * rint(dx * ix), ix = 1.0 / Lx formed once a frame
 *     on the host; rint rounds half to even (numpy.rint's bits),
 *   d2 = (dx*dx + dy*dy) + dz*dz, d = sqrt(d2) correctly rounded,
 *   edges e_k = k * ((rmax - rmin) / nbins) + rmin for k < nbins, e_nbins = rmax
 *     (numpy.linspace(rmin, rmax, nbins + 1)'s bits),
 *   bin k iff e_k <= d < e_(k+1); the last bin also takes d == rmax; a NaN is
 *     in no bin (numpy.histogram(d, bins=nbins, range=(rmin, rmax))'s counts).
 * rmsf_rdf_edges: h_edges[nbins + 1] as above and h_thresholds_sq[nbins + 1],
 *   the same predicate on d2 (either may be NULL; host only): T_k for k < nbins
 *   is the smallest double whose correctly rounded root is >= e_k, T_nbins the
 *   first double above the largest whose root is <= rmax, and bin k is
 *   T_k <= d2 < T_(k+1).  The device compares d2 and takes no f64 root a pair.
 * rmsf_rdf_counts: d_counts[k] (int64 [nbins]; nothing past nbins is written)
 *   = the pairs (i, j, frame), i < n_a, j < n_b, whose distance is in bin k.
 *   Frames, strides and index arrays as rmsf_contact_counts takes them.
 *   symmetric != 0: A against itself (n_a == n_b, d_idx_a == d_idx_b): the
 *   ordered pairs i != j; only tiles on or above the diagonal run, each
 *   unordered pair adds 2, and the entry (i, i) is never counted.
 *   excl_a, excl_b (0, 0: none): the pair (i, j) is skipped when i / excl_a ==
 *   j / excl_b -- positions in the two sides, blocks of excl_a and excl_b of
 *   them (upstream's exclusion_block); each must divide its side, and on the
 *   symmetric route they are equal.
 *   d_box / h_box (f64 [n_frames][6] = Lx, Ly, Lz, 1/Lx, 1/Ly, 1/Lz; the
 *   device copy the kernel reads and the host copy the call checks; both NULL:
 *   free space, with no image term compiled in).  Orthorhombic boxes only.
 *   d_work: rmsf_rdf_counts_workspace_bytes(nbins) bytes, for the thresholds.
 *   A workgroup owns a 64 x 64 tile of pairs and a run of frames staged
 *   through LDS, and keeps int32 counters in LDS that it adds to the int64
 *   bins by integer atomicAdd after one zeroing; a run of frames is short
 *   enough that no int32 counter can wrap.  Integer sums: the same bytes
 *   every run.  rmsf_rdf_counts_plan reports the tile's edges, the frame chunk
 *   and the number of splits of the frames (host only).
 * rmsf_rdf_counts_host: the definition in plain C++ on host pointers, a sqrt
 *   a pair and a search of the edges; touches no device.
 * RMSF_EINVAL before any launch: nbins outside 1..2048; rmin < 0, rmax <=
 *   rmin or either non-finite; a box edge that is not positive and finite;
 *   h_box[3 + k] != 1.0 / h_box[k]; rmax over half a box edge of any frame
 *   (the minimum image is then not the only image in range); an index out of
 *   range; symmetric with n_a != n_b; an exclusion block that does not divide
 *   its side; a NULL or a size out of range.                                 */
int rmsf_rdf_edges(double rmin, double rmax, int32_t nbins, double *h_edges,
                   double *h_thresholds_sq);
int rmsf_rdf_counts_plan(int64_t n_a, int64_t n_b, int64_t n_frames,
                         int symmetric, int32_t *tile_a, int32_t *tile_b,
                         int32_t *frame_chunk, int32_t *n_splits);
size_t rmsf_rdf_counts_workspace_bytes(int32_t nbins);
int rmsf_rdf_counts(const float *d_xyz, int64_t frame_stride, int64_t n_frames,
                    int64_t n_atoms, const int32_t *d_idx_a,
                    const int32_t *h_idx_a, int64_t n_a, const int32_t *d_idx_b,
                    const int32_t *h_idx_b, int64_t n_b, int symmetric,
                    int64_t excl_a, int64_t excl_b, const double *d_box,
                    const double *h_box, double rmin, double rmax,
                    int32_t nbins, int64_t *d_counts, void *d_work,
                    size_t work_bytes, void *stream);
int rmsf_rdf_counts_host(const float *h_xyz, int64_t frame_stride,
                         int64_t n_frames, int64_t n_atoms,
                         const int32_t *h_idx_a, int64_t n_a,
                         const int32_t *h_idx_b, int64_t n_b, int symmetric,
                         int64_t excl_a, int64_t excl_b, const double *h_box,
                         double rmin, double rmax, int32_t nbins,
                         int64_t *h_counts);

/* ---- mean squared displacement: every atom at every lag, with the "nojump"
 * unwrap (csrc/msd.hip, csrc/pair_image.h) ------------------------------------
 * One rule everywhere, host and device, all f64, no FMA anywhere.  Frames are
 * positions k = 0..F-1 of the run; a lag counts positions.
 *   coordinates: f32 as stored, widened: (double)x_c(k);
 *   free:    u_c(k) = (double)x_c(k);
 *   nojump:  u_c(0) = (double)x_c(0),
 *            u_c(k) = u_c(k-1) + image((double)x_c(k) - (double)x_c(k-1)),
 *            image(d) = d - L_c(k) * rint(d * i_c(k)) with the box of frame k,
 *            i = 1.0 / L formed on the host, rint half to even (numpy.rint's
 *            bits): one in-order add chain an atom-coordinate, all three
 *            coordinates whatever the mask.  A non-finite coordinate at frame
 *            k makes that chain NaN from k on and touches nothing else;
 *   term:    d(a,t,tau) = (dx*dx + dy*dy) + dz*dz, dc = u_c(t+tau) - u_c(t);
 *            dims_mask (bit 0 x, bit 1 y, bit 2 z; 1..7) names the
 *            coordinates, the others are left out of the expression (not
 *            multiplied by zero): dx*dx + dz*dz, dy*dy, ...;
 *   sum:     S(a,tau) = sum over t = 0..F-tau-1 of d(a,t,tau), in a fixed
 *            order of the kernel's choosing, no float atomics, the same bytes
 *            every run; msd(a,tau) = S(a,tau) / (double)(F - tau), one
 *            division.  The terms are not negative, so any order of the N =
 *            F - tau terms is within (N - 1) 2^-53 relative of the exact sum
 *            and msd within (N + 8) 2^-53 of the exact quotient; msd(a,0) is
 *            0.0 exactly for a finite atom;
 *   mean:    mean(tau) = (sum over a of msd(a,tau)) / (double)n_sel, summed in
 *            a fixed order, within (n_sel + 8) 2^-53 relative of the exact
 *            mean of the values summed; a NaN propagates;
 *   lags:    tau = 0..n_lags-1, 1 <= n_lags <= F.
 * rmsf_msd_plane_ld(n_frames): the leading dimension the planes should have
 *   (>= n_frames; 0 for a size out of range).
 * rmsf_msd_planes: d_planes (f64 [n_sel][3][ld], ld >= n_frames) = u_c(k) of
 *   the rows d_idx names (frames, strides and the index array as
 *   rmsf_contact_counts takes them), atom-major from frame-major rows through
 *   an LDS transpose.  d_box / h_box (f64 [n_frames][6] = Lx, Ly, Lz, 1/Lx,
 *   1/Ly, 1/Lz; the device copy the kernel reads and the host copy the call
 *   checks): nojump; both NULL: free.  Columns n_frames..ld-1 are written 0.0
 *   and nothing past [n_sel][3][ld] is written.
 * rmsf_msd_lags: d_msd (f64 [n_lags][ld_out], ld_out >= n_sel; columns at or
 *   past n_sel are not written) = msd(a,tau), and d_mean (f64 [n_lags], or
 *   NULL to skip it) = mean(tau).  A workgroup owns an atom, a block of lags
 *   and a run of origins staged through LDS; where atoms times lag blocks are
 *   few the origins are split across workgroups, the partial sums go through
 *   d_work (rmsf_msd_workspace_bytes; 0 with no split, d_work may then be
 *   NULL) and a second launch adds them in split order.  rmsf_msd_plan reports
 *   what the launcher chooses: the lags a workgroup, the origins staged at a
 *   time and the number of splits (host only).
 * The _host entries are the definition in plain C++ on host pointers, summed
 * in order of t (the mean in order of a), and touch no device.
 * RMSF_EINVAL before any launch: n_lags outside 1..n_frames; a mask outside
 *   1..7; a box edge that is not positive and finite; h_box[3 + k] != 1.0 /
 *   h_box[k]; exactly one of d_box / h_box NULL; an index out of range; ld <
 *   n_frames; ld_out < n_sel; a workspace too small; a NULL or a size out of
 *   range (frames up to 4,194,240, rows up to INT32_MAX / 3).               */
int64_t rmsf_msd_plane_ld(int64_t n_frames);
int rmsf_msd_plan(int64_t n_sel, int64_t n_frames, int64_t n_lags,
                  int32_t *lag_block, int32_t *origin_chunk, int32_t *n_splits);
size_t rmsf_msd_workspace_bytes(int64_t n_sel, int64_t n_frames,
                                int64_t n_lags);
int rmsf_msd_planes(const float *d_xyz, int64_t frame_stride, int64_t n_frames,
                    int64_t n_atoms, const int32_t *d_idx, const int32_t *h_idx,
                    int64_t n_sel, const double *d_box, const double *h_box,
                    double *d_planes, int64_t ld, void *stream);
int rmsf_msd_lags(const double *d_planes, int64_t ld, int64_t n_sel,
                  int64_t n_frames, int64_t n_lags, int dims_mask,
                  double *d_msd, int64_t ld_out, double *d_mean, void *d_work,
                  size_t work_bytes, void *stream);
int rmsf_msd_planes_host(const float *h_xyz, int64_t frame_stride,
                         int64_t n_frames, int64_t n_atoms,
                         const int32_t *h_idx, int64_t n_sel,
                         const double *h_box, double *h_planes, int64_t ld);
int rmsf_msd_lags_host(const double *h_planes, int64_t ld, int64_t n_sel,
                       int64_t n_frames, int64_t n_lags, int dims_mask,
                       double *h_msd, int64_t ld_out, double *h_mean);

/* ---- qcprot.CalcRMSDRotationalMatrix (RMSF.py:48) --------------------------
 * Batched QCP on device: A[n][9], E0[n], atom counts N[n] -> rot[n][9],
 * rmsd[n].  Exposed for the upstream known-answer test.                      */
int rmsf_qcp_batch(const double *d_A, const double *d_E0, const double *d_N,
                   int64_t n, double *d_rot, double *d_rmsd, void *stream);

/* Host-pointer form with the signature of
 * MDAnalysis.lib.qcprot.CalcRMSDRotationalMatrix(ref, conf, N, rot, weights)
 * (called at RMSF.py:48): ref/conf f64 [N][3] (already centred by the
 * caller), rot f64[9] out, weights NULL or f64[N].  Runs on the current
 * device, synchronous.  *rmsd_out receives the rmsd.                        */
int rmsf_calc_rmsd_rotational_matrix(const double *h_ref, const double *h_conf,
                                     int64_t N, double *h_rot,
                                     const double *h_weights,
                                     double *rmsd_out);

/* ---- scattered frames (RMSF.run(frames=...), RMSF.py:92,124 frame source) --
 * Compact batch d_dst[k][j][3] (k < n_frames <= 65535, j < n_sel) of the
 * frames at d_src + d_frames[k]*frame_stride (device int64 indices), the
 * selection d_sel (NULL = atoms 0..n_sel-1) gathered: one launch per batch
 * of a scattered frame list instead of kernel launches per frame.           */
int rmsf_gather_frames(const float *d_src, int64_t frame_stride,
                       const int64_t *d_frames, int64_t n_frames, int64_t n_sel,
                       const int32_t *d_sel, float *d_dst, void *stream);

/* The same compact batch from HBM-resident frames stored as coordinate
 * planes (SoA): frame k's x[n_atoms], y and z at d_src + d_frames[k] *
 * frame_stride + {0, 1, 2} * plane_stride floats (frame_stride >=
 * 3 * plane_stride).  The selection is gathered from each plane and
 * interleaved into d_dst's [n_frames][n_sel][3] rows for the kernels above
 * (an extra read and write of the selected bytes: a convenience path for
 * data that already lives in HBM as planes).                               */
int rmsf_gather_planes(const float *d_src, int64_t frame_stride,
                       int64_t plane_stride, const int64_t *d_frames,
                       int64_t n_frames, int64_t n_sel, const int32_t *d_sel,
                       float *d_dst, void *stream);

/* Per-coordinate f64 statistics in plane order (x[n], y[n], z[n]) to
 * (atom, xyz) order, d_dst[3a + c] = d_src[c*n + a] (d_dst != d_src): the
 * unaligned accumulate reads contiguous coordinate planes in place, as it
 * reads rows (its statistics are per coordinate), and its mean / M2 come
 * out in plane order.                                                      */
int rmsf_planes_to_rows(const double *d_src, int64_t n, double *d_dst,
                        void *stream);

/* ---- synthetic trajectories -------------------------------
 * out[f*frame_stride + 3*a + c] for frames [f0, f0+nf) of n_atoms atoms:
 *   base(a,c) ~ U[0,100), sigma(a) ~ U[0.2,2.0), g ~ triangular, unit var,
 *   p = base + sigma*g ; optional rigid motion from d_motion[f][12]
 *   (R[9] row-major, t[3]):  p' = ((p-50) @ R) + t ; out = f32(p').
 * Counter-based (splitmix64 of seed/frame/atom/axis) with every float op
 * explicitly rounded, so the CPU regenerates any slice bit-identically.     */
int rmsf_synth_frames(float *d_out, int64_t frame_stride, int64_t n_atoms,
                      int64_t f0, int64_t nf, uint64_t seed,
                      const double *d_motion, void *stream);
/* The generator's noise scale sigma(a) of atoms a0..a0+n-1 (f64, device):
 * an unaligned synthetic atom's population RMSF is sqrt(3) sigma(a) -- the
 * reference value of the bench's per-mode sanity figure.                    */
int rmsf_synth_sigma(double *d_sigma, int64_t a0, int64_t n, uint64_t seed,
                     void *stream);

/* ---- host -> device frame stager (north star subsystem 1) ---
 * Pinned-host, multi-buffered hipMemcpyAsync stager.  Frames arrive as host
 * float32 arrays of n_atoms_frame atoms; the selection (h_sel, NULL = first
 * n_sel atoms) is gathered on the host into a pinned slot by a thread pool,
 * the slot is copied on the stager's own copy stream, and the consumer
 * stream is made to wait on the copy event.  A slot is reused only after
 * the consumer released it (an event recorded on the consumer stream).     */
typedef struct rmsf_stager rmsf_stager;
int rmsf_stager_create(int64_t n_atoms_frame, int64_t n_sel,
                       const int32_t *h_sel, int64_t batch_frames,
                       int n_slots, int n_threads, rmsf_stager **out);
int rmsf_stager_destroy(rmsf_stager *st);
/* Stage n_frames (<= batch_frames) host frames (stride h_frame_stride
 * floats) into the next slot.  Returns the slot index and its device
 * pointer (compact [n_frames][n_sel][3] layout, frame_stride = 3*n_sel).
 * `consumer_stream` waits on the copy before any later work it runs.       */
int rmsf_stager_stage(rmsf_stager *st, const float *h_frames,
                      int64_t h_frame_stride, int64_t n_frames,
                      void *consumer_stream, int *slot, float **d_batch);
/* Stage frames given as an array of n_frames host pointers (one per frame,
 * each n_atoms_frame*3 floats) -- the per-Timestep MDAnalysis path.        */
int rmsf_stager_stage_ptrs(rmsf_stager *st, const float *const *h_frame_ptrs,
                           int64_t n_frames, void *consumer_stream, int *slot,
                           float **d_batch);
/* Stage frames stored as coordinate planes (SoA): frame f's x[n_atoms_frame],
 * y and z at h_frame_ptrs[f], + h_plane_stride and + 2*h_plane_stride floats
 * (h_plane_stride >= n_atoms_frame) -- a synthetic [F][3][n] array, or a DCD
 * frame's X/Y/Z records in place (RMSF.py:92,124's reader interleaves them
 * per frame).  The selection is gathered and interleaved on the host into
 * the same compact [n_frames][n_sel][3] device batch as rmsf_stager_stage().*/
int rmsf_stager_stage_planes(rmsf_stager *st, const float *const *h_frame_ptrs,
                             int64_t h_plane_stride, int64_t n_frames,
                             void *consumer_stream, int *slot, float **d_batch);
/* Decode XTC frames f0, f0+step, ... (n_frames of them) frame-parallel
 * straight into the next pinned slot (selection applied), then DMA it. */
typedef struct rmsf_xtc rmsf_xtc;
int rmsf_stager_stage_xtc(rmsf_stager *st, const rmsf_xtc *x, int64_t f0,
                          int64_t n_frames, int64_t step,
                          void *consumer_stream, int *slot, float **d_batch);
/* Mark the slot free once the work queued so far on consumer_stream ends. */
int rmsf_stager_release(rmsf_stager *st, int slot, void *consumer_stream);
/* Wait until every copy issued by the stager has completed. */
int rmsf_stager_synchronize(rmsf_stager *st);

/* ---- GROMACS XTC trajectories ---------------------------
 * Host reader/writer replacing libxdrfile behind MDAnalysis' XTCReader, the
 * frame source of RMSF.py:56,92,124 (GRO/XTC input, RMSF.py:34).  Published
 * xdrfile format (magic 1995, xdr3dfcoord compression).  Positions are in
 * Angstrom, rounded as MDAnalysis does: f32(f32(int * f32(1/prec)) * 10).
 * Host-only code: no HIP calls.                                             */
int rmsf_xtc_open(const char *path, rmsf_xtc **out, int64_t *n_atoms,
                  int64_t *n_frames);
int rmsf_xtc_close(rmsf_xtc *x);
int rmsf_xtc_frame_info(const rmsf_xtc *x, int64_t frame, int32_t *step,
                        float *time, float *box9);
/* Every frame's box as the file holds it: h_box9[n_frames][9], nm.          */
int rmsf_xtc_boxes(const rmsf_xtc *x, float *h_box9);
/* Decode frames f0, f0+step, ... (n) into h_out[n][rows][3] (rows = n_sel
 * when h_sel != NULL, else n_atoms), frame-parallel on n_threads threads. */
int rmsf_xtc_read(const rmsf_xtc *x, int64_t f0, int64_t n, int64_t step,
                  const int32_t *h_sel, int64_t n_sel, float *h_out,
                  int n_threads);
/* Write (append != 0: append) n_frames frames given in Angstrom. */
int rmsf_xtc_write(const char *path, const float *h_xyz, int64_t n_frames,
                   int64_t n_atoms, float precision, const float *h_box9,
                   int append);
/* Byte offset (a multiple of 4) and length of frame f's XDR record. */
int rmsf_xtc_frame_record(const rmsf_xtc *x, int64_t frame, int64_t *offset,
                          int64_t *bytes);

/* ---- XTC decompression on the GPU (config C5) -------------------------------
 * The same decoder on the device: the compressed frame records (about 1/6
 * of the decoded bytes) are read into a pinned slot (pread, n_threads host
 * threads), copied to HBM on the slot's own stream and decompressed there,
 * one wave per frame (the xdr3dfcoord stream of a frame is sequential;
 * frames run in parallel), into float32 [n][n_atoms][3] Angstrom frames,
 * bit-identical to rmsf_xtc_read().  Replaces the libxdrfile decode behind
 * trajectory[frame] (RMSF.py:92,124).
 * A decoder from rmsf_xtcdec_create writes every atom, and the selection is
 * applied downstream (rmsf_accumulate / rmsf_superpose gather it in-kernel).
 * One from rmsf_xtcdec_create_sel writes the selected atoms only: compact
 * float32 [n][n_sel][3] frames in the selection's order, rmsf_xtc_read(h_sel)'s
 * bits, ready for the kernels' contiguous path (d_sel = NULL).  Below,
 * "rows" is n_atoms for the former and n_sel for the latter.              */
typedef struct rmsf_xtcdec rmsf_xtcdec;
int rmsf_xtcdec_create(const rmsf_xtc *x, int64_t batch_frames, int n_slots,
                       int n_threads, rmsf_xtcdec **out);
/* A decoder of the atoms h_sel[0..n_sel) only (any order, each index once:
 * RMSF_EINVAL for a duplicate, which has no single output row, or an index
 * outside the file's atoms).  RMSF.py reads every atom of every frame and
 * keeps 214 CA atoms of 47,681 (RMSF.py:77,92,124,126); here the other
 * atoms are never written: the slots' frame buffers are
 * batch_frames * n_sel * 12 bytes.  The device map of the selection is
 * built once, on the current device.                                       */
int rmsf_xtcdec_create_sel(const rmsf_xtc *x, int64_t batch_frames,
                           int n_slots, int n_threads, const int32_t *h_sel,
                           int64_t n_sel, rmsf_xtcdec **out);
int rmsf_xtcdec_destroy(rmsf_xtcdec *d);
/* Decode frames f0, f0+step, ... (n_frames <= batch_frames) into the next
 * slot; *d_frames = its device frames (frame stride 3*rows floats).
 * consumer_stream waits for the decode.  Per-frame errors (corrupt data:
 * the frame is filled with NaN) are reported when the slot is next used or
 * by rmsf_xtcdec_synchronize().                                             */
int rmsf_xtcdec_decode(rmsf_xtcdec *d, int64_t f0, int64_t n_frames,
                       int64_t step, void *consumer_stream, int *slot,
                       float **d_frames);
/* Decode the n_frames frames h_frames[0..n) (any order, repeats allowed;
 * n_frames <= batch_frames) into the next slot, frame k of the list at
 * *d_frames + k*3*rows: a run(frames=...) list of scattered frames costs
 * one batched read + decode instead of one per frame.                      */
int rmsf_xtcdec_decode_list(rmsf_xtcdec *d, const int64_t *h_frames,
                            int64_t n_frames, void *consumer_stream, int *slot,
                            float **d_frames);
/* The same into the caller's device buffer: frame k of the batch at
 * d_out + k*out_stride floats, out_stride >= 3*rows (e.g. a trajectory kept
 * resident in HBM).                                                         */
int rmsf_xtcdec_decode_into(rmsf_xtcdec *d, int64_t f0, int64_t n_frames,
                            int64_t step, float *d_out, int64_t out_stride,
                            void *consumer_stream, int *slot);
/* The slot may be reused once the work queued so far on consumer_stream ends. */
int rmsf_xtcdec_release(rmsf_xtcdec *d, int slot, void *consumer_stream);
/* Wait for every outstanding decode; first per-frame error, if any. */
int rmsf_xtcdec_synchronize(rmsf_xtcdec *d);
/* Kernel level: decode n_frames XDR frame records (each starting at its
 * magic word) held in device memory at 32-bit word offsets d_rec_off with
 * lengths d_rec_len (words); d_status[f] = 0 or a per-frame error code.   */
int rmsf_xtc_decode_records(const void *d_records, const int64_t *d_rec_off,
                            const int64_t *d_rec_len, int64_t n_frames,
                            int64_t n_atoms, float *d_out, int64_t out_stride,
                            int32_t *d_status, void *stream);
/* The device decoder's code run on the host (tests; no HIP calls). */
int rmsf_xtc_decode_records_host(const void *h_records,
                                 const int64_t *h_rec_off,
                                 const int64_t *h_rec_len, int64_t n_frames,
                                 int64_t n_atoms, float *h_out,
                                 int64_t out_stride, int32_t *h_status);
/* Kernel level, selected atoms only (the positions RMSF.py:92,124 read and
 * RMSF.py:77,126 then cut down to the CA atoms): d_row_of_atom[n_atoms] holds
 * each atom's output row in [0, n_sel), or -1; frame f's selected atoms go
 * to d_out + f*out_stride + 3*row (out_stride >= 3*n_sel) and nothing else
 * is written.  A corrupt frame's n_sel rows are filled with NaN.  The map
 * is trusted (as the record table is): every row must be < n_sel.         */
int rmsf_xtc_decode_records_sel(const void *d_records,
                                const int64_t *d_rec_off,
                                const int64_t *d_rec_len, int64_t n_frames,
                                int64_t n_atoms, const int32_t *d_row_of_atom,
                                int64_t n_sel, float *d_out,
                                int64_t out_stride, int32_t *d_status,
                                void *stream);
/* The same code run on the host (the CPU tier of the tests; no HIP calls:
 * what RMSF.py:77,92,124,126 keep of a frame, without a device).  Checks
 * the map's entries.                                                       */
int rmsf_xtc_decode_records_sel_host(const void *h_records,
                                     const int64_t *h_rec_off,
                                     const int64_t *h_rec_len,
                                     int64_t n_frames, int64_t n_atoms,
                                     const int32_t *h_row_of_atom,
                                     int64_t n_sel, float *h_out,
                                     int64_t out_stride, int32_t *h_status);

/* ---- RMSF context: the whole per-rank loop behind one opaque handle -------
 * SURVEY.md 8(b)'s minimal export set, for hosts that bring neither torch
 * nor their own device allocator (a C/C++ program, an MPI code, ctypes).
 * A context owns, on one device: the selection and masses, the centred
 * reference, the running Welford (n, mean, M2) and sweep-1 sum partials,
 * workspaces, a host stager and a non-blocking stream.  Calls on one context
 * are not re-entrant; different contexts may be driven from different host
 * threads.  Every call makes the context's device current for its duration
 * and restores the caller's device.  Work is asynchronous on the context
 * stream; rmsf_get_* synchronise.
 *
 * RMSF.py's per-rank loop (RMSF.py:80-146) in these terms:
 *   rmsf_ctx_create(dev, n_atoms, n_sel, ca_indices, masses, 0, &c);
 *   rmsf_set_reference_frame(c, frame0, is_dev);            RMSF.py:80-87
 *   rmsf_push_frames(c, block, n, 0, RMSF_PUSH_ALIGN_SUM, is_dev);  :89-105
 *   rmsf_multi_allreduce_sum(&c, 1)   (or the callback form)  :107-110
 *   rmsf_set_reference_average(c);                           :111-118
 *   rmsf_push_frames(c, block, n, 0, RMSF_PUSH_ALIGN_WELFORD, is_dev); :120-138
 *   rmsf_multi_chan_merge(&c, 1)      (or the callback form)  :140-143
 *   rmsf_get_rmsf(c, h_rmsf);                                 :145-146    */
typedef struct rmsf_ctx rmsf_ctx;

/* push modes for rmsf_push_frames() / rmsf_push_xtc() */
#define RMSF_PUSH_WELFORD 0       /* Welford on the raw frames (rms.RMSF)     */
#define RMSF_PUSH_ALIGN_SUM 1     /* superpose, f64 sum      (RMSF.py:91-105) */
#define RMSF_PUSH_ALIGN_WELFORD 2 /* superpose, Welford      (RMSF.py:123-138)*/
#define RMSF_PUSH_SUM 3           /* f64 sum of the raw frames                */
/* RMSF.py:137-138 as written on the raw frames (rmsf_welford_sequential):
 * the running Welford state continued frame by frame with the reference's
 * own arithmetic, so rmsf_get_partial returns a rank's S of RMSF.py:140 bit
 * for bit.  rmsf_multi_chan_merge_exact reduces such contexts with
 * second_order_moments in comm.reduce's order (RMSF_MERGE_MPI4PY), device to
 * device: the script's result bit for bit.  (rmsf_multi_chan_merge combines
 * them too, to rounding.)                                                   */
#define RMSF_PUSH_EXACT 4

/* h_sel: n_sel int64 atom indices (MDAnalysis AtomGroup.indices; copied),
 * NULL = atoms 0..n_sel-1.  h_masses: n_sel f64 (copied) or NULL = uniform
 * (RMSF.py:84 center_of_mass).  flags must be 0.      */
int rmsf_ctx_create(int device, int64_t n_atoms, int64_t n_sel,
                    const int64_t *h_sel, const double *h_masses, int flags,
                    rmsf_ctx **out);
int rmsf_ctx_destroy(rmsf_ctx *ctx);
/* the context's hipStream_t (order producer work of device frames on it) */
int rmsf_ctx_stream(rmsf_ctx *ctx, void **stream);
int rmsf_ctx_synchronize(rmsf_ctx *ctx);
/* Host-frame staging: frames per pinned slot (<= 0: ~64 MiB worth), slots
 * (>= 1) and gather threads.  Takes effect at the next host push.           */
int rmsf_ctx_set_staging(rmsf_ctx *ctx, int64_t batch_frames, int n_slots,
                         int n_threads);
/* Measurement: with timing on, every superpose and accumulate launch the
 * context makes is bracketed by HIP events on its stream.
 * rmsf_ctx_kernel_time() synchronises and returns, for one kernel family,
 * the number of launches, their summed duration (ms) and the atom-frames
 * they processed (x 12 B = algorithmic bytes), then clears
 * that family's record.  Note: a push recorded for atom slabs
 * (rmsf_multi_push_frames with merge_slabs > 1) is run whole before the
 * timings are read, so reading them between that push and
 * rmsf_multi_chan_merge_root makes the merge take its non-overlapped form
 * (same bits; only the slab overlap is lost).  Read timings after the
 * merge to keep the overlap.                                                 */
#define RMSF_TIME_ACCUMULATE 0 /* rmsf_accumulate_balanced (RMSF.py:99-103,133-138) */
#define RMSF_TIME_SUPERPOSE 1  /* rmsf_superpose (RMSF.py:94-97 + qcprot, :43-51)  */
/* the cross-context merge, per context: from its packed moments to its
 * finished result on its stream (collective, waits for the slowest context,
 * unpack/finalise; with atom slabs the part after the last slab's pack);
 * atom_frames = 0                                                           */
#define RMSF_TIME_MERGE 2
int rmsf_ctx_set_timing(rmsf_ctx *ctx, int on);
int rmsf_ctx_kernel_time(rmsf_ctx *ctx, int which, int64_t *launches,
                         double *ms, double *atom_frames);
/* Per-frame QCP rmsd (the value RMSF.py:48 discards; AlignTraj's
 * results.rmsd): with collection on, every RMSF_PUSH_ALIGN_WELFORD push
 * appends its frames' rmsd, in push order, to a device list the context
 * keeps (cleared by turning collection on and by rmsf_ctx_reset(what & 1)).
 * rmsf_get_rmsd synchronises; *n = frames collected, h_rmsd (capacity
 * doubles, may be NULL to query n) receives them.                          */
int rmsf_ctx_collect_rmsd(rmsf_ctx *ctx, int on);
int rmsf_get_rmsd(rmsf_ctx *ctx, int64_t *n, double *h_rmsd, int64_t capacity);
/* Zero the running Welford (what & 1) and/or sweep-1 sum (what & 2) state. */
int rmsf_ctx_reset(rmsf_ctx *ctx, int what);

/* Reference given directly: h_ref_centered f64 [n_sel][3], h_ref_com f64[3]
 * (RMSF.py:85-86 ref_ca / ref_com).                                         */
int rmsf_set_reference(rmsf_ctx *ctx, const double *h_ref_centered,
                       const double *h_ref_com);
/* Reference from a float32 frame of n_atoms atoms (RMSF.py:80-87). */
int rmsf_set_reference_frame(rmsf_ctx *ctx, const float *xyz,
                             int is_device_ptr);
/* Reference = the context's sweep-1 average sum/n (RMSF.py:111-118);
 * RMSF_EEMPTY when no frame was summed.                                      */
int rmsf_set_reference_average(rmsf_ctx *ctx);

/* exact=True for the context (RMSF.py:80-146 with the reference's own
 * summation orders, the sequential entry points above): with on != 0 the
 * reference setters run rmsf_reference_setup_sequential, RMSF_PUSH_ALIGN_SUM
 * / RMSF_PUSH_ALIGN_WELFORD run rmsf_superpose_sequential +
 * rmsf_accumulate_sequential (RMSF_PUSH_WELFORD the sequential Welford, as
 * RMSF_PUSH_EXACT), and rmsf_multi_allreduce_sum over contexts of this
 * process adds the sums in rank order.  mass_total = numpy's masses.sum()
 * of the selection (pairwise; n_sel for unit masses), the centre of mass's
 * divisor.  Set it before the reference (an earlier reference is refused by
 * the aligned pushes); merge the Welford states with
 * rmsf_multi_chan_merge_exact.                                              */
int rmsf_ctx_set_exact(rmsf_ctx *ctx, int on, double mass_total);

/* Push n_frames float32 frames of n_atoms atoms (frame_stride floats apart,
 * 0 = 3*n_atoms; a multiple of it implements `step`).  is_device_ptr != 0:
 * the frames are in HBM and must stay valid and unmodified until the
 * context is synchronised; otherwise they are host memory, gathered to the
 * selection and streamed through the context's pinned stager (the host
 * buffer may be reused when the call returns).                               */
int rmsf_push_frames(rmsf_ctx *ctx, const float *xyz, int64_t n_frames,
                     int64_t frame_stride, int mode, int is_device_ptr);
/* Push XTC frames f0, f0+step, ... (n_frames) of an open file (RMSF.py:92,124
 * frame source): the compressed records are decompressed on the GPU (the
 * context keeps an rmsf_xtcdec for the file, up to 3 batches in flight).
 * When the context's selection is a proper subset of the atoms with no
 * index listed twice, only the selected atoms are decoded
 * (rmsf_xtcdec_create_sel); otherwise whole frames, gathered in-kernel.
 * Synchronises at the end to report corrupt frames.                          */
int rmsf_push_xtc(rmsf_ctx *ctx, const rmsf_xtc *x, int64_t f0,
                  int64_t n_frames, int64_t step, int mode);

/* Push the XTC frames h_frames[0..n) (a frame list, e.g. run(frames=...)):
 * decoded on the GPU in batches of scattered records, one wait at the end. */
int rmsf_push_xtc_frames(rmsf_ctx *ctx, const rmsf_xtc *x, const int64_t *h_frames,
                         int64_t n_frames, int mode);
/* Push n_frames host frames given as one pointer per frame (n_atoms float32
 * atoms each; e.g. the rows of a frame list, or per-Timestep buffers): the
 * stager gathers the selection from every frame into its pinned slots.      */
int rmsf_push_frame_ptrs(rmsf_ctx *ctx, const float *const *h_ptrs,
                         int64_t n_frames, int mode);
/* The same for host frames stored as coordinate planes (SoA; see
 * rmsf_stager_stage_planes): x, y, z of frame f at h_ptrs[f] + {0, 1, 2} *
 * plane_stride floats.                                                      */
int rmsf_push_frame_planes(rmsf_ctx *ctx, const float *const *h_ptrs,
                           int64_t plane_stride, int64_t n_frames, int mode);

/* Running Welford partial (RMSF.py:120-121,137-138): *n frames, mean and M2
 * f64 [n_sel][3] (any output may be NULL).  Synchronises.                    */
int rmsf_get_partial(rmsf_ctx *ctx, int64_t *n, double *h_mean, double *h_m2);
/* Sweep-1 sum (RMSF.py:103,105): *n frames and f64 [n_sel][3]. */
int rmsf_get_sum(rmsf_ctx *ctx, int64_t *n, double *h_sum);
/* Average structure sum/n (RMSF.py:111; AverageStructure.results.positions). */
int rmsf_get_average(rmsf_ctx *ctx, double *h_avg);
/* rmsf = sqrt(M2.sum(axis=1)/n) (RMSF.py:146), f64 [n_sel]. */
int rmsf_get_rmsf(rmsf_ctx *ctx, double *h_rmsf);
/* Replace the running Welford state (checkpoint restore / external merge). */
int rmsf_set_partial(rmsf_ctx *ctx, int64_t n, const double *h_mean,
                     const double *h_m2);

/* ---- cross-rank exchange (RMSF.py:107-110 all-reduce, :140-143 reduce) -----
 * Each exchange leaves the GLOBAL result in every participating context:
 *   allreduce_sum: sweep-1 sum and frame count summed over ranks;
 *   chan_merge:    exact k-way Chan of the Welford partials, as three
 *                  all-reduce(SUM) steps -- n, sum w_k mean_k (w_k=n_k/n),
 *                  sum M2_k + n_k (mean_k - mean)^2.  Empty ranks contribute
 *                  nothing; RMSF_EEMPTY if n == 0.
 * Three transports, the same arithmetic:
 *   (1) a caller callback -- fn sums the device buffer d_buf[0..count) in
 *       place over all ranks (MPI, gloo, ...) and returns 0.  d_buf is
 *       produced by work queued on `stream` (the context's): fn orders its
 *       reduction after it (enqueues on `stream`, or synchronises it first),
 *       and the sum is complete when fn returns or is queued on `stream`;
 *   (2) RCCL communicators (rmsf_multi_init / rmsf_multi_init_all);
 *   (3) neither: the n contexts of this process are reduced among themselves
 *       on the host, in context order (one process, any devices).          */
typedef int (*rmsf_allreduce_fn)(double *d_buf, int64_t count, void *stream,
                                 void *user);
int rmsf_ctx_allreduce_sum(rmsf_ctx *ctx, rmsf_allreduce_fn fn, void *user);
int rmsf_ctx_chan_merge(rmsf_ctx *ctx, rmsf_allreduce_fn fn, void *user);
/* The same merge with ONE data all-reduce (2*3*n_sel doubles, plus the
 * frame-count exchange): moments about the context's reference structure
 * (rmsf_chan_shift_pack / _finish).  Precondition, as in RMSF.py: every rank
 * holds the SAME reference (rmsf_ctx_set_reference_frame on the same frame,
 * or rmsf_ctx_set_reference_average after rmsf_ctx_allreduce_sum); every rank
 * must call this form (the buffer sizes differ from the two-pass form).
 * rmsf_multi_chan_merge uses it by itself when all ranks are contexts of the
 * calling process and each holds a reference.                              */
int rmsf_ctx_chan_merge_shifted(rmsf_ctx *ctx, rmsf_allreduce_fn fn, void *user);

/* RCCL (librccl.so.1, loaded on first use).  One process per GPU:
 * rank 0 calls rmsf_multi_unique_id, the host broadcasts the 128 bytes, each
 * rank calls rmsf_multi_init.  One process, many GPUs: rmsf_multi_init_all
 * (ncclCommInitAll over the contexts' devices).                              */
#define RMSF_UNIQUE_ID_BYTES 128
int rmsf_multi_unique_id(void *id_out);
int rmsf_multi_init(rmsf_ctx *ctx, const void *id, int nranks, int rank);
int rmsf_multi_init_all(rmsf_ctx **ctxs, int n);
int rmsf_multi_allreduce_sum(rmsf_ctx **ctxs, int n);
int rmsf_multi_chan_merge(rmsf_ctx **ctxs, int n);

/* ---- one process, several contexts: the torchrun rank step's shape --------
 * The merge's shift for UNALIGNED Welford state (RMSF.py:141-143 as one
 * collective of moments about a shift every rank holds; aligned state uses
 * the reference): frame 0 of the frame list, n_atoms float32 atoms, host or
 * device pointer; the context keeps its selected rows (f32) and a digest.
 * rmsf_multi_chan_merge[_root] merges unaligned contexts in one collective
 * when all hold the same shift frame, else in the two-pass form.           */
int rmsf_set_merge_shift_frame(rmsf_ctx *ctx, const float *xyz,
                               int is_device_ptr);
/* rmsf_multi_chan_merge with RMSF.py:143's shape: root >= 0 reduces the
 * moments to context `root` only (half the link bytes of an all-reduce);
 * the other contexts then refuse rmsf_get_rmsf / rmsf_get_partial with
 * RMSF_EINVAL until they are reset.  root = -1: every context gets the
 * result (rmsf_multi_chan_merge).  Only the one-collective (shifted) merge
 * can reduce to a root; the two-pass form leaves the result everywhere.
 * Replaces RMSF.py:140-143 (comm.Barrier + comm.reduce(root=0)).           */
int rmsf_multi_chan_merge_root(rmsf_ctx **ctxs, int n, int root);
/* RMSF.py:141-143 as the script computes it: the contexts' Welford states
 * (each a rank's S of RMSF.py:140, context i = rank i) reduced with
 * second_order_moments in `order` (RMSF_MERGE_MPI4PY: comm.reduce's
 * binomial tree; RMSF_MERGE_RANK: rank order) -- each step copies the
 * source context's state to the destination's device (peer copy over xGMI,
 * or a device copy) and merges it there (rmsf_chan_merge_pair), the steps of
 * one tree level on their own streams at once.  The result is context 0's,
 * then forwarded to `root` (the others refuse getters with RMSF_EINVAL until
 * reset) or, root = -1, to every context.  Bit for bit with RMSF.py:143 on
 * RMSF_PUSH_EXACT states.  Contexts of this process only (a communicator
 * spanning processes: RMSF_EINVAL).                                        */
int rmsf_multi_chan_merge_exact(rmsf_ctx **ctxs, int n, int root, int order);
/* Push each context's HBM frames d_frames[i] (n_frames[i] frames,
 * frame_stride floats apart, 0 = 3*n_atoms) in `mode`, the n contexts'
 * launches enqueued from one host thread per device (asynchronous: the
 * frames must stay valid until the contexts are synchronised).  Per context,
 * first: flags & RMSF_MULTI_RESET resets the state `mode` accumulates into;
 * d_ref_frames[i] (device frame, may be NULL) sets the reference
 * (rmsf_set_reference_frame); d_shift_frames[i] the merge shift frame.
 * merge_slabs (unaligned Welford, no selection, one launch group whose flat
 * plan is chunk-aligned, a shift frame set, fresh state): 0 = auto (2 slabs
 * from 1M atoms, as the torchrun pipeline), 1 = off, k >= 2 = k slabs -- the
 * push is then recorded, and the next rmsf_multi_chan_merge_root streams it
 * slab by slab with each slab's collective (on a communicator stream, RCCL)
 * beside the next slab's accumulate; any other call runs it whole.          */
#define RMSF_MULTI_RESET 1
int rmsf_multi_push_frames(rmsf_ctx **ctxs, int n, const float *const *d_frames,
                           const int64_t *n_frames, int64_t frame_stride,
                           int mode, int flags, const float *const *d_ref_frames,
                           const float *const *d_shift_frames, int merge_slabs);
/* Transport of the contexts' exchanges: AUTO = RCCL when every context has a
 * communicator, else the in-process host fold; NOOP = a timing rehearsal of
 * N contexts on fewer devices -- the exchanges move no data, so the merged
 * statistics are NOT the global ones (measurement only).                    */
#define RMSF_TRANSPORT_AUTO 0
#define RMSF_TRANSPORT_NOOP 1
int rmsf_multi_set_transport(rmsf_ctx **ctxs, int n, int transport);

#ifdef __cplusplus
}
#endif
#endif /* RMSF_HIP_H */
