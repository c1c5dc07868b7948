// pca_backproject.hip -- the adjoint of the PCA projection on the f64 matrix
// cores of gfx950 (MI355X, CDNA4), and the extern "C" launchers declared in
// include/rmsf_hip.h.
//
//   Y[i][c] (+)= sum_f d_i(f) P[f][c],   d = f64(p) - mean
//
// where p is the selected atom's three floats, through apply_xform
// (rmsf_device.h: the transform of RMSF.py:99-101 / 133-135, the very code
// the Welford, covariance and projection sweeps run) when transform records
// are given.  With pca_project.hip's X Q it is the matrix-free covariance
// product M Q = D^T (D Q) / (F - ddof) of PCA(solver="matrix_free"): the
// fourth dense contraction of the domain, over the frames like
// covariance.hip, with operand B the rows of P where that kernel stages a
// second tile of deviations.
//
//   * k_bproj_tiles  one workgroup per (macro tile of 16 atoms = 48
//                    coordinates, frame range): coordinates are the M side of
//                    v_mfma_f64_16x16x4_f64 (3 tiles), the columns of P the N
//                    side (1-3 tiles: 3 x NT accumulators of 4 f64 a wave),
//                    frames the contraction.  The deviations of 32 frames are
//                    staged as f64 [frame][coord] in LDS; each of the 4 waves
//                    contracts 8 of them.  The rows of P already have B's
//                    shape and are read through L2 into registers.
//   * k_bproj_fold   the split-K partials, summed in frame-range order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dense_f64.h"
#include "rmsf_device.h"
#include "rmsf_host.h"

namespace {

constexpr int kTA = 16;                    // atoms of a macro tile
constexpr int kTC = 3 * kTA;               // its coordinates: 3 MFMA tiles
constexpr int kTN = 16;                    // columns of P an N tile
constexpr int kMaxNT = 3;                  // N tiles a workgroup
constexpr int kPanel = kTN * kMaxNT;       // the widest P: 48 columns
constexpr int kKT = 32;                    // frames staged at a time (8 per wave: 2 MFMA k-steps)
constexpr int kFrameLanes = kBlock / kTA;  // frames staged per pass (one atom per lane)
constexpr int kPasses = kKT / kFrameLanes;
constexpr int kSteps = kKT / (4 * kWaves);  // k-steps a wave and stage
constexpr int64_t kTargetGroups = 512;      // 2 resident workgroups per CU on MI355X
constexpr int64_t kMinStages = 4;           // no frame range under 128 frames: below, prologue and fold cost more
constexpr int kSm = kKT * kTC > kTC * kPanel ? kKT * kTC : kTC * kPanel;  // a stage, or the waves' sum

static_assert(kKT % (4 * kWaves) == 0, "whole k-steps a wave");
static_assert(sizeof(double) * (kSm + kKT * kRec) <= kLdsLimit, "sm and sxf fit");

// The work decomposition, a function of (n_frames, n_sel, n_cols) alone, so
// the workspace layout and the summation order are fixed by the shapes.
struct BackPlan {
  int64_t n_tiles;    // macro tiles of 16 atoms
  int n_nt;           // N tiles of P
  int64_t n_ks;       // frame ranges (split-K); 1 = results go straight to d_y
  int64_t ks_frames;  // frames per range, a multiple of kKT
};

BackPlan back_plan(int64_t n_frames, int64_t n_sel, int64_t n_cols) {
  BackPlan p;
  p.n_tiles = (n_sel + kTA - 1) / kTA;
  p.n_nt = (int)((n_cols + kTN - 1) / kTN);
  const int64_t stages = std::max<int64_t>(1, (n_frames + kKT - 1) / kKT);
  const SplitK k = split_k(stages, std::max<int64_t>(1, p.n_tiles), kTargetGroups, kMinStages);
  p.n_ks = k.n_ks;
  p.ks_frames = k.per * kKT;
  return p;
}

size_t back_work_doubles(const BackPlan &p, int64_t n_sel, int64_t n_cols) {
  if (p.n_ks <= 1) return 0;
  return (size_t)p.n_ks * (size_t)(3 * n_sel) * (size_t)n_cols;
}

// acc[i][j] += a_i b_j over one k-step of four, in row order (mfma_3x3's).
template <int NT>
__device__ __forceinline__ void mfma_3xn(f64x4 (&acc)[3][NT], const double (&a)[3], const double (&b)[NT]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
}
__device__ __forceinline__ void mfma_3xn(f64x4 (&acc)[3][3], const double (&a)[3], const double (&b)[3]) {
  mfma_3x3(acc, a[0], a[1], a[2], b[0], b[1], b[2]);
}

// One workgroup: atoms [16 blockIdx.x, +16), frames [blockIdx.y ks_frames,
// ...).  Staging (k_comoment_tiles' operand A): lane (tid & 15) owns one atom
// of the tile, (tid >> 4) one of 16 frames per pass; its three deviations go
// to sm[k][3 atom + c].  MFMA operands (16x16x4 f64, dense_f64.h): lane l holds
// A[i = l & 15][k = l >> 4] = the deviation of coordinate 16 t + i in staged
// frame k, one of 16 consecutive doubles of row k, and B[k = l >> 4][j = l &
// 15] = P's row of frame k, 16 consecutive doubles of d_p; the result D has
// col = l & 15 (column of P), row = (l >> 4) + 4 reg (coordinate).
template <bool ALIGN, bool GATHER, int NT>
__global__ __launch_bounds__(kBlock, 2) void k_bproj_tiles(const float *__restrict__ xyz, int64_t fstride,
                                                        int64_t n_frames, int64_t n_sel,
                                                        const int32_t *__restrict__ sel,
                                                        const double *__restrict__ xform,
                                                        const double *__restrict__ refinfo,
                                                        const double *__restrict__ mean,
                                                        const double *__restrict__ pm, int64_t ldp, int64_t n_cols,
                                                        double *__restrict__ y, int64_t ldy, int accumulate,
                                                        double *__restrict__ work, int64_t ks_frames, int direct) {
  __shared__ double sm[kSm];                      // a stage of deviations; reused for the waves' sum
  __shared__ double sxf[ALIGN ? kKT * kRec : 1];  // the staged frames' transform records (R, mobile COM)

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ta = tid & (kTA - 1), tf = tid >> 4;
  const int64_t I = blockIdx.x, ks = blockIdx.y;
  const int64_t n_coord = 3 * n_sel;
  const int64_t f0 = ks * ks_frames;
  const int64_t f1 = f0 + ks_frames < n_frames ? f0 + ks_frames : n_frames;

  // Every load is unconditional and in bounds: an atom past the selection's
  // end reads the last atom, a frame past the range's end the last frame, a
  // column past n_cols the last column, and what came of it is zeroed
  // afterwards (a load inside a branch is waited for on the spot).
  const int64_t a = kTA * I + ta;
  const bool live = a < n_sel;
  const int64_t ac = live ? a : n_sel - 1;
  const float *__restrict__ p_at = xyz + 3 * (GATHER ? (int64_t)sel[ac] : ac);
  const double mu0 = mean[3 * ac], mu1 = mean[3 * ac + 1], mu2 = mean[3 * ac + 2];
  const double rc0 = ALIGN ? refinfo[0] : 0.0, rc1 = ALIGN ? refinfo[1] : 0.0, rc2 = ALIGN ? refinfo[2] : 0.0;

  // the lane's column of each N tile
  const double *__restrict__ bcol[NT];
  bool c_on[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int64_t c = kTN * j + (lane & 15);
    c_on[j] = c < n_cols;
    bcol[j] = pm + (c_on[j] ? c : n_cols - 1);
  }

  f64x4 acc[3][NT];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  // The next stage's floats, its transform records (1.5 doubles a lane) and
  // the wave's rows of P are loaded into registers before the current stage's
  // MFMAs, so the global-load latency runs under the matrix pipe; the floats
  // become deviations in LDS after, and the records are parked in LDS (sxf)
  // once the MFMAs are issued, where the 16 lanes of a frame read them as a
  // broadcast (load_records / park_records, rmsf_device.h).
  float raw[kPasses][3];
  double recv[rec_loads(kKT, kBlock)];
  double bn[kSteps][NT];
  auto prefetch = [&](int64_t fb) {
    if (ALIGN) load_records<kKT, kBlock>(recv, xform, fb, f1, tid);
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const int64_t f = fb + (kKT / kWaves) * wave + 4 * s + (lane >> 4);
      const int64_t fc = f < f1 ? f : f1 - 1;
#pragma unroll
      for (int j = 0; j < NT; ++j) bn[s][j] = bcol[j][fc * ldp];
    }
#pragma unroll
    for (int pass = 0; pass < kPasses; ++pass) {
      const int64_t f = fb + pass * kFrameLanes + tf;
      const float *__restrict__ q = p_at + (f < f1 ? f : f1 - 1) * fstride;
      raw[pass][0] = q[0], raw[pass][1] = q[1], raw[pass][2] = q[2];
    }
  };
  prefetch(f0);
  if (ALIGN) park_records<kKT, kBlock>(sxf, recv, tid);
  __syncthreads();

  for (int64_t fb = f0; fb < f1; fb += kKT) {
    // ---- this stage's rows of P (zeros past either edge)
    double b[kSteps][NT];
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const bool on = fb + (kKT / kWaves) * wave + 4 * s + (lane >> 4) < f1;
#pragma unroll
      for (int j = 0; j < NT; ++j) b[s][j] = on && c_on[j] ? bn[s][j] : 0.0;
    }
    // ---- stage kKT frames of the tile's deviations (zeros past either edge)
#pragma unroll
    for (int pass = 0; pass < kPasses; ++pass) {
      const int k = pass * kFrameLanes + tf;
      const bool on = live && fb + k < f1;
      float x = raw[pass][0], yy = raw[pass][1], z = raw[pass][2];
      if (ALIGN) apply_xform(x, yy, z, sxf + k * kRec, rc0, rc1, rc2);
      double *__restrict__ o = sm + k * kTC + 3 * ta;
      o[0] = on ? (double)x - mu0 : 0.0;
      o[1] = on ? (double)yy - mu1 : 0.0;
      o[2] = on ? (double)z - mu2 : 0.0;
    }
    __syncthreads();
    // (after the barrier: its fence waits for every load in flight)
    if (fb + kKT < f1) prefetch(fb + kKT);
    // ---- contract: wave w takes rows [8 w, 8 w + 8) of the staged tile
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const int k = (kKT / kWaves) * wave + 4 * s + (lane >> 4);
      const double *__restrict__ ra = sm + k * kTC + (lane & 15);
      const double av[3] = {ra[0], ra[16], ra[32]};
      mfma_3xn(acc, av, b[s]);
    }
    if (ALIGN) park_records<kKT, kBlock>(sxf, recv, tid);  // this stage's were last read before the barrier above
    __syncthreads();
  }

  // ---- the four waves' accumulators, summed in wave order: row-major [kTC][16 NT]
  wave_sum_3x3(acc, sm, lane, wave,
               [](int i, int j, int row, int col) { return (16 * i + row) * (kTN * NT) + 16 * j + col; });

  for (int e = tid; e < kTC * kTN * NT; e += kBlock) {
    const int64_t i = kTC * I + e / (kTN * NT);
    const int64_t c = e % (kTN * NT);
    if (i >= n_coord || c >= n_cols) continue;
    if (direct) {
      double *__restrict__ o = y + i * ldy + c;
      *o = accumulate ? *o + sm[e] : sm[e];
    } else {
      work[(ks * n_coord + i) * n_cols + c] = sm[e];
    }
  }
}

// d_y = the n_ks partials of every element, summed in frame-range order:
// from d_y when accumulating, else from the first range's partial.
__global__ __launch_bounds__(kBlock) void k_bproj_fold(const double *__restrict__ work, int64_t n_coord,
                                                       int64_t n_cols, int64_t n_ks, double *__restrict__ y,
                                                       int64_t ldy, int accumulate) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n = n_coord * n_cols;
  if (e >= n) return;
  double *__restrict__ o = y + (e / n_cols) * ldy + e % n_cols;
  double s = accumulate ? *o + work[e] : work[e];
  for (int64_t k = 1; k < n_ks; ++k) s += work[k * n + e];
  *o = s;
}

template <bool A_, bool G_>
void launch_tiles(int nt, dim3 grid, hipStream_t st, const float *d_xyz, int64_t fstride, int64_t n_frames,
                  int64_t n_sel, const int32_t *d_sel, const double *d_xform, const double *d_refinfo,
                  const double *d_mean, const double *d_p, int64_t ldp, int64_t n_cols, double *d_y, int64_t ldy,
                  int accumulate, double *work, int64_t ks_frames, int direct) {
#define BPROJ_LAUNCH(NT_)                                                                                        \
  hipLaunchKernelGGL((k_bproj_tiles<A_, G_, NT_>), grid, dim3(kBlock), 0, st, d_xyz, fstride, n_frames, n_sel,  \
                     d_sel, d_xform, d_refinfo, d_mean, d_p, ldp, n_cols, d_y, ldy, accumulate, work, ks_frames, \
                     direct)
  if (nt == 1) BPROJ_LAUNCH(1);
  else if (nt == 2) BPROJ_LAUNCH(2);
  else BPROJ_LAUNCH(3);
#undef BPROJ_LAUNCH
}

}  // namespace

extern "C" {

RMSF_EXPORT size_t rmsf_pca_backproject_workspace_bytes(int64_t n_frames, int64_t n_sel, int64_t n_cols) {
  if (n_frames < 1 || n_sel < 1 || n_cols < 1 || n_cols > kPanel) return 0;
  return back_work_doubles(back_plan(n_frames, n_sel, n_cols), n_sel, n_cols) * sizeof(double);
}

RMSF_EXPORT int rmsf_pca_backproject(const float *d_xyz, int64_t fstride, int64_t n_frames, int64_t n_sel,
                                     const int32_t *d_sel, const double *d_xform, const double *d_refinfo,
                                     const double *d_mean, const double *d_p, int64_t ldp, int64_t n_cols,
                                     double *d_y, int64_t ldy, int accumulate, void *d_work, size_t work_bytes,
                                     void *stream) {
  if (!d_xyz || !d_mean || !d_p || !d_y) return fail(RMSF_EINVAL, "rmsf_pca_backproject: NULL pointer");
  if (n_sel < 1 || n_frames < 0 || fstride < 0) return fail(RMSF_EINVAL, "rmsf_pca_backproject: bad sizes");
  if (n_cols < 1 || n_cols > kPanel) return fail(RMSF_EINVAL, "rmsf_pca_backproject: n_cols must be in 1..48");
  if (ldp < n_cols || ldy < n_cols)
    return fail(RMSF_EINVAL, "rmsf_pca_backproject: ldp and ldy must be >= n_cols");
  if ((d_xform != nullptr) != (d_refinfo != nullptr))
    return fail(RMSF_EINVAL, "rmsf_pca_backproject: d_xform and d_refinfo go together");
  if (n_frames == 0) return RMSF_OK;
  const BackPlan pl = back_plan(n_frames, n_sel, n_cols);
  const int64_t n_out = 3 * n_sel * n_cols;
  if (pl.n_tiles > INT32_MAX || pl.n_ks > 65535 || (n_out + kBlock - 1) / kBlock > INT32_MAX)
    return fail(RMSF_EINVAL, "rmsf_pca_backproject: selection or batch too large for one launch");
  const size_t need = back_work_doubles(pl, n_sel, n_cols) * sizeof(double);
  if (need && (!d_work || work_bytes < need))
    return fail(RMSF_EINVAL, "rmsf_pca_backproject: workspace too small");
  const int direct = pl.n_ks == 1;
  const int acc = accumulate != 0;
  double *work = static_cast<double *>(d_work);
  const dim3 grid((unsigned)pl.n_tiles, (unsigned)pl.n_ks);
#define BPROJ_ARGS                                                                                                 \
  pl.n_nt, grid, S(stream), d_xyz, fstride, n_frames, n_sel, d_sel, d_xform, d_refinfo, d_mean, d_p, ldp, n_cols, \
      d_y, ldy, acc, work, pl.ks_frames, direct
  const bool al = d_xform != nullptr, g = d_sel != nullptr;
  if (al && g) launch_tiles<true, true>(BPROJ_ARGS);
  else if (al) launch_tiles<true, false>(BPROJ_ARGS);
  else if (g) launch_tiles<false, true>(BPROJ_ARGS);
  else launch_tiles<false, false>(BPROJ_ARGS);
#undef BPROJ_ARGS
  if (int rc = after_launch("k_bproj_tiles")) return rc;
  if (!direct) {
    hipLaunchKernelGGL(k_bproj_fold, dim3((unsigned)((n_out + kBlock - 1) / kBlock)), dim3(kBlock), 0, S(stream), work,
                       3 * n_sel, n_cols, pl.n_ks, d_y, ldy, acc);
    if (int rc = after_launch("k_bproj_fold")) return rc;
  }
  return RMSF_OK;
}

}  // extern "C"
