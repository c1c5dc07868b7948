// covariance.hip -- the positional co-moment matrix of the (aligned)
// coordinates on the f64 matrix cores of gfx950 (MI355X, CDNA4), and the
// extern "C" launchers declared in include/rmsf_hip.h.
//
//   C[i][j] += sum_f d_i(f) d_j(f),  T1[i] += sum_f d_i(f),  d = f64(p) - shift
//
// where p is the selected atom's three floats, through apply_xform
// (rmsf_device.h: the transform of RMSF.py:99-101 / 133-135, the very code
// the Welford sweep runs) when transform records are given.  The RMSF of
// RMSF.py:146 is the diagonal of this matrix; its eigenvectors are the
// modes of MDAnalysis.analysis.pca.PCA.
//
//   * k_cov_tiles   one workgroup per (macro tile pair J >= I, frame range):
//                   16 atoms = 48 coordinates a side, 3 x 3 tiles of
//                   v_mfma_f64_16x16x4_f64 per wave (9 accumulators of 4 f64).
//                   The deviations of 32 frames are staged as f64 [k][coord]
//                   in LDS; each of the 4 waves contracts 8 of them.
//   * k_cov_fold    the split-K partials, summed in frame-range order.
//   * k_cov_finish  M = C - T1 T1^T / N, mirrored to the full matrix.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dense_f64.h"
#include "rmsf_device.h"
#include "rmsf_host.h"

namespace {

constexpr int kTA = 16;                // atoms a side of a macro tile
constexpr int kTC = 3 * kTA;           // coordinates a side: 3 MFMA tiles
constexpr int kKT = 32;                // frames staged at a time (8 per wave: 2 MFMA k-steps)
constexpr int kTile = kTC * kTC;       // results of a macro tile pair
constexpr int kFrameLanes = kBlock / kTA;  // frames staged per pass (one atom per lane)
constexpr int64_t kTargetGroups = 512;     // 2 resident workgroups (152-200 VGPRs) per CU on MI355X

static_assert(sizeof(double) * (2 * kKT * kTC + kFrameLanes * kTC + kKT * kRec) <= kLdsLimit, "sm, st1 and sxf fit");

// The work decomposition, a function of (n_sel, n_frames) alone, so the
// workspace layout and the summation order are fixed by the batching.
struct CovPlan {
  int64_t n_tiles;    // macro tiles a side
  int64_t n_pairs;    // tile pairs J >= I
  int64_t n_ks;       // frame ranges (split-K); 1 = results go straight to d_cov
  int64_t ks_frames;  // frames per range, a multiple of kKT
};

CovPlan cov_plan(int64_t n_sel, int64_t n_frames) {
  CovPlan p;
  p.n_tiles = (n_sel + kTA - 1) / kTA;
  p.n_pairs = p.n_tiles * (p.n_tiles + 1) / 2;
  const SplitK k = split_k(std::max<int64_t>(1, (n_frames + kKT - 1) / kKT), p.n_pairs, kTargetGroups, 1);
  p.n_ks = k.n_ks;
  p.ks_frames = k.per * kKT;
  return p;
}

size_t cov_work_doubles(const CovPlan &p) {
  if (p.n_ks <= 1) return 0;
  return (size_t)p.n_ks * ((size_t)p.n_pairs * kTile + (size_t)p.n_tiles * kTC);
}

// One workgroup: tile pair blockIdx.x, frames [blockIdx.y ks_frames, ...).
// Staging: lane (tid & 15) owns one atom of the tile, (tid >> 4) one of 16
// frames per pass; its three deviations go to sm[op][k][3 atom + c], so an
// MFMA operand (mfma_3x3, dense_f64.h) is 16 consecutive doubles of row k.
template <bool ALIGN, bool GATHER>
__global__ __launch_bounds__(kBlock, 2) void k_cov_tiles(const float *__restrict__ xyz, int64_t fstride,
                                                      int64_t n_frames, int64_t n_sel,
                                                      const int32_t *__restrict__ sel,
                                                      const double *__restrict__ xform,
                                                      const double *__restrict__ refinfo,
                                                      const double *__restrict__ shift, double *__restrict__ cov,
                                                      int64_t ld, double *__restrict__ t1, double *__restrict__ work,
                                                      int64_t n_tiles, int64_t n_pairs, int64_t ks_frames,
                                                      int direct) {
  __shared__ double sm[2 * kKT * kTC];      // A then B deviations; reused for the waves' sum
  __shared__ double st1[kFrameLanes * kTC];  // T1 partials per frame lane
  __shared__ double sxf[ALIGN ? kKT * kRec : 1];  // the staged frames' transform records (R, mobile COM)

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ta = tid & (kTA - 1), tf = tid >> 4;
  const int64_t pair = blockIdx.x, ks = blockIdx.y;
  int64_t I, J;
  pair_to_tiles(pair, n_tiles, I, J);
  const bool diag = I == J;
  const int n_ops = diag ? 1 : 2;
  const int64_t n_coord = 3 * n_sel;

  const int64_t f0 = ks * ks_frames;
  const int64_t f1 = f0 + ks_frames < n_frames ? f0 + ks_frames : n_frames;

  // The lane's atom of each operand tile: its row offset, its shift, and
  // whether it exists.  A lane past the selection's end reads the last atom
  // instead (and a frame past the range's end the last frame), so every load
  // is unconditional and in bounds -- a load inside a branch is waited for on
  // the spot, one latency after another -- and its deviation is zeroed after.
  const float *p_op[2];
  double sh[2][3];
  bool live[2];
#pragma unroll
  for (int op = 0; op < 2; ++op) {
    const int64_t a = kTA * (op ? J : I) + ta;
    live[op] = a < n_sel;
    const int64_t ac = live[op] ? a : n_sel - 1;
    p_op[op] = xyz + 3 * (GATHER ? (int64_t)sel[ac] : ac);
    sh[op][0] = shift[3 * ac], sh[op][1] = shift[3 * ac + 1], sh[op][2] = shift[3 * ac + 2];
  }
  const double rc0 = ALIGN ? refinfo[0] : 0.0, rc1 = ALIGN ? refinfo[1] : 0.0, rc2 = ALIGN ? refinfo[2] : 0.0;

  f64x4 acc[3][3];
  zero_3x3(acc);
  double ts[3] = {0.0, 0.0, 0.0};  // the lane's share of T1 (operand A, its frames in order)

  const double *sA = sm;
  const double *sB = diag ? sm : sm + kKT * kTC;

  // The next stage's floats are loaded into registers before the current
  // stage's MFMAs, so the global-load latency runs under the matrix pipe; they
  // become deviations in LDS after.  The stage's transform records travel
  // the same way, 1.5 doubles a lane, and are parked in LDS (sxf) once the
  // MFMAs are issued, where the 16 lanes of a frame read them as a broadcast.
  constexpr int kPasses = kKT / kFrameLanes;
  constexpr int kRecLoads = (kKT * kRec + kBlock - 1) / kBlock;
  float raw[2][kPasses][3];
  double recv[kRecLoads];
  auto prefetch = [&](int64_t fb) {
    if (ALIGN) {
#pragma unroll
      for (int r = 0; r < kRecLoads; ++r) {
        const int e = (r * kBlock + tid) % (kKT * kRec);  // (the last round wraps: its extra lanes reload)
        const int64_t f = fb + e / kRec;
        recv[r] = xform[(f < f1 ? f : f1 - 1) * kXform + e % kRec];
      }
    }
#pragma unroll
    for (int pass = 0; pass < kPasses; ++pass) {
      const int64_t f = fb + pass * kFrameLanes + tf;
      const int64_t fc = f < f1 ? f : f1 - 1;
#pragma unroll
      for (int op = 0; op < 2; ++op) {
        const float *__restrict__ q = p_op[op] + fc * fstride;
        raw[op][pass][0] = q[0], raw[op][pass][1] = q[1], raw[op][pass][2] = q[2];
      }
    }
  };
  auto park_records = [&]() {
    if (ALIGN) {
#pragma unroll
      for (int r = 0; r < kRecLoads; ++r) {
        const int e = r * kBlock + tid;
        if (e < kKT * kRec) sxf[e] = recv[r];
      }
    }
  };
  prefetch(f0);
  park_records();
  __syncthreads();

  for (int64_t fb = f0; fb < f1; fb += kKT) {
    // ---- stage kKT frames of both operand tiles (zeros past either edge)
#pragma unroll
    for (int op = 0; op < 2; ++op) {
      if (op >= n_ops) break;
#pragma unroll
      for (int pass = 0; pass < kPasses; ++pass) {
        const int k = pass * kFrameLanes + tf;
        const int64_t f = fb + k;
        const bool on = live[op] && f < f1;
        float x = raw[op][pass][0], y = raw[op][pass][1], z = raw[op][pass][2];
        if (ALIGN) apply_xform(x, y, z, sxf + k * kRec, rc0, rc1, rc2);
        const double d0 = on ? (double)x - sh[op][0] : 0.0;
        const double d1 = on ? (double)y - sh[op][1] : 0.0;
        const double d2 = on ? (double)z - sh[op][2] : 0.0;
        double *__restrict__ o = sm + (op * kKT + k) * kTC + 3 * ta;
        o[0] = d0, o[1] = d1, o[2] = d2;
        if (op == 0) ts[0] += d0, ts[1] += d1, ts[2] += d2;
      }
    }
    __syncthreads();
    // (after the barrier: its fence waits for every load in flight)
    if (fb + kKT < f1) prefetch(fb + kKT);
    // ---- contract: wave w takes rows [8 w, 8 w + 8) of the staged tile
#pragma unroll
    for (int s = 0; s < kKT / (4 * kWaves); ++s) {
      const int k = (kKT / kWaves) * wave + 4 * s + (lane >> 4);
      const double *__restrict__ ra = sA + k * kTC + (lane & 15);
      const double *__restrict__ rb = sB + k * kTC + (lane & 15);
      const double a0 = ra[0], a1 = ra[16], a2 = ra[32];
      const double b0 = rb[0], b1 = rb[16], b2 = rb[32];
      mfma_3x3(acc, a0, a1, a2, b0, b1, b2);
    }
    park_records();  // this stage's were last read before the barrier above
    __syncthreads();
  }

  // ---- the four waves' accumulators, summed in wave order: row-major [kTC][kTC]
  wave_sum_3x3(acc, sm, lane, wave,
               [](int i, int j, int row, int col) { return (16 * i + row) * kTC + 16 * j + col; });
  if (diag) st1[tf * kTC + 3 * ta] = ts[0], st1[tf * kTC + 3 * ta + 1] = ts[1], st1[tf * kTC + 3 * ta + 2] = ts[2];
  __syncthreads();

  if (direct) {
    for (int e = tid; e < kTile; e += kBlock) {
      const int64_t i = kTC * I + e / kTC, j = kTC * J + e % kTC;
      if (i < n_coord && j < n_coord) cov[i * ld + j] += sm[e];
    }
  } else {
    double *__restrict__ w = work + ((int64_t)ks * n_pairs + pair) * kTile;
    for (int e = tid; e < kTile; e += kBlock) w[e] = sm[e];
  }
  if (diag && tid < kTC) {
    double s = 0.0;
    for (int g = 0; g < kFrameLanes; ++g) s += st1[g * kTC + tid];
    const int64_t i = kTC * I + tid;
    if (direct) {
      if (i < n_coord) t1[i] += s;
    } else {
      work[(int64_t)gridDim.y * n_pairs * kTile + ((int64_t)ks * n_tiles + I) * kTC + tid] = s;
    }
  }
}

// d_cov / d_t1 += the n_ks partials of every element, in frame-range order.
// Workgroups (pair, ninth of the tile); the last n_tiles columns fold T1.
__global__ __launch_bounds__(kBlock) void k_cov_fold(const double *__restrict__ work, int64_t n_sel, int64_t n_tiles,
                                                     int64_t n_pairs, int64_t n_ks, double *__restrict__ cov,
                                                     int64_t ld, double *__restrict__ t1) {
  const int64_t n_coord = 3 * n_sel;
  const int64_t bx = blockIdx.x;
  if (bx >= n_pairs) {
    const int64_t I = bx - n_pairs;
    if (blockIdx.y != 0 || threadIdx.x >= kTC) return;
    const int64_t i = kTC * I + threadIdx.x;
    if (i >= n_coord) return;
    const double *__restrict__ w = work + n_ks * n_pairs * kTile + I * kTC + threadIdx.x;
    double s = 0.0;
    for (int64_t k = 0; k < n_ks; ++k) s += w[k * n_tiles * kTC];
    t1[i] += s;
    return;
  }
  int64_t I, J;
  pair_to_tiles(bx, n_tiles, I, J);
  const int e = blockIdx.y * kBlock + threadIdx.x;
  if (e >= kTile) return;
  const int64_t i = kTC * I + e / kTC, j = kTC * J + e % kTC;
  if (i >= n_coord || j >= n_coord) return;
  const double *__restrict__ w = work + bx * kTile + e;
  double s = 0.0;
  for (int64_t k = 0; k < n_ks; ++k) s += w[k * n_pairs * kTile];
  cov[i * ld + j] += s;
}

// M = C - T1 T1^T / N over the upper triangle's 32 x 32 tiles, each written
// back with its mirror image (through LDS, so both stores run along rows).
__global__ __launch_bounds__(kBlock) void k_cov_finish(double *__restrict__ cov, int64_t ld,
                                                       const double *__restrict__ t1, int64_t n, double n_frames) {
  __shared__ double s[32][33];
  const int64_t bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += kBlock / 32) {
    const int64_t i = 32 * bi + r, j = 32 * bj + tx;
    double v = 0.0;
    if (i < n && j < n) {
      const int64_t a = j >= i ? i : j, b = j >= i ? j : i;  // the upper triangle's element
      v = cov[a * ld + b] - t1[a] * t1[b] / n_frames;
    }
    s[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += kBlock / 32) {
    const int64_t i = 32 * bi + r, j = 32 * bj + tx;
    if (i < n && j < n) cov[i * ld + j] = s[r][tx];
    if (bi != bj) {
      const int64_t i2 = 32 * bj + r, j2 = 32 * bi + tx;
      if (i2 < n && j2 < n) cov[i2 * ld + j2] = s[tx][r];
    }
  }
}

}  // namespace

extern "C" {

// (for the tests: the tile mapping of this kernel and pairwise.hip's, on the host)
RMSF_EXPORT void rmsf_internal_pair_to_tiles(int64_t p, int64_t n_tiles, int64_t *I, int64_t *J) {
  pair_to_tiles(p, n_tiles, *I, *J);
}

RMSF_EXPORT size_t rmsf_covariance_workspace_bytes(int64_t n_sel, int64_t n_frames) {
  if (n_sel < 1 || n_frames < 1) return 0;
  return cov_work_doubles(cov_plan(n_sel, n_frames)) * sizeof(double);
}

RMSF_EXPORT int rmsf_covariance_accumulate(const float *d_xyz, int64_t fstride, int64_t n_frames, int64_t n_sel,
                                           const int32_t *d_sel, const double *d_xform, const double *d_refinfo,
                                           const double *d_shift, double *d_cov, int64_t ld, double *d_t1,
                                           void *d_work, size_t work_bytes, void *stream) {
  if (!d_xyz || n_sel < 1 || n_frames < 0 || fstride < 0 || !d_shift || !d_cov || !d_t1 || ld < 3 * n_sel)
    return fail(RMSF_EINVAL, "rmsf_covariance_accumulate: bad arguments");
  if ((d_xform != nullptr) != (d_refinfo != nullptr))
    return fail(RMSF_EINVAL, "rmsf_covariance_accumulate: d_xform and d_refinfo go together");
  if (n_frames == 0) return RMSF_OK;
  const CovPlan pl = cov_plan(n_sel, n_frames);
  if (pl.n_pairs > INT32_MAX - pl.n_tiles || pl.n_ks > 65535)
    return fail(RMSF_EINVAL, "rmsf_covariance_accumulate: selection or batch too large for one launch");
  const size_t need = cov_work_doubles(pl) * sizeof(double);
  if (need && (!d_work || work_bytes < need))
    return fail(RMSF_ENOMEM, "rmsf_covariance_accumulate: workspace too small");
  const int direct = pl.n_ks == 1;
  double *work = static_cast<double *>(d_work);
  const dim3 grid((unsigned)pl.n_pairs, (unsigned)pl.n_ks), block(kBlock);
#define COV_LAUNCH(A_, G_)                                                                                      \
  hipLaunchKernelGGL((k_cov_tiles<A_, G_>), grid, block, 0, S(stream), d_xyz, fstride, n_frames, n_sel, d_sel, \
                     d_xform, d_refinfo, d_shift, d_cov, ld, d_t1, work, pl.n_tiles, pl.n_pairs, pl.ks_frames, direct)
  const bool al = d_xform != nullptr, g = d_sel != nullptr;
  if (al && g) COV_LAUNCH(true, true);
  else if (al) COV_LAUNCH(true, false);
  else if (g) COV_LAUNCH(false, true);
  else COV_LAUNCH(false, false);
#undef COV_LAUNCH
  if (int rc = after_launch("k_cov_tiles")) return rc;
  if (!direct) {
    const dim3 fgrid((unsigned)(pl.n_pairs + pl.n_tiles), (kTile + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_cov_fold, fgrid, block, 0, S(stream), work, n_sel, pl.n_tiles, pl.n_pairs, pl.n_ks, d_cov,
                       ld, d_t1);
    if (int rc = after_launch("k_cov_fold")) return rc;
  }
  return RMSF_OK;
}

RMSF_EXPORT int rmsf_covariance_finish(double *d_cov, int64_t ld, const double *d_t1, int64_t n_coord,
                                       int64_t n_frames, void *stream) {
  if (!d_cov || !d_t1 || n_coord < 1 || ld < n_coord)
    return fail(RMSF_EINVAL, "rmsf_covariance_finish: bad arguments");
  if (n_frames < 1) return fail(RMSF_EEMPTY, "rmsf_covariance_finish: no frames");
  const int64_t nb = (n_coord + 31) / 32;
  if (nb > 65535) return fail(RMSF_EINVAL, "rmsf_covariance_finish: n_coord too large for one launch");
  hipLaunchKernelGGL(k_cov_finish, dim3((unsigned)nb, (unsigned)nb), dim3(kBlock), 0, S(stream), d_cov, ld, d_t1,
                     n_coord, (double)n_frames);
  return after_launch("k_cov_finish");
}

}  // extern "C"
