// covariance.hip -- the two co-moment matrices of the (aligned) coordinates
// on the f64 matrix cores of gfx950 (MI355X, CDNA4), and the extern "C"
// launchers declared in include/rmsf_hip.h.
//
//   positional:   C[i][j] += sum_f d_i(f) d_j(f),  T1[i] += sum_f d_i(f)
//   time-lagged:  S[i][j] += sum_p d_i(a_p) d_j(b_p)
//
// with d = f64(p) - shift, where p is the selected atom's three floats,
// through apply_xform (rmsf_device.h: the transform of RMSF.py:99-101 /
// 133-135, the very code the Welford sweep runs) when transform records are
// given.  The RMSF of RMSF.py:146 is the diagonal of C; its eigenvectors are
// the modes of MDAnalysis.analysis.pca.PCA.  S is the contraction of TICA: a_p
// and b_p are frame p of operand A and frame p of operand B, each with its own
// base pointer, frame stride and transform records (the caller offsets B by
// the lag).  C is symmetric: the upper triangle of tile pairs is computed, a
// diagonal pair stages one operand, and T1 rides along.  S != S^T: the full
// square, both operands always staged, no T1.  Everything else is one body.
//
//   * k_comoment_tiles  one workgroup per (macro tile pair, frame range):
//                       16 atoms = 48 coordinates a side, 3 x 3 tiles of
//                       v_mfma_f64_16x16x4_f64 per wave (9 accumulators of 4
//                       f64).  The deviations of 32 frames are staged as f64
//                       [k][coord] in LDS; each of the 4 waves contracts 8.
//   * k_comoment_fold   the split-K partials, summed in frame-range order.
//   * k_cov_finish      M = C - T1 T1^T / N, mirrored to the full matrix.
//   * k_lag_finish      M = S + S^T - T T^T / m in place, each sum computed once.
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
constexpr int64_t kTargetGroups = 512;     // 2 resident workgroups (134-200 VGPRs) per CU on MI355X

static_assert(sizeof(double) * (2 * kKT * kTC + kFrameLanes * kTC + kKT * kRec) <= kLdsLimit,
              "positional: sm, st1 and sxf fit");
static_assert(sizeof(double) * (2 * kKT * kTC + 2 * kKT * kRec) <= kLdsLimit,
              "time-lagged: sm and both operands' sxf fit");
static_assert(kTile <= 2 * kKT * kTC, "the waves' sum fits in sm");

// One operand of the contraction: its frames and their transform records
// (NULL: unaligned).  The positional matrix has the same operand twice.
struct Operand {
  const float *xyz;
  int64_t fstride;
  const double *xform;
};

// The work decomposition, a function of (n_sel, n_frames) alone, so the
// workspace layout and the summation order are fixed by the batching.
struct Plan {
  int64_t n_tiles;    // macro tiles a side
  int64_t n_groups;   // tile pairs: J >= I (positional) or the full square (time-lagged)
  int64_t n_ks;       // frame ranges (split-K); 1 = results go straight to the matrix
  int64_t ks_frames;  // frames per range, a multiple of kKT
};

Plan comoment_plan(int64_t n_sel, int64_t n_frames, bool lagged) {
  Plan p;
  p.n_tiles = (n_sel + kTA - 1) / kTA;
  p.n_groups = lagged ? p.n_tiles * p.n_tiles : p.n_tiles * (p.n_tiles + 1) / 2;
  const SplitK k = split_k(std::max<int64_t>(1, (n_frames + kKT - 1) / kKT), p.n_groups, kTargetGroups, 1);
  p.n_ks = k.n_ks;
  p.ks_frames = k.per * kKT;
  return p;
}

// (the positional workspace ends on the ranges' T1 partials)
size_t work_doubles(const Plan &p, bool lagged) {
  if (p.n_ks <= 1) return 0;
  return (size_t)p.n_ks * ((size_t)p.n_groups * kTile + (lagged ? 0 : (size_t)p.n_tiles * kTC));
}

// One workgroup: tile pair blockIdx.x, frames [blockIdx.y ks_frames, ...).
// Staging: lane (tid & 15) owns one atom of the tile, (tid >> 4) one of 16
// frames per pass; operand 0 is tile I of a's frame, operand 1 tile J of b's,
// and their three deviations go to sm[op][k][3 atom + c], so an MFMA operand
// (mfma_3x3, dense_f64.h) is 16 consecutive doubles of row k.
template <bool ALIGN, bool GATHER, bool LAGGED>
__global__ __launch_bounds__(kBlock, 2) void k_comoment_tiles(Operand oa, Operand ob_lagged, int64_t n_frames,
                                                           int64_t n_sel, const int32_t *__restrict__ sel,
                                                           const double *__restrict__ refinfo,
                                                           const double *__restrict__ shift,
                                                           double *__restrict__ out, int64_t ld,
                                                           double *__restrict__ t1, double *__restrict__ work,
                                                           int64_t n_tiles, int64_t n_groups, int64_t ks_frames,
                                                           int direct) {
  constexpr int kSets = LAGGED ? 2 : 1;  // operands with transform records of their own
  __shared__ double sm[2 * kKT * kTC];                    // A then B deviations; reused for the waves' sum
  __shared__ double st1[LAGGED ? 1 : kFrameLanes * kTC];  // T1 partials per frame lane
  __shared__ double sxf[ALIGN ? kSets * kKT * kRec : 1];  // the staged frames' transform records (R, mobile COM)

  const Operand &ob = LAGGED ? ob_lagged : oa;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ta = tid & (kTA - 1), tf = tid >> 4;
  const int64_t group = blockIdx.x, ks = blockIdx.y;
  int64_t I, J;
  if (LAGGED) I = group / n_tiles, J = group % n_tiles;
  else pair_to_tiles(group, n_tiles, I, J);
  const bool diag = !LAGGED && I == J;  // one operand to stage, and the tile that owns T1's
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
    p_op[op] = (op ? ob : oa).xyz + 3 * (GATHER ? (int64_t)sel[ac] : ac);
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
  // the same way (load_records / park_records, rmsf_device.h).
  constexpr int kPasses = kKT / kFrameLanes;
  float raw[2][kPasses][3];
  double recv[kSets][rec_loads(kKT, kBlock)];
  auto prefetch = [&](int64_t fb) {
    if (ALIGN) {
#pragma unroll
      for (int op = 0; op < kSets; ++op) load_records<kKT, kBlock>(recv[op], (op ? ob : oa).xform, fb, f1, tid);
    }
#pragma unroll
    for (int pass = 0; pass < kPasses; ++pass) {
      const int64_t f = fb + pass * kFrameLanes + tf;
      const int64_t fc = f < f1 ? f : f1 - 1;
#pragma unroll
      for (int op = 0; op < 2; ++op) {
        const float *__restrict__ q = p_op[op] + fc * (op ? ob : oa).fstride;
        raw[op][pass][0] = q[0], raw[op][pass][1] = q[1], raw[op][pass][2] = q[2];
      }
    }
  };
  auto park = [&]() {
    if (ALIGN) {
#pragma unroll
      for (int op = 0; op < kSets; ++op) park_records<kKT, kBlock>(sxf + op * kKT * kRec, recv[op], tid);
    }
  };
  prefetch(f0);
  park();
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
        if (ALIGN) apply_xform(x, y, z, sxf + ((LAGGED ? op : 0) * kKT + k) * kRec, rc0, rc1, rc2);
        // (each deviation stored as it is formed: with the three formed first, the aligned time-lagged
        // kernel takes 170 VGPRs, not 166, and loses its third wave a SIMD)
        double *__restrict__ o = sm + (op * kKT + k) * kTC + 3 * ta;
        const double d0 = o[0] = on ? (double)x - sh[op][0] : 0.0;
        const double d1 = o[1] = on ? (double)y - sh[op][1] : 0.0;
        const double d2 = o[2] = on ? (double)z - sh[op][2] : 0.0;
        if (!LAGGED && op == 0) ts[0] += d0, ts[1] += d1, ts[2] += d2;
      }
    }
    __syncthreads();
    // (after the barrier: its fence waits for every load in flight)
    if (fb + kKT < f1) prefetch(fb + kKT);
    // ---- contract: wave w takes rows [8 w, 8 w + 8) of the staged tiles
#pragma unroll
    for (int s = 0; s < kKT / (4 * kWaves); ++s) {
      const int k = (kKT / kWaves) * wave + 4 * s + (lane >> 4);
      const double *__restrict__ ra = sA + k * kTC + (lane & 15);
      const double *__restrict__ rb = sB + k * kTC + (lane & 15);
      const double a0 = ra[0], a1 = ra[16], a2 = ra[32];
      const double b0 = rb[0], b1 = rb[16], b2 = rb[32];
      mfma_3x3(acc, a0, a1, a2, b0, b1, b2);
    }
    park();  // this stage's were last read before the barrier above
    __syncthreads();
  }

  // ---- the four waves' accumulators, summed in wave order: row-major [kTC][kTC]
  wave_sum_3x3(acc, sm, lane, wave,
               [](int i, int j, int row, int col) { return (16 * i + row) * kTC + 16 * j + col; });
  if (!LAGGED) {
    if (diag) st1[tf * kTC + 3 * ta] = ts[0], st1[tf * kTC + 3 * ta + 1] = ts[1], st1[tf * kTC + 3 * ta + 2] = ts[2];
    __syncthreads();
  }

  if (direct) {
    for (int e = tid; e < kTile; e += kBlock) {
      const int64_t i = kTC * I + e / kTC, j = kTC * J + e % kTC;
      if (i < n_coord && j < n_coord) out[i * ld + j] += sm[e];
    }
  } else {
    double *__restrict__ w = work + ((int64_t)ks * n_groups + group) * kTile;
    for (int e = tid; e < kTile; e += kBlock) w[e] = sm[e];
  }
  if (diag && tid < kTC) {
    double s = 0.0;
    for (int g = 0; g < kFrameLanes; ++g) s += st1[g * kTC + tid];
    const int64_t i = kTC * I + tid;
    if (direct) {
      if (i < n_coord) t1[i] += s;
    } else {
      work[(int64_t)gridDim.y * n_groups * kTile + ((int64_t)ks * n_tiles + I) * kTC + tid] = s;
    }
  }
}

// out / t1 += the n_ks partials of every element, in frame-range order, from
// 0.0.  Workgroups (tile pair, ninth of the tile); the positional fold has
// n_tiles columns more, which fold T1.
template <bool LAGGED>
__global__ __launch_bounds__(kBlock) void k_comoment_fold(const double *__restrict__ work, int64_t n_sel,
                                                          int64_t n_tiles, int64_t n_groups, int64_t n_ks,
                                                          double *__restrict__ out, int64_t ld,
                                                          double *__restrict__ t1) {
  const int64_t n_coord = 3 * n_sel;
  const int64_t bx = blockIdx.x;
  if (!LAGGED && bx >= n_groups) {
    const int64_t I = bx - n_groups;
    if (blockIdx.y != 0 || threadIdx.x >= kTC) return;
    const int64_t i = kTC * I + threadIdx.x;
    if (i >= n_coord) return;
    const double *__restrict__ w = work + n_ks * n_groups * kTile + I * kTC + threadIdx.x;
    double s = 0.0;
    for (int64_t k = 0; k < n_ks; ++k) s += w[k * n_tiles * kTC];
    t1[i] += s;
    return;
  }
  int64_t I, J;
  if (LAGGED) I = bx / n_tiles, J = bx % n_tiles;
  else pair_to_tiles(bx, n_tiles, I, J);
  const int e = blockIdx.y * kBlock + threadIdx.x;
  if (e >= kTile) return;
  const int64_t i = kTC * I + e / kTC, j = kTC * J + e % kTC;
  if (i >= n_coord || j >= n_coord) return;
  const double *__restrict__ w = work + bx * kTile + e;
  double s = 0.0;
  for (int64_t k = 0; k < n_ks; ++k) s += w[k * n_groups * kTile];
  out[i * ld + j] += s;
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

// M = S + S^T - T T^T / m in place over 32 x 32 blocks: the workgroup of
// (bi, bj), bj >= bi, reads both that block and its mirror image into LDS,
// forms each sum once and stores it to both (through LDS, so both stores run
// along rows): the result is symmetric in its bits.
__global__ __launch_bounds__(kBlock) void k_lag_finish(double *__restrict__ s, int64_t ld,
                                                       const double *__restrict__ t, int64_t n, double m) {
  __shared__ double su[32][33];  // block (bi, bj), then the sums
  __shared__ double sl[32][33];  // block (bj, bi)
  const int64_t bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += kBlock / 32) {
    const int64_t i = 32 * bi + r, j = 32 * bj + tx;
    su[r][tx] = i < n && j < n ? s[i * ld + j] : 0.0;
    const int64_t i2 = 32 * bj + r, j2 = 32 * bi + tx;
    sl[r][tx] = i2 < n && j2 < n ? s[i2 * ld + j2] : 0.0;
  }
  __syncthreads();
  double v[32 / (kBlock / 32)];
#pragma unroll
  for (int q = 0; q < 32 / (kBlock / 32); ++q) {
    const int r = ty + q * (kBlock / 32);
    const int64_t i = 32 * bi + r, j = 32 * bj + tx;
    // on the diagonal block the element below the diagonal takes the one above's operands in its order
    const bool flip = bi == bj && tx < r;
    const double up = flip ? su[tx][r] : su[r][tx], lo = flip ? sl[r][tx] : sl[tx][r];
    v[q] = i < n && j < n ? (up + lo) - t[flip ? j : i] * t[flip ? i : j] / m : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 32 / (kBlock / 32); ++q) su[ty + q * (kBlock / 32)][tx] = v[q];
  __syncthreads();
  for (int r = ty; r < 32; r += kBlock / 32) {
    const int64_t i = 32 * bi + r, j = 32 * bj + tx;
    if (i < n && j < n) s[i * ld + j] = su[r][tx];
    if (bi != bj) {
      const int64_t i2 = 32 * bj + r, j2 = 32 * bi + tx;
      if (i2 < n && j2 < n) s[i2 * ld + j2] = su[tx][r];
    }
  }
}

// The accumulate launch of either matrix, after the entry point (`who` in the
// messages) has checked its own arguments: plan, grid limits, workspace, the
// tile kernel for (aligned, gathered), the fold.
template <bool LAGGED>
int launch_accumulate(const char *who, const Operand &oa, const Operand &ob, int64_t n_frames, int64_t n_sel,
                      const int32_t *d_sel, const double *d_refinfo, const double *d_shift, double *d_out, int64_t ld,
                      double *d_t1, void *d_work, size_t work_bytes, void *stream) {
  const Plan pl = comoment_plan(n_sel, n_frames, LAGGED);
  const int64_t fold_groups = pl.n_groups + (LAGGED ? 0 : pl.n_tiles);
  if (fold_groups > INT32_MAX || pl.n_ks > 65535)
    return fail(RMSF_EINVAL, std::string(who) + ": selection or batch too large for one launch");
  const size_t need = work_doubles(pl, LAGGED) * sizeof(double);
  if (need && (!d_work || work_bytes < need)) return fail(RMSF_ENOMEM, std::string(who) + ": workspace too small");
  const int direct = pl.n_ks == 1;
  double *work = static_cast<double *>(d_work);
  const dim3 grid((unsigned)pl.n_groups, (unsigned)pl.n_ks), block(kBlock);
  const bool al = oa.xform != nullptr, g = d_sel != nullptr;
  const auto tiles = al ? (g ? k_comoment_tiles<true, true, LAGGED> : k_comoment_tiles<true, false, LAGGED>)
                        : (g ? k_comoment_tiles<false, true, LAGGED> : k_comoment_tiles<false, false, LAGGED>);
  hipLaunchKernelGGL(tiles, grid, block, 0, S(stream), oa, ob, n_frames, n_sel, d_sel, d_refinfo, d_shift, d_out, ld,
                     d_t1, work, pl.n_tiles, pl.n_groups, pl.ks_frames, direct);
  if (int rc = after_launch("k_comoment_tiles")) return rc;
  if (!direct) {
    const dim3 fgrid((unsigned)fold_groups, (kTile + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_comoment_fold<LAGGED>, fgrid, block, 0, S(stream), work, n_sel, pl.n_tiles, pl.n_groups,
                       pl.n_ks, d_out, ld, d_t1);
    if (int rc = after_launch("k_comoment_fold")) return rc;
  }
  return RMSF_OK;
}

// Either finish kernel over the n_coord / 32 square of blocks.
int launch_finish(const char *who, void (*kernel)(double *, int64_t, const double *, int64_t, double),
                  const char *kernel_name, double *d_m, int64_t ld, const double *d_t, int64_t n_coord, int64_t count,
                  void *stream) {
  if (!d_m || !d_t || n_coord < 1 || ld < n_coord) return fail(RMSF_EINVAL, std::string(who) + ": bad arguments");
  if (count < 1) return fail(RMSF_EEMPTY, std::string(who) + ": no frames");
  const int64_t nb = (n_coord + 31) / 32;
  if (nb > 65535) return fail(RMSF_EINVAL, std::string(who) + ": n_coord too large for one launch");
  hipLaunchKernelGGL(kernel, dim3((unsigned)nb, (unsigned)nb), dim3(kBlock), 0, S(stream), d_m, ld, d_t, n_coord,
                     (double)count);
  return after_launch(kernel_name);
}

}  // namespace

extern "C" {

// (for the tests: the tile mapping of this kernel and pairwise.hip's, on the host)
RMSF_EXPORT void rmsf_internal_pair_to_tiles(int64_t p, int64_t n_tiles, int64_t *I, int64_t *J) {
  pair_to_tiles(p, n_tiles, *I, *J);
}

RMSF_EXPORT size_t rmsf_covariance_workspace_bytes(int64_t n_sel, int64_t n_frames) {
  if (n_sel < 1 || n_frames < 1) return 0;
  return work_doubles(comoment_plan(n_sel, n_frames, false), false) * sizeof(double);
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
  const Operand o{d_xyz, fstride, d_xform};
  return launch_accumulate<false>("rmsf_covariance_accumulate", o, o, n_frames, n_sel, d_sel, d_refinfo, d_shift,
                                  d_cov, ld, d_t1, d_work, work_bytes, stream);
}

RMSF_EXPORT int rmsf_covariance_finish(double *d_cov, int64_t ld, const double *d_t1, int64_t n_coord,
                                       int64_t n_frames, void *stream) {
  return launch_finish("rmsf_covariance_finish", k_cov_finish, "k_cov_finish", d_cov, ld, d_t1, n_coord, n_frames,
                       stream);
}

RMSF_EXPORT size_t rmsf_lagged_comoment_workspace_bytes(int64_t n_sel, int64_t n_pairs) {
  if (n_sel < 1 || n_pairs < 1) return 0;
  return work_doubles(comoment_plan(n_sel, n_pairs, true), true) * sizeof(double);
}

RMSF_EXPORT int rmsf_lagged_comoment_accumulate(const float *d_xyz_a, int64_t fstride_a, const float *d_xyz_b,
                                                int64_t fstride_b, int64_t n_pairs, int64_t n_sel,
                                                const int32_t *d_sel, const double *d_xform_a,
                                                const double *d_xform_b, const double *d_refinfo,
                                                const double *d_shift, double *d_s, int64_t ld, void *d_work,
                                                size_t work_bytes, void *stream) {
  if (!d_xyz_a || !d_xyz_b || n_sel < 1 || n_pairs < 0 || fstride_a < 0 || fstride_b < 0 || !d_shift || !d_s ||
      ld < 3 * n_sel)
    return fail(RMSF_EINVAL, "rmsf_lagged_comoment_accumulate: bad arguments");
  if ((d_xform_a != nullptr) != (d_xform_b != nullptr))
    return fail(RMSF_EINVAL, "rmsf_lagged_comoment_accumulate: d_xform_a and d_xform_b go together");
  if ((d_xform_a != nullptr) != (d_refinfo != nullptr))
    return fail(RMSF_EINVAL, "rmsf_lagged_comoment_accumulate: the records and d_refinfo go together");
  if (n_pairs == 0) return RMSF_OK;
  return launch_accumulate<true>("rmsf_lagged_comoment_accumulate", Operand{d_xyz_a, fstride_a, d_xform_a},
                                 Operand{d_xyz_b, fstride_b, d_xform_b}, n_pairs, n_sel, d_sel, d_refinfo, d_shift,
                                 d_s, ld, nullptr, d_work, work_bytes, stream);
}

RMSF_EXPORT int rmsf_lagged_comoment_finish(double *d_s, int64_t ld, const double *d_t, int64_t n_coord, int64_t m,
                                            void *stream) {
  return launch_finish("rmsf_lagged_comoment_finish", k_lag_finish, "k_lag_finish", d_s, ld, d_t, n_coord, m, stream);
}

}  // extern "C"
