// lagged.hip -- the time-lagged co-moment matrix of the (aligned) coordinates
// on the f64 matrix cores of gfx950 (MI355X, CDNA4), and the extern "C"
// launchers declared in include/rmsf_hip.h: the contraction of TICA.
//
//   S[i][j] += sum_p d_i(a_p) d_j(b_p),  d = f64(x) - shift
//
// where a_p and b_p are the two frames of pair p -- frame p of operand A and
// frame p of operand B, each with its own base pointer, frame stride and
// transform records: the caller offsets B by the lag -- and x is the selected
// atom's three floats, through apply_xform (rmsf_device.h, the very code the
// Welford and covariance sweeps run) when transform records are given.
// covariance.hip's contraction with its two operands apart in time: S != S^T,
// so there is no triangle to save and no diagonal shortcut.
//
//   * k_lag_tiles   one workgroup per (macro tile I, macro tile J, pair
//                   range) of the full square: 16 atoms = 48 coordinates a
//                   side, 3 x 3 tiles of v_mfma_f64_16x16x4_f64 per wave.  The
//                   deviations of 32 pairs are staged as f64 [k][coord] in
//                   LDS, both operands always; each of the 4 waves contracts 8.
//   * k_lag_fold    the split-K partials, summed in pair-range order.
//   * k_lag_finish  M = S + S^T - T T^T / m in place, each sum computed once.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dense_f64.h"
#include "rmsf_device.h"
#include "rmsf_host.h"

namespace {

constexpr int kTA = 16;                // atoms a side of a macro tile
constexpr int kTC = 3 * kTA;           // coordinates a side: 3 MFMA tiles
constexpr int kKT = 32;                // pairs staged at a time (8 per wave: 2 MFMA k-steps)
constexpr int kTile = kTC * kTC;       // results of a macro tile
constexpr int kFrameLanes = kBlock / kTA;  // pairs staged per pass (one atom per lane)
constexpr int64_t kTargetGroups = 512;     // 2 resident workgroups per CU on MI355X

static_assert(sizeof(double) * (2 * kKT * kTC + 2 * kKT * kRec) <= kLdsLimit, "sm and both operands' sxf fit");
static_assert(kTile <= 2 * kKT * kTC, "the waves' sum fits in sm");

// The work decomposition, a function of (n_sel, n_pairs) alone, so the
// workspace layout and the summation order are fixed by the batching.
struct LagPlan {
  int64_t n_tiles;    // macro tiles a side
  int64_t n_groups;   // n_tiles^2: the full square
  int64_t n_ks;       // pair ranges (split-K); 1 = results go straight to d_s
  int64_t ks_pairs;   // pairs per range, a multiple of kKT
};

LagPlan lag_plan(int64_t n_sel, int64_t n_pairs) {
  LagPlan p;
  p.n_tiles = (n_sel + kTA - 1) / kTA;
  p.n_groups = p.n_tiles * p.n_tiles;
  const SplitK k = split_k(std::max<int64_t>(1, (n_pairs + kKT - 1) / kKT), p.n_groups, kTargetGroups, 1);
  p.n_ks = k.n_ks;
  p.ks_pairs = k.per * kKT;
  return p;
}

size_t lag_work_doubles(const LagPlan &p) {
  if (p.n_ks <= 1) return 0;
  return (size_t)p.n_ks * (size_t)p.n_groups * kTile;
}

// One workgroup: tile (I, J) = blockIdx.x, pairs [blockIdx.y ks_pairs, ...).
// Staging as k_cov_tiles: lane (tid & 15) owns one atom of the tile, (tid >> 4)
// one of 16 pairs per pass; operand 0 is tile I of frame a_p, operand 1 tile J
// of frame b_p, and their deviations go to sm[op][k][3 atom + c].
template <bool ALIGN, bool GATHER>
__global__ __launch_bounds__(kBlock, 2) void k_lag_tiles(const float *__restrict__ xyz_a, int64_t fstride_a,
                                                      const float *__restrict__ xyz_b, int64_t fstride_b,
                                                      int64_t n_pairs, int64_t n_sel,
                                                      const int32_t *__restrict__ sel,
                                                      const double *__restrict__ xform_a,
                                                      const double *__restrict__ xform_b,
                                                      const double *__restrict__ refinfo,
                                                      const double *__restrict__ shift, double *__restrict__ s,
                                                      int64_t ld, double *__restrict__ work, int64_t n_tiles,
                                                      int64_t ks_pairs, int direct) {
  __shared__ double sm[2 * kKT * kTC];                // A then B deviations; reused for the waves' sum
  __shared__ double sxf[ALIGN ? 2 * kKT * kRec : 1];  // the staged frames' transform records, A then B

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ta = tid & (kTA - 1), tf = tid >> 4;
  const int64_t group = blockIdx.x, ks = blockIdx.y;
  const int64_t I = group / n_tiles, J = group % n_tiles;
  const int64_t n_coord = 3 * n_sel;

  const int64_t f0 = ks * ks_pairs;
  const int64_t f1 = f0 + ks_pairs < n_pairs ? f0 + ks_pairs : n_pairs;

  // The lane's atom of each operand tile: a lane past the selection's end
  // reads the last atom instead (and a pair past the range's end the last
  // pair), so every load is unconditional and in bounds; its deviation is
  // zeroed after.
  const float *p_op[2];
  int64_t fs[2] = {fstride_a, fstride_b};
  double sh[2][3];
  bool live[2];
#pragma unroll
  for (int op = 0; op < 2; ++op) {
    const int64_t a = kTA * (op ? J : I) + ta;
    live[op] = a < n_sel;
    const int64_t ac = live[op] ? a : n_sel - 1;
    p_op[op] = (op ? xyz_b : xyz_a) + 3 * (GATHER ? (int64_t)sel[ac] : ac);
    sh[op][0] = shift[3 * ac], sh[op][1] = shift[3 * ac + 1], sh[op][2] = shift[3 * ac + 2];
  }
  const double rc0 = ALIGN ? refinfo[0] : 0.0, rc1 = ALIGN ? refinfo[1] : 0.0, rc2 = ALIGN ? refinfo[2] : 0.0;

  f64x4 acc[3][3];
  zero_3x3(acc);

  const double *sA = sm;
  const double *sB = sm + kKT * kTC;

  // The next stage's floats and records are loaded into registers before the
  // current stage's MFMAs, so the global-load latency runs under the matrix
  // pipe; the records are parked in LDS (sxf) once the MFMAs are issued.
  constexpr int kPasses = kKT / kFrameLanes;
  constexpr int kRecLoads = (kKT * kRec + kBlock - 1) / kBlock;
  float raw[2][kPasses][3];
  double recv[2][kRecLoads];
  auto prefetch = [&](int64_t fb) {
    if (ALIGN) {
#pragma unroll
      for (int op = 0; op < 2; ++op) {
        const double *__restrict__ xf = op ? xform_b : xform_a;
#pragma unroll
        for (int r = 0; r < kRecLoads; ++r) {
          const int e = (r * kBlock + tid) % (kKT * kRec);  // (the last round wraps: its extra lanes reload)
          const int64_t f = fb + e / kRec;
          recv[op][r] = xf[(f < f1 ? f : f1 - 1) * kXform + e % kRec];
        }
      }
    }
#pragma unroll
    for (int pass = 0; pass < kPasses; ++pass) {
      const int64_t f = fb + pass * kFrameLanes + tf;
      const int64_t fc = f < f1 ? f : f1 - 1;
#pragma unroll
      for (int op = 0; op < 2; ++op) {
        const float *__restrict__ q = p_op[op] + fc * fs[op];
        raw[op][pass][0] = q[0], raw[op][pass][1] = q[1], raw[op][pass][2] = q[2];
      }
    }
  };
  auto park_records = [&]() {
    if (ALIGN) {
#pragma unroll
      for (int op = 0; op < 2; ++op)
#pragma unroll
        for (int r = 0; r < kRecLoads; ++r) {
          const int e = r * kBlock + tid;
          if (e < kKT * kRec) sxf[op * kKT * kRec + e] = recv[op][r];
        }
    }
  };
  prefetch(f0);
  park_records();
  __syncthreads();

  for (int64_t fb = f0; fb < f1; fb += kKT) {
    // ---- stage kKT pairs of both operand tiles (zeros past either edge)
#pragma unroll
    for (int op = 0; op < 2; ++op) {
#pragma unroll
      for (int pass = 0; pass < kPasses; ++pass) {
        const int k = pass * kFrameLanes + tf;
        const int64_t f = fb + k;
        const bool on = live[op] && f < f1;
        float x = raw[op][pass][0], y = raw[op][pass][1], z = raw[op][pass][2];
        if (ALIGN) apply_xform(x, y, z, sxf + (op * kKT + k) * kRec, rc0, rc1, rc2);
        double *__restrict__ o = sm + (op * kKT + k) * kTC + 3 * ta;
        o[0] = on ? (double)x - sh[op][0] : 0.0;
        o[1] = on ? (double)y - sh[op][1] : 0.0;
        o[2] = on ? (double)z - sh[op][2] : 0.0;
      }
    }
    __syncthreads();
    // (after the barrier: its fence waits for every load in flight)
    if (fb + kKT < f1) prefetch(fb + kKT);
    // ---- contract: wave w takes rows [8 w, 8 w + 8) of the staged tiles
#pragma unroll
    for (int st = 0; st < kKT / (4 * kWaves); ++st) {
      const int k = (kKT / kWaves) * wave + 4 * st + (lane >> 4);
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

  if (direct) {
    for (int e = tid; e < kTile; e += kBlock) {
      const int64_t i = kTC * I + e / kTC, j = kTC * J + e % kTC;
      if (i < n_coord && j < n_coord) s[i * ld + j] += sm[e];
    }
  } else {
    double *__restrict__ w = work + ((int64_t)ks * gridDim.x + group) * kTile;
    for (int e = tid; e < kTile; e += kBlock) w[e] = sm[e];
  }
}

// d_s += the n_ks partials of every element, in pair-range order.
// Workgroups (tile, ninth of the tile).
__global__ __launch_bounds__(kBlock) void k_lag_fold(const double *__restrict__ work, int64_t n_sel, int64_t n_tiles,
                                                     int64_t n_groups, int64_t n_ks, double *__restrict__ s,
                                                     int64_t ld) {
  const int64_t n_coord = 3 * n_sel;
  const int64_t group = blockIdx.x;
  const int64_t I = group / n_tiles, J = group % n_tiles;
  const int e = blockIdx.y * kBlock + threadIdx.x;
  if (e >= kTile) return;
  const int64_t i = kTC * I + e / kTC, j = kTC * J + e % kTC;
  if (i >= n_coord || j >= n_coord) return;
  const double *__restrict__ w = work + group * kTile + e;
  double sum = 0.0;
  for (int64_t k = 0; k < n_ks; ++k) sum += w[k * n_groups * kTile];
  s[i * ld + j] += sum;
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

}  // namespace

extern "C" {

RMSF_EXPORT size_t rmsf_lagged_comoment_workspace_bytes(int64_t n_sel, int64_t n_pairs) {
  if (n_sel < 1 || n_pairs < 1) return 0;
  return lag_work_doubles(lag_plan(n_sel, n_pairs)) * sizeof(double);
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
  const LagPlan pl = lag_plan(n_sel, n_pairs);
  if (pl.n_groups > INT32_MAX || pl.n_ks > 65535)
    return fail(RMSF_EINVAL, "rmsf_lagged_comoment_accumulate: selection or batch too large for one launch");
  const size_t need = lag_work_doubles(pl) * sizeof(double);
  if (need && (!d_work || work_bytes < need))
    return fail(RMSF_ENOMEM, "rmsf_lagged_comoment_accumulate: workspace too small");
  const int direct = pl.n_ks == 1;
  double *work = static_cast<double *>(d_work);
  const dim3 grid((unsigned)pl.n_groups, (unsigned)pl.n_ks), block(kBlock);
#define LAG_LAUNCH(A_, G_)                                                                                       \
  hipLaunchKernelGGL((k_lag_tiles<A_, G_>), grid, block, 0, S(stream), d_xyz_a, fstride_a, d_xyz_b, fstride_b, \
                     n_pairs, n_sel, d_sel, d_xform_a, d_xform_b, d_refinfo, d_shift, d_s, ld, work, pl.n_tiles, \
                     pl.ks_pairs, direct)
  const bool al = d_xform_a != nullptr, g = d_sel != nullptr;
  if (al && g) LAG_LAUNCH(true, true);
  else if (al) LAG_LAUNCH(true, false);
  else if (g) LAG_LAUNCH(false, true);
  else LAG_LAUNCH(false, false);
#undef LAG_LAUNCH
  if (int rc = after_launch("k_lag_tiles")) return rc;
  if (!direct) {
    const dim3 fgrid((unsigned)pl.n_groups, (kTile + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_lag_fold, fgrid, block, 0, S(stream), work, n_sel, pl.n_tiles, pl.n_groups, pl.n_ks, d_s,
                       ld);
    if (int rc = after_launch("k_lag_fold")) return rc;
  }
  return RMSF_OK;
}

RMSF_EXPORT int rmsf_lagged_comoment_finish(double *d_s, int64_t ld, const double *d_t, int64_t n_coord, int64_t m,
                                            void *stream) {
  if (!d_s || !d_t || n_coord < 1 || ld < n_coord)
    return fail(RMSF_EINVAL, "rmsf_lagged_comoment_finish: bad arguments");
  if (m < 1) return fail(RMSF_EEMPTY, "rmsf_lagged_comoment_finish: no frames");
  const int64_t nb = (n_coord + 31) / 32;
  if (nb > 65535) return fail(RMSF_EINVAL, "rmsf_lagged_comoment_finish: n_coord too large for one launch");
  hipLaunchKernelGGL(k_lag_finish, dim3((unsigned)nb, (unsigned)nb), dim3(kBlock), 0, S(stream), d_s, ld, d_t,
                     n_coord, (double)m);
  return after_launch("k_lag_finish");
}

}  // extern "C"
