// eigen_block.hip -- the three products of a blocked subspace iteration on a
// symmetric f64 matrix that sits in HBM (rmsf_amd/eigen.py: the top modes of
// the positional covariance without leaving the device), for gfx950 (MI355X,
// CDNA4), and the extern "C" launchers declared in include/rmsf_hip.h.  A
// block is a tall, skinny f64 matrix [n][<= 48].
//
//   * k_symm_tiles    Y = M Q, the n^2-sized product, on
//                     v_mfma_f64_16x16x4_f64.  One workgroup per (48 rows of
//                     Y, range of the contraction index); its waves take the
//                     k-steps of four in turn.  M == M^T in its bits, so the
//                     A operand -- rows of M along the lanes -- is read as
//                     columns of M's rows k: 128 contiguous bytes per 16
//                     lanes, straight from HBM into registers, no LDS staging.
//   * k_gram_tiles    G = A^T B, one 48 x 48 block, contracted over the n
//                     rows, which are cut into ranges over the workgroups.
//                     Both run contract_rows, the one load-and-MFMA loop.
//   * k_block_fold    the ranges' partials of either, summed in range order.
//   * k_block_update  C = alpha A + B T with T [<= 48][<= 48]: plain VALU, one
//                     lane per column, T parked in LDS.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dense_f64.h"
#include "rmsf_host.h"

// The constants of k_symm_tiles' plan and pipeline, overridable for A/B builds
// (tools/build_ab.sh NAME -DRMSF_SYMM_...=..., timed by tools/ab_symm_block.py;
// DESIGN §4 "Device eigen-solver" has what was measured).
#ifndef RMSF_SYMM_KSTEPS
#define RMSF_SYMM_KSTEPS 2  // k-steps of a wave whose loads are in flight together
#endif
#ifndef RMSF_SYMM_WAVES_PER_SIMD
#define RMSF_SYMM_WAVES_PER_SIMD 2  // __launch_bounds__' second argument: workgroups a CU the registers must allow
#endif
#ifndef RMSF_SYMM_TARGET_GROUPS
#define RMSF_SYMM_TARGET_GROUPS 1024  // workgroups the k-split aims at: 4 a CU on MI355X
#endif
#ifndef RMSF_SYMM_MIN_STAGES
#define RMSF_SYMM_MIN_STAGES 4  // no k-range under 128 indices: below, the fold costs more
#endif

namespace {

constexpr int kTile = 16;                     // one MFMA tile's side
constexpr int kMaxNT = 3;                     // column tiles of a block
constexpr int kCols = kTile * kMaxNT;         // 48: the widest block
constexpr int kRows = 48;                     // rows of Y a workgroup owns: 3 M tiles
constexpr int kU = RMSF_SYMM_KSTEPS;
constexpr int kStage = 4 * kWaves * kU;       // contraction indices a workgroup takes per turn
constexpr int64_t kTargetGroups = RMSF_SYMM_TARGET_GROUPS;
constexpr int64_t kMinStages = RMSF_SYMM_MIN_STAGES;
constexpr int64_t kGramTargetGroups = 256;    // one gram workgroup a CU at the most
constexpr int kUpdRows = 32;                  // rows of C a workgroup of k_block_update writes

// The work decomposition of Y = M Q, a function of (n, n_cols) alone.
struct SymmPlan {
  int64_t n_rt;    // 48-row tiles
  int n_nt;        // column tiles of Q and Y
  int64_t n_ks;    // ranges of the contraction index; 1 = results go straight to d_y
  int64_t ks_len;  // indices per range, a multiple of kStage
};

SymmPlan symm_plan(int64_t n, int64_t n_cols) {
  SymmPlan p;
  p.n_rt = (n + kRows - 1) / kRows;
  p.n_nt = (int)((n_cols + kTile - 1) / kTile);
  const SplitK k = split_k((n + kStage - 1) / kStage, p.n_rt, kTargetGroups, kMinStages);
  p.n_ks = k.n_ks;
  p.ks_len = k.per * kStage;
  return p;
}

// G = A^T B: the rows are the contraction, cut into n_ks ranges of ks_len.
struct GramPlan {
  int64_t n_ks;
  int64_t ks_len;
};

GramPlan gram_plan(int64_t n) {
  const SplitK k = split_k((n + kStage - 1) / kStage, 1, kGramTargetGroups, kMinStages);
  return {k.n_ks, k.per * kStage};
}

// A lane's column of each of N 16-wide tiles of a row-major matrix: tile t is
// columns [c0 + 16 t, +16), of which `limit` exist.  A column past the end is
// clamped to the last one and marked off, so a load through p is always in
// bounds and what it returns is zeroed where `on` is false.
template <int N>
struct LaneCols {
  const double *p[N];
  bool on[N];
};

template <int N>
__device__ __forceinline__ LaneCols<N> lane_cols(const double *base, int64_t c0, int64_t limit, int lane) {
  LaneCols<N> c;
#pragma unroll
  for (int t = 0; t < N; ++t) {
    const int64_t col = c0 + kTile * t + (lane & 15);
    c.on[t] = col < limit;
    c.p[t] = base + (c.on[t] ? col : limit - 1);
  }
  return c;
}

// acc[t][j] = sum_k A[k][a's tile t] B[k][b's tile j] over the k-steps of
// [k_beg, k_end) that are this wave's: k_beg + 4 wave + 16 s.  MFMA operands
// (16x16x4 f64, dense_f64.h): lane l holds A^T[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15], each one of 16 consecutive doubles of row k:
// straight row reads from global memory into registers, no LDS, no barrier
// (the waves' trip counts may differ).
//
// Every load is unconditional and in bounds: an index past the range's end
// reads the range's last row, a column past the end the last one (LaneCols),
// and what came of it is zeroed where it is used, one turn later (a load whose
// only use sits in a branch beside it is waited for on the spot).  The padding
// of the rows is therefore never read.  The next turn's loads -- kU k-steps
// -- are issued before this turn's MFMAs.
template <int NA, int NB>
__device__ __forceinline__ void contract_rows(const LaneCols<NA> &a, int64_t lda, const LaneCols<NB> &b, int64_t ldb,
                                              int64_t k_beg, int64_t k_end, int lane, int wave,
                                              f64x4 (&acc)[NA][NB]) {
#pragma unroll
  for (int t = 0; t < NA; ++t)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[t][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  double an[kU][NA], bn[kU][NB];
  auto prefetch = [&](int64_t kb) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t k = kb + 4 * kWaves * u + (lane >> 4);
      const int64_t kc = k < k_end ? k : k_end - 1;
#pragma unroll
      for (int t = 0; t < NA; ++t) an[u][t] = a.p[t][kc * lda];
#pragma unroll
      for (int j = 0; j < NB; ++j) bn[u][j] = b.p[j][kc * ldb];
    }
  };
  const int64_t kw = k_beg + 4 * wave;
  prefetch(kw);
  for (int64_t kb = kw; kb < k_end; kb += kStage) {
    double av[kU][NA], bv[kU][NB];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const bool on = kb + 4 * kWaves * u + (lane >> 4) < k_end;
#pragma unroll
      for (int t = 0; t < NA; ++t) av[u][t] = on && a.on[t] ? an[u][t] : 0.0;
#pragma unroll
      for (int j = 0; j < NB; ++j) bv[u][j] = on && b.on[j] ? bn[u][j] : 0.0;
    }
    prefetch(kb + kStage);
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int t = 0; t < NA; ++t)
#pragma unroll
        for (int j = 0; j < NB; ++j)
          acc[t][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][t], bv[u][j], acc[t][j], 0, 0, 0);
  }
}

// where element (row, col) of MFMA tile (i, j) lands in a workgroup's [48][48] LDS tile
struct TileAt {
  __device__ __forceinline__ int operator()(int i, int j, int row, int col) const {
    return (kTile * i + row) * kCols + kTile * j + col;
  }
};

// One workgroup: rows [48 blockIdx.x, +48) of Y, contraction indices
// [blockIdx.y ks_len, ...).  A^T[i][k] = M[row0 + 16 t + i][k] is read as
// M[k][row0 + 16 t + i] (M == M^T in its bits): columns of M's row k.
template <int NT>
__global__ __launch_bounds__(kBlock, RMSF_SYMM_WAVES_PER_SIMD) void k_symm_tiles(
    const double *__restrict__ m, int64_t ldm, int64_t n, const double *__restrict__ q, int64_t ldq, int64_t n_cols,
    double *__restrict__ y, int64_t ldy, double *__restrict__ work, int64_t ks_len, int direct) {
  __shared__ double sm[kRows * kCols];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int64_t k_beg = (int64_t)blockIdx.y * ks_len;
  const int64_t k_end = k_beg + ks_len < n ? k_beg + ks_len : n;

  f64x4 acc[3][NT];
  contract_rows<3, NT>(lane_cols<3>(m, row0, n, lane), ldm, lane_cols<NT>(q, 0, n_cols, lane), ldq, k_beg, k_end, lane,
                       wave, acc);

  wave_sum_3x3(acc, sm, lane, wave, TileAt{});
  for (int e = tid; e < kRows * kTile * NT; e += kBlock) {
    const int row = e / (kTile * NT), col = e % (kTile * NT);
    const int64_t r = row0 + row;
    if (r >= n || col >= n_cols) continue;
    const double v = sm[row * kCols + col];
    if (direct) y[r * ldy + col] = v;
    else work[((int64_t)blockIdx.y * n + r) * n_cols + col] = v;
  }
}

// One workgroup: rows [blockIdx.x ks_len, ...) of A and B, the whole 48 x 48
// block of G = A^T B.
__global__ __launch_bounds__(kBlock, 2) void k_gram_tiles(const double *__restrict__ a_, int64_t lda, int64_t na,
                                                       const double *__restrict__ b_, int64_t ldb, int64_t nb,
                                                       int64_t n, double *__restrict__ g, int64_t ldg,
                                                       double *__restrict__ work, int64_t ks_len, int direct) {
  __shared__ double sm[kCols * kCols];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int64_t k_beg = (int64_t)blockIdx.x * ks_len;
  const int64_t k_end = k_beg + ks_len < n ? k_beg + ks_len : n;

  f64x4 acc[3][3];
  contract_rows<3, 3>(lane_cols<3>(a_, 0, na, lane), lda, lane_cols<3>(b_, 0, nb, lane), ldb, k_beg, k_end, lane, wave,
                      acc);

  wave_sum_3x3(acc, sm, lane, wave, TileAt{});
  for (int e = tid; e < kCols * kCols; e += kBlock) {
    const int row = e / kCols, col = e % kCols;
    if (row >= na || col >= nb) continue;
    if (direct) g[row * ldg + col] = sm[e];
    else work[((int64_t)blockIdx.x * na + row) * nb + col] = sm[e];
  }
}

// d_out[rows][cols] = the n_ks partials of every element, summed in range order.
__global__ __launch_bounds__(kBlock) void k_block_fold(const double *__restrict__ work, int64_t rows, int64_t cols,
                                                       int64_t n_ks, double *__restrict__ out, int64_t ldo) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n = rows * cols;
  if (e >= n) return;
  double s = work[e];
  for (int64_t k = 1; k < n_ks; ++k) s += work[k * n + e];
  out[(e / cols) * ldo + e % cols] = s;
}

// C = alpha A + B T (C = B T when a is NULL).  One workgroup: kUpdRows rows of
// C, T in LDS; wave w takes every fourth row, lane = column, the nb products
// summed in order.  c may be a itself (each element is read, then written, by
// one lane); it is not b.
__global__ __launch_bounds__(kBlock) void k_block_update(double alpha, const double *a, int64_t lda,
                                                         const double *__restrict__ b, int64_t ldb, int64_t nb,
                                                         const double *__restrict__ t, int64_t ldt, int64_t n,
                                                         int64_t nc, double *c, int64_t ldc) {
  __shared__ double st[kCols * kCols];
  const int tid = threadIdx.x;
  for (int e = tid; e < nb * nc; e += kBlock) st[e] = t[(e / nc) * ldt + e % nc];
  __syncthreads();
  const int col = tid & 63, wave = tid >> 6;
  if (col >= nc) return;
  const int64_t r0 = (int64_t)blockIdx.x * kUpdRows;
  for (int i = wave; i < kUpdRows; i += kWaves) {
    const int64_t r = r0 + i;
    if (r >= n) break;
    const double *__restrict__ br = b + r * ldb;
    double s = 0.0;
    for (int j = 0; j < nb; ++j) s += br[j] * st[j * nc + col];
    c[r * ldc + col] = a ? alpha * a[r * lda + col] + s : s;
  }
}

int launch_fold(const char *who, const double *work, int64_t rows, int64_t cols, int64_t n_ks, double *out,
                int64_t ldo, hipStream_t st) {
  const int64_t n_out = rows * cols;
  hipLaunchKernelGGL(k_block_fold, dim3((unsigned)((n_out + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, work, rows,
                     cols, n_ks, out, ldo);
  return after_launch(who);
}

}  // namespace

extern "C" {

RMSF_EXPORT size_t rmsf_symm_block_workspace_bytes(int64_t n, int64_t n_cols) {
  if (n < 1 || n_cols < 1 || n_cols > kCols) return 0;
  const SymmPlan p = symm_plan(n, n_cols);
  return p.n_ks <= 1 ? 0 : (size_t)p.n_ks * (size_t)n * (size_t)n_cols * sizeof(double);
}

RMSF_EXPORT int rmsf_symm_block(const double *d_m, int64_t ldm, int64_t n, const double *d_q, int64_t ldq,
                                int64_t n_cols, double *d_y, int64_t ldy, void *d_work, size_t work_bytes,
                                void *stream) {
  if (!d_m || !d_q || !d_y) return fail(RMSF_EINVAL, "rmsf_symm_block: NULL pointer");
  if (n < 1 || n_cols < 1) return fail(RMSF_EINVAL, "rmsf_symm_block: bad sizes");
  if (n_cols > kCols) return fail(RMSF_EINVAL, "rmsf_symm_block: more than 48 columns");
  if (ldm < n || ldq < n_cols || ldy < n_cols)
    return fail(RMSF_EINVAL, "rmsf_symm_block: ldm must be >= n, ldq and ldy >= n_cols");
  const SymmPlan pl = symm_plan(n, n_cols);
  if (pl.n_rt > INT32_MAX || pl.n_ks > 65535 || (n * n_cols + kBlock - 1) / kBlock > INT32_MAX)
    return fail(RMSF_EINVAL, "rmsf_symm_block: matrix too large for one launch");
  const size_t need = rmsf_symm_block_workspace_bytes(n, n_cols);
  if (need && (!d_work || work_bytes < need)) return fail(RMSF_EINVAL, "rmsf_symm_block: workspace too small");
  const int direct = pl.n_ks == 1;
  double *work = static_cast<double *>(d_work);
  const dim3 grid((unsigned)pl.n_rt, (unsigned)pl.n_ks);
#define SYMM_LAUNCH(NT_)                                                                                      \
  hipLaunchKernelGGL((k_symm_tiles<NT_>), grid, dim3(kBlock), 0, S(stream), d_m, ldm, n, d_q, ldq, n_cols, d_y, \
                     ldy, work, pl.ks_len, direct)
  if (pl.n_nt == 1) SYMM_LAUNCH(1);
  else if (pl.n_nt == 2) SYMM_LAUNCH(2);
  else SYMM_LAUNCH(3);
#undef SYMM_LAUNCH
  if (int rc = after_launch("k_symm_tiles")) return rc;
  if (!direct) return launch_fold("k_block_fold (symm)", work, n, n_cols, pl.n_ks, d_y, ldy, S(stream));
  return RMSF_OK;
}

RMSF_EXPORT size_t rmsf_block_gram_workspace_bytes(int64_t n, int64_t na, int64_t nb) {
  if (n < 1 || na < 1 || nb < 1 || na > kCols || nb > kCols) return 0;
  const GramPlan p = gram_plan(n);
  return p.n_ks <= 1 ? 0 : (size_t)p.n_ks * (size_t)na * (size_t)nb * sizeof(double);
}

RMSF_EXPORT int rmsf_block_gram(const double *d_a, int64_t lda, int64_t na, const double *d_b, int64_t ldb,
                                int64_t nb, int64_t n, double *d_g, int64_t ldg, void *d_work, size_t work_bytes,
                                void *stream) {
  if (!d_a || !d_b || !d_g) return fail(RMSF_EINVAL, "rmsf_block_gram: NULL pointer");
  if (n < 1 || na < 1 || nb < 1) return fail(RMSF_EINVAL, "rmsf_block_gram: bad sizes");
  if (na > kCols || nb > kCols) return fail(RMSF_EINVAL, "rmsf_block_gram: more than 48 columns");
  if (lda < na || ldb < nb || ldg < nb)
    return fail(RMSF_EINVAL, "rmsf_block_gram: lda must be >= na, ldb and ldg >= nb");
  const GramPlan pl = gram_plan(n);
  const size_t need = rmsf_block_gram_workspace_bytes(n, na, nb);
  if (need && (!d_work || work_bytes < need)) return fail(RMSF_EINVAL, "rmsf_block_gram: workspace too small");
  const int direct = pl.n_ks == 1;
  double *work = static_cast<double *>(d_work);
  hipLaunchKernelGGL(k_gram_tiles, dim3((unsigned)pl.n_ks), dim3(kBlock), 0, S(stream), d_a, lda, na, d_b, ldb, nb, n,
                     d_g, ldg, work, pl.ks_len, direct);
  if (int rc = after_launch("k_gram_tiles")) return rc;
  if (!direct) return launch_fold("k_block_fold (gram)", work, na, nb, pl.n_ks, d_g, ldg, S(stream));
  return RMSF_OK;
}

RMSF_EXPORT int rmsf_block_update(double alpha, const double *d_a, int64_t lda, const double *d_b, int64_t ldb,
                                  int64_t nb, const double *d_t, int64_t ldt, int64_t n, int64_t nc, double *d_c,
                                  int64_t ldc, void *stream) {
  if (!d_b || !d_t || !d_c) return fail(RMSF_EINVAL, "rmsf_block_update: NULL pointer");
  if (n < 1 || nb < 1 || nc < 1) return fail(RMSF_EINVAL, "rmsf_block_update: bad sizes");
  if (nb > kCols || nc > kCols) return fail(RMSF_EINVAL, "rmsf_block_update: more than 48 columns");
  if (ldb < nb || ldt < nc || ldc < nc || (d_a && lda < nc))
    return fail(RMSF_EINVAL, "rmsf_block_update: ldb must be >= nb, ldt, ldc and lda >= nc");
  if (d_c == d_b) return fail(RMSF_EINVAL, "rmsf_block_update: d_c must not be d_b");
  const int64_t groups = (n + kUpdRows - 1) / kUpdRows;
  if (groups > INT32_MAX) return fail(RMSF_EINVAL, "rmsf_block_update: block too long for one launch");
  hipLaunchKernelGGL(k_block_update, dim3((unsigned)groups), dim3(kBlock), 0, S(stream), alpha, d_a, lda, d_b, ldb, nb,
                     d_t, ldt, n, nc, d_c, ldc);
  return after_launch("k_block_update");
}

}  // extern "C"
