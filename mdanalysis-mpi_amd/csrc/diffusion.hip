// diffusion.hip -- the two passes DiffusionMap(solver="device") adds to the
// device eigen-solver (rmsf_amd/eigen.py, KernelOps; DESIGN §4, "Diffusion map
// on the device"), for gfx950 (MI355X, CDNA4), and their extern "C" launchers.
//
//   * k_diffusion_rows    the distance matrix in HBM becomes the diffusion
//                         kernel in place, K = exp(-(d d) / epsilon), and each
//                         row's sum of K goes to d_rowsum: one read and one
//                         write of the matrix, HBM-bound.  One workgroup a
//                         row, every wave on whole 1 KiB (512 B where a row is
//                         not 16-byte aligned) pieces of it, kDiffUnroll loads
//                         in flight per lane.
//   * k_block_scale_rows  C = diag(s) A for a block of at most 48 columns:
//                         plain VALU, one lane per column, as k_block_update.
//
// The argument is -(d * d) / epsilon with a true division, as numpy evaluates
// it: the same bits go into either exp.  The transform is element-wise, so a
// matrix symmetric in its bits stays so (k_symm_tiles' precondition).  The row
// sums have a fixed order and no atomics: a lane adds its own terms in column
// order, the 64 lanes meet in a halving tree of shuffles, the waves' sums are
// added in wave order.
#include <cmath>
#include <cstdint>

#include "rmsf_host.h"

namespace {

constexpr int kWave = 64;
// waves a row, and the loads each lane has in flight (overridable for A/B builds: tools/build_ab.sh).
// Measured and left alone: 2-16 waves x 2-8 loads are within 4 % of each other at 4,096-60,000 frames
// (tools/ab_diffusion_pass.py, profiles/diffusion_pass_variants.json; DESIGN §4 "Diffusion map on the device").
#ifndef RMSF_DIFF_WAVES
#define RMSF_DIFF_WAVES 4
#endif
#ifndef RMSF_DIFF_UNROLL
#define RMSF_DIFF_UNROLL 4
#endif
constexpr int kDiffWaves = RMSF_DIFF_WAVES;
constexpr int kDiffBlock = kDiffWaves * kWave;
constexpr int kDiffUnroll = RMSF_DIFF_UNROLL;
constexpr int kScaleBlock = 256;
constexpr int kScaleWaves = kScaleBlock / kWave;
constexpr int kScaleRows = 32;  // rows of C a workgroup of k_block_scale_rows writes
constexpr int kCols = 48;       // the widest block (csrc/eigen_block.hip)

typedef double f64x2 __attribute__((ext_vector_type(2)));

// d = 0 gives exp(-0.0) = 1; d = +-inf gives exp(-inf) = 0; an argument below
// the underflow point gives 0; a NaN stays a NaN.
__device__ __forceinline__ double kernel_value(double d, double epsilon) { return exp(-(d * d) / epsilon); }

// V doubles per lane and access.  V = 2 needs every row 16-byte aligned (m
// itself, and an even ld); the row's last element, when n is odd, is then the
// last term of the lane whose pair it would have begun.  Columns >= n are
// neither read nor written.  In place: a lane writes what it alone has read.
template <int V>
__global__ __launch_bounds__(kDiffBlock) void k_diffusion_rows(double *m, int64_t ld, int64_t n, double epsilon,
                                                               double *__restrict__ rowsum) {
  __shared__ double s_sum[kDiffWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row = blockIdx.x;
  double *r = m + row * ld;
  double s = 0.0;
  if (V == 2) {
    const int64_t n_pairs = n >> 1;
    int64_t p = tid;
    for (; p + (int64_t)(kDiffUnroll - 1) * kDiffBlock < n_pairs; p += (int64_t)kDiffUnroll * kDiffBlock) {
      f64x2 v[kDiffUnroll];
#pragma unroll
      for (int u = 0; u < kDiffUnroll; ++u)
        v[u] = *reinterpret_cast<const f64x2 *>(r + 2 * (p + (int64_t)u * kDiffBlock));
#pragma unroll
      for (int u = 0; u < kDiffUnroll; ++u) {
        v[u].x = kernel_value(v[u].x, epsilon);
        v[u].y = kernel_value(v[u].y, epsilon);
        s += v[u].x;
        s += v[u].y;
        *reinterpret_cast<f64x2 *>(r + 2 * (p + (int64_t)u * kDiffBlock)) = v[u];
      }
    }
    for (; p < n_pairs; p += kDiffBlock) {
      f64x2 v = *reinterpret_cast<const f64x2 *>(r + 2 * p);
      v.x = kernel_value(v.x, epsilon);
      v.y = kernel_value(v.y, epsilon);
      s += v.x;
      s += v.y;
      *reinterpret_cast<f64x2 *>(r + 2 * p) = v;
    }
    if ((n & 1) && tid == (int)(n_pairs % kDiffBlock)) {
      const double v = kernel_value(r[n - 1], epsilon);
      s += v;
      r[n - 1] = v;
    }
  } else {
    int64_t c = tid;
    for (; c + (int64_t)(kDiffUnroll - 1) * kDiffBlock < n; c += (int64_t)kDiffUnroll * kDiffBlock) {
      double v[kDiffUnroll];
#pragma unroll
      for (int u = 0; u < kDiffUnroll; ++u) v[u] = r[c + (int64_t)u * kDiffBlock];
#pragma unroll
      for (int u = 0; u < kDiffUnroll; ++u) {
        v[u] = kernel_value(v[u], epsilon);
        s += v[u];
        r[c + (int64_t)u * kDiffBlock] = v[u];
      }
    }
    for (; c < n; c += kDiffBlock) {
      const double v = kernel_value(r[c], epsilon);
      s += v;
      r[c] = v;
    }
  }
  for (int d = kWave / 2; d > 0; d >>= 1) s += __shfl_down(s, d);
  if (lane == 0) s_sum[wave] = s;
  __syncthreads();
  if (tid == 0) {
    double sum = s_sum[0];
    for (int k = 1; k < kDiffWaves; ++k) sum += s_sum[k];
    rowsum[row] = sum;
  }
}

// C = diag(s) A.  One workgroup: kScaleRows rows of C; wave w takes every
// fourth row, lane = column.  c may be a itself (each element is read, then
// written, by one lane).
__global__ __launch_bounds__(kScaleBlock) void k_block_scale_rows(const double *__restrict__ s, const double *a,
                                                                  int64_t lda, int64_t n, int64_t nc, double *c,
                                                                  int64_t ldc) {
  const int col = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (col >= nc) return;
  const int64_t r0 = (int64_t)blockIdx.x * kScaleRows;
  for (int i = wave; i < kScaleRows; i += kScaleWaves) {
    const int64_t r = r0 + i;
    if (r >= n) break;
    c[r * ldc + col] = s[r] * a[r * lda + col];
  }
}

}  // namespace

extern "C" {

RMSF_EXPORT int rmsf_diffusion_kernel(double *d_m, int64_t ld, int64_t n, double epsilon, double *d_rowsum,
                                      void *stream) {
  if (!d_m || !d_rowsum) return fail(RMSF_EINVAL, "rmsf_diffusion_kernel: NULL pointer");
  if (n < 1 || n > INT32_MAX) return fail(RMSF_EINVAL, "rmsf_diffusion_kernel: n must be in 1..INT32_MAX");
  if (ld < n) return fail(RMSF_EINVAL, "rmsf_diffusion_kernel: ld must be >= n");
  if (!(epsilon > 0.0) || !std::isfinite(epsilon))
    return fail(RMSF_EINVAL, "rmsf_diffusion_kernel: epsilon must be positive and finite");
  const bool wide = reinterpret_cast<uintptr_t>(d_m) % 16 == 0 && ld % 2 == 0;
  if (wide)
    hipLaunchKernelGGL(k_diffusion_rows<2>, dim3((unsigned)n), dim3(kDiffBlock), 0, S(stream), d_m, ld, n, epsilon,
                       d_rowsum);
  else
    hipLaunchKernelGGL(k_diffusion_rows<1>, dim3((unsigned)n), dim3(kDiffBlock), 0, S(stream), d_m, ld, n, epsilon,
                       d_rowsum);
  return after_launch("k_diffusion_rows");
}

RMSF_EXPORT int rmsf_block_scale_rows(const double *d_s, const double *d_a, int64_t lda, int64_t n, int64_t nc,
                                      double *d_c, int64_t ldc, void *stream) {
  if (!d_s || !d_a || !d_c) return fail(RMSF_EINVAL, "rmsf_block_scale_rows: NULL pointer");
  if (n < 1 || nc < 1) return fail(RMSF_EINVAL, "rmsf_block_scale_rows: bad sizes");
  if (nc > kCols) return fail(RMSF_EINVAL, "rmsf_block_scale_rows: more than 48 columns");
  if (lda < nc || ldc < nc) return fail(RMSF_EINVAL, "rmsf_block_scale_rows: lda and ldc must be >= nc");
  const int64_t groups = (n + kScaleRows - 1) / kScaleRows;
  if (groups > INT32_MAX) return fail(RMSF_EINVAL, "rmsf_block_scale_rows: block too long for one launch");
  hipLaunchKernelGGL(k_block_scale_rows, dim3((unsigned)groups), dim3(kScaleBlock), 0, S(stream), d_s, d_a, lda, n, nc,
                     d_c, ldc);
  return after_launch("k_block_scale_rows");
}

}  // extern "C"
