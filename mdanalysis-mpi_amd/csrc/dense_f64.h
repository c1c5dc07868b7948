// dense_f64.h -- what the dense f64 MFMA contractions (covariance.hip,
// pairwise.hip, pca_project.hip, pca_backproject.hip, eigen_block.hip) have in common: the workgroup's shape, the
// 3 x 3 block of v_mfma_f64_16x16x4_f64 and its wave-order sum, the split-K
// plan and the upper block triangle's pair index.  Staging, pipelining and
// the fold kernels differ for reasons DESIGN.md records and stay in each file.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

constexpr int kBlock = 256;           // threads a workgroup
constexpr int kWaves = kBlock / 64;
constexpr int kLdsLimit = 64 * 1024;  // bytes of LDS a workgroup may declare on gfx950

typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void zero_3x3(f64x4 (&acc)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
}

// acc[i][j] += a_i b_j over one k-step of four: the nine MFMAs in row order.
// Lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; the
// result D has col = l & 15, row = (l >> 4) + 4 reg.
__device__ __forceinline__ void mfma_3x3(f64x4 (&acc)[3][3], double a0, double a1, double a2, double b0, double b1,
                                         double b2) {
  acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
  acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
  acc[0][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b2, acc[0][2], 0, 0, 0);
  acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
  acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  acc[1][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b2, acc[1][2], 0, 0, 0);
  acc[2][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b0, acc[2][0], 0, 0, 0);
  acc[2][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b1, acc[2][1], 0, 0, 0);
  acc[2][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, acc[2][2], 0, 0, 0);
}

// The four waves' accumulators, summed in wave order through LDS: wave 0
// stores, waves 1..3 add in turn.  Every wave maps lane -> element alike, so
// a lane only meets its own.  at(i, j, row, col) is where element (row, col)
// of MFMA tile (i, j) lands in sm.  lane and wave are the kernel's own values
// (recomputed here from threadIdx, the compiler no longer pairs the LDS
// accesses).  Called by every thread; ends on a barrier.  NJ: the column
// tiles held (3, or fewer where a kernel is built for narrower panels).
template <int N, int NJ, class At>
__device__ __forceinline__ void wave_sum_3x3(const f64x4 (&acc)[3][NJ], double (&sm)[N], int lane, int wave,
                                             At at) {
  for (int w = 0; w < kWaves; ++w) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int e = at(i, j, (lane >> 4) + 4 * r, lane & 15);
            sm[e] = w == 0 ? acc[i][j][r] : sm[e] + acc[i][j][r];
          }
    }
    __syncthreads();
  }
}

// Split-K: `stages` contraction stages over up to target_groups / groups
// ranges of at least min_stages each, evenly, with no empty range.
struct SplitK {
  int64_t n_ks;  // ranges
  int64_t per;   // stages per range
};

inline SplitK split_k(int64_t stages, int64_t groups, int64_t target_groups, int64_t min_stages) {
  const int64_t ks = std::max<int64_t>(1, std::min<int64_t>(stages / min_stages, target_groups / groups));
  const int64_t per = (stages + ks - 1) / ks;
  return {(stages + per - 1) / per, per};
}

// pair index -> (I, J), J >= I, rows of the upper block triangle in order.
// Row I starts at I n - I (I - 1) / 2; the root of that quadratic, then a
// step either way for its rounding.
__host__ __device__ __forceinline__ void pair_to_tiles(int64_t p, int64_t n_tiles, int64_t &I, int64_t &J) {
  const double b = 2.0 * (double)n_tiles + 1.0;
  int64_t i = (int64_t)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
  if (i < 0) i = 0;
  if (i > n_tiles - 1) i = n_tiles - 1;
  while (i > 0 && i * n_tiles - i * (i - 1) / 2 > p) --i;
  while (i + 1 < n_tiles && (i + 1) * n_tiles - (i + 1) * i / 2 <= p) ++i;
  I = i;
  J = i + (p - (i * n_tiles - i * (i - 1) / 2));
}
