// ubench_mfma_f64.hip -- issue rate of v_mfma_f64_16x16x4_f64 on gfx950: the
// yardstick the covariance kernel (csrc/covariance.hip) is quoted against.
// Back-to-back MFMAs on NACC independent accumulators, W waves per SIMD on
// every CU; prints ns, TFLOP/s (2 * 16 * 16 * 4 FLOP each) and the cycles per
// MFMA per SIMD at the device's reported clock.
//   hipcc -O3 --offload-arch=gfx950 tools/ubench_mfma_f64.hip -o tools/ubench_mfma_f64
//   tools/ubench_mfma_f64 [iters]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define CHECK(e)                                                                  \
  do {                                                                            \
    hipError_t r_ = (e);                                                          \
    if (r_ != hipSuccess) {                                                       \
      fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_));                     \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

template <int NACC>
__global__ __launch_bounds__(1024) void k_mfma(double *out, int iters, double a0, double b0) {
  f64x4 acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
  const double a = a0 + threadIdx.x, b = b0 - threadIdx.x;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
  }
  f64x4 s = acc[0];
#pragma unroll
  for (int i = 1; i < NACC; ++i) s += acc[i];
  if (s[0] + s[1] + s[2] + s[3] == 12345.678) out[blockIdx.x] = s[0];  // keeps the chain alive
}

template <int NACC>
int run(int waves_per_simd, int iters, int cus, double ghz, double *d_out) {
  const int block = 64 * 4 * waves_per_simd;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  float best = 1e30f;
  for (int rep = 0; rep < 6; ++rep) {  // the first launches warm the clocks
    CHECK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(k_mfma<NACC>, dim3(cus), dim3(block), 0, 0, d_out, iters, 1.0, 2.0);
    CHECK(hipEventRecord(e1, 0));
    CHECK(hipEventSynchronize(e1));
    float ms;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (rep >= 2 && ms < best) best = ms;
  }
  const double n_mfma_simd = (double)iters * NACC * waves_per_simd;  // per SIMD
  const double flop = n_mfma_simd * 4.0 * cus * 2.0 * 16 * 16 * 4;
  printf("acc=%d waves/SIMD=%d: %.3f ms, %.2f TFLOP/s, %.2f cycles/MFMA/SIMD at %.2f GHz\n", NACC, waves_per_simd,
         best, flop / (best * 1e-3) / 1e12, best * 1e-3 * ghz * 1e9 / n_mfma_simd, ghz);
  return 0;
}

int main(int argc, char **argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 20000;
  hipDeviceProp_t p;
  CHECK(hipGetDeviceProperties(&p, 0));
  const double ghz = p.clockRate * 1e-6;
  printf("%s: %d CUs, %.2f GHz\n", p.name, p.multiProcessorCount, ghz);
  double *d_out;
  CHECK(hipMalloc(&d_out, sizeof(double) * p.multiProcessorCount));
  if (run<1>(1, iters, p.multiProcessorCount, ghz, d_out)) return 1;  // dependent chain: the latency
  if (run<4>(1, iters, p.multiProcessorCount, ghz, d_out)) return 1;
  if (run<9>(1, iters, p.multiProcessorCount, ghz, d_out)) return 1;  // the covariance kernel's 3 x 3
  if (run<9>(2, iters, p.multiProcessorCount, ghz, d_out)) return 1;
  CHECK(hipFree(d_out));
  return 0;
}
