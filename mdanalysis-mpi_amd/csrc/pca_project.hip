// pca_project.hip -- the projection of a trajectory on principal components
// (MDAnalysis.analysis.pca.PCA.transform) on the f64 matrix cores of gfx950
// (MI355X, CDNA4), and the extern "C" launchers declared in
// include/rmsf_hip.h.
//
//   out[f][c] = sum_i d_i(f) V[i][c],   d = f64(p) - mean
//
// where p is the selected atom's three floats, through apply_xform
// (rmsf_device.h: the transform of RMSF.py:99-101 / 133-135, the very code
// the Welford and covariance sweeps run) when transform records are given.
// The third dense contraction of the domain: covariance.hip contracts over
// the frames, pairwise.hip over the atoms of two frames, this one over the
// coordinates of a tall, skinny product [F x 3n] . [3n x k].
//
//   * k_proj_tiles  one workgroup per (16 frames, panel of up to 48
//                   components, coordinate range): frames are the M side of
//                   v_mfma_f64_16x16x4_f64, components the N side (1-3 tiles,
//                   1-3 accumulators of 4 f64 a wave), coordinates the
//                   contraction.  The deviations of 32 atoms are staged as f64
//                   [coordinate][frame] in LDS; each of the 4 waves contracts
//                   24 of the 96 coordinates.  The rows of V already have B's
//                   shape and are read through L2 into registers.
//   * k_proj_fold   the split-K partials, summed in coordinate-range order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dense_f64.h"
#include "rmsf_device.h"
#include "rmsf_host.h"

namespace {

constexpr int kTF = 16;                    // frames a workgroup: the MFMA's M side
constexpr int kTN = 16;                    // components an N tile
constexpr int kMaxNT = 3;                  // N tiles a workgroup: a panel of 48 components
constexpr int kPanel = kTN * kMaxNT;
constexpr int kTA = 16;                    // atoms staged per pass (one atom per lane, 16 frames)
constexpr int kKA = 32;                    // atoms staged at a time
constexpr int kPasses = kKA / kTA;
constexpr int kKC = 3 * kKA;               // coordinates staged at a time: 24 MFMA k-steps
constexpr int kSteps = kKC / (4 * kWaves); // k-steps a wave and stage
constexpr int kDepth = 2;                  // stages whose frame loads are in flight
constexpr int kLd = kTF + 1;               // doubles a staged coordinate: 16 frames and a pad (the 16 atoms
                                           // a wave stores for one frame then fall on 16 different bank pairs)
constexpr int64_t kTargetGroups = 1024;    // 4 workgroups a CU on MI355X
constexpr int64_t kMinStages = 16;         // no coordinate range under 512 atoms: below, the fold costs more

static_assert(kBlock == kTF * kTA, "one (atom, frame) per thread and pass");
static_assert(kKC % (4 * kWaves) == 0, "whole k-steps a wave");
static_assert(2 * kKC * kLd >= kWaves * kTF * kPanel, "the waves' results fit the staging buffers");
static_assert(sizeof(double) * (2 * kKC * kLd + kTF * kRec) <= kLdsLimit, "sm and sxf fit");

typedef float f32x3 __attribute__((ext_vector_type(3)));

// The barrier between a stage's LDS stores and its LDS reads: every wave
// waits for its own LDS operations, then for the other waves.  Global loads
// stay in flight across it.
__device__ __forceinline__ void stage_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The work decomposition, a function of (n_frames, n_sel, n_comp) alone, so
// the workspace layout and the summation order are fixed by the shapes.
struct ProjPlan {
  int64_t n_ft;      // 16-frame tiles
  int64_t n_pan;     // component panels
  int n_nt;          // N tiles of a panel (the last panel's spare tiles contribute zeros)
  int64_t n_ks;      // coordinate ranges (split-K); 1 = results go straight to d_out
  int64_t ks_atoms;  // atoms per range, a multiple of kKA
};

ProjPlan proj_plan(int64_t n_frames, int64_t n_sel, int64_t n_comp) {
  ProjPlan p;
  p.n_ft = (n_frames + kTF - 1) / kTF;
  p.n_pan = (n_comp + kPanel - 1) / kPanel;
  p.n_nt = (int)std::min<int64_t>(kMaxNT, (n_comp + kTN - 1) / kTN);
  const int64_t stages = std::max<int64_t>(1, (n_sel + kKA - 1) / kKA);
  const int64_t base = std::max<int64_t>(1, p.n_ft * p.n_pan);
  const SplitK k = split_k(stages, base, kTargetGroups, kMinStages);
  p.n_ks = k.n_ks;
  p.ks_atoms = k.per * kKA;
  return p;
}

size_t proj_work_doubles(const ProjPlan &p, int64_t n_frames, int64_t n_comp) {
  if (p.n_ks <= 1) return 0;
  return (size_t)p.n_ks * (size_t)n_frames * (size_t)n_comp;
}

// One workgroup: frames [16 blockIdx.x, +16), components [48 blockIdx.y, +48),
// atoms [blockIdx.z ks_atoms, ...).  Staging: lane (tid & 15) owns one atom
// of the pass, (tid >> 4) one of the 16 frames; its three deviations go to
// s[3 atom + c][frame].  MFMA operands (16x16x4 f64, covariance.hip): lane l
// holds A[i = l & 15][k = l >> 4] = the deviation of frame i at coordinate k,
// one of 16 consecutive doubles of the staged row, and B[k = l >> 4][j = l & 15]
// = V's row k, 16 consecutive doubles of d_comp; the result D has
// col = l & 15 (component), row = (l >> 4) + 4 reg (frame).
//
// The workgroup's frames are the same for every stage, so their transform
// records are parked in LDS once, before the first stage.  The staging
// buffer is double: stage s + 1 is written while a slow wave may still read
// stage s, and one barrier a stage suffices.
template <bool ALIGN, bool GATHER, int NT>
__global__ __launch_bounds__(kBlock, 2) void k_proj_tiles(const float *__restrict__ xyz, int64_t fstride,
                                                       int64_t n_frames, int64_t n_sel,
                                                       const int32_t *__restrict__ sel,
                                                       const double *__restrict__ xform,
                                                       const double *__restrict__ refinfo,
                                                       const double *__restrict__ mean,
                                                       const double *__restrict__ comp, int64_t ldc, int64_t n_comp,
                                                       double *__restrict__ out, int64_t ldo,
                                                       double *__restrict__ work, int64_t ks_atoms, int direct) {
  __shared__ double sm[2 * kKC * kLd];            // two stages of deviations; reused for the waves' results
  __shared__ double sxf[ALIGN ? kTF * kRec : 1];  // the 16 frames' transform records (R, mobile COM)

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ta = tid & (kTA - 1), tf = tid >> 4;
  const int64_t f0 = (int64_t)blockIdx.x * kTF;
  const int64_t n0 = (int64_t)blockIdx.y * kPanel;
  const int64_t a0 = (int64_t)blockIdx.z * ks_atoms;
  const int64_t a1 = a0 + ks_atoms < n_sel ? a0 + ks_atoms : n_sel;

  // Every load is unconditional and in bounds: a frame, atom, coordinate or
  // component past the end reads the last one instead, and what came of it
  // is zeroed afterwards (a load inside a branch is waited for on the spot).
  const bool f_on = f0 + tf < n_frames;
  const float *__restrict__ frame = xyz + (f_on ? f0 + tf : n_frames - 1) * fstride;
  if (ALIGN) {
    for (int e = tid; e < kTF * kRec; e += kBlock) {
      const int64_t f = f0 + e / kRec;
      sxf[e] = xform[(f < n_frames ? f : n_frames - 1) * kXform + e % kRec];
    }
  }
  const double rc0 = ALIGN ? refinfo[0] : 0.0, rc1 = ALIGN ? refinfo[1] : 0.0, rc2 = ALIGN ? refinfo[2] : 0.0;

  // the lane's component of each N tile
  const double *__restrict__ bcol[NT];
  bool c_on[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int64_t c = n0 + kTN * j + (lane & 15);
    c_on[j] = c < n_comp;
    bcol[j] = comp + (c_on[j] ? c : n_comp - 1);
  }

  f64x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};

  // The floats and means of the next kDepth stages, and the rows of V of the
  // next one (an L2 hit, half the wait), are in flight in registers while a
  // stage is staged and contracted, so a stage's floats were asked for two
  // stages earlier; they become deviations in LDS when their turn comes.
  // The stage barrier therefore waits for the LDS stores only
  // (stage_barrier): __syncthreads' fence would drain the loads in flight.
  // V's rows are issued before the floats, so waiting for them (loads return
  // in order) leaves the younger floats in flight.  A gathered selection's
  // indices travel one turn further ahead still, so no row load waits for an
  // index just asked for.  Every prefetch is unconditional -- past the range's
  // end it re-reads the last atom -- and what it loaded is masked where it is
  // used, a stage later: a load whose only use sits in a branch beside it is
  // moved into that branch and waited for on the spot.
  f32x3 raw[kDepth][kPasses];  // (one value an atom: carried round the loop in the registers it was loaded into)
  double mu[kDepth][kPasses][3];
  int32_t ia[kDepth][kPasses];
  double bn[kSteps][NT];
  auto load_idx = [&](int d, int64_t ab) {
#pragma unroll
    for (int pass = 0; pass < kPasses; ++pass) {
      const int64_t a = ab + pass * kTA + ta;
      ia[d][pass] = sel[a < a1 ? a : a1 - 1];
    }
  };
  auto prefetch_a = [&](int d, int64_t ab) {
#pragma unroll
    for (int pass = 0; pass < kPasses; ++pass) {
      const int64_t a = ab + pass * kTA + ta;
      const int64_t ac = a < a1 ? a : a1 - 1;
      const float *__restrict__ q = frame + 3 * (GATHER ? (int64_t)ia[d][pass] : ac);
      __builtin_memcpy(&raw[d][pass], q, sizeof(f32x3));
      mu[d][pass][0] = mean[3 * ac], mu[d][pass][1] = mean[3 * ac + 1], mu[d][pass][2] = mean[3 * ac + 2];
    }
    if (GATHER) load_idx(d, ab + kDepth * kKA);
  };
  auto prefetch_b = [&](int64_t ab) {
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const int64_t i = 3 * ab + (kKC / kWaves) * wave + 4 * s + (lane >> 4);
      const int64_t ic = i < 3 * a1 ? i : 3 * a1 - 1;
#pragma unroll
      for (int j = 0; j < NT; ++j) bn[s][j] = bcol[j][ic * ldc];
    }
  };
  if (GATHER) {
#pragma unroll
    for (int d = 0; d < kDepth; ++d) load_idx(d, a0 + d * kKA);
  }
  prefetch_a(0, a0);
  prefetch_b(a0);
#pragma unroll
  for (int d = 1; d < kDepth; ++d) prefetch_a(d, a0 + d * kKA);
  // The loop is entered with nothing in flight (s_waitcnt vmcnt(0); the
  // records parked above become visible at the barrier): its waits are
  // counted back from the younger loads, and with the first loads still in
  // flight, in another order, the stricter count of the two ways in would hold
  // for every stage.
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();

  int buf = 0;
  for (int64_t ag = a0; ag < a1; ag += kDepth * kKA) {
#pragma unroll
    for (int d = 0; d < kDepth; ++d) {
      const int64_t ab = ag + d * kKA;
      if (ab >= a1) break;  // (the same for every thread of the workgroup)
      double *__restrict__ s_ = sm + buf * (kKC * kLd);
      buf ^= 1;
      double b[kSteps][NT];
#pragma unroll
      for (int s = 0; s < kSteps; ++s) {
        const bool on = 3 * ab + (kKC / kWaves) * wave + 4 * s + (lane >> 4) < 3 * a1;
#pragma unroll
        for (int j = 0; j < NT; ++j) b[s][j] = on && c_on[j] ? bn[s][j] : 0.0;
      }
      // ---- stage kKA atoms of the 16 frames (zeros past either edge)
#pragma unroll
      for (int pass = 0; pass < kPasses; ++pass) {
        const bool on = f_on && ab + pass * kTA + ta < a1;
        float x = raw[d][pass].x, y = raw[d][pass].y, z = raw[d][pass].z;
        if (ALIGN) apply_xform(x, y, z, sxf + tf * kRec, rc0, rc1, rc2);
        double *__restrict__ o = s_ + 3 * (pass * kTA + ta) * kLd + tf;
        o[0] = on ? (double)x - mu[d][pass][0] : 0.0;
        o[kLd] = on ? (double)y - mu[d][pass][1] : 0.0;
        o[2 * kLd] = on ? (double)z - mu[d][pass][2] : 0.0;
      }
      stage_barrier();
      prefetch_b(ab + kKA);
      prefetch_a(d, ab + kDepth * kKA);
      // ---- contract: wave w takes coordinates [24 w, 24 w + 24) of the stage
#pragma unroll
      for (int s = 0; s < kSteps; ++s) {
        const int k = (kKC / kWaves) * wave + 4 * s + (lane >> 4);
        const double a = s_[k * kLd + (lane & 15)];
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[s][j], acc[j], 0, 0, 0);
      }
    }
  }

  // ---- the four waves' accumulators, each to its own LDS tile, then summed
  // in wave order by the thread that writes the element
  __syncthreads();
  double *__restrict__ red = sm + wave * (kTF * kPanel);
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[((lane >> 4) + 4 * r) * kPanel + kTN * j + (lane & 15)] = acc[j][r];
  __syncthreads();
  for (int e = tid; e < kTF * kTN * NT; e += kBlock) {
    const int row = e / (kTN * NT), col = e % (kTN * NT);
    const int64_t f = f0 + row, c = n0 + col;
    if (f >= n_frames || c >= n_comp) continue;
    const double *__restrict__ r = sm + row * kPanel + col;
    const double v = ((r[0] + r[kTF * kPanel]) + r[2 * kTF * kPanel]) + r[3 * kTF * kPanel];
    if (direct) out[f * ldo + c] = v;
    else work[((int64_t)blockIdx.z * n_frames + f) * n_comp + c] = v;
  }
}

// d_out = the n_ks partials of every element, summed in coordinate-range order.
__global__ __launch_bounds__(kBlock) void k_proj_fold(const double *__restrict__ work, int64_t n_frames,
                                                      int64_t n_comp, int64_t n_ks, double *__restrict__ out,
                                                      int64_t ldo) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n = n_frames * n_comp;
  if (e >= n) return;
  double s = work[e];
  for (int64_t k = 1; k < n_ks; ++k) s += work[k * n + e];
  out[(e / n_comp) * ldo + e % n_comp] = s;
}

template <bool A_, bool G_>
void launch_tiles(int nt, dim3 grid, hipStream_t st, const float *d_xyz, int64_t fstride, int64_t n_frames,
                  int64_t n_sel, const int32_t *d_sel, const double *d_xform, const double *d_refinfo,
                  const double *d_mean, const double *d_comp, int64_t ldc, int64_t n_comp, double *d_out, int64_t ldo,
                  double *work, int64_t ks_atoms, int direct) {
#define PROJ_LAUNCH(NT_)                                                                                          \
  hipLaunchKernelGGL((k_proj_tiles<A_, G_, NT_>), grid, dim3(kBlock), 0, st, d_xyz, fstride, n_frames, n_sel,     \
                     d_sel, d_xform, d_refinfo, d_mean, d_comp, ldc, n_comp, d_out, ldo, work, ks_atoms, direct)
  if (nt == 1) PROJ_LAUNCH(1);
  else if (nt == 2) PROJ_LAUNCH(2);
  else PROJ_LAUNCH(3);
#undef PROJ_LAUNCH
}

}  // namespace

extern "C" {

RMSF_EXPORT size_t rmsf_pca_project_workspace_bytes(int64_t n_frames, int64_t n_sel, int64_t n_comp) {
  if (n_frames < 1 || n_sel < 1 || n_comp < 1) return 0;
  return proj_work_doubles(proj_plan(n_frames, n_sel, n_comp), n_frames, n_comp) * sizeof(double);
}

RMSF_EXPORT int rmsf_pca_project(const float *d_xyz, int64_t fstride, int64_t n_frames, int64_t n_sel,
                                 const int32_t *d_sel, const double *d_xform, const double *d_refinfo,
                                 const double *d_mean, const double *d_comp, int64_t ldc, int64_t n_comp,
                                 double *d_out, int64_t ldo, void *d_work, size_t work_bytes, void *stream) {
  if (!d_xyz || !d_mean || !d_comp || !d_out) return fail(RMSF_EINVAL, "rmsf_pca_project: NULL pointer");
  if (n_sel < 1 || n_frames < 0 || fstride < 0) return fail(RMSF_EINVAL, "rmsf_pca_project: bad sizes");
  if (n_comp < 1) return fail(RMSF_EINVAL, "rmsf_pca_project: n_comp < 1");
  if (ldc < n_comp || ldo < n_comp) return fail(RMSF_EINVAL, "rmsf_pca_project: ldc and ldo must be >= n_comp");
  if ((d_xform != nullptr) != (d_refinfo != nullptr))
    return fail(RMSF_EINVAL, "rmsf_pca_project: d_xform and d_refinfo go together");
  if (n_frames == 0) return RMSF_OK;
  const ProjPlan pl = proj_plan(n_frames, n_sel, n_comp);
  const int64_t n_out = n_frames * n_comp;
  if (pl.n_ft > INT32_MAX || pl.n_pan > 65535 || pl.n_ks > 65535 || (n_out + kBlock - 1) / kBlock > INT32_MAX)
    return fail(RMSF_EINVAL, "rmsf_pca_project: batch too large for one launch");
  const size_t need = proj_work_doubles(pl, n_frames, n_comp) * sizeof(double);
  if (need && (!d_work || work_bytes < need)) return fail(RMSF_EINVAL, "rmsf_pca_project: workspace too small");
  const int direct = pl.n_ks == 1;
  double *work = static_cast<double *>(d_work);
  const dim3 grid((unsigned)pl.n_ft, (unsigned)pl.n_pan, (unsigned)pl.n_ks);
#define PROJ_ARGS                                                                                                  \
  pl.n_nt, grid, S(stream), d_xyz, fstride, n_frames, n_sel, d_sel, d_xform, d_refinfo, d_mean, d_comp, ldc, n_comp, \
      d_out, ldo, work, pl.ks_atoms, direct
  const bool al = d_xform != nullptr, g = d_sel != nullptr;
  if (al && g) launch_tiles<true, true>(PROJ_ARGS);
  else if (al) launch_tiles<true, false>(PROJ_ARGS);
  else if (g) launch_tiles<false, true>(PROJ_ARGS);
  else launch_tiles<false, false>(PROJ_ARGS);
#undef PROJ_ARGS
  if (int rc = after_launch("k_proj_tiles")) return rc;
  if (!direct) {
    hipLaunchKernelGGL(k_proj_fold, dim3((unsigned)((n_out + kBlock - 1) / kBlock)), dim3(kBlock), 0, S(stream), work,
                       n_frames, n_comp, pl.n_ks, d_out, ldo);
    if (int rc = after_launch("k_proj_fold")) return rc;
  }
  return RMSF_OK;
}

}  // extern "C"
