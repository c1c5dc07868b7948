// msd.hip -- the mean squared displacement of every atom at every lag (the
// Einstein relation's left side), with the trajectory unwrapped by the "nojump"
// rule first ("Mean squared displacement").  All f64, no FMA.
//
//   u_c(0) = (double)x_c(0)
//   free:   u_c(k) = (double)x_c(k)
//   nojump: u_c(k) = u_c(k-1) + pair_image::image((double)x_c(k) - (double)x_c(k-1), L_c(k), 1/L_c(k))
//   d(a,t,tau) = (dx*dx + dy*dy) + dz*dz, dc = u_c(t+tau) - u_c(t), the
//                coordinates the mask leaves out left out of the expression
//   S(a,tau) = sum over t < F - tau of d(a,t,tau);  msd(a,tau) = S / (double)(F - tau)
//   mean(tau) = (sum over a of msd(a,tau)) / (double)n
//
// k_msd_planes  frame-major f32 rows -> atom-major f64 planes [3 n_sel][ld].  A
//               workgroup owns 64 atom-coordinates (q = 3 a + c) and marches
//               over the frames 64 at a time: every lane forms the increments
//               of its (frame, q) elements -- they do not depend on each other
//               -- into an LDS tile, reading the frame-major rows with q along
//               the lanes; the first wave then adds each column up in frame
//               order, one lane a column carrying u across the chunks (the
//               one serial chain of the definition); then the tile is written
//               out with the frames along the lanes.
// k_msd_lags    a workgroup of 16 x 16 lanes owns one atom, a block of 64 lags
//               and a run of origins, staged through LDS kChunk origins at a
//               time (the origins' window and the ends' window, a coordinate
//               each; the next chunk's loads fly under this chunk's sums).  Lane (tx, ty) holds origins t + ty + 16 r and lags
//               tau0 + tx + 16 s, r, s < 4: 4 origin values and the 7 distinct
//               end values t + tau0 + tx + ty + 16 (r + s) a coordinate serve
//               16 terms.  Four accumulators a lane, one a lag, live across
//               the whole run; the 16 lanes of a lag meet in a fixed tree.
//               Terms past the end of the trajectory or of the run are selected
//               out; a step of 64 origins that lies wholly inside takes the
//               body with no selects.
// k_msd_fold    where the origins were split over workgroups: the partial sums
//               of a (lag, atom) added in split order, then the one division.
// k_msd_mean    a workgroup a lag: lanes stride the atoms in order, then a
//               fixed tree.
//
// No float atomics anywhere: the same bytes on every run.
#include <climits>
#include <cmath>
#include <cstdint>

#include "pair_image.h"
#include "rmsf_host.h"

namespace {

constexpr int kLagBlock = 64;            // lags a workgroup
constexpr int kLanes = 16;               // lanes a side: 16 x 16 = 256
constexpr int kReg = kLagBlock / kLanes; // lags, and origins a step, a lane
constexpr int kBlock = kLanes * kLanes;
constexpr int kStep = kLanes * kReg;     // origins a step of the body
constexpr int kChunk = 256;              // origins staged in LDS at a time
constexpr int kEnds = kChunk + kLagBlock; // the ends' window: kChunk + kLagBlock - 1 used
constexpr int64_t kTargetBlocks = 2048;  // as k_contact_counts: 8 workgroups a CU
constexpr int64_t kMaxLagBlocks = 65535; // gridDim.y
constexpr int64_t kMaxFrames = kMaxLagBlocks * kLagBlock;
constexpr int kTile = 64;                // k_msd_planes: atom-coordinates, and frames a chunk
constexpr int kPlaneAlign = 16;          // doubles: a plane row starts on 128 bytes

static_assert(kChunk % kStep == 0 && kStep == kLagBlock, "a step is 64 origins by 64 lags");
static_assert(kBlock % kTile == 0, "k_msd_planes: whole rows of the tile a pass");

inline int64_t plane_ld(int64_t n_frames) { return (n_frames + kPlaneAlign - 1) / kPlaneAlign * kPlaneAlign; }

struct Plan {
  int64_t lag_blocks, per_split, n_splits;
};
inline Plan plan(int64_t n_sel, int64_t n_frames, int64_t n_lags) {
  Plan p;
  p.lag_blocks = (n_lags + kLagBlock - 1) / kLagBlock;
  const int64_t chunks = (n_frames + kChunk - 1) / kChunk;
  const int64_t base = n_sel * p.lag_blocks;
  int64_t want = (kTargetBlocks + base - 1) / base;
  if (want > chunks) want = chunks;
  if (want < 1) want = 1;
  p.per_split = (chunks + want - 1) / want * kChunk;  // whole chunks a split; the last may be ragged
  p.n_splits = (n_frames + p.per_split - 1) / p.per_split;
  return p;
}

inline int popcount3(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1); }

// ---- device ------------------------------------------------------------------------------
template <bool kBox>
__global__ __launch_bounds__(kBlock) void k_msd_planes(const float *__restrict__ xyz, int64_t fstride, int64_t n_frames,
                                                       const int32_t *__restrict__ idx, int64_t n_q,
                                                       const double *__restrict__ box, double *__restrict__ planes,
                                                       int64_t ld) {
  __shared__ double s_u[kTile][kTile + 1];  // [frame][q]; + 1: the write-out reads a column a lane
  const int tid = threadIdx.x, lane = tid & (kTile - 1), row0 = tid / kTile;
  const int64_t q0 = (int64_t)blockIdx.x * kTile;
  // this lane's column while loading: atom-coordinate q0 + lane
  const int64_t q = q0 + lane;
  const int c = (int)(q % 3);
  const int64_t col = q < n_q ? 3 * (int64_t)(idx ? idx[q / 3] : q / 3) + c : -1;
  double carry = 0.0;  // (the first wave's lanes) u of the frame before this chunk
  for (int64_t f0 = 0; f0 < ld; f0 += kTile) {
    // the increments (the first frame, and free space: the coordinate itself)
#pragma unroll
    for (int k = 0; k < kTile / (kBlock / kTile); ++k) {
      const int ff = row0 + k * (kBlock / kTile);
      const int64_t f = f0 + ff;
      double v = 0.0;
      if (col >= 0 && f < n_frames) {
        const double x = (double)xyz[f * fstride + col];
        v = x;
        if (kBox && f > 0) {
          const double before = (double)xyz[(f - 1) * fstride + col];
          v = pair_image::image(x - before, box[6 * f + c], box[6 * f + 3 + c]);
        }
      }
      s_u[ff][lane] = v;
    }
    __syncthreads();
    if (kBox && tid < kTile) {  // the chain: one lane a column, in frame order
      const int nf = n_frames - f0 < kTile ? (int)(n_frames - f0) : kTile;
      for (int ff = 0; ff < nf; ++ff) {
        const double v = s_u[ff][lane];
        carry = f0 + ff == 0 ? v : carry + v;
        s_u[ff][lane] = carry;
      }
    }
    if (kBox) __syncthreads();
    // out: the frames along the lanes; the columns from n_frames to ld are the zeros staged above
    const int64_t f = f0 + lane;
#pragma unroll 4
    for (int k = 0; k < kTile / (kBlock / kTile); ++k) {
      const int qq = row0 + k * (kBlock / kTile);
      if (q0 + qq < n_q && f < ld) planes[(q0 + qq) * ld + f] = s_u[lane][qq];
    }
    __syncthreads();
  }
}

template <int kMask>
struct Dims {
  static constexpr int n = (kMask & 1) + ((kMask >> 1) & 1) + ((kMask >> 2) & 1);
  // the c-th coordinate present: its plane
  __host__ __device__ static constexpr int plane(int c) {
    int seen = 0;
    for (int p = 0; p < 3; ++p)
      if ((kMask >> p) & 1) {
        if (seen == c) return p;
        ++seen;
      }
    return 0;
  }
};

// One ds_read_b64.  The volatile keeps the compiler from pairing two of them
// into a ds_read2_b64, which moves 128 bytes a clock where two single reads
// move 256: paired, the reads of a step take as long as its arithmetic.
__device__ inline double lds_read(const double *p) {
  typedef __attribute__((address_space(3))) const volatile double lds_double;
  return *(lds_double *)p;
}

// One step: 64 origins (s_o[c][o + ty + 16 r]) by 64 lags; the ends are
// s_e[c][o + tx + ty + 16 (r + s)].  kMasked: a term counts iff its origin
// t + ty + 16 r is below lim[s].
template <int kN, bool kMasked>
__device__ inline void step(const double (*s_o)[kChunk], const double (*s_e)[kEnds], int o, int tx, int ty, int64_t t,
                            const int64_t *lim, double *acc) {
  // a coordinate at a time, so that one coordinate's 11 values are live, not three's:
  // d = dx*dx, then d + dy*dy, then that + dz*dz is the definition's order
  double d[kReg][kReg];
#pragma unroll
  for (int c = 0; c < kN; ++c) {
    double org[kReg], end[2 * kReg - 1];
#pragma unroll
    for (int r = 0; r < kReg; ++r) org[r] = lds_read(&s_o[c][o + ty + kLanes * r]);
#pragma unroll
    for (int m = 0; m < 2 * kReg - 1; ++m) end[m] = lds_read(&s_e[c][o + tx + ty + kLanes * m]);
#pragma unroll
    for (int r = 0; r < kReg; ++r)
#pragma unroll
      for (int s = 0; s < kReg; ++s) {
        const double e = end[r + s] - org[r];
        d[r][s] = c == 0 ? e * e : d[r][s] + e * e;
      }
  }
#pragma unroll
  for (int r = 0; r < kReg; ++r)
#pragma unroll
    for (int s = 0; s < kReg; ++s) {
      if (kMasked) d[r][s] = t + ty + kLanes * r < lim[s] ? d[r][s] : 0.0;
      acc[s] = acc[s] + d[r][s];
    }
}

// out: n_splits == 1: d_msd [n_lags][ld_out], divided; else the partial sums
// work [split][n_lags][n_sel].
template <int kMask>
__global__ __launch_bounds__(kBlock) void k_msd_lags(const double *__restrict__ planes, int64_t ld, int64_t n_sel,
                                                     int64_t n_frames, int64_t n_lags, int64_t per_split,
                                                     double *__restrict__ msd, int64_t ld_out,
                                                     double *__restrict__ work) {
  constexpr int kN = Dims<kMask>::n;
  __shared__ double s_o[kN][kChunk];
  __shared__ double s_e[kN][kEnds];
  __shared__ double s_red[kLanes][kLagBlock];
  const int tid = threadIdx.x, tx = tid & (kLanes - 1), ty = tid / kLanes;
  const int64_t a = blockIdx.x, tau0 = (int64_t)blockIdx.y * kLagBlock;
  const int64_t t_begin = (int64_t)blockIdx.z * per_split;
  int64_t t_end = t_begin + per_split < n_frames ? t_begin + per_split : n_frames;
  if (t_end > n_frames - tau0) t_end = n_frames - tau0;  // no origin past it has an end for any lag of the block
  // lag s of this lane counts the origins below lim[s]
  int64_t lim[kReg];
  int64_t lim_all = t_end;  // origins below it count for every lag of the block
#pragma unroll
  for (int s = 0; s < kReg; ++s) {
    const int64_t tau = tau0 + tx + kLanes * s;
    lim[s] = tau < n_lags ? (t_end < n_frames - tau ? t_end : n_frames - tau) : 0;
  }
  if (tau0 + kLagBlock > n_lags)
    lim_all = 0;
  else if (lim_all > n_frames - (tau0 + kLagBlock - 1))
    lim_all = n_frames - (tau0 + kLagBlock - 1);
  double acc[kReg] = {};
  const double *rows[kN];
#pragma unroll
  for (int c = 0; c < kN; ++c) rows[c] = planes + (3 * a + Dims<kMask>::plane(c)) * ld;
  // A chunk's values are loaded into registers while the chunk before is summed
  // and go to LDS after it: every load is issued before any is waited for, and
  // the wait falls under a chunk's arithmetic.  Frames past the end are read
  // at the last frame and stored as zeros: the zeros rmsf_msd_planes writes from
  // n_frames to ld are never read here, any ld >= n_frames will do.
  static_assert(kChunk == kBlock && kEnds <= 2 * kBlock, "a lane stages one origin and two ends a coordinate");
  const int64_t last = n_frames - 1;
  double v_o[kN], v_e0[kN], v_e1[kN];
  auto fetch = [&](int64_t t0) {
    const int64_t fo = t0 + tid, fe = t0 + tau0 + tid;
#pragma unroll
    for (int c = 0; c < kN; ++c) {
      v_o[c] = rows[c][fo < last ? fo : last];
      v_e0[c] = rows[c][fe < last ? fe : last];
      v_e1[c] = rows[c][fe + kBlock < last ? fe + kBlock : last];
    }
  };
  if (t_begin < t_end) fetch(t_begin);
  for (int64_t t0 = t_begin; t0 < t_end; t0 += kChunk) {
    __syncthreads();  // the chunk before has been read
    const int64_t fo = t0 + tid, fe = t0 + tau0 + tid;
#pragma unroll
    for (int c = 0; c < kN; ++c) {
      s_o[c][tid] = fo <= last ? v_o[c] : 0.0;
      s_e[c][tid] = fe <= last ? v_e0[c] : 0.0;
      if (tid < kEnds - kBlock) s_e[c][kBlock + tid] = fe + kBlock <= last ? v_e1[c] : 0.0;
    }
    __syncthreads();
    if (t0 + kChunk < t_end) fetch(t0 + kChunk);
    const int n_steps = t_end - t0 < kChunk ? (int)((t_end - t0 + kStep - 1) / kStep) : kChunk / kStep;
    for (int k = 0; k < n_steps; ++k) {
      const int64_t t = t0 + (int64_t)k * kStep;
      if (t + kStep <= lim_all)
        step<kN, false>(s_o, s_e, k * kStep, tx, ty, t, lim, acc);
      else
        step<kN, true>(s_o, s_e, k * kStep, tx, ty, t, lim, acc);
    }
  }
  // the 16 lanes (ty) of a lag meet in a fixed tree, one lane a lag
#pragma unroll
  for (int s = 0; s < kReg; ++s) s_red[ty][tx + kLanes * s] = acc[s];
  __syncthreads();
  if (tid < kLagBlock) {
    const int64_t tau = tau0 + tid;
    if (tau < n_lags) {
      double v[kLanes];
#pragma unroll
      for (int i = 0; i < kLanes; ++i) v[i] = s_red[i][tid];
#pragma unroll
      for (int w = kLanes / 2; w >= 1; w /= 2)
#pragma unroll
        for (int i = 0; i < w; ++i) v[i] = v[2 * i] + v[2 * i + 1];
      if (work)
        work[((int64_t)blockIdx.z * n_lags + tau) * n_sel + a] = v[0];
      else
        msd[tau * ld_out + a] = v[0] / (double)(n_frames - tau);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_msd_fold(const double *__restrict__ work, int64_t n_splits, int64_t n_sel,
                                                     int64_t n_frames, int64_t n_lags, double *__restrict__ msd,
                                                     int64_t ld_out) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_lags * n_sel) return;
  const int64_t tau = e / n_sel, a = e % n_sel;
  double s = work[e];
  for (int64_t z = 1; z < n_splits; ++z) s = s + work[z * n_lags * n_sel + e];
  msd[tau * ld_out + a] = s / (double)(n_frames - tau);
}

__global__ __launch_bounds__(kBlock) void k_msd_mean(const double *__restrict__ msd, int64_t ld_out, int64_t n_sel,
                                                     double *__restrict__ mean) {
  __shared__ double s[kBlock];
  const int tid = threadIdx.x;
  const double *row = msd + (int64_t)blockIdx.x * ld_out;
  double v = 0.0;
  for (int64_t a = tid; a < n_sel; a += kBlock) v = v + row[a];
  s[tid] = v;
  __syncthreads();
  for (int w = kBlock / 2; w >= 1; w /= 2) {
    if (tid < w) s[tid] = s[tid] + s[tid + w];
    __syncthreads();
  }
  if (tid == 0) mean[blockIdx.x] = s[0] / (double)n_sel;
}

// ---- checks ------------------------------------------------------------------------------
inline int check_planes(const char *who, const void *xyz, int64_t fstride, int64_t n_frames, int64_t n_atoms,
                        const int32_t *h_idx, int64_t n_sel, const double *h_box, const void *planes, int64_t ld) {
  const std::string w(who);
  if (!xyz || !planes) return fail(RMSF_EINVAL, w + ": a NULL pointer");
  if (n_frames < 1 || n_frames > kMaxFrames || n_atoms < 1 || n_atoms > INT32_MAX / 3 || n_sel < 1 ||
      n_sel > INT32_MAX / 3 || fstride < 3 * n_atoms)
    return fail(RMSF_EINVAL, w + ": a size out of range");
  if (ld < n_frames) return fail(RMSF_EINVAL, w + ": ld is smaller than n_frames");
  if (h_idx)
    for (int64_t i = 0; i < n_sel; ++i)
      if (h_idx[i] < 0 || h_idx[i] >= n_atoms) return fail(RMSF_EINVAL, w + ": a row index is out of range");
  if (h_box)
    for (int64_t f = 0; f < n_frames; ++f)
      for (int k = 0; k < 3; ++k) {
        const double L = h_box[6 * f + k];
        if (!(std::isfinite(L) && L > 0.0)) return fail(RMSF_EINVAL, w + ": a box edge is not positive and finite");
        if (h_box[6 * f + 3 + k] != 1.0 / L) return fail(RMSF_EINVAL, w + ": a box's inverse edge is not 1.0 / edge");
      }
  return RMSF_OK;
}

inline int check_lags(const char *who, const void *planes, int64_t ld, int64_t n_sel, int64_t n_frames, int64_t n_lags,
                      int dims_mask, const void *msd, int64_t ld_out) {
  const std::string w(who);
  if (!planes || !msd) return fail(RMSF_EINVAL, w + ": a NULL pointer");
  if (n_frames < 1 || n_frames > kMaxFrames || n_sel < 1 || n_sel > INT32_MAX / 3)
    return fail(RMSF_EINVAL, w + ": a size out of range");
  if (n_lags < 1 || n_lags > n_frames) return fail(RMSF_EINVAL, w + ": n_lags must be in 1..n_frames");
  if (dims_mask < 1 || dims_mask > 7) return fail(RMSF_EINVAL, w + ": dims_mask must be in 1..7");
  if (ld < n_frames) return fail(RMSF_EINVAL, w + ": ld is smaller than n_frames");
  if (ld_out < n_sel) return fail(RMSF_EINVAL, w + ": ld_out is smaller than n_sel");
  return RMSF_OK;
}

inline bool good_sizes(int64_t n_sel, int64_t n_frames, int64_t n_lags) {
  return n_sel >= 1 && n_sel <= INT32_MAX / 3 && n_frames >= 1 && n_frames <= kMaxFrames && n_lags >= 1 &&
         n_lags <= n_frames;
}

}  // namespace

extern "C" {

RMSF_EXPORT int64_t rmsf_msd_plane_ld(int64_t n_frames) {
  return n_frames >= 1 && n_frames <= kMaxFrames ? plane_ld(n_frames) : 0;
}

RMSF_EXPORT int rmsf_msd_plan(int64_t n_sel, int64_t n_frames, int64_t n_lags, int32_t *lag_block,
                              int32_t *origin_chunk, int32_t *n_splits) {
  if (!good_sizes(n_sel, n_frames, n_lags) || !lag_block || !origin_chunk || !n_splits)
    return fail(RMSF_EINVAL, "rmsf_msd_plan: bad arguments");
  *lag_block = kLagBlock;
  *origin_chunk = kChunk;
  *n_splits = (int32_t)plan(n_sel, n_frames, n_lags).n_splits;
  return RMSF_OK;
}

RMSF_EXPORT size_t rmsf_msd_workspace_bytes(int64_t n_sel, int64_t n_frames, int64_t n_lags) {
  if (!good_sizes(n_sel, n_frames, n_lags)) return 0;
  const Plan p = plan(n_sel, n_frames, n_lags);
  return p.n_splits > 1 ? sizeof(double) * (size_t)p.n_splits * (size_t)n_lags * (size_t)n_sel : 0;
}

RMSF_EXPORT int rmsf_msd_planes(const float *d_xyz, int64_t frame_stride, int64_t n_frames, int64_t n_atoms,
                                const int32_t *d_idx, const int32_t *h_idx, int64_t n_sel, const double *d_box,
                                const double *h_box, double *d_planes, int64_t ld, void *stream) {
  const char *who = "rmsf_msd_planes";
  if (int rc = check_planes(who, d_xyz, frame_stride, n_frames, n_atoms, h_idx, n_sel, h_box, d_planes, ld)) return rc;
  if (!d_idx && n_sel > n_atoms) return fail(RMSF_EINVAL, "rmsf_msd_planes: more dense rows than the frame has atoms");
  if ((d_box == nullptr) != (h_box == nullptr))
    return fail(RMSF_EINVAL, "rmsf_msd_planes: the boxes need their device and their host copy");
  const int64_t n_q = 3 * n_sel;
  const dim3 grid((unsigned)((n_q + kTile - 1) / kTile));
  if (d_box)
    hipLaunchKernelGGL(k_msd_planes<true>, grid, dim3(kBlock), 0, S(stream), d_xyz, frame_stride, n_frames, d_idx, n_q,
                       d_box, d_planes, ld);
  else
    hipLaunchKernelGGL(k_msd_planes<false>, grid, dim3(kBlock), 0, S(stream), d_xyz, frame_stride, n_frames, d_idx,
                       n_q, d_box, d_planes, ld);
  return after_launch("k_msd_planes");
}

RMSF_EXPORT int rmsf_msd_lags(const double *d_planes, int64_t ld, int64_t n_sel, int64_t n_frames, int64_t n_lags,
                              int dims_mask, double *d_msd, int64_t ld_out, double *d_mean, void *d_work,
                              size_t work_bytes, void *stream) {
  const char *who = "rmsf_msd_lags";
  if (int rc = check_lags(who, d_planes, ld, n_sel, n_frames, n_lags, dims_mask, d_msd, ld_out)) return rc;
  const size_t need = rmsf_msd_workspace_bytes(n_sel, n_frames, n_lags);
  if (need && (!d_work || work_bytes < need))
    return fail(RMSF_EINVAL, "rmsf_msd_lags: the workspace is smaller than rmsf_msd_workspace_bytes");
  const Plan p = plan(n_sel, n_frames, n_lags);
  double *work = p.n_splits > 1 ? static_cast<double *>(d_work) : nullptr;
  // x the atoms, y the lag blocks: the small lags, whose origins are the most, are issued first
  const dim3 grid((unsigned)n_sel, (unsigned)p.lag_blocks, (unsigned)p.n_splits);
#define RMSF_MSD(MASK)                                                                                          \
  case MASK:                                                                                                    \
    hipLaunchKernelGGL(k_msd_lags<MASK>, grid, dim3(kBlock), 0, S(stream), d_planes, ld, n_sel, n_frames, n_lags, \
                       p.per_split, d_msd, ld_out, work);                                                       \
    break
  switch (dims_mask) {
    RMSF_MSD(1);
    RMSF_MSD(2);
    RMSF_MSD(3);
    RMSF_MSD(4);
    RMSF_MSD(5);
    RMSF_MSD(6);
    RMSF_MSD(7);
  }
#undef RMSF_MSD
  if (int rc = after_launch("k_msd_lags")) return rc;
  if (work) {
    const int64_t n = n_lags * n_sel;
    hipLaunchKernelGGL(k_msd_fold, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, S(stream), work,
                       p.n_splits, n_sel, n_frames, n_lags, d_msd, ld_out);
    if (int rc = after_launch("k_msd_fold")) return rc;
  }
  if (d_mean) {
    hipLaunchKernelGGL(k_msd_mean, dim3((unsigned)n_lags), dim3(kBlock), 0, S(stream), d_msd, ld_out, n_sel, d_mean);
    if (int rc = after_launch("k_msd_mean")) return rc;
  }
  return RMSF_OK;
}

RMSF_EXPORT int rmsf_msd_planes_host(const float *h_xyz, int64_t frame_stride, int64_t n_frames, int64_t n_atoms,
                                     const int32_t *h_idx, int64_t n_sel, const double *h_box, double *h_planes,
                                     int64_t ld) {
  if (int rc = check_planes("rmsf_msd_planes_host", h_xyz, frame_stride, n_frames, n_atoms, h_idx, n_sel, h_box,
                            h_planes, ld))
    return rc;
  if (!h_idx && n_sel > n_atoms)
    return fail(RMSF_EINVAL, "rmsf_msd_planes_host: more dense rows than the frame has atoms");
  for (int64_t a = 0; a < n_sel; ++a)
    for (int c = 0; c < 3; ++c) {
      const float *x = h_xyz + 3 * (int64_t)(h_idx ? h_idx[a] : a) + c;
      double *u = h_planes + (3 * a + c) * ld;
      u[0] = (double)x[0];
      for (int64_t k = 1; k < n_frames; ++k) {
        const double now = (double)x[k * frame_stride];
        u[k] = h_box ? u[k - 1] + pair_image::image(now - (double)x[(k - 1) * frame_stride], h_box[6 * k + c],
                                                    h_box[6 * k + 3 + c])
                     : now;
      }
      for (int64_t k = n_frames; k < ld; ++k) u[k] = 0.0;
    }
  return RMSF_OK;
}

RMSF_EXPORT int rmsf_msd_lags_host(const double *h_planes, int64_t ld, int64_t n_sel, int64_t n_frames, int64_t n_lags,
                                   int dims_mask, double *h_msd, int64_t ld_out, double *h_mean) {
  if (int rc = check_lags("rmsf_msd_lags_host", h_planes, ld, n_sel, n_frames, n_lags, dims_mask, h_msd, ld_out))
    return rc;
  const int n_dims = popcount3(dims_mask);
  int pl[3] = {0, 0, 0};
  for (int p = 0, c = 0; p < 3; ++p)
    if ((dims_mask >> p) & 1) pl[c++] = p;
  for (int64_t tau = 0; tau < n_lags; ++tau) {
    double total = 0.0;
    for (int64_t a = 0; a < n_sel; ++a) {
      const double *u0 = h_planes + (3 * a + pl[0]) * ld, *u1 = h_planes + (3 * a + pl[1]) * ld,
                   *u2 = h_planes + (3 * a + pl[2]) * ld;
      double s = 0.0;
      for (int64_t t = 0; t + tau < n_frames; ++t) {
        const double d0 = u0[t + tau] - u0[t];
        double d = d0 * d0;
        if (n_dims > 1) {
          const double d1 = u1[t + tau] - u1[t];
          d = d + d1 * d1;
        }
        if (n_dims > 2) {
          const double d2 = u2[t + tau] - u2[t];
          d = d + d2 * d2;
        }
        s = s + d;
      }
      const double m = s / (double)(n_frames - tau);
      h_msd[tau * ld_out + a] = m;
      total = total + m;
    }
    if (h_mean) h_mean[tau] = total / (double)n_sel;
  }
  return RMSF_OK;
}

}  // extern "C"
