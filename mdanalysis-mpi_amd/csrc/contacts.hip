// contacts.hip -- distances between atoms within a frame, after one comparison
// all integers ("Contacts").
//
//   dx = (double)xa - (double)xb, dy, dz likewise (f32 coordinates as stored)
//   d2 = (dx*dx + dy*dy) + dz*dz          no FMA (-ffp-contract=off)
//   d  = sqrt(d2), correctly rounded;  in contact  iff  d <= radius
//
// sqrt is monotone, so d <= radius iff d2 <= t for t = contact_threshold(radius),
// the largest double whose root is <= radius: the counting kernels compare d2
// and take no root.  A NaN compares false: never a contact.
//
// k_contact_counts    counts[i][j] = frames in which atoms a_i and b_j touch.
//                     A workgroup owns a 64 x 64 tile of pairs and a run of
//                     frames; a lane a 4 x 4 block of int counters.  Frames go
//                     through LDS kChunk at a time as f64 planes: plain loads
//                     into registers, one conversion an atom and frame, then
//                     ds_write.  Lane (tx, ty) has atoms ty + 16 r of A and
//                     tx + 16 s of B, so a ds_read_b64's 32-lane group reads
//                     16 consecutive doubles of B (every bank once) and two of
//                     A (broadcast).  Rows past a tile's end are staged as NaN
//                     and the frame loop has no bounds in it.
// k_contact_zero      the [n_a][n_b] corner of the output, before split runs.
// k_contact_fraction  Q(t) over a list of pairs: a frame's rows to LDS once,
//                     the lanes stride the pairs, a fixed tree sums the lanes.
//
// Few tiles (small selections) leave the chip idle: the frames are then split
// over gridDim.z and the splits meet in the output by integer atomicAdd, the
// same sum in any order.  No float atomics anywhere.
#include <climits>
#include <cmath>
#include <cstdint>

#include "rmsf_host.h"

namespace {

constexpr int kWave = 64;
constexpr int kTile = 64;               // atoms a side of a workgroup's tile
constexpr int kLanes = 16;              // lanes a side: 16 x 16 = 256
constexpr int kReg = kTile / kLanes;    // atoms a side of a lane's block
constexpr int kBlock = kLanes * kLanes;
constexpr int kChunk = 8;               // frames in LDS: 2 * 8 * 3 * 64 * 8 = 24 KB
constexpr int kStageRows = kBlock / kTile;  // frames the staging threads cover at once
// What the frame split aims for: 8 workgroups a CU, more than the 5 that fit.
// Measured at 214 atoms x 20,000 frames: 256 / 512 / 1,024 / 2,048 give 0.686 /
// 0.591 / 0.508 / 0.453 ms -- the waves hide each other's staging, and the
// atomic adds of more splits cost less than that.
constexpr int64_t kTargetBlocks = 2048;
constexpr int64_t kMaxSplits = 65535;   // gridDim.z

constexpr int kFracBlock = 256;
constexpr int64_t kFracWavePairs = 1024;          // up to here a wave a frame, 4 frames a workgroup
constexpr size_t kFracWaveLds = 48 * 1024;        // ... if their rows fit in this much LDS
constexpr size_t kFracBlockLds = 60 * 1024;       // one frame's rows; past it they are read from L2

// The largest t with sqrt(t) <= r, for finite r > 0: r * r rounds to within an
// ulp of it, and the two loops walk the rest.
inline double contact_threshold(double r) {
  double t = r * r;
  while (std::sqrt(t) > r) t = std::nextafter(t, 0.0);
  for (double u = std::nextafter(t, INFINITY); std::sqrt(u) <= r; u = std::nextafter(t, INFINITY)) t = u;
  return t;
}

__host__ __device__ inline double dist2(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

struct Plan {
  int64_t tiles_a, tiles_b, tiles, per_split, n_splits;
};
inline Plan plan(int64_t n_a, int64_t n_b, int64_t n_frames, int symmetric) {
  Plan p;
  p.tiles_a = (n_a + kTile - 1) / kTile;
  p.tiles_b = (n_b + kTile - 1) / kTile;
  p.tiles = symmetric ? p.tiles_a * (p.tiles_a + 1) / 2 : p.tiles_a * p.tiles_b;
  const int64_t chunks = (n_frames + kChunk - 1) / kChunk;
  int64_t want = (kTargetBlocks + p.tiles - 1) / p.tiles;
  if (want > chunks) want = chunks;
  if (want > kMaxSplits) want = kMaxSplits;
  p.per_split = (chunks + want - 1) / want * kChunk;  // whole chunks a split; the last may be ragged
  p.n_splits = (n_frames + p.per_split - 1) / p.per_split;
  return p;
}

// One side's kChunk frames of kTile atoms into s[frame][xyz][atom].  Thread
// (atom = tid % 64, tid / 64) takes frames tid / 64 and tid / 64 + 4; `row` is
// 3 * the atom's row in a frame, or -1 past the side's end.
__device__ inline void stage_side(const float *__restrict__ xyz, int64_t fstride, int64_t f0, int nf, int64_t row,
                                  double (*s)[3][kTile], int tid) {
  const int atom = tid & (kTile - 1);
#pragma unroll
  for (int k = 0; k < kChunk / kStageRows; ++k) {
    const int ff = (tid / kTile) + k * kStageRows;
    if (ff >= nf) continue;
    float x = NAN, y = NAN, z = NAN;
    if (row >= 0) {
      const float *p = xyz + (f0 + ff) * fstride + row;
      x = p[0], y = p[1], z = p[2];
    }
    s[ff][0][atom] = (double)x;
    s[ff][1][atom] = (double)y;
    s[ff][2][atom] = (double)z;
  }
}

template <bool kAtomic>
__global__ __launch_bounds__(kBlock) void k_contact_counts(const float *__restrict__ xyz, int64_t fstride,
                                                           int64_t n_frames, const int32_t *__restrict__ idx_a,
                                                           int64_t n_a, const int32_t *__restrict__ idx_b, int64_t n_b,
                                                           int symmetric, double t, int64_t per_split,
                                                           int32_t *__restrict__ counts, int64_t ld) {
  __shared__ double s_ab[2][kChunk][3][kTile];  // (one array: the epilogue's transpose reuses it)
  double(*s_a)[3][kTile] = s_ab[0], (*s_b)[3][kTile] = s_ab[1];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (symmetric && bj < bi) return;  // (the whole workgroup: the tile below the diagonal is a mirror)
  const int tid = threadIdx.x, tx = tid & (kLanes - 1), ty = tid / kLanes;
  const int64_t a0 = (int64_t)bi * kTile, b0 = (int64_t)bj * kTile;
  const int64_t f_begin = (int64_t)blockIdx.z * per_split;
  const int64_t f_end = f_begin + per_split < n_frames ? f_begin + per_split : n_frames;
  const int64_t ia = a0 + (tid & (kTile - 1)), ib = b0 + (tid & (kTile - 1));
  const int64_t row_a = ia < n_a ? 3 * (int64_t)(idx_a ? idx_a[ia] : ia) : -1;
  const int64_t row_b = ib < n_b ? 3 * (int64_t)(idx_b ? idx_b[ib] : ib) : -1;
  int32_t cnt[kReg][kReg] = {};
  for (int64_t f0 = f_begin; f0 < f_end; f0 += kChunk) {
    const int nf = f_end - f0 < kChunk ? (int)(f_end - f0) : kChunk;
    __syncthreads();  // the chunk before has been read
    stage_side(xyz, fstride, f0, nf, row_a, s_a, tid);
    stage_side(xyz, fstride, f0, nf, row_b, s_b, tid);
    __syncthreads();
    for (int ff = 0; ff < nf; ++ff) {  // (unrolled by 2 or 4 it runs no faster: measured)
      double a[kReg][3], b[kReg][3];
#pragma unroll
      for (int r = 0; r < kReg; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          a[r][c] = s_a[ff][c][ty + kLanes * r];
          b[r][c] = s_b[ff][c][tx + kLanes * r];
        }
#pragma unroll
      for (int r = 0; r < kReg; ++r)
#pragma unroll
        for (int s = 0; s < kReg; ++s)
          cnt[r][s] += dist2(a[r][0], a[r][1], a[r][2], b[s][0], b[s][1], b[s][2]) <= t ? 1 : 0;
    }
  }
#pragma unroll
  for (int r = 0; r < kReg; ++r)
#pragma unroll
    for (int s = 0; s < kReg; ++s) {
      const int64_t i = a0 + ty + kLanes * r, j = b0 + tx + kLanes * s;
      if (i >= n_a || j >= n_b) continue;
      if (kAtomic)
        atomicAdd(&counts[i * ld + j], cnt[r][s]);
      else
        counts[i * ld + j] = cnt[r][s];
    }
  if (!symmetric || bi == bj) return;  // (the whole workgroup)
  // The mirror tile, transposed through LDS so that its 16 tx lanes write 16
  // consecutive ints of a row too; rows of kTile + 1 keep the column reads off
  // one bank.
  static_assert(sizeof(s_ab) >= sizeof(int32_t) * kTile * (kTile + 1), "the transpose fits in the staging LDS");
  int32_t(*s_t)[kTile + 1] = reinterpret_cast<int32_t(*)[kTile + 1]>(&s_ab[0][0][0][0]);
  __syncthreads();  // the last chunk has been read
#pragma unroll
  for (int r = 0; r < kReg; ++r)
#pragma unroll
    for (int s = 0; s < kReg; ++s) s_t[ty + kLanes * r][tx + kLanes * s] = cnt[r][s];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kReg; ++r)
#pragma unroll
    for (int s = 0; s < kReg; ++s) {
      const int la = tx + kLanes * s, lb = ty + kLanes * r;  // the entry (a, b) goes to row b, column a
      const int64_t i = a0 + la, j = b0 + lb;
      if (i >= n_a || j >= n_b) continue;
      if (kAtomic)
        atomicAdd(&counts[j * ld + i], s_t[la][lb]);
      else
        counts[j * ld + i] = s_t[la][lb];
    }
}

__global__ __launch_bounds__(kBlock) void k_contact_zero(int32_t *__restrict__ counts, int64_t n_a, int64_t n_b,
                                                         int64_t ld) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e < n_a * n_b) counts[(e / n_b) * ld + e % n_b] = 0;
}

// A frame's term of Q for the lane's pairs.  kLanesPerFrame = 64: a wave a
// frame, four frames a workgroup; 256: the workgroup a frame.  kStage: the
// frame's rows are in LDS, 3 floats a row; otherwise each pair gathers its two
// rows from the frame where it lies.
template <int kLanesPerFrame, bool kStage>
__global__ __launch_bounds__(kFracBlock) void k_contact_fraction(
    const float *__restrict__ xyz, int64_t fstride, int64_t n_frames, int64_t n_rows,
    const int32_t *__restrict__ rows, const int32_t *__restrict__ pair_a, const int32_t *__restrict__ pair_b,
    const double *__restrict__ r0, int64_t n_pairs, double radius_sq, int soft, double beta, double lambda,
    double *__restrict__ q, int32_t *__restrict__ n_contacts) {
  extern __shared__ float s_xyz[];
  __shared__ double s_sum[kFracBlock / kWave];
  __shared__ int32_t s_cnt[kFracBlock / kWave];
  constexpr int kGroups = kFracBlock / kLanesPerFrame;
  const int tid = threadIdx.x, g = tid / kLanesPerFrame, l = tid % kLanesPerFrame;
  const int64_t frame = (int64_t)blockIdx.x * kGroups + g;
  const bool live = frame < n_frames;  // (kLanesPerFrame lanes together)
  const float *src = xyz + (live ? frame : 0) * fstride;
  const float *at = kStage ? s_xyz + (size_t)g * 3 * n_rows : src;
  if (kStage) {
    float *dst = s_xyz + (size_t)g * 3 * n_rows;
    if (live)
      for (int64_t e = l; e < n_rows; e += kLanesPerFrame) {
        const float *p = src + 3 * (int64_t)(rows ? rows[e] : e);
        dst[3 * e] = p[0], dst[3 * e + 1] = p[1], dst[3 * e + 2] = p[2];
      }
    __syncthreads();
  }
  double sum = 0.0;
  int32_t cnt = 0;
  if (live)
    for (int64_t p = l; p < n_pairs; p += kLanesPerFrame) {
      int64_t ra = pair_a[p], rb = pair_b[p];
      if (!kStage && rows) ra = rows[ra], rb = rows[rb];
      const float *pa = at + 3 * ra, *pb = at + 3 * rb;
      const double d2 = dist2(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2]);
      cnt += d2 <= radius_sq ? 1 : 0;
      if (soft) sum += 1.0 / (1.0 + exp(beta * (sqrt(d2) - lambda * r0[p])));
    }
  // the lanes' sums by the same butterfly every run, then the waves' in order
  for (int d = kWave / 2; d > 0; d >>= 1) {
    sum += __shfl_xor(sum, d);
    cnt += __shfl_xor(cnt, d);
  }
  if (kLanesPerFrame > kWave) {
    if ((tid & (kWave - 1)) == 0) s_sum[tid / kWave] = sum, s_cnt[tid / kWave] = cnt;
    __syncthreads();
    sum = s_sum[0], cnt = s_cnt[0];
    for (int w = 1; w < kFracBlock / kWave; ++w) sum += s_sum[w], cnt += s_cnt[w];
  }
  if (live && l == 0) {
    n_contacts[frame] = cnt;
    q[frame] = (soft ? sum : (double)cnt) / (double)n_pairs;
  }
}

// index arrays the caller holds on the host: every entry in 0..bound-1
inline bool in_range(const int32_t *h, int64_t n, int64_t bound) {
  if (h)
    for (int64_t i = 0; i < n; ++i)
      if (h[i] < 0 || h[i] >= bound) return false;
  return true;
}

inline bool good_radius(double r) { return std::isfinite(r) && r > 0.0; }

inline int check_counts(const char *who, const void *xyz, int64_t fstride, int64_t n_frames, int64_t n_atoms,
                        const int32_t *h_idx_a, int64_t n_a, const int32_t *h_idx_b, int64_t n_b, double radius,
                        const void *counts, int64_t ld) {
  const std::string w(who);
  if (!xyz || !counts || n_frames < 1 || n_frames > INT32_MAX || n_atoms < 1 || n_atoms > INT32_MAX / 3 || n_a < 1 ||
      n_b < 1 || n_a > INT32_MAX || n_b > INT32_MAX || ld < n_b || fstride < 3 * n_atoms)
    return fail(RMSF_EINVAL, w + ": bad arguments");
  if (!good_radius(radius)) return fail(RMSF_EINVAL, w + ": the radius must be positive and finite");
  if (!in_range(h_idx_a, n_a, n_atoms) || !in_range(h_idx_b, n_b, n_atoms))
    return fail(RMSF_EINVAL, w + ": a row index is out of range");
  return RMSF_OK;
}

inline int check_fraction(const char *who, const void *xyz, int64_t fstride, int64_t n_frames, int64_t n_atoms,
                          int64_t n_rows, const int32_t *h_rows, const int32_t *h_pair_a, const int32_t *h_pair_b,
                          const void *r0, int64_t n_pairs, double radius, int method, double beta, double lambda,
                          const void *q, const void *n_contacts) {
  const std::string w(who);
  if (n_pairs < 1) return fail(RMSF_EINVAL, w + ": at least one pair is needed");
  if (!xyz || !q || !n_contacts || n_frames < 1 || n_atoms < 1 || n_atoms > INT32_MAX / 3 || n_rows < 1 ||
      n_rows > INT32_MAX || n_pairs > INT32_MAX || fstride < 3 * n_atoms)
    return fail(RMSF_EINVAL, w + ": bad arguments");
  if (method != RMSF_CONTACT_HARD_CUT && method != RMSF_CONTACT_RADIUS_CUT && method != RMSF_CONTACT_SOFT_CUT)
    return fail(RMSF_EINVAL, w + ": unknown method");
  if (!good_radius(radius)) return fail(RMSF_EINVAL, w + ": the radius must be positive and finite");
  if (method == RMSF_CONTACT_SOFT_CUT && (!r0 || !std::isfinite(beta) || !std::isfinite(lambda)))
    return fail(RMSF_EINVAL, w + ": soft_cut needs r0 and finite beta and lambda_constant");
  if (!in_range(h_rows, n_rows, n_atoms) || !in_range(h_pair_a, n_pairs, n_rows) ||
      !in_range(h_pair_b, n_pairs, n_rows))
    return fail(RMSF_EINVAL, w + ": a row index is out of range");
  return RMSF_OK;
}

}  // namespace

extern "C" {

RMSF_EXPORT double rmsf_contact_threshold_sq(double radius) { return good_radius(radius) ? contact_threshold(radius) : NAN; }

RMSF_EXPORT int rmsf_contact_counts_plan(int64_t n_a, int64_t n_b, int64_t n_frames, int symmetric, int32_t *tile_a,
                                         int32_t *tile_b, int32_t *frame_chunk, int32_t *n_splits) {
  if (n_a < 1 || n_b < 1 || n_frames < 1 || n_a > INT32_MAX || n_b > INT32_MAX || n_frames > INT32_MAX ||
      (symmetric && n_a != n_b) || !tile_a || !tile_b || !frame_chunk || !n_splits)
    return fail(RMSF_EINVAL, "rmsf_contact_counts_plan: bad arguments");
  *tile_a = *tile_b = kTile;
  *frame_chunk = kChunk;
  *n_splits = (int32_t)plan(n_a, n_b, n_frames, symmetric).n_splits;
  return RMSF_OK;
}

RMSF_EXPORT size_t rmsf_contact_counts_workspace_bytes(int64_t n_a, int64_t n_b, int64_t n_frames, int symmetric) {
  (void)n_a, (void)n_b, (void)n_frames, (void)symmetric;
  return 0;  // the splits meet in the output itself
}

RMSF_EXPORT int rmsf_contact_counts(const float *d_xyz, int64_t frame_stride, int64_t n_frames, int64_t n_atoms,
                                    const int32_t *d_idx_a, const int32_t *h_idx_a, int64_t n_a,
                                    const int32_t *d_idx_b, const int32_t *h_idx_b, int64_t n_b, int symmetric,
                                    double radius, int32_t *d_counts, int64_t ld, void *d_work, size_t work_bytes,
                                    void *stream) {
  (void)d_work, (void)work_bytes;
  if (int rc = check_counts("rmsf_contact_counts", d_xyz, frame_stride, n_frames, n_atoms, h_idx_a, n_a, h_idx_b, n_b,
                            radius, d_counts, ld))
    return rc;
  if ((!d_idx_a && n_a > n_atoms) || (!d_idx_b && n_b > n_atoms))
    return fail(RMSF_EINVAL, "rmsf_contact_counts: more dense rows than the frame has atoms");
  if (symmetric && (n_a != n_b || d_idx_a != d_idx_b))
    return fail(RMSF_EINVAL, "rmsf_contact_counts: symmetric needs the same rows on both sides");
  const Plan p = plan(n_a, n_b, n_frames, symmetric);
  // gridDim.y, and the zeroing launch's gridDim.x (n_b <= INT32_MAX bounds the tiles of columns)
  if (p.tiles_a > 65535 || (n_a * n_b + kBlock - 1) / kBlock > INT32_MAX)
    return fail(RMSF_EINVAL, "rmsf_contact_counts: more than 65535 tiles of rows, or more entries than one launch zeroes");
  const double t = contact_threshold(radius);
  const dim3 grid((unsigned)p.tiles_b, (unsigned)p.tiles_a, (unsigned)p.n_splits);
  if (p.n_splits > 1) {
    hipLaunchKernelGGL(k_contact_zero, dim3((unsigned)((n_a * n_b + kBlock - 1) / kBlock)), dim3(kBlock), 0, S(stream),
                       d_counts, n_a, n_b, ld);
    hipLaunchKernelGGL(k_contact_counts<true>, grid, dim3(kBlock), 0, S(stream), d_xyz, frame_stride, n_frames,
                       d_idx_a, n_a, d_idx_b, n_b, symmetric, t, p.per_split, d_counts, ld);
  } else {
    hipLaunchKernelGGL(k_contact_counts<false>, grid, dim3(kBlock), 0, S(stream), d_xyz, frame_stride, n_frames,
                       d_idx_a, n_a, d_idx_b, n_b, symmetric, t, p.per_split, d_counts, ld);
  }
  return after_launch("k_contact_counts");
}

RMSF_EXPORT int rmsf_contact_counts_host(const float *h_xyz, int64_t frame_stride, int64_t n_frames, int64_t n_atoms,
                                         const int32_t *h_idx_a, int64_t n_a, const int32_t *h_idx_b, int64_t n_b,
                                         double radius, int32_t *h_counts, int64_t ld) {
  if (int rc = check_counts("rmsf_contact_counts_host", h_xyz, frame_stride, n_frames, n_atoms, h_idx_a, n_a, h_idx_b,
                            n_b, radius, h_counts, ld))
    return rc;
  if ((!h_idx_a && n_a > n_atoms) || (!h_idx_b && n_b > n_atoms))
    return fail(RMSF_EINVAL, "rmsf_contact_counts_host: more dense rows than the frame has atoms");
  for (int64_t i = 0; i < n_a; ++i)
    for (int64_t j = 0; j < n_b; ++j) {
      const int64_t ra = 3 * (int64_t)(h_idx_a ? h_idx_a[i] : i), rb = 3 * (int64_t)(h_idx_b ? h_idx_b[j] : j);
      int32_t c = 0;
      for (int64_t f = 0; f < n_frames; ++f) {
        const float *pa = h_xyz + f * frame_stride + ra, *pb = h_xyz + f * frame_stride + rb;
        c += std::sqrt(dist2(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2])) <= radius ? 1 : 0;
      }
      h_counts[i * ld + j] = c;
    }
  return RMSF_OK;
}

RMSF_EXPORT int rmsf_contact_fraction(const float *d_xyz, int64_t frame_stride, int64_t n_frames, int64_t n_atoms,
                                      int64_t n_rows, const int32_t *d_rows, const int32_t *h_rows,
                                      const int32_t *d_pair_a, const int32_t *d_pair_b, const int32_t *h_pair_a,
                                      const int32_t *h_pair_b, const double *d_r0, int64_t n_pairs, double radius,
                                      int method, double beta, double lambda_constant, double *d_q,
                                      int32_t *d_n_contacts, void *stream) {
  if (int rc = check_fraction("rmsf_contact_fraction", d_xyz, frame_stride, n_frames, n_atoms, n_rows, h_rows,
                              h_pair_a, h_pair_b, d_r0, n_pairs, radius, method, beta, lambda_constant, d_q,
                              d_n_contacts))
    return rc;
  if (!d_pair_a || !d_pair_b || (!d_rows && n_rows > n_atoms))
    return fail(RMSF_EINVAL, "rmsf_contact_fraction: bad arguments");
  const double t = contact_threshold(radius);
  const int soft = method == RMSF_CONTACT_SOFT_CUT;
  const size_t row_bytes = 12 * (size_t)n_rows;
  constexpr int kWaveFrames = kFracBlock / kWave;
#define RMSF_FRACTION(LANES, STAGE, GRID, LDS)                                                                       \
  hipLaunchKernelGGL((k_contact_fraction<LANES, STAGE>), dim3((unsigned)(GRID)), dim3(kFracBlock), LDS, S(stream),   \
                     d_xyz, frame_stride, n_frames, n_rows, d_rows, d_pair_a, d_pair_b, d_r0, n_pairs, t, soft, beta, \
                     lambda_constant, d_q, d_n_contacts)
  if (n_frames > (int64_t)INT32_MAX) return fail(RMSF_EINVAL, "rmsf_contact_fraction: too many frames");
  if (n_pairs <= kFracWavePairs && kWaveFrames * row_bytes <= kFracWaveLds)
    RMSF_FRACTION(kWave, true, (n_frames + kWaveFrames - 1) / kWaveFrames, kWaveFrames * row_bytes);
  else if (row_bytes <= kFracBlockLds)
    RMSF_FRACTION(kFracBlock, true, n_frames, row_bytes);
  else
    RMSF_FRACTION(kFracBlock, false, n_frames, 0);
#undef RMSF_FRACTION
  return after_launch("k_contact_fraction");
}

RMSF_EXPORT int rmsf_contact_fraction_host(const float *h_xyz, int64_t frame_stride, int64_t n_frames, int64_t n_atoms,
                                           int64_t n_rows, const int32_t *h_rows, const int32_t *h_pair_a,
                                           const int32_t *h_pair_b, const double *h_r0, int64_t n_pairs, double radius,
                                           int method, double beta, double lambda_constant, double *h_q,
                                           int32_t *h_n_contacts) {
  if (int rc = check_fraction("rmsf_contact_fraction_host", h_xyz, frame_stride, n_frames, n_atoms, n_rows, h_rows,
                              h_pair_a, h_pair_b, h_r0, n_pairs, radius, method, beta, lambda_constant, h_q,
                              h_n_contacts))
    return rc;
  if (!h_pair_a || !h_pair_b || (!h_rows && n_rows > n_atoms))
    return fail(RMSF_EINVAL, "rmsf_contact_fraction_host: bad arguments");
  const bool soft = method == RMSF_CONTACT_SOFT_CUT;
  for (int64_t f = 0; f < n_frames; ++f) {
    const float *x = h_xyz + f * frame_stride;
    double sum = 0.0;
    int32_t cnt = 0;
    for (int64_t p = 0; p < n_pairs; ++p) {
      const int64_t ra = h_rows ? h_rows[h_pair_a[p]] : h_pair_a[p], rb = h_rows ? h_rows[h_pair_b[p]] : h_pair_b[p];
      const float *pa = x + 3 * ra, *pb = x + 3 * rb;
      const double d = std::sqrt(dist2(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2]));
      cnt += d <= radius ? 1 : 0;
      if (soft) sum += 1.0 / (1.0 + std::exp(beta * (d - lambda_constant * h_r0[p])));
    }
    h_n_contacts[f] = cnt;
    h_q[f] = (soft ? sum : (double)cnt) / (double)n_pairs;
  }
  return RMSF_OK;
}

}  // extern "C"
