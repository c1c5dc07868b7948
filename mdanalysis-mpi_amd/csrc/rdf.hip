// rdf.hip -- the histogram of the distances between two sets of atoms, frame by
// frame, free or under the minimum image of a per-frame orthorhombic box: the
// counts of a radial distribution function ("Radial distribution
// function").  All integers after one comparison.
//
//   d2 by csrc/pair_image.h (f64 differences of the f32 coordinates, the image
//   term with rint, no FMA);  d = sqrt(d2) correctly rounded
//   edges e_k = k * ((rmax - rmin) / nbins) + rmin for k < nbins, e_nbins = rmax
//   bin k iff e_k <= d < e_(k+1); the last bin also takes d == rmax; NaN: no bin
//
// sqrt is monotone, so the host turns every edge into a threshold on d2
// (thresholds(): T_k the smallest double whose root is >= e_k, T_nbins the
// first double above the largest whose root is <= rmax) and bin k is
// T_k <= d2 < T_(k+1): the device takes no f64 root.  It guesses k from an f32
// root and walks the table until the two comparisons hold.
//
// k_rdf_counts  k_contact_counts' tile: a workgroup owns 64 x 64 pairs and a run
//               of frames, a lane a 4 x 4 block of pairs (atoms ty + 16 r of A,
//               tx + 16 s of B), the frames go through LDS kChunk at a time as
//               f64 planes, rows past a side's end are staged as NaN.  The
//               thresholds and the histogram are in LDS too: one set of int32
//               counters a workgroup (more copies measured no faster, and at
//               2,048 bins slower: they cost a workgroup a CU), flushed once to
//               the int64 bins by 64-bit integer atomicAdd.  A lane reads the
//               thresholds of a row of four pairs together and adds for itself;
//               voting a wave's equal bins into one add measured slower at 75
//               bins.  With one bin there is no table to walk and nothing to
//               share: a lane counts in a register (kOne).
//
// The splits of the frames (gridDim.z) and the tiles meet in the int64 bins by
// integer adds after one zeroing: the same bytes in any order.  No float atomics.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "pair_image.h"
#include "rmsf_host.h"

namespace {

constexpr int kTile = 64;               // atoms a side of a workgroup's tile
constexpr int kLanes = 16;              // lanes a side: 16 x 16 = 256
constexpr int kReg = kTile / kLanes;    // atoms a side of a lane's block
constexpr int kBlock = kLanes * kLanes;
constexpr int kChunk = 8;               // frames in LDS: 2 * 8 * 3 * 64 * 8 = 24 KB
constexpr int kStageRows = kBlock / kTile;
constexpr int kMaxBins = 2048;
constexpr int64_t kTargetBlocks = 2048; // as k_contact_counts: 8 workgroups a CU
constexpr int64_t kMaxSplits = 65535;   // gridDim.z
// A workgroup adds at most 2 * 64 * 64 a frame to one int32 counter (every
// pair of an off-diagonal symmetric tile in one bin): 2^13 * 2^17 = 2^30
// before the flush.
constexpr int64_t kMaxSplitFrames = 1 << 17;
static_assert(2 * kTile * kTile * kMaxSplitFrames < (int64_t)INT32_MAX, "an LDS counter cannot wrap before the flush");

// ---- edges and thresholds (host) -------------------------------------------------------
inline bool good_range(double rmin, double rmax, int64_t nbins) {
  return nbins >= 1 && nbins <= kMaxBins && std::isfinite(rmin) && std::isfinite(rmax) && rmin >= 0.0 && rmax > rmin;
}

// numpy.linspace(rmin, rmax, nbins + 1)'s bits
inline void edges(double rmin, double rmax, int nbins, double *e) {
  const double step = (rmax - rmin) / (double)nbins;
  for (int k = 0; k < nbins; ++k) e[k] = (double)k * step + rmin;
  e[nbins] = rmax;
}

// the smallest t with sqrt(t) >= e, for finite e >= 0
inline double threshold_ge(double e) {
  if (e == 0.0) return 0.0;
  double t = e * e;
  while (std::sqrt(t) < e) t = std::nextafter(t, INFINITY);
  for (double u = std::nextafter(t, 0.0); std::sqrt(u) >= e; u = std::nextafter(t, 0.0)) t = u;
  return t;
}

// the first double above the largest t with sqrt(t) <= r, for finite r > 0
inline double threshold_gt(double r) {
  double t = r * r;
  while (std::sqrt(t) <= r) t = std::nextafter(t, INFINITY);
  for (double u = std::nextafter(t, 0.0); std::sqrt(u) > r; u = std::nextafter(t, 0.0)) t = u;
  return t;
}

inline void thresholds(const double *e, int nbins, double *t) {
  for (int k = 0; k < nbins; ++k) t[k] = threshold_ge(e[k]);
  t[nbins] = threshold_gt(e[nbins]);
}

// the bin of a distance by the edges, -1 for none (the definition, with a root a pair)
inline int bin_of(double d, const double *e, int nbins) {
  if (!(d >= e[0]) || d > e[nbins]) return -1;
  if (d == e[nbins]) return nbins - 1;
  int lo = 0, hi = nbins;  // e[lo] <= d < e[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (d >= e[mid]) lo = mid; else hi = mid;
  }
  return lo;
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
  const int64_t least = (n_frames + kMaxSplitFrames - 1) / kMaxSplitFrames;  // no int32 counter wraps
  if (want < least) want = least;
  if (want > chunks) want = chunks;
  if (want > kMaxSplits) want = kMaxSplits;
  p.per_split = (chunks + want - 1) / want * kChunk;  // whole chunks a split; the last may be ragged
  p.n_splits = (n_frames + p.per_split - 1) / p.per_split;
  return p;
}

// ---- device ------------------------------------------------------------------------------
// as contacts.hip's: one side's kChunk frames of kTile atoms into s[frame][xyz][atom]
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

// The bin of a pair in range whose guess missed: T_0 <= d2 ends the first walk
// by k = 0, d2 < T_nbins the second by k = nbins - 1 (the bounds in the loops
// only say so again).
__device__ inline int walk(int k, double d2, const double *__restrict__ s_t, int nbins) {
  while (k > 0 && d2 < s_t[k]) --k;
  while (k < nbins - 1 && d2 >= s_t[k + 1]) ++k;
  return k;
}

// kOne: nbins == 1, where a pair in range needs no table and no LDS counter: a
// lane counts its own pairs in a register and adds once at the end.
template <bool kBox, bool kOne>
__global__ __launch_bounds__(kBlock) void k_rdf_counts(const float *__restrict__ xyz, int64_t fstride, int64_t n_frames,
                                                       const int32_t *__restrict__ idx_a, int64_t n_a,
                                                       const int32_t *__restrict__ idx_b, int64_t n_b, int symmetric,
                                                       int32_t excl_a, int32_t excl_b, const double *__restrict__ box,
                                                       const double *__restrict__ thr, int nbins, float rmin_f,
                                                       float inv_width_f, int64_t per_split,
                                                       unsigned long long *__restrict__ counts) {
  __shared__ double s_ab[2][kChunk][3][kTile];
  extern __shared__ double s_dyn[];  // thresholds [nbins + 1], then int32 counters [nbins]
  double(*s_a)[3][kTile] = s_ab[0], (*s_b)[3][kTile] = s_ab[1];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (symmetric && bj < bi) return;  // (the whole workgroup: the tile below the diagonal is a mirror)
  double *s_t = s_dyn;
  int32_t *hist = reinterpret_cast<int32_t *>(s_dyn + nbins + 1);
  const int tid = threadIdx.x, tx = tid & (kLanes - 1), ty = tid / kLanes;
  for (int e = tid; e <= nbins; e += kBlock) s_t[e] = thr[e];
  for (int e = tid; e < nbins; e += kBlock) hist[e] = 0;
  const double t_lo = thr[0], t_hi = thr[nbins];
  const int64_t a0 = (int64_t)bi * kTile, b0 = (int64_t)bj * kTile;
  const int64_t f_begin = (int64_t)blockIdx.z * per_split;
  const int64_t f_end = f_begin + per_split < n_frames ? f_begin + per_split : n_frames;
  const int64_t ia = a0 + (tid & (kTile - 1)), ib = b0 + (tid & (kTile - 1));
  const int64_t row_a = ia < n_a ? 3 * (int64_t)(idx_a ? idx_a[ia] : ia) : -1;
  const int64_t row_b = ib < n_b ? 3 * (int64_t)(idx_b ? idx_b[ib] : ib) : -1;
  // The pairs of this lane that are never counted, a bit each: the same atom
  // on both sides of the symmetric route, and an exclusion block's pairs.
  unsigned masked = 0;
#pragma unroll
  for (int r = 0; r < kReg; ++r)
#pragma unroll
    for (int s = 0; s < kReg; ++s) {
      const int64_t i = a0 + ty + kLanes * r, j = b0 + tx + kLanes * s;
      const bool out = (symmetric && i == j) || (excl_a && i / excl_a == j / excl_b);
      masked |= (out ? 1u : 0u) << (kReg * r + s);
    }
  // an unordered pair of the symmetric route is met once above the diagonal
  // tiles and twice (both orders) inside one
  const int weight = symmetric && bi != bj ? 2 : 1;
  int32_t mine = 0;  // (kOne) at most 16 pairs a frame over kMaxSplitFrames frames
  for (int64_t f0 = f_begin; f0 < f_end; f0 += kChunk) {
    const int nf = f_end - f0 < kChunk ? (int)(f_end - f0) : kChunk;
    __syncthreads();  // the chunk before has been read (the first time: the table and the zeros are written)
    stage_side(xyz, fstride, f0, nf, row_a, s_a, tid);
    stage_side(xyz, fstride, f0, nf, row_b, s_b, tid);
    __syncthreads();
    for (int ff = 0; ff < nf; ++ff) {
      double bx[6] = {};
      if (kBox) {
        const double *p = box + (f0 + ff) * 6;  // the same address in every lane: scalar loads, once a frame
#pragma unroll
        for (int c = 0; c < 6; ++c) bx[c] = p[c];
      }
      double a[kReg][3], b[kReg][3];
#pragma unroll
      for (int r = 0; r < kReg; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          a[r][c] = s_a[ff][c][ty + kLanes * r];
          b[r][c] = s_b[ff][c][tx + kLanes * r];
        }
#pragma unroll
      for (int r = 0; r < kReg; ++r) {
        double d2[kReg];
        bool in[kReg];
#pragma unroll
        for (int s = 0; s < kReg; ++s) {
          d2[s] = kBox ? pair_image::dist2_box(a[r][0], a[r][1], a[r][2], b[s][0], b[s][1], b[s][2], bx)
                       : pair_image::dist2_free(a[r][0], a[r][1], a[r][2], b[s][0], b[s][1], b[s][2]);
          in[s] = d2[s] >= t_lo && d2[s] < t_hi && !((masked >> (kReg * r + s)) & 1u);
        }
        if (kOne) {
#pragma unroll
          for (int s = 0; s < kReg; ++s) mine += in[s] ? 1 : 0;
          continue;
        }
        // The four guesses and their two thresholds each are read together,
        // by every lane (a pair out of range reads T_0 and T_1, a broadcast):
        // one wait for the LDS a row of pairs, not two a pair.
        int k[kReg];
        double lo[kReg], hi[kReg];
#pragma unroll
        for (int s = 0; s < kReg; ++s) {
          const int g = (int)((__builtin_amdgcn_sqrtf((float)d2[s]) - rmin_f) * inv_width_f);  // (a guess: v_sqrt_f32 as it is)
          k[s] = in[s] ? (g < 0 ? 0 : (g > nbins - 1 ? nbins - 1 : g)) : 0;
          lo[s] = s_t[k[s]], hi[s] = s_t[k[s] + 1];
        }
#pragma unroll
        for (int s = 0; s < kReg; ++s)
          if (in[s]) {
            if (d2[s] < lo[s] || d2[s] >= hi[s]) k[s] = walk(k[s], d2[s], s_t, nbins);
            atomicAdd(&hist[k[s]], weight);
          }
      }
    }
  }
  if (kOne) atomicAdd(&hist[0], weight * mine);
  __syncthreads();
  for (int e = tid; e < nbins; e += kBlock)
    if (hist[e]) atomicAdd(&counts[e], (unsigned long long)hist[e]);
}

// ---- checks ------------------------------------------------------------------------------
inline bool in_range(const int32_t *h, int64_t n, int64_t bound) {
  if (h)
    for (int64_t i = 0; i < n; ++i)
      if (h[i] < 0 || h[i] >= bound) return false;
  return true;
}

inline int check(const char *who, const void *xyz, int64_t fstride, int64_t n_frames, int64_t n_atoms,
                 const int32_t *h_idx_a, int64_t n_a, const int32_t *h_idx_b, int64_t n_b, int symmetric, int64_t excl_a,
                 int64_t excl_b, const double *h_box, double rmin, double rmax, int64_t nbins, const void *counts) {
  const std::string w(who);
  if (!xyz || !counts || n_frames < 1 || n_frames > INT32_MAX || n_atoms < 1 || n_atoms > INT32_MAX / 3 || n_a < 1 ||
      n_b < 1 || n_a > INT32_MAX || n_b > INT32_MAX || fstride < 3 * n_atoms)
    return fail(RMSF_EINVAL, w + ": bad arguments");
  if (nbins < 1 || nbins > kMaxBins) return fail(RMSF_EINVAL, w + ": nbins must be in 1..2048");
  if (!good_range(rmin, rmax, nbins))
    return fail(RMSF_EINVAL, w + ": the range needs 0 <= rmin < rmax, both finite");
  if (symmetric && n_a != n_b) return fail(RMSF_EINVAL, w + ": symmetric needs the same rows on both sides");
  if ((excl_a != 0) != (excl_b != 0) || excl_a < 0 || excl_b < 0 || (excl_a && (n_a % excl_a || n_b % excl_b)) ||
      (symmetric && excl_a != excl_b))
    return fail(RMSF_EINVAL, w + ": an exclusion block must divide its side (and be square on the symmetric route)");
  if (!in_range(h_idx_a, n_a, n_atoms) || !in_range(h_idx_b, n_b, n_atoms))
    return fail(RMSF_EINVAL, w + ": a row index is out of range");
  if (h_box)
    for (int64_t f = 0; f < n_frames; ++f)
      for (int k = 0; k < 3; ++k) {
        const double L = h_box[6 * f + k];
        if (!(std::isfinite(L) && L > 0.0)) return fail(RMSF_EINVAL, w + ": a box edge is not positive and finite");
        if (h_box[6 * f + 3 + k] != 1.0 / L) return fail(RMSF_EINVAL, w + ": a box's inverse edge is not 1.0 / edge");
        if (rmax > 0.5 * L)
          return fail(RMSF_EINVAL, w + ": rmax is over half a box edge: the minimum image is not the only one in range");
      }
  return RMSF_OK;
}

}  // namespace

extern "C" {

RMSF_EXPORT int rmsf_rdf_edges(double rmin, double rmax, int32_t nbins, double *h_edges, double *h_thresholds_sq) {
  if (!good_range(rmin, rmax, nbins)) return fail(RMSF_EINVAL, "rmsf_rdf_edges: 0 <= rmin < rmax, both finite, nbins in 1..2048");
  std::vector<double> e((size_t)nbins + 1);
  edges(rmin, rmax, nbins, e.data());
  if (h_edges) std::copy(e.begin(), e.end(), h_edges);
  if (h_thresholds_sq) thresholds(e.data(), nbins, h_thresholds_sq);
  return RMSF_OK;
}

RMSF_EXPORT int rmsf_rdf_counts_plan(int64_t n_a, int64_t n_b, int64_t n_frames, int symmetric, int32_t *tile_a,
                                     int32_t *tile_b, int32_t *frame_chunk, int32_t *n_splits) {
  if (n_a < 1 || n_b < 1 || n_frames < 1 || n_a > INT32_MAX || n_b > INT32_MAX || n_frames > INT32_MAX ||
      (symmetric && n_a != n_b) || !tile_a || !tile_b || !frame_chunk || !n_splits)
    return fail(RMSF_EINVAL, "rmsf_rdf_counts_plan: bad arguments");
  *tile_a = *tile_b = kTile;
  *frame_chunk = kChunk;
  *n_splits = (int32_t)plan(n_a, n_b, n_frames, symmetric).n_splits;
  return RMSF_OK;
}

RMSF_EXPORT size_t rmsf_rdf_counts_workspace_bytes(int32_t nbins) {
  return nbins >= 1 && nbins <= kMaxBins ? sizeof(double) * ((size_t)nbins + 1) : 0;  // the thresholds
}

RMSF_EXPORT int rmsf_rdf_counts(const float *d_xyz, int64_t frame_stride, int64_t n_frames, int64_t n_atoms,
                                const int32_t *d_idx_a, const int32_t *h_idx_a, int64_t n_a, const int32_t *d_idx_b,
                                const int32_t *h_idx_b, int64_t n_b, int symmetric, int64_t excl_a, int64_t excl_b,
                                const double *d_box, const double *h_box, double rmin, double rmax, int32_t nbins,
                                int64_t *d_counts, void *d_work, size_t work_bytes, void *stream) {
  const char *who = "rmsf_rdf_counts";
  if (int rc = check(who, d_xyz, frame_stride, n_frames, n_atoms, h_idx_a, n_a, h_idx_b, n_b, symmetric, excl_a,
                     excl_b, h_box, rmin, rmax, nbins, d_counts))
    return rc;
  if ((!d_idx_a && n_a > n_atoms) || (!d_idx_b && n_b > n_atoms))
    return fail(RMSF_EINVAL, "rmsf_rdf_counts: more dense rows than the frame has atoms");
  if ((d_box == nullptr) != (h_box == nullptr))
    return fail(RMSF_EINVAL, "rmsf_rdf_counts: the boxes need their device and their host copy");
  if (symmetric && d_idx_a != d_idx_b)
    return fail(RMSF_EINVAL, "rmsf_rdf_counts: symmetric needs the same rows on both sides");
  if (!d_work || work_bytes < rmsf_rdf_counts_workspace_bytes(nbins))
    return fail(RMSF_EINVAL, "rmsf_rdf_counts: the workspace is smaller than rmsf_rdf_counts_workspace_bytes");
  const Plan p = plan(n_a, n_b, n_frames, symmetric);
  if (p.tiles_a > 65535 || p.n_splits > kMaxSplits)
    return fail(RMSF_EINVAL, "rmsf_rdf_counts: more than 65535 tiles of rows");
  // The thresholds go through a buffer that outlives the copy; a pageable
  // source is staged before hipMemcpyAsync returns.
  static thread_local std::vector<double> table;
  table.resize(2 * ((size_t)nbins + 1));
  double *e = table.data(), *t = e + nbins + 1;
  edges(rmin, rmax, nbins, e);
  thresholds(e, nbins, t);
  hipError_t err = hipMemcpyAsync(d_work, t, sizeof(double) * ((size_t)nbins + 1), hipMemcpyHostToDevice, S(stream));
  if (err == hipSuccess) err = hipMemsetAsync(d_counts, 0, sizeof(int64_t) * (size_t)nbins, S(stream));
  if (err != hipSuccess) return fail(RMSF_EHIP, std::string(who) + ": " + hipGetErrorString(err));
  const size_t lds = sizeof(double) * ((size_t)nbins + 1) + sizeof(int32_t) * (size_t)nbins;
  const float rmin_f = (float)rmin, inv_width_f = (float)((double)nbins / (rmax - rmin));
  const dim3 grid((unsigned)p.tiles_b, (unsigned)p.tiles_a, (unsigned)p.n_splits);
#define RMSF_RDF(BOX, ONE)                                                                                        \
  hipLaunchKernelGGL((k_rdf_counts<BOX, ONE>), grid, dim3(kBlock), lds, S(stream), d_xyz, frame_stride, n_frames, \
                     d_idx_a, n_a, d_idx_b, n_b, symmetric, (int32_t)excl_a, (int32_t)excl_b, d_box,              \
                     static_cast<const double *>(d_work), (int)nbins, rmin_f, inv_width_f, p.per_split,           \
                     reinterpret_cast<unsigned long long *>(d_counts))
  if (d_box && nbins == 1)
    RMSF_RDF(true, true);
  else if (d_box)
    RMSF_RDF(true, false);
  else if (nbins == 1)
    RMSF_RDF(false, true);
  else
    RMSF_RDF(false, false);
#undef RMSF_RDF
  return after_launch("k_rdf_counts");
}

RMSF_EXPORT int rmsf_rdf_counts_host(const float *h_xyz, int64_t frame_stride, int64_t n_frames, int64_t n_atoms,
                                     const int32_t *h_idx_a, int64_t n_a, const int32_t *h_idx_b, int64_t n_b,
                                     int symmetric, int64_t excl_a, int64_t excl_b, const double *h_box, double rmin,
                                     double rmax, int32_t nbins, int64_t *h_counts) {
  if (int rc = check("rmsf_rdf_counts_host", h_xyz, frame_stride, n_frames, n_atoms, h_idx_a, n_a, h_idx_b, n_b,
                     symmetric, excl_a, excl_b, h_box, rmin, rmax, nbins, h_counts))
    return rc;
  if (symmetric && h_idx_a != h_idx_b)
    return fail(RMSF_EINVAL, "rmsf_rdf_counts_host: symmetric needs the same rows on both sides");
  if ((!h_idx_a && n_a > n_atoms) || (!h_idx_b && n_b > n_atoms))
    return fail(RMSF_EINVAL, "rmsf_rdf_counts_host: more dense rows than the frame has atoms");
  std::vector<double> e((size_t)nbins + 1);
  edges(rmin, rmax, nbins, e.data());
  for (int k = 0; k < nbins; ++k) h_counts[k] = 0;
  for (int64_t f = 0; f < n_frames; ++f) {
    const float *x = h_xyz + f * frame_stride;
    const double *bx = h_box ? h_box + 6 * f : nullptr;
    for (int64_t i = 0; i < n_a; ++i)
      for (int64_t j = 0; j < n_b; ++j) {
        if ((symmetric && i == j) || (excl_a && i / excl_a == j / excl_b)) continue;
        const float *pa = x + 3 * (int64_t)(h_idx_a ? h_idx_a[i] : i), *pb = x + 3 * (int64_t)(h_idx_b ? h_idx_b[j] : j);
        const double d2 = bx ? pair_image::dist2_box(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2], bx)
                             : pair_image::dist2_free(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2]);
        const int k = bin_of(std::sqrt(d2), e.data(), nbins);
        if (k >= 0) ++h_counts[k];
      }
  }
  return RMSF_OK;
}

}  // extern "C"
