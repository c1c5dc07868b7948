// pairwise.hip -- the all-pairs RMSD matrix of a trajectory's frames ("2D
// RMSD", what MDAnalysis.analysis.diffusionmap.DistanceMatrix produces) on
// the f64 matrix cores of gfx950 (MI355X, CDNA4), and the extern "C" launchers
// declared in include/rmsf_hip.h.
//
// covariance.hip contracts over frames and keeps the atoms' coordinates as
// rows; this is the same contraction turned on its side: over atoms, the
// frames' coordinates as rows.  For frames i, j the 3 x 3 inner product of
// qcprot,
//
//   A_ij = sum_a w_a (x_i,a - c_i) (x_j,a - c_j)^T,
//
// is one 3 x 3 block of the Gram matrix X W X^T; with E0 = (G_i + G_j) / 2,
// G_f = sum_a w_a |x_f,a - c_f|^2, the largest root of the QCP quartic gives
// the minimal RMSD without the rotation (Theobald 2005).
//
//   * k_pw_centres  one workgroup per frame: the weighted centre and G_f.
//   * k_pw_tiles    one workgroup per (macro tile pair, atom range): 16 frames
//                   = 48 coordinates a side, rows coordinate-major (row = 16 c
//                   + frame), 3 x 3 tiles of v_mfma_f64_16x16x4_f64 per wave.
//                   The deviations of 32 atoms are staged as f64 [atom][row]
//                   in LDS; each of the 4 waves contracts 8 of them.  With
//                   that row order one lane's nine accumulators hold the nine
//                   entries of A_ij of one frame pair per register.
//   * k_pw_fold     the split-K partials, summed in atom-range order.
//   * pair_epilogue lambda by Newton's iteration, by Jacobi on the key matrix
//                   where the largest root is not simple (or the trace,
//                   without superposition), the cutoff, the store and its
//                   mirror -- of the distances, or (rmsf_pairwise_adjacency)
//                   of the bits d <= radius alone, as 16-bit segments of the
//                   rows of csrc/clustering.hip's neighbour bits, so that the
//                   f64 matrix is never stored.
//
// The rectangle d[i, j] = RMSD(A_i, B_j) of two trajectories is the same
// contraction with a second operand side of its own (Side: base, stride,
// selection, centres, G), so both shapes are one kernel template, one fold,
// one plan (TilePlan) and one launcher (launch_tiles); the square fills both
// sides from the same arrays.  What stays with the shape (RECT):
//
//   * tiles_of_pair   the tile pairs J >= I of the square's upper triangle, or
//                     the whole tile rectangle, pair = I tiles_b + J;
//   * n_ops           an unweighted diagonal tile of the square stages one
//                     operand; the rectangle always both (operand 0 is the A
//                     tile and carries the weight);
//   * tile_epilogue   pair_epilogue, or cross_epilogue: the same distance
//                     without the mirror, one store a pair.
//
//   * k_row_argmin    one workgroup per row: the first least entry, a NaN
//                     below every number.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>

#include "dense_f64.h"
#include "rmsf_device.h"
#include "rmsf_host.h"

namespace {

constexpr int kTF = 16;                    // frames a side of a macro tile
constexpr int kTC = 3 * kTF;               // rows a side: 3 MFMA tiles (x, y, z of the 16 frames)
constexpr int kKA = 32;                    // atoms staged at a time (8 per wave: 2 MFMA k-steps)
constexpr int kPitch = kTC + 2;            // doubles a staged atom: 50, so the 16 atom lanes of a frame
                                           // store to 16 different LDS bank pairs
constexpr int kAtomLanes = kBlock / kTF;   // lanes of a frame, along its atoms (a frame's row is contiguous)
constexpr int kPasses = kKA / kAtomLanes;  // atoms a lane stages
constexpr int kPairs = kTF * kTF;          // frame pairs of a tile pair: one per thread
constexpr int kTile = 9 * kPairs;          // A_ij entries of a tile pair
constexpr int64_t kTargetGroups = 512;     // 2 resident workgroups per CU on MI355X
// Tile pairs a launch of k_pw_tiles: a grid's threads along x (workgroups x kBlock) must stay below 2^32 -- a
// launch of more is not refused, it runs the count modulo 2^32 (seen at 200,000 frames, 78 M tile pairs: 14 % of
// them ran) -- so more pairs than this go in several launches.
constexpr int64_t kMaxGroups = int64_t(1) << 23;

static_assert(kPairs == kBlock, "the epilogue gives every thread one frame pair");
static_assert(kTile <= 2 * kKA * kPitch, "the waves' sum reuses the staging buffer");
static_assert(sizeof(double) * (2 * kKA * kPitch + kTF * (kTF + 1)) <= kLdsLimit, "sm and sd fit");

// One operand side of a tile pair: n frames at xyz + f fstride, their
// selection (NULL: atoms 0..n_sel-1), centres and G.  The square matrix has
// the same side twice.
struct Side {
  const float *xyz;
  int64_t fstride;
  int64_t n;
  const int32_t *sel;
  const double *centre;
  const double *g;
};

// The work decomposition, a function of the frame counts and n_sel alone, so
// the workspace layout and the summation order are fixed by the sizes.
struct TilePlan {
  int64_t tiles_a, tiles_b;  // macro tiles a side (the square: the same twice)
  int64_t n_pairs;           // tile pairs: J >= I of the square, pair = I tiles_b + J of the rectangle;
                             // 0 = a rectangle of more than a launch sequence takes
  int64_t n_ks;              // atom ranges (split-K); 1 = the epilogue runs in k_pw_tiles
  int64_t ks_atoms;          // atoms per range, a multiple of kKA
};

TilePlan tile_plan(int64_t tiles_a, int64_t tiles_b, int64_t n_pairs, int64_t n_sel) {
  TilePlan p{tiles_a, tiles_b, n_pairs, 0, 0};
  if (n_pairs == 0) return p;
  const SplitK k = split_k(std::max<int64_t>(1, (n_sel + kKA - 1) / kKA), n_pairs, kTargetGroups, 1);
  p.n_ks = k.n_ks;
  p.ks_atoms = k.per * kKA;
  return p;
}

TilePlan pw_plan(int64_t n_frames, int64_t n_sel) {
  const int64_t t = (n_frames + kTF - 1) / kTF;
  return tile_plan(t, t, t * (t + 1) / 2, n_sel);
}

TilePlan cross_plan(int64_t n_a, int64_t n_b, int64_t n_sel) {
  const int64_t ta = (n_a + kTF - 1) / kTF, tb = (n_b + kTF - 1) / kTF;
  // (each factor first: the product of two int64 tile counts may not fit)
  const bool fits = ta <= INT32_MAX && tb <= INT32_MAX && ta * tb <= INT32_MAX;
  return tile_plan(ta, tb, fits ? ta * tb : 0, n_sel);
}

size_t work_doubles(const TilePlan &p) {
  if (p.n_ks <= 1) return 0;
  return (size_t)p.n_ks * (size_t)p.n_pairs * kTile;
}

// Sum of v over the workgroup in a fixed order (a halving tree over LDS);
// every thread returns the total.
__device__ __forceinline__ double block_sum(double v, double *__restrict__ sh) {
  const int tid = threadIdx.x;
  __syncthreads();  // sh may still be read from the call before
  sh[tid] = v;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] = sh[tid] + sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

// One workgroup per frame f: c = sum_a w_a x_a / sum_a w_a over the frame
// (over frame 0 when !per_frame: a common shift; `about`, three doubles, when
// given: a shift found elsewhere), then G = sum_a w_a |x_f,a - c|^2.
// Each thread adds its atoms in order, the threads are added by block_sum.
template <bool GATHER>
__global__ __launch_bounds__(kBlock) void k_pw_centres(const float *__restrict__ xyz, int64_t fstride, int64_t n_sel,
                                                       const int32_t *__restrict__ sel,
                                                       const double *__restrict__ weights, int per_frame,
                                                       const double *__restrict__ about,
                                                       double *__restrict__ centre, double *__restrict__ g) {
  __shared__ double sh[kBlock];
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.x;
  double c0, c1, c2;
  if (about) {  // (the same for every thread of the grid)
    c0 = about[0], c1 = about[1], c2 = about[2];
  } else {
    const float *__restrict__ src = xyz + (per_frame ? f : 0) * fstride;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, sw = 0.0;
    for (int64_t a = tid; a < n_sel; a += kBlock) {
      const float *__restrict__ q = src + 3 * (GATHER ? (int64_t)sel[a] : a);
      const double w = weights ? weights[a] : 1.0;
      s0 += w * (double)q[0], s1 += w * (double)q[1], s2 += w * (double)q[2], sw += w;
    }
    s0 = block_sum(s0, sh), s1 = block_sum(s1, sh), s2 = block_sum(s2, sh), sw = block_sum(sw, sh);
    c0 = s0 / sw, c1 = s1 / sw, c2 = s2 / sw;
  }
  const float *__restrict__ own = xyz + f * fstride;
  double gs = 0.0;
  for (int64_t a = tid; a < n_sel; a += kBlock) {
    const float *__restrict__ q = own + 3 * (GATHER ? (int64_t)sel[a] : a);
    const double w = weights ? weights[a] : 1.0;
    const double d0 = (double)q[0] - c0, d1 = (double)q[1] - c1, d2 = (double)q[2] - c2;
    gs += w * (d0 * d0 + d1 * d1 + d2 * d2);
  }
  gs = block_sum(gs, sh);
  if (tid == 0) {
    centre[3 * f] = c0, centre[3 * f + 1] = c1, centre[3 * f + 2] = c2;
    g[f] = gs;
  }
}

// The distance of one pair from its A_ij and the two frames' G: lambda as
// pair_lambda finds it (rmsf_device.h: Newton's iteration as in qcp_solve,
// the key matrix' largest eigenvalue where the largest root is not simple),
// or the trace without superposition; then the cutoff.
__device__ __forceinline__ double pair_distance(const double *A, double gi, double gj, int superpose,
                                                double w_total, double cutoff) {
  double d;
  if (superpose) {
    const double E0 = (gi + gj) * 0.5;
    int path;
    const double l = pair_lambda(A, E0, &path);
    d = sqrt(fabs(2.0 * (E0 - l)) / w_total);
  } else {
    d = sqrt(fabs(gi + gj - 2.0 * (A[0] + A[4] + A[8])) / w_total);
  }
  return d <= cutoff ? 0.0 : d;
}

// What a tile pair stores: its distances as f64, or (BITS) only whether each is
// within a radius -- rows of the neighbour bits of csrc/clustering.hip, which
// are addressed here in the 16-bit quarters of their 64-bit words: tile column
// J of a row is element J of uint16 [n][4 ldw].
template <bool BITS>
using PairOut = std::conditional_t<BITS, uint16_t, double>;

// The 16 predicates of tile row (tid >> 4), one a lane, as that row's segment
// of the bit matrix: a wave is 4 tile rows x 16 columns, so its ballot is four
// such segments, and the row's first lane stores its own with one 2-byte
// vector store.  Tiles that share a 64-bit word write different quarters of
// it, so no store meets another.  With `tail` (the last tile column of the
// row) the quarters of the row's last word that no tile covers are cleared
// too: elements [n_tiles, quarters).  Called by every lane of every wave.
__device__ __forceinline__ void store_row_bits(bool bit, bool row_in, uint16_t *__restrict__ row, int64_t q,
                                               bool tail, int64_t n_tiles, int64_t quarters) {
  const int lane = threadIdx.x & 63;
  const uint64_t b = __ballot(bit);
  if ((lane & 15) == 0 && row_in) {
    row[q] = (uint16_t)(b >> (lane & 48));
    if (tail)
      for (int64_t z = n_tiles; z < quarters; ++z) row[z] = 0;
  }
}

// pair_epilogue's BITS form: bit (i, j) = (i == j) || (d <= radius) of the
// same d (a NaN is never within it), columns >= n_frames 0, rows >= n_frames
// not written; the mirror's predicate is read from sd as the f64 mirror is.
__device__ __forceinline__ void pair_epilogue_bits(double d, int64_t I, int64_t J, int64_t n_frames, double radius,
                                                   uint16_t *__restrict__ out, int64_t ld,
                                                   double (*__restrict__ sd)[kTF + 1]) {
  const int tid = threadIdx.x;
  const int fi = tid >> 4, fj = tid & 15;
  const int64_t i = kTF * I + fi, j = kTF * J + fj;
  const bool in = i < n_frames && j < n_frames;
  const int64_t n_tiles = (n_frames + kTF - 1) / kTF, quarters = 4 * ((n_frames + 63) / 64);
  const bool tail = J == n_tiles - 1;
  if (I == J) {
    if (fj > fi) sd[fi][fj] = d, sd[fj][fi] = d;
    if (fj == fi) sd[fi][fi] = 0.0;
    __syncthreads();
    store_row_bits(in && (fi == fj || sd[fi][fj] <= radius), i < n_frames, out + i * ld, J, tail, n_tiles, quarters);
  } else {
    sd[fi][fj] = d;
    store_row_bits(in && d <= radius, i < n_frames, out + i * ld, J, tail, n_tiles, quarters);
    __syncthreads();
    const int64_t jj = kTF * J + fi, ii = kTF * I + fj;  // row of tile J, column of tile I
    store_row_bits(jj < n_frames && ii < n_frames && sd[fj][fi] <= radius, jj < n_frames, out + jj * ld, I, false,
                   n_tiles, quarters);
  }
}

// Thread tid owns the frame pair (fi = tid >> 4 of tile I, fj = tid & 15 of
// tile J) and its A_ij.  Pairs j > i are computed; each value goes to [i, j]
// and, through LDS so that both stores run along rows, to [j, i]; the
// diagonal is written as 0.  BITS: the same distances, stored as neighbour
// bits within `radius` (pair_epilogue_bits).  Called by every thread of the
// workgroup.
template <bool BITS>
__device__ __forceinline__ void pair_epilogue(const double *A, int64_t I, int64_t J, int64_t n_frames,
                                              const double *__restrict__ g, int superpose, double w_total,
                                              double cutoff, double radius, PairOut<BITS> *__restrict__ out,
                                              int64_t ld, double (*__restrict__ sd)[kTF + 1]) {
  const int tid = threadIdx.x;
  const int fi = tid >> 4, fj = tid & 15;
  const int64_t i = kTF * I + fi, j = kTF * J + fj;
  const bool in = i < n_frames && j < n_frames;
  double d = 0.0;
  if (in && j > i) d = pair_distance(A, g[i], g[j], superpose, w_total, cutoff);
  if constexpr (BITS) {
    pair_epilogue_bits(d, I, J, n_frames, radius, out, ld, sd);
  } else if (I == J) {
    // the tile is its own mirror image: the upper half fills both
    if (fj > fi) sd[fi][fj] = d, sd[fj][fi] = d;
    if (fj == fi) sd[fi][fi] = 0.0;
    __syncthreads();
    if (in) out[i * ld + j] = sd[fi][fj];
  } else {
    if (in) out[i * ld + j] = d;
    sd[fi][fj] = d;
    __syncthreads();
    const int64_t jj = kTF * J + fi, ii = kTF * I + fj;  // row of tile J, column of tile I
    if (jj < n_frames && ii < n_frames) out[jj * ld + ii] = sd[fj][fi];
  }
}

// Thread tid owns the pair (fi = tid >> 4 of A's tile I, fj = tid & 15 of B's
// tile J) and its A_ij: pair_epilogue's arithmetic, one store, no mirror (fj
// is the fastest index: the stores of 16 lanes run along a row).
__device__ __forceinline__ void cross_epilogue(const double *A, int64_t I, int64_t J, int64_t n_a, int64_t n_b,
                                               const double *__restrict__ g_a, const double *__restrict__ g_b,
                                               int superpose, double w_total, double cutoff,
                                               double *__restrict__ out, int64_t ld) {
  const int tid = threadIdx.x;
  const int64_t i = kTF * I + (tid >> 4), j = kTF * J + (tid & 15);
  if (i >= n_a || j >= n_b) return;
  out[i * ld + j] = pair_distance(A, g_a[i], g_b[j], superpose, w_total, cutoff);
}

// What differs between the two shapes, for k_pw_tiles and k_pw_fold alike: the
// tile pair of a pair index, and the epilogue -- the square's with its sd tile
// (the tile's distances, for the mirrored store) from side a alone.
template <bool RECT>
__device__ __forceinline__ void tiles_of_pair(int64_t pair, int64_t tiles_b, int64_t &I, int64_t &J) {
  if constexpr (RECT) {
    I = pair / tiles_b, J = pair - I * tiles_b;
  } else {
    pair_to_tiles(pair, tiles_b, I, J);
  }
}

template <bool RECT, bool BITS>
__device__ __forceinline__ void tile_epilogue(const double *A, int64_t I, int64_t J, int64_t n_a, int64_t n_b,
                                              const double *__restrict__ g_a, const double *__restrict__ g_b,
                                              int superpose, double w_total, double cutoff, double radius,
                                              PairOut<BITS> *__restrict__ out, int64_t ld) {
  if constexpr (RECT) {
    cross_epilogue(A, I, J, n_a, n_b, g_a, g_b, superpose, w_total, cutoff, out, ld);
  } else {
    __shared__ double sd[kTF][kTF + 1];
    pair_epilogue<BITS>(A, I, J, n_a, g_a, superpose, w_total, cutoff, radius, out, ld, sd);
  }
}

// One workgroup: tile pair pair0 + blockIdx.x, atoms [blockIdx.y ks_atoms, ...),
// of the square (tiles J >= I of side sa against itself; sb is not read) or,
// RECT, of the rectangle (tile I of sa against tile J of sb).
// Staging: lane (tid & 15) walks the atoms of frame (tid >> 4) of the tile;
// its three deviations f64(x) - c_f go to sm[op][atom k][16 c + frame]
// (operand 0, the tile of sa, times the atom's weight), so an MFMA operand
// (mfma_3x3, dense_f64.h) is 16 consecutive doubles of staged atom k, and
// acc[ci][cj][reg] of lane l is entry (ci, cj) of A_ij for frames
// i = (l >> 4) + 4 reg of tile I and j = l & 15 of tile J.  An unweighted
// diagonal tile of the square stages one operand and contracts it with itself;
// a tile of A and a tile of B are different data also where I = J.  GATHER:
// some side has a selection -- which, is the same for the whole grid.
template <bool GATHER, bool WEIGHTED, bool RECT, bool BITS>
__global__ __launch_bounds__(kBlock, 2) void k_pw_tiles(Side sa, Side sb_rect, int64_t n_sel,
                                                     const double *__restrict__ weights, int superpose,
                                                     double w_total, double cutoff, double radius,
                                                     PairOut<BITS> *__restrict__ out, int64_t ld,
                                                     double *__restrict__ work, int64_t tiles_b, int64_t n_pairs,
                                                     int64_t ks_atoms, int direct, int64_t pair0) {
  __shared__ double sm[2 * kKA * kPitch];  // A then B deviations; reused for the waves' sum

  const Side &sb = RECT ? sb_rect : sa;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ta = tid & (kAtomLanes - 1), tf = tid >> 4;
  const int64_t pair = pair0 + blockIdx.x, ks = blockIdx.y;
  int64_t I, J;
  tiles_of_pair<RECT>(pair, tiles_b, I, J);
  // a weighted diagonal tile still needs both operands: w d and d
  const int n_ops = (!RECT && I == J && !WEIGHTED) ? 1 : 2;

  const int64_t a0 = ks * ks_atoms;
  const int64_t a1 = a0 + ks_atoms < n_sel ? a0 + ks_atoms : n_sel;

  // The lane's frame of each operand tile: its row, its centre, and whether
  // it exists.  A lane past a side's last frame reads that side's last frame
  // instead (and an atom past the range's end the range's last atom), so every
  // load is unconditional and in bounds, and its deviation is zeroed after.
  const float *p_op[2];
  const int32_t *sel_op[2];
  double cen[2][3];
  bool live[2];
#pragma unroll
  for (int op = 0; op < 2; ++op) {
    const Side &s = op ? sb : sa;
    const int64_t f = kTF * (op ? J : I) + tf;
    live[op] = f < s.n;
    const int64_t fc = live[op] ? f : s.n - 1;
    p_op[op] = s.xyz + fc * s.fstride;
    sel_op[op] = s.sel;
    cen[op][0] = s.centre[3 * fc], cen[op][1] = s.centre[3 * fc + 1], cen[op][2] = s.centre[3 * fc + 2];
  }

  f64x4 acc[3][3];
  zero_3x3(acc);

  const double *sA = sm;
  const double *sB = n_ops == 1 ? sm : sm + kKA * kPitch;

  // The next stage's floats are loaded into registers before the current
  // stage's MFMAs, so the global-load latency runs under the matrix pipe;
  // they become deviations in LDS after.
  float raw[2][kPasses][3];
  double wv[kPasses];
  auto prefetch = [&](int64_t ab) {
#pragma unroll
    for (int pass = 0; pass < kPasses; ++pass) {
      const int64_t a = ab + pass * kAtomLanes + ta;
      const int64_t ac = a < a1 ? a : a1 - 1;
      if (WEIGHTED) wv[pass] = weights[ac];
#pragma unroll
      for (int op = 0; op < 2; ++op) {
        if (op >= n_ops) break;
        // (the square's one selection is there whenever GATHER is)
        const int64_t row = 3 * (GATHER && (!RECT || sel_op[op]) ? (int64_t)sel_op[op][ac] : ac);
        const float *__restrict__ q = p_op[op] + row;
        raw[op][pass][0] = q[0], raw[op][pass][1] = q[1], raw[op][pass][2] = q[2];
      }
    }
  };
  prefetch(a0);

  for (int64_t ab = a0; ab < a1; ab += kKA) {
    // ---- stage kKA atoms of both operand tiles (zeros past either edge)
#pragma unroll
    for (int op = 0; op < 2; ++op) {
      if (op >= n_ops) break;
#pragma unroll
      for (int pass = 0; pass < kPasses; ++pass) {
        const int k = pass * kAtomLanes + ta;
        const bool on = live[op] && ab + k < a1;
        double d0 = on ? (double)raw[op][pass][0] - cen[op][0] : 0.0;
        double d1 = on ? (double)raw[op][pass][1] - cen[op][1] : 0.0;
        double d2 = on ? (double)raw[op][pass][2] - cen[op][2] : 0.0;
        if (WEIGHTED && op == 0) d0 *= wv[pass], d1 *= wv[pass], d2 *= wv[pass];
        double *__restrict__ o = sm + (op * kKA + k) * kPitch + tf;
        o[0] = d0, o[kTF] = d1, o[2 * kTF] = d2;
      }
    }
    __syncthreads();
    // (after the barrier: its fence waits for every load in flight)
    if (ab + kKA < a1) prefetch(ab + kKA);
    // ---- contract: wave w takes atoms [8 w, 8 w + 8) of the staged tile
#pragma unroll
    for (int s = 0; s < kKA / (4 * kWaves); ++s) {
      const int k = (kKA / kWaves) * wave + 4 * s + (lane >> 4);
      const double *__restrict__ ra = sA + k * kPitch + (lane & 15);
      const double *__restrict__ rb = sB + k * kPitch + (lane & 15);
      const double x0 = ra[0], x1 = ra[kTF], x2 = ra[2 * kTF];
      const double y0 = rb[0], y1 = rb[kTF], y2 = rb[2 * kTF];
      mfma_3x3(acc, x0, x1, x2, y0, y1, y2);
    }
    __syncthreads();
  }

  // ---- the four waves' accumulators, summed in wave order: entry
  // q = 3 ci + cj of the pair (fi = row, fj = col) lands at sm[256 q + 16 fi + fj]
  wave_sum_3x3(acc, sm, lane, wave,
               [](int i, int j, int row, int col) { return kPairs * (3 * i + j) + kTF * row + col; });

  if (direct) {
    double A[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) A[q] = sm[kPairs * q + tid];
    tile_epilogue<RECT, BITS>(A, I, J, sa.n, sb.n, sa.g, sb.g, superpose, w_total, cutoff, radius, out, ld);
  } else {
    double *__restrict__ w = work + ((int64_t)ks * n_pairs + pair) * kTile;
    for (int e = tid; e < kTile; e += kBlock) w[e] = sm[e];
  }
}

// The n_ks partials of every A_ij entry, summed in atom-range order, then
// the epilogue.  One workgroup per tile pair.
template <bool RECT, bool BITS>
__global__ __launch_bounds__(kBlock) void k_pw_fold(const double *__restrict__ work, int64_t n_a, int64_t n_b,
                                                    int64_t tiles_b, int64_t n_pairs, int64_t n_ks,
                                                    const double *__restrict__ g_a, const double *__restrict__ g_b,
                                                    int superpose, double w_total, double cutoff, double radius,
                                                    PairOut<BITS> *__restrict__ out, int64_t ld) {
  const int tid = threadIdx.x;
  const int64_t pair = blockIdx.x;
  int64_t I, J;
  tiles_of_pair<RECT>(pair, tiles_b, I, J);
  double A[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const double *__restrict__ w = work + pair * kTile + kPairs * q + tid;
    double s = 0.0;
    for (int64_t k = 0; k < n_ks; ++k) s += w[k * n_pairs * kTile];
    A[q] = s;
  }
  tile_epilogue<RECT, BITS>(A, I, J, n_a, n_b, g_a, g_b, superpose, w_total, cutoff, radius, out, ld);
}

// One workgroup per row of m[n_rows][ld]: its least entry and that entry's
// lowest column.  Thread t scans columns t, t + 256, ... in order with a
// strict <, so it keeps the first of equal values; the threads are then
// joined by a halving tree that prefers the lower column among equal values --
// the result is the same as one left-to-right scan.  A NaN counts as below
// every number and equal to another NaN (numpy.argmin's order): a row that
// holds one returns its first NaN.
__device__ __forceinline__ bool argmin_below(double v, double than) {
  return v < than || (v != v && than == than);
}

__global__ __launch_bounds__(kBlock) void k_row_argmin(const double *__restrict__ m, int64_t n_cols, int64_t ld,
                                                       int64_t *__restrict__ idx, double *__restrict__ val) {
  __shared__ double sv[kBlock];
  __shared__ int64_t si[kBlock];
  const int tid = threadIdx.x;
  const double *__restrict__ row = m + (int64_t)blockIdx.x * ld;
  double bv = INFINITY;
  int64_t bi = INT64_MAX;  // a thread without a column never wins a tie
  if (tid < n_cols) bv = row[tid], bi = tid;
  for (int64_t c = (int64_t)tid + kBlock; c < n_cols; c += kBlock) {
    const double v = row[c];
    if (argmin_below(v, bv)) bv = v, bi = c;
  }
  sv[tid] = bv, si[tid] = bi;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const double ov = sv[tid + s];
      const int64_t oi = si[tid + s];
      const double mv = sv[tid];
      // (neither below the other: equal, or both NaN)
      if (argmin_below(ov, mv) || (!argmin_below(mv, ov) && oi < si[tid])) sv[tid] = ov, si[tid] = oi;
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (idx) idx[blockIdx.x] = si[0];
    if (val) val[blockIdx.x] = sv[0];
  }
}

// k_pw_centres for n_frames frames, about each frame's own centre, frame 0's
// (per_frame = 0) or d_about (when given).  The arguments are the caller's,
// already checked; `who` names it in the message.
int launch_centres(const char *who, const float *d_xyz, int64_t fstride, int64_t n_frames, int64_t n_sel,
                   const int32_t *d_sel, const double *d_weights, int per_frame, const double *d_about,
                   double *d_centre, double *d_g, void *stream) {
  if (n_frames > INT32_MAX) return fail(RMSF_EINVAL, std::string(who) + ": too many frames for one launch");
  if (n_frames == 0) return RMSF_OK;
  const dim3 grid((unsigned)n_frames), block(kBlock);
  if (d_sel)
    hipLaunchKernelGGL(k_pw_centres<true>, grid, block, 0, S(stream), d_xyz, fstride, n_sel, d_sel, d_weights,
                       per_frame, d_about, d_centre, d_g);
  else
    hipLaunchKernelGGL(k_pw_centres<false>, grid, block, 0, S(stream), d_xyz, fstride, n_sel, d_sel, d_weights,
                       per_frame, d_about, d_centre, d_g);
  return after_launch("k_pw_centres");
}

// k_pw_tiles and, with more than one atom range, k_pw_fold over every tile
// pair of the plan: of the square of side sa (sb the same), storing distances
// (out f64 [n][ld]) or, BITS, the neighbour bits within `radius` (out uint16
// [n][ld], ld in 16-bit elements), or, RECT, of the rectangle sa x sb.
// Everything that can be refused is refused before the first launch; the
// pointers and sizes that do not depend on the plan are the caller's, already
// checked, and `who` names it in the messages.
template <bool RECT, bool BITS>
int launch_tiles(const char *who, const TilePlan &pl, const Side &sa, const Side &sb, int64_t n_sel,
                 const double *d_weights, double w_total, int superpose, double cutoff, double radius,
                 PairOut<BITS> *d_out, int64_t ld, void *d_work, size_t work_bytes, void *stream) {
  if (pl.n_pairs == 0 || pl.n_pairs > INT32_MAX || pl.n_ks > 65535)
    return fail(RMSF_EINVAL, std::string(who) + ": too many frames for one launch");
  const size_t need = work_doubles(pl) * sizeof(double);
  if (need && (!d_work || work_bytes < need)) return fail(RMSF_ENOMEM, std::string(who) + ": workspace too small");
  const int direct = pl.n_ks == 1;
  double *work = static_cast<double *>(d_work);
  const dim3 block(kBlock);
#define PW_LAUNCH(G_, W_)                                                                                       \
  hipLaunchKernelGGL((k_pw_tiles<G_, W_, RECT, BITS>), grid, block, 0, S(stream), sa, sb, n_sel, d_weights,      \
                     superpose, w_total, cutoff, radius, d_out, ld, work, pl.tiles_b, pl.n_pairs, pl.ks_atoms, \
                     direct, p0)
  const bool gt = sa.sel != nullptr || sb.sel != nullptr, wt = d_weights != nullptr;
  // kMaxGroups tile pairs a launch (past 256 tile pairs there is one atom range, and below there is one launch)
  for (int64_t p0 = 0; p0 < pl.n_pairs; p0 += kMaxGroups) {
    const dim3 grid((unsigned)std::min<int64_t>(kMaxGroups, pl.n_pairs - p0), (unsigned)pl.n_ks);
    if (gt && wt) PW_LAUNCH(true, true);
    else if (gt) PW_LAUNCH(true, false);
    else if (wt) PW_LAUNCH(false, true);
    else PW_LAUNCH(false, false);
    if (int rc = after_launch("k_pw_tiles")) return rc;
  }
#undef PW_LAUNCH
  if (!direct) {
    hipLaunchKernelGGL((k_pw_fold<RECT, BITS>), dim3((unsigned)pl.n_pairs), block, 0, S(stream), work, sa.n, sb.n,
                       pl.tiles_b, pl.n_pairs, pl.n_ks, sa.g, sb.g, superpose, w_total, cutoff, radius, d_out, ld);
    if (int rc = after_launch("k_pw_fold")) return rc;
  }
  return RMSF_OK;
}

// launch_tiles over the square of one trajectory's frames.
template <bool BITS>
int launch_pairs(const char *who, const float *d_xyz, int64_t fstride, int64_t n_frames, int64_t n_sel,
                 const int32_t *d_sel, const double *d_weights, double w_total, const double *d_centre,
                 const double *d_g, int superpose, double cutoff, double radius, PairOut<BITS> *d_out, int64_t ld,
                 void *d_work, size_t work_bytes, void *stream) {
  if (n_frames == 0) return RMSF_OK;
  const Side s{d_xyz, fstride, n_frames, d_sel, d_centre, d_g};
  return launch_tiles<false, BITS>(who, pw_plan(n_frames, n_sel), s, s, n_sel, d_weights, w_total, superpose, cutoff,
                                   radius, d_out, ld, d_work, work_bytes, stream);
}

}  // namespace

extern "C" {

RMSF_EXPORT int rmsf_pairwise_centres(const float *d_xyz, int64_t fstride, int64_t n_frames, int64_t n_sel,
                                      const int32_t *d_sel, const double *d_weights, int per_frame,
                                      double *d_centre, double *d_g, void *stream) {
  if (!d_xyz || !d_centre || !d_g || n_sel < 1 || n_frames < 0 || fstride < 0)
    return fail(RMSF_EINVAL, "rmsf_pairwise_centres: bad arguments");
  return launch_centres("rmsf_pairwise_centres", d_xyz, fstride, n_frames, n_sel, d_sel, d_weights, per_frame,
                        nullptr, d_centre, d_g, stream);
}

RMSF_EXPORT int rmsf_pairwise_centres_about(const float *d_xyz, int64_t fstride, int64_t n_frames, int64_t n_sel,
                                            const int32_t *d_sel, const double *d_weights, const double *d_about,
                                            double *d_centre, double *d_g, void *stream) {
  if (!d_xyz || !d_about || !d_centre || !d_g || n_sel < 1 || n_frames < 0 || fstride < 0)
    return fail(RMSF_EINVAL, "rmsf_pairwise_centres_about: bad arguments");
  return launch_centres("rmsf_pairwise_centres_about", d_xyz, fstride, n_frames, n_sel, d_sel, d_weights, 0,
                        d_about, d_centre, d_g, stream);
}

RMSF_EXPORT size_t rmsf_pairwise_workspace_bytes(int64_t n_frames, int64_t n_sel) {
  if (n_sel < 1 || n_frames < 1) return 0;
  return work_doubles(pw_plan(n_frames, n_sel)) * sizeof(double);
}

RMSF_EXPORT int rmsf_pairwise_rmsd(const float *d_xyz, int64_t fstride, int64_t n_frames, int64_t n_sel,
                                   const int32_t *d_sel, const double *d_weights, double w_total,
                                   const double *d_centre, const double *d_g, int superpose, double cutoff,
                                   double *d_out, int64_t ld, void *d_work, size_t work_bytes, void *stream) {
  if (!d_xyz || !d_centre || !d_g || !d_out || n_sel < 1 || n_frames < 0 || fstride < 0 || ld < n_frames ||
      !(w_total > 0.0))
    return fail(RMSF_EINVAL, "rmsf_pairwise_rmsd: bad arguments");
  return launch_pairs<false>("rmsf_pairwise_rmsd", d_xyz, fstride, n_frames, n_sel, d_sel, d_weights, w_total,
                             d_centre, d_g, superpose, cutoff, 0.0, d_out, ld, d_work, work_bytes, stream);
}

RMSF_EXPORT int rmsf_pairwise_adjacency(const float *d_xyz, int64_t fstride, int64_t n_frames, int64_t n_sel,
                                        const int32_t *d_sel, const double *d_weights, double w_total,
                                        const double *d_centre, const double *d_g, int superpose,
                                        double zero_cutoff, double cutoff, uint64_t *d_adj, int64_t ldw,
                                        int32_t *d_count, void *d_work, size_t work_bytes, void *stream) {
  if (!d_xyz || !d_centre || !d_g || !d_adj || n_sel < 1 || n_frames < 0 || fstride < 0 ||
      ldw < rmsf_adjacency_words(n_frames) || !(w_total > 0.0) || !(cutoff >= 0.0))
    return fail(RMSF_EINVAL, "rmsf_pairwise_adjacency: bad arguments");
  // a row as its 16-bit quarters: tile column J is element J of uint16 [n_frames][4 ldw]
  if (int rc = launch_pairs<true>("rmsf_pairwise_adjacency", d_xyz, fstride, n_frames, n_sel, d_sel, d_weights,
                                  w_total, d_centre, d_g, superpose, zero_cutoff, cutoff,
                                  reinterpret_cast<uint16_t *>(d_adj), 4 * ldw, d_work, work_bytes, stream))
    return rc;
  if (!d_count || n_frames == 0) return RMSF_OK;
  return rmsf_adjacency_count(d_adj, n_frames, ldw, d_count, stream);
}

RMSF_EXPORT size_t rmsf_cross_workspace_bytes(int64_t n_a, int64_t n_b, int64_t n_sel) {
  if (n_sel < 1 || n_a < 1 || n_b < 1) return 0;
  return work_doubles(cross_plan(n_a, n_b, n_sel)) * sizeof(double);
}

RMSF_EXPORT int rmsf_cross_rmsd(const float *d_a, int64_t stride_a, int64_t n_a, const int32_t *d_sel_a,
                                const double *d_centre_a, const double *d_g_a, const float *d_b, int64_t stride_b,
                                int64_t n_b, const int32_t *d_sel_b, const double *d_centre_b, const double *d_g_b,
                                int64_t n_sel, const double *d_weights, double w_total, int superpose,
                                double cutoff, double *d_out, int64_t ld, void *d_work, size_t work_bytes,
                                void *stream) {
  if (!d_a || !d_centre_a || !d_g_a || !d_b || !d_centre_b || !d_g_b || !d_out || n_sel < 1 || n_a < 0 || n_b < 0 ||
      stride_a < 0 || stride_b < 0 || ld < n_b || !(w_total > 0.0))
    return fail(RMSF_EINVAL, "rmsf_cross_rmsd: bad arguments");
  if (n_a == 0 || n_b == 0) return RMSF_OK;
  const Side sa{d_a, stride_a, n_a, d_sel_a, d_centre_a, d_g_a};
  const Side sb{d_b, stride_b, n_b, d_sel_b, d_centre_b, d_g_b};
  return launch_tiles<true, false>("rmsf_cross_rmsd", cross_plan(n_a, n_b, n_sel), sa, sb, n_sel, d_weights, w_total,
                                   superpose, cutoff, 0.0, d_out, ld, d_work, work_bytes, stream);
}

RMSF_EXPORT int rmsf_row_argmin(const double *d_m, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t *d_idx,
                                double *d_val, void *stream) {
  if (!d_m || (!d_idx && !d_val) || n_rows < 0 || n_cols < 1 || ld < n_cols)
    return fail(RMSF_EINVAL, "rmsf_row_argmin: bad arguments");
  if (n_rows > INT32_MAX) return fail(RMSF_EINVAL, "rmsf_row_argmin: too many rows for one launch");
  if (n_rows == 0) return RMSF_OK;
  hipLaunchKernelGGL(k_row_argmin, dim3((unsigned)n_rows), dim3(kBlock), 0, S(stream), d_m, n_cols, ld, d_idx, d_val);
  return after_launch("k_row_argmin");
}

RMSF_EXPORT int rmsf_pair_lambda_host(const double *h_A, const double *h_E0, int64_t n, double *h_lambda,
                                      int32_t *h_path) {
  if (!h_A || !h_E0 || !h_lambda || n < 0) return fail(RMSF_EINVAL, "rmsf_pair_lambda_host: bad arguments");
  for (int64_t k = 0; k < n; ++k) {
    int path;
    h_lambda[k] = pair_lambda(h_A + 9 * k, h_E0[k], &path);
    if (h_path) h_path[k] = path;
  }
  return RMSF_OK;
}

}  // extern "C"
