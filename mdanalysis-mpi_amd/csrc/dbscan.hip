// dbscan.hip -- DBSCAN (Ester et al. 1996, as scikit-learn states it) on the
// neighbour bits of csrc/clustering.hip, all integers ("DBSCAN").
//
//   core[i] = count[i] >= min_samples.  Clusters are the connected components
//   of adj restricted to core x core; a cluster's id is the rank of its lowest
//   core index; a non-core row with a core neighbour takes the lowest id among
//   its core neighbours' clusters; every other row is noise, -1.
//
// Components by min-hooking with shortcutting (the FastSV family: Zhang, Azad
// and Hu 2020).  f is a forest over the core rows, f[i] <= i, f[i] in i's
// component.  A round reads f and gf[j] = f[f[j]] and writes fn, which starts
// as a copy of f:
//   m = min over the core neighbours j of row i (i among them) of gf[j]
//   fn[f[i]] = min(fn[f[i]], m)     the hook on the parent
//   fn[i]    = min(fn[i], m)        the hook on the row; m <= gf[i], so this
//                                    is the shortcut too
// The hooks are integer atomicMin: the minimum of a set, the same whatever the
// order.  At the fixpoint every tree is a star whose root is its component's
// lowest core index.
//
// k_dbscan_init    core words (one ballot a word), f = fn = gf = identity.
// k_dbscan_hook    one wave a core row: the row's minimum, the two hooks.
// k_dbscan_sync    f = fn, gf = fn[fn], and the round's number where f changed.
// k_dbscan_ids     one workgroup: root words, their exclusive popcount scan.
// k_dbscan_label   one wave a row: the rank of a core row's root, or of the
//                  lowest root among a non-core row's core neighbours.
//
// Workgroups talk to each other at kernel boundaries only: plain launches on
// one stream, nothing polled.  rmsf_cluster_dbscan_host is the same definition
// on the host, the reference of the CPU tests.
#include <climits>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "rmsf_host.h"

namespace {

constexpr int kWave = 64;
constexpr int kInitBlock = 256;
constexpr int kRowWaves = 4;       // rows a workgroup of k_dbscan_hook and k_dbscan_label
constexpr int kRowUnroll = 8;      // gathers a wave has in flight
constexpr int kIdsBlock = 1024;    // the one workgroup of k_dbscan_ids
constexpr int kIdsWaves = kIdsBlock / kWave;
constexpr int kRoundBatch = 4;     // rounds enqueued between two reads of the state

// the int32 state words at the head of the workspace
enum { kStLastChanged = 0, kStClusters = 1, kStWords = 16 };

__host__ __device__ inline int64_t row_words(int64_t n) { return n < 1 ? 0 : (n + 63) / 64; }
inline size_t up8(size_t b) { return (b + 7) & ~size_t(7); }

// state | f | fn | gf | root words | word offsets
struct Workspace {
  size_t f, fn, gf, roots, wordoff, bytes;
};
inline Workspace workspace(int64_t n) {
  const size_t nw = (size_t)row_words(n);
  Workspace w;
  w.f = kStWords * sizeof(int32_t);
  w.fn = w.f + up8(4 * (size_t)n);
  w.gf = w.fn + up8(4 * (size_t)n);
  w.roots = w.gf + up8(4 * (size_t)n);
  w.wordoff = w.roots + 8 * nw;
  w.bytes = w.wordoff + up8(4 * nw);
  return w;
}

__device__ inline uint64_t read_lane64(uint64_t x, int k) {  // k is wave-uniform
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)x, k);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), k);
  return ((uint64_t)hi << 32) | lo;
}

// min over the set bits j of (row & core) of val[j]; INT32_MAX for none.  A
// wave reads 64 words of the row at a time (512 bytes), the words that have a
// core neighbour are walked kRowUnroll at a time -- the others are skipped by a
// branch the whole wave takes -- and lane l reads val[64 w + l] where bit l is
// set, val[0] (and ignores it) where it is not: loads without a branch, so
// that kRowUnroll of them are in flight before the first is waited for.
// Bits at or past n are never set in core, so nothing past val[n - 1] is read.
__device__ inline int32_t row_min(const uint64_t *__restrict__ row, const uint64_t *__restrict__ core,
                                  int64_t n_words, const int32_t *__restrict__ val, int lane) {
  int32_t best = INT32_MAX;
  for (int64_t w0 = 0; w0 < n_words; w0 += kWave) {
    const int64_t w = w0 + lane;
    const uint64_t x = w < n_words ? (row[w] & core[w]) : 0;
    uint64_t nz = __ballot(x != 0);
    while (nz) {
      int32_t v[kRowUnroll];
      bool bit[kRowUnroll];
#pragma unroll
      for (int u = 0; u < kRowUnroll; ++u) {
        const int k = __builtin_amdgcn_readfirstlane(nz ? __builtin_ctzll(nz) : 0);
        const uint64_t word = nz ? read_lane64(x, k) : 0;  // (past the last non-zero word: no bit, nothing kept)
        nz &= nz - 1;
        bit[u] = (word >> lane) & 1;
        v[u] = val[bit[u] ? 64 * (w0 + k) + lane : 0];
      }
#pragma unroll
      for (int u = 0; u < kRowUnroll; ++u) {
        const int32_t c = bit[u] ? v[u] : INT32_MAX;
        best = c < best ? c : best;
      }
    }
  }
  for (int d = kWave / 2; d > 0; d >>= 1) {
    const int32_t o = __shfl_xor(best, d);
    best = o < best ? o : best;
  }
  return best;
}

__global__ __launch_bounds__(kInitBlock) void k_dbscan_init(const int32_t *__restrict__ count, int64_t n,
                                                            int64_t min_samples, uint64_t *__restrict__ core,
                                                            int32_t *__restrict__ f, int32_t *__restrict__ fn,
                                                            int32_t *__restrict__ gf, int32_t *__restrict__ state) {
  const int64_t i = (int64_t)blockIdx.x * kInitBlock + threadIdx.x;
  const uint64_t word = __ballot(i < n && count[i] >= min_samples);
  if ((threadIdx.x & (kWave - 1)) == 0 && i < n) core[i >> 6] = word;
  if (i < n) f[i] = fn[i] = gf[i] = (int32_t)i;
  if (i < kStWords) state[i] = 0;
}

// Round `round` (1, 2, ...) runs if round - 1 changed f; state[kStLastChanged]
// is the last round that did (0 before the first).
__global__ __launch_bounds__(kRowWaves *kWave) void k_dbscan_hook(const uint64_t *__restrict__ adj, int64_t n,
                                                                  int64_t ldw, const uint64_t *__restrict__ core,
                                                                  const int32_t *__restrict__ f,
                                                                  const int32_t *__restrict__ gf, int32_t *fn,
                                                                  const int32_t *__restrict__ state, int32_t round) {
  if (state[kStLastChanged] < round - 1) return;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t i = (int64_t)blockIdx.x * kRowWaves + wave;
  if (i >= n || !((core[i >> 6] >> (i & 63)) & 1)) return;  // (a whole wave; nothing is shared between waves)
  const int32_t m = row_min(adj + i * ldw, core, row_words(n), gf, lane);
  if (lane == 0) {
    const int32_t p = f[i];
    if (m < gf[i]) atomicMin(&fn[p], m);
    if (m < p) atomicMin(&fn[i], m);
  }
}

__global__ __launch_bounds__(kInitBlock) void k_dbscan_sync(int64_t n, int32_t *__restrict__ f,
                                                            const int32_t *__restrict__ fn,
                                                            int32_t *__restrict__ gf, int32_t *state, int32_t round) {
  if (state[kStLastChanged] < round - 1) return;
  const int64_t i = (int64_t)blockIdx.x * kInitBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t v = fn[i];
  gf[i] = fn[v];
  if (v != f[i]) {
    f[i] = v;
    atomicMax(&state[kStLastChanged], round);
  }
}

// The roots are the core rows with f[i] == i.  One workgroup: a pass makes
// kIdsBlock root words (wave v the words base + 64 v ..., one ballot each, lane
// k keeping the k-th) and scans their popcounts; the carry crosses the passes.
__global__ __launch_bounds__(kIdsBlock) void k_dbscan_ids(const uint64_t *__restrict__ core, int64_t n,
                                                          const int32_t *__restrict__ f,
                                                          uint64_t *__restrict__ roots,
                                                          int32_t *__restrict__ wordoff, int32_t *__restrict__ state) {
  __shared__ int s_sum[kIdsWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t n_words = row_words(n);
  int carry = 0;
  for (int64_t base = 0; base < n_words; base += kIdsBlock) {
    const int64_t w = base + tid;
    uint64_t mine = 0;
    for (int k = 0; k < kWave; ++k) {
      const int64_t wk = base + wave * kWave + k;  // wave-uniform
      if (wk >= n_words) break;
      const int64_t i = 64 * wk + lane;
      const uint64_t word = __ballot(i < n && f[i] == (int32_t)i) & core[wk];
      if (lane == k) mine = word;
    }
    if (w < n_words) roots[w] = mine;
    const int pc = __popcll(mine);
    int incl = pc;
    for (int d = 1; d < kWave; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    if (lane == kWave - 1) s_sum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int v = 0; v < kIdsWaves; ++v) {
      if (v < wave) before += s_sum[v];
      total += s_sum[v];
    }
    if (w < n_words) wordoff[w] = carry + before + incl - pc;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) state[kStClusters] = carry;
}

// A cluster's id is its root's rank among the roots, so the lowest id among a
// border row's core neighbours is the rank of the lowest root among them.
__global__ __launch_bounds__(kRowWaves *kWave) void k_dbscan_label(const uint64_t *__restrict__ adj, int64_t n,
                                                                   int64_t ldw, const uint64_t *__restrict__ core,
                                                                   const int32_t *__restrict__ f,
                                                                   const uint64_t *__restrict__ roots,
                                                                   const int32_t *__restrict__ wordoff,
                                                                   int32_t *__restrict__ label) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t i = (int64_t)blockIdx.x * kRowWaves + wave;
  if (i >= n) return;  // (a whole wave)
  int32_t r;
  if ((core[i >> 6] >> (i & 63)) & 1)
    r = f[i];
  else
    r = row_min(adj + i * ldw, core, row_words(n), f, lane);
  if (lane == 0)
    label[i] = r == INT32_MAX ? -1
                              : wordoff[r >> 6] + __popcll(roots[r >> 6] & ((uint64_t(1) << (r & 63)) - 1));
}

inline int hip_fail(const char *what, hipError_t e) {
  return fail(RMSF_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace

extern "C" {

RMSF_EXPORT size_t rmsf_cluster_dbscan_workspace_bytes(int64_t n) {
  if (n < 1 || n > INT32_MAX) return 0;
  return workspace(n).bytes;
}

RMSF_EXPORT int rmsf_cluster_dbscan(const uint64_t *d_adj, int64_t n, int64_t ldw, const int32_t *d_count,
                                    int64_t min_samples, int32_t *d_label, uint64_t *d_core, int32_t *h_n_clusters,
                                    int32_t *h_n_rounds, void *d_work, size_t work_bytes, void *stream) {
  if (!d_adj || !d_count || !d_label || !d_core || !h_n_clusters || !h_n_rounds || n < 1 || n > INT32_MAX ||
      ldw < row_words(n) || min_samples < 1)
    return fail(RMSF_EINVAL, "rmsf_cluster_dbscan: bad arguments");
  const Workspace ws = workspace(n);
  if (!d_work || work_bytes < ws.bytes) return fail(RMSF_ENOMEM, "rmsf_cluster_dbscan: workspace too small");
  char *base = static_cast<char *>(d_work);
  int32_t *state = reinterpret_cast<int32_t *>(base);
  int32_t *f = reinterpret_cast<int32_t *>(base + ws.f);
  int32_t *fn = reinterpret_cast<int32_t *>(base + ws.fn);
  int32_t *gf = reinterpret_cast<int32_t *>(base + ws.gf);
  uint64_t *roots = reinterpret_cast<uint64_t *>(base + ws.roots);
  int32_t *wordoff = reinterpret_cast<int32_t *>(base + ws.wordoff);
  const dim3 flat((unsigned)((n + kInitBlock - 1) / kInitBlock)), rows((unsigned)((n + kRowWaves - 1) / kRowWaves));
  hipLaunchKernelGGL(k_dbscan_init, flat, dim3(kInitBlock), 0, S(stream), d_count, n, min_samples, d_core, f, fn, gf,
                     state);
  if (int rc = after_launch("k_dbscan_init")) return rc;
  // After t rounds f[i] is at most what plain min-propagation has after t, and
  // that settles within the diameter, below n: the cap only bounds the loop.
  const int64_t cap = n + 1;
  int32_t seen[2] = {0, 0};  // kStLastChanged, kStClusters
  bool done = false;
  for (int64_t enqueued = 0; enqueued < cap && !done;) {
    const int64_t batch = cap - enqueued < kRoundBatch ? cap - enqueued : kRoundBatch;
    for (int64_t b = 1; b <= batch; ++b) {
      const int32_t round = (int32_t)(enqueued + b);
      hipLaunchKernelGGL(k_dbscan_hook, rows, dim3(kRowWaves * kWave), 0, S(stream), d_adj, n, ldw, d_core, f, gf, fn,
                         state, round);
      hipLaunchKernelGGL(k_dbscan_sync, flat, dim3(kInitBlock), 0, S(stream), n, f, fn, gf, state, round);
    }
    if (int rc = after_launch("k_dbscan_hook / k_dbscan_sync")) return rc;
    enqueued += batch;
    // the one host synchronisation of a batch: the last round that changed anything
    hipError_t e = hipMemcpyAsync(seen, state, sizeof(int32_t), hipMemcpyDeviceToHost, S(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(S(stream));
    if (e != hipSuccess) return hip_fail("rmsf_cluster_dbscan: reading the state back", e);
    done = seen[kStLastChanged] < enqueued;  // round seen + 1 ran and changed nothing
  }
  if (!done) return fail(RMSF_EHIP, "rmsf_cluster_dbscan: the components did not settle in n + 1 rounds");
  hipLaunchKernelGGL(k_dbscan_ids, dim3(1), dim3(kIdsBlock), 0, S(stream), d_core, n, f, roots, wordoff, state);
  hipLaunchKernelGGL(k_dbscan_label, rows, dim3(kRowWaves * kWave), 0, S(stream), d_adj, n, ldw, d_core, f, roots,
                     wordoff, d_label);
  if (int rc = after_launch("k_dbscan_ids / k_dbscan_label")) return rc;
  hipError_t e = hipMemcpyAsync(seen, state, sizeof seen, hipMemcpyDeviceToHost, S(stream));
  if (e == hipSuccess) e = hipStreamSynchronize(S(stream));
  if (e != hipSuccess) return hip_fail("rmsf_cluster_dbscan: reading the cluster count back", e);
  *h_n_clusters = seen[kStClusters];
  *h_n_rounds = seen[kStLastChanged] + 1;
  return RMSF_OK;
}

RMSF_EXPORT int rmsf_cluster_dbscan_host(const double *h_m, int64_t n, int64_t ld, double cutoff, int64_t min_samples,
                                         int32_t *h_label, uint64_t *h_core, int32_t *h_n_clusters) {
  if (!h_m || !h_label || !h_core || !h_n_clusters || n < 1 || n > INT32_MAX || ld < n || min_samples < 1 ||
      !(cutoff >= 0.0))
    return fail(RMSF_EINVAL, "rmsf_cluster_dbscan_host: bad arguments");
  const int64_t nw = row_words(n);
  std::vector<uint64_t> adj;
  std::vector<int32_t> stack;
  try {
    adj.assign((size_t)(n * nw), 0);
    stack.reserve((size_t)n);
  } catch (const std::bad_alloc &) {
    return fail(RMSF_ENOMEM, "rmsf_cluster_dbscan_host: out of host memory for the neighbour bits");
  }
  for (int64_t w = 0; w < nw; ++w) h_core[w] = 0;
  for (int64_t i = 0; i < n; ++i) {
    int32_t count = 0;
    for (int64_t j = 0; j < n; ++j)
      if (j == i || h_m[i * ld + j] <= cutoff) {
        adj[(size_t)(i * nw + (j >> 6))] |= uint64_t(1) << (j & 63);
        ++count;
      }
    if (count >= min_samples) h_core[i >> 6] |= uint64_t(1) << (i & 63);
    h_label[i] = -1;
  }
  const auto is_core = [&](int64_t i) { return (h_core[i >> 6] >> (i & 63)) & 1; };
  // core rows in index order: an unlabelled one is the lowest of a new cluster
  int32_t k = 0;
  for (int64_t s = 0; s < n; ++s) {
    if (!is_core(s) || h_label[s] >= 0) continue;
    h_label[s] = k;
    stack.push_back((int32_t)s);
    while (!stack.empty()) {
      const int64_t i = stack.back();
      stack.pop_back();
      for (int64_t w = 0; w < nw; ++w)
        for (uint64_t x = adj[(size_t)(i * nw + w)] & h_core[w]; x; x &= x - 1) {
          const int64_t j = 64 * w + __builtin_ctzll(x);
          if (h_label[j] < 0) {
            h_label[j] = k;
            stack.push_back((int32_t)j);
          }
        }
    }
    ++k;
  }
  // border rows: the lowest id among the core neighbours' clusters
  for (int64_t i = 0; i < n; ++i) {
    if (is_core(i)) continue;
    int32_t best = -1;
    for (int64_t w = 0; w < nw; ++w)
      for (uint64_t x = adj[(size_t)(i * nw + w)] & h_core[w]; x; x &= x - 1) {
        const int32_t l = h_label[64 * w + __builtin_ctzll(x)];
        if (best < 0 || l < best) best = l;
      }
    h_label[i] = best;
  }
  *h_n_clusters = k;
  return RMSF_OK;
}

}  // extern "C"
