// clustering.hip -- GROMOS clustering (Daura et al. 1999) of a symmetric distance
// matrix, all integers after one threshold ("Clustering").
//
//   adj(i, j) = (d[i, j] <= cutoff) for i != j, adj(i, i) = 1; a NaN is never a
//   neighbour.  count[i] = the set bits of row i.  While a frame is active: the
//   centre is the active frame of the largest count (the lowest index among
//   equals), its members adj(centre, .) & active get the next cluster id and
//   leave, and every frame still active loses its neighbours among them.
//
// k_adj_pack        f64 matrix -> bit rows (one ballot a word) and the counts.
// k_adj_count       the counts of bit rows written elsewhere (csrc/pairwise.hip).
// k_gromos_init     the working copy of the counts, the active words, the state.
// k_gromos_pick     one workgroup: argmax, member words, labels, member list.
// k_gromos_decrement  one workgroup a column word: walks the members' rows.
//
// Workgroups talk to each other at kernel boundaries only: plain launches on one
// stream, no atomics, nothing polled.  rmsf_cluster_gromos_host is the same
// definition on the host, the reference of the CPU tests.
#include <climits>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "rmsf_host.h"

namespace {

constexpr int kWave = 64;
// waves a row of the f64 matrix, and the loads each has in flight (tools/ab_cluster_pack.py times other values)
#ifndef RMSF_PACK_WAVES
#define RMSF_PACK_WAVES 4
#endif
#ifndef RMSF_PACK_UNROLL
#define RMSF_PACK_UNROLL 4
#endif
constexpr int kPackWaves = RMSF_PACK_WAVES;
constexpr int kPackUnroll = RMSF_PACK_UNROLL;
constexpr int kCountWaves = 4;    // rows a workgroup of k_adj_count
constexpr int kPickBlock = 1024;  // the one workgroup of k_gromos_pick
constexpr int kPickWaves = kPickBlock / kWave;
constexpr int kDecWaves = 8;      // waves sharing one column word's member list
constexpr int kInitBlock = 256;
constexpr int kBatch = 32;        // clusters enqueued between two reads of the state

// the int32 state words at the head of the workspace
enum { kStClusters = 0, kStFinished = 1, kStMembers = 2, kStRemaining = 3, kStWords = 16 };

__host__ __device__ inline int64_t adj_words(int64_t n) { return n < 1 ? 0 : (n + 63) / 64; }
inline size_t up8(size_t b) { return (b + 7) & ~size_t(7); }

// state | count (working copy) | active | members | word offsets | member list
struct Workspace {
  size_t count, active, members, wordoff, list, bytes;
};
inline Workspace workspace(int64_t n) {
  const size_t nw = (size_t)adj_words(n);
  Workspace w;
  w.count = kStWords * sizeof(int32_t);
  w.active = w.count + up8(4 * (size_t)n);
  w.members = w.active + 8 * nw;
  w.wordoff = w.members + 8 * nw;
  w.list = w.wordoff + up8(4 * nw);
  w.bytes = w.list + up8(4 * (size_t)n);
  return w;
}

// ---- pack --------------------------------------------------------------------
// One workgroup a row; a wave reads 64 consecutive f64 (512 bytes) and its
// ballot is that row's word.  Full words go kPackUnroll at a time so that a wave
// has that many loads in flight; the row's count is the sum of the words' popcounts.
__global__ __launch_bounds__(kPackWaves *kWave) void k_adj_pack(const double *__restrict__ m, int64_t n, int64_t ld,
                                                                 double cutoff, uint64_t *__restrict__ adj,
                                                                 int64_t ldw, int32_t *__restrict__ count) {
  __shared__ int s_cnt[kPackWaves];
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t n_full = n >> 6, n_words = adj_words(n);
  const double *__restrict__ r = m + row * ld;
  uint64_t *__restrict__ a = adj + row * ldw;
  int cnt = 0;
  int64_t w = wave;
  for (; w + (kPackUnroll - 1) * kPackWaves < n_full; w += kPackUnroll * kPackWaves) {
    double v[kPackUnroll];
#pragma unroll
    for (int u = 0; u < kPackUnroll; ++u) v[u] = r[64 * (w + u * kPackWaves) + lane];
#pragma unroll
    for (int u = 0; u < kPackUnroll; ++u) {
      const int64_t col = 64 * (w + u * kPackWaves) + lane;
      const uint64_t word = __ballot(col == row || v[u] <= cutoff);
      if (lane == 0) a[w + u * kPackWaves] = word;
      cnt += __popcll(word);
    }
  }
  for (; w < n_words; w += kPackWaves) {
    const int64_t col = 64 * w + lane;
    bool bit = false;
    if (col < n) bit = col == row || r[col] <= cutoff;
    const uint64_t word = __ballot(bit);
    if (lane == 0) a[w] = word;
    cnt += __popcll(word);
  }
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int k = 0; k < kPackWaves; ++k) sum += s_cnt[k];
    count[row] = sum;
  }
}

// ---- count ---------------------------------------------------------------------
// The counts of bit rows that were not packed here (rmsf_pairwise_adjacency
// writes them a tile at a time, each row from many workgroups).  One wave a
// row: lane l adds the popcounts of words l, l + 64, ... in order, the lanes
// are added by a halving tree of shuffles.  The bits are read once.
__global__ __launch_bounds__(kCountWaves *kWave) void k_adj_count(const uint64_t *__restrict__ adj, int64_t n,
                                                                  int64_t ldw, int32_t *__restrict__ count) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t row = (int64_t)blockIdx.x * kCountWaves + wave;
  if (row >= n) return;  // (a whole wave; nothing below is shared between waves)
  const int64_t n_words = adj_words(n);
  const uint64_t *__restrict__ a = adj + row * ldw;
  int cnt = 0;
#pragma unroll 4
  for (int64_t w = lane; w < n_words; w += kWave) cnt += __popcll(a[w]);
  for (int d = kWave / 2; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
  if (lane == 0) count[row] = cnt;
}

// ---- the loop ------------------------------------------------------------------
__global__ __launch_bounds__(kInitBlock) void k_gromos_init(const int32_t *__restrict__ count, int64_t n,
                                                            int32_t *__restrict__ work_count,
                                                            uint64_t *__restrict__ active,
                                                            int32_t *__restrict__ state) {
  const int64_t i = (int64_t)blockIdx.x * kInitBlock + threadIdx.x;
  if (i < n) work_count[i] = count[i];
  if (i < adj_words(n)) {
    const int64_t left = n - 64 * i;
    active[i] = left >= 64 ? ~uint64_t(0) : (uint64_t(1) << left) - 1;
  }
  if (i < kStWords) state[i] = i == kStRemaining ? (int32_t)n : 0;
}

// Picks cluster k = state[kStClusters] and assigns its members; one workgroup.
// The key of a frame is (count << 32) | (INT32_MAX - index): the largest key is
// the largest count and, among equals, the lowest index.
__global__ __launch_bounds__(kPickBlock) void k_gromos_pick(const uint64_t *__restrict__ adj, int64_t n, int64_t ldw,
                                                            const int32_t *__restrict__ count, uint64_t *active,
                                                            uint64_t *members, int32_t *wordoff,
                                                            int32_t *__restrict__ list, int32_t *state,
                                                            int32_t *__restrict__ label, int32_t *__restrict__ centre,
                                                            int32_t *__restrict__ size) {
  __shared__ long long s_key[kPickWaves];
  __shared__ int s_sum[kPickWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int k = state[kStClusters], remaining = state[kStRemaining];
  if (state[kStFinished]) return;
  const int64_t n_words = adj_words(n);

  long long best = -1;
  for (int64_t i = tid; i < n; i += kPickBlock)
    if ((active[i >> 6] >> (i & 63)) & 1) {
      const long long key = ((long long)count[i] << 32) | (long long)(INT32_MAX - (int32_t)i);
      best = key > best ? key : best;
    }
  for (int d = kWave / 2; d > 0; d >>= 1) {
    const long long o = __shfl_xor(best, d);
    best = o > best ? o : best;
  }
  if (lane == 0) s_key[wave] = best;
  __syncthreads();  // also: every thread has read the state and the active words
  for (int v = 0; v < kPickWaves; ++v) best = s_key[v] > best ? s_key[v] : best;
  if (best < 0) {  // no frame is active
    if (tid == 0) {
      state[kStFinished] = 1;
      state[kStMembers] = 0;
    }
    return;
  }
  const int64_t c = INT32_MAX - (int32_t)(best & 0xffffffffLL);
  const bool singles = (best >> 32) == 1;  // every active frame is alone: all of them, in index order

  // member words, and each word's offset in the member list (exclusive scan)
  int carry = 0;
  for (int64_t base = 0; base < n_words; base += kPickBlock) {
    const int64_t w = base + tid;
    uint64_t mw = 0;
    if (w < n_words) {
      const uint64_t a = active[w];
      mw = singles ? a : (adj[c * ldw + w] & a);
      members[w] = mw;
      active[w] = a & ~mw;
    }
    const int pc = __popcll(mw);
    int incl = pc;
    for (int d = 1; d < kWave; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    if (lane == kWave - 1) s_sum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int v = 0; v < kPickWaves; ++v) {
      if (v < wave) before += s_sum[v];
      total += s_sum[v];
    }
    if (w < n_words) wordoff[w] = carry + before + incl - pc;
    carry += total;
    __syncthreads();
  }

  // labels and the member list, one lane a frame
  for (int64_t i = tid; i < n; i += kPickBlock) {
    const uint64_t mw = members[i >> 6];
    const int b = (int)(i & 63);
    if ((mw >> b) & 1) {
      const int pos = wordoff[i >> 6] + __popcll(mw & ((uint64_t(1) << b) - 1));
      if (singles) {
        label[i] = k + pos;
        centre[k + pos] = (int32_t)i;
        size[k + pos] = 1;
      } else {
        label[i] = k;
        list[pos] = (int32_t)i;
      }
    }
  }
  if (tid == 0) {
    if (!singles) {
      centre[k] = (int32_t)c;
      size[k] = carry;
    }
    state[kStClusters] = singles ? k + carry : k + 1;
    state[kStMembers] = singles ? 0 : carry;
    state[kStRemaining] = remaining - carry;
    if (singles || remaining == carry) state[kStFinished] = 1;
  }
}

// count[i] -= |adj(i, .) & members| for the active frames i of column word
// blockIdx.x.  adj is symmetric, so adj(i, j) of member j is bit i of row j:
// one 8-byte word a member and wave, at a wave-uniform address.  The waves of
// the workgroup split the member list and their sums meet in LDS.
__global__ __launch_bounds__(kDecWaves *kWave) void k_gromos_decrement(const uint64_t *__restrict__ adj, int64_t ldw,
                                                                       int32_t *__restrict__ count,
                                                                       const uint64_t *__restrict__ active,
                                                                       const int32_t *__restrict__ list,
                                                                       const int32_t *__restrict__ state) {
  __shared__ int s_acc[kDecWaves][kWave];
  if (state[kStFinished]) return;
  const int n_members = state[kStMembers];
  const int64_t w = blockIdx.x;
  const uint64_t a = active[w];
  if (a == 0) return;  // nobody left in these 64 columns (the whole workgroup returns)
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int per = (n_members + kDecWaves - 1) / kDecWaves;
  const int j0 = wave * per, j1 = min(n_members, j0 + per);
  const uint64_t *__restrict__ col = adj + w;
  int acc = 0;
#pragma unroll 8
  for (int j = j0; j < j1; ++j) {
    const uint64_t word = col[(int64_t)list[j] * ldw];
    acc += (int)((word >> lane) & 1);
  }
  s_acc[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && ((a >> lane) & 1)) {
    int sum = 0;
    for (int v = 0; v < kDecWaves; ++v) sum += s_acc[v][lane];
    count[64 * w + lane] -= sum;
  }
}

inline int hip_fail(const char *what, hipError_t e) {
  return fail(RMSF_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace

extern "C" {

RMSF_EXPORT int64_t rmsf_adjacency_words(int64_t n) { return adj_words(n); }

RMSF_EXPORT int rmsf_adjacency_pack(const double *d_m, int64_t n, int64_t ld, double cutoff, uint64_t *d_adj,
                                    int64_t ldw, int32_t *d_count, void *stream) {
  if (!d_m || !d_adj || !d_count || n < 1 || n > INT32_MAX || ld < n || ldw < adj_words(n) || !(cutoff >= 0.0))
    return fail(RMSF_EINVAL, "rmsf_adjacency_pack: bad arguments");
  hipLaunchKernelGGL(k_adj_pack, dim3((unsigned)n), dim3(kPackWaves * kWave), 0, S(stream), d_m, n, ld, cutoff, d_adj,
                     ldw, d_count);
  return after_launch("k_adj_pack");
}

RMSF_EXPORT int rmsf_adjacency_count(const uint64_t *d_adj, int64_t n, int64_t ldw, int32_t *d_count, void *stream) {
  if (!d_adj || !d_count || n < 1 || n > INT32_MAX || ldw < adj_words(n))
    return fail(RMSF_EINVAL, "rmsf_adjacency_count: bad arguments");
  hipLaunchKernelGGL(k_adj_count, dim3((unsigned)((n + kCountWaves - 1) / kCountWaves)), dim3(kCountWaves * kWave), 0,
                     S(stream), d_adj, n, ldw, d_count);
  return after_launch("k_adj_count");
}

RMSF_EXPORT size_t rmsf_cluster_gromos_workspace_bytes(int64_t n) {
  if (n < 1 || n > INT32_MAX) return 0;
  return workspace(n).bytes;
}

RMSF_EXPORT int rmsf_cluster_gromos(const uint64_t *d_adj, int64_t n, int64_t ldw, const int32_t *d_count,
                                    int32_t *d_label, int32_t *d_centre, int32_t *d_size, int32_t *h_n_clusters,
                                    void *d_work, size_t work_bytes, void *stream) {
  if (!d_adj || !d_count || !d_label || !d_centre || !d_size || !h_n_clusters || n < 1 || n > INT32_MAX ||
      ldw < adj_words(n))
    return fail(RMSF_EINVAL, "rmsf_cluster_gromos: bad arguments");
  const Workspace ws = workspace(n);
  if (!d_work || work_bytes < ws.bytes) return fail(RMSF_ENOMEM, "rmsf_cluster_gromos: workspace too small");
  char *base = static_cast<char *>(d_work);
  int32_t *state = reinterpret_cast<int32_t *>(base);
  int32_t *count = reinterpret_cast<int32_t *>(base + ws.count);
  uint64_t *active = reinterpret_cast<uint64_t *>(base + ws.active);
  uint64_t *members = reinterpret_cast<uint64_t *>(base + ws.members);
  int32_t *wordoff = reinterpret_cast<int32_t *>(base + ws.wordoff);
  int32_t *list = reinterpret_cast<int32_t *>(base + ws.list);
  const int64_t n_words = adj_words(n);
  hipLaunchKernelGGL(k_gromos_init, dim3((unsigned)((n + kInitBlock - 1) / kInitBlock)), dim3(kInitBlock), 0,
                     S(stream), d_count, n, count, active, state);
  if (int rc = after_launch("k_gromos_init")) return rc;
  int32_t seen[2] = {0, 0};  // kStClusters, kStFinished
  for (int64_t enqueued = 0; enqueued < n && !seen[kStFinished];) {
    const int64_t batch = n - enqueued < kBatch ? n - enqueued : kBatch;
    for (int64_t b = 0; b < batch; ++b) {
      hipLaunchKernelGGL(k_gromos_pick, dim3(1), dim3(kPickBlock), 0, S(stream), d_adj, n, ldw, count, active,
                         members, wordoff, list, state, d_label, d_centre, d_size);
      hipLaunchKernelGGL(k_gromos_decrement, dim3((unsigned)n_words), dim3(kDecWaves * kWave), 0, S(stream), d_adj,
                         ldw, count, active, list, state);
    }
    if (int rc = after_launch("k_gromos_pick / k_gromos_decrement")) return rc;
    enqueued += batch;
    // the one host synchronisation of a batch: the cluster count and the "finished" word
    hipError_t e = hipMemcpyAsync(seen, state, sizeof seen, hipMemcpyDeviceToHost, S(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(S(stream));
    if (e != hipSuccess) return hip_fail("rmsf_cluster_gromos: reading the state back", e);
  }
  *h_n_clusters = seen[kStClusters];
  return RMSF_OK;
}

RMSF_EXPORT int rmsf_cluster_gromos_host(const double *h_m, int64_t n, int64_t ld, double cutoff, int32_t *h_label,
                                         int32_t *h_centre, int32_t *h_size, int32_t *h_n_clusters) {
  if (!h_m || !h_label || !h_centre || !h_size || !h_n_clusters || n < 1 || n > INT32_MAX || ld < n ||
      !(cutoff >= 0.0))
    return fail(RMSF_EINVAL, "rmsf_cluster_gromos_host: bad arguments");
  const int64_t nw = adj_words(n);
  std::vector<uint64_t> adj, active, members;
  std::vector<int32_t> count;
  try {
    adj.assign((size_t)(n * nw), 0);
    active.assign((size_t)nw, 0);
    members.assign((size_t)nw, 0);
    count.assign((size_t)n, 0);
  } catch (const std::bad_alloc &) {
    return fail(RMSF_ENOMEM, "rmsf_cluster_gromos_host: out of host memory for the neighbour bits");
  }
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t j = 0; j < n; ++j)
      if (j == i || h_m[i * ld + j] <= cutoff) {
        adj[(size_t)(i * nw + (j >> 6))] |= uint64_t(1) << (j & 63);
        ++count[(size_t)i];
      }
    active[(size_t)(i >> 6)] |= uint64_t(1) << (i & 63);
  }
  const auto is_active = [&](int64_t i) { return (active[(size_t)(i >> 6)] >> (i & 63)) & 1; };
  int32_t k = 0;
  for (int64_t remaining = n; remaining > 0; ++k) {
    int64_t c = -1;
    for (int64_t i = 0; i < n; ++i)
      if (is_active(i) && (c < 0 || count[(size_t)i] > count[(size_t)c])) c = i;  // strict: the lowest index wins
    int32_t n_members = 0;
    for (int64_t w = 0; w < nw; ++w) {
      const uint64_t mw = adj[(size_t)(c * nw + w)] & active[(size_t)w];
      members[(size_t)w] = mw;
      active[(size_t)w] &= ~mw;
      n_members += __builtin_popcountll(mw);
    }
    for (int64_t i = 0; i < n; ++i) {
      if ((members[(size_t)(i >> 6)] >> (i & 63)) & 1) h_label[i] = k;
      if (!is_active(i)) continue;
      int32_t lost = 0;
      for (int64_t w = 0; w < nw; ++w) lost += __builtin_popcountll(adj[(size_t)(i * nw + w)] & members[(size_t)w]);
      count[(size_t)i] -= lost;
    }
    h_centre[k] = (int32_t)c;
    h_size[k] = n_members;
    remaining -= n_members;
  }
  *h_n_clusters = k;
  return RMSF_OK;
}

}  // extern "C"
