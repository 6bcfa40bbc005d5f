// hg_cluster_setcover.hip -- greedy set-cover clustering of sketches at an ANI threshold (an extension like
// hg_cluster_greedy.hip: the scheme MMseqs2 and Linclust cluster with by default).  A hit record COUNTS iff
// ani >= ani_th (the float comparison of hg_dist_dev: NaN never counts) and ref_idx != qry_idx; a counting record is an
// edge between its two indices, in either orientation.  U is the set of undecided nodes, at first all of them.  While U
// is not empty:
//   1. deg(v) = the number of counting RECORDS with v at one end and the other end in U, for every v in U (a pair given
//      twice counts twice; a list that holds every pair the same number of times resolves like the list with each pair once);
//   2. v* = the node of U with the largest deg, ties to the smallest index: a REPRESENTATIVE;
//   3. every u in U with a counting record {v*, u} becomes a MEMBER of v*, ani[u] = the highest ANI among those records;
//   4. v* and its new members leave U.
// A node of degree 0 is thereby its own representative; a member covers nobody and never changes representative.
// Representatives are pairwise below the threshold, every member is at or above it with its own representative.
//
// The sequential rule is resolved in ROUNDS over the whole hit list.  A record is LIVE while both its ends are undecided.
// One round:
//   * count  : one lane per live record: integer atomic add into deg[] of both ends;
//   * m1     : one lane per live record: key(v) = deg(v) << 32 | (0xFFFFFFFF - v) of each end, 64-bit atomic max into the
//              other end's m1 word -- with its own key, m1(v) = the largest key among v and its live neighbours;
//   * m2     : the same with max(m1, key) of each end into the other end's m2 word: the largest key within two live hops;
//   * select : one lane per node: undecided and neither m1 nor m2 above its own key -> representative; deg, m1 and m2 of
//              the node are cleared for the next round;
//   * cover  : one lane per record {representative, undecided}: atomic max of (ani key << 32 | 0xFFFFFFFF - representative)
//              into the undecided end's best word;
//   * settle : one lane per node: undecided with a best word -> member; the nodes that stay undecided are counted into a
//              device word.
// Then rep / ani from status and best, and the dense ids with hg_cluster.hip's finishing launches (every tree has depth 1).
// Every kernel runs to its end on its own: no cooperative launch, no grid-wide barrier, no workgroup waits for another
// one's store.  The host queues a few rounds, reads the undecided count back (hg_publish_words) and stops at 0; the
// rounds queued behind the one that reached 0 see that word and return at once.  Six launches per round over the list.
//
// Why it equals the sequential rule.  Degrees only fall.  The key of u, and the set u would cover, change only when a
// node within two live hops of u is chosen (the chosen node or one of its new members is then a neighbour of u).  If u is
// the strict maximum of its live 2-hop neighbourhood now (keys of undecided nodes differ in their index part), no node of
// that neighbourhood can be the global maximum before u is chosen: its key would have to exceed u's unchanged one while
// its own can only fall.  So the sequential walk chooses u, with exactly the cover set u has now.  Nodes selected in one
// round are more than two hops apart: they touch neither each other's keys nor each other's neighbours, and no undecided
// node has records to two of them.  The global maximum is selected in every round, so every round makes progress.
// Keys travel through LIVE records only: two candidates whose only common neighbour is already a member do not conflict
// (going through decided nodes would not change the result, only cost rounds).
// Status moves undecided -> representative inside select and undecided -> member inside settle, never back, and cover
// -- which reads status of both ends -- writes none: a duplicate record with a higher ANI still finds its end undecided.
// best[] is an atomic max over a total order of (ani, index), deg[] an integer sum, m1 / m2 atomic maxima: neither the
// order of the hits, their orientation, the rounds per readback nor the scheduling show in the result.
// The worst case is a path 0 - 1 - 2 - ...: one representative per round (every third node), about n / 3 rounds.  It is
// accepted, as n / 2 is for the greedy resolution: dense groups -- what a dereplication sees -- resolve in a few rounds.
//
// Cross-workgroup traffic inside one launch is agent-scope relaxed atomics only (the adds of count, the maxima of m1, m2
// and cover, the counter of settle).  Everything else is read behind a launch boundary.
//
// The rule is global -- the first representative is the best-covering node of the whole graph -- so hg_cluster_setcover_dev
// cannot resolve a row block before it has seen them all: it APPENDS the hits of every row block of the symmetric
// comparison to one list (12 bytes per hit) and resolves once.  deg is a 32-bit count of records: 2^32 - 1 hits or more
// are HG_ERR_UNSUPPORTED.
#include <algorithm>
#include <cstring>

#include "hg_block_scan.h"
#include "hg_cluster_common.h"
#include "hg_internal.h"

namespace {
constexpr uint32_t ST_UNDECIDED = 0, ST_REP = 1, ST_MEMBER = 2;
constexpr uint64_t SC_DEFAULT_ROUNDS = 4;            // rounds queued per readback of the undecided count
constexpr size_t SC_DEFAULT_HITS = (size_t)1 << 22;  // first size of the hit list (as hg_cluster_dev)
constexpr uint64_t SC_MAX_HITS = 0xFFFFFFFEull;      // deg[] counts records in 32 bits

struct SetCover {
  uint64_t *best;    // n: (ani key << 32 | 0xFFFFFFFF - representative) of the covering representative, 0 = none
  uint64_t *m1;      // n: largest key among the live neighbours (0 between rounds)
  uint64_t *m2;      // n: largest max(m1, key) among the live neighbours (0 between rounds)
  uint32_t *status;  // n: ST_*
  uint32_t *deg;     // n: live records at the node (0 between rounds)
  uint32_t *res;     // the ctx's clustering result words (HG_CLU_*)
  uint32_t round;    // rounds queued so far in this call
};

__device__ __forceinline__ uint64_t node_key(uint32_t deg, uint32_t v) { return (uint64_t)deg << 32 | (uint64_t)(0xFFFFFFFFu - v); }

// the two ends of a counting record; an index >= n is remembered in *err and the record skipped
__device__ __forceinline__ bool sc_edge(const hg_ani_hit *__restrict__ hits, size_t h, uint32_t n, float ani_th, uint32_t *err,
                                        uint32_t *a, uint32_t *b, float *ani) {
  const hg_ani_hit e = hits[h];
  if (e.ref_idx >= n || e.qry_idx >= n) {
    __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return false;
  }
  if (!(e.ani >= ani_th) || e.ref_idx == e.qry_idx) return false;  // (the side of the threshold exactly as in dist)
  *a = e.ref_idx, *b = e.qry_idx, *ani = e.ani;
  return true;
}

// res[HG_CLU_UNDECIDED] (the count "of the round before" the first one) is made non-zero
__global__ __launch_bounds__(256) void setcover_init_kernel(uint64_t *__restrict__ best, uint64_t *__restrict__ m1, uint64_t *__restrict__ m2,
                                                            uint32_t *__restrict__ status, uint32_t *__restrict__ deg, uint32_t n,
                                                            uint32_t *__restrict__ res) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    best[i] = 0ull, m1[i] = 0ull, m2[i] = 0ull, status[i] = ST_UNDECIDED, deg[i] = 0u;
  if (blockIdx.x == 0 && threadIdx.x < HG_CLU_WORDS) res[threadIdx.x] = threadIdx.x == HG_CLU_UNDECIDED ? 1u : 0u;
}

// One lane per record, grid-stride.  res[HG_CLU_UNDECIDED + parity]: the count of the previous round is read (0: the list
// is resolved, nothing to do), the one of this round is cleared for setcover_settle_kernel behind the launch boundaries.
__global__ __launch_bounds__(256) void setcover_count_kernel(const hg_ani_hit *__restrict__ hits, size_t n_hits, uint32_t n, float ani_th,
                                                             const uint32_t *__restrict__ status, uint32_t *deg, uint32_t *res,
                                                             uint32_t round) {
  const uint32_t left = res[HG_CLU_UNDECIDED + ((round - 1u) & 1u)];
  if (blockIdx.x == 0 && threadIdx.x == 0) res[HG_CLU_UNDECIDED + (round & 1u)] = 0u;
  if (left == 0u) return;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x; h < n_hits; h += stride) {
    uint32_t a, b;
    float ani;
    if (!sc_edge(hits, h, n, ani_th, res + HG_CLU_ERR, &a, &b, &ani)) continue;
    if (status[a] != ST_UNDECIDED || status[b] != ST_UNDECIDED) continue;
    (void)__hip_atomic_fetch_add(deg + a, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(deg + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One lane per record.  second == 0: key of each end into the other end's m1 word; second != 0: max(m1, key) of each end
// into the other end's m2 word.  What a launch reads (status, deg, and m1 in the second one) it does not write.
__global__ __launch_bounds__(256) void setcover_spread_kernel(const hg_ani_hit *__restrict__ hits, size_t n_hits, uint32_t n, float ani_th,
                                                              const uint32_t *__restrict__ status, const uint32_t *__restrict__ deg,
                                                              const uint64_t *from_m1, uint64_t *to, uint32_t *res, uint32_t round,
                                                              int second) {
  if (res[HG_CLU_UNDECIDED + ((round - 1u) & 1u)] == 0u) return;  // (uniform over the grid: nobody writes that word in this launch)
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x; h < n_hits; h += stride) {
    uint32_t a, b;
    float ani;
    if (!sc_edge(hits, h, n, ani_th, res + HG_CLU_ERR, &a, &b, &ani)) continue;
    if (status[a] != ST_UNDECIDED || status[b] != ST_UNDECIDED) continue;
    uint64_t ka = node_key(deg[a], a), kb = node_key(deg[b], b);
    if (second) {
      const uint64_t ma = from_m1[a], mb = from_m1[b];
      ka = ma > ka ? ma : ka, kb = mb > kb ? mb : kb;
    }
    (void)__hip_atomic_fetch_max(to + a, kb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_max(to + b, ka, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One lane per node.  Everything it reads was written behind a launch boundary.
__global__ __launch_bounds__(256) void setcover_select_kernel(uint32_t *__restrict__ status, uint32_t *__restrict__ deg,
                                                              uint64_t *__restrict__ m1, uint64_t *__restrict__ m2, uint32_t n,
                                                              const uint32_t *__restrict__ res, uint32_t round) {
  if (res[HG_CLU_UNDECIDED + ((round - 1u) & 1u)] == 0u) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || status[i] != ST_UNDECIDED) return;  // (the words of a decided node are zero already: no live record reaches it)
  const uint64_t key = node_key(deg[i], (uint32_t)i);
  if (m1[i] <= key && m2[i] <= key) status[i] = ST_REP;  // (keys of different nodes differ: the strict maximum of two hops)
  deg[i] = 0u, m1[i] = 0ull, m2[i] = 0ull;
}

// One lane per record (status is not written here: a duplicate with a higher ANI finds its end undecided too).
__global__ __launch_bounds__(256) void setcover_cover_kernel(const hg_ani_hit *__restrict__ hits, size_t n_hits, uint32_t n, float ani_th,
                                                             const uint32_t *__restrict__ status, uint64_t *best, uint32_t *res,
                                                             uint32_t round) {
  if (res[HG_CLU_UNDECIDED + ((round - 1u) & 1u)] == 0u) return;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x; h < n_hits; h += stride) {
    uint32_t a, b;
    float ani;
    if (!sc_edge(hits, h, n, ani_th, res + HG_CLU_ERR, &a, &b, &ani)) continue;
    const uint32_t sa = status[a], sb = status[b];
    // (a representative of an earlier round has no undecided neighbour left: this round's alone pass the test)
    if (sa == ST_REP && sb == ST_UNDECIDED)
      (void)__hip_atomic_fetch_max(best + b, (uint64_t)ani_key(ani) << 32 | (uint64_t)(0xFFFFFFFFu - a), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    else if (sb == ST_REP && sa == ST_UNDECIDED)
      (void)__hip_atomic_fetch_max(best + a, (uint64_t)ani_key(ani) << 32 | (uint64_t)(0xFFFFFFFFu - b), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One lane per node.  Everything it reads was written behind a launch boundary.
__global__ __launch_bounds__(256) void setcover_settle_kernel(uint32_t *__restrict__ status, const uint64_t *__restrict__ best, uint32_t n,
                                                              uint32_t *res, uint32_t round) {
  __shared__ uint32_t s_wave[4];
  if (res[HG_CLU_UNDECIDED + ((round - 1u) & 1u)] == 0u) return;  // (uniform over the grid: nobody writes that word in this launch)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t undecided = 0;
  if (i < n && status[i] == ST_UNDECIDED) {
    if (best[i]) status[i] = ST_MEMBER;
    else undecided = 1;
  }
  uint32_t total;
  (void)block_excl_scan<4>(undecided, s_wave, &total);
  if (threadIdx.x == 0) {
    if (total) __hip_atomic_fetch_add(res + HG_CLU_UNDECIDED + (round & 1u), total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (blockIdx.x == 0) res[HG_CLU_ROUNDS] += 1u;  // (this lane alone touches the word in this launch)
  }
}

__global__ __launch_bounds__(256) void setcover_finish_kernel(const uint64_t *__restrict__ best, const uint32_t *__restrict__ status,
                                                              uint32_t n, uint32_t *__restrict__ rep, float *__restrict__ ani) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t b = best[i];
    const bool is_rep = status[i] != ST_MEMBER || b == 0ull;  // (a member always has a best word: the second test only keeps rep[] in range)
    rep[i] = is_rep ? (uint32_t)i : 0xFFFFFFFFu - (uint32_t)b;
    if (ani) ani[i] = is_rep ? 100.0f : key_ani((uint32_t)(b >> 32));
  }
}

hg_status too_many_hits(hg_ctx *c) {
  return hg_fail(c, HG_ERR_UNSUPPORTED,
                 "the hit list of the set-cover resolution does not fit (2^32 - 1 hits or more): a higher threshold would");
}

// the whole list: init, rounds until no node is undecided, rep / ani, dense ids, the result words back
hg_status setcover_resolve(hg_ctx *c, const hg_ani_hit *d_hits, size_t n_hits, size_t n, float ani_th, uint32_t *d_rep,
                           uint32_t *d_cluster, float *d_ani, size_t *n_clusters) {
  hg_status s;
  SetCover g{};
  if ((s = hg_cluster_res(c, &g.res)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_setcover, n * 32 + 64)) != HG_OK) return s;
  g.best = static_cast<uint64_t *>(c->w_setcover.p);
  g.m1 = g.best + n, g.m2 = g.m1 + n;
  g.status = reinterpret_cast<uint32_t *>(g.m2 + n);
  g.deg = g.status + n;
  c->setcover_rounds = 0;
  const uint32_t m = (uint32_t)n;
  hipLaunchKernelGGL(setcover_init_kernel, dim3(grid_for(c, n)), dim3(256), 0, c->stream, g.best, g.m1, g.m2, g.status, g.deg, m, g.res);
  HG_HIP(c, hipGetLastError());
  const uint64_t per = c->dbg_setcover_rounds ? c->dbg_setcover_rounds : SC_DEFAULT_ROUNDS;
  const dim3 hit_grid(grid_for(c, n_hits)), node_grid((unsigned)((n + 255) / 256));
  for (;;) {
    for (uint64_t k = 0; k < per; ++k) {
      const uint32_t r = ++g.round;
      hipLaunchKernelGGL(setcover_count_kernel, hit_grid, dim3(256), 0, c->stream, d_hits, n_hits, m, ani_th, g.status, g.deg, g.res, r);
      HG_HIP(c, hipGetLastError());
      hipLaunchKernelGGL(setcover_spread_kernel, hit_grid, dim3(256), 0, c->stream, d_hits, n_hits, m, ani_th, g.status, g.deg, g.m1, g.m1,
                         g.res, r, 0);
      HG_HIP(c, hipGetLastError());
      hipLaunchKernelGGL(setcover_spread_kernel, hit_grid, dim3(256), 0, c->stream, d_hits, n_hits, m, ani_th, g.status, g.deg, g.m1, g.m2,
                         g.res, r, 1);
      HG_HIP(c, hipGetLastError());
      hipLaunchKernelGGL(setcover_select_kernel, node_grid, dim3(256), 0, c->stream, g.status, g.deg, g.m1, g.m2, m, g.res, r);
      HG_HIP(c, hipGetLastError());
      hipLaunchKernelGGL(setcover_cover_kernel, hit_grid, dim3(256), 0, c->stream, d_hits, n_hits, m, ani_th, g.status, g.best, g.res, r);
      HG_HIP(c, hipGetLastError());
      hipLaunchKernelGGL(setcover_settle_kernel, node_grid, dim3(256), 0, c->stream, g.status, g.best, m, g.res, r);
      HG_HIP(c, hipGetLastError());
    }
    const uint32_t *h_res = nullptr;
    if ((s = hg_publish_words(c, g.res, HG_CLU_WORDS, &h_res)) != HG_OK) return s;  // (nothing cleared: the call goes on)
    if (h_res[HG_CLU_UNDECIDED + (g.round & 1u)] == 0u) break;
  }
  hipLaunchKernelGGL(setcover_finish_kernel, dim3(grid_for(c, n)), dim3(256), 0, c->stream, g.best, g.status, m, d_rep, d_ani);
  HG_HIP(c, hipGetLastError());
  if ((s = hg_cluster_queue_ids(c, d_rep, n, d_cluster, g.res)) != HG_OK) return s;
  // (the publishing kernel clears the words behind its copy: the next clustering on this ctx starts clean)
  const uint32_t *h_res = nullptr;
  if ((s = hg_publish_words(c, g.res, HG_CLU_WORDS, &h_res, HG_CLU_WORDS)) != HG_OK) return s;
  c->setcover_rounds = h_res[HG_CLU_ROUNDS];
  if (h_res[HG_CLU_ERR]) return hg_fail(c, HG_ERR_INVALID, "a hit given to hg_cluster_setcover_hits_dev had an index >= n");
  *n_clusters = h_res[HG_CLU_COUNT];
  return HG_OK;
}

// The list grows to `hits` records and keeps its first `keep` ones (hg_ensure would drop them).
hg_status grow_list(hg_ctx *c, size_t keep, size_t hits) {
  hg_ctx::Buf bigger;
  hg_status s = hg_ensure(c, bigger, hits * sizeof(hg_ani_hit));  // (waits for the stream: nothing in flight uses the old block)
  if (s != HG_OK) return s;
  hipError_t e = hipSuccess;
  if (keep) e = hipMemcpyAsync(bigger.p, c->w_clu_hits.p, keep * sizeof(hg_ani_hit), hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    (void)hipFree(bigger.p);
    return hg_fail(c, HG_ERR_HIP, std::string("growing the hit list: ") + hipGetErrorString(e));
  }
  if (c->w_clu_hits.p) (void)hipFree(c->w_clu_hits.p);
  c->w_clu_hits = bigger;
  return HG_OK;
}

hg_status check_args(hg_ctx *c, size_t n, size_t *n_clusters) {
  if (!n_clusters) return hg_fail(c, HG_ERR_INVALID, "n_clusters == NULL");
  *n_clusters = 0;
  if (n > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "n must be < 2^31");
  return HG_OK;
}
hg_status check_metric(hg_ctx *c) {
  if (c->ani_metric == HG_ANI_CONTAINMENT)  // (the graph is undirected: HG_ANI_MASH or HG_ANI_MAX_CONTAINMENT)
    return hg_fail(c, HG_ERR_INVALID, "clustering needs a symmetric ANI metric: HG_ANI_CONTAINMENT is directional");
  return HG_OK;
}
}  // namespace

extern "C" uint64_t hg_ctx_cluster_setcover_rounds(const hg_ctx *c) { return c ? c->setcover_rounds : 0; }

extern "C" hg_status hg_cluster_setcover_hits_dev(hg_ctx *c, size_t n, const hg_ani_hit *d_hits, size_t n_hits, float ani_th,
                                                  uint32_t *d_rep, uint32_t *d_cluster, float *d_ani, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_args(c, n, n_clusters);
  if (s != HG_OK) return s;
  if (n_hits > 0xFFFFFFFFull) return too_many_hits(c);
  if (n == 0) return HG_OK;
  if (!d_rep || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (n_hits && !d_hits) return hg_fail(c, HG_ERR_INVALID, "NULL hit list");
  HG_ENTER(c);
  return setcover_resolve(c, d_hits, n_hits, n, ani_th, d_rep, d_cluster, d_ani, n_clusters);
}

extern "C" hg_status hg_cluster_setcover_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d,
                                             uint32_t ksize, float ani_th, uint32_t *d_rep, uint32_t *d_cluster, float *d_ani,
                                             size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_args(c, n, n_clusters);
  if (s != HG_OK) return s;
  if ((s = check_metric(c)) != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!d_hv || !d_norm2 || !d_rep || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  // The block loop of hg_cluster_dev: rows [r0, r0 + rows) x columns [r0, n) of the symmetric comparison, within the pairs
  // one launch may count ("pair_limit").  Every block writes behind the hits of the blocks before it; when it overflows
  // the list, the list grows to what is needed -- the earlier hits are kept -- and the block runs again
  // ("cluster_hit_cap": the list's first size).  The last row has no pairs of its own.
  const uint64_t pair_limit = hg_pair_limit(c);
  const uint64_t pairs = (uint64_t)n * (n - 1) / 2;
  size_t cap = c->dbg_cluster_hit_cap ? (size_t)c->dbg_cluster_hit_cap
                                      : std::max(c->w_clu_hits.cap / sizeof(hg_ani_hit), (size_t)std::min<uint64_t>(pairs, SC_DEFAULT_HITS));
  if ((s = hg_ensure(c, c->w_clu_hits, std::max<size_t>(cap, 1) * sizeof(hg_ani_hit))) != HG_OK) return s;
  size_t total = 0;
  for (size_t r0 = 0; r0 + 1 < n;) {
    const size_t cols = n - r0, rows = (size_t)std::min<uint64_t>(cols, std::max<uint64_t>(1, pair_limit / cols));
    size_t got = 0;
    for (;;) {
      s = hg_dist_block_dev(c, d_hv + r0 * (size_t)hv_d, d_norm2 + r0, rows, r0, d_hv + r0 * (size_t)hv_d, d_norm2 + r0, cols, r0,
                            hv_d, ksize, 1, ani_th, static_cast<hg_ani_hit *>(c->w_clu_hits.p) + total, cap - total, &got);
      if (s != HG_ERR_CAPACITY) break;
      // (a capacity retry: the block ran to the end and counted every hit)
      if ((uint64_t)total + got > SC_MAX_HITS) return too_many_hits(c);
      if ((s = grow_list(c, total, total + got)) != HG_OK) return s;
      cap = c->w_clu_hits.cap / sizeof(hg_ani_hit);  // (with the slack hg_ensure adds: the blocks that follow grow it less often)
    }
    if (s != HG_OK) return s;
    total += got;
    if ((uint64_t)total > SC_MAX_HITS) return too_many_hits(c);
    r0 += rows;
  }
  return setcover_resolve(c, static_cast<const hg_ani_hit *>(c->w_clu_hits.p), total, n, ani_th, d_rep, d_cluster, d_ani, n_clusters);
}

extern "C" hg_status hg_cluster_setcover(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                         float ani_th, uint32_t *rep, uint32_t *cluster, float *ani, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_args(c, n, n_clusters);
  if (s != HG_OK) return s;
  if ((s = check_metric(c)) != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!hv || !norm2 || !rep || !cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  const size_t hb = n * (size_t)hv_d * sizeof(int16_t);
  if ((s = hg_ensure(c, c->w_hv, hb + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_n2a, n * sizeof(int32_t) + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_ani, 3 * n * sizeof(uint32_t) + 64)) != HG_OK) return s;
  HG_HIP(c, hipMemcpyAsync(c->w_hv.p, hv, hb, hipMemcpyHostToDevice, c->stream));
  HG_HIP(c, hipMemcpyAsync(c->w_n2a.p, norm2, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  auto *d_rep = static_cast<uint32_t *>(c->w_ani.p), *d_cluster = d_rep + n;
  auto *d_ani = reinterpret_cast<float *>(d_cluster + n);
  if ((s = hg_cluster_setcover_dev(c, static_cast<const int16_t *>(c->w_hv.p), static_cast<const int32_t *>(c->w_n2a.p), n, hv_d, ksize,
                                   ani_th, d_rep, d_cluster, d_ani, n_clusters)) != HG_OK)
    return s;
  HG_HIP(c, hipMemcpyAsync(rep, d_rep, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(cluster, d_cluster, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (ani) HG_HIP(c, hipMemcpyAsync(ani, d_ani, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}
