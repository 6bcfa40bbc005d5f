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
// Then rep / ani from status and best (hg_cluster_queue_rep_ani), and the dense ids with hg_cluster.hip's finishing
// launches (every tree has depth 1).
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
// comparison to one list (12 bytes per hit; hg_cluster_row_blocks' append mode) and resolves once.  deg is a 32-bit count of records: 2^32 - 1 hits or more
// are HG_ERR_UNSUPPORTED.
#include <algorithm>
#include <cstring>

#include "hg_block_scan.h"
#include "hg_cluster_common.h"
#include "hg_internal.h"

namespace {
constexpr uint64_t SC_DEFAULT_ROUNDS = 4;  // rounds queued per readback of the undecided count

struct SetCover {
  uint64_t *best;    // n: best_word of the covering representative, 0 = none
  uint64_t *m1;      // n: largest key among the live neighbours (0 between rounds)
  uint64_t *m2;      // n: largest max(m1, key) among the live neighbours (0 between rounds)
  uint32_t *status;  // n: ST_*
  uint32_t *deg;     // n: live records at the node (0 between rounds)
  uint32_t *res;     // the ctx's clustering result words (HG_CLU_*)
  uint32_t round;    // rounds queued so far in this call
};

__device__ __forceinline__ uint64_t node_key(uint32_t deg, uint32_t v) { return (uint64_t)deg << 32 | (uint64_t)(0xFFFFFFFFu - v); }

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
    const hg_ani_hit e = hits[h];
    if (!hit_counts(e, n, ani_th, res + HG_CLU_ERR)) continue;
    const uint32_t a = e.ref_idx, b = e.qry_idx;
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
    const hg_ani_hit e = hits[h];
    if (!hit_counts(e, n, ani_th, res + HG_CLU_ERR)) continue;
    const uint32_t a = e.ref_idx, b = e.qry_idx;
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
    const hg_ani_hit e = hits[h];
    if (!hit_counts(e, n, ani_th, res + HG_CLU_ERR)) continue;
    const uint32_t a = e.ref_idx, b = e.qry_idx;
    const uint32_t sa = status[a], sb = status[b];
    // (a representative of an earlier round has no undecided neighbour left: this round's alone pass the test)
    if (sa == ST_REP && sb == ST_UNDECIDED)
      (void)__hip_atomic_fetch_max(best + b, best_word(e.ani, a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (sb == ST_REP && sa == ST_UNDECIDED)
      (void)__hip_atomic_fetch_max(best + a, best_word(e.ani, b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
  if ((s = hg_cluster_queue_rep_ani(c, g.best, g.status, n, d_rep, d_ani)) != HG_OK) return s;
  if ((s = hg_cluster_queue_ids(c, d_rep, n, d_cluster, g.res)) != HG_OK) return s;
  return hg_cluster_close(c, g.res, &c->setcover_rounds, "hg_cluster_setcover_hits_dev", n_clusters);
}
}  // namespace

extern "C" uint64_t hg_ctx_cluster_setcover_rounds(const hg_ctx *c) { return c ? c->setcover_rounds : 0; }

extern "C" hg_status hg_cluster_setcover_hits_dev(hg_ctx *c, size_t n, const hg_ani_hit *d_hits, size_t n_hits, float ani_th,
                                                  uint32_t *d_rep, uint32_t *d_cluster, float *d_ani, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_cluster_check(c, n, n_clusters, false);
  if (s != HG_OK) return s;
  if (n_hits > 0xFFFFFFFFull) return hg_cluster_list_too_long(c);
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
  hg_status s = hg_cluster_check(c, n, n_clusters, true);
  if (s != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!d_hv || !d_norm2 || !d_rep || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  // every row block's hits behind those of the blocks before it, nothing done per block: the rule is global
  size_t total = 0;
  s = hg_cluster_row_blocks(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, true, &total,
                            [](const hg_ani_hit *, size_t, size_t, size_t) { return HG_OK; });
  if (s != HG_OK) return s;
  return setcover_resolve(c, static_cast<const hg_ani_hit *>(c->w_clu_hits.p), total, n, ani_th, d_rep, d_cluster, d_ani, n_clusters);
}

extern "C" hg_status hg_cluster_setcover(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                         float ani_th, uint32_t *rep, uint32_t *cluster, float *ani, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_cluster_check(c, n, n_clusters, true);
  if (s != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!hv || !norm2 || !rep || !cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  const int16_t *d_hv;
  const int32_t *d_norm2;
  uint32_t *d_rep;
  if ((s = hg_cluster_stage(c, hv, norm2, n, hv_d, 3 * n * sizeof(uint32_t), &d_hv, &d_norm2, &d_rep)) != HG_OK) return s;
  uint32_t *d_cluster = d_rep + n;
  auto *d_ani = reinterpret_cast<float *>(d_cluster + n);
  if ((s = hg_cluster_setcover_dev(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, d_rep, d_cluster, d_ani, n_clusters)) != HG_OK) return s;
  HG_HIP(c, hipMemcpyAsync(rep, d_rep, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(cluster, d_cluster, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (ani) HG_HIP(c, hipMemcpyAsync(ani, d_ani, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}
