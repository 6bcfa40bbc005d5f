// hg_cluster_greedy.hip -- greedy representative clustering of sketches at an ANI threshold (an extension like
// hg_cluster.hip: what dereplication tools do, CD-HIT's incremental scheme).  The nodes are walked in index order: node i
// is a REPRESENTATIVE iff no representative j < i has ani(j, i) >= ani_th, otherwise a MEMBER of the representative j < i
// with the highest ani(j, i) (float comparison, ties to the smallest j).  A member covers nobody.  Representatives are
// pairwise below the threshold, every member is at or above it with its own representative.
//
// The sequential walk is resolved in ROUNDS over the hits of one block of rows [r0, r1) (the whole list for
// hg_cluster_greedy_hits_dev, a row block of the symmetric comparison for hg_cluster_greedy_dev):
//   * enter   : a block node that a representative of an EARLIER block covers (best != 0) is a member, every other one
//               is undecided;
//   * mark    : one lane per hit lo < hi with both ends in the block: lo a representative -> hi becomes a member;
//               both undecided -> hi is blocked this round (blocked[hi] = the round's number: nothing is cleared);
//   * decide  : one lane per block node: undecided and not blocked this round -> representative; the nodes that stay
//               undecided are counted into a device word;
//   * assign  : once per block, over ALL its hits: lo a representative -> atomic max of (ani, -lo) into best[hi].  Columns
//               behind the block get their coverage here, which is the entry condition of the blocks that follow;
//   * finish  : rep / ani from status and best (hg_cluster_queue_rep_ani), then the dense ids with hg_cluster.hip's
//               finishing launches (every tree has depth 1).
// Every kernel runs to its end on its own: no cooperative launch, no grid-wide barrier, no workgroup waits for another
// one's store.  The host queues a few rounds, reads the undecided count back (hg_publish_words) and stops at 0; the
// rounds queued behind the one that reached 0 see that word and return at once.
//
// Why it is correct.  Status moves undecided -> member inside mark and undecided -> representative inside decide, and
// never back.  Representatives are written by decide only, so mark -- behind a launch boundary -- sees every one of them;
// a lane of mark that reads a stale "undecided" for a node another lane has just made a member only blocks `hi`
// needlessly for this round.  A node becomes a representative when it is undecided after mark and no lane blocked it:
// then every earlier neighbour inside the block was read as decided (decisions are final), none of them is a
// representative (that lane would have made the node a member, and decide reads status behind the launch boundary), and
// no representative of an earlier block covers it (enter).  That is the sequential rule.  A node becomes a member only
// through a hit from a representative with a smaller index.  best[] is an atomic max over a total order of (ani, index),
// so neither the order of the hits, the blocks, the rounds per readback nor the scheduling show in the result.
// Why it ends.  The smallest undecided node of the block has only decided earlier neighbours: nothing blocks it, and
// the round makes it a member or a representative.  The worst case is a path 0 - 1 - 2 - ...: one or two nodes per
// round, about rows / 2 rounds for a block of `rows` nodes.  It is accepted: dense groups -- what a dereplication
// sees -- resolve in about two rounds (representative, then its members).
//
// Cross-workgroup traffic inside one launch is the two benign races of mark (status -> member, the blocked mark; agent-scope
// relaxed atomics, so that a read is served by L2 and a write goes there) and the atomic max of assign / the counter of
// decide.  Everything else is read behind a launch boundary.
//
// The hits with both ends in the block are not partitioned off: mark tests `hi < r1` per hit.  With the one-block
// hit-list form, and whenever n^2 / 2 stays within one launch's pairs, every hit passes the test; the alternatives (a
// partition per block, the diagonal square as its own dist call) were not measured.
#include <algorithm>
#include <cstring>

#include "hg_block_scan.h"
#include "hg_cluster_common.h"
#include "hg_internal.h"

namespace {
constexpr uint64_t GR_DEFAULT_ROUNDS = 4;  // rounds queued per readback of the undecided count

__device__ __forceinline__ uint32_t st_load(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_store(uint32_t *p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct Greedy {
  uint64_t *best;     // n: best_word of the best covering representative, 0 = none
  uint32_t *status;   // n: ST_*
  uint32_t *blocked;  // n: number of the last round that blocked the node
  uint32_t *res;      // the ctx's clustering result words (HG_CLU_*)
  uint32_t round;     // rounds queued so far in this call (1-based stamps of blocked[])
};

__global__ __launch_bounds__(256) void greedy_init_kernel(uint64_t *__restrict__ best, uint32_t *__restrict__ blocked, uint32_t n,
                                                          uint32_t *__restrict__ res) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) best[i] = 0ull, blocked[i] = 0u;
  if (blockIdx.x == 0 && threadIdx.x < HG_CLU_WORDS) res[threadIdx.x] = 0u;
}

// block entry; prev_word (the undecided count "of the round before" the block's first one) is made non-zero
__global__ __launch_bounds__(256) void greedy_enter_kernel(const uint64_t *__restrict__ best, uint32_t *__restrict__ status,
                                                           uint32_t r0, uint32_t r1, uint32_t *__restrict__ prev_word) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)r0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < r1; i += stride)
    status[i] = best[i] ? ST_MEMBER : ST_UNDECIDED;
  if (blockIdx.x == 0 && threadIdx.x == 0) *prev_word = 1u;
}

// One lane per hit, grid-stride.  res[HG_CLU_UNDECIDED + parity]: the count of the previous round is read (0: the block
// is resolved, nothing to do), the one of this round is cleared for greedy_decide_kernel behind the launch boundary.
__global__ __launch_bounds__(256) void greedy_mark_kernel(const hg_ani_hit *__restrict__ hits, size_t n_hits, uint32_t n, uint32_t r0,
                                                          uint32_t r1, float ani_th, uint32_t *status, uint32_t *blocked,
                                                          uint32_t *res, uint32_t round) {
  const uint32_t left = res[HG_CLU_UNDECIDED + ((round - 1u) & 1u)];
  if (blockIdx.x == 0 && threadIdx.x == 0) res[HG_CLU_UNDECIDED + (round & 1u)] = 0u;
  if (left == 0u) return;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x; h < n_hits; h += stride) {
    const hg_ani_hit e = hits[h];
    uint32_t lo, hi;
    if (!hit_edge(e, n, ani_th, res + HG_CLU_ERR, &lo, &hi)) continue;
    if (lo < r0 || hi >= r1) continue;  // (a column behind the block: assign covers it, its own block decides it)
    const uint32_t s_lo = st_load(status + lo);
    if (s_lo == ST_REP) st_store(status + hi, ST_MEMBER);
    else if (s_lo == ST_UNDECIDED && st_load(status + hi) == ST_UNDECIDED) st_store(blocked + hi, round);
  }
}

// One lane per block node.  Everything it reads was written behind a launch boundary.
__global__ __launch_bounds__(256) void greedy_decide_kernel(uint32_t *__restrict__ status, const uint32_t *__restrict__ blocked,
                                                            uint32_t r0, uint32_t r1, uint32_t *res, uint32_t round) {
  __shared__ uint32_t s_wave[4];
  if (res[HG_CLU_UNDECIDED + ((round - 1u) & 1u)] == 0u) return;  // (uniform over the grid: nobody writes that word in this launch)
  const size_t i = (size_t)r0 + (size_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t undecided = 0;
  if (i < r1 && status[i] == ST_UNDECIDED) {
    if (blocked[i] == round) undecided = 1;
    else status[i] = ST_REP;
  }
  uint32_t total;
  (void)block_excl_scan<4>(undecided, s_wave, &total);
  if (threadIdx.x == 0) {
    if (total) __hip_atomic_fetch_add(res + HG_CLU_UNDECIDED + (round & 1u), total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (blockIdx.x == 0) res[HG_CLU_ROUNDS] += 1u;  // (this lane alone touches the word in this launch)
  }
}

// One lane per hit of the block (status is final for the block's rows and not written here).
__global__ __launch_bounds__(256) void greedy_assign_kernel(const hg_ani_hit *__restrict__ hits, size_t n_hits, uint32_t n, uint32_t r0,
                                                            uint32_t r1, float ani_th, const uint32_t *__restrict__ status,
                                                            uint64_t *best, uint32_t *res) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x; h < n_hits; h += stride) {
    const hg_ani_hit e = hits[h];
    uint32_t lo, hi;
    if (!hit_edge(e, n, ani_th, res + HG_CLU_ERR, &lo, &hi)) continue;
    if (lo < r0 || lo >= r1 || status[lo] != ST_REP) continue;
    (void)__hip_atomic_fetch_max(best + hi, best_word(e.ani, lo), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

hg_status greedy_begin(hg_ctx *c, size_t n, Greedy *g) {
  hg_status s;
  if ((s = hg_cluster_res(c, &g->res)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_grd, n * 16 + 64)) != HG_OK) return s;
  g->best = static_cast<uint64_t *>(c->w_grd.p);
  g->status = reinterpret_cast<uint32_t *>(g->best + n);
  g->blocked = g->status + n;
  g->round = 0;
  c->greedy_rounds = 0;
  hipLaunchKernelGGL(greedy_init_kernel, dim3(grid_for(c, n)), dim3(256), 0, c->stream, g->best, g->blocked, (uint32_t)n, g->res);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

// rows [r0, r1) against the block's hits: enter, rounds until no node of the block is undecided, assign
hg_status greedy_block(hg_ctx *c, Greedy *g, const hg_ani_hit *d_hits, size_t n_hits, size_t n, size_t r0, size_t r1, float ani_th) {
  hg_status s;
  const uint32_t m = (uint32_t)n, a = (uint32_t)r0, b = (uint32_t)r1;
  hipLaunchKernelGGL(greedy_enter_kernel, dim3(grid_for(c, r1 - r0)), dim3(256), 0, c->stream, g->best, g->status, a, b,
                     g->res + HG_CLU_UNDECIDED + (g->round & 1u));
  HG_HIP(c, hipGetLastError());
  const uint64_t per = c->dbg_greedy_rounds ? c->dbg_greedy_rounds : GR_DEFAULT_ROUNDS;
  const unsigned node_grid = (unsigned)((r1 - r0 + 255) / 256);
  for (;;) {
    for (uint64_t k = 0; k < per; ++k) {
      ++g->round;
      hipLaunchKernelGGL(greedy_mark_kernel, dim3(grid_for(c, n_hits)), dim3(256), 0, c->stream, d_hits, n_hits, m, a, b, ani_th,
                         g->status, g->blocked, g->res, g->round);
      HG_HIP(c, hipGetLastError());
      hipLaunchKernelGGL(greedy_decide_kernel, dim3(node_grid), dim3(256), 0, c->stream, g->status, g->blocked, a, b, g->res, g->round);
      HG_HIP(c, hipGetLastError());
    }
    const uint32_t *h_res = nullptr;
    if ((s = hg_publish_words(c, g->res, HG_CLU_WORDS, &h_res)) != HG_OK) return s;  // (nothing cleared: the call goes on)
    if (h_res[HG_CLU_UNDECIDED + (g->round & 1u)] == 0u) break;
  }
  hipLaunchKernelGGL(greedy_assign_kernel, dim3(grid_for(c, n_hits)), dim3(256), 0, c->stream, d_hits, n_hits, m, a, b, ani_th, g->status,
                     g->best, g->res);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

hg_status greedy_end(hg_ctx *c, Greedy *g, size_t n, uint32_t *d_rep, uint32_t *d_cluster, float *d_ani, size_t *n_clusters) {
  hg_status s;
  if ((s = hg_cluster_queue_rep_ani(c, g->best, g->status, n, d_rep, d_ani)) != HG_OK) return s;
  if ((s = hg_cluster_queue_ids(c, d_rep, n, d_cluster, g->res)) != HG_OK) return s;
  return hg_cluster_close(c, g->res, &c->greedy_rounds, "hg_cluster_greedy_hits_dev", n_clusters);
}
}  // namespace

extern "C" uint64_t hg_ctx_cluster_greedy_rounds(const hg_ctx *c) { return c ? c->greedy_rounds : 0; }

extern "C" hg_status hg_cluster_greedy_hits_dev(hg_ctx *c, size_t n, const hg_ani_hit *d_hits, size_t n_hits, float ani_th,
                                                uint32_t *d_rep, uint32_t *d_cluster, float *d_ani, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_cluster_check(c, n, n_clusters, false);
  if (s != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!d_rep || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (n_hits && !d_hits) return hg_fail(c, HG_ERR_INVALID, "NULL hit list");
  HG_ENTER(c);
  Greedy g{};
  if ((s = greedy_begin(c, n, &g)) != HG_OK) return s;
  if ((s = greedy_block(c, &g, d_hits, n_hits, n, 0, n, ani_th)) != HG_OK) return s;  // the list is one block over all rows
  return greedy_end(c, &g, n, d_rep, d_cluster, d_ani, n_clusters);
}

extern "C" hg_status hg_cluster_greedy_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d,
                                           uint32_t ksize, float ani_th, uint32_t *d_rep, uint32_t *d_cluster, float *d_ani,
                                           size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_cluster_check(c, n, n_clusters, true);
  if (s != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!d_hv || !d_norm2 || !d_rep || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  Greedy g{};
  if ((s = greedy_begin(c, n, &g)) != HG_OK) return s;
  // Each row block is resolved before the next one reuses the list; the last row has no pairs of its own but is a block
  // all the same (its node is decided like any other).
  s = hg_cluster_row_blocks(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, false, nullptr,
                            [&](const hg_ani_hit *d_hits, size_t got, size_t r0, size_t r1) {
                              return greedy_block(c, &g, d_hits, got, n, r0, r1, ani_th);
                            });
  if (s != HG_OK) return s;
  return greedy_end(c, &g, n, d_rep, d_cluster, d_ani, n_clusters);
}

extern "C" hg_status hg_cluster_greedy(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
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
  if ((s = hg_cluster_greedy_dev(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, d_rep, d_cluster, d_ani, n_clusters)) != HG_OK) return s;
  HG_HIP(c, hipMemcpyAsync(rep, d_rep, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(cluster, d_cluster, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (ani) HG_HIP(c, hipMemcpyAsync(ani, d_ani, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}
