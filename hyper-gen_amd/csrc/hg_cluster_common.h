// hg_cluster_common.h -- what the clustering files share (hg_cluster.hip, hg_cluster_greedy.hip, hg_cluster_setcover.hip,
// hg_cluster_tree.hip; hg_hits.hip for the tree's edge order).  Host side: the ctx's result words and the helpers of
// hg_cluster.hip that every scheme is built from -- the argument check, the staging of the host forms, the row-block
// driver of the symmetric comparison, the finishing launches and the closing readback.  Device side: the rule for which
// hit record counts, the lock-free union-find over rep[n], the order-preserving ANI key, the node states and the best[]
// word of the representative schemes, and the grid of a grid-stride launch.  One copy of each.
#pragma once
#include <algorithm>
#include <functional>

#include "hg_internal.h"

// The ctx's 16 clustering result words (w_clu_res): [0] cluster count, [1] error word (a hit with an index >= n); the
// greedy and the set-cover resolution keep [2], [3] = nodes still undecided after the odd / even rounds and [4] = rounds
// run behind them;
// the tree resolution [5], [6] = roots that selected an edge in the odd / even rounds, [7] = edges of the forest being
// written, and counts its rounds in [4] too.
// The call that reads them back clears them behind the copy (hg_publish_words), but no entry point may count on finding
// them zero: an incremental clustering dropped behind hg_cluster_add_hits_dev leaves [1] raised.  Every scheme's init kernel
// clears the words it uses, and hg_cluster_stats*, which has none, clears its two in front of its first kernel.
enum : uint32_t {
  HG_CLU_COUNT = 0,
  HG_CLU_ERR = 1,
  HG_CLU_UNDECIDED = 2,
  HG_CLU_ROUNDS = 4,
  HG_CLU_SELECTING = 5,
  HG_CLU_EDGES = 7,
  HG_CLU_WORDS = 8
};
hg_status hg_cluster_res(hg_ctx *ctx, uint32_t **out);

// The checks every entry point starts with, in this order: n_clusters (zeroed), n < 2^31, and for the forms that run the
// comparison themselves (dist_form) a symmetric metric.
hg_status hg_cluster_check(hg_ctx *ctx, size_t n, size_t *n_clusters, bool dist_form);

// The host forms' staging: hv and norm2 uploaded into w_hv / w_n2a, out_bytes of w_ani for the results (all stream-ordered).
hg_status hg_cluster_stage(hg_ctx *ctx, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, size_t out_bytes,
                           const int16_t **d_hv, const int32_t **d_norm2, uint32_t **d_out);

// The symmetric comparison of n resident sketches as row blocks [r0, r1) x columns [r0, n), r0 = 0 .. n: each block stays
// within the pairs one launch may count (hg_pair_limit) and hands block(d_hits, got, r0, r1) its hits in w_clu_hits.  The
// last row is a block of its own without pairs: got = 0, nothing is launched for it.  When a block's hits outgrow the
// list, the list grows to the reported count and the block runs again ("cluster_hit_cap": the list's first size).
//   reuse  : every block writes at the front of the list -- block() must have queued all its reads before it returns;
//   append : every block writes behind the hits of the blocks before it, which growing keeps; d_hits is the block's own
//            part.  *total = the hits of all blocks, in w_clu_hits.p; HG_CLU_MAX_LIST of them at most (HG_ERR_UNSUPPORTED).
constexpr size_t HG_CLU_DEFAULT_HITS = (size_t)1 << 22;  // first size of the list (48 MB)
constexpr uint64_t HG_CLU_MAX_LIST = 0xFFFFFFFEull;       // (the set-cover resolution counts records in 32 bits)
using hg_cluster_block_fn = std::function<hg_status(const hg_ani_hit *d_hits, size_t got, size_t r0, size_t r1)>;
hg_status hg_cluster_row_blocks(hg_ctx *ctx, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                float ani_th, bool append, size_t *total, const hg_cluster_block_fn &block);
hg_status hg_cluster_list_too_long(hg_ctx *ctx);

// rep[i] / ani[i] (ani may be NULL) of the representative schemes from their best[] and status[] (below): one launch.
hg_status hg_cluster_queue_rep_ani(hg_ctx *ctx, const uint64_t *best, const uint32_t *status, size_t n, uint32_t *d_rep, float *d_ani);
// rep[] (trees of any depth) -> rep[i] = root, d_cluster = dense ids of the roots in index order, res[HG_CLU_COUNT] = their
// number: the compress / scan / root-id / member-id launches of hg_cluster_finish_dev, stream-ordered, nothing read back.
hg_status hg_cluster_queue_ids(hg_ctx *ctx, uint32_t *d_rep, size_t n, uint32_t *d_cluster, uint32_t *res);
// The end of a round-based call: the HG_CLU_WORDS result words read back and cleared behind the copy (the next
// clustering on this ctx starts clean), *rounds = the rounds run, *count = the cluster count; a set error word fails the
// call with hits_fn -- the entry point that takes a caller's list -- in the text.
hg_status hg_cluster_close(hg_ctx *ctx, uint32_t *res, uint64_t *rounds, const char *hits_fn, size_t *count);

// The order of a single-linkage tree (hg_hits.hip's stable radix passes: qry_idx ascending, then ref_idx ascending, then
// ANI descending by its order-preserving key): d_in[0, n) -> d_out[0, n), n < 2^31, every index < n_nodes, stream-ordered.
// d_out != d_in.
hg_status hg_sort_tree_edges_dev(hg_ctx *ctx, const hg_ani_hit *d_in, size_t n, size_t n_nodes, hg_ani_hit *d_out);

// Which hit record counts, for every scheme: both indices < n (one that is not sets *err when err is given, and the
// record is skipped), ani >= ani_th on the side of the threshold exactly as in dist (NaN never counts), not a self pair.
__device__ __forceinline__ bool hit_counts(const hg_ani_hit &e, uint32_t n, float ani_th, uint32_t *err) {
  if (e.ref_idx >= n || e.qry_idx >= n) {
    if (err) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return false;
  }
  if (!(e.ani >= ani_th) || e.ref_idx == e.qry_idx) return false;
  return true;
}
// ... and its ends in order: the edge {lo, hi}
__device__ __forceinline__ bool hit_edge(const hg_ani_hit &e, uint32_t n, float ani_th, uint32_t *err, uint32_t *lo, uint32_t *hi) {
  if (!hit_counts(e, n, ani_th, err)) return false;
  *lo = e.ref_idx < e.qry_idx ? e.ref_idx : e.qry_idx, *hi = e.ref_idx < e.qry_idx ? e.qry_idx : e.ref_idx;
  return true;
}

// Inside a hooking kernel other workgroups -- on other CUs, other XCDs -- move rep[] under our feet: a CU's L1 is never
// refreshed by another CU's stores and the XCDs' L2s are not coherent with each other, so a plain load could return a
// value that is stale for as long as the line stays cached, and a CAS loop fed by it would spin.  Every access of rep[] in
// such a kernel is therefore an agent-scope atomic (relaxed: each value read is used only for itself -- correctness needs
// no ordering between locations, see find_root and the hooking loops).
__device__ __forceinline__ uint32_t rep_load(uint32_t *rep, uint32_t x) {
  return __hip_atomic_load(rep + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rep_store(uint32_t *rep, uint32_t x, uint32_t v) {
  __hip_atomic_store(rep + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Invariants of rep[] (they hold for every value any lane can read, stale or fresh):
//   (1) rep[x] <= x, and rep[x] < x once x is not a root: only a CAS on a root writes a smaller index into it, path
//       halving writes into non-roots only, and always an ancestor, which is smaller;
//   (2) a non-root never becomes a root again (nothing writes x into rep[x] after init);
//   (3) an ancestor stays an ancestor: trees only merge.
// find_root terminates because x strictly decreases in every step (1).  A root it returns may be stale -- hooked meanwhile
// -- but is an ancestor of the argument (3); the CAS of the hooking loop finds out.
__device__ __forceinline__ uint32_t find_root(uint32_t *rep, uint32_t x) {
  uint32_t p = rep_load(rep, x);
  while (p != x) {
    const uint32_t g = rep_load(rep, p);
    if (g == p) return p;
    rep_store(rep, x, g);  // path halving: x skips its parent (x is a non-root, g an ancestor of it)
    x = g;
    p = rep_load(rep, x);
  }
  return x;
}

// The union of the trees of x and y.  Why the loop terminates: each round either hooks (CAS succeeds: done) or the CAS
// fails, which means `hi` is no longer a root -- another lane hooked it under a smaller index, which the CAS returns (1).
// The loop then goes on with the root of that index, which is < hi, in place of hi: a + b strictly decreases every round
// and is bounded below.  When a == b both ends share an ancestor, and by (3) they stay in one tree.
__device__ __forceinline__ void hook_roots(uint32_t *rep, uint32_t x, uint32_t y) {
  uint32_t a = find_root(rep, x), b = find_root(rep, y);
  while (a != b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    uint32_t seen = hi;
    if (__hip_atomic_compare_exchange_strong(rep + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      break;
    a = lo, b = find_root(rep, seen);  // hi was hooked under seen < hi
  }
}

// Any float -> a 32-bit key of the same order (negative values and both zeros included; -0.0f + 0.0f = +0.0f), and back.
// No float that is not a NaN has the key 0.
__device__ __forceinline__ uint32_t ani_key(float a) {
  const uint32_t b = __float_as_uint(a + 0.0f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_ani(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// The representative schemes (greedy, set cover): a node's state, and its best[] word -- the covering representative with
// the highest ANI, ties to the smallest index, as one 64-bit maximum: ani key << 32 | 0xFFFFFFFF - representative; 0 = none.
enum : uint32_t { ST_UNDECIDED = 0, ST_REP = 1, ST_MEMBER = 2 };
__device__ __forceinline__ uint64_t best_word(float ani, uint32_t rep) { return (uint64_t)ani_key(ani) << 32 | (uint64_t)(0xFFFFFFFFu - rep); }
__device__ __forceinline__ void best_unpack(uint64_t b, uint32_t *rep, float *ani) {
  *rep = 0xFFFFFFFFu - (uint32_t)b, *ani = key_ani((uint32_t)(b >> 32));
}

// workgroups of 256 lanes for a grid-stride loop over `items`
inline unsigned grid_for(hg_ctx *c, size_t items) {
  const size_t want = (items + 255) / 256, most = (size_t)c->n_cu * 16;
  return (unsigned)std::max<size_t>(1, std::min(want, most));
}
