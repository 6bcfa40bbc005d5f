// hg_cluster_tree.hip -- the single-linkage tree of sketches above an ANI floor (an extension like hg_cluster.hip): the
// maximum-ANI spanning forest of the hit graph.  It has n - clusters <= n - 1 edges however many pairs lie above the
// floor; cut at any threshold t >= the floor (hg_cluster_init_dev + hg_cluster_add_hits_dev(tree, t) +
// hg_cluster_finish_dev) it gives the components of the full graph at t; its edges, strongest first, are the merge
// order of single-linkage clustering.
//
// A hit counts iff ani >= ani_th (dist's float comparison) and its ends differ; it is the edge {lo, hi}.  Edge e is
// STRONGER than f iff ani(e) > ani(f), or the ANIs are equal and (lo, hi)(e) < (lo, hi)(f) lexicographically; two edges
// equal in all three are the same edge.  The tree is what Kruskal builds under that order, written strongest first.
//
// It is resolved as Boruvka rounds over a candidate list (the whole list for hg_cluster_tree_hits_dev; for
// hg_cluster_tree_dev the forest carried from the row blocks before plus the block's hits, from singleton components):
//   * best_ani  : one lane per candidate whose ends lie in different components: atomic max of the ANI key into
//                 best_ani[] of both components;
//   * best_pair : the same candidates: where the key equals the component's best, atomic min of lo << 32 | hi into its
//                 best_pair[].  Two passes because the order has 96 bits and the atomics 64;
//   * select    : one lane per node: a root with a selection emits its edge into the new forest (one counter add per
//                 wave) unless the other end's component selected the same edge and has the smaller root; the
//                 selecting roots are counted into the round's word;
//   * hook      : one lane per node: the selected edge's ends are united (find_root + CAS, hg_cluster_common.h);
//   * compress  : comp[i] = root(i), both best words cleared for the next round.
// Every kernel runs to its end on its own: no cooperative launch, no grid-wide barrier, no workgroup waits for another
// one's store.  The host queues a few rounds, reads the count of selecting roots back (hg_publish_words) and stops at 0;
// the rounds queued behind the one that reached 0 see that word and return at once.
//
// Why it is correct.  The order is strict and total on distinct edges, so the forest Kruskal builds is the only
// maximum spanning forest, and an edge that is the strongest one leaving some component -- of ANY partition into connected
// pieces of that forest -- belongs to it (cut property).  best_ani / best_pair are atomic max / min over that order, read
// behind a launch boundary: after the two passes best_pair[c] is exactly the strongest edge leaving component c, whatever
// the order of the candidates, the block size or the scheduling.  An edge leaves exactly two components, so it is
// selected at most twice, and select emits it once (the smaller root).  The selected edges of a round hold no cycle
// other than those pairs: along a cycle of components each selection would have to be strictly stronger than the one
// before.  So the emitted edges are forest edges, none twice.  comp[] is compressed before a round reads it, so every
// lane sees the same components.  When no root selects, no candidate joins two components: the forest is complete.
// For the row blocks: the forest of (forest(A) u B) is the forest of A u B -- an edge of A outside forest(A) is the
// weakest of a cycle inside A and stays so in A u B.
// Why it ends.  Every component that a candidate leaves selects an edge and is hooked to another one, so the live
// components at least halve per round: a block runs at most ceil(log2 n) rounds that merge and one that finds nothing.
// find_root / hook_roots end as in hg_cluster.hip (roots only move to smaller indices).
//
// Cross-workgroup traffic inside one launch: the atomic max / min of the two passes, the two counters of select, the
// union-find of hook and the ancestor walks of compress (agent-scope relaxed atomics).  Everything else is read behind a
// launch boundary.  Many candidates between two large components meet in two words; they are not pre-reduced per wave
// (not measured: tools/cluster_tree_bench.py).
#include <algorithm>
#include <cstring>

#include "hg_cluster_common.h"
#include "hg_internal.h"

namespace {
constexpr uint64_t TR_DEFAULT_ROUNDS = 4;  // rounds queued per readback of the count of selecting roots
constexpr uint64_t TR_NONE = ~0ull;        // best_pair: no selection

struct Tree {
  uint64_t *best_pair;    // n: lo << 32 | hi of the strongest edge leaving the component rooted here, TR_NONE = none
  uint32_t *comp;         // n: component root, fully compressed between rounds
  uint32_t *best_ani;     // n: ANI key of that edge, 0 = none
  hg_ani_hit *forest[2];  // n - 1 edges each: the carried forest and the one being written
  int cur;                // forest[cur][0, n_forest) is the carried forest
  size_t n_forest;
  uint32_t *res;          // the ctx's clustering result words (HG_CLU_*)
  uint32_t round;         // rounds queued so far in this call
};

// candidate h of the two ranges (which of them counts: hit_edge, hg_cluster_common.h)
__device__ __forceinline__ hg_ani_hit tree_candidate(const hg_ani_hit *__restrict__ a, size_t na, const hg_ani_hit *__restrict__ b, size_t h) {
  return h < na ? a[h] : b[h - na];
}

// call / block entry: singleton components, no selection, an empty new forest; prev_word (the selecting roots "of the
// round before" the block's first one) is made non-zero
__global__ __launch_bounds__(256) void tree_init_kernel(uint32_t *__restrict__ comp, uint32_t *__restrict__ best_ani,
                                                        uint64_t *__restrict__ best_pair, uint32_t n, uint32_t *__restrict__ res,
                                                        uint32_t prev_parity, uint32_t clear_all) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    comp[i] = (uint32_t)i, best_ani[i] = 0u, best_pair[i] = TR_NONE;
  if (blockIdx.x == 0) {
    if (clear_all && threadIdx.x < HG_CLU_WORDS) res[threadIdx.x] = 0u;
    if (!clear_all && threadIdx.x == 0) res[HG_CLU_SELECTING + prev_parity] = 1u, res[HG_CLU_EDGES] = 0u;
  }
}

// One lane per candidate, grid-stride.  res[HG_CLU_SELECTING + parity]: the count of the previous round is read (0: the
// block is resolved, nothing to do), the one of this round is cleared for tree_select_kernel behind the launch boundary.
__global__ __launch_bounds__(256) void tree_best_ani_kernel(const hg_ani_hit *__restrict__ a, size_t na, const hg_ani_hit *__restrict__ b,
                                                            size_t nb, uint32_t n, float ani_th, const uint32_t *__restrict__ comp,
                                                            uint32_t *best_ani, uint32_t *res, uint32_t round) {
  const uint32_t left = res[HG_CLU_SELECTING + ((round - 1u) & 1u)];
  if (blockIdx.x == 0 && threadIdx.x == 0) res[HG_CLU_SELECTING + (round & 1u)] = 0u;
  if (left == 0u) return;
  const size_t stride = (size_t)gridDim.x * blockDim.x, total = na + nb;
  for (size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x; h < total; h += stride) {
    const hg_ani_hit e = tree_candidate(a, na, b, h);
    uint32_t lo, hi;
    if (!hit_edge(e, n, ani_th, res + HG_CLU_ERR, &lo, &hi)) continue;
    const uint32_t key = ani_key(e.ani);
    const uint32_t cl = comp[lo], ch = comp[hi];
    if (cl == ch) continue;
    (void)__hip_atomic_fetch_max(best_ani + cl, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_max(best_ani + ch, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The same candidates; best_ani[] is final (behind a launch boundary).
__global__ __launch_bounds__(256) void tree_best_pair_kernel(const hg_ani_hit *__restrict__ a, size_t na, const hg_ani_hit *__restrict__ b,
                                                             size_t nb, uint32_t n, float ani_th, const uint32_t *__restrict__ comp,
                                                             const uint32_t *__restrict__ best_ani, uint64_t *best_pair,
                                                             const uint32_t *__restrict__ res, uint32_t round) {
  if (res[HG_CLU_SELECTING + ((round - 1u) & 1u)] == 0u) return;  // (uniform over the grid: nobody writes that word in this launch)
  const size_t stride = (size_t)gridDim.x * blockDim.x, total = na + nb;
  for (size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x; h < total; h += stride) {
    const hg_ani_hit e = tree_candidate(a, na, b, h);
    uint32_t lo, hi;
    if (!hit_edge(e, n, ani_th, nullptr, &lo, &hi)) continue;
    const uint32_t key = ani_key(e.ani);
    const uint32_t cl = comp[lo], ch = comp[hi];
    if (cl == ch) continue;
    const uint64_t pair = (uint64_t)lo << 32 | hi;
    if (best_ani[cl] == key) (void)__hip_atomic_fetch_min(best_pair + cl, pair, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (best_ani[ch] == key) (void)__hip_atomic_fetch_min(best_pair + ch, pair, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One lane per node; only a root has a selection.  Everything it reads was written behind a launch boundary.
__global__ __launch_bounds__(256) void tree_select_kernel(const uint32_t *__restrict__ comp, const uint32_t *__restrict__ best_ani,
                                                          const uint64_t *__restrict__ best_pair, uint32_t n,
                                                          hg_ani_hit *__restrict__ forest, uint32_t forest_cap, uint32_t *res,
                                                          uint32_t round) {
  if (res[HG_CLU_SELECTING + ((round - 1u) & 1u)] == 0u) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  bool selects = false, emits = false;
  uint32_t lo = 0, hi = 0, key = 0;
  if (i < n) {
    const uint64_t pair = best_pair[i];
    if (pair != TR_NONE) {
      selects = true;
      lo = (uint32_t)(pair >> 32), hi = (uint32_t)pair, key = best_ani[i];
      const uint32_t cl = comp[lo], other = cl == (uint32_t)i ? comp[hi] : cl;
      const bool mutual = best_pair[other] == pair && best_ani[other] == key;
      emits = !mutual || (uint32_t)i < other;
    }
  }
  const unsigned long long sel = __ballot(selects), emi = __ballot(emits);
  if (sel == 0ull) return;
  const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint32_t base = 0;
  if (lane == 0) {
    (void)__hip_atomic_fetch_add(res + HG_CLU_SELECTING + (round & 1u), (uint32_t)__popcll(sel), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (emi) base = __hip_atomic_fetch_add(res + HG_CLU_EDGES, (uint32_t)__popcll(emi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  base = __shfl(base, 0);
  const uint32_t pos = base + (uint32_t)__popcll(emi & lt);
  if (emits && pos < forest_cap) forest[pos] = hg_ani_hit{lo, hi, key_ani(key)};  // (a forest has at most n - 1 edges: the test only keeps the store in range)
}

// One lane per node: the selected edges united.  comp[] moves under the lanes' feet (hg_cluster_common.h).
__global__ __launch_bounds__(256) void tree_hook_kernel(uint32_t *comp, const uint64_t *__restrict__ best_pair, uint32_t n,
                                                        const uint32_t *__restrict__ res, uint32_t round) {
  if (res[HG_CLU_SELECTING + ((round - 1u) & 1u)] == 0u) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t pair = best_pair[i];
  if (pair != TR_NONE) hook_roots(comp, (uint32_t)(pair >> 32), (uint32_t)pair);
}

// comp[i] = root(i) (roots do not change here and every other entry only moves to an ancestor, so whatever value a lane
// reads is a valid step towards the root); the best words cleared; the round counted.
__global__ __launch_bounds__(256) void tree_compress_kernel(uint32_t *comp, uint32_t *__restrict__ best_ani, uint64_t *__restrict__ best_pair,
                                                            uint32_t n, uint32_t *res, uint32_t round) {
  if (res[HG_CLU_SELECTING + ((round - 1u) & 1u)] == 0u) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    uint32_t r = rep_load(comp, (uint32_t)i);
    if (r != (uint32_t)i) {
      for (uint32_t p = rep_load(comp, r); p != r; p = rep_load(comp, r)) r = p;
      rep_store(comp, (uint32_t)i, r);
    }
    best_ani[i] = 0u, best_pair[i] = TR_NONE;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) res[HG_CLU_ROUNDS] += 1u;  // (this lane alone touches the word in this launch)
}

hg_status tree_queue_init(hg_ctx *c, Tree *g, size_t n, bool clear_all) {
  hipLaunchKernelGGL(tree_init_kernel, dim3(grid_for(c, n)), dim3(256), 0, c->stream, g->comp, g->best_ani, g->best_pair, (uint32_t)n,
                     g->res, g->round & 1u, clear_all ? 1u : 0u);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

hg_status tree_begin(hg_ctx *c, size_t n, Tree *g) {
  hg_status s;
  if ((s = hg_cluster_res(c, &g->res)) != HG_OK) return s;
  const size_t fe = n - 1;  // (n >= 1)
  if ((s = hg_ensure(c, c->w_tree, n * 16 + 2 * fe * sizeof(hg_ani_hit) + 64)) != HG_OK) return s;
  g->best_pair = static_cast<uint64_t *>(c->w_tree.p);
  g->comp = reinterpret_cast<uint32_t *>(g->best_pair + n);
  g->best_ani = g->comp + n;
  g->forest[0] = reinterpret_cast<hg_ani_hit *>(g->best_ani + n);
  g->forest[1] = g->forest[0] + fe;
  g->cur = 0, g->n_forest = 0, g->round = 0;
  c->tree_rounds = 0;
  return tree_queue_init(c, g, n, true);
}

// the result words back and cleared; a set error word fails the call
hg_status tree_close(hg_ctx *c, Tree *g, size_t *count) {
  return hg_cluster_close(c, g->res, &c->tree_rounds, "hg_cluster_tree_hits_dev", count);
}

// The forest of (carried forest u d_hits[0, n_hits)), from singleton components, into the other forest buffer, which
// then is the carried one.
hg_status tree_block(hg_ctx *c, Tree *g, const hg_ani_hit *d_hits, size_t n_hits, size_t n, float ani_th) {
  hg_status s;
  if ((s = tree_queue_init(c, g, n, false)) != HG_OK) return s;
  const uint32_t m = (uint32_t)n;
  const hg_ani_hit *a = g->forest[g->cur];
  hg_ani_hit *out = g->forest[g->cur ^ 1];
  const size_t na = g->n_forest;
  const uint64_t per = c->dbg_tree_rounds ? c->dbg_tree_rounds : TR_DEFAULT_ROUNDS;
  const unsigned edge_grid = grid_for(c, na + n_hits), node_grid = (unsigned)((n + 255) / 256);
  const uint32_t *h_res = nullptr;
  for (;;) {
    for (uint64_t k = 0; k < per; ++k) {
      ++g->round;
      hipLaunchKernelGGL(tree_best_ani_kernel, dim3(edge_grid), dim3(256), 0, c->stream, a, na, d_hits, n_hits, m, ani_th, g->comp,
                         g->best_ani, g->res, g->round);
      HG_HIP(c, hipGetLastError());
      hipLaunchKernelGGL(tree_best_pair_kernel, dim3(edge_grid), dim3(256), 0, c->stream, a, na, d_hits, n_hits, m, ani_th, g->comp,
                         g->best_ani, g->best_pair, g->res, g->round);
      HG_HIP(c, hipGetLastError());
      hipLaunchKernelGGL(tree_select_kernel, dim3(node_grid), dim3(256), 0, c->stream, g->comp, g->best_ani, g->best_pair, m, out,
                         (uint32_t)(n - 1), g->res, g->round);
      HG_HIP(c, hipGetLastError());
      hipLaunchKernelGGL(tree_hook_kernel, dim3(node_grid), dim3(256), 0, c->stream, g->comp, g->best_pair, m, g->res, g->round);
      HG_HIP(c, hipGetLastError());
      hipLaunchKernelGGL(tree_compress_kernel, dim3(node_grid), dim3(256), 0, c->stream, g->comp, g->best_ani, g->best_pair, m, g->res,
                         g->round);
      HG_HIP(c, hipGetLastError());
    }
    if ((s = hg_publish_words(c, g->res, HG_CLU_WORDS, &h_res)) != HG_OK) return s;  // (nothing cleared: the call goes on)
    if (h_res[HG_CLU_SELECTING + (g->round & 1u)] == 0u) break;
  }
  if (h_res[HG_CLU_ERR]) {  // (seen without clearing: close the call, which fails it)
    size_t count;
    return tree_close(c, g, &count);
  }
  g->n_forest = std::min<size_t>(h_res[HG_CLU_EDGES], n - 1);
  g->cur ^= 1;
  return HG_OK;
}

hg_status tree_end(hg_ctx *c, Tree *g, size_t n, hg_ani_hit *d_tree, size_t *n_edges, uint32_t *d_rep, uint32_t *d_cluster,
                   size_t *n_clusters) {
  hg_status s;
  if ((s = hg_sort_tree_edges_dev(c, g->forest[g->cur], g->n_forest, n, d_tree)) != HG_OK) return s;
  if (d_rep) {
    HG_HIP(c, hipMemcpyAsync(d_rep, g->comp, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    if ((s = hg_cluster_queue_ids(c, d_rep, n, d_cluster, g->res)) != HG_OK) return s;
  }
  size_t count = 0;
  if ((s = tree_close(c, g, &count)) != HG_OK) return s;  // (no error word here: tree_block saw to it)
  *n_edges = g->n_forest;
  *n_clusters = d_rep ? count : n - g->n_forest;
  return HG_OK;
}

// the checks every form shares (the tree's own around hg_cluster_check); *done: the call is answered (n == 0, or an error)
hg_status check_args(hg_ctx *c, size_t n, const hg_ani_hit *tree, size_t tree_cap, size_t *n_edges, const uint32_t *rep,
                     const uint32_t *cluster, size_t *n_clusters, bool dist_form, bool *done) {
  *done = true;
  if (!n_edges || !n_clusters) return hg_fail(c, HG_ERR_INVALID, "n_edges == NULL or n_clusters == NULL");
  *n_edges = 0;
  const hg_status s = hg_cluster_check(c, n, n_clusters, dist_form);
  if (s != HG_OK || n == 0) return s;
  if (!tree) return hg_fail(c, HG_ERR_INVALID, "NULL tree array");
  if ((rep == nullptr) != (cluster == nullptr)) return hg_fail(c, HG_ERR_INVALID, "rep and cluster: both or neither");
  if (tree_cap < n - 1) {
    *n_edges = n - 1;
    return hg_fail(c, HG_ERR_CAPACITY, "tree_cap < n - 1");
  }
  *done = false;
  return HG_OK;
}
}  // namespace

extern "C" uint64_t hg_ctx_cluster_tree_rounds(const hg_ctx *c) { return c ? c->tree_rounds : 0; }

extern "C" hg_status hg_cluster_tree_hits_dev(hg_ctx *c, size_t n, const hg_ani_hit *d_hits, size_t n_hits, float ani_th,
                                              hg_ani_hit *d_tree, size_t tree_cap, size_t *n_edges, uint32_t *d_rep,
                                              uint32_t *d_cluster, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  bool done;
  hg_status s = check_args(c, n, d_tree, tree_cap, n_edges, d_rep, d_cluster, n_clusters, false, &done);
  if (done) return s;
  if (n_hits && !d_hits) return hg_fail(c, HG_ERR_INVALID, "NULL hit list");
  HG_ENTER(c);
  Tree g{};
  if ((s = tree_begin(c, n, &g)) != HG_OK) return s;
  if (n_hits && (s = tree_block(c, &g, d_hits, n_hits, n, ani_th)) != HG_OK) return s;  // the list is one block
  return tree_end(c, &g, n, d_tree, n_edges, d_rep, d_cluster, n_clusters);
}

extern "C" hg_status hg_cluster_tree_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d,
                                         uint32_t ksize, float ani_th, hg_ani_hit *d_tree, size_t tree_cap, size_t *n_edges,
                                         uint32_t *d_rep, uint32_t *d_cluster, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  bool done;
  hg_status s = check_args(c, n, d_tree, tree_cap, n_edges, d_rep, d_cluster, n_clusters, true, &done);
  if (done) return s;
  if (!d_hv || !d_norm2) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  Tree g{};
  if ((s = tree_begin(c, n, &g)) != HG_OK) return s;
  // A row block's candidates are the carried forest and its hits; a block without hits leaves the forest as it is.
  s = hg_cluster_row_blocks(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, false, nullptr,
                            [&](const hg_ani_hit *d_hits, size_t got, size_t, size_t) {
                              return got ? tree_block(c, &g, d_hits, got, n, ani_th) : HG_OK;
                            });
  if (s != HG_OK) return s;
  return tree_end(c, &g, n, d_tree, n_edges, d_rep, d_cluster, n_clusters);
}

extern "C" hg_status hg_cluster_tree(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                     float ani_th, hg_ani_hit *tree, size_t tree_cap, size_t *n_edges, uint32_t *rep,
                                     uint32_t *cluster, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  bool done;
  hg_status s = check_args(c, n, tree, tree_cap, n_edges, rep, cluster, n_clusters, true, &done);
  if (done) return s;
  if (!hv || !norm2) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  const int16_t *d_hv;
  const int32_t *d_norm2;
  uint32_t *d_rep;
  if ((s = hg_cluster_stage(c, hv, norm2, n, hv_d, 2 * n * sizeof(uint32_t) + (n - 1) * sizeof(hg_ani_hit), &d_hv, &d_norm2, &d_rep)) != HG_OK)
    return s;
  uint32_t *d_cluster = d_rep + n;
  auto *d_tree = reinterpret_cast<hg_ani_hit *>(d_cluster + n);
  if ((s = hg_cluster_tree_dev(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, d_tree, n - 1, n_edges, rep ? d_rep : nullptr,
                               rep ? d_cluster : nullptr, n_clusters)) != HG_OK)
    return s;
  if (*n_edges) HG_HIP(c, hipMemcpyAsync(tree, d_tree, *n_edges * sizeof(hg_ani_hit), hipMemcpyDeviceToHost, c->stream));
  if (rep) {
    HG_HIP(c, hipMemcpyAsync(rep, d_rep, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HG_HIP(c, hipMemcpyAsync(cluster, d_cluster, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  }
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}
