// hg_cluster.hip -- single-linkage clustering of sketches at an ANI threshold (an extension: the reference has no such step;
// its users cluster the TSV of `dist` in another tool).  Two genomes share a cluster when a chain of pairs with ani >= ani_th
// joins them; rep[i] = the smallest index of i's connected component, cluster[i] = the component's dense id in increasing
// order of rep.
//   * hook    : one lane per hit, lock-free union-find over rep[n] (ECL-CC, Jaykrishnan & Burtscher 2018; the routines
//               are in hg_cluster_common.h, which hg_cluster_greedy.hip and hg_cluster_tree.hip share): find both roots
//               with path halving, hook the larger root under the smaller one with a CAS, on failure go on from what the CAS
//               returned.  Roots only ever move to smaller indices, so the root of a component is its minimum index.
//   * finish  : compress (rep[i] = root(i)) + roots per tile -> scan of the tile counts (cluster count) -> dense ids of the
//               roots -> ids of the other members, separate launches: each launch boundary publishes the previous one.
#include <algorithm>

#include "hg_block_scan.h"
#include "hg_cluster_common.h"
#include "hg_internal.h"

namespace {
constexpr uint32_t CL_ITEMS = 4, CL_TILE = 256 * CL_ITEMS;  // nodes per workgroup of the finishing kernels
constexpr size_t CL_DEFAULT_HITS = (size_t)1 << 22;         // first size of hg_cluster_dev's scratch hit list (48 MB)

__global__ __launch_bounds__(256) void cluster_init_kernel(uint32_t *__restrict__ rep, uint32_t n, uint32_t *__restrict__ res) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) rep[i] = (uint32_t)i;
  if (blockIdx.x == 0 && threadIdx.x < 2) res[threadIdx.x] = 0u;  // cluster count, error word
}

// One lane per hit, grid-stride (find_root, hook_roots and why they terminate: hg_cluster_common.h).
__global__ __launch_bounds__(256) void cluster_hook_kernel(uint32_t *rep, uint32_t n, const hg_ani_hit *__restrict__ hits,
                                                           size_t n_hits, float ani_th, uint32_t *err) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x; h < n_hits; h += stride) {
    const hg_ani_hit e = hits[h];
    if (e.ref_idx >= n || e.qry_idx >= n) {
      __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    if (!(e.ani >= ani_th) || e.ref_idx == e.qry_idx) continue;  // (the side of the threshold exactly as in dist)
    hook_roots(rep, e.ref_idx, e.qry_idx);
  }
}

// rep[i] = root(i), and the roots of each tile of CL_TILE nodes counted.  Roots do not change here and every other entry
// only moves to an ancestor, so whatever value a lane reads is a valid step towards the root.
__global__ __launch_bounds__(256) void cluster_compress_kernel(uint32_t *rep, uint32_t n, uint32_t *__restrict__ tile_cnt) {
  __shared__ uint32_t s_wave[4];
  const size_t base = (size_t)blockIdx.x * CL_TILE;
  uint32_t roots = 0;
#pragma unroll
  for (uint32_t j = 0; j < CL_ITEMS; ++j) {
    const size_t i = base + j * 256 + threadIdx.x;
    if (i >= n) continue;
    uint32_t r = rep_load(rep, (uint32_t)i);
    if (r == (uint32_t)i) {
      ++roots;
      continue;
    }
    for (uint32_t p = rep_load(rep, r); p != r; p = rep_load(rep, r)) r = p;
    rep_store(rep, (uint32_t)i, r);
  }
  uint32_t total;
  (void)block_excl_scan<4>(roots, s_wave, &total);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// one workgroup: exclusive prefix of the tile counts (in place); res[0] = number of clusters
__global__ __launch_bounds__(256) void cluster_scan_tiles_kernel(uint32_t *__restrict__ tile_cnt, uint32_t n_tiles,
                                                                 uint32_t *__restrict__ res) {
  __shared__ uint32_t s_wave[4];
  uint32_t running = 0;
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += 256) {
    const uint32_t t = t0 + threadIdx.x, v = t < n_tiles ? tile_cnt[t] : 0u;
    uint32_t tot;
    const uint32_t ex = block_excl_scan<4>(v, s_wave, &tot);
    if (t < n_tiles) tile_cnt[t] = running + ex;
    running += tot;
  }
  if (threadIdx.x == 0) res[0] = running;
}

// cluster[r] = dense id of every root r: the roots before it in index order
__global__ __launch_bounds__(256) void cluster_root_ids_kernel(const uint32_t *__restrict__ rep, uint32_t n,
                                                               const uint32_t *__restrict__ tile_pre, uint32_t *__restrict__ cluster) {
  __shared__ uint32_t s_wave[4];
  const size_t base = (size_t)blockIdx.x * CL_TILE;
  uint32_t run = tile_pre[blockIdx.x];
#pragma unroll
  for (uint32_t j = 0; j < CL_ITEMS; ++j) {
    const size_t i = base + j * 256 + threadIdx.x;
    const uint32_t root = i < n && rep[i] == (uint32_t)i;
    uint32_t tot;
    const uint32_t ex = block_excl_scan<4>(root, s_wave, &tot);
    if (root) cluster[i] = run + ex;
    run += tot;
  }
}

// the other members take their root's id (the roots' entries are final: written by the previous launch, not touched here)
__global__ __launch_bounds__(256) void cluster_member_ids_kernel(const uint32_t *__restrict__ rep, uint32_t n, uint32_t *cluster) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t r = rep[i];
    if (r != (uint32_t)i) cluster[i] = cluster[r];
  }
}

hg_status check_n(hg_ctx *c, size_t n, const uint32_t *d_rep) {
  if (n > 0xFFFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "n must be < 2^32 (indices are uint32)");
  if (n && !d_rep) return hg_fail(c, HG_ERR_INVALID, "NULL rep array");
  return HG_OK;
}
}  // namespace

// the ctx's result block: [0] cluster count, [1] error word (an index >= n was given to hg_cluster_add_hits_dev or
// hg_cluster_greedy_hits_dev); hg_cluster_greedy.hip keeps its round words behind them (hg_internal.h)
hg_status hg_cluster_res(hg_ctx *c, uint32_t **out) {
  const bool fresh = c->w_clu_res.p == nullptr;
  hg_status s = hg_ensure(c, c->w_clu_res, 64);
  if (s != HG_OK) return s;
  *out = static_cast<uint32_t *>(c->w_clu_res.p);
  if (fresh) HG_HIP(c, hipMemsetAsync(*out, 0, 64, c->stream));
  return HG_OK;
}

// The finishing launches on a rep[] whose trees may have any depth (the greedy resolution's have depth 1): compress + roots
// per tile, scan (res[0] = cluster count), dense ids of the roots, ids of the other members.  Stream-ordered.
hg_status hg_cluster_queue_ids(hg_ctx *c, uint32_t *d_rep, size_t n, uint32_t *d_cluster, uint32_t *res) {
  hg_status s;
  const size_t n_tiles = (n + CL_TILE - 1) / CL_TILE;
  if ((s = hg_ensure(c, c->w_clu, n_tiles * sizeof(uint32_t) + 64)) != HG_OK) return s;
  auto *tiles = static_cast<uint32_t *>(c->w_clu.p);
  const uint32_t m = (uint32_t)n;
  if (n_tiles) {
    hipLaunchKernelGGL(cluster_compress_kernel, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, d_rep, m, tiles);
    HG_HIP(c, hipGetLastError());
  }
  hipLaunchKernelGGL(cluster_scan_tiles_kernel, dim3(1), dim3(256), 0, c->stream, tiles, (uint32_t)n_tiles, res);
  HG_HIP(c, hipGetLastError());
  if (n_tiles) {
    hipLaunchKernelGGL(cluster_root_ids_kernel, dim3((unsigned)n_tiles), dim3(256), 0, c->stream, d_rep, m, tiles, d_cluster);
    HG_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(cluster_member_ids_kernel, dim3(grid_for(c, n)), dim3(256), 0, c->stream, d_rep, m, d_cluster);
    HG_HIP(c, hipGetLastError());
  }
  return HG_OK;
}

extern "C" hg_status hg_cluster_init_dev(hg_ctx *c, uint32_t *d_rep, size_t n) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_n(c, n, d_rep);
  if (s != HG_OK) return s;
  HG_ENTER(c);
  uint32_t *res;
  if ((s = hg_cluster_res(c, &res)) != HG_OK) return s;
  hipLaunchKernelGGL(cluster_init_kernel, dim3(grid_for(c, n)), dim3(256), 0, c->stream, d_rep, (uint32_t)n, res);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

extern "C" hg_status hg_cluster_add_hits_dev(hg_ctx *c, uint32_t *d_rep, size_t n, const hg_ani_hit *d_hits, size_t n_hits,
                                             float ani_th) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_n(c, n, d_rep);
  if (s != HG_OK) return s;
  if (n_hits == 0) return HG_OK;
  if (!d_hits) return hg_fail(c, HG_ERR_INVALID, "NULL hit list");
  HG_ENTER(c);
  uint32_t *res;
  if ((s = hg_cluster_res(c, &res)) != HG_OK) return s;
  hipLaunchKernelGGL(cluster_hook_kernel, dim3(grid_for(c, n_hits)), dim3(256), 0, c->stream, d_rep, (uint32_t)n, d_hits, n_hits,
                     ani_th, res + 1);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

extern "C" hg_status hg_cluster_finish_dev(hg_ctx *c, uint32_t *d_rep, size_t n, uint32_t *d_cluster, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  if (!n_clusters) return hg_fail(c, HG_ERR_INVALID, "n_clusters == NULL");
  *n_clusters = 0;
  hg_status s = check_n(c, n, d_rep);
  if (s != HG_OK) return s;
  if (n && !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL cluster array");
  HG_ENTER(c);
  uint32_t *res;
  if ((s = hg_cluster_res(c, &res)) != HG_OK) return s;
  if ((s = hg_cluster_queue_ids(c, d_rep, n, d_cluster, res)) != HG_OK) return s;
  // (the publishing kernel clears both words behind its copy: the next clustering on this ctx starts clean)
  const uint32_t *h_res = nullptr;
  if ((s = hg_publish_words(c, res, 2, &h_res, 2)) != HG_OK) return s;
  if (h_res[1]) return hg_fail(c, HG_ERR_INVALID, "a hit given to hg_cluster_add_hits_dev had an index >= n");
  *n_clusters = h_res[0];
  return HG_OK;
}

extern "C" hg_status hg_cluster_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d,
                                    uint32_t ksize, float ani_th, uint32_t *d_rep, uint32_t *d_cluster, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  if (!n_clusters) return hg_fail(c, HG_ERR_INVALID, "n_clusters == NULL");
  *n_clusters = 0;
  if (n > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "n must be < 2^31");
  if (c->ani_metric == HG_ANI_CONTAINMENT)  // (the graph is undirected: HG_ANI_MASH or HG_ANI_MAX_CONTAINMENT)
    return hg_fail(c, HG_ERR_INVALID, "clustering needs a symmetric ANI metric: HG_ANI_CONTAINMENT is directional");
  if (n && (!d_hv || !d_norm2 || !d_rep || !d_cluster)) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  hg_status s = hg_cluster_init_dev(c, d_rep, n);
  if (s != HG_OK) return s;
  // Symmetric dist over blocks of rows [r0, r0 + rows) x columns [r0, n) (the lower triangle is never enumerated), each
  // block's hits unioned before the next block reuses the scratch list: the whole matrix's hits are never held at once.
  // A block stays within the pairs one launch may count (2^32 - 1, or the "pair_limit" test hook), so
  // hg_dist_block_dev runs it as one launch; when its hits outgrow the scratch list, the list grows to the reported count
  // and the block runs again.
  const uint64_t pair_limit = c->dbg_pair_limit ? c->dbg_pair_limit : 0xFFFFFFFFull;
  const uint64_t pairs = (uint64_t)n * (n ? n - 1 : 0) / 2;
  size_t cap = c->dbg_cluster_hit_cap ? (size_t)c->dbg_cluster_hit_cap
                                      : std::max(c->w_clu_hits.cap / sizeof(hg_ani_hit), (size_t)std::min<uint64_t>(pairs, CL_DEFAULT_HITS));
  if ((s = hg_ensure(c, c->w_clu_hits, std::max<size_t>(cap, 1) * sizeof(hg_ani_hit))) != HG_OK) return s;
  for (size_t r0 = 0; r0 + 1 < n;) {
    const size_t cols = n - r0, rows = (size_t)std::min<uint64_t>(cols, std::max<uint64_t>(1, pair_limit / cols));
    size_t got = 0;
    for (;;) {
      s = hg_dist_block_dev(c, d_hv + r0 * (size_t)hv_d, d_norm2 + r0, rows, r0, d_hv + r0 * (size_t)hv_d, d_norm2 + r0, cols, r0,
                            hv_d, ksize, 1, ani_th, static_cast<hg_ani_hit *>(c->w_clu_hits.p), cap, &got);
      if (s != HG_ERR_CAPACITY) break;
      cap = got;  // (a capacity retry: the block ran to the end and counted every hit)
      if ((s = hg_ensure(c, c->w_clu_hits, cap * sizeof(hg_ani_hit))) != HG_OK) return s;
    }
    if (s != HG_OK) return s;
    if ((s = hg_cluster_add_hits_dev(c, d_rep, n, static_cast<const hg_ani_hit *>(c->w_clu_hits.p), got, ani_th)) != HG_OK) return s;
    r0 += rows;
  }
  return hg_cluster_finish_dev(c, d_rep, n, d_cluster, n_clusters);
}

extern "C" hg_status hg_cluster(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                float ani_th, uint32_t *rep, uint32_t *cluster, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  if (!n_clusters) return hg_fail(c, HG_ERR_INVALID, "n_clusters == NULL");
  *n_clusters = 0;
  if (n > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "n must be < 2^31");
  if (c->ani_metric == HG_ANI_CONTAINMENT)  // (the graph is undirected: HG_ANI_MASH or HG_ANI_MAX_CONTAINMENT)
    return hg_fail(c, HG_ERR_INVALID, "clustering needs a symmetric ANI metric: HG_ANI_CONTAINMENT is directional");
  if (n == 0) return HG_OK;
  if (!hv || !norm2 || !rep || !cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  hg_status s;
  const size_t hb = n * (size_t)hv_d * sizeof(int16_t);
  if ((s = hg_ensure(c, c->w_hv, hb + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_n2a, n * sizeof(int32_t) + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_ani, 2 * n * sizeof(uint32_t) + 64)) != HG_OK) return s;
  HG_HIP(c, hipMemcpyAsync(c->w_hv.p, hv, hb, hipMemcpyHostToDevice, c->stream));
  HG_HIP(c, hipMemcpyAsync(c->w_n2a.p, norm2, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  auto *d_rep = static_cast<uint32_t *>(c->w_ani.p), *d_cluster = d_rep + n;
  if ((s = hg_cluster_dev(c, static_cast<const int16_t *>(c->w_hv.p), static_cast<const int32_t *>(c->w_n2a.p), n, hv_d, ksize, ani_th,
                          d_rep, d_cluster, n_clusters)) != HG_OK)
    return s;
  HG_HIP(c, hipMemcpyAsync(rep, d_rep, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(cluster, d_cluster, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}
