// hg_cluster.hip -- single-linkage clustering of sketches at an ANI threshold (an extension: the reference has no such step;
// its users cluster the TSV of `dist` in another tool).  Two genomes share a cluster when a chain of pairs with ani >= ani_th
// joins them; rep[i] = the smallest index of i's connected component, cluster[i] = the component's dense id in increasing
// order of rep.
//   * hook    : one lane per hit, lock-free union-find over rep[n] (ECL-CC, Jaykrishnan & Burtscher 2018; the routines
//               are in hg_cluster_common.h, which hg_cluster_tree.hip shares): find both roots
//               with path halving, hook the larger root under the smaller one with a CAS, on failure go on from what the CAS
//               returned.  Roots only ever move to smaller indices, so the root of a component is its minimum index.
//   * finish  : compress (rep[i] = root(i)) + roots per tile -> scan of the tile counts (cluster count) -> dense ids of the
//               roots -> ids of the other members, separate launches: each launch boundary publishes the previous one.
// The file also holds the host parts every scheme is built from (declared in hg_cluster_common.h): the argument check, the
// staging of the host forms, the row-block driver of the symmetric comparison, the rep / ani launch of the representative
// schemes, the finishing launches and the closing readback.
#include <algorithm>

#include "hg_block_scan.h"
#include "hg_cluster_common.h"
#include "hg_internal.h"

namespace {
constexpr uint32_t CL_ITEMS = 4, CL_TILE = 256 * CL_ITEMS;  // nodes per workgroup of the finishing kernels

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
    if (hit_counts(e, n, ani_th, err)) hook_roots(rep, e.ref_idx, e.qry_idx);
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

// rep / ani of the representative schemes: a representative is its own, at 100; a member has its best word's
__global__ __launch_bounds__(256) void cluster_rep_ani_kernel(const uint64_t *__restrict__ best, const uint32_t *__restrict__ status,
                                                              uint32_t n, uint32_t *__restrict__ rep, float *__restrict__ ani) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t b = best[i];
    const bool is_rep = status[i] != ST_MEMBER || b == 0ull;  // (a member always has a best word: the second test only keeps rep[] in range)
    uint32_t r;
    float a;
    best_unpack(b, &r, &a);
    rep[i] = is_rep ? (uint32_t)i : r;
    if (ani) ani[i] = is_rep ? 100.0f : a;
  }
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

hg_status check_n(hg_ctx *c, size_t n, const uint32_t *d_rep) {
  if (n > 0xFFFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "n must be < 2^32 (indices are uint32)");
  if (n && !d_rep) return hg_fail(c, HG_ERR_INVALID, "NULL rep array");
  return HG_OK;
}
}  // namespace

// the ctx's result words (HG_CLU_*: hg_cluster_common.h), zeroed when they are first allocated
hg_status hg_cluster_res(hg_ctx *c, uint32_t **out) {
  const bool fresh = c->w_clu_res.p == nullptr;
  hg_status s = hg_ensure(c, c->w_clu_res, 64);
  if (s != HG_OK) return s;
  *out = static_cast<uint32_t *>(c->w_clu_res.p);
  if (fresh) HG_HIP(c, hipMemsetAsync(*out, 0, 64, c->stream));
  return HG_OK;
}

hg_status hg_cluster_check(hg_ctx *c, size_t n, size_t *n_clusters, bool dist_form) {
  if (!n_clusters) return hg_fail(c, HG_ERR_INVALID, "n_clusters == NULL");
  *n_clusters = 0;
  if (n > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "n must be < 2^31");
  if (dist_form && c->ani_metric == HG_ANI_CONTAINMENT)  // (the graph is undirected: HG_ANI_MASH or HG_ANI_MAX_CONTAINMENT)
    return hg_fail(c, HG_ERR_INVALID, "clustering needs a symmetric ANI metric: HG_ANI_CONTAINMENT is directional");
  return HG_OK;
}

hg_status hg_cluster_stage(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, size_t out_bytes,
                           const int16_t **d_hv, const int32_t **d_norm2, uint32_t **d_out) {
  hg_status s;
  const size_t hb = n * (size_t)hv_d * sizeof(int16_t);
  if ((s = hg_ensure(c, c->w_hv, hb + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_n2a, n * sizeof(int32_t) + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_ani, out_bytes + 64)) != HG_OK) return s;
  HG_HIP(c, hipMemcpyAsync(c->w_hv.p, hv, hb, hipMemcpyHostToDevice, c->stream));
  HG_HIP(c, hipMemcpyAsync(c->w_n2a.p, norm2, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  *d_hv = static_cast<const int16_t *>(c->w_hv.p), *d_norm2 = static_cast<const int32_t *>(c->w_n2a.p);
  *d_out = static_cast<uint32_t *>(c->w_ani.p);
  return HG_OK;
}

// (the append mode's limit, and hg_cluster_setcover_hits_dev's for a caller's list: set cover is the scheme that holds a whole list)
hg_status hg_cluster_list_too_long(hg_ctx *c) {
  return hg_fail(c, HG_ERR_UNSUPPORTED,
                 "the hit list of the set-cover resolution does not fit (2^32 - 1 hits or more): a higher threshold would");
}

// (the contract: hg_cluster_common.h)  The lower triangle is never enumerated, and in the reuse mode the whole matrix's
// hits are never held at once.  A block within hg_pair_limit pairs is one launch of hg_dist_block_dev; a capacity retry
// means that the block ran to its end and counted every hit.
hg_status hg_cluster_row_blocks(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                float ani_th, bool append, size_t *total, const hg_cluster_block_fn &block) {
  hg_status s;
  const uint64_t pair_limit = hg_pair_limit(c);
  const uint64_t pairs = (uint64_t)n * (n ? n - 1 : 0) / 2;
  size_t cap = c->dbg_cluster_hit_cap ? (size_t)c->dbg_cluster_hit_cap
                                      : std::max(c->w_clu_hits.cap / sizeof(hg_ani_hit), (size_t)std::min<uint64_t>(pairs, HG_CLU_DEFAULT_HITS));
  if ((s = hg_ensure(c, c->w_clu_hits, std::max<size_t>(cap, 1) * sizeof(hg_ani_hit))) != HG_OK) return s;
  size_t held = 0;  // append: the hits of the blocks before this one
  for (size_t r0 = 0; r0 < n;) {
    const size_t cols = n - r0, rows = (size_t)std::min<uint64_t>(cols, std::max<uint64_t>(1, pair_limit / cols));
    size_t got = 0;
    while (cols > 1) {
      s = hg_dist_block_dev(c, d_hv + r0 * (size_t)hv_d, d_norm2 + r0, rows, r0, d_hv + r0 * (size_t)hv_d, d_norm2 + r0, cols, r0,
                            hv_d, ksize, 1, ani_th, static_cast<hg_ani_hit *>(c->w_clu_hits.p) + held, cap - held, &got);
      if (s == HG_OK) break;
      if (s != HG_ERR_CAPACITY) return s;
      if (append) {
        if ((uint64_t)held + got > HG_CLU_MAX_LIST) return hg_cluster_list_too_long(c);
        if ((s = grow_list(c, held, held + got)) != HG_OK) return s;
        cap = c->w_clu_hits.cap / sizeof(hg_ani_hit);  // (with the slack hg_ensure adds: the blocks that follow grow it less often)
      } else {
        cap = got;
        if ((s = hg_ensure(c, c->w_clu_hits, cap * sizeof(hg_ani_hit))) != HG_OK) return s;
      }
    }
    if ((s = block(static_cast<const hg_ani_hit *>(c->w_clu_hits.p) + held, got, r0, r0 + rows)) != HG_OK) return s;
    if (append) {
      held += got;
      if ((uint64_t)held > HG_CLU_MAX_LIST) return hg_cluster_list_too_long(c);
    }
    r0 += rows;
  }
  if (total) *total = held;
  return HG_OK;
}

hg_status hg_cluster_queue_rep_ani(hg_ctx *c, const uint64_t *best, const uint32_t *status, size_t n, uint32_t *d_rep, float *d_ani) {
  hipLaunchKernelGGL(cluster_rep_ani_kernel, dim3(grid_for(c, n)), dim3(256), 0, c->stream, best, status, (uint32_t)n, d_rep, d_ani);
  HG_HIP(c, hipGetLastError());
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

hg_status hg_cluster_close(hg_ctx *c, uint32_t *res, uint64_t *rounds, const char *hits_fn, size_t *count) {
  const uint32_t *h_res = nullptr;
  const hg_status s = hg_publish_words(c, res, HG_CLU_WORDS, &h_res, HG_CLU_WORDS);
  if (s != HG_OK) return s;
  *rounds = h_res[HG_CLU_ROUNDS];
  if (h_res[HG_CLU_ERR]) return hg_fail(c, HG_ERR_INVALID, std::string("a hit given to ") + hits_fn + " had an index >= n");
  *count = h_res[HG_CLU_COUNT];
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
  hg_status s = hg_cluster_check(c, n, n_clusters, true);
  if (s != HG_OK) return s;
  if (n && (!d_hv || !d_norm2 || !d_rep || !d_cluster)) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  if ((s = hg_cluster_init_dev(c, d_rep, n)) != HG_OK) return s;
  // each block's hits are unioned before the next block reuses the list
  s = hg_cluster_row_blocks(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, false, nullptr,
                            [&](const hg_ani_hit *d_hits, size_t got, size_t, size_t) {
                              return hg_cluster_add_hits_dev(c, d_rep, n, d_hits, got, ani_th);
                            });
  if (s != HG_OK) return s;
  return hg_cluster_finish_dev(c, d_rep, n, d_cluster, n_clusters);
}

extern "C" hg_status hg_cluster(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                float ani_th, uint32_t *rep, uint32_t *cluster, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_cluster_check(c, n, n_clusters, true);
  if (s != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!hv || !norm2 || !rep || !cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  const int16_t *d_hv;
  const int32_t *d_norm2;
  uint32_t *d_rep;
  if ((s = hg_cluster_stage(c, hv, norm2, n, hv_d, 2 * n * sizeof(uint32_t), &d_hv, &d_norm2, &d_rep)) != HG_OK) return s;
  uint32_t *d_cluster = d_rep + n;
  if ((s = hg_cluster_dev(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, d_rep, d_cluster, n_clusters)) != HG_OK) return s;
  HG_HIP(c, hipMemcpyAsync(rep, d_rep, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(cluster, d_cluster, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}
