// hg_cluster_stats.hip -- what a clustering looks like from the inside (an extension like the hg_cluster_*.hip files: the
// figures dRep, skDER and galah report or use): per cluster its medoid, the sum and the minimum of the within-cluster ANI
// and the nearest item outside, from the dense ANI matrix and a cluster assignment in any labelling.  Everything is decided
// on integers (include/hypergen.h, "Cluster statistics"):
//   m(i, j) = hg_avg_milli(ani[i][j]), the ANI as `dist` prints it, in thousandths; the row of i uses row i of the matrix
//   only, the diagonal is never read, nothing assumes symmetry;
//   node i    : within_sum = the sum of m(i, j) over j != i of i's cluster; (within_min, within_min_idx) the smallest such
//               m and the smallest j that attains it; (outside_max, outside_max_idx) the largest m(i, j) over j outside
//               i's cluster and the smallest j that attains it;
//   cluster c : the sum of its members' within_sum, its size, its smallest member, the medoid -- the member with the
//               largest within_sum, ties to the smallest index --, the minimum of within_min with the smallest member
//               that attains it, the maximum of outside_max with the smallest member that attains it.
// Only integer add, min and max are used: the result depends on the matrix and the assignment alone.
//
//   * check : one lane per cluster id clears its accumulator, one lane per node tests cluster[i] < n_clusters (the error
//             word; such a node indexes nothing anywhere below).
//   * rows  : cluster_stats_rows_kernel, one workgroup per row of a block of the matrix: the row's floats in 16-byte loads
//             (a block row starts at blk + r * n, 16-byte aligned only when n % 4 == 0: head and tail are peeled), the ids
//             in 16-byte loads where the ids behind the head are aligned, else in dwords.  Per lane a sum and two 64-bit
//             keys -- m << 32 | j under min, m << 32 | ~j under max: the tie goes to the smaller j --, reduced by wave
//             shuffles, then across the four waves in LDS.  Every row is finished inside its block.
//   * fold  : one lane per node: 64-bit agent-scope atomics on the accumulator of its cluster -- add (within_sum, size),
//             min (first, within_min << 32 | i), max (outside_max << 32 | ~i, the largest within_sum);
//   * medoid: one lane per node: the smallest i whose within_sum equals its cluster's largest (min);
//   * emit  : one lane per cluster id writes the record.
//
// Memory: n_clusters accumulators of 48 bytes, n node records of 24 bytes when the caller wants none, and for resident
// sketches one block of the ANI matrix -- rows [r0, r1) x all n columns from hg_dist_full_dev in the search's scratch
// block, at most HG_SEARCH_BLOCK_BYTES ("stats_block_rows" forces the row count; the row-block driver is
// hg_dense_matrix.h's, with whole rows in the place of the triangle).  No n x n matrix is held.
#include <algorithm>

#include "hg_average_cmp.h"
#include "hg_cluster_common.h"
#include "hg_dense_matrix.h"

static_assert(sizeof(hg_node_stat) == 24 && sizeof(hg_cluster_stat) == 48, "the records of include/hypergen.h");

namespace {
constexpr uint32_t NONE = HG_STATS_NONE;
constexpr uint64_t NO_MIN = ~0ull;  // (a key holds m <= 100 000 in its upper word: never this)
constexpr uint64_t NO_MAX = 0ull;   // (a key holds ~j, j < 2^31, in its lower word: never this)

struct Acc {  // one cluster id while the nodes are folded
  uint64_t sum;      // add: within_sum of the members
  uint64_t min_key;  // min: within_min << 32 | member
  uint64_t max_key;  // max: outside_max << 32 | ~member
  uint64_t top_sum;  // max: the largest within_sum of a member
  uint32_t size, first, medoid, pad;
};
static_assert(sizeof(Acc) == 48, "Acc");

__global__ __launch_bounds__(256) void cluster_stats_check_kernel(const uint32_t *__restrict__ cluster, uint32_t n, uint32_t n_clusters,
                                                                  Acc *__restrict__ acc, uint32_t *res) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t k = t0; k < n_clusters; k += stride) acc[k] = Acc{0ull, NO_MIN, NO_MAX, 0ull, 0u, NONE, NONE, 0u};
  bool bad = false;
  for (size_t i = t0; i < n; i += stride) bad |= cluster[i] >= n_clusters;
  if (bad) __hip_atomic_store(res + HG_CLU_ERR, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct Run {  // what a lane, a wave, a workgroup knows of its row
  uint64_t sum, min_key, max_key;
};
__device__ __forceinline__ void run_take(Run &x, float ani, uint32_t j, uint32_t cj, uint32_t i, uint32_t ci) {
  if (j == i) return;  // (the diagonal's value is not looked at)
  const uint64_t m = hg_avg_milli(ani);
  if (cj == ci) {
    x.sum += m;
    x.min_key = min(x.min_key, m << 32 | (uint64_t)j);
  } else {
    x.max_key = max(x.max_key, m << 32 | (uint64_t)(uint32_t)~j);
  }
}
__device__ __forceinline__ void run_merge(Run &x, const Run &y) {
  x.sum += y.sum, x.min_key = min(x.min_key, y.min_key), x.max_key = max(x.max_key, y.max_key);
}

// One workgroup per row: blk[r * n + j] = ani(r0 + r, j), j < n.  node[r0 + r] is written by lane 0.
__global__ __launch_bounds__(256) void cluster_stats_rows_kernel(const float *__restrict__ blk, uint32_t r0, uint32_t n,
                                                                 const uint32_t *__restrict__ cluster, hg_node_stat *__restrict__ node) {
  __shared__ uint64_t s_sum[4], s_min[4], s_max[4];
  const uint32_t t = threadIdx.x, i = r0 + blockIdx.x;
  const float *row = blk + (size_t)blockIdx.x * n;
  const uint32_t ci = cluster[i];
  // [0, head) in dwords up to the first 16-byte boundary of the row, nvec float4 behind it, [tail, n) in dwords
  const uint32_t head = min(n, (uint32_t)((0u - (uint32_t)(reinterpret_cast<uintptr_t>(row) >> 2)) & 3u));
  const uint32_t nvec = (n - head) >> 2, tail = head + 4u * nvec;
  const bool ids_aligned = (reinterpret_cast<uintptr_t>(cluster + head) & 15u) == 0;  // (uniform over the workgroup)
  Run x{0ull, NO_MIN, NO_MAX};
  if (t < head) run_take(x, row[t], t, cluster[t], i, ci);
  if (t < n - tail) run_take(x, row[tail + t], tail + t, cluster[tail + t], i, ci);
  const float4 *rv = reinterpret_cast<const float4 *>(row + head);
  for (uint32_t v = t; v < nvec; v += 256u) {
    const uint32_t j = head + 4u * v;  // j + 3 < tail <= n
    const float4 a = rv[v];
    uint4 c;
    if (ids_aligned) c = *reinterpret_cast<const uint4 *>(cluster + j);
    else c = make_uint4(cluster[j], cluster[j + 1u], cluster[j + 2u], cluster[j + 3u]);
    run_take(x, a.x, j, c.x, i, ci);
    run_take(x, a.y, j + 1u, c.y, i, ci);
    run_take(x, a.z, j + 2u, c.z, i, ci);
    run_take(x, a.w, j + 3u, c.w, i, ci);
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const Run y{__shfl_xor((unsigned long long)x.sum, d), __shfl_xor((unsigned long long)x.min_key, d),
                __shfl_xor((unsigned long long)x.max_key, d)};
    run_merge(x, y);
  }
  if ((t & 63u) == 0) s_sum[t >> 6] = x.sum, s_min[t >> 6] = x.min_key, s_max[t >> 6] = x.max_key;
  __syncthreads();
  if (t == 0) {
    for (uint32_t w = 1; w < 4; ++w) run_merge(x, Run{s_sum[w], s_min[w], s_max[w]});
    hg_node_stat o;
    o.within_sum = x.sum;
    o.within_min = x.min_key == NO_MIN ? NONE : (uint32_t)(x.min_key >> 32);
    o.within_min_idx = x.min_key == NO_MIN ? NONE : (uint32_t)x.min_key;
    o.outside_max = x.max_key == NO_MAX ? NONE : (uint32_t)(x.max_key >> 32);
    o.outside_max_idx = x.max_key == NO_MAX ? NONE : ~(uint32_t)x.max_key;
    node[i] = o;
  }
}

__device__ __forceinline__ void acc_add(uint64_t *p, uint64_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void acc_min(uint64_t *p, uint64_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void acc_max(uint64_t *p, uint64_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One lane per node (behind the launch boundary of the last rows kernel: every node record is final).
__global__ __launch_bounds__(256) void cluster_stats_fold_kernel(const hg_node_stat *__restrict__ node, const uint32_t *__restrict__ cluster,
                                                                 uint32_t n, uint32_t n_clusters, Acc *acc) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
    const uint32_t i = (uint32_t)k, c = cluster[i];
    if (c >= n_clusters) continue;  // (the check kernel has set the error word)
    const hg_node_stat s = node[i];
    Acc *a = acc + c;
    acc_add(&a->sum, s.within_sum);
    acc_max(&a->top_sum, s.within_sum);
    if (s.within_min_idx != NONE) acc_min(&a->min_key, (uint64_t)s.within_min << 32 | i);
    if (s.outside_max_idx != NONE) acc_max(&a->max_key, (uint64_t)s.outside_max << 32 | (uint32_t)~i);
    __hip_atomic_fetch_add(&a->size, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(&a->first, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One lane per node (behind the fold's launch boundary: top_sum is final).
__global__ __launch_bounds__(256) void cluster_stats_medoid_kernel(const hg_node_stat *__restrict__ node, const uint32_t *__restrict__ cluster,
                                                                   uint32_t n, uint32_t n_clusters, Acc *acc) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
    const uint32_t i = (uint32_t)k, c = cluster[i];
    if (c >= n_clusters) continue;
    if (node[i].within_sum == acc[c].top_sum) __hip_atomic_fetch_min(&acc[c].medoid, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One lane per cluster id.  node == nullptr: n == 0, every record is empty.
__global__ __launch_bounds__(256) void cluster_stats_emit_kernel(const Acc *__restrict__ acc, const hg_node_stat *__restrict__ node,
                                                                 uint32_t n_clusters, hg_cluster_stat *__restrict__ stat) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_clusters; k += stride) {
    hg_cluster_stat o{0ull, 0u, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, 0u};
    if (node) {
      const Acc a = acc[k];
      o.within_sum = a.sum, o.size = a.size, o.first = a.first, o.medoid = a.medoid;
      if (a.min_key != NO_MIN) {
        o.within_min = (uint32_t)(a.min_key >> 32), o.within_min_a = (uint32_t)a.min_key;
        o.within_min_b = node[o.within_min_a].within_min_idx;
      }
      if (a.max_key != NO_MAX) {
        o.outside_max = (uint32_t)(a.max_key >> 32), o.outside_member = ~(uint32_t)a.max_key;
        o.outside_idx = node[o.outside_member].outside_max_idx;
      }
    }
    stat[k] = o;
  }
}

struct Stats {
  Acc *acc;
  hg_node_stat *node;  // the caller's, or n records behind the accumulators
  uint32_t *res;
};

hg_status stats_args(hg_ctx *c, size_t n, size_t n_clusters, const void *d_node, const void *d_stat) {
  if (!d_node && !d_stat) return hg_fail(c, HG_ERR_INVALID, "d_node and d_stat are both NULL: nothing to compute");
  if (n > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "n must be < 2^31");
  if (n_clusters > 0xFFFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "n_clusters must be < 2^32");
  return HG_OK;
}

// n == 0: the n_clusters records, all empty
hg_status stats_empty(hg_ctx *c, size_t n_clusters, hg_cluster_stat *d_stat) {
  if (d_stat && n_clusters) {
    hg_timed tm(c, HG_T_DIST);
    hipLaunchKernelGGL(cluster_stats_emit_kernel, dim3(grid_for(c, n_clusters)), dim3(256), 0, c->stream, nullptr, nullptr,
                       (uint32_t)n_clusters, d_stat);
    HG_HIP(c, hipGetLastError());
  }
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

// the accumulators (and the node records the caller does not take) in w_cstats, cleared; the ids checked
hg_status stats_begin(hg_ctx *c, size_t n, const uint32_t *d_cluster, size_t n_clusters, hg_node_stat *d_node, Stats &g) {
  hg_status s;
  if ((s = hg_cluster_res(c, &g.res)) != HG_OK) return s;
  const size_t acc_bytes = n_clusters * sizeof(Acc);
  if ((s = hg_ensure(c, c->w_cstats, acc_bytes + (d_node ? 0 : n * sizeof(hg_node_stat)) + 64)) != HG_OK) return s;
  g.acc = static_cast<Acc *>(c->w_cstats.p);
  g.node = d_node ? d_node : reinterpret_cast<hg_node_stat *>(static_cast<char *>(c->w_cstats.p) + acc_bytes);
  // The check kernel only raises the error word, so it has to find it clear, and "zero between calls" does not hold: an
  // incremental clustering may be dropped behind hg_cluster_add_hits_dev, which leaves the word raised by a hit with an
  // index >= n.  Cleared here in stream order, not inside the kernel: other lanes of the same launch raise the word.
  HG_HIP(c, hipMemsetAsync(g.res, 0, 2 * sizeof(uint32_t), c->stream));
  hg_timed tm(c, HG_T_DIST);
  hipLaunchKernelGGL(cluster_stats_check_kernel, dim3(grid_for(c, std::max(n, n_clusters))), dim3(256), 0, c->stream, d_cluster, (uint32_t)n,
                     (uint32_t)n_clusters, g.acc, g.res);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

// rows [r0, r0 + rows) from a block of ANI values, n columns each (cluster_stats_rows_kernel)
hg_status stats_rows(hg_ctx *c, const Stats &g, const float *blk, size_t r0, size_t rows, size_t n, const uint32_t *d_cluster) {
  hg_timed tm(c, HG_T_DIST);
  hipLaunchKernelGGL(cluster_stats_rows_kernel, dim3((unsigned)rows), dim3(256), 0, c->stream, blk, (uint32_t)r0, (uint32_t)n, d_cluster,
                     g.node);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

// the node records -> the cluster records; the error word back, and cleared behind the copy
hg_status stats_finish(hg_ctx *c, const Stats &g, size_t n, const uint32_t *d_cluster, size_t n_clusters, hg_cluster_stat *d_stat) {
  if (d_stat) {
    hg_timed tm(c, HG_T_DIST);
    const dim3 node_grid(grid_for(c, n));
    hipLaunchKernelGGL(cluster_stats_fold_kernel, node_grid, dim3(256), 0, c->stream, g.node, d_cluster, (uint32_t)n, (uint32_t)n_clusters,
                       g.acc);
    HG_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(cluster_stats_medoid_kernel, node_grid, dim3(256), 0, c->stream, g.node, d_cluster, (uint32_t)n, (uint32_t)n_clusters,
                       g.acc);
    HG_HIP(c, hipGetLastError());
    if (n_clusters) {
      hipLaunchKernelGGL(cluster_stats_emit_kernel, dim3(grid_for(c, n_clusters)), dim3(256), 0, c->stream, g.acc, g.node,
                         (uint32_t)n_clusters, d_stat);
      HG_HIP(c, hipGetLastError());
    }
  }
  const uint32_t *h_res = nullptr;
  const hg_status s = hg_publish_words(c, g.res, 2, &h_res, 2);
  if (s != HG_OK) return s;
  if (h_res[HG_CLU_ERR]) return hg_fail(c, HG_ERR_INVALID, "a cluster id given to hg_cluster_stats* was >= n_clusters");
  return HG_OK;
}
}  // namespace

extern "C" hg_status hg_cluster_stats_matrix_dev(hg_ctx *c, const float *d_ani, size_t n, const uint32_t *d_cluster, size_t n_clusters,
                                                 hg_node_stat *d_node, hg_cluster_stat *d_stat) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = stats_args(c, n, n_clusters, d_node, d_stat);
  if (s != HG_OK) return s;
  HG_ENTER(c);
  if (n == 0) return stats_empty(c, n_clusters, d_stat);
  if (!d_ani || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  Stats g{};
  if ((s = stats_begin(c, n, d_cluster, n_clusters, d_node, g)) != HG_OK) return s;
  if ((s = stats_rows(c, g, d_ani, 0, n, n, d_cluster)) != HG_OK) return s;
  return stats_finish(c, g, n, d_cluster, n_clusters, d_stat);
}

extern "C" hg_status hg_cluster_stats_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                          const uint32_t *d_cluster, size_t n_clusters, hg_node_stat *d_node, hg_cluster_stat *d_stat) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = stats_args(c, n, n_clusters, d_node, d_stat);
  if (s != HG_OK) return s;
  if (c->ani_metric == HG_ANI_CONTAINMENT)
    return hg_fail(c, HG_ERR_INVALID, "clustering needs a symmetric ANI metric: HG_ANI_CONTAINMENT is directional");
  HG_ENTER(c);
  if (n == 0) return stats_empty(c, n_clusters, d_stat);
  if (!d_hv || !d_norm2 || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if ((s = hg_sketch_dims_check(c, hv_d, ksize)) != HG_OK) return s;
  // rows [r0, r0 + rows) x all n columns of the ANI matrix per block
  Stats g{};
  s = hg_matrix_row_blocks(
      c, d_hv, d_norm2, n, hv_d, ksize, c->dbg_stats_block_rows, false, [&] { return stats_begin(c, n, d_cluster, n_clusters, d_node, g); },
      [&](const float *blk, size_t, size_t, size_t r0, size_t rows) { return stats_rows(c, g, blk, r0, rows, n, d_cluster); });
  if (s != HG_OK) return s;
  return stats_finish(c, g, n, d_cluster, n_clusters, d_stat);
}

extern "C" hg_status hg_cluster_stats(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                      const uint32_t *cluster, size_t n_clusters, hg_node_stat *node, hg_cluster_stat *stat) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = stats_args(c, n, n_clusters, node, stat);
  if (s != HG_OK) return s;
  if (c->ani_metric == HG_ANI_CONTAINMENT)
    return hg_fail(c, HG_ERR_INVALID, "clustering needs a symmetric ANI metric: HG_ANI_CONTAINMENT is directional");
  if (n == 0) {
    const hg_cluster_stat empty{0ull, 0u, HG_STATS_NONE, HG_STATS_NONE, HG_STATS_NONE, HG_STATS_NONE, HG_STATS_NONE,
                                HG_STATS_NONE, HG_STATS_NONE, HG_STATS_NONE, 0u};
    if (stat) std::fill(stat, stat + n_clusters, empty);
    return HG_OK;
  }
  if (!hv || !norm2 || !cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  // in w_ani: the cluster records, the node records, the ids (each part a multiple of 16 bytes behind a 16-byte boundary)
  const size_t stat_bytes = stat ? n_clusters * sizeof(hg_cluster_stat) : 0, node_bytes = node ? (n * sizeof(hg_node_stat) + 15) & ~(size_t)15 : 0;
  const int16_t *d_hv;
  const int32_t *d_norm2;
  uint32_t *d_out;
  if ((s = hg_cluster_stage(c, hv, norm2, n, hv_d, stat_bytes + node_bytes + n * sizeof(uint32_t), &d_hv, &d_norm2, &d_out)) != HG_OK) return s;
  char *base = reinterpret_cast<char *>(d_out);
  auto *d_stat = stat ? reinterpret_cast<hg_cluster_stat *>(base) : nullptr;
  auto *d_node = node ? reinterpret_cast<hg_node_stat *>(base + stat_bytes) : nullptr;
  auto *d_cluster = reinterpret_cast<uint32_t *>(base + stat_bytes + node_bytes);
  HG_HIP(c, hipMemcpyAsync(d_cluster, cluster, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  if ((s = hg_cluster_stats_dev(c, d_hv, d_norm2, n, hv_d, ksize, d_cluster, n_clusters, d_node, d_stat)) != HG_OK) return s;
  if (node) HG_HIP(c, hipMemcpyAsync(node, d_node, n * sizeof(hg_node_stat), hipMemcpyDeviceToHost, c->stream));
  if (stat && n_clusters) HG_HIP(c, hipMemcpyAsync(stat, d_stat, stat_bytes, hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}
