// hg_linkage_rounds.h -- the rounds of mutual best partners that average and complete linkage share (hg_cluster_average.hip,
// hg_cluster_complete.hip: each states its rule and why the rounds resolve it), on the matrix of hg_dense_matrix.h.  A
// scheme gives two structs.  Its Op, for the kernel bodies: the element type T, the 16-byte vector V of it, comb() -- what
// a merge does to two entries, + or min -- and level() of a merge.  Its scheme struct L : Op, for the host side: the names
// in its messages, its limit, its buffer, round counter and test hooks in the ctx, whether the per-node arrays are padded
// to the row pitch, its eight kernels -- the __global__ wrappers of the bodies below and its own best kernel -- and
// launch_best().  One round is best, pair, rows, cols; the three extern "C" forms of a scheme are linkage_matrix_dev,
// linkage_dev and linkage_host of its L.
#pragma once
#include "hg_average_cmp.h"
#include "hg_block_scan.h"
#include "hg_cluster_common.h"
#include "hg_dense_matrix.h"

constexpr uint64_t LINKAGE_DEFAULT_ROUNDS = 4;         // rounds queued per readback of the merge count
constexpr uint32_t LINKAGE_MERGED = HG_CLU_UNDECIDED;  // result words [2], [3]: merges of the odd / even rounds

// len = n, or the row pitch ld where L::padded_nodes (cnt[] is then read in the same 16-byte pieces as a row)
template <typename T>
struct Linkage {
  T *M;              // n rows of ld entries
  size_t ld;         // n rounded up to the entries of 16 bytes
  uint32_t *nn;      // len: best partner of the round, DENSE_NONE = none (dead rows too)
  uint32_t *partner; // len: the name absorbed into this one in this round, else DENSE_NONE
  uint32_t *cnt;     // len: the size of a live name, 0 of an absorbed one and of the padding
  uint32_t *msize;   // len: size[] of an absorbed name
  float *level;      // len: level[] of an absorbed name
  uint32_t *res;     // the ctx's clustering result words
  uint32_t round;
};

// res[LINKAGE_MERGED] (the count "of the round before" the first one) is made non-zero; i runs to len, over the padding too
__device__ __forceinline__ void linkage_init_body(uint32_t *__restrict__ rep, uint32_t *__restrict__ nn, uint32_t *__restrict__ partner,
                                                  uint32_t *__restrict__ cnt, uint32_t *__restrict__ msize, float *__restrict__ level, uint32_t n,
                                                  uint32_t len, uint32_t *__restrict__ res, size_t i0, size_t stride) {
  for (size_t i = i0; i < len; i += stride) {
    if (i < n) rep[i] = (uint32_t)i;
    nn[i] = DENSE_NONE, partner[i] = DENSE_NONE, cnt[i] = i < n ? 1u : 0u, msize[i] = 1u, level[i] = 0.0f;
  }
  if (blockIdx.x == 0 && threadIdx.x < HG_CLU_WORDS) res[threadIdx.x] = threadIdx.x == LINKAGE_MERGED ? 1u : 0u;
}

// One lane per node.  nn[] is this round's for every node, and a merged pair's words -- cnt, rep, msize, level of its two
// names -- are touched by the lane of its lower name alone: mutual pairs are disjoint, and no other lane reads cnt of a
// name that is not its own or its mutual partner's.  partner[] is written for every node in every round.
template <typename Op>
__device__ __forceinline__ void linkage_pair_body(const typename Op::T *__restrict__ M, size_t ld, uint32_t n, const uint32_t *__restrict__ nn,
                                                  uint32_t *__restrict__ partner, uint32_t *cnt, uint32_t *rep, uint32_t *msize, float *level,
                                                  uint32_t *res, uint32_t round) {
  __shared__ uint32_t s_wave[4];
  if (res[LINKAGE_MERGED + ((round - 1u) & 1u)] == 0u) return;  // (uniform over the grid)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t merged = 0;
  if (i < n) {
    const uint32_t A = (uint32_t)i, B = nn[A];
    uint32_t p = DENSE_NONE;
    if (B != DENSE_NONE && B < n && B > A && nn[B] == A) {
      const uint32_t cA = cnt[A], cB = cnt[B];
      level[B] = Op::level(M[(size_t)A * ld + B], cA, cB);
      msize[B] = cA + cB, rep[B] = A;
      cnt[A] = cA + cB, cnt[B] = 0u;
      p = B, merged = 1;
    }
    partner[A] = p;
  }
  uint32_t total;
  (void)block_excl_scan<4>(merged, s_wave, &total);
  if (threadIdx.x == 0) {
    if (total) __hip_atomic_fetch_add(res + LINKAGE_MERGED + (round & 1u), total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (blockIdx.x == 0) res[HG_CLU_ROUNDS] += 1u;  // (this lane alone touches the word in this launch)
  }
}

template <typename Op>
__device__ __forceinline__ void linkage_comb(ulonglong2 &x, const ulonglong2 &y) {
  x.x = Op::comb(x.x, y.x), x.y = Op::comb(x.y, y.y);
}
template <typename Op>
__device__ __forceinline__ void linkage_comb(uint4 &x, const uint4 &y) {
  x.x = Op::comb(x.x, y.x), x.y = Op::comb(x.y, y.y), x.z = Op::comb(x.z, y.z), x.w = Op::comb(x.w, y.w);
}

// One workgroup per node: the lower name of a merged pair combines the absorbed row into its own (whole rows, padding
// included), in 16-byte pieces.
template <typename Op>
__device__ __forceinline__ void linkage_rows_body(typename Op::T *M, size_t ld, const uint32_t *__restrict__ partner,
                                                  const uint32_t *__restrict__ res, uint32_t round) {
  using V = typename Op::V;
  if (res[LINKAGE_MERGED + (round & 1u)] == 0u) return;  // (this round's count: final behind the pair kernel's launch)
  const uint32_t A = blockIdx.x, B = partner[A];
  if (B == DENSE_NONE) return;
  V *a = reinterpret_cast<V *>(M + (size_t)A * ld);
  const V *b = reinterpret_cast<const V *>(M + (size_t)B * ld);
  for (size_t j = threadIdx.x; j < ld / (sizeof(V) / sizeof(typename Op::T)); j += 256) {
    V x = a[j];
    const V y = b[j];
    linkage_comb<Op>(x, y);
    a[j] = x;
  }
}

// One workgroup per surviving row: for every merged pair the absorbed column is combined into the one that stays.
template <typename Op>
__device__ __forceinline__ void linkage_cols_body(typename Op::T *M, size_t ld, uint32_t n, const uint32_t *__restrict__ partner,
                                                  const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ res, uint32_t round) {
  if (res[LINKAGE_MERGED + (round & 1u)] == 0u) return;
  const uint32_t R = blockIdx.x;
  if (cnt[R] == 0u) return;
  typename Op::T *row = M + (size_t)R * ld;
  for (uint32_t j = threadIdx.x; j < n; j += 256u) {
    const uint32_t B = partner[j];
    if (B != DENSE_NONE) row[j] = Op::comb(row[j], row[B]);  // (B < n: the pair kernel checked it; row[B] is written by nobody)
  }
}

// the dendrogram arrays the caller asked for, from rep[] before hg_cluster_queue_ids flattens it
__device__ __forceinline__ void linkage_emit_body(const uint32_t *__restrict__ rep, const uint32_t *__restrict__ cnt,
                                                  const uint32_t *__restrict__ msize, const float *__restrict__ level, uint32_t n,
                                                  uint32_t *__restrict__ into, float *__restrict__ level_out, uint32_t *__restrict__ size_out,
                                                  size_t i0, size_t stride) {
  for (size_t i = i0; i < n; i += stride) {
    const uint32_t r = rep[i];
    const bool kept = r == (uint32_t)i;
    if (into) into[i] = r;
    if (level_out) level_out[i] = kept ? 0.0f : level[i];
    if (size_out) size_out[i] = kept ? cnt[i] : msize[i];
  }
}

// per-node state in the scheme's buffer, the matrix in `hold`, everything initialised (stream-ordered)
template <typename L>
hg_status linkage_begin(hg_ctx *c, size_t n, uint32_t *d_rep, Linkage<typename L::T> &g, MatrixHold &hold) {
  using T = typename L::T;
  constexpr size_t piece = sizeof(typename L::V) / sizeof(T);
  hg_status s;
  if ((s = hg_cluster_res(c, &g.res)) != HG_OK) return s;
  g.ld = (n + piece - 1) & ~(piece - 1);
  const size_t len = L::padded_nodes ? g.ld : n;
  if ((s = hg_ensure(c, c->*L::buf, len * 20 + 64)) != HG_OK) return s;
  g.nn = static_cast<uint32_t *>((c->*L::buf).p);
  g.partner = g.nn + len, g.cnt = g.partner + len, g.msize = g.cnt + len;
  g.level = reinterpret_cast<float *>(g.msize + len);
  if ((s = hg_matrix_alloc(c, hold, n * g.ld * sizeof(T), L::scheme)) != HG_OK) return s;
  g.M = static_cast<T *>(hold.p);
  c->*L::rounds = 0;
  hg_timed tm(c, HG_T_DIST);
  if constexpr (L::padded_nodes)
    hipLaunchKernelGGL(L::init_kernel, dim3(grid_for(c, len)), dim3(256), 0, c->stream, d_rep, g.nn, g.partner, g.cnt, g.msize, g.level,
                       (uint32_t)n, (uint32_t)len, g.res);
  else
    hipLaunchKernelGGL(L::init_kernel, dim3(grid_for(c, len)), dim3(256), 0, c->stream, d_rep, g.nn, g.partner, g.cnt, g.msize, g.level,
                       (uint32_t)n, g.res);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

template <typename L>
hg_status linkage_fill(hg_ctx *c, const Linkage<typename L::T> &g, const float *blk, size_t pitch, size_t c0, size_t r0, size_t rows, size_t n) {
  return hg_matrix_fill<typename L::T>(c, L::fill_kernel, g.M, g.ld, blk, pitch, c0, r0, rows, n);
}

// the filled upper triangle -> mirror, rounds until one merges nothing, the dendrogram, dense ids, the result words back
template <typename L>
hg_status linkage_resolve(hg_ctx *c, Linkage<typename L::T> &g, size_t n, float ani_th, uint32_t *d_rep, uint32_t *d_cluster, uint32_t *d_into,
                          float *d_level, uint32_t *d_size, size_t *n_clusters) {
  hg_status s;
  const uint32_t m = (uint32_t)n;
  if ((s = hg_matrix_mirror<typename L::T>(c, L::mirror_kernel, g.M, n, g.ld)) != HG_OK) return s;
  const bool merges = ani_th == ani_th && !(ani_th > 100.0f);  // (a NaN threshold, one above 100: nothing merges)
  const uint64_t th_milli = hg_avg_milli(ani_th);
  const uint64_t per = c->*L::dbg_rounds ? c->*L::dbg_rounds : LINKAGE_DEFAULT_ROUNDS;
  const dim3 row_grid((unsigned)n), node_grid((unsigned)((n + 255) / 256));
  while (merges) {
    {
      hg_timed tm(c, HG_T_DIST);
      for (uint64_t k = 0; k < per; ++k) {
        const uint32_t r = ++g.round;
        L::launch_best(c, g, row_grid, m, th_milli, r);
        HG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(L::pair_kernel, node_grid, dim3(256), 0, c->stream, g.M, g.ld, m, g.nn, g.partner, g.cnt, d_rep, g.msize, g.level,
                           g.res, r);
        HG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(L::rows_kernel, row_grid, dim3(256), 0, c->stream, g.M, g.ld, g.partner, g.res, r);
        HG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(L::cols_kernel, row_grid, dim3(256), 0, c->stream, g.M, g.ld, m, g.partner, g.cnt, g.res, r);
        HG_HIP(c, hipGetLastError());
      }
    }
    const uint32_t *h_res = nullptr;
    if ((s = hg_publish_words(c, g.res, HG_CLU_WORDS, &h_res)) != HG_OK) return s;  // (nothing cleared: the call goes on)
    if (h_res[LINKAGE_MERGED + (g.round & 1u)] == 0u) break;
  }
  if (d_into || d_level || d_size) {
    hg_timed tm(c, HG_T_DIST);
    hipLaunchKernelGGL(L::emit_kernel, dim3(grid_for(c, n)), dim3(256), 0, c->stream, d_rep, g.cnt, g.msize, g.level, m, d_into, d_level, d_size);
    HG_HIP(c, hipGetLastError());
  }
  if ((s = hg_cluster_queue_ids(c, d_rep, n, d_cluster, g.res)) != HG_OK) return s;
  return hg_cluster_close(c, g.res, &(c->*L::rounds), L::hits_fn, n_clusters);
}

// the checks every form starts with, in this order; *done = nothing to do (n == 0)
template <typename L>
hg_status linkage_check(hg_ctx *c, size_t n, size_t *n_clusters, bool dist_form, bool *done) {
  *done = false;
  if (!c) return HG_ERR_INVALID;
  const hg_status s = hg_cluster_check(c, n, n_clusters, dist_form);
  if (s != HG_OK) return s;
  if (n > L::max_n) return hg_fail(c, HG_ERR_UNSUPPORTED, L::too_large);
  *done = n == 0;
  return HG_OK;
}

template <typename L>
hg_status linkage_matrix_dev(hg_ctx *c, const float *d_ani, size_t n, float ani_th, uint32_t *d_rep, uint32_t *d_cluster, uint32_t *d_into,
                             float *d_level, uint32_t *d_size, size_t *n_clusters) {
  bool done;
  hg_status s = linkage_check<L>(c, n, n_clusters, false, &done);
  if (s != HG_OK || done) return s;
  if (!d_ani || !d_rep || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  Linkage<typename L::T> g{};
  MatrixHold hold;
  if ((s = linkage_begin<L>(c, n, d_rep, g, hold)) != HG_OK) return s;
  if ((s = linkage_fill<L>(c, g, d_ani, n, 0, 0, n, n)) != HG_OK) return s;
  return linkage_resolve<L>(c, g, n, ani_th, d_rep, d_cluster, d_into, d_level, d_size, n_clusters);
}

template <typename L>
hg_status linkage_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize, float ani_th,
                      uint32_t *d_rep, uint32_t *d_cluster, uint32_t *d_into, float *d_level, uint32_t *d_size, size_t *n_clusters) {
  bool done;
  hg_status s = linkage_check<L>(c, n, n_clusters, true, &done);
  if (s != HG_OK || done) return s;
  if (!d_hv || !d_norm2 || !d_rep || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if ((s = hg_sketch_dims_check(c, hv_d, ksize)) != HG_OK) return s;
  HG_ENTER(c);
  Linkage<typename L::T> g{};
  MatrixHold hold;
  s = hg_matrix_row_blocks(
      c, d_hv, d_norm2, n, hv_d, ksize, c->*L::dbg_block_rows, true, [&] { return linkage_begin<L>(c, n, d_rep, g, hold); },
      [&](const float *blk, size_t pitch, size_t c0, size_t r0, size_t rows) { return linkage_fill<L>(c, g, blk, pitch, c0, r0, rows, n); });
  if (s != HG_OK) return s;
  return linkage_resolve<L>(c, g, n, ani_th, d_rep, d_cluster, d_into, d_level, d_size, n_clusters);
}

template <typename L>
hg_status linkage_host(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize, float ani_th, uint32_t *rep,
                       uint32_t *cluster, uint32_t *into, float *level, uint32_t *size, size_t *n_clusters) {
  bool done;
  hg_status s = linkage_check<L>(c, n, n_clusters, true, &done);
  if (s != HG_OK || done) return s;
  if (!hv || !norm2 || !rep || !cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  const int16_t *d_hv;
  const int32_t *d_norm2;
  uint32_t *d_rep;
  if ((s = hg_cluster_stage(c, hv, norm2, n, hv_d, 5 * n * sizeof(uint32_t), &d_hv, &d_norm2, &d_rep)) != HG_OK) return s;
  uint32_t *d_cluster = d_rep + n, *d_into = d_cluster + n, *d_size = d_into + n;
  auto *d_level = reinterpret_cast<float *>(d_size + n);
  if ((s = linkage_dev<L>(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, d_rep, d_cluster, into ? d_into : nullptr, level ? d_level : nullptr,
                          size ? d_size : nullptr, n_clusters)) != HG_OK)
    return s;
  HG_HIP(c, hipMemcpyAsync(rep, d_rep, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(cluster, d_cluster, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (into) HG_HIP(c, hipMemcpyAsync(into, d_into, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (level) HG_HIP(c, hipMemcpyAsync(level, d_level, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (size) HG_HIP(c, hipMemcpyAsync(size, d_size, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}
