// hg_cluster_complete.hip -- complete-linkage clustering of sketches at an ANI threshold (an extension like the other
// hg_cluster_*.hip files: dRep's --clusterAlg complete, scipy's linkage(method="complete") on an ANI matrix): the scheme in
// which EVERY pair inside a cluster is at least the threshold.  Like average linkage it works on the dense matrix and
// decides on integers only:
//   m(i, j)  = the integer `dist` prints for ani(i, j), in thousandths (hg_avg_milli: NaN and negative 0, above 100 100 000);
//   th_milli = the same of ani_th (NaN or above 100: nothing merges; <= 0: everything does);
//   a cluster is named by its smallest member, W(A, B) is the minimum of m(a, b) over a in A, b in B;
//   pair {A, B} is BETTER than {C, D} iff W(A, B) > W(C, D); on equality the smaller lower name wins, then the smaller
//   higher name;
//   while the best pair has W(A, B) >= th_milli: merge it -- the smaller name stays, W(K, A u B) = min(W(K, A), W(K, B)).
// rep[i] = the smallest index of i's cluster, cluster[i] its dense id in increasing order of rep.  The dendrogram: for a
// name B absorbed into A, into[B] = A, level[B] = (float)((double)W / 1000.0), size[B] = the merged size; for a name never
// absorbed into[i] = i, level[i] = 0, size[i] = the final size of its cluster.  Only integer min and compares occur: the
// result depends on the matrix alone.
//
// The sequential rule is resolved in ROUNDS on a dense n x n matrix of u32 minima (live rows and columns: the names that
// are still clusters), the structure of hg_cluster_average.hip with min in the place of +.  Complete linkage is reducible
// -- the merged cluster is never closer to K than the closer of the two was -- so every pair of MUTUAL best partners is a
// merge of the sequential rule, and all of them can be done at once.  The index tie-break survives a merge: the key of K
// in row A is (W(A, K), -K); the key of C u D, C < D, is (min(W(A, C), W(A, D)), -C), which is key(C) itself or something
// strictly smaller in its first component -- it never exceeds key(C), so a partner that beat both C and D still beats
// their union.  The global best pair is mutual, so every round but the last one merges.  One round:
//   * best  : one workgroup per live row A: its best partner among the live columns with m >= th_milli, as one 64-bit
//             maximum per lane (m << 32 | 0xFFFFFFFF - j: one compare, ties to the smaller name).  16-byte loads of the row
//             and of cnt[], a reduction by wave shuffles and four LDS words.
//   * pair  : one lane per node: nn[A] == B, nn[B] == A and A < B merge.  Level, size and into of B are written, c(A)
//             grows, B leaves; partner[] is written for every node; the round's merges are counted into a result word.
//   * rows  : one workgroup per merged pair: row A = min(row A, row B).
//   * cols  : one workgroup per surviving row R: M[R][A] = min(M[R][A], M[R][B]) for every merged pair.
// Two pairs {A, B} and {C, D} of one round get W(A u B, C u D), the minimum of four, from the two passes together: rows
// makes M[A][C] and M[A][D] the minima over A u B, cols folds the second into the first.  Neither pass has a race: rows
// writes row A alone and reads row B, which nobody writes; cols works within one row, writes the columns that stay and
// reads the ones that leave.
// Similarities between clusters only ever FALL, which average linkage cannot say, and the best kernel uses it.  From round
// 2 on a live row keeps its nn[A] without a scan when
//   * nn[A] is NONE: the row is retired -- no partner at the threshold now, none ever again (and nobody's partner: the
//     matrix is symmetric among the live names); or
//   * neither A nor B = nn[A] took part in a merge of the previous round (partner[A] == NONE, cnt[B] != 0, partner[B] ==
//     NONE, as the previous round's pair kernel left them): M[A][B] is what it was, every other entry of the row is what
//     it was or smaller, and a union of two columns has a key not above the first one's (above).
// "complete_rescan" = "all" turns both off; the results and the round counts are identical.
// Every kernel runs to its end on its own: no cooperative launch, no wait between workgroups, a launch boundary publishes
// each kernel.  The host queues a few rounds ("complete_rounds"), reads the merges of the last one back (hg_publish_words)
// and stops at a round that merged nothing; the rounds queued behind such a round see its word and return at once.
// The worst case is O(n) rounds -- a chain whose neighbour similarities fall with the index merges one pair per round.
//
// Memory: n x ld u32, ld = n rounded up to a multiple of 4 (every row starts on 16 bytes): 400 MB at 10 000 sketches, 17 GB
// at the limit HG_CLUSTER_COMPLETE_MAX_N; allocated per call and released before the call returns.  The per-node arrays
// have ld entries each, so that cnt[] is read in the same 16-byte pieces as a row; cnt of a padding column is 0, dead.
// hg_cluster_complete_dev fills the upper triangle from row blocks of hg_dist_full_dev (rows [r0, r1) x columns [r0, n) in
// the search's scratch block, at most HG_SEARCH_BLOCK_BYTES; "complete_block_rows" forces the row count) and mirrors it.
#include <algorithm>

#include "hg_average_cmp.h"
#include "hg_block_scan.h"
#include "hg_cluster_common.h"
#include "hg_internal.h"

namespace {
constexpr uint64_t CPL_DEFAULT_ROUNDS = 4;  // rounds queued per readback of the merge count
constexpr uint32_t CPL_NONE = 0xFFFFFFFFu;
constexpr uint32_t CPL_MERGED = HG_CLU_UNDECIDED;  // result words [2], [3]: merges of the odd / even rounds
constexpr uint32_t MIRROR_TILE = 32;
constexpr uint32_t SCAN_STEP = 1024;  // columns one step of the row scan covers: 256 lanes x 4

struct Complete {
  uint32_t *M;       // n rows of ld minima
  size_t ld;         // n rounded up to a multiple of 4
  uint32_t *nn;      // ld: best partner, CPL_NONE = none (dead rows, retired rows)
  uint32_t *partner; // ld: the name absorbed into this one in this round, else CPL_NONE
  uint32_t *cnt;     // ld: the size of a live name, 0 of an absorbed one and of the padding
  uint32_t *msize;   // ld: size[] of an absorbed name
  float *level;      // ld: level[] of an absorbed name
  uint32_t *res;     // the ctx's clustering result words
  uint32_t round;
};

// the matrix, released when the call returns (hipFree waits for the device)
struct MatrixHold {
  void *p = nullptr;
  ~MatrixHold() {
    if (p) (void)hipFree(p);
  }
};

// res[CPL_MERGED] (the count "of the round before" the first one) is made non-zero; i runs over the padding too
__global__ __launch_bounds__(256) void complete_init_kernel(uint32_t *__restrict__ rep, uint32_t *__restrict__ nn, uint32_t *__restrict__ partner,
                                                            uint32_t *__restrict__ cnt, uint32_t *__restrict__ msize, float *__restrict__ level,
                                                            uint32_t n, uint32_t ld, uint32_t *__restrict__ res) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ld; i += stride) {
    if (i < n) rep[i] = (uint32_t)i;
    nn[i] = CPL_NONE, partner[i] = CPL_NONE, cnt[i] = i < n ? 1u : 0u, msize[i] = 1u, level[i] = 0.0f;
  }
  if (blockIdx.x == 0 && threadIdx.x < HG_CLU_WORDS) res[threadIdx.x] = threadIdx.x == CPL_MERGED ? 1u : 0u;
}

// Rows [r0, r0 + rows) of the matrix from a block of ANI values: blk[r * pitch + (j - c0)] is ani(r0 + r, j), c0 <= r0.
// Only j > row is read; the diagonal, the lower triangle (the mirror kernel writes it) and the padding columns become 0.
__global__ __launch_bounds__(256) void complete_fill_kernel(const float *__restrict__ blk, size_t pitch, uint32_t c0, uint32_t r0, uint32_t rows,
                                                            uint32_t n, size_t ld, uint32_t *__restrict__ M) {
  for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const uint32_t gi = r0 + r;
    const float *src = blk + (size_t)r * pitch;
    uint32_t *dst = M + (size_t)gi * ld;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < ld; j += (size_t)gridDim.x * blockDim.x)
      dst[j] = (j > gi && j < n) ? (uint32_t)hg_avg_milli(src[j - c0]) : 0u;
  }
}

// M[j][i] = M[i][j] for i < j: tiles of 32 x 32 through LDS (the column padded by one word against bank conflicts), the
// workgroups of the upper triangle of tiles each write their transposed tile (a diagonal tile its own lower half).
// blockDim = (32, 8).
__global__ __launch_bounds__(256) void complete_mirror_kernel(uint32_t *M, uint32_t n, size_t ld) {
  __shared__ uint32_t tile[MIRROR_TILE][MIRROR_TILE + 1];
  if (blockIdx.x < blockIdx.y) return;  // (uniform over the workgroup)
  const uint32_t row0 = blockIdx.y * MIRROR_TILE, col0 = blockIdx.x * MIRROR_TILE;
  for (uint32_t k = threadIdx.y; k < MIRROR_TILE; k += 8) {
    const uint32_t i = row0 + k, j = col0 + threadIdx.x;
    tile[k][threadIdx.x] = (i < n && j < n) ? M[(size_t)i * ld + j] : 0u;
  }
  __syncthreads();
  for (uint32_t k = threadIdx.y; k < MIRROR_TILE; k += 8) {
    const uint32_t j = col0 + k, i = row0 + threadIdx.x;  // writes M[j][i], the value of M[i][j]
    if (j < n && i < j) M[(size_t)j * ld + i] = tile[threadIdx.x][k];
  }
}

// a candidate of row A as one word under max: the larger m, ties to the smaller column; 0 = none (a column is < 65536)
__device__ __forceinline__ uint64_t cand_key(uint32_t m, uint32_t j) { return (uint64_t)m << 32 | (uint64_t)(0xFFFFFFFFu - j); }
__device__ __forceinline__ uint64_t take4(uint64_t best, const uint4 v, const uint4 c, uint32_t j, uint32_t A, uint32_t th_milli) {
  const uint32_t m[4] = {v.x, v.y, v.z, v.w}, live[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const uint64_t counts = (uint64_t)(live[k] != 0u) & (uint64_t)(j + k != A) & (uint64_t)(m[k] >= th_milli);
    const uint64_t key = cand_key(m[k], j + k) & (0ull - counts);  // (a mask, not a branch)
    best = key > best ? key : best;
  }
  return best;
}

// One workgroup per row.  res[CPL_MERGED + parity]: the count of the previous round is read (0: the last round merged
// nothing, the call is resolved), the one of this round is cleared for complete_pair_kernel behind the launch boundary.
// nn[A] is read and written by the workgroup of A alone; partner[] and cnt[] are the previous round's, final.
__global__ __launch_bounds__(256) void complete_best_kernel(const uint32_t *__restrict__ M, size_t ld, uint32_t n,
                                                            const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ partner,
                                                            uint32_t th_milli, uint32_t *nn, uint32_t *res, uint32_t round,
                                                            uint32_t rescan_all) {
  __shared__ uint64_t s_best[4];
  const uint32_t merged_before = res[CPL_MERGED + ((round - 1u) & 1u)];
  if (blockIdx.x == 0 && threadIdx.x == 0) res[CPL_MERGED + (round & 1u)] = 0u;
  if (merged_before == 0u) return;  // (uniform over the grid: nobody writes that word in this launch)
  const uint32_t A = blockIdx.x, t = threadIdx.x;
  if (cnt[A] == 0u) {  // absorbed: nobody's partner, and no partner of its own
    if (t == 0) nn[A] = CPL_NONE;
    return;
  }
  if (round >= 2u && !rescan_all) {  // (uniform over the workgroup: every lane reads the same words)
    const uint32_t B = nn[A];
    if (B == CPL_NONE) return;  // retired: values only fall
    if (partner[A] == CPL_NONE && cnt[B] != 0u && partner[B] == CPL_NONE) return;  // neither end merged: B is still the best
  }
  const uint4 *row = reinterpret_cast<const uint4 *>(M + (size_t)A * ld);
  const uint4 *live = reinterpret_cast<const uint4 *>(cnt);
  uint64_t best = 0ull;
  // four columns per lane and step (j + 3 < ld: ld is a multiple of 4; the padding columns have cnt 0); two steps per trip
  // while both are inside the row, their four 16-byte loads independent of each other, then at most one step more
  uint32_t j = 4u * t;
  for (; j + SCAN_STEP < n; j += 2u * SCAN_STEP) {
    const uint32_t j1 = j + SCAN_STEP;
    const uint4 v0 = row[j >> 2], c0 = live[j >> 2], v1 = row[j1 >> 2], c1 = live[j1 >> 2];
    best = take4(best, v0, c0, j, A, th_milli);
    best = take4(best, v1, c1, j1, A, th_milli);
  }
  if (j < n) best = take4(best, row[j >> 2], live[j >> 2], j, A, th_milli);
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t y = __shfl_xor((unsigned long long)best, d);
    best = y > best ? y : best;
  }
  if ((t & 63u) == 0) s_best[t >> 6] = best;
  __syncthreads();
  if (t == 0) {
    for (uint32_t w = 1; w < 4; ++w) best = s_best[w] > best ? s_best[w] : best;
    nn[A] = best ? 0xFFFFFFFFu - (uint32_t)best : CPL_NONE;
  }
}

// One lane per node.  A merged pair's words -- cnt, rep, msize, level of its two names -- are touched by the lane of its
// lower name alone: mutual pairs are disjoint, and no other lane reads cnt of a name that is not its own or its mutual
// partner's.  partner[] is written for every node in every round (the next round's best kernel reads all of it).
__global__ __launch_bounds__(256) void complete_pair_kernel(const uint32_t *__restrict__ M, size_t ld, uint32_t n, const uint32_t *__restrict__ nn,
                                                            uint32_t *__restrict__ partner, uint32_t *cnt, uint32_t *rep, uint32_t *msize,
                                                            float *level, uint32_t *res, uint32_t round) {
  __shared__ uint32_t s_wave[4];
  if (res[CPL_MERGED + ((round - 1u) & 1u)] == 0u) return;  // (uniform over the grid)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t merged = 0;
  if (i < n) {
    const uint32_t A = (uint32_t)i, B = nn[A];
    uint32_t p = CPL_NONE;
    if (B != CPL_NONE && B < n && B > A && nn[B] == A) {
      const uint32_t cA = cnt[A], cB = cnt[B];
      const uint32_t W = M[(size_t)A * ld + B];
      level[B] = (float)((double)W / 1000.0);
      msize[B] = cA + cB, rep[B] = A;
      cnt[A] = cA + cB, cnt[B] = 0u;
      p = B, merged = 1;
    }
    partner[A] = p;
  }
  uint32_t total;
  (void)block_excl_scan<4>(merged, s_wave, &total);
  if (threadIdx.x == 0) {
    if (total) __hip_atomic_fetch_add(res + CPL_MERGED + (round & 1u), total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (blockIdx.x == 0) res[HG_CLU_ROUNDS] += 1u;  // (this lane alone touches the word in this launch)
  }
}

// One workgroup per node: the lower name of a merged pair takes the minimum of its row and the absorbed one (whole rows,
// padding included), in 16-byte pieces.
__global__ __launch_bounds__(256) void complete_rows_kernel(uint32_t *M, size_t ld, const uint32_t *__restrict__ partner,
                                                            const uint32_t *__restrict__ res, uint32_t round) {
  if (res[CPL_MERGED + (round & 1u)] == 0u) return;  // (this round's count: final behind complete_pair_kernel's launch)
  const uint32_t A = blockIdx.x, B = partner[A];
  if (B == CPL_NONE) return;
  uint4 *a = reinterpret_cast<uint4 *>(M + (size_t)A * ld);
  const uint4 *b = reinterpret_cast<const uint4 *>(M + (size_t)B * ld);
  for (size_t j = threadIdx.x; j < ld / 4; j += 256) {
    uint4 x = a[j];
    const uint4 y = b[j];
    x.x = min(x.x, y.x), x.y = min(x.y, y.y), x.z = min(x.z, y.z), x.w = min(x.w, y.w);
    a[j] = x;
  }
}

// One workgroup per surviving row: for every merged pair the column that stays takes the minimum with the absorbed one.
__global__ __launch_bounds__(256) void complete_cols_kernel(uint32_t *M, size_t ld, uint32_t n, const uint32_t *__restrict__ partner,
                                                            const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ res, uint32_t round) {
  if (res[CPL_MERGED + (round & 1u)] == 0u) return;
  const uint32_t R = blockIdx.x;
  if (cnt[R] == 0u) return;
  uint32_t *row = M + (size_t)R * ld;
  for (uint32_t j = threadIdx.x; j < n; j += 256u) {
    const uint32_t B = partner[j];
    if (B != CPL_NONE) row[j] = min(row[j], row[B]);  // (B < n: complete_pair_kernel checked it; row[B] is written by nobody)
  }
}

// the dendrogram arrays the caller asked for, from rep[] before hg_cluster_queue_ids flattens it
__global__ __launch_bounds__(256) void complete_emit_kernel(const uint32_t *__restrict__ rep, const uint32_t *__restrict__ cnt,
                                                            const uint32_t *__restrict__ msize, const float *__restrict__ level, uint32_t n,
                                                            uint32_t *__restrict__ into, float *__restrict__ level_out, uint32_t *__restrict__ size_out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t r = rep[i];
    const bool kept = r == (uint32_t)i;
    if (into) into[i] = r;
    if (level_out) level_out[i] = kept ? 0.0f : level[i];
    if (size_out) size_out[i] = kept ? cnt[i] : msize[i];
  }
}

hg_status complete_too_large(hg_ctx *c) {
  return hg_fail(c, HG_ERR_UNSUPPORTED, "complete linkage holds the dense matrix: n must be <= HG_CLUSTER_COMPLETE_MAX_N (65536)");
}

// per-node state in w_complete, the matrix in `hold`, everything initialised (stream-ordered)
hg_status complete_begin(hg_ctx *c, size_t n, uint32_t *d_rep, Complete &g, MatrixHold &hold) {
  hg_status s;
  if ((s = hg_cluster_res(c, &g.res)) != HG_OK) return s;
  g.ld = (n + 3) & ~(size_t)3;
  if ((s = hg_ensure(c, c->w_complete, g.ld * 20 + 64)) != HG_OK) return s;
  g.nn = static_cast<uint32_t *>(c->w_complete.p);
  g.partner = g.nn + g.ld, g.cnt = g.partner + g.ld, g.msize = g.cnt + g.ld;
  g.level = reinterpret_cast<float *>(g.msize + g.ld);
  const size_t bytes = n * g.ld * sizeof(uint32_t);
  const hipError_t e = hipMalloc(&hold.p, bytes);
  if (e != hipSuccess) {
    hold.p = nullptr;
    return hg_fail(c, HG_ERR_OOM, "hipMalloc(" + std::to_string(bytes) + ") for the matrix of complete linkage: " + hipGetErrorString(e));
  }
  g.M = static_cast<uint32_t *>(hold.p);
  c->complete_rounds = 0;
  hg_timed tm(c, HG_T_DIST);
  hipLaunchKernelGGL(complete_init_kernel, dim3(grid_for(c, g.ld)), dim3(256), 0, c->stream, d_rep, g.nn, g.partner, g.cnt, g.msize, g.level,
                     (uint32_t)n, (uint32_t)g.ld, g.res);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

// rows [r0, r0 + rows) from a block of ANI values (complete_fill_kernel)
hg_status complete_fill(hg_ctx *c, const Complete &g, const float *blk, size_t pitch, size_t c0, size_t r0, size_t rows, size_t n) {
  hg_timed tm(c, HG_T_DIST);
  const dim3 grid((unsigned)std::min<size_t>((g.ld + 255) / 256, 64), (unsigned)std::min<size_t>(rows, 16384));
  hipLaunchKernelGGL(complete_fill_kernel, grid, dim3(256), 0, c->stream, blk, pitch, (uint32_t)c0, (uint32_t)r0, (uint32_t)rows, (uint32_t)n,
                     g.ld, g.M);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

// the filled upper triangle -> mirror, rounds until one merges nothing, the dendrogram, dense ids, the result words back
hg_status complete_resolve(hg_ctx *c, Complete &g, size_t n, float ani_th, uint32_t *d_rep, uint32_t *d_cluster, uint32_t *d_into,
                           float *d_level, uint32_t *d_size, size_t *n_clusters) {
  hg_status s;
  const uint32_t m = (uint32_t)n;
  {
    hg_timed tm(c, HG_T_DIST);
    const unsigned tiles = (unsigned)((n + MIRROR_TILE - 1) / MIRROR_TILE);
    hipLaunchKernelGGL(complete_mirror_kernel, dim3(tiles, tiles), dim3(MIRROR_TILE, 8), 0, c->stream, g.M, m, g.ld);
    HG_HIP(c, hipGetLastError());
  }
  const bool merges = ani_th == ani_th && !(ani_th > 100.0f);  // (a NaN threshold, one above 100: nothing merges)
  const uint32_t th_milli = (uint32_t)hg_avg_milli(ani_th);
  const uint64_t per = c->dbg_complete_rounds ? c->dbg_complete_rounds : CPL_DEFAULT_ROUNDS;
  const uint32_t rescan_all = c->dbg_complete_rescan_all ? 1u : 0u;
  const dim3 row_grid((unsigned)n), node_grid((unsigned)((n + 255) / 256));
  while (merges) {
    {
      hg_timed tm(c, HG_T_DIST);
      for (uint64_t k = 0; k < per; ++k) {
        const uint32_t r = ++g.round;
        hipLaunchKernelGGL(complete_best_kernel, row_grid, dim3(256), 0, c->stream, g.M, g.ld, m, g.cnt, g.partner, th_milli, g.nn, g.res, r,
                           rescan_all);
        HG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(complete_pair_kernel, node_grid, dim3(256), 0, c->stream, g.M, g.ld, m, g.nn, g.partner, g.cnt, d_rep, g.msize,
                           g.level, g.res, r);
        HG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(complete_rows_kernel, row_grid, dim3(256), 0, c->stream, g.M, g.ld, g.partner, g.res, r);
        HG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(complete_cols_kernel, row_grid, dim3(256), 0, c->stream, g.M, g.ld, m, g.partner, g.cnt, g.res, r);
        HG_HIP(c, hipGetLastError());
      }
    }
    const uint32_t *h_res = nullptr;
    if ((s = hg_publish_words(c, g.res, HG_CLU_WORDS, &h_res)) != HG_OK) return s;  // (nothing cleared: the call goes on)
    if (h_res[CPL_MERGED + (g.round & 1u)] == 0u) break;
  }
  if (d_into || d_level || d_size) {
    hg_timed tm(c, HG_T_DIST);
    hipLaunchKernelGGL(complete_emit_kernel, dim3(grid_for(c, n)), dim3(256), 0, c->stream, d_rep, g.cnt, g.msize, g.level, m, d_into, d_level,
                       d_size);
    HG_HIP(c, hipGetLastError());
  }
  if ((s = hg_cluster_queue_ids(c, d_rep, n, d_cluster, g.res)) != HG_OK) return s;
  return hg_cluster_close(c, g.res, &c->complete_rounds, "hg_cluster_complete_matrix_dev", n_clusters);
}
}  // namespace

extern "C" uint64_t hg_ctx_cluster_complete_rounds(const hg_ctx *c) { return c ? c->complete_rounds : 0; }

extern "C" hg_status hg_cluster_complete_matrix_dev(hg_ctx *c, const float *d_ani, size_t n, float ani_th, uint32_t *d_rep, uint32_t *d_cluster,
                                                    uint32_t *d_into, float *d_level, uint32_t *d_size, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_cluster_check(c, n, n_clusters, false);
  if (s != HG_OK) return s;
  if (n > HG_CLUSTER_COMPLETE_MAX_N) return complete_too_large(c);
  if (n == 0) return HG_OK;
  if (!d_ani || !d_rep || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  Complete g{};
  MatrixHold hold;
  if ((s = complete_begin(c, n, d_rep, g, hold)) != HG_OK) return s;
  if ((s = complete_fill(c, g, d_ani, n, 0, 0, n, n)) != HG_OK) return s;
  return complete_resolve(c, g, n, ani_th, d_rep, d_cluster, d_into, d_level, d_size, n_clusters);
}

extern "C" hg_status hg_cluster_complete_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                             float ani_th, uint32_t *d_rep, uint32_t *d_cluster, uint32_t *d_into, float *d_level,
                                             uint32_t *d_size, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_cluster_check(c, n, n_clusters, true);
  if (s != HG_OK) return s;
  if (n > HG_CLUSTER_COMPLETE_MAX_N) return complete_too_large(c);
  if (n == 0) return HG_OK;
  if (!d_hv || !d_norm2 || !d_rep || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (hv_d == 0 || hv_d > 65536) return hg_fail(c, HG_ERR_UNSUPPORTED, "hv_d must be in 1..65536");
  if (ksize == 0) return hg_fail(c, HG_ERR_INVALID, "ksize must be >= 1");
  HG_ENTER(c);
  // the scratch block: rows [r0, r0 + rb) x columns [r0, n) of the ANI matrix, the first block being the widest
  const size_t fit = std::max<size_t>(1, HG_SEARCH_BLOCK_BYTES / (sizeof(float) * n));
  const size_t rb = std::min<size_t>(n, c->dbg_complete_block_rows ? (size_t)c->dbg_complete_block_rows : fit);
  if ((s = hg_ensure(c, c->w_srch_blk, rb * n * sizeof(float))) != HG_OK) return s;
  auto *blk = static_cast<float *>(c->w_srch_blk.p);
  Complete g{};
  MatrixHold hold;
  if ((s = complete_begin(c, n, d_rep, g, hold)) != HG_OK) return s;
  for (size_t r0 = 0; r0 < n; r0 += rb) {
    const size_t rows = std::min(rb, n - r0), cols = n - r0;
    if ((s = hg_dist_full_dev(c, d_hv + r0 * (size_t)hv_d, d_norm2 + r0, rows, d_hv + r0 * (size_t)hv_d, d_norm2 + r0, cols, hv_d, ksize,
                              blk)) != HG_OK)
      return s;
    if ((s = complete_fill(c, g, blk, cols, r0, r0, rows, n)) != HG_OK) return s;
  }
  return complete_resolve(c, g, n, ani_th, d_rep, d_cluster, d_into, d_level, d_size, n_clusters);
}

extern "C" hg_status hg_cluster_complete(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                         float ani_th, uint32_t *rep, uint32_t *cluster, uint32_t *into, float *level, uint32_t *size,
                                         size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_cluster_check(c, n, n_clusters, true);
  if (s != HG_OK) return s;
  if (n > HG_CLUSTER_COMPLETE_MAX_N) return complete_too_large(c);
  if (n == 0) return HG_OK;
  if (!hv || !norm2 || !rep || !cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  const int16_t *d_hv;
  const int32_t *d_norm2;
  uint32_t *d_rep;
  if ((s = hg_cluster_stage(c, hv, norm2, n, hv_d, 5 * n * sizeof(uint32_t), &d_hv, &d_norm2, &d_rep)) != HG_OK) return s;
  uint32_t *d_cluster = d_rep + n, *d_into = d_cluster + n, *d_size = d_into + n;
  auto *d_level = reinterpret_cast<float *>(d_size + n);
  if ((s = hg_cluster_complete_dev(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, d_rep, d_cluster, into ? d_into : nullptr, level ? d_level : nullptr,
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
