// hg_cluster_average.hip -- average-linkage (UPGMA) clustering of sketches at an ANI threshold (an extension like the other
// hg_cluster_*.hip files: dRep's primary clustering, scipy's linkage(method="average") on an ANI matrix).  Unlike the other
// schemes it cannot be decided from the pairs at or above the threshold -- the pairs below it enter the averages -- so it
// works on the dense matrix, and it decides on integers only:
//   m(i, j)  = the integer `dist` prints for ani(i, j), in thousandths (hg_avg_milli: NaN and negative 0, above 100 100 000);
//   th_milli = the same of ani_th (NaN or above 100: nothing merges; <= 0: everything does);
//   a cluster is named by its smallest member, c(A) is its size, S(A, B) the sum of m(a, b) over a in A, b in B;
//   pair {A, B} is BETTER than {C, D} iff S(A,B) c(C) c(D) > S(C,D) c(A) c(B), exactly; on equality the smaller lower name
//   wins, then the smaller higher name;
//   while the best pair has S(A,B) >= th_milli c(A) c(B): merge it -- the smaller name stays, S(K, A u B) = S(K,A) + S(K,B).
// rep[i] = the smallest index of i's cluster, cluster[i] its dense id in increasing order of rep.  The dendrogram: for a
// name B absorbed into A, into[B] = A, level[B] = (float)(((double)S / (double)(c(A) c(B))) / 1000.0), size[B] = c(A) + c(B)
// right after the merge; for a name never absorbed into[i] = i, level[i] = 0, size[i] = the final size of its cluster.
// Only integers are added and every comparison is exact: the result depends on the matrix alone.
//
// The sequential rule is resolved in ROUNDS on a dense n x n matrix of u64 sums (live rows and columns: the names that are
// still clusters).  Average linkage is reducible -- merging A and B never makes the merged cluster closer to K than the
// closer of the two was -- so every pair of MUTUAL best partners is a merge of the sequential rule, and all of them can be
// done at once; with the merged cluster named by its minimum the index tie-break survives.  One round:
//   * best  : one workgroup per live row A: its best partner among the live columns whose pair meets the threshold.  c(A)
//             is common to the row, so S(A,B) / c(B) is compared, exactly (hg_average_cmp.h: 128-bit cross products), ties
//             to the smaller B -- the pair order above restricted to one row.  16-byte loads, a reduction in LDS.
//   * pair  : one lane per node: nn[A] == B, nn[B] == A and A < B merge.  Level, size and into of B are written, c(A)
//             grows, B leaves; the round's merges are counted into a result word.
//   * rows  : one workgroup per merged pair: row A += row B.
//   * cols  : one workgroup per surviving row R: M[R][A] += M[R][B] for every merged pair.
// Two pairs {A, B} and {C, D} of one round get S(A u B, C u D) from the two passes together: rows makes M[A][C] and
// M[A][D] the sums over A u B, cols adds the second to the first.  Neither pass has a race: rows writes row A alone and
// reads row B, which nobody writes; cols works within one row, writes the columns that stay and reads the ones that leave.
// Every kernel runs to its end on its own.  The host queues a few rounds ("average_rounds"), reads the merges of the last
// one back (hg_publish_words) and stops at a round that merged nothing; the rounds queued behind such a round see its word
// and return at once.  The global best pair is mutual, so every round but the last one merges.
// The worst case is O(n) rounds -- a chain whose neighbour similarities fall with the index merges one pair per round --
// and is accepted as the greedy resolution's path is: groups, what a dereplication sees, take some tens of rounds (100
// groups of 100 near-equal members: 43).
//
// Memory: n x n u64 (rows padded to an even count: 16-byte aligned), 800 MB at 10 000 sketches, 34 GB at the limit
// HG_CLUSTER_AVERAGE_MAX_N; allocated per call and released before the call returns.  hg_cluster_average_dev fills the upper
// triangle from row blocks of hg_dist_full_dev (rows [r0, r1) x columns [r0, n) in the search's scratch block, at most
// HG_SEARCH_BLOCK_BYTES; "average_block_rows" forces the row count) and mirrors it, so that every row scan is contiguous.
#include <algorithm>

#include "hg_average_cmp.h"
#include "hg_block_scan.h"
#include "hg_cluster_common.h"
#include "hg_internal.h"

namespace {
constexpr uint64_t AVG_DEFAULT_ROUNDS = 4;  // rounds queued per readback of the merge count
constexpr uint32_t AVG_NONE = 0xFFFFFFFFu;
constexpr uint32_t AVG_MERGED = HG_CLU_UNDECIDED;  // result words [2], [3]: merges of the odd / even rounds
constexpr uint32_t MIRROR_TILE = 32;

struct Average {
  uint64_t *M;       // n rows of ld sums
  size_t ld;         // n rounded up to an even count
  uint32_t *nn;      // n: best partner of the round, AVG_NONE = none (dead rows too)
  uint32_t *partner; // n: the name absorbed into this one in this round, else AVG_NONE
  uint32_t *cnt;     // n: c(A) of a live name, 0 of an absorbed one
  uint32_t *msize;   // n: size[] of an absorbed name
  float *level;      // n: level[] of an absorbed name
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

// res[AVG_MERGED] (the count "of the round before" the first one) is made non-zero
__global__ __launch_bounds__(256) void average_init_kernel(uint32_t *__restrict__ rep, uint32_t *__restrict__ nn, uint32_t *__restrict__ partner,
                                                           uint32_t *__restrict__ cnt, uint32_t *__restrict__ msize, float *__restrict__ level,
                                                           uint32_t n, uint32_t *__restrict__ res) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    rep[i] = (uint32_t)i, nn[i] = AVG_NONE, partner[i] = AVG_NONE, cnt[i] = 1u, msize[i] = 1u, level[i] = 0.0f;
  if (blockIdx.x == 0 && threadIdx.x < HG_CLU_WORDS) res[threadIdx.x] = threadIdx.x == AVG_MERGED ? 1u : 0u;
}

// Rows [r0, r0 + rows) of the matrix from a block of ANI values: blk[r * pitch + (j - c0)] is ani(r0 + r, j), c0 <= r0.
// Only j > row is read; the diagonal, the lower triangle (the mirror kernel writes it) and the padding column become 0.
__global__ __launch_bounds__(256) void average_fill_kernel(const float *__restrict__ blk, size_t pitch, uint32_t c0, uint32_t r0, uint32_t rows,
                                                           uint32_t n, size_t ld, uint64_t *__restrict__ M) {
  for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const uint32_t gi = r0 + r;
    const float *src = blk + (size_t)r * pitch;
    uint64_t *dst = M + (size_t)gi * ld;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < ld; j += (size_t)gridDim.x * blockDim.x)
      dst[j] = (j > gi && j < n) ? hg_avg_milli(src[j - c0]) : 0ull;
  }
}

// M[j][i] = M[i][j] for i < j: tiles of 32 x 32 through LDS, the workgroups of the upper triangle of tiles each write
// their transposed tile (a diagonal tile its own lower half).  blockDim = (32, 8).
__global__ __launch_bounds__(256) void average_mirror_kernel(uint64_t *M, uint32_t n, size_t ld) {
  __shared__ uint64_t tile[MIRROR_TILE][MIRROR_TILE + 1];
  if (blockIdx.x < blockIdx.y) return;  // (uniform over the workgroup)
  const uint32_t row0 = blockIdx.y * MIRROR_TILE, col0 = blockIdx.x * MIRROR_TILE;
  for (uint32_t k = threadIdx.y; k < MIRROR_TILE; k += 8) {
    const uint32_t i = row0 + k, j = col0 + threadIdx.x;
    tile[k][threadIdx.x] = (i < n && j < n) ? M[(size_t)i * ld + j] : 0ull;
  }
  __syncthreads();
  for (uint32_t k = threadIdx.y; k < MIRROR_TILE; k += 8) {
    const uint32_t j = col0 + k, i = row0 + threadIdx.x;  // writes M[j][i], the value of M[i][j]
    if (j < n && i < j) M[(size_t)j * ld + i] = tile[threadIdx.x][k];
  }
}

struct Cand {
  uint64_t s;   // S(A, B)
  uint32_t c;   // c(B)
  uint32_t b;   // B, AVG_NONE = no candidate
};
// the better partner of one row: the larger S / c, ties to the smaller name
__device__ __forceinline__ bool cand_better(const Cand &x, const Cand &y) {
  if (x.b == AVG_NONE) return false;
  if (y.b == AVG_NONE) return true;
  const int o = hg_avg_compare(x.s, x.c, y.s, y.c);
  return o > 0 || (o == 0 && x.b < y.b);
}

// One workgroup per row.  res[AVG_MERGED + parity]: the count of the previous round is read (0: the last round merged
// nothing, the call is resolved), the one of this round is cleared for average_pair_kernel behind the launch boundary.
__global__ __launch_bounds__(256) void average_best_kernel(const uint64_t *__restrict__ M, size_t ld, uint32_t n,
                                                           const uint32_t *__restrict__ cnt, uint64_t th_milli, uint32_t *__restrict__ nn,
                                                           uint32_t *res, uint32_t round) {
  __shared__ uint64_t s_s[256];
  __shared__ uint32_t s_c[256], s_b[256];
  const uint32_t merged_before = res[AVG_MERGED + ((round - 1u) & 1u)];
  if (blockIdx.x == 0 && threadIdx.x == 0) res[AVG_MERGED + (round & 1u)] = 0u;
  if (merged_before == 0u) return;  // (uniform over the grid: nobody writes that word in this launch)
  const uint32_t A = blockIdx.x, t = threadIdx.x;
  const uint32_t cA = cnt[A];
  if (cA == 0u) {  // absorbed: nobody's partner, and no partner of its own
    if (t == 0) nn[A] = AVG_NONE;
    return;
  }
  const uint64_t *row = M + (size_t)A * ld;
  const uint64_t need = th_milli * cA;  // S >= th_milli c(A) c(B): below 2^47
  Cand best{0ull, 0u, AVG_NONE};
  // two columns per lane and step (ld is even: j + 1 < ld, and the row starts on 16 bytes)
  for (uint32_t j = 2u * t; j < n; j += 512u) {
    const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(row + j);
    const uint32_t c0 = cnt[j], c1 = j + 1u < n ? cnt[j + 1u] : 0u;
    if (c0 != 0u && j != A && v.x >= need * c0) {
      const Cand x{v.x, c0, j};
      if (cand_better(x, best)) best = x;
    }
    if (c1 != 0u && j + 1u != A && v.y >= need * c1) {
      const Cand x{v.y, c1, j + 1u};
      if (cand_better(x, best)) best = x;
    }
  }
  s_s[t] = best.s, s_c[t] = best.c, s_b[t] = best.b;
  __syncthreads();
  for (uint32_t step = 128u; step >= 1u; step >>= 1) {
    if (t < step) {
      const Cand x{s_s[t + step], s_c[t + step], s_b[t + step]}, y{s_s[t], s_c[t], s_b[t]};
      if (cand_better(x, y)) s_s[t] = x.s, s_c[t] = x.c, s_b[t] = x.b;
    }
    __syncthreads();
  }
  if (t == 0) nn[A] = s_b[0];
}

// One lane per node.  nn[] is this round's for every node (average_best_kernel wrote all of them), and a merged pair's
// words -- cnt, rep, msize, level of its two names -- are touched by the lane of its lower name alone: mutual pairs are
// disjoint, and no other lane reads cnt of a name that is not its own or its mutual partner's.
__global__ __launch_bounds__(256) void average_pair_kernel(const uint64_t *__restrict__ M, size_t ld, uint32_t n, const uint32_t *__restrict__ nn,
                                                           uint32_t *__restrict__ partner, uint32_t *cnt, uint32_t *rep, uint32_t *msize,
                                                           float *level, uint32_t *res, uint32_t round) {
  __shared__ uint32_t s_wave[4];
  if (res[AVG_MERGED + ((round - 1u) & 1u)] == 0u) return;  // (uniform over the grid)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t merged = 0;
  if (i < n) {
    const uint32_t A = (uint32_t)i, B = nn[A];
    uint32_t p = AVG_NONE;
    if (B != AVG_NONE && B < n && B > A && nn[B] == A) {
      const uint32_t cA = cnt[A], cB = cnt[B];
      const uint64_t S = M[(size_t)A * ld + B];
      level[B] = (float)(((double)S / (double)((uint64_t)cA * cB)) / 1000.0);
      msize[B] = cA + cB, rep[B] = A;
      cnt[A] = cA + cB, cnt[B] = 0u;
      p = B, merged = 1;
    }
    partner[A] = p;
  }
  uint32_t total;
  (void)block_excl_scan<4>(merged, s_wave, &total);
  if (threadIdx.x == 0) {
    if (total) __hip_atomic_fetch_add(res + AVG_MERGED + (round & 1u), total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (blockIdx.x == 0) res[HG_CLU_ROUNDS] += 1u;  // (this lane alone touches the word in this launch)
  }
}

// One workgroup per node: the lower name of a merged pair adds the absorbed row to its own (whole rows, padding included).
__global__ __launch_bounds__(256) void average_rows_kernel(uint64_t *M, size_t ld, const uint32_t *__restrict__ partner,
                                                           const uint32_t *__restrict__ res, uint32_t round) {
  if (res[AVG_MERGED + (round & 1u)] == 0u) return;  // (this round's count: final behind average_pair_kernel's launch)
  const uint32_t A = blockIdx.x, B = partner[A];
  if (B == AVG_NONE) return;
  ulonglong2 *a = reinterpret_cast<ulonglong2 *>(M + (size_t)A * ld);
  const ulonglong2 *b = reinterpret_cast<const ulonglong2 *>(M + (size_t)B * ld);
  for (size_t j = threadIdx.x; j < ld / 2; j += 256) {
    ulonglong2 x = a[j];
    const ulonglong2 y = b[j];
    x.x += y.x, x.y += y.y;
    a[j] = x;
  }
}

// One workgroup per surviving row: for every merged pair the absorbed column is added to the one that stays.
__global__ __launch_bounds__(256) void average_cols_kernel(uint64_t *M, size_t ld, uint32_t n, const uint32_t *__restrict__ partner,
                                                           const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ res, uint32_t round) {
  if (res[AVG_MERGED + (round & 1u)] == 0u) return;
  const uint32_t R = blockIdx.x;
  if (cnt[R] == 0u) return;
  uint64_t *row = M + (size_t)R * ld;
  for (uint32_t j = threadIdx.x; j < n; j += 256u) {
    const uint32_t B = partner[j];
    if (B != AVG_NONE) row[j] += row[B];  // (B < n: average_pair_kernel checked it; row[B] is written by nobody)
  }
}

// the dendrogram arrays the caller asked for, from rep[] before hg_cluster_queue_ids flattens it
__global__ __launch_bounds__(256) void average_emit_kernel(const uint32_t *__restrict__ rep, const uint32_t *__restrict__ cnt,
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

hg_status average_too_large(hg_ctx *c) {
  return hg_fail(c, HG_ERR_UNSUPPORTED, "average linkage holds the dense matrix: n must be <= HG_CLUSTER_AVERAGE_MAX_N (65536)");
}

// per-node state in w_average, the matrix in `hold`, everything initialised (stream-ordered)
hg_status average_begin(hg_ctx *c, size_t n, uint32_t *d_rep, Average &g, MatrixHold &hold) {
  hg_status s;
  if ((s = hg_cluster_res(c, &g.res)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_average, n * 20 + 64)) != HG_OK) return s;
  g.nn = static_cast<uint32_t *>(c->w_average.p);
  g.partner = g.nn + n, g.cnt = g.partner + n, g.msize = g.cnt + n;
  g.level = reinterpret_cast<float *>(g.msize + n);
  g.ld = (n + 1) & ~(size_t)1;
  const size_t bytes = n * g.ld * sizeof(uint64_t);
  const hipError_t e = hipMalloc(&hold.p, bytes);
  if (e != hipSuccess) {
    hold.p = nullptr;
    return hg_fail(c, HG_ERR_OOM, "hipMalloc(" + std::to_string(bytes) + ") for the matrix of average linkage: " + hipGetErrorString(e));
  }
  g.M = static_cast<uint64_t *>(hold.p);
  c->average_rounds = 0;
  hg_timed tm(c, HG_T_DIST);
  hipLaunchKernelGGL(average_init_kernel, dim3(grid_for(c, n)), dim3(256), 0, c->stream, d_rep, g.nn, g.partner, g.cnt, g.msize, g.level,
                     (uint32_t)n, g.res);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

// rows [r0, r0 + rows) from a block of ANI values (average_fill_kernel)
hg_status average_fill(hg_ctx *c, const Average &g, const float *blk, size_t pitch, size_t c0, size_t r0, size_t rows, size_t n) {
  hg_timed tm(c, HG_T_DIST);
  const dim3 grid((unsigned)std::min<size_t>((g.ld + 255) / 256, 64), (unsigned)std::min<size_t>(rows, 16384));
  hipLaunchKernelGGL(average_fill_kernel, grid, dim3(256), 0, c->stream, blk, pitch, (uint32_t)c0, (uint32_t)r0, (uint32_t)rows, (uint32_t)n,
                     g.ld, g.M);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

// the filled upper triangle -> mirror, rounds until one merges nothing, the dendrogram, dense ids, the result words back
hg_status average_resolve(hg_ctx *c, Average &g, size_t n, float ani_th, uint32_t *d_rep, uint32_t *d_cluster, uint32_t *d_into,
                          float *d_level, uint32_t *d_size, size_t *n_clusters) {
  hg_status s;
  const uint32_t m = (uint32_t)n;
  {
    hg_timed tm(c, HG_T_DIST);
    const unsigned tiles = (unsigned)((n + MIRROR_TILE - 1) / MIRROR_TILE);
    hipLaunchKernelGGL(average_mirror_kernel, dim3(tiles, tiles), dim3(MIRROR_TILE, 8), 0, c->stream, g.M, m, g.ld);
    HG_HIP(c, hipGetLastError());
  }
  const bool merges = ani_th == ani_th && !(ani_th > 100.0f);  // (a NaN threshold, one above 100: nothing merges)
  const uint64_t th_milli = hg_avg_milli(ani_th);
  const uint64_t per = c->dbg_average_rounds ? c->dbg_average_rounds : AVG_DEFAULT_ROUNDS;
  const dim3 row_grid((unsigned)n), node_grid((unsigned)((n + 255) / 256));
  while (merges) {
    {
      hg_timed tm(c, HG_T_DIST);
      for (uint64_t k = 0; k < per; ++k) {
        const uint32_t r = ++g.round;
        hipLaunchKernelGGL(average_best_kernel, row_grid, dim3(256), 0, c->stream, g.M, g.ld, m, g.cnt, th_milli, g.nn, g.res, r);
        HG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(average_pair_kernel, node_grid, dim3(256), 0, c->stream, g.M, g.ld, m, g.nn, g.partner, g.cnt, d_rep, g.msize,
                           g.level, g.res, r);
        HG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(average_rows_kernel, row_grid, dim3(256), 0, c->stream, g.M, g.ld, g.partner, g.res, r);
        HG_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(average_cols_kernel, row_grid, dim3(256), 0, c->stream, g.M, g.ld, m, g.partner, g.cnt, g.res, r);
        HG_HIP(c, hipGetLastError());
      }
    }
    const uint32_t *h_res = nullptr;
    if ((s = hg_publish_words(c, g.res, HG_CLU_WORDS, &h_res)) != HG_OK) return s;  // (nothing cleared: the call goes on)
    if (h_res[AVG_MERGED + (g.round & 1u)] == 0u) break;
  }
  if (d_into || d_level || d_size) {
    hg_timed tm(c, HG_T_DIST);
    hipLaunchKernelGGL(average_emit_kernel, dim3(grid_for(c, n)), dim3(256), 0, c->stream, d_rep, g.cnt, g.msize, g.level, m, d_into, d_level,
                       d_size);
    HG_HIP(c, hipGetLastError());
  }
  if ((s = hg_cluster_queue_ids(c, d_rep, n, d_cluster, g.res)) != HG_OK) return s;
  return hg_cluster_close(c, g.res, &c->average_rounds, "hg_cluster_average_matrix_dev", n_clusters);
}
}  // namespace

extern "C" uint64_t hg_ctx_cluster_average_rounds(const hg_ctx *c) { return c ? c->average_rounds : 0; }

extern "C" hg_status hg_cluster_average_matrix_dev(hg_ctx *c, const float *d_ani, size_t n, float ani_th, uint32_t *d_rep, uint32_t *d_cluster,
                                                   uint32_t *d_into, float *d_level, uint32_t *d_size, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_cluster_check(c, n, n_clusters, false);
  if (s != HG_OK) return s;
  if (n > HG_CLUSTER_AVERAGE_MAX_N) return average_too_large(c);
  if (n == 0) return HG_OK;
  if (!d_ani || !d_rep || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  Average g{};
  MatrixHold hold;
  if ((s = average_begin(c, n, d_rep, g, hold)) != HG_OK) return s;
  if ((s = average_fill(c, g, d_ani, n, 0, 0, n, n)) != HG_OK) return s;
  return average_resolve(c, g, n, ani_th, d_rep, d_cluster, d_into, d_level, d_size, n_clusters);
}

extern "C" hg_status hg_cluster_average_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                            float ani_th, uint32_t *d_rep, uint32_t *d_cluster, uint32_t *d_into, float *d_level,
                                            uint32_t *d_size, size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_cluster_check(c, n, n_clusters, true);
  if (s != HG_OK) return s;
  if (n > HG_CLUSTER_AVERAGE_MAX_N) return average_too_large(c);
  if (n == 0) return HG_OK;
  if (!d_hv || !d_norm2 || !d_rep || !d_cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (hv_d == 0 || hv_d > 65536) return hg_fail(c, HG_ERR_UNSUPPORTED, "hv_d must be in 1..65536");
  if (ksize == 0) return hg_fail(c, HG_ERR_INVALID, "ksize must be >= 1");
  HG_ENTER(c);
  // the scratch block: rows [r0, r0 + rb) x columns [r0, n) of the ANI matrix, the first block being the widest
  const size_t fit = std::max<size_t>(1, HG_SEARCH_BLOCK_BYTES / (sizeof(float) * n));
  const size_t rb = std::min<size_t>(n, c->dbg_average_block_rows ? (size_t)c->dbg_average_block_rows : fit);
  if ((s = hg_ensure(c, c->w_srch_blk, rb * n * sizeof(float))) != HG_OK) return s;
  auto *blk = static_cast<float *>(c->w_srch_blk.p);
  Average g{};
  MatrixHold hold;
  if ((s = average_begin(c, n, d_rep, g, hold)) != HG_OK) return s;
  for (size_t r0 = 0; r0 < n; r0 += rb) {
    const size_t rows = std::min(rb, n - r0), cols = n - r0;
    if ((s = hg_dist_full_dev(c, d_hv + r0 * (size_t)hv_d, d_norm2 + r0, rows, d_hv + r0 * (size_t)hv_d, d_norm2 + r0, cols, hv_d, ksize,
                              blk)) != HG_OK)
      return s;
    if ((s = average_fill(c, g, blk, cols, r0, r0, rows, n)) != HG_OK) return s;
  }
  return average_resolve(c, g, n, ani_th, d_rep, d_cluster, d_into, d_level, d_size, n_clusters);
}

extern "C" hg_status hg_cluster_average(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                        float ani_th, uint32_t *rep, uint32_t *cluster, uint32_t *into, float *level, uint32_t *size,
                                        size_t *n_clusters) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_cluster_check(c, n, n_clusters, true);
  if (s != HG_OK) return s;
  if (n > HG_CLUSTER_AVERAGE_MAX_N) return average_too_large(c);
  if (n == 0) return HG_OK;
  if (!hv || !norm2 || !rep || !cluster) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  const int16_t *d_hv;
  const int32_t *d_norm2;
  uint32_t *d_rep;
  if ((s = hg_cluster_stage(c, hv, norm2, n, hv_d, 5 * n * sizeof(uint32_t), &d_hv, &d_norm2, &d_rep)) != HG_OK) return s;
  uint32_t *d_cluster = d_rep + n, *d_into = d_cluster + n, *d_size = d_into + n;
  auto *d_level = reinterpret_cast<float *>(d_size + n);
  if ((s = hg_cluster_average_dev(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, d_rep, d_cluster, into ? d_into : nullptr, level ? d_level : nullptr,
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
