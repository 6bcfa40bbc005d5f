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
//
// The matrix, its fill and mirror and the row blocks are hg_dense_matrix.h's; the round loop, the pair, rows, cols and emit
// passes and the three forms of the call are hg_linkage_rounds.h's, shared with complete linkage.  Here: what a merge does
// to two sums (AverageOp), the best kernel, and the kernels' names.
#include "hg_linkage_rounds.h"

namespace {
struct AverageOp {
  using T = uint64_t;    // S(A, B); n per-node entries, rows of an even count
  using V = ulonglong2;
  static __device__ __forceinline__ T comb(T a, T b) { return a + b; }
  static __device__ __forceinline__ float level(T S, uint32_t cA, uint32_t cB) {
    return (float)(((double)S / (double)((uint64_t)cA * cB)) / 1000.0);
  }
};
struct AverageMilli {
  __device__ __forceinline__ uint64_t operator()(float ani) const { return hg_avg_milli(ani); }
};

__global__ __launch_bounds__(256) void average_init_kernel(uint32_t *__restrict__ rep, uint32_t *__restrict__ nn, uint32_t *__restrict__ partner,
                                                           uint32_t *__restrict__ cnt, uint32_t *__restrict__ msize, float *__restrict__ level,
                                                           uint32_t n, uint32_t *__restrict__ res) {
  linkage_init_body(rep, nn, partner, cnt, msize, level, n, n, res, HG_LANE0, HG_LANES);
}
__global__ __launch_bounds__(256) void average_fill_kernel(const float *__restrict__ blk, size_t pitch, uint32_t c0, uint32_t r0, uint32_t rows,
                                                           uint32_t n, size_t ld, uint64_t *__restrict__ M) {
  matrix_fill_body<uint64_t, AverageMilli>(blk, pitch, c0, r0, rows, n, ld, M, HG_LANE0, HG_LANES);
}
__global__ __launch_bounds__(256) void average_mirror_kernel(uint64_t *M, uint32_t n, size_t ld) { matrix_mirror_body(M, n, ld); }

struct Cand {
  uint64_t s;   // S(A, B)
  uint32_t c;   // c(B)
  uint32_t b;   // B, DENSE_NONE = no candidate
};
// the better partner of one row: the larger S / c, ties to the smaller name
__device__ __forceinline__ bool cand_better(const Cand &x, const Cand &y) {
  if (x.b == DENSE_NONE) return false;
  if (y.b == DENSE_NONE) return true;
  const int o = hg_avg_compare(x.s, x.c, y.s, y.c);
  return o > 0 || (o == 0 && x.b < y.b);
}

// One workgroup per row.  res[LINKAGE_MERGED + parity]: the count of the previous round is read (0: the last round merged
// nothing, the call is resolved), the one of this round is cleared for average_pair_kernel behind the launch boundary.
__global__ __launch_bounds__(256) void average_best_kernel(const uint64_t *__restrict__ M, size_t ld, uint32_t n,
                                                           const uint32_t *__restrict__ cnt, uint64_t th_milli, uint32_t *__restrict__ nn,
                                                           uint32_t *res, uint32_t round) {
  __shared__ uint64_t s_s[256];
  __shared__ uint32_t s_c[256], s_b[256];
  const uint32_t merged_before = res[LINKAGE_MERGED + ((round - 1u) & 1u)];
  if (blockIdx.x == 0 && threadIdx.x == 0) res[LINKAGE_MERGED + (round & 1u)] = 0u;
  if (merged_before == 0u) return;  // (uniform over the grid: nobody writes that word in this launch)
  const uint32_t A = blockIdx.x, t = threadIdx.x;
  const uint32_t cA = cnt[A];
  if (cA == 0u) {  // absorbed: nobody's partner, and no partner of its own
    if (t == 0) nn[A] = DENSE_NONE;
    return;
  }
  const uint64_t *row = M + (size_t)A * ld;
  const uint64_t need = th_milli * cA;  // S >= th_milli c(A) c(B): below 2^47
  Cand best{0ull, 0u, DENSE_NONE};
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

__global__ __launch_bounds__(256) void average_pair_kernel(const uint64_t *__restrict__ M, size_t ld, uint32_t n, const uint32_t *__restrict__ nn,
                                                           uint32_t *__restrict__ partner, uint32_t *cnt, uint32_t *rep, uint32_t *msize,
                                                           float *level, uint32_t *res, uint32_t round) {
  linkage_pair_body<AverageOp>(M, ld, n, nn, partner, cnt, rep, msize, level, res, round);
}
__global__ __launch_bounds__(256) void average_rows_kernel(uint64_t *M, size_t ld, const uint32_t *__restrict__ partner,
                                                           const uint32_t *__restrict__ res, uint32_t round) {
  linkage_rows_body<AverageOp>(M, ld, partner, res, round);
}
__global__ __launch_bounds__(256) void average_cols_kernel(uint64_t *M, size_t ld, uint32_t n, const uint32_t *__restrict__ partner,
                                                           const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ res, uint32_t round) {
  linkage_cols_body<AverageOp>(M, ld, n, partner, cnt, res, round);
}
__global__ __launch_bounds__(256) void average_emit_kernel(const uint32_t *__restrict__ rep, const uint32_t *__restrict__ cnt,
                                                           const uint32_t *__restrict__ msize, const float *__restrict__ level, uint32_t n,
                                                           uint32_t *__restrict__ into, float *__restrict__ level_out, uint32_t *__restrict__ size_out) {
  linkage_emit_body(rep, cnt, msize, level, n, into, level_out, size_out, HG_LANE0, HG_LANES);
}

struct AverageLinkage : AverageOp {
  static constexpr const char *scheme = "average linkage", *hits_fn = "hg_cluster_average_matrix_dev";
  static constexpr const char *too_large = "average linkage holds the dense matrix: n must be <= HG_CLUSTER_AVERAGE_MAX_N (65536)";
  static constexpr size_t max_n = HG_CLUSTER_AVERAGE_MAX_N;
  static constexpr bool padded_nodes = false;
  static constexpr auto buf = &hg_ctx::w_average;
  static constexpr auto rounds = &hg_ctx::average_rounds, dbg_rounds = &hg_ctx::dbg_average_rounds,
                        dbg_block_rows = &hg_ctx::dbg_average_block_rows;
  static constexpr auto init_kernel = average_init_kernel;
  static constexpr auto fill_kernel = average_fill_kernel;
  static constexpr auto mirror_kernel = average_mirror_kernel;
  static constexpr auto pair_kernel = average_pair_kernel;
  static constexpr auto rows_kernel = average_rows_kernel;
  static constexpr auto cols_kernel = average_cols_kernel;
  static constexpr auto emit_kernel = average_emit_kernel;
  static void launch_best(hg_ctx *c, const Linkage<T> &g, dim3 row_grid, uint32_t n, uint64_t th_milli, uint32_t round) {
    hipLaunchKernelGGL(average_best_kernel, row_grid, dim3(256), 0, c->stream, g.M, g.ld, n, g.cnt, th_milli, g.nn, g.res, round);
  }
};
}  // namespace

extern "C" uint64_t hg_ctx_cluster_average_rounds(const hg_ctx *c) { return c ? c->average_rounds : 0; }

extern "C" hg_status hg_cluster_average_matrix_dev(hg_ctx *c, const float *d_ani, size_t n, float ani_th, uint32_t *d_rep, uint32_t *d_cluster,
                                                   uint32_t *d_into, float *d_level, uint32_t *d_size, size_t *n_clusters) {
  return linkage_matrix_dev<AverageLinkage>(c, d_ani, n, ani_th, d_rep, d_cluster, d_into, d_level, d_size, n_clusters);
}

extern "C" hg_status hg_cluster_average_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                            float ani_th, uint32_t *d_rep, uint32_t *d_cluster, uint32_t *d_into, float *d_level,
                                            uint32_t *d_size, size_t *n_clusters) {
  return linkage_dev<AverageLinkage>(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, d_rep, d_cluster, d_into, d_level, d_size, n_clusters);
}

extern "C" hg_status hg_cluster_average(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                        float ani_th, uint32_t *rep, uint32_t *cluster, uint32_t *into, float *level, uint32_t *size,
                                        size_t *n_clusters) {
  return linkage_host<AverageLinkage>(c, hv, norm2, n, hv_d, ksize, ani_th, rep, cluster, into, level, size, n_clusters);
}
