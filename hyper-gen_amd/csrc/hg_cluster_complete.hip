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
//
// The matrix, its fill and mirror and the row blocks are hg_dense_matrix.h's; the round loop, the pair, rows, cols and emit
// passes and the three forms of the call are hg_linkage_rounds.h's, shared with average linkage.  Here: what a merge does
// to two minima (CompleteOp), the best kernel with its rescan rule, and the kernels' names.
#include "hg_linkage_rounds.h"

namespace {
constexpr uint32_t SCAN_STEP = 1024;  // columns one step of the row scan covers: 256 lanes x 4

struct CompleteOp {
  using T = uint32_t;  // W(A, B); ld per-node entries, rows of a multiple of 4
  using V = uint4;
  static __device__ __forceinline__ T comb(T a, T b) { return min(a, b); }
  static __device__ __forceinline__ float level(T W, uint32_t, uint32_t) { return (float)((double)W / 1000.0); }
};
struct CompleteMilli {
  __device__ __forceinline__ uint32_t operator()(float ani) const { return (uint32_t)hg_avg_milli(ani); }
};

__global__ __launch_bounds__(256) void complete_init_kernel(uint32_t *__restrict__ rep, uint32_t *__restrict__ nn, uint32_t *__restrict__ partner,
                                                            uint32_t *__restrict__ cnt, uint32_t *__restrict__ msize, float *__restrict__ level,
                                                            uint32_t n, uint32_t ld, uint32_t *__restrict__ res) {
  linkage_init_body(rep, nn, partner, cnt, msize, level, n, ld, res, HG_LANE0, HG_LANES);
}
__global__ __launch_bounds__(256) void complete_fill_kernel(const float *__restrict__ blk, size_t pitch, uint32_t c0, uint32_t r0, uint32_t rows,
                                                            uint32_t n, size_t ld, uint32_t *__restrict__ M) {
  matrix_fill_body<uint32_t, CompleteMilli>(blk, pitch, c0, r0, rows, n, ld, M, HG_LANE0, HG_LANES);
}
__global__ __launch_bounds__(256) void complete_mirror_kernel(uint32_t *M, uint32_t n, size_t ld) { matrix_mirror_body(M, n, ld); }

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

// One workgroup per row.  res[LINKAGE_MERGED + parity]: the count of the previous round is read (0: the last round merged
// nothing, the call is resolved), the one of this round is cleared for complete_pair_kernel behind the launch boundary.
// nn[A] is read and written by the workgroup of A alone; partner[] and cnt[] are the previous round's, final.
__global__ __launch_bounds__(256) void complete_best_kernel(const uint32_t *__restrict__ M, size_t ld, uint32_t n,
                                                            const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ partner,
                                                            uint32_t th_milli, uint32_t *nn, uint32_t *res, uint32_t round,
                                                            uint32_t rescan_all) {
  __shared__ uint64_t s_best[4];
  const uint32_t merged_before = res[LINKAGE_MERGED + ((round - 1u) & 1u)];
  if (blockIdx.x == 0 && threadIdx.x == 0) res[LINKAGE_MERGED + (round & 1u)] = 0u;
  if (merged_before == 0u) return;  // (uniform over the grid: nobody writes that word in this launch)
  const uint32_t A = blockIdx.x, t = threadIdx.x;
  if (cnt[A] == 0u) {  // absorbed: nobody's partner, and no partner of its own
    if (t == 0) nn[A] = DENSE_NONE;
    return;
  }
  if (round >= 2u && !rescan_all) {  // (uniform over the workgroup: every lane reads the same words)
    const uint32_t B = nn[A];
    if (B == DENSE_NONE) return;  // retired: values only fall
    if (partner[A] == DENSE_NONE && cnt[B] != 0u && partner[B] == DENSE_NONE) return;  // neither end merged: B is still the best
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
    nn[A] = best ? 0xFFFFFFFFu - (uint32_t)best : DENSE_NONE;
  }
}

__global__ __launch_bounds__(256) void complete_pair_kernel(const uint32_t *__restrict__ M, size_t ld, uint32_t n, const uint32_t *__restrict__ nn,
                                                            uint32_t *__restrict__ partner, uint32_t *cnt, uint32_t *rep, uint32_t *msize,
                                                            float *level, uint32_t *res, uint32_t round) {
  linkage_pair_body<CompleteOp>(M, ld, n, nn, partner, cnt, rep, msize, level, res, round);
}
__global__ __launch_bounds__(256) void complete_rows_kernel(uint32_t *M, size_t ld, const uint32_t *__restrict__ partner,
                                                            const uint32_t *__restrict__ res, uint32_t round) {
  linkage_rows_body<CompleteOp>(M, ld, partner, res, round);
}
__global__ __launch_bounds__(256) void complete_cols_kernel(uint32_t *M, size_t ld, uint32_t n, const uint32_t *__restrict__ partner,
                                                            const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ res, uint32_t round) {
  linkage_cols_body<CompleteOp>(M, ld, n, partner, cnt, res, round);
}
__global__ __launch_bounds__(256) void complete_emit_kernel(const uint32_t *__restrict__ rep, const uint32_t *__restrict__ cnt,
                                                            const uint32_t *__restrict__ msize, const float *__restrict__ level, uint32_t n,
                                                            uint32_t *__restrict__ into, float *__restrict__ level_out, uint32_t *__restrict__ size_out) {
  linkage_emit_body(rep, cnt, msize, level, n, into, level_out, size_out, HG_LANE0, HG_LANES);
}

struct CompleteLinkage : CompleteOp {
  static constexpr const char *scheme = "complete linkage", *hits_fn = "hg_cluster_complete_matrix_dev";
  static constexpr const char *too_large = "complete linkage holds the dense matrix: n must be <= HG_CLUSTER_COMPLETE_MAX_N (65536)";
  static constexpr size_t max_n = HG_CLUSTER_COMPLETE_MAX_N;
  static constexpr bool padded_nodes = true;
  static constexpr auto buf = &hg_ctx::w_complete;
  static constexpr auto rounds = &hg_ctx::complete_rounds, dbg_rounds = &hg_ctx::dbg_complete_rounds,
                        dbg_block_rows = &hg_ctx::dbg_complete_block_rows;
  static constexpr auto init_kernel = complete_init_kernel;
  static constexpr auto fill_kernel = complete_fill_kernel;
  static constexpr auto mirror_kernel = complete_mirror_kernel;
  static constexpr auto pair_kernel = complete_pair_kernel;
  static constexpr auto rows_kernel = complete_rows_kernel;
  static constexpr auto cols_kernel = complete_cols_kernel;
  static constexpr auto emit_kernel = complete_emit_kernel;
  static void launch_best(hg_ctx *c, const Linkage<T> &g, dim3 row_grid, uint32_t n, uint64_t th_milli, uint32_t round) {
    hipLaunchKernelGGL(complete_best_kernel, row_grid, dim3(256), 0, c->stream, g.M, g.ld, n, g.cnt, g.partner, (uint32_t)th_milli, g.nn, g.res,
                       round, c->dbg_complete_rescan_all ? 1u : 0u);
  }
};
}  // namespace

extern "C" uint64_t hg_ctx_cluster_complete_rounds(const hg_ctx *c) { return c ? c->complete_rounds : 0; }

extern "C" hg_status hg_cluster_complete_matrix_dev(hg_ctx *c, const float *d_ani, size_t n, float ani_th, uint32_t *d_rep, uint32_t *d_cluster,
                                                    uint32_t *d_into, float *d_level, uint32_t *d_size, size_t *n_clusters) {
  return linkage_matrix_dev<CompleteLinkage>(c, d_ani, n, ani_th, d_rep, d_cluster, d_into, d_level, d_size, n_clusters);
}

extern "C" hg_status hg_cluster_complete_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                             float ani_th, uint32_t *d_rep, uint32_t *d_cluster, uint32_t *d_into, float *d_level,
                                             uint32_t *d_size, size_t *n_clusters) {
  return linkage_dev<CompleteLinkage>(c, d_hv, d_norm2, n, hv_d, ksize, ani_th, d_rep, d_cluster, d_into, d_level, d_size, n_clusters);
}

extern "C" hg_status hg_cluster_complete(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                         float ani_th, uint32_t *rep, uint32_t *cluster, uint32_t *into, float *level, uint32_t *size,
                                         size_t *n_clusters) {
  return linkage_host<CompleteLinkage>(c, hv, norm2, n, hv_d, ksize, ani_th, rep, cluster, into, level, size, n_clusters);
}
