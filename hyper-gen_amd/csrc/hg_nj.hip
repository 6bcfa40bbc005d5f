// hg_nj.hip -- neighbour-joining tree of sketches (an extension: what mashtree, `mash triangle | rapidnj` and the
// dendrogram step of pyani and dRep reports draw from an all-pairs table).  Like the matrix schemes of clustering it
// decides on integers only, so that anyone can reproduce the tree from a `dist -a 0` TSV:
//   m(i, j) = the integer `dist` prints for ani(i, j), in thousandths (hg_avg_milli: NaN and negative 0, above 100 100 000);
//   d(i, j) = (100 000 - m(i, j)) << HG_NJ_FRAC_BITS: fixed point, one unit = 2^-15 thousandths of an ANI percent; u32;
//   a node is named by an index, a joined node keeps the smaller of its children's names; c = the live count;
//   while c >= 3: r(i) = the sum of d(i, k) over live k != i; Q(i, j) = (c - 2) d(i, j) - r(i) - r(j) in signed 64 bits;
//     the pair a < b with the minimum (Q, i, j), compared lexicographically, joins; D = d(a, b),
//     len_a = floor(((c - 2) D + r(a) - r(b)) / (2 (c - 2))), len_b = D - len_a (either may be negative, neither is clamped);
//     d(a, k) = max(0, (d(a, k) + d(b, k) - D) >> 1) for every live k other than a and b; b dies;
//   at c = 2 the two live names a < b give the last join (a, b, d(a, b), 0).
// The three formulas are hg_nj_math.h's.  Neighbour joining is not reducible -- a join changes every Q through r() and
// c --, so unlike the mutual-best-partner rounds of average and complete linkage this is ONE join per round, n - 2 rounds
// and the last join, all queued ahead without a readback: the host knows c = n - t, it is a launch argument.
// Per round:
//   * nj_best_kernel   : one workgroup per row; a dead row exits.  A live row i scans the columns j > i only -- from the
//                        16-byte piece that holds i + 1, columns j <= i and dead columns masked -- with 16-byte loads of the
//                        row and of live[] and r[j] beside them: the minimum of (c - 2) d - r(j), ties to the smaller j (one
//                        signed compare and an index compare), by wave shuffles and a few LDS words; writes (Q, j) of the row.
//                        Half the traffic of a full-row scan, and the global tie-break is a plain minimum of (Q, i, j).
//   * nj_pick_kernel   : one workgroup: the minimum of the row results, join t, live[b] = 0, r[a] = 0.
//   * nj_update_kernel : one lane per k: reads rows a and b, writes M[a][k] and M[k][a], r[k] += new - d(a, k) - d(b, k);
//                        the new values are summed per workgroup into r[a] with one 64-bit agent-scope atomic add --
//                        integer adds, their order does not matter.
// Every kernel runs to its end on its own: no cooperative launch, no wait between workgroups, a launch boundary publishes
// each kernel.  Entries of dead rows and columns go stale and are never read unmasked.
//
// Memory: n x ld u32, ld = n rounded up to a multiple of 4 (every row starts on 16 bytes): 400 MB at 10 000 sketches, 17 GB
// at HG_NJ_MAX_N; allocated per call, released before the call returns.  Per node (w_nj, ld entries each): r[] and the row
// results Q (i64), live[] and the row results j (u32); live of a padding column is 0.  hg_nj_dev fills the upper triangle
// from row blocks of hg_dist_full_dev (rows [r0, r1) x columns [r0, n) in the search's scratch block, at most
// HG_SEARCH_BLOCK_BYTES; "nj_block_rows" forces the row count) and mirrors it: the rounds read rows a and b whole.
// The matrix, its fill and mirror and the row blocks are hg_dense_matrix.h's, shared with average and complete linkage.
#include "hg_cluster_common.h"
#include "hg_dense_matrix.h"
#include "hg_nj_math.h"

static_assert(HG_NJ_MATH_FRAC_BITS == HG_NJ_FRAC_BITS, "hg_nj_math.h and hypergen.h agree on the fixed point");
static_assert(sizeof(hg_nj_join) == 24, "hg_nj_join is 24 bytes");

namespace {
constexpr uint32_t SCAN_STEP = 1024;  // columns one step of the row scan covers: 256 lanes x 4
constexpr uint32_t PICK_LANES = 1024;

struct Nj {
  uint32_t *M;     // n rows of ld distances
  size_t ld;       // n rounded up to a multiple of 4
  int64_t *r;      // ld: r(i) of a live name
  int64_t *row_q;  // ld: Q of the row's best pair
  uint32_t *live;  // ld: 1 of a live name, 0 of a dead one and of the padding
  uint32_t *row_j; // ld: the higher name of the row's best pair, DENSE_NONE = none (dead rows, the last live row)
};

struct NjDist {
  __device__ __forceinline__ uint32_t operator()(float ani) const { return hg_nj_dist(ani); }
};

__global__ __launch_bounds__(256) void nj_init_kernel(uint32_t *__restrict__ live, uint32_t *__restrict__ row_j, uint32_t n, uint32_t ld) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ld; i += stride) live[i] = i < n ? 1u : 0u, row_j[i] = DENSE_NONE;
}

__global__ __launch_bounds__(256) void nj_fill_kernel(const float *__restrict__ blk, size_t pitch, uint32_t c0, uint32_t r0, uint32_t rows,
                                                      uint32_t n, size_t ld, uint32_t *__restrict__ M) {
  matrix_fill_body<uint32_t, NjDist>(blk, pitch, c0, r0, rows, n, ld, M, HG_LANE0, HG_LANES);
}
__global__ __launch_bounds__(256) void nj_mirror_kernel(uint32_t *M, uint32_t n, size_t ld) { matrix_mirror_body(M, n, ld); }

__device__ __forceinline__ int64_t block_sum_i64(int64_t v, int64_t *s_wave) {
  for (int d = 32; d >= 1; d >>= 1) v += (int64_t)__shfl_xor((long long)v, d);
  if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  return s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];  // (workgroups of 256 lanes)
}

// The initial r(i): one workgroup per row, the whole row in 16-byte pieces (the diagonal and the padding are 0).
__global__ __launch_bounds__(256) void nj_rsum_kernel(const uint32_t *__restrict__ M, size_t ld, int64_t *__restrict__ r) {
  __shared__ int64_t s_wave[4];
  const uint4 *row = reinterpret_cast<const uint4 *>(M + (size_t)blockIdx.x * ld);
  int64_t sum = 0;
  for (size_t j = threadIdx.x; j < ld / 4; j += 256) {
    const uint4 v = row[j];
    sum += (int64_t)v.x + (int64_t)v.y + (int64_t)v.z + (int64_t)v.w;
  }
  sum = block_sum_i64(sum, s_wave);
  if (threadIdx.x == 0) r[blockIdx.x] = sum;
}

// a candidate (key, j) against the best so far: the smaller key, ties to the smaller column
__device__ __forceinline__ void take_min(int64_t &bk, uint32_t &bj, int64_t k, uint32_t j) {
  const bool better = (k < bk) | ((k == bk) & (j < bj));  // (| and &: selects, no branch per element)
  bk = better ? k : bk, bj = better ? j : bj;
}
__device__ __forceinline__ void take4(int64_t &bk, uint32_t &bj, const uint4 v, const uint4 l, const int64_t *__restrict__ r, uint32_t j,
                                      uint32_t i, uint32_t c) {
  const uint32_t d[4] = {v.x, v.y, v.z, v.w}, live[4] = {l.x, l.y, l.z, l.w};
  const longlong2 r01 = *reinterpret_cast<const longlong2 *>(r + j), r23 = *reinterpret_cast<const longlong2 *>(r + j + 2);
  const int64_t rj[4] = {r01.x, r01.y, r23.x, r23.y};
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const int64_t counts = (int64_t)((live[k] != 0u) & (j + k > i));
    const int64_t mask = 0 - counts;  // (a mask, not a branch: the loads above stay whole; no key reaches 2^50)
    const int64_t key = (hg_nj_key(c, d[k], rj[k]) & mask) | (INT64_MAX & ~mask);
    take_min(bk, bj, key, (j + k) | ~(uint32_t)mask);
  }
}

// One workgroup per row.  live[] and r[] are the previous round's, final; row_q[i] and row_j[i] are written by the workgroup
// of i alone.  Every piece read lies inside the row: j is a multiple of 4 below n, so j + 3 < ld.
__global__ __launch_bounds__(256) void nj_best_kernel(const uint32_t *__restrict__ M, size_t ld, uint32_t n, const uint32_t *__restrict__ live,
                                                      const int64_t *__restrict__ r, uint32_t c, int64_t *__restrict__ row_q,
                                                      uint32_t *__restrict__ row_j) {
  __shared__ int64_t s_k[4];
  __shared__ uint32_t s_j[4];
  const uint32_t i = blockIdx.x, t = threadIdx.x;
  if (live[i] == 0u) return;  // (uniform over the workgroup; nj_pick_kernel skips dead rows by live[] itself)
  const uint4 *row = reinterpret_cast<const uint4 *>(M + (size_t)i * ld);
  const uint4 *lv = reinterpret_cast<const uint4 *>(live);
  int64_t bk = INT64_MAX;
  uint32_t bj = DENSE_NONE;
  // from the piece that holds column i + 1; two steps per trip while both are inside the row, their loads independent of
  // each other, then at most one step more
  uint32_t j = ((i + 1u) & ~3u) + 4u * t;
  for (; j + SCAN_STEP < n; j += 2u * SCAN_STEP) {
    const uint32_t j1 = j + SCAN_STEP;
    const uint4 v0 = row[j >> 2], l0 = lv[j >> 2], v1 = row[j1 >> 2], l1 = lv[j1 >> 2];
    take4(bk, bj, v0, l0, r, j, i, c);
    take4(bk, bj, v1, l1, r, j1, i, c);
  }
  if (j < n) take4(bk, bj, row[j >> 2], lv[j >> 2], r, j, i, c);
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t yk = (int64_t)__shfl_xor((long long)bk, d);
    const uint32_t yj = (uint32_t)__shfl_xor((int)bj, d);
    take_min(bk, bj, yk, yj);
  }
  if ((t & 63u) == 0) s_k[t >> 6] = bk, s_j[t >> 6] = bj;
  __syncthreads();
  if (t == 0) {
    for (uint32_t w = 1; w < 4; ++w) take_min(bk, bj, s_k[w], s_j[w]);
    row_j[i] = bj;
    row_q[i] = bj != DENSE_NONE ? bk - r[i] : 0;
  }
}

// One workgroup of PICK_LANES lanes: the minimum of (Q, i) over the live rows that have a pair (a row's j is its own
// tie-break already), join t, and the two words the update kernel and the next round rely on: live[b] = 0, r[a] = 0.
// c == 2 is the last join: the only pair there is, len_a = d(a, b), len_b = 0.
__global__ __launch_bounds__(PICK_LANES) void nj_pick_kernel(const uint32_t *__restrict__ M, size_t ld, uint32_t n, uint32_t *live, int64_t *r,
                                                             const int64_t *__restrict__ row_q, const uint32_t *__restrict__ row_j, uint32_t c,
                                                             hg_nj_join *__restrict__ joins, uint32_t t_join) {
  __shared__ int64_t s_k[PICK_LANES / 64];
  __shared__ uint32_t s_i[PICK_LANES / 64];
  const uint32_t t = threadIdx.x;
  int64_t bk = INT64_MAX;
  uint32_t bi = DENSE_NONE;
  for (uint32_t i = t; i < n; i += PICK_LANES) {
    const bool counts = live[i] != 0u && row_j[i] != DENSE_NONE;
    take_min(bk, bi, counts ? row_q[i] : INT64_MAX, counts ? i : DENSE_NONE);
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t yk = (int64_t)__shfl_xor((long long)bk, d);
    const uint32_t yi = (uint32_t)__shfl_xor((int)bi, d);
    take_min(bk, bi, yk, yi);
  }
  if ((t & 63u) == 0) s_k[t >> 6] = bk, s_i[t >> 6] = bi;
  __syncthreads();
  if (t == 0) {
    for (uint32_t w = 1; w < PICK_LANES / 64; ++w) take_min(bk, bi, s_k[w], s_i[w]);
    hg_nj_join out{DENSE_NONE, DENSE_NONE, 0, 0};  // (never written with c >= 2 live names: a pair exists)
    if (bi != DENSE_NONE) {
      const uint32_t a = bi, b = row_j[a];
      const uint32_t D = M[(size_t)a * ld + b];
      const int64_t len_a = c == 2u ? (int64_t)D : hg_nj_len_a(c, D, r[a], r[b]);
      out = hg_nj_join{a, b, len_a, (int64_t)D - len_a};
      live[b] = 0u, r[a] = 0;
    }
    joins[t_join] = out;
  }
}

// One lane per k, grid-stride.  a, b and D = len_a + len_b come from join t.  Lane k alone touches M[a][k], M[k][a] and
// r[k]; rows a and b are read at column k only, by lane k; r[a] takes atomic adds alone.
__global__ __launch_bounds__(256) void nj_update_kernel(uint32_t *M, size_t ld, uint32_t n, const uint32_t *__restrict__ live, int64_t *r,
                                                        const hg_nj_join *__restrict__ joins, uint32_t t_join) {
  __shared__ int64_t s_wave[4];
  const hg_nj_join jn = joins[t_join];
  const uint32_t a = jn.a, b = jn.b;
  if (a >= n || b >= n) return;  // (uniform over the grid)
  const uint32_t D = (uint32_t)(jn.len_a + jn.len_b);
  uint32_t *row_a = M + (size_t)a * ld;
  const uint32_t *row_b = M + (size_t)b * ld;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  int64_t sum = 0;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
    if (live[k] == 0u || k == a) continue;  // (b is dead already)
    const uint32_t da = row_a[k], db = row_b[k];
    const uint32_t nv = hg_nj_update(da, db, D);
    row_a[k] = nv, M[k * ld + a] = nv;
    r[k] += (int64_t)nv - (int64_t)da - (int64_t)db;
    sum += (int64_t)nv;
  }
  sum = block_sum_i64(sum, s_wave);
  if (threadIdx.x == 0 && sum != 0)
    __hip_atomic_fetch_add(reinterpret_cast<long long *>(r + a), (long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hg_status nj_too_large(hg_ctx *c) {
  return hg_fail(c, HG_ERR_UNSUPPORTED, "neighbour joining holds the dense matrix: n must be <= HG_NJ_MAX_N (65536)");
}

// the checks every entry point starts with: n_joins (zeroed), the limit, and for the forms that run the comparison a
// symmetric metric; *done = nothing to do (n <= 1)
hg_status nj_check(hg_ctx *c, size_t n, size_t *n_joins, bool dist_form, bool *done) {
  *done = false;
  if (!n_joins) return hg_fail(c, HG_ERR_INVALID, "n_joins == NULL");
  hg_status s = hg_cluster_check(c, 0, n_joins, dist_form);  // (the metric, with clustering's own error; the size is checked below)
  if (s != HG_OK) return s;
  if (n > HG_NJ_MAX_N) return nj_too_large(c);
  *done = n <= 1;
  return HG_OK;
}

// per-node state in w_nj, the matrix in `hold`, live[] initialised (stream-ordered)
hg_status nj_begin(hg_ctx *c, size_t n, Nj &g, MatrixHold &hold) {
  hg_status s;
  g.ld = (n + 3) & ~(size_t)3;
  if ((s = hg_ensure(c, c->w_nj, g.ld * 24 + 64)) != HG_OK) return s;
  g.r = static_cast<int64_t *>(c->w_nj.p);
  g.row_q = g.r + g.ld;
  g.live = reinterpret_cast<uint32_t *>(g.row_q + g.ld), g.row_j = g.live + g.ld;
  if ((s = hg_matrix_alloc(c, hold, n * g.ld * sizeof(uint32_t), "neighbour joining")) != HG_OK) return s;
  g.M = static_cast<uint32_t *>(hold.p);
  hg_timed tm(c, HG_T_DIST);
  hipLaunchKernelGGL(nj_init_kernel, dim3(grid_for(c, g.ld)), dim3(256), 0, c->stream, g.live, g.row_j, (uint32_t)n, (uint32_t)g.ld);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

// rows [r0, r0 + rows) from a block of ANI values (nj_fill_kernel)
hg_status nj_fill(hg_ctx *c, const Nj &g, const float *blk, size_t pitch, size_t c0, size_t r0, size_t rows, size_t n) {
  return hg_matrix_fill<uint32_t>(c, nj_fill_kernel, g.M, g.ld, blk, pitch, c0, r0, rows, n);
}

// the filled upper triangle -> mirror, r(), n - 2 rounds and the last join, all queued; final on return
hg_status nj_resolve(hg_ctx *c, Nj &g, size_t n, hg_nj_join *d_joins, size_t *n_joins) {
  const uint32_t m = (uint32_t)n;
  const hg_status s = hg_matrix_mirror<uint32_t>(c, nj_mirror_kernel, g.M, n, g.ld);
  if (s != HG_OK) return s;
  {
    hg_timed tm(c, HG_T_DIST);
    hipLaunchKernelGGL(nj_rsum_kernel, dim3(m), dim3(256), 0, c->stream, g.M, g.ld, g.r);
    HG_HIP(c, hipGetLastError());
    const dim3 row_grid(m), node_grid(grid_for(c, n));
    for (uint32_t t = 0; t + 1 < m; ++t) {
      const uint32_t live = m - t;  // c of the rule: 2 at the last join, which has nothing to update
      hipLaunchKernelGGL(nj_best_kernel, row_grid, dim3(256), 0, c->stream, g.M, g.ld, m, g.live, g.r, live, g.row_q, g.row_j);
      HG_HIP(c, hipGetLastError());
      hipLaunchKernelGGL(nj_pick_kernel, dim3(1), dim3(PICK_LANES), 0, c->stream, g.M, g.ld, m, g.live, g.r, g.row_q, g.row_j, live, d_joins, t);
      HG_HIP(c, hipGetLastError());
      if (live == 2u) break;
      hipLaunchKernelGGL(nj_update_kernel, node_grid, dim3(256), 0, c->stream, g.M, g.ld, m, g.live, g.r, d_joins, t);
      HG_HIP(c, hipGetLastError());
    }
  }
  HG_HIP(c, hipStreamSynchronize(c->stream));
  *n_joins = n - 1;
  return HG_OK;
}
}  // namespace

extern "C" hg_status hg_nj_matrix_dev(hg_ctx *c, const float *d_ani, size_t n, hg_nj_join *d_joins, size_t *n_joins) {
  if (!c) return HG_ERR_INVALID;
  bool done;
  hg_status s = nj_check(c, n, n_joins, false, &done);
  if (s != HG_OK || done) return s;
  if (!d_ani || !d_joins) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  Nj g{};
  MatrixHold hold;
  if ((s = nj_begin(c, n, g, hold)) != HG_OK) return s;
  if ((s = nj_fill(c, g, d_ani, n, 0, 0, n, n)) != HG_OK) return s;
  return nj_resolve(c, g, n, d_joins, n_joins);
}

extern "C" hg_status hg_nj_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                               hg_nj_join *d_joins, size_t *n_joins) {
  if (!c) return HG_ERR_INVALID;
  bool done;
  hg_status s = nj_check(c, n, n_joins, true, &done);
  if (s != HG_OK || done) return s;
  if (!d_hv || !d_norm2 || !d_joins) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if ((s = hg_sketch_dims_check(c, hv_d, ksize)) != HG_OK) return s;
  HG_ENTER(c);
  Nj g{};
  MatrixHold hold;
  s = hg_matrix_row_blocks(
      c, d_hv, d_norm2, n, hv_d, ksize, c->dbg_nj_block_rows, true, [&] { return nj_begin(c, n, g, hold); },
      [&](const float *blk, size_t pitch, size_t c0, size_t r0, size_t rows) { return nj_fill(c, g, blk, pitch, c0, r0, rows, n); });
  if (s != HG_OK) return s;
  return nj_resolve(c, g, n, d_joins, n_joins);
}

extern "C" hg_status hg_nj(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize, hg_nj_join *joins,
                           size_t *n_joins) {
  if (!c) return HG_ERR_INVALID;
  bool done;
  hg_status s = nj_check(c, n, n_joins, true, &done);
  if (s != HG_OK || done) return s;
  if (!hv || !norm2 || !joins) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  const int16_t *d_hv;
  const int32_t *d_norm2;
  uint32_t *d_out;
  if ((s = hg_cluster_stage(c, hv, norm2, n, hv_d, (n - 1) * sizeof(hg_nj_join), &d_hv, &d_norm2, &d_out)) != HG_OK) return s;
  auto *d_joins = reinterpret_cast<hg_nj_join *>(d_out);
  if ((s = hg_nj_dev(c, d_hv, d_norm2, n, hv_d, ksize, d_joins, n_joins)) != HG_OK) return s;
  HG_HIP(c, hipMemcpyAsync(joins, d_joins, (n - 1) * sizeof(hg_nj_join), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}
