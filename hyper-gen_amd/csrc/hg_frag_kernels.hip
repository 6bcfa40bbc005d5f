// hg_frag_kernels.hip -- the two kernels of libhypergen_frag.so and their launchers (hg_frag.h).
//
// The reduction reads a block of the ANI matrix once and keeps 8 bytes per (reference genome, query fragment): it is bound
// by the read of the block, like cluster_stats_rows_kernel.
//   frag_best_kernel   one wave per (chunk of <= 32 rows of ONE reference genome) x (256 columns): a lane owns four
//                      consecutive columns and walks down the chunk's rows with one 16-byte load per row -- a wave reads
//                      1 KiB of a row contiguously.  A row of the block starts at blk + r * Q, which is 16-byte aligned
//                      only when Q % 4 == 0; the load is declared 4-byte aligned and compiles to global_load_dwordx4, which
//                      gfx950 serves at any dword address, so no row needs a peeled head.  The tail is peeled: the lane
//                      whose four columns hang over Q reads the ones that exist as dwords (reading on would leave the block
//                      behind its last row).  Per column the running best is a 64-bit key m << 32 | ~row in registers; at the
//                      end one 64-bit atomic max per column into the table of bests.  Rows ascend, max is associative and
//                      commutative: the order of the atomics cannot show.
//   frag_fold_kernel   one workgroup per (reference genome g, query genome h): the keys of h's fragments in g's row of the
//                      table, decoded, compared with m_th, summed by wave shuffles and across the four waves in LDS.  No
//                      atomics: a record has one writer.  With to_best every key is rewritten as its hg_frag_best record by
//                      the one lane that read it (every column lies in exactly one query genome).
#include <atomic>

#include "hg_average_cmp.h"
#include "hg_frag.h"

static_assert(sizeof(hg_frag_pair) == 16 && sizeof(hg_frag_best) == 8 && sizeof(hg_frag_chunk) == 16, "the records of include/hypergen_frag.h");

namespace {

typedef float frag_f4 __attribute__((ext_vector_type(4), aligned(4)));  // four floats at any dword address

__device__ __forceinline__ void take(unsigned long long &key, float ani, uint32_t not_row) {
  const unsigned long long k = (unsigned long long)hg_avg_milli(ani) << 32 | not_row;
  key = k > key ? k : key;
}

__global__ __launch_bounds__(HG_FRAG_WAVE) void frag_best_kernel(const float *__restrict__ blk, uint32_t r0, uint32_t rows, uint32_t Q,
                                                                 const hg_frag_chunk *__restrict__ chunks, uint32_t c_lo, uint32_t g0,
                                                                 unsigned long long *keys) {
  const hg_frag_chunk ch = chunks[c_lo + blockIdx.y];
  const uint32_t lo = max(ch.row0, r0), hi = min(ch.row0 + ch.n_rows, r0 + rows);  // (the launcher passes chunks that meet the block)
  const uint32_t c0 = blockIdx.x * HG_FRAG_COL_TILE + threadIdx.x * HG_FRAG_LANE_COLS;
  if (c0 >= Q || lo >= hi) return;
  const uint32_t n_own = min(HG_FRAG_LANE_COLS, Q - c0);  // columns of this lane that exist
  unsigned long long k0 = 0, k1 = 0, k2 = 0, k3 = 0;
  const float *p = blk + (size_t)(lo - r0) * Q + c0;
  if (n_own == HG_FRAG_LANE_COLS) {
#pragma unroll 4
    for (uint32_t r = lo; r < hi; ++r, p += Q) {
      const frag_f4 a = *reinterpret_cast<const frag_f4 *>(p);
      const uint32_t nr = ~r;
      take(k0, a.x, nr), take(k1, a.y, nr), take(k2, a.z, nr), take(k3, a.w, nr);
    }
  } else {  // the row's tail: one to three columns, as dwords
    for (uint32_t r = lo; r < hi; ++r, p += Q) {
      const uint32_t nr = ~r;
      take(k0, p[0], nr);
      if (n_own > 1) take(k1, p[1], nr);
      if (n_own > 2) take(k2, p[2], nr);
    }
  }
  unsigned long long *out = keys + (size_t)(ch.genome - g0) * Q + c0;
  __hip_atomic_fetch_max(out, k0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (n_own > 1) __hip_atomic_fetch_max(out + 1, k1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (n_own > 2) __hip_atomic_fetch_max(out + 2, k2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (n_own > 3) __hip_atomic_fetch_max(out + 3, k3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(HG_FRAG_FOLD_THREADS) void frag_fold_kernel(unsigned long long *keys, uint32_t g0, uint32_t Q,
                                                                         const uint32_t *__restrict__ qry_first, uint32_t n_qry, uint32_t m_th,
                                                                         hg_frag_pair *__restrict__ pair, int to_best) {
  __shared__ unsigned long long s_sum[HG_FRAG_FOLD_THREADS / HG_FRAG_WAVE];
  __shared__ uint32_t s_cnt[HG_FRAG_FOLD_THREADS / HG_FRAG_WAVE];
  const uint32_t t = threadIdx.x, h = blockIdx.x, gi = blockIdx.y;
  const uint32_t q_lo = qry_first[h], q_hi = qry_first[h + 1];
  unsigned long long *row = keys + (size_t)gi * Q;
  unsigned long long sum = 0;
  uint32_t cnt = 0;
  for (uint32_t q = q_lo + t; q < q_hi; q += HG_FRAG_FOLD_THREADS) {
    const unsigned long long key = row[q];
    const uint32_t m = (uint32_t)(key >> 32), r = ~(uint32_t)key;  // (key 0: m 0, row HG_FRAG_NONE)
    if (m >= m_th) sum += m, ++cnt;
    if (to_best) row[q] = (unsigned long long)r << 32 | m;  // hg_frag_best{m, row}, little endian
  }
  for (int d = HG_FRAG_WAVE / 2; d >= 1; d >>= 1) sum += __shfl_xor(sum, d), cnt += __shfl_xor(cnt, d);
  if ((t & (HG_FRAG_WAVE - 1)) == 0) s_sum[t / HG_FRAG_WAVE] = sum, s_cnt[t / HG_FRAG_WAVE] = cnt;
  __syncthreads();
  if (t == 0) {
    for (uint32_t w = 1; w < HG_FRAG_FOLD_THREADS / HG_FRAG_WAVE; ++w) sum += s_sum[w], cnt += s_cnt[w];
    pair[(size_t)(g0 + gi) * n_qry + h] = hg_frag_pair{sum, cnt, q_hi - q_lo};
  }
}

std::atomic<uint64_t> g_launches[HG_FRAG_N_KERNELS];

}  // namespace

uint64_t hg_frag_launches(uint32_t kernel) { return kernel < HG_FRAG_N_KERNELS ? g_launches[kernel].load() : 0; }

hipError_t hg_frag_launch_best(hipStream_t st, const float *blk, uint32_t r0, uint32_t rows, uint32_t Q, const hg_frag_chunk *d_chunks,
                               uint32_t c_lo, uint32_t n_chunks, uint32_t g0, unsigned long long *d_keys) {
  ++g_launches[HG_FRAG_K_BEST];
  const dim3 grid((Q + HG_FRAG_COL_TILE - 1) / HG_FRAG_COL_TILE, n_chunks);
  frag_best_kernel<<<grid, HG_FRAG_WAVE, 0, st>>>(blk, r0, rows, Q, d_chunks, c_lo, g0, d_keys);
  return hipGetLastError();
}

hipError_t hg_frag_launch_fold(hipStream_t st, unsigned long long *d_keys, uint32_t g0, uint32_t n_g, uint32_t Q, const uint32_t *d_qry_first,
                               uint32_t n_qry, uint32_t m_th, hg_frag_pair *d_pair, bool to_best) {
  ++g_launches[HG_FRAG_K_FOLD];
  frag_fold_kernel<<<dim3(n_qry, n_g), HG_FRAG_FOLD_THREADS, 0, st>>>(d_keys, g0, Q, d_qry_first, n_qry, m_th, d_pair, to_best ? 1 : 0);
  return hipGetLastError();
}
