// hg_hist_kernels.hip -- the kernel of libhypergen_hist.so and its launcher (hg_hist.h).
//
// The count reads a block of the ANI matrix and keeps nothing but a table of counters: it is bound by the read of the block,
// like cluster_stats_rows_kernel and frag_best_kernel.  The input is badly skewed -- about half of all unrelated pairs have a
// non-positive dot product and read exactly 0, a collection of one species puts every pair into a few dozen bins -- so the
// counters a pair touches are kept as close to the lanes as they can be:
//   hist_count_kernel  one workgroup of four waves per tile of 256 rows x 256 columns and per slice of the bin range.  A lane
//                      owns four consecutive columns and a wave walks down every fourth row of the tile with one 16-byte load
//                      per lane and row -- a wave reads 1 KiB of a row contiguously.  A row starts at blk + r * pitch, 16-byte
//                      aligned only by luck: the load is declared 4-byte aligned and compiles to global_load_dwordx4, which
//                      gfx950 serves at any dword address, so no row needs a peeled head (frag_best_kernel reads this way).
//                      The tail is peeled: the lane whose four columns hang over the block's last column reads the ones that
//                      exist as dwords.
//                      Bin 0 -- every NaN, negative and zero value, and whatever else prints below w -- never reaches LDS: a
//                      lane counts it in a register, the workgroup sums the registers once and issues one global add.
//                      Every other bin is an LDS u32 atomic into a table of HG_HIST_LDS_BINS counters.  A histogram whose bins
//                      fit the table two or four times over keeps that many copies, one per wave or pair of waves: same-address
//                      LDS atomics serialise, and the copies spread the hottest bin.  A histogram of more bins than the table
//                      is counted in slices: the grid's z layer names the slice, a workgroup counts the bins of its slice and
//                      drops the rest, and the block is read once per slice.
//                      A tile that lies wholly below the diagonal of HG_HIST_UPPER returns at once; a tile the diagonal does
//                      not cross takes no per-element test of the selection.
//                      At the end the non-zero counters go to the 64-bit table in global memory with one atomic add each, at
//                      agent scope.  A u32 counter cannot overflow: a tile has 65 536 elements.  Integer adds commute: neither
//                      the grid nor the order of the atomics can show in the result.
#include <atomic>

#include "hg_average_cmp.h"
#include "hg_hist.h"

namespace {

typedef float hist_f4 __attribute__((ext_vector_type(4), aligned(4)));  // four floats at any dword address

__global__ __launch_bounds__(HG_HIST_THREADS) void hist_count_kernel(const float *__restrict__ blk, uint32_t rows, uint32_t cols, size_t pitch,
                                                                     uint32_t row0, uint32_t col0, uint32_t pairs, uint64_t magic,
                                                                     uint32_t n_bins, uint32_t copies, uint32_t tile_y0,
                                                                     unsigned long long *counts) {
  __shared__ uint32_t s_tab[HG_HIST_LDS_BINS];
  __shared__ uint32_t s_zero[HG_HIST_WAVES];
  const uint32_t t = threadIdx.x, lane = t & (HG_HIST_WAVE - 1), wave = t / HG_HIST_WAVE;
  const uint32_t r_lo = (tile_y0 + blockIdx.y) * HG_HIST_TILE_ROWS, r_hi = min(rows, r_lo + HG_HIST_TILE_ROWS);
  const uint32_t c_lo = blockIdx.x * HG_HIST_TILE_COLS, c_hi = min(cols, c_lo + HG_HIST_TILE_COLS);
  // the tile's global rows [gi_lo, gi_hi) and columns [gj_lo, gj_hi), all <= 2^31
  const uint32_t gi_lo = row0 + r_lo, gi_hi = row0 + r_hi, gj_lo = col0 + c_lo, gj_hi = col0 + c_hi;
  if (pairs == HG_HIST_UPPER && gj_hi - 1 <= gi_lo) return;  // no i < j in the tile (uniform: in front of every barrier)
  // does the diagonal cross the tile?  (UPPER: a tile not wholly below it is wholly above when its last row is below its first column)
  const bool masked = pairs != HG_HIST_ALL && gj_lo < gi_hi && (pairs == HG_HIST_UPPER || gi_lo < gj_hi);
  const bool upper = pairs == HG_HIST_UPPER;
  const uint32_t slice_lo = blockIdx.z * HG_HIST_LDS_BINS, slice_n = min(HG_HIST_LDS_BINS, n_bins - slice_lo);
  for (uint32_t k = t; k < copies * slice_n; k += HG_HIST_THREADS) s_tab[k] = 0;  // (copies * slice_n <= HG_HIST_LDS_BINS: hg_hist_copies)
  __syncthreads();
  uint32_t *tab = s_tab + (wave & (copies - 1)) * slice_n;
  uint32_t zeros = 0;
  auto put = [&](float ani, uint32_t i, uint32_t j) {
    const uint32_t b = hg_hist_div((uint32_t)hg_avg_milli(ani), magic);
    if (masked && !(upper ? i < j : i != j)) return;
    if (b == 0) {
      ++zeros;
    } else if (b - slice_lo < slice_n) {  // (a bin below the slice wraps far above it)
      __hip_atomic_fetch_add(tab + (b - slice_lo), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  };
  const uint32_t c0 = c_lo + lane * HG_HIST_LANE_COLS;
  const uint32_t n_own = c0 < c_hi ? min(HG_HIST_LANE_COLS, c_hi - c0) : 0;  // columns of this lane that exist
  const uint32_t j0 = col0 + c0;
  const float *p = blk + (size_t)(r_lo + wave) * pitch + c0;
  const size_t step = (size_t)HG_HIST_WAVES * pitch;
  if (n_own == HG_HIST_LANE_COLS) {
#pragma unroll 4
    for (uint32_t r = r_lo + wave; r < r_hi; r += HG_HIST_WAVES, p += step) {
      const hist_f4 a = *reinterpret_cast<const hist_f4 *>(p);
      const uint32_t i = row0 + r;
      put(a.x, i, j0), put(a.y, i, j0 + 1), put(a.z, i, j0 + 2), put(a.w, i, j0 + 3);
    }
  } else if (n_own) {  // the block's last columns: one to three, as dwords
    for (uint32_t r = r_lo + wave; r < r_hi; r += HG_HIST_WAVES, p += step) {
      const uint32_t i = row0 + r;
      put(p[0], i, j0);
      if (n_own > 1) put(p[1], i, j0 + 1);
      if (n_own > 2) put(p[2], i, j0 + 2);
    }
  }
  // bin 0: the registers of a wave by shuffles, the four waves through LDS, one add (the first slice's workgroups only)
  for (int d = HG_HIST_WAVE / 2; d >= 1; d >>= 1) zeros += __shfl_xor(zeros, d);
  if (lane == 0) s_zero[wave] = zeros;
  __syncthreads();  // (and every LDS atomic of the tile is done)
  if (t == 0 && blockIdx.z == 0) {
    unsigned long long z = 0;
    for (uint32_t v = 0; v < HG_HIST_WAVES; ++v) z += s_zero[v];
    if (z) __hip_atomic_fetch_add(counts, z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  for (uint32_t k = t; k < slice_n; k += HG_HIST_THREADS) {
    unsigned long long v = 0;
    for (uint32_t cp = 0; cp < copies; ++cp) v += s_tab[cp * slice_n + k];
    if (v) __hip_atomic_fetch_add(counts + slice_lo + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

std::atomic<uint64_t> g_launches[HG_HIST_N_KERNELS];

}  // namespace

uint64_t hg_hist_launches(uint32_t kernel) { return kernel < HG_HIST_N_KERNELS ? g_launches[kernel].load() : 0; }

uint32_t hg_hist_copies(uint32_t n_bins) { return 4 * n_bins <= HG_HIST_LDS_BINS ? 4 : 2 * n_bins <= HG_HIST_LDS_BINS ? 2 : 1; }

hipError_t hg_hist_launch_count(hipStream_t st, const float *blk, uint32_t rows, uint32_t cols, size_t pitch, uint32_t row0, uint32_t col0,
                                uint32_t pairs, uint32_t bin_milli, unsigned long long *d_counts) {
  const uint32_t n_bins = HG_HIST_MILLI_MAX / bin_milli + 1;
  const uint32_t slices = (n_bins + HG_HIST_LDS_BINS - 1) / HG_HIST_LDS_BINS, copies = hg_hist_copies(n_bins);
  const uint32_t tiles_x = (cols + HG_HIST_TILE_COLS - 1) / HG_HIST_TILE_COLS, tiles_y = (rows + HG_HIST_TILE_ROWS - 1) / HG_HIST_TILE_ROWS;
  for (uint32_t y0 = 0; y0 < tiles_y; y0 += HG_HIST_MAX_GRID_Y) {
    ++g_launches[HG_HIST_K_COUNT];
    const dim3 grid(tiles_x, min(HG_HIST_MAX_GRID_Y, tiles_y - y0), slices);
    hist_count_kernel<<<grid, HG_HIST_THREADS, 0, st>>>(blk, rows, cols, pitch, row0, col0, pairs, hg_hist_magic(bin_milli), n_bins, copies, y0,
                                                        d_counts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
