// hg_hist.h -- what hg_hist.hip (host entry points) and hg_hist_kernels.hip (the kernel) of libhypergen_hist.so share: the
// geometry of the kernel, the exact division by the run-time bin width and the launcher.  Not installed.  The division is
// usable from host code without HIP: tests/native/hist_div_driver.cpp sweeps it on the CPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HG_HIST_HD __host__ __device__
#else
#define HG_HIST_HD
#endif

// ---- m / w without a division ------------------------------------------------------------------------------------------------
// m / w for m in 0..100 000 and w in 1..100 000 as a multiply and a shift: magic = floor(2^40 / w) + 1, q = (m magic) >> 40.
// With e = magic w - 2^40 (0 < e <= w) the product is m / w + m e / (w 2^40), and the floor is that of m / w as long as the
// second term stays below 1 / w: m e < 2^40, which 100 000 x 100 000 = 10^10 < 2^40 = 1.0995 10^12 grants.  The product
// m magic is below 2^17 (2^40 + 1) < 2^58: 64 bits hold it.
constexpr uint32_t HG_HIST_DIV_SHIFT = 40;
HG_HIST_HD inline uint64_t hg_hist_magic(uint32_t w) { return ((uint64_t)1 << HG_HIST_DIV_SHIFT) / w + 1; }
HG_HIST_HD inline uint32_t hg_hist_div(uint32_t m, uint64_t magic) { return (uint32_t)(((uint64_t)m * magic) >> HG_HIST_DIV_SHIFT); }

// ---- geometry ----------------------------------------------------------------------------------------------------------------
constexpr uint32_t HG_HIST_THREADS = 256;                               // hist_count_kernel: four waves per workgroup
constexpr uint32_t HG_HIST_WAVE = 64;
constexpr uint32_t HG_HIST_WAVES = HG_HIST_THREADS / HG_HIST_WAVE;
constexpr uint32_t HG_HIST_LANE_COLS = 4;                               // one 16-byte load per lane and row
constexpr uint32_t HG_HIST_TILE_COLS = HG_HIST_WAVE * HG_HIST_LANE_COLS;  // columns per workgroup: 256, a wave reads 1 KiB of a row
constexpr uint32_t HG_HIST_TILE_ROWS = 256;                             // rows per workgroup, wave v takes rows v, v + 4, ...
constexpr uint32_t HG_HIST_LDS_BINS = 8192;                             // u32 counters of one workgroup: 32 KiB, five workgroups per CU
constexpr uint32_t HG_HIST_MAX_GRID_Y = 32768;                          // row tiles per launch
static_assert((uint64_t)HG_HIST_TILE_ROWS * HG_HIST_TILE_COLS < ((uint64_t)1 << 32), "a tile's elements fit an LDS counter");

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "../../include/hypergen_hist.h"

// ---- launcher (hg_hist_kernels.hip), on `st` --------------------------------------------------------------------------------------
enum : uint32_t { HG_HIST_K_COUNT, HG_HIST_N_KERNELS };
// how often the process has launched kernel k so far (hg_hist_launch_counts)
uint64_t hg_hist_launches(uint32_t kernel);
// the copies of its table a workgroup keeps for a histogram of n_bins bins: 4, 2 or 1 (1 too when the histogram is sliced)
uint32_t hg_hist_copies(uint32_t n_bins);
// blk[r * pitch + c] = ani(row0 + r, col0 + c), r < rows, c < cols: the selected pairs into d_counts[m / w] (64-bit adds).
// rows and cols > 0, row0 + rows and col0 + cols <= 2^31, the block meets the selection.  One launch per HG_HIST_MAX_GRID_Y row
// tiles; its grid has one z layer per slice of HG_HIST_LDS_BINS bins.
hipError_t hg_hist_launch_count(hipStream_t st, const float *blk, uint32_t rows, uint32_t cols, size_t pitch, uint32_t row0, uint32_t col0,
                                uint32_t pairs, uint32_t bin_milli, unsigned long long *d_counts);
#endif
