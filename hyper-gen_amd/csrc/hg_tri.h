// hg_tri.h -- what hg_tri.hip (host entry points) and hg_tri_kernels.hip (the kernel) of libhypergen_tri.so share: the
// geometry of the kernel, the packer of one field, the size of a streamed block and the launcher.  Not installed.  The packer
// is usable from host code without HIP: tests/native/tri_format_driver.cpp sweeps it on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HG_TRI_HD __host__ __device__
#else
#define HG_TRI_HD
#endif

// ---- one field: seven characters and a separator in one 64-bit word -------------------------------------------------------------
// The field of m in 0..100 000, thousandths, as the little-endian word whose bytes are the text: m / 1000 right-aligned in
// three characters, '.', m % 1000 in three digits, the separator.  No division: every quotient is a multiply and a shift.
//   m / 1000   = (m * 4 294 968) >> 32: the constant is ceil(2^32 / 1000), its excess over 2^32 / 1000 times 1000 is 704, and
//                m * 704 < 2^32 up to m = 6 100 804.  (The high half of a 32 x 32 product: one v_mul_hi_u32.)
//   f / 100    = (f * 41) >> 12 for f < 1000: 41 * 100 - 4096 = 4, and f * 4 < 4096 up to f = 1023.
//   r / 10     = (r * 205) >> 11 for r <= 100: 205 * 10 - 2048 = 2, and r * 2 < 2048 up to r = 1023.
// The driver compares all 100 001 values with snprintf("%7.3f").
HG_TRI_HD inline uint64_t hg_tri_field(uint32_t m, uint32_t sep) {
  const uint32_t ip = (uint32_t)(((uint64_t)m * 4294968u) >> 32), f = m - ip * 1000u;  // 0..100, 0..999
  const uint32_t t = (ip * 205u) >> 11, u = ip - t * 10u;                               // ip / 10 (0..10), ip % 10
  const uint32_t d2 = (f * 41u) >> 12, r = f - d2 * 100u, d1 = (r * 205u) >> 11, d0 = r - d1 * 10u;
  const uint32_t c0 = ip >= 100u ? '1' : ' ';
  const uint32_t c1 = ip >= 100u ? '0' : ip >= 10u ? '0' + t : ' ';
  const uint32_t lo = c0 | c1 << 8 | ('0' + u) << 16 | (uint32_t)'.' << 24;
  const uint32_t hi = ('0' + d2) | ('0' + d1) << 8 | ('0' + d0) << 16 | sep << 24;
  return (uint64_t)hi << 32 | lo;
}

// ---- geometry ----------------------------------------------------------------------------------------------------------------
constexpr uint32_t HG_TRI_THREADS = 256;                              // tri_format_kernel: four waves per workgroup
constexpr uint32_t HG_TRI_WAVE = 64;
constexpr uint32_t HG_TRI_WAVES = HG_TRI_THREADS / HG_TRI_WAVE;
constexpr uint32_t HG_TRI_LANE_COLS = 4;                              // one 16-byte load and 32 bytes of text per lane and row
constexpr uint32_t HG_TRI_TILE_COLS = HG_TRI_WAVE * HG_TRI_LANE_COLS;  // columns per workgroup: 256, a wave reads 1 KiB and writes 2 KiB of a row
constexpr uint32_t HG_TRI_TILE_ROWS = 32;                             // rows per workgroup, wave v takes rows v, v + 4, ...: no state to amortise
constexpr uint32_t HG_TRI_MAX_GRID_Y = 32768;                         // row tiles per launch

// ---- the streamed block ------------------------------------------------------------------------------------------------------
// hg_tri_stream_dev cuts the set into blocks of at most this much text (one row where a row is longer) and keeps two device and
// two page-locked host buffers of it.  (hg_tri_dev keeps no text buffer: its blocks fill HG_SEARCH_BLOCK_BYTES of floats.)
constexpr size_t HG_TRI_TEXT_BLOCK_BYTES = (size_t)64 << 20;

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "../../include/hypergen_tri.h"

// ---- launcher (hg_tri_kernels.hip), on `st` ----------------------------------------------------------------------------------------
enum : uint32_t { HG_TRI_K_FORMAT, HG_TRI_N_KERNELS };
// how often the process has launched kernel k so far (hg_tri_launch_counts)
uint64_t hg_tri_launches(uint32_t kernel);
// blk[r * pitch + c] = ani(row0 + r, c), r < rows, c < cols: the fields of the block into text (8-byte aligned), row r's at
// the block-relative offset of hg_tri_field_offset.  rows and cols > 0, row0 + rows and cols <= 2^31; LOWER: cols >= row0 +
// rows - 1 >= 1.  One launch per HG_TRI_MAX_GRID_Y row tiles.
hipError_t hg_tri_launch_format(hipStream_t st, const float *blk, uint32_t rows, uint32_t cols, size_t pitch, uint32_t row0, uint32_t layout,
                                char *text);
#endif
