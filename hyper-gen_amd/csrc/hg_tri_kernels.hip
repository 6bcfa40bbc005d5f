// hg_tri_kernels.hip -- the kernel of libhypergen_tri.so and its launcher (hg_tri.h).
//
// The format reads a block of the ANI matrix once and writes eight bytes of text per pair: it is bound by the read of 4 and the
// write of 8 bytes per pair, like cluster_stats_rows_kernel and hist_count_kernel by their reads alone.
//   tri_format_kernel  one workgroup of four waves per tile of 32 rows x 256 columns.  A lane owns four consecutive columns and a
//                      wave walks down every fourth row of the tile with one 16-byte load per lane and row -- a wave reads 1 KiB
//                      and writes 2 KiB of a row contiguously.  A row of the matrix starts at blk + r * pitch, 16-byte aligned
//                      only by luck: the load is declared 4-byte aligned (hist_count_kernel reads this way).
//                      Per value: hg_avg_milli, then the seven characters and the separator of hg_tri_field packed into one
//                      64-bit word in registers -- multiplies and shifts, no division.
//                      A row of the text starts at a multiple of 8 bytes and is 16-byte aligned or not by the parity of the
//                      fields in front of it and of the text's own address; that is a property of the row, so of the wave.
//                      An aligned row stores a lane's 32 bytes as two 16-byte stores.  A row off by 8 stores the lane's first
//                      and last field as 8 bytes and the two between them as 16: every 16-byte store is 16-byte aligned.
//                      The fields a row has are j < lim: lim = i under HG_TRI_LOWER, cols under HG_TRI_FULL, and the field
//                      lim - 1 carries the '\n'.  A tile whose every row has lim behind the tile's last column tests nothing
//                      and writes tabs only.  Any other tile -- the diagonal's under LOWER, the last column's under FULL --
//                      works out per lane how many of its four columns exist: all four go the vector way with the separator
//                      chosen for the fourth, one to three are read as dwords and stored as single fields, none is skipped.
//                      A LOWER tile wholly at or above the diagonal returns at once.
//                      No LDS, no atomics, vector stores only.
#include <atomic>

#include "hg_average_cmp.h"
#include "hg_tri.h"

namespace {

typedef float tri_f4 __attribute__((ext_vector_type(4), aligned(4)));  // four floats at any dword address
typedef uint64_t tri_u2 __attribute__((ext_vector_type(2)));           // two fields, 16-byte aligned

__device__ __forceinline__ uint64_t field_of(float ani, uint32_t sep) { return hg_tri_field((uint32_t)hg_avg_milli(ani), sep); }

// a lane's four fields at w (8-byte aligned; 16-byte aligned iff `even`)
__device__ __forceinline__ void store4(uint64_t *w, bool even, uint64_t f0, uint64_t f1, uint64_t f2, uint64_t f3) {
  if (even) {
    *reinterpret_cast<tri_u2 *>(w) = tri_u2{f0, f1};
    *reinterpret_cast<tri_u2 *>(w + 2) = tri_u2{f2, f3};
  } else {
    w[0] = f0;
    *reinterpret_cast<tri_u2 *>(w + 1) = tri_u2{f1, f2};
    w[3] = f3;
  }
}

__global__ __launch_bounds__(HG_TRI_THREADS) void tri_format_kernel(const float *__restrict__ blk, uint32_t rows, uint32_t cols, size_t pitch,
                                                                    uint32_t row0, uint32_t lower, uint32_t tile_y0, uint64_t *__restrict__ text) {
  const uint32_t t = threadIdx.x, lane = t & (HG_TRI_WAVE - 1), wave = t / HG_TRI_WAVE;
  const uint32_t r_lo = (tile_y0 + blockIdx.y) * HG_TRI_TILE_ROWS, r_hi = min(rows, r_lo + HG_TRI_TILE_ROWS);
  const uint32_t c_lo = blockIdx.x * HG_TRI_TILE_COLS, c_hi = min(cols, c_lo + HG_TRI_TILE_COLS);
  const uint32_t gi_lo = row0 + r_lo, gi_hi = row0 + r_hi;  // the tile's global rows [gi_lo, gi_hi), <= 2^31
  if (lower && c_lo + 1 >= gi_hi) return;                   // no j < i in the tile: its first column against its last row
  // every row of the tile has fields behind the tile's last column: LOWER lim = i >= gi_lo, FULL lim = cols
  const bool inner = lower ? c_hi < gi_lo : c_hi < cols;
  const uint32_t c0 = c_lo + lane * HG_TRI_LANE_COLS;
  const uint64_t t0 = (uint64_t)row0 * (row0 - (row0 ? 1u : 0u)) / 2;  // fields of the triangle in front of the block
  const uint64_t odd0 = (uint64_t)(reinterpret_cast<uintptr_t>(text) >> 3);  // (its lowest bit: the text itself may start off by 8)
  const float *p = blk + (size_t)(r_lo + wave) * pitch + c0;
  const size_t step = (size_t)HG_TRI_WAVES * pitch;
  if (inner) {  // (the tile is whole in its columns: c_hi < cols leaves c_hi = c_lo + 256)
#pragma unroll 4
    for (uint32_t r = r_lo + wave; r < r_hi; r += HG_TRI_WAVES, p += step) {
      const uint64_t i = (uint64_t)row0 + r;
      const uint64_t first = lower ? i * (i - 1) / 2 - t0 : (uint64_t)r * cols;  // the row's first field, in fields
      const tri_f4 a = *reinterpret_cast<const tri_f4 *>(p);
      store4(text + first + c0, !((first + odd0) & 1), field_of(a.x, '\t'), field_of(a.y, '\t'), field_of(a.z, '\t'), field_of(a.w, '\t'));
    }
    return;
  }
  for (uint32_t r = r_lo + wave; r < r_hi; r += HG_TRI_WAVES, p += step) {
    const uint64_t i = (uint64_t)row0 + r;
    const uint32_t lim = lower ? (uint32_t)i : cols;  // (LOWER: i <= row0 + rows - 1 <= cols)
    if (c0 >= lim) continue;
    const uint64_t first = lower ? i * (i - 1) / 2 - t0 : (uint64_t)r * cols;
    const uint32_t n_own = min(HG_TRI_LANE_COLS, lim - c0);
    uint64_t *w = text + first + c0;
    if (n_own == HG_TRI_LANE_COLS) {
      const tri_f4 a = *reinterpret_cast<const tri_f4 *>(p);
      store4(w, !((first + odd0) & 1), field_of(a.x, '\t'), field_of(a.y, '\t'), field_of(a.z, '\t'), field_of(a.w, c0 + 4 == lim ? '\n' : '\t'));
    } else {  // the row's last one to three fields: dwords in, single fields out
      w[0] = field_of(p[0], n_own == 1 ? '\n' : '\t');
      if (n_own > 1) w[1] = field_of(p[1], n_own == 2 ? '\n' : '\t');
      if (n_own > 2) w[2] = field_of(p[2], '\n');
    }
  }
}

std::atomic<uint64_t> g_launches[HG_TRI_N_KERNELS];

}  // namespace

uint64_t hg_tri_launches(uint32_t kernel) { return kernel < HG_TRI_N_KERNELS ? g_launches[kernel].load() : 0; }

hipError_t hg_tri_launch_format(hipStream_t st, const float *blk, uint32_t rows, uint32_t cols, size_t pitch, uint32_t row0, uint32_t layout,
                                char *text) {
  const bool lower = layout == HG_TRI_LOWER;
  // LOWER: no row of the block has a field at or behind column row0 + rows - 1
  const uint32_t used = lower ? min(cols, row0 + rows - 1) : cols;
  const uint32_t tiles_x = (used + HG_TRI_TILE_COLS - 1) / HG_TRI_TILE_COLS, tiles_y = (rows + HG_TRI_TILE_ROWS - 1) / HG_TRI_TILE_ROWS;
  for (uint32_t y0 = 0; y0 < tiles_y; y0 += HG_TRI_MAX_GRID_Y) {
    ++g_launches[HG_TRI_K_FORMAT];
    const dim3 grid(tiles_x, min(HG_TRI_MAX_GRID_Y, tiles_y - y0));
    tri_format_kernel<<<grid, HG_TRI_THREADS, 0, st>>>(blk, rows, used, pitch, row0, lower ? 1u : 0u, y0, reinterpret_cast<uint64_t *>(text));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
