// hg_frag.h -- what hg_frag.hip (host entry points) and hg_frag_kernels.hip (kernels) of libhypergen_frag.so share: the
// geometry of the two kernels, the row chunk table and the launchers.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hypergen_frag.h"

// ---- geometry ------------------------------------------------------------------------------------------------------------
constexpr uint32_t HG_FRAG_WAVE = 64;                              // frag_best_kernel: one wave per workgroup
constexpr uint32_t HG_FRAG_LANE_COLS = 4;                          // one 16-byte load per lane and row
constexpr uint32_t HG_FRAG_COL_TILE = HG_FRAG_WAVE * HG_FRAG_LANE_COLS;  // columns per workgroup: 256
constexpr uint32_t HG_FRAG_ROW_CHUNK = 32;                         // rows of one genome per workgroup
constexpr uint32_t HG_FRAG_FOLD_THREADS = 256;                     // frag_fold_kernel
constexpr uint32_t HG_FRAG_MAX_GRID_Y = 32768;                     // chunks per best launch, genomes per fold launch

// Rows [row0, row0 + n_rows) of the matrix belong to reference genome `genome`, n_rows <= HG_FRAG_ROW_CHUNK: the rows of a
// genome in chunks counted from its first row, all genomes in order (a genome without rows has no chunk).  A launch over the
// rows [r0, r0 + rows) of a block runs the chunks that meet them and clips each to the block: a maximum does not mind where
// a chunk is cut.
struct hg_frag_chunk {
  uint32_t row0, n_rows, genome, pad;
};

// A running best as one 64-bit key under max: m << 32 | ~row, so that equal m goes to the smaller row.  0 = no row seen
// (a key of a row has ~row != 0: rows are below 2^31), and it decodes to {0, HG_FRAG_NONE} by the same arithmetic.
__host__ __device__ inline uint64_t hg_frag_key(uint32_t m, uint32_t row) { return (uint64_t)m << 32 | (uint32_t)~row; }

// ---- launchers (hg_frag_kernels.hip), all on `st` ----------------------------------------------------------------------------
enum : uint32_t { HG_FRAG_K_BEST, HG_FRAG_K_FOLD, HG_FRAG_N_KERNELS };
// how often the process has launched kernel k so far (hg_frag_launch_counts)
uint64_t hg_frag_launches(uint32_t kernel);
// blk[(r - r0) * Q + q] = ani(r, q) for the rows [r0, r0 + rows): the chunks [c_lo, c_lo + n_chunks) of d_chunks, clipped to
// those rows, into d_keys[(genome - g0) * Q + q] (64-bit max).  n_chunks <= HG_FRAG_MAX_GRID_Y.
hipError_t hg_frag_launch_best(hipStream_t st, const float *blk, uint32_t r0, uint32_t rows, uint32_t Q, const hg_frag_chunk *d_chunks,
                               uint32_t c_lo, uint32_t n_chunks, uint32_t g0, unsigned long long *d_keys);
// the keys of the genomes [g0, g0 + n_g) -> d_pair[(g0 + i) * n_qry + h]; to_best: every key is rewritten in place as its
// hg_frag_best record.  m_th above 100 000 matches nothing.  n_g <= HG_FRAG_MAX_GRID_Y.
hipError_t hg_frag_launch_fold(hipStream_t st, unsigned long long *d_keys, uint32_t g0, uint32_t n_g, uint32_t Q, const uint32_t *d_qry_first,
                               uint32_t n_qry, uint32_t m_th, hg_frag_pair *d_pair, bool to_best);
