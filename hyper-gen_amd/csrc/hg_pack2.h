// hg_pack2.h -- the hg_pack2 blob layout (include/hypergen.h) as arithmetic and the job records of hg_pack2_kernels.hip.  No HIP
// include: read by host-only code (hg_formats.cpp, hg_stream_layout.h), by .hip host code and by kernels (constexpr: both sides).
#pragma once
#include <stdint.h>

// a blob of n bases: [2-bit codes, 4 per byte][not-a-base bitmap, 1 bit per base], each area padded to 16 bytes
constexpr uint64_t hg_pack2_code_bytes(uint64_t n) { return ((n + 3) / 4 + 15) & ~(uint64_t)15; }
constexpr uint64_t hg_pack2_mask_bytes(uint64_t n) { return ((n + 7) / 8 + 15) & ~(uint64_t)15; }

// one packed genome of a chunk: where its blob sits in the chunk's packed area, where its ASCII goes
struct UnpackJob {
  uint64_t pk_off, out_off, n_bps, mask_off;  // (mask_off: where the genome's not-a-base bitmap lies in the packed area)
  uint32_t first_block, pad;
};
// one sparse genome of a chunk: its run table lies behind its codes, its bitmap is rebuilt at mask_off
struct SparseJob {
  uint64_t codes_off, mask_off, n_bps;
  uint32_t first_block, pad;
};
constexpr uint32_t SLICE_WORDS = 1024;  // bitmap words one workgroup rebuilds: 4 KiB = 32 768 bases
constexpr uint32_t UNPACK_GROUPS_PER_BLOCK = 1024;  // 256 threads x 4 groups of 16 bases
// workgroups a genome of n bases takes in unpack2_kernel / expand_runs_kernel (its job's share of the grid)
constexpr uint32_t hg_unpack2_blocks(uint64_t n) { return (uint32_t)(((n + 15) / 16 + UNPACK_GROUPS_PER_BLOCK - 1) / UNPACK_GROUPS_PER_BLOCK); }
constexpr uint32_t hg_expand_runs_blocks(uint64_t n) { return (uint32_t)((hg_pack2_mask_bytes(n) / 4 + SLICE_WORDS - 1) / SLICE_WORDS); }
