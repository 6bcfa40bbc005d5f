// hg_dense_matrix.h -- the dense n x n matrix of the schemes that hold one (hg_cluster_average.hip, hg_cluster_complete.hip,
// hg_nj.hip), one copy of each part: the allocation that lives for one call, the bodies and launchers of the fill and the
// mirror kernels, and the row-block driver of the forms that take resident sketches, which hg_cluster_stats.hip runs too
// (it reads the blocks and holds no matrix).  Every scheme keeps its own __global__ wrappers around the bodies, so that a
// profile tells the schemes apart; a wrapper hands its launch geometry in, because a body is optimised before it is inlined
// and does not see the kernel's launch bounds.
#pragma once
#include <algorithm>
#include <functional>
#include <string>

#include "hg_internal.h"

constexpr uint32_t DENSE_NONE = 0xFFFFFFFFu;  // no name: no partner, no pair, no join
constexpr uint32_t MIRROR_TILE = 32;

// a lane's first index and the stride of a grid-stride loop, as a kernel wrapper spells them for its body
#define HG_LANE0 ((size_t)blockIdx.x * blockDim.x + threadIdx.x)
#define HG_LANES ((size_t)gridDim.x * blockDim.x)

// the matrix, released when the call returns (hipFree waits for the device)
struct MatrixHold {
  void *p = nullptr;
  ~MatrixHold() {
    if (p) (void)hipFree(p);
  }
};
inline hg_status hg_matrix_alloc(hg_ctx *c, MatrixHold &hold, size_t bytes, const char *scheme) {
  const hipError_t e = hipMalloc(&hold.p, bytes);
  if (e == hipSuccess) return HG_OK;
  hold.p = nullptr;
  return hg_fail(c, HG_ERR_OOM, "hipMalloc(" + std::to_string(bytes) + ") for the matrix of " + scheme + ": " + hipGetErrorString(e));
}

// Rows [r0, r0 + rows) of the matrix from a block of ANI values: blk[r * pitch + (j - c0)] is ani(r0 + r, j), c0 <= r0.
// Only j > row is read; the diagonal, the lower triangle (the mirror kernel writes it) and the padding columns become 0.
// Quant: the scheme's integer of an ANI value.  (j0, jstride): the lane's first column and the columns of the grid's x.
template <typename T, typename Quant>
__device__ __forceinline__ void matrix_fill_body(const float *__restrict__ blk, size_t pitch, uint32_t c0, uint32_t r0, uint32_t rows, uint32_t n,
                                                 size_t ld, T *__restrict__ M, size_t j0, size_t jstride) {
  for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const uint32_t gi = r0 + r;
    const float *src = blk + (size_t)r * pitch;
    T *dst = M + (size_t)gi * ld;
    for (size_t j = j0; j < ld; j += jstride) dst[j] = (j > gi && j < n) ? Quant()(src[j - c0]) : (T)0;
  }
}

// M[j][i] = M[i][j] for i < j: tiles of 32 x 32 through LDS (the column padded by one word against bank conflicts), the
// workgroups of the upper triangle of tiles each write their transposed tile (a diagonal tile its own lower half).
// blockDim = (32, 8).
template <typename T>
__device__ __forceinline__ void matrix_mirror_body(T *M, uint32_t n, size_t ld) {
  __shared__ T tile[MIRROR_TILE][MIRROR_TILE + 1];
  if (blockIdx.x < blockIdx.y) return;  // (uniform over the workgroup)
  const uint32_t row0 = blockIdx.y * MIRROR_TILE, col0 = blockIdx.x * MIRROR_TILE;
  for (uint32_t k = threadIdx.y; k < MIRROR_TILE; k += 8) {
    const uint32_t i = row0 + k, j = col0 + threadIdx.x;
    tile[k][threadIdx.x] = (i < n && j < n) ? M[(size_t)i * ld + j] : (T)0;
  }
  __syncthreads();
  for (uint32_t k = threadIdx.y; k < MIRROR_TILE; k += 8) {
    const uint32_t j = col0 + k, i = row0 + threadIdx.x;  // writes M[j][i], the value of M[i][j]
    if (j < n && i < j) M[(size_t)j * ld + i] = tile[threadIdx.x][k];
  }
}

// the launches of a scheme's fill and mirror kernels
template <typename T>
using matrix_fill_fn = void (*)(const float *, size_t, uint32_t, uint32_t, uint32_t, uint32_t, size_t, T *);
template <typename T>
hg_status hg_matrix_fill(hg_ctx *c, matrix_fill_fn<T> kernel, T *M, size_t ld, const float *blk, size_t pitch, size_t c0, size_t r0, size_t rows,
                         size_t n) {
  hg_timed tm(c, HG_T_DIST);
  const dim3 grid((unsigned)std::min<size_t>((ld + 255) / 256, 64), (unsigned)std::min<size_t>(rows, 16384));
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->stream, blk, pitch, (uint32_t)c0, (uint32_t)r0, (uint32_t)rows, (uint32_t)n, ld, M);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}
template <typename T>
hg_status hg_matrix_mirror(hg_ctx *c, void (*kernel)(T *, uint32_t, size_t), T *M, size_t n, size_t ld) {
  hg_timed tm(c, HG_T_DIST);
  const unsigned tiles = (unsigned)((n + MIRROR_TILE - 1) / MIRROR_TILE);
  hipLaunchKernelGGL(kernel, dim3(tiles, tiles), dim3(MIRROR_TILE, 8), 0, c->stream, M, (uint32_t)n, ld);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

// what the forms that take resident sketches check behind their NULL arguments
inline hg_status hg_sketch_dims_check(hg_ctx *c, uint32_t hv_d, uint32_t ksize) {
  if (hv_d == 0 || hv_d > 65536) return hg_fail(c, HG_ERR_UNSUPPORTED, "hv_d must be in 1..65536");
  if (ksize == 0) return hg_fail(c, HG_ERR_INVALID, "ksize must be >= 1");
  return HG_OK;
}

// The ANI matrix of n resident sketches as row blocks in the search's scratch block, at most HG_SEARCH_BLOCK_BYTES each
// (block_rows != 0, a scheme's "*_block_rows" hook, forces the row count): rows [r0, r0 + rows) x columns [c0, n) from
// hg_dist_full_dev, blk[r * pitch + (j - c0)] = ani(r0 + r, j); c0 = r0 for a scheme that reads the upper triangle (the
// first block is the widest), c0 = 0 for one that reads whole rows.  begin() runs once the scratch block stands, before
// the first block; block() must have queued all its reads of blk before it returns.
using hg_matrix_block_fn = std::function<hg_status(const float *blk, size_t pitch, size_t c0, size_t r0, size_t rows)>;
inline hg_status hg_matrix_row_blocks(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                      uint64_t block_rows, bool triangle, const std::function<hg_status()> &begin,
                                      const hg_matrix_block_fn &block) {
  hg_status s;
  const size_t fit = std::max<size_t>(1, HG_SEARCH_BLOCK_BYTES / (sizeof(float) * n));
  const size_t rb = std::min<size_t>(n, block_rows ? (size_t)block_rows : fit);
  if ((s = hg_ensure(c, c->w_srch_blk, rb * n * sizeof(float))) != HG_OK) return s;
  auto *blk = static_cast<float *>(c->w_srch_blk.p);
  if ((s = begin()) != HG_OK) return s;
  for (size_t r0 = 0; r0 < n; r0 += rb) {
    const size_t rows = std::min(rb, n - r0), c0 = triangle ? r0 : 0, cols = n - c0;
    if ((s = hg_dist_full_dev(c, d_hv + r0 * (size_t)hv_d, d_norm2 + r0, rows, d_hv + c0 * (size_t)hv_d, d_norm2 + c0, cols, hv_d, ksize, blk)) !=
        HG_OK)
      return s;
    if ((s = block(blk, cols, c0, r0, rows)) != HG_OK) return s;
  }
  return HG_OK;
}
