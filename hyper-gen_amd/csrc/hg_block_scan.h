// hg_block_scan.h -- block-wide scan primitives shared by the device kernels (hg_hits.hip: radix sort; hg_cluster.hip: dense
// cluster ids; hg_sort_kernels.hip: counting sort and unique).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// block-wide exclusive scan of one value per thread (WAVES * 64 threads); returns the block total through *total
template <uint32_t WAVES>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *s_wave /* WAVES words */, uint32_t *total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(inc, o);
    if (lane >= (uint32_t)o) inc += up;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < WAVES; ++w) {
    const uint32_t t = s_wave[w];
    before += w < wave ? t : 0u, all += t;
  }
  __syncthreads();  // (s_wave may be reused by the caller's next round)
  *total = all;
  return before + inc - v;
}
