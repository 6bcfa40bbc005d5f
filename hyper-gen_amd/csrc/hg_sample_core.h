// hg_sample_core.h -- the device code aa_kmer_sample_kernel and tx_kmer_sample_kernel share (not installed): the LDS hit
// stage with its append and flush, the sample step of one gathered k-mer (hash, compare, stage), the wide load type and the
// dispatch of KW = ceil(k / 8) onto a kernel template.  The window's integer arithmetic is hg_kmer_window.h's, t1ha2 hg_aa.h's.
// A kernel keeps what is its own: staging, the residue or codon classification, the tile walk.
//
// The nucleotide kernels (hg_kmer_kernels.hip) keep their own append_hit and stage on purpose: their stage is dynamic LDS
// sized at launch, not a member of a static struct, their translation unit is built with its own -mllvm option, and they are
// the headline kernels -- sharing code with them would put their generated code at stake for nothing they need.
#pragma once
#include "hg_aa.h"

// sampled hashes waiting for a flush; n_hits counts past N when the stage is full
template <uint32_t N>
struct HgHitStage {
  uint64_t hits[N];
  uint32_t n_hits, base;
};

// the hit region's slots [base, base + n) reserved with one atomic for all lanes of the wave that are here together
__device__ __forceinline__ void append_hit(uint64_t h, const hg_genome_meta &gm, uint32_t g, uint64_t *__restrict__ hits,
                                           uint32_t *__restrict__ cnt) {
  const unsigned long long m = __ballot(1);
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(&cnt[g], (uint32_t)__popcll(m));
  base = __builtin_amdgcn_readfirstlane(base);  // (the first active lane is the one that asked)
  const uint32_t idx = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (idx < gm.hit_cap) hits[gm.hit_off + idx] = h;
}

// Empties the stage into the genome's hit region (the raw counter keeps counting past hit_cap).  Two barriers; every lane
// of the workgroup of WG lanes calls it.  The caller's next barrier lies between this call's reads and the next hit.
template <uint32_t WG, uint32_t N>
__device__ __forceinline__ void flush_stage(HgHitStage<N> &s, const hg_genome_meta &gm, uint32_t g, uint64_t *__restrict__ hits,
                                            uint32_t *__restrict__ cnt) {
  __syncthreads();
  const uint32_t n = s.n_hits < N ? s.n_hits : N;
  if (threadIdx.x == 0 && n) s.base = atomicAdd(&cnt[g], n);
  __syncthreads();
  const uint32_t base = s.base;
  for (uint32_t i = threadIdx.x; i < n; i += WG) {
    const uint32_t idx = base + i;
    if (idx < gm.hit_cap) hits[gm.hit_off + idx] = s.hits[i];
  }
  __syncthreads();  // (n_hits and base have been read by every lane)
  if (threadIdx.x == 0) s.n_hits = 0;
}

// what a window needs beside its place: the same for every window of a launch
struct HgWindowParams {
  uint32_t ksize, win_mask;
  uint64_t tail_mask, threshold, seed;
};
// the k-mer of the KW words w (hg_win_gather's): hashed, and if sampled staged, or appended when the stage is full
template <int KW, uint32_t N>
__device__ __forceinline__ void sample_kmer(HgHitStage<N> &s, const uint64_t *w, const HgWindowParams &wn, const hg_genome_meta &gm,
                                            uint32_t g, uint64_t *hits, uint32_t *cnt) {
  const uint64_t h = hg_aa_t1ha2::hash_words<KW>(w, wn.ksize, wn.seed);
  if (h < wn.threshold) {
    const uint32_t idx = atomicAdd(&s.n_hits, 1u);
    if (idx < N) s.hits[idx] = h;
    else append_hit(h, gm, g, hits, cnt);
  }
}

typedef uint32_t __attribute__((ext_vector_type(4), aligned(4))) u32x4_a4;  // 16 bytes at a 4-byte aligned address

// kernel<ceil(ksize / 8)> over n_items workgroups of wg lanes on stream st, 1 <= ksize <= 32
#define HG_LAUNCH_BY_KW(kernel, ksize, n_items, wg, st, ...)                                              \
  switch (((ksize) + 7) / 8) {                                                                            \
    case 1: hipLaunchKernelGGL((kernel<1>), dim3(n_items), dim3(wg), 0, st, __VA_ARGS__); break;          \
    case 2: hipLaunchKernelGGL((kernel<2>), dim3(n_items), dim3(wg), 0, st, __VA_ARGS__); break;          \
    case 3: hipLaunchKernelGGL((kernel<3>), dim3(n_items), dim3(wg), 0, st, __VA_ARGS__); break;          \
    default: hipLaunchKernelGGL((kernel<4>), dim3(n_items), dim3(wg), 0, st, __VA_ARGS__); break;         \
  }
