// hg_kmer_hits.h -- where the k-mer kernels put a sampled hash: a workgroup's LDS list (the kernels' dynamic LDS), flushed
// to the genome's hit slice with one global atomic per flush, and the wave-aggregated global path behind a full list.
// Separate from hg_sample_core.h, which gives the reasons.  Included by hg_kmer_kernels.hip only.  Expects: hg_internal.h
// (hg_genome_meta); hg_launch_kmer_sample sizes the list from HIT_STAGE .. HIT_STAGE_MAX.
#pragma once
namespace {

// One hit straight to the genome's list.  The lanes of a wave that arrive here together (a divergent branch: g is
// wave-uniform) reserve their slots with ONE atomic: the counters of a genome are one address for all of its work items,
// and per-lane atomics on it serialise at ~3.5 ns each (1 000 x 5 Mbp at scaled = 50, when every work item overflowed its
// LDS list by 300 hits: 194 ms instead of 9).
__device__ __forceinline__ void append_hit(uint64_t h, const hg_genome_meta &gm, uint32_t g,
                                           uint64_t *__restrict__ hits, uint32_t *__restrict__ cnt) {
  const unsigned long long m = __ballot(1);  // the lanes in this branch
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(&cnt[g], (uint32_t)__popcll(m));
  base = __builtin_amdgcn_readfirstlane(base);  // (the first active lane is the one that asked)
  const uint32_t idx = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (idx < gm.hit_cap) hits[gm.hit_off + idx] = h;
}

// Workgroup-level staging of the sampled hashes.  A hit is 1 k-mer in `scaled`, but every
// one used to cost its wave a returning global atomic -- a full memory round trip in the middle of ~1 400
// VALU instructions, about once per two tiles per wave.  Hits go to an LDS list instead (LDS atomic) and the
// workgroup reserves its range of the genome's hit buffer once, at the end of its work item.  A list that
// overflows (low-complexity sequence: every position of a repeat samples the same hash) spills straight to
// the global path; the raw counter semantics (it keeps counting past the capacity) are unchanged.
constexpr uint32_t HIT_STAGE = 256, HIT_STAGE_MAX = 4096;
struct HitStage {
  uint32_t n, base;
};
// The list itself is the kernels' dynamic LDS: `cap` entries, HIT_STAGE at the default sampling rate and up to HIT_STAGE_MAX
// when a tile alone yields hundreds of hits (hg_launch_kmer_sample sizes it: scaled = 5 samples 610 of a tile's 3 048
// starts, and a list of 256 sent the rest through a global atomic per wave and k-mer step -- 168 ms for 1 000 x 5 Mbp).
extern __shared__ __attribute__((aligned(8))) uint64_t s_stage_h[];
__device__ __forceinline__ void stage_hit(HitStage &st, uint32_t cap, uint64_t h, const hg_genome_meta &gm, uint32_t g,
                                          uint64_t *__restrict__ hits, uint32_t *__restrict__ cnt) {
  const uint32_t idx = atomicAdd(&st.n, 1u);
  if (idx < cap) s_stage_h[idx] = h;
  else append_hit(h, gm, g, hits, cnt);
}
// AGAIN: the list is emptied between two tiles and filled again afterwards (the caller's next barrier lies between this
// call's reads and the next writes)
template <bool AGAIN = false>
__device__ __forceinline__ void flush_hits(HitStage &st, uint32_t cap, const hg_genome_meta &gm, uint32_t g,
                                           uint64_t *__restrict__ hits, uint32_t *__restrict__ cnt) {
  __syncthreads();
  const uint32_t n = st.n < cap ? st.n : cap;
  if (threadIdx.x == 0 && n) st.base = atomicAdd(&cnt[g], n);
  __syncthreads();
  if (AGAIN && threadIdx.x == 0) st.n = 0;  // (every lane has read it)
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    const uint32_t idx = st.base + i;
    if (idx < gm.hit_cap) hits[gm.hit_off + idx] = s_stage_h[i];
  }
}
// Between two tiles (behind the barrier that ends a tile: st.n is final and the same for every lane): a list that is a
// quarter full goes out now.  At the default sampling rate a work item collects ~18 hits and never gets here; a denser
// sketch (scaled = 100: 270 hits per item) used to overflow the list and pay a global atomic per hit.
__device__ __forceinline__ void flush_hits_if_filling(HitStage &st, uint32_t cap, const hg_genome_meta &gm, uint32_t g,
                                                      uint64_t *__restrict__ hits, uint32_t *__restrict__ cnt) {
  if (st.n >= cap / 4) flush_hits<true>(st, cap, gm, g, hits, cnt);  // workgroup-uniform
}
// Whether the sampling rate can fill a quarter of the list within one work item at all (a kernel argument: the test
// between the tiles is a scalar branch that the default rate, 1 in 1 500, never takes -- the LDS read of the fill level
// cost the headline 0.2 %): more than ~32 expected hits per 27 000 starts, i.e. scaled < 850.  (A repeat that piles more hits than that into an
// item of a sparse sketch overflows the list as before; those hits go out one atomic per wave.)
__device__ __forceinline__ bool dense_sampling(uint64_t threshold) { return threshold > (~0ull / 850ull); }
}  // namespace
