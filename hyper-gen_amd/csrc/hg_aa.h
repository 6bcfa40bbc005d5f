// hg_aa.h -- what the two translation units of libhypergen_aa.so share (not installed): the residue test and t1ha2 for at
// most 32 bytes, both as plain C++ for host and device (the host forms are what a stand-alone CPU check of the kernel's
// arithmetic compiles), and the launcher.  The kernel's geometry (HG_AA_*) is hg_kmer_window.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hg_internal.h"
#include "hg_kmer_window.h"

// bit (c - 'A') set <=> upper-case letter c is one of ACDEFGHIKLMNPQRSTVWY
constexpr uint32_t HG_AA_LETTERS = (1u << 0) | (1u << 2) | (1u << 3) | (1u << 4) | (1u << 5) | (1u << 6) | (1u << 7) | (1u << 8) |
                                   (1u << 10) | (1u << 11) | (1u << 12) | (1u << 13) | (1u << 15) | (1u << 16) | (1u << 17) |
                                   (1u << 18) | (1u << 19) | (1u << 21) | (1u << 22) | (1u << 24);
// whether byte value c (0..255) is a residue, in either case: clearing bit 5 maps a..z onto A..Z and nothing else into A..Z
__host__ __device__ inline bool hg_aa_is_residue(uint32_t c) {
  const uint32_t idx = (c & 0xDFu) - 0x41u;
  return idx < 26u && ((HG_AA_LETTERS >> idx) & 1u) != 0u;
}

// ---- t1ha2_atonce for 1..32 bytes (published t1ha2; the tail switch of src/cuda_kernel.cu:205-245) ----------------------
namespace hg_aa_t1ha2 {
constexpr uint64_t P0 = 0xEC99BF0D8372CAABull, P1 = 0x82434FE90EDCEF39ull, P2 = 0xD4F06DB99D67BE4Bull, P3 = 0xBD9CACC22C6E9571ull;
constexpr uint64_t P4 = 0x9C06FAF4D023E3ABull, P5 = 0xC060724A8424F345ull, P6 = 0xCB5AF53AE3AAAC31ull;
__host__ __device__ inline uint64_t rot64(uint64_t v, unsigned s) { return (v >> s) | (v << (64 - s)); }  // rotate right, 0 < s < 64
__host__ __device__ inline void mixup64(uint64_t &a, uint64_t &b, uint64_t v, uint64_t prime) {
  const unsigned __int128 m = (unsigned __int128)(b + v) * prime;
  a ^= (uint64_t)m;
  b += (uint64_t)(m >> 64);
}
__host__ __device__ inline uint64_t final64(uint64_t a, uint64_t b) {
  const uint64_t x = (a + rot64(b, 41)) * P0;
  const uint64_t y = (rot64(a, 23) + b) * P6;
  const unsigned __int128 m = (unsigned __int128)(x ^ y) * P5;
  return (uint64_t)m ^ (uint64_t)(m >> 64);
}
// len bytes as KW = ceil(len / 8) little-endian words, the bytes of the last word behind the k-mer zero
template <int KW>
__host__ __device__ inline uint64_t hash_words(const uint64_t *w, uint32_t len, uint64_t seed) {
  static_assert(KW >= 1 && KW <= 4, "t1ha2's path for at most 32 bytes");
  uint64_t a = seed, b = (uint64_t)len;
  int i = 0;
  if (KW > 3) mixup64(a, b, w[i++], P4);
  if (KW > 2) mixup64(b, a, w[i++], P3);
  if (KW > 1) mixup64(a, b, w[i++], P2);
  mixup64(b, a, w[i], P1);
  return final64(a, b);
}
}  // namespace hg_aa_t1ha2

// The hash + sample launch over all work items of a plan (an hg_kmer_hook): one workgroup per work item.
hipError_t hg_aa_launch_kmer_sample(hipStream_t st, const uint8_t *d_seq, const hg_genome_meta *d_meta, const uint32_t *d_item_genome,
                                    uint32_t n_items, uint32_t ksize, uint64_t threshold, uint64_t seed, uint64_t *d_hits, uint32_t *d_cnt);
