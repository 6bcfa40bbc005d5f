// hg_tx.h -- what the two translation units of libhypergen_tx.so share (not installed): the base classification and the
// codon translation as plain C++ for host and device -- the kernel fills its LDS tables from the very functions
// hg_tx_translate_frame runs on the host, so a CPU test of the frame strings is a test of the kernel's tables -- and the
// launcher.  t1ha2 for at most 32 bytes is hg_aa.h's, the kernel's geometry (HG_TX_*) hg_kmer_window.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hg_aa.h"

// ---- bases --------------------------------------------------------------------------------------------------------------
// The code of byte value c (0..255): 0 A, 1 C, 2 T, 3 G -- bits 1..2 of the ASCII letter, in either case -- or HG_TX_NOT_A_BASE
// for every other byte (N, IUPAC codes, U, ...).  The complement of a code is code ^ 2.
constexpr uint32_t HG_TX_NOT_A_BASE = 4;
__host__ __device__ inline uint32_t hg_tx_base_code(uint32_t c) {
  const uint32_t u = c & 0xDFu;  // a..z -> A..Z; no byte outside the letters lands on one of the four
  const bool base = c < 0x80u && (u == 0x41u || u == 0x43u || u == 0x47u || u == 0x54u);
  return base ? (c >> 1) & 3u : HG_TX_NOT_A_BASE;
}

// ---- codons (NCBI table 1) ------------------------------------------------------------------------------------------------
// the residue of the codon with base codes (b1, b2, b3): the published table is indexed with bases ordered T, C, A, G
__host__ __device__ inline uint8_t hg_tx_codon(uint32_t b1, uint32_t b2, uint32_t b3) {
  // code (A C T G = 0 1 2 3) -> rank in T C A G: 2 1 0 3
  const uint32_t r1 = b1 ^ ((~b1 & 1u) << 1), r2 = b2 ^ ((~b2 & 1u) << 1), r3 = b3 ^ ((~b3 & 1u) << 1);
  return (uint8_t)"FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"[16u * r1 + 4u * r2 + r3];
}
// The kernel's two tables, both indexed by i = 16 * code(s[q]) + 4 * code(s[q + 1]) + code(s[q + 2]): the residue of the three
// bases read forward, and read on the other strand (complemented, last base first) -- a permutation of the first.
__host__ __device__ inline uint8_t hg_tx_table_fwd(uint32_t i) { return hg_tx_codon((i >> 4) & 3u, (i >> 2) & 3u, i & 3u); }
__host__ __device__ inline uint8_t hg_tx_table_rev(uint32_t i) { return hg_tx_codon((i & 3u) ^ 2u, ((i >> 2) & 3u) ^ 2u, ((i >> 4) & 3u) ^ 2u); }
// what a codon holding a byte that is no base translates to; like '*' it is not a residue
constexpr uint8_t HG_TX_X = 'X', HG_TX_STOP = '*';

// The hash + sample launch over all work items of a plan (an hg_kmer_hook): one workgroup per work item.
hipError_t hg_tx_launch_kmer_sample(hipStream_t st, const uint8_t *d_seq, const hg_genome_meta *d_meta, const uint32_t *d_item_genome,
                                    uint32_t n_items, uint32_t ksize, uint64_t threshold, uint64_t seed, uint64_t *d_hits, uint32_t *d_cnt);
