// hg_kmer_kernels.hip -- FracMinHash k-mer hash + threshold sample on gfx950.
//
// Computes what extract_kmer_hash (src/sketch.rs:71-98) / cuda_kmer_t1ha2
// (src/cuda_kernel.cu:250-321) compute: for every k-window of ACGT bases the canonical
// strand's ASCII bytes are hashed with t1ha2_atonce(seed) and hashes below the threshold
// are kept.  The design is MI355X-first, not the reference's (1 thread x 512 k-mers with
// two 544-byte scratch arrays):
//
//  * kmer_sample_shared<K, CANON> (k = 1..32): a workgroup stages its tile -- 254 lanes x 12 k-mer starts -- in LDS
//    once, classified 4 bases per instruction (SWAR on dwords: 2-bit codes, upper-cased ASCII and complement ASCII
//    from v_perm_b32 lookups, validity from one XOR), as a forward image and a reverse-complement image in all four
//    byte phases, so that both strands of every k-mer are runs of whole dwords;
//  * the canonical strand is chosen by ONE compare of 2-bit packed k-mers (A<C<G<T holds both in ASCII and in the 2-bit
//    code, so this equals the reference's byte-wise compare, src/cuda_kernel.cu:306-311; 32-bit on the top 16 bases for
//    odd k, 64-bit for even k) and becomes an
//    ADDRESS: one v_cndmask picks the image, the hash words are ds_reads with immediate offsets -- no instruction
//    touches the bytes;
//  * t1ha2 is specialised per k; for k = 17..32 the whole k-mer body (word reads, three or four mixup64 stages,
//    final64, candidate compare on the high dword) is one asm statement on fixed register pairs: 54 / 63 vector
//    instructions, 24 / 29 of them v_mad_u64_u32 (the first mixup multiplies a bounded operand: HG_KS_MUL128_BOUNDED; the
//    products with P1 and P3 have no carry op: HG_KS_MUL128_NC);
//  * survivors (1/scaled of the k-mers) are staged in a small LDS list and the workgroup reserves its range of the
//    genome's hit slice with ONE global atomic at the end of its work item; lossless: no 8-slot cap like
//    src/cuda_kernel.cu:316, hash value 0 is kept;
//  * kmer_sample_long (k = 33..255): run-time k, t1ha2's long-input loop.
// Predecessors, removed from the source after the shared-image kernel replaced them for every k (DESIGN.md 4.1 has
// their measurements): kmer_sample_fast (32-base register windows), kmer_sample_grouped (56-base windows, per-lane
// LDS images, run-time byte shifts), kmer_sample_fast64 (64-base windows).
//
// The kernel is integer-VALU bound, not HBM bound.
//
// One translation unit: the headers included below are parts of this file and of nothing else; here are the host functions.
// The source has no compile-time switches for alternatives that were measured and dropped: an A/B against any of them is a
// build of the parent commit (tools/build_variant.sh builds one translation unit into a library of its own).
#include <cstdlib>
#include <utility>

#include "hg_internal.h"

namespace {
constexpr int WG = 256;                              // lanes per workgroup
constexpr int GEN_STARTS = 48;                       // long-k kernel: starts per lane and work item (eight tiles of 1 536)
constexpr int GEN_ITEM = WG * GEN_STARTS;            // and per work item
}  // namespace

#include "hg_kmer_t1ha2.h"   // the hash: primes, 128-bit products, mixup64 / final64, t1ha2 for k <= 16 and k > 32
#include "hg_kmer_asm.h"     // the k-mer body of k = 17..32 as assembly text and asm statements
#include "hg_kmer_bases.h"   // four bases at a time: ASCII dword -> codes, strand bytes, validity
#include "hg_kmer_hits.h"    // the LDS hit list and its flushes
#include "hg_kmer_shared.h"  // kmer_sample_shared and its parts
#include "hg_kmer_long.h"    // kmer_sample_long

const char *hg_kmer_kernel_name(uint32_t k, bool canonical, bool packed) {  // mirrors hg_launch_kmer_sample
  static thread_local char buf[64];
  if (k > 32) {
    snprintf(buf, sizeof buf, "kmer_sample_long<%u, %s>", k <= 64 ? k : 0u, packed ? "true" : "false");
    return buf;
  }
  snprintf(buf, sizeof buf, "kmer_sample_shared<%u, %s, %s>", k, canonical ? "true" : "false", packed ? "true" : "false");
  return buf;
}

uint32_t hg_kmer_item_starts(uint32_t k) {
  if (k > 32) return GEN_ITEM;
  return k >= 22 ? (uint32_t)GeoS<32>::ITEM : (uint32_t)GeoS<21>::ITEM;  // (the same within each code-window class)
}

uint32_t hg_kmer_tile_starts(uint32_t k) {
  if (k > 32) return 0;  // (kmer_sample_long takes one item per workgroup)
  return k >= 22 ? (uint32_t)GeoS<32>::TILE : (uint32_t)GeoS<21>::TILE;
}
// tiles a workgroup takes at most when the plan groups the work items of small genomes: three full items' worth (27 genomes of
// up to 3 kbp, 6 of 10 kbp; an item that fills its TILES tiles alone still has a workgroup of its own)
uint32_t hg_kmer_item_tiles(uint32_t k) { return k > 32 ? 0u : 3u * (uint32_t)GeoS<21>::TILES; }

hipError_t hg_launch_kmer_sample(hipStream_t st, const uint8_t *d_seq, const hg_genome_meta *d_meta,
                                 const uint32_t *d_item_genome, uint32_t n_items, uint32_t ksize,
                                 uint64_t threshold, uint64_t seed, bool canonical, uint32_t norm_mode,
                                 uint64_t *d_hits, uint32_t *d_cnt, bool packed, const uint32_t *d_group_first,
                                 uint32_t n_groups) {
  if (n_items == 0) return hipSuccess;
  if (ksize > 32 || n_groups == 0) d_group_first = nullptr;
  const uint32_t n_wg = d_group_first ? n_groups : n_items;
  const uint32_t u2t = (norm_mode == HG_NORM_U2T && !packed) ? 1u : 0u;  // (a blob was normalised when it was packed)
  // entries of a work item's LDS hit list: twice what one tile is expected to sample (+ slack), 256 .. 4 096
  auto stage_entries = [&](uint32_t tile_starts) {
    const double per_tile = (double)tile_starts * ((double)threshold / 18446744073709551616.0);
    uint32_t cap = HIT_STAGE;
    while (cap < HIT_STAGE_MAX && (double)cap < 2.0 * per_tile + 128.0) cap <<= 1;
    return cap;
  };
  const uint32_t cap_s = stage_entries((uint32_t)GeoS<21>::TILE), cap_l = stage_entries(LONG_TILE);
#define HG_K_LAUNCH(KK, CN, PK)                                                                            \
  hipLaunchKernelGGL((kmer_sample_shared<KK, CN, PK>), dim3(n_wg), dim3(WG), cap_s * sizeof(uint64_t), st, d_seq, d_meta, \
                     d_item_genome, threshold, seed, u2t, d_hits, d_cnt, cap_s, d_group_first)
#define HG_K_CASE(KK)                                                                                     \
  case KK:                                                                                                \
    if (canonical && packed) HG_K_LAUNCH(KK, true, true);                                                 \
    else if (canonical) HG_K_LAUNCH(KK, true, false);                                                     \
    else if (packed) HG_K_LAUNCH(KK, false, true);                                                        \
    else HG_K_LAUNCH(KK, false, false);                                                                   \
    return hipGetLastError();
  switch (ksize) {
    HG_K_CASE(1) HG_K_CASE(2) HG_K_CASE(3) HG_K_CASE(4) HG_K_CASE(5) HG_K_CASE(6) HG_K_CASE(7) HG_K_CASE(8)
    HG_K_CASE(9) HG_K_CASE(10) HG_K_CASE(11) HG_K_CASE(12) HG_K_CASE(13) HG_K_CASE(14) HG_K_CASE(15) HG_K_CASE(16)
    HG_K_CASE(17) HG_K_CASE(18) HG_K_CASE(19) HG_K_CASE(20) HG_K_CASE(21) HG_K_CASE(22) HG_K_CASE(23) HG_K_CASE(24)
    HG_K_CASE(25) HG_K_CASE(26) HG_K_CASE(27) HG_K_CASE(28) HG_K_CASE(29) HG_K_CASE(30) HG_K_CASE(31) HG_K_CASE(32)
    default:
      break;
  }
#undef HG_K_CASE
#undef HG_K_LAUNCH
  // 33 <= k <= 255: k up to 64 as a compile-time constant
#define HG_KL_LAUNCH(PK, KK)                                                                                                   \
  hipLaunchKernelGGL((kmer_sample_long<KK, PK>), dim3(n_items), dim3(WG), cap_l * sizeof(uint64_t), st, d_seq, d_meta, d_item_genome, \
                     ksize, threshold, seed, canonical ? 1u : 0u, u2t, d_hits, d_cnt, cap_l)
#define HG_KL_CASE(KK)                        \
  case KK:                                    \
    if (packed) HG_KL_LAUNCH(true, KK);       \
    else HG_KL_LAUNCH(false, KK);             \
    return hipGetLastError();
  switch (ksize) {
    HG_KL_CASE(33) HG_KL_CASE(34) HG_KL_CASE(35) HG_KL_CASE(36) HG_KL_CASE(37) HG_KL_CASE(38) HG_KL_CASE(39) HG_KL_CASE(40)
    HG_KL_CASE(41) HG_KL_CASE(42) HG_KL_CASE(43) HG_KL_CASE(44) HG_KL_CASE(45) HG_KL_CASE(46) HG_KL_CASE(47) HG_KL_CASE(48)
    HG_KL_CASE(49) HG_KL_CASE(50) HG_KL_CASE(51) HG_KL_CASE(52) HG_KL_CASE(53) HG_KL_CASE(54) HG_KL_CASE(55) HG_KL_CASE(56)
    HG_KL_CASE(57) HG_KL_CASE(58) HG_KL_CASE(59) HG_KL_CASE(60) HG_KL_CASE(61) HG_KL_CASE(62) HG_KL_CASE(63) HG_KL_CASE(64)
    default:
      break;
  }
#undef HG_KL_CASE
  if (packed) HG_KL_LAUNCH(true, 0);
  else HG_KL_LAUNCH(false, 0);
#undef HG_KL_LAUNCH
  return hipGetLastError();
}
