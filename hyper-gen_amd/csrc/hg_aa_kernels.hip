// hg_aa_kernels.hip -- amino-acid k-mer hash + FracMinHash sample on gfx950 (libhypergen_aa.so).
//
// For every window of k residues (ACDEFGHIKLMNPQRSTVWY in either case, 1 <= k <= 32) of a proteome the k bytes, upper-cased,
// are hashed with t1ha2_atonce(seed) and hashes below the threshold are kept: the protein twin of hg_kmer_kernels.hip with
// one strand, no canonical choice and a 20-letter alphabet (include/hypergen_aa.h is the specification).  The kernel reads
// the tables of the nucleotide library's plan as they are -- hg_genome_meta, work item -> genome, hg_kmer_item_starts(k)
// starts per work item -- and fills the same hit regions and raw counters, so sort / unique, the encoders and the
// overflow-and-regrow path behind it are the nucleotide library's, unchanged.
//
//  * one work item per workgroup of 256 lanes; the item is walked in tiles of HG_AA_TILE = 4 032 starts;
//  * a tile is staged once: every lane loads 16 bytes (one global_load_dwordx4), clears bit 5 of every byte (a..z -> A..Z; what
//    it does to other bytes does not matter, their windows are never hashed), tests every byte for "is a residue" with bit
//    arithmetic on a 26-bit letter mask and writes its 16 bytes and its 16 not-a-residue bits to LDS: a 4 KiB byte image and a
//    512-byte bit image.  Bytes behind the proteome's end are not residues.  Loads start inside the proteome and so end at
//    most 15 bytes behind it (the caller leaves 32);
//  * lane t takes the starts t, t + 256, ... of the tile.  A start p tests bits [p, p + k) of the bit image (one funnel shift;
//    skipped when the whole tile is clean), reads the dwords of its k-mer -- 256 is a multiple of 4, so a lane's byte phase is
//    the same for all of its starts -- shifts them into ceil(k / 8) little-endian words, masks the last to k mod 8 bytes and
//    runs t1ha2's path for at most 32 bytes: ceil(k / 8) 128-bit products and final64, scheduled by the compiler;
//  * a hit goes to an LDS stage of HG_AA_STAGE entries; the stage is flushed into the proteome's hit region with one atomic
//    reservation per flush, between tiles once it is a quarter full and at the end of the work item.  Hits that find the
//    stage full (every window of a repeat samples the same hash) reserve their slots with one atomic per wave.
// Templated on KW = ceil(k / 8); k itself is a kernel argument: four instantiations.  Plain C++, no inline assembly.
// 12.8 KiB of LDS per workgroup, 48 VGPRs; the kernel is integer-VALU bound like its nucleotide twins.
// The window test and the gather are hg_kmer_window.h's, the hit stage, the sample step and the KW dispatch hg_sample_core.h's
// (shared with tx_kmer_sample_kernel); staging, the residue test, the tile walk and the clean-tile shortcut are this file's.
#include "hg_sample_core.h"

namespace {

constexpr uint32_t WG = HG_AA_WG;

struct AaLds {
  uint32_t img[HG_AA_IMG_WORDS];   // the tile's bytes, bit 5 cleared
  uint32_t inv[HG_AA_INV_WORDS];   // bit i set <=> staged byte i is not a residue
  HgHitStage<HG_AA_STAGE> stage;   // sampled hashes waiting for a flush
};

template <int KW>
__global__ __launch_bounds__(WG) void aa_kmer_sample_kernel(const uint8_t *__restrict__ seq, const hg_genome_meta *__restrict__ meta,
                                                            const uint32_t *__restrict__ item_genome, uint32_t ksize,
                                                            uint32_t item_starts, uint64_t threshold, uint64_t seed,
                                                            uint64_t *__restrict__ hits, uint32_t *__restrict__ cnt) {
  __shared__ AaLds s;
  const uint32_t item = blockIdx.x, tid = threadIdx.x;
  const uint32_t g = item_genome[item];
  const hg_genome_meta gm = meta[g];
  const uint64_t n_res = gm.n_bps;
  if (n_res < ksize) return;  // (workgroup-uniform)
  const uint64_t n_starts = n_res - ksize + 1;
  const uint8_t *__restrict__ gseq = seq + gm.seq_off;
  const uint64_t item_start = (uint64_t)(item - gm.item_first) * item_starts;  // a multiple of 4, like every tile's first start
  const uint64_t item_end = item_start + item_starts < n_starts ? item_start + item_starts : n_starts;
  if (tid == 0) s.stage.n_hits = 0;
  if (tid < 2) s.inv[HG_AA_BYTES / 32 + tid] = 0u;
  const HgWindowParams wn = {ksize, hg_win_mask(ksize), hg_win_tail_mask(ksize, KW), threshold, seed};
  const uint32_t sh8 = 8u * (tid & 3u);  // the lane's byte phase, as a bit shift

  for (uint64_t tile0 = item_start; tile0 < item_end; tile0 += HG_AA_TILE) {
    __syncthreads();  // the previous tile's readers are done, its hits are counted
    if (s.stage.n_hits >= HG_AA_STAGE / 4) flush_stage<WG>(s.stage, gm, g, hits, cnt);  // (workgroup-uniform)
    // ---- stage: the lane's 16 bytes [q, q + 16)
    uint32_t bad16 = 0xFFFFu;
    {
      const uint64_t q = tile0 + 16ull * tid;
      uint32_t v[4] = {0u, 0u, 0u, 0u};
      if (q < n_res) {
        const u32x4_a4 x = *reinterpret_cast<const u32x4_a4 *>(gseq + q);  // ends at most 15 bytes behind the proteome
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
        bad16 = 0u;
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t)
#pragma unroll
          for (uint32_t b = 0; b < 4; ++b)
            if (!hg_aa_is_residue((v[t] >> (8u * b)) & 0xFFu)) bad16 |= 1u << (4u * t + b);
        const uint64_t left = n_res - q;  // > 0: bytes of the proteome from q on
        if (left < 16) bad16 |= 0xFFFFu & ~((1u << (uint32_t)left) - 1u);
      }
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t) s.img[4 * tid + t] = v[t] & 0xDFDFDFDFu;
      reinterpret_cast<uint16_t *>(s.inv)[tid] = (uint16_t)bad16;
    }
    const bool dirty = __syncthreads_or(bad16 != 0u) != 0;  // a clean tile (most of them) tests no window
    // ---- the lane's starts p = tid + 256 j inside [tile0, item_end)
    const uint64_t left_starts = item_end - tile0;  // > 0
    const uint32_t lim = left_starts < HG_AA_TILE ? (uint32_t)left_starts : HG_AA_TILE;
    for (uint32_t p = tid; p < lim; p += WG) {
      if (dirty && hg_win_any_bit(s.inv, p, wn.win_mask)) continue;  // a non-residue inside [p, p + k)
      uint64_t w[KW];
      hg_win_gather(s.img + (p >> 2), sh8, KW, wn.tail_mask, w);
      sample_kmer<KW>(s.stage, w, wn, gm, g, hits, cnt);
    }
  }
  flush_stage<WG>(s.stage, gm, g, hits, cnt);
}

}  // namespace

hipError_t hg_aa_launch_kmer_sample(hipStream_t st, const uint8_t *d_seq, const hg_genome_meta *d_meta, const uint32_t *d_item_genome,
                                    uint32_t n_items, uint32_t ksize, uint64_t threshold, uint64_t seed, uint64_t *d_hits, uint32_t *d_cnt) {
  if (n_items == 0) return hipSuccess;
  if (ksize < 1 || ksize > 32) return hipErrorInvalidValue;
  const uint32_t item_starts = hg_kmer_item_starts(ksize);  // the plan's
  HG_LAUNCH_BY_KW(aa_kmer_sample_kernel, ksize, n_items, WG, st, d_seq, d_meta, d_item_genome, ksize, item_starts, threshold, seed,
                  d_hits, d_cnt);
  return hipGetLastError();
}
