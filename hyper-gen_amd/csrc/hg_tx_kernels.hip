// hg_tx_kernels.hip -- six-frame translated k-mer hash + FracMinHash sample on gfx950 (libhypergen_tx.so).
//
// For every nucleotide start p of a genome the 3k bases [p, p + 3k) are translated twice by the standard genetic code -- as
// they stand, and as their reverse complement -- and each string of k residues (1 <= k <= 32) that holds no stop and no codon
// with a byte other than ACGT in it is hashed with t1ha2_atonce(seed); hashes below the threshold are kept.  Over all starts
// these are the amino-acid k-mers of the six reading frames (include/hypergen_tx.h is the specification), hashed as
// aa_kmer_sample_kernel hashes the same residues of a protein.  The kernel reads the tables of the nucleotide library's plan
// -- hg_genome_meta, work item -> genome, hg_kmer_item_starts(k) starts per work item -- and fills the same hit regions and
// raw counters; the plan is built for windows of 3k bytes and two k-mers per start (hg_plan_shape).
//
//  * one work item per workgroup of 256 lanes; the item is walked in tiles of HG_TX_TILE = 4 000 starts;
//  * a tile is staged in two steps.  First every lane loads 16 bytes (one global_load_dwordx4) and writes 16 code bytes to LDS:
//    bits 0..1 the base (hg_tx_base_code), bit 2 "not a base"; bytes behind the genome's end are not bases.  Loads start inside
//    the genome and so end at most 15 bytes behind it (the caller leaves 32).  Then lane c < 171 takes the 24 codon starts
//    [24c, 24c + 24): for each it reads the residue of the three bases from two 64-byte LDS tables -- forward, and on the other
//    strand -- filled once from hg_tx_table_fwd / hg_tx_table_rev ('X' when one of the three is not a base).  The residues go
//    to six byte images, de-interleaved by start mod 3: image r holds the forward residue of start 3j + r at byte j, image
//    3 + r the reverse-strand residue of the same start at byte 1 367 - j.  So both k-mers of a start are k ascending bytes of
//    one image: the forward one from byte j of image r, the reverse one from byte 1 368 - k - j of image 3 + r.  A lane's 8
//    residues per image are two dword stores, their 8 not-a-residue bits ('*', 'X') one byte of the image's bit image;
//  * the starts of a tile are walked phase by phase, lane t taking j = t, t + 256, ... of each.  Each of the two windows of a
//    start tests its k bits of the bit image (one funnel shift; never skipped: one codon in 21 is a stop), reads the dwords
//    that hold its k bytes, shifts them into ceil(k / 8) little-endian words, masks the last and runs t1ha2's path for at most
//    32 bytes (hg_aa_t1ha2::hash_words);
//  * a hit goes to an LDS stage of HG_TX_STAGE entries; the stage is flushed into the genome's hit region with one atomic
//    reservation per flush, between tiles once it is a quarter full and at the end of the work item.  Hits that find the
//    stage full reserve their slots with one atomic per wave.
// Templated on KW = ceil(k / 8); k itself is a kernel argument: four instantiations.  Plain C++, no inline assembly.
// 21 992 bytes of LDS per workgroup (4.0 KiB codes, 8.3 images, 1.1 bit images, 0.1 tables, 8.0 hit stage) and 80 VGPRs
// (78 for KW = 4), no scratch: six workgroups per CU by registers, seven by LDS.  Integer-VALU bound like
// its twins: two hashes per byte.
// The window test and the gather are hg_kmer_window.h's, the hit stage, the sample step and the KW dispatch hg_sample_core.h's
// (shared with aa_kmer_sample_kernel); the two staging steps and the walk over the phase images are this file's.
#include "hg_sample_core.h"
#include "hg_tx.h"

namespace {

constexpr uint32_t WG = HG_TX_WG;
constexpr uint32_t CODE_WORDS = HG_TX_BYTES / 4 + 4;       // the code image, 16 bytes of "not a base" behind it
constexpr uint32_t IMG_WORDS = HG_TX_IMG_WORDS, INV_WORDS = HG_TX_INV_WORDS;
static_assert(6 * (HG_TX_CHUNKS - 1) + 7 <= CODE_WORDS, "a chunk reads 26 code bytes as 7 dwords");

struct TxLds {
  uint32_t codes[CODE_WORDS];     // per staged byte: base code | 4 * (not a base)
  uint32_t img[6][IMG_WORDS];     // residues: [r] forward, [3 + r] reverse strand (descending), r = start mod 3
  uint32_t inv[6][INV_WORDS];     // bit i set <=> byte i of the image is not a residue
  uint8_t tab[2][64];             // hg_tx_table_fwd, hg_tx_table_rev
  HgHitStage<HG_TX_STAGE> stage;  // sampled hashes waiting for a flush
};

// the k-mer of the k bytes from byte a of one phase image: tested (a stop or an 'X' inside [a, a + k)?), hashed, sampled
template <int KW>
__device__ __forceinline__ void sample_window(TxLds &s, const uint32_t *__restrict__ img, const uint32_t *__restrict__ inv, uint32_t a,
                                              const HgWindowParams &wn, const hg_genome_meta &gm, uint32_t g,
                                              uint64_t *__restrict__ hits, uint32_t *__restrict__ cnt) {
  if (hg_win_any_bit(inv, a, wn.win_mask)) return;
  uint64_t w[KW];
  hg_win_gather(img + (a >> 2), 8u * (a & 3u), KW, wn.tail_mask, w);
  sample_kmer<KW>(s.stage, w, wn, gm, g, hits, cnt);
}

template <int KW>
__global__ __launch_bounds__(WG) void tx_kmer_sample_kernel(const uint8_t *__restrict__ seq, const hg_genome_meta *__restrict__ meta,
                                                            const uint32_t *__restrict__ item_genome, uint32_t ksize,
                                                            uint32_t item_starts, uint64_t threshold, uint64_t seed,
                                                            uint64_t *__restrict__ hits, uint32_t *__restrict__ cnt) {
  __shared__ TxLds s;
  const uint32_t item = blockIdx.x, tid = threadIdx.x;
  const uint32_t g = item_genome[item];
  const hg_genome_meta gm = meta[g];
  const uint64_t n_bps = gm.n_bps;
  const uint32_t span = 3u * ksize;
  if (n_bps < span) return;  // (workgroup-uniform)
  const uint64_t n_starts = n_bps - span + 1;
  const uint8_t *__restrict__ gseq = seq + gm.seq_off;
  const uint64_t item_start = (uint64_t)(item - gm.item_first) * item_starts;  // a multiple of 4, like every tile's first start
  const uint64_t item_end = item_start + item_starts < n_starts ? item_start + item_starts : n_starts;
  if (tid == 0) s.stage.n_hits = 0;
  if (tid < 4) s.codes[HG_TX_BYTES / 4 + tid] = 0x04040404u;  // behind the staged bytes: not bases
  if (tid < 64) s.tab[0][tid] = hg_tx_table_fwd(tid), s.tab[1][tid] = hg_tx_table_rev(tid);
  for (uint32_t i = tid; i < 6 * INV_WORDS; i += WG) (&s.inv[0][0])[i] = 0u;
  // the words behind an image's residues: a window near the top reads them (and shifts or masks them away); staging never writes them
  if (tid < 6 * (IMG_WORDS - HG_TX_PHASE_LEN / 4)) s.img[tid / (IMG_WORDS - HG_TX_PHASE_LEN / 4)][HG_TX_PHASE_LEN / 4 + tid % (IMG_WORDS - HG_TX_PHASE_LEN / 4)] = 0u;
  const HgWindowParams wn = {ksize, hg_win_mask(ksize), hg_win_tail_mask(ksize, KW), threshold, seed};
  const uint32_t rev_top = HG_TX_PHASE_LEN - ksize;           // first byte of the reverse window of j = 0

  for (uint64_t tile0 = item_start; tile0 < item_end; tile0 += HG_TX_TILE) {
    __syncthreads();  // the previous tile's readers are done, its hits are counted (first tile: the tables are written)
    if (s.stage.n_hits >= HG_TX_STAGE / 4) flush_stage<WG>(s.stage, gm, g, hits, cnt);  // (workgroup-uniform)
    // ---- stage 1: the lane's 16 bytes [q, q + 16) as codes
    {
      const uint64_t q = tile0 + 16ull * tid;
      uint32_t code[4] = {0x04040404u, 0x04040404u, 0x04040404u, 0x04040404u};
      if (q < n_bps) {
        const u32x4_a4 x = *reinterpret_cast<const u32x4_a4 *>(gseq + q);  // ends at most 15 bytes behind the genome
        const uint32_t v[4] = {x.x, x.y, x.z, x.w};
        const uint64_t left = n_bps - q;  // > 0: bytes of the genome from q on
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
          uint32_t cw = 0;
#pragma unroll
          for (uint32_t b = 0; b < 4; ++b) {
            const uint32_t cb = 4u * t + b < left ? hg_tx_base_code((v[t] >> (8u * b)) & 0xFFu) : HG_TX_NOT_A_BASE;
            cw |= cb << (8u * b);
          }
          code[t] = cw;
        }
      }
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t) s.codes[4 * tid + t] = code[t];
    }
    __syncthreads();
    // ---- stage 2: the lane's 24 codon starts, 8 of each phase, on both strands
    if (tid < HG_TX_CHUNKS) {
      uint32_t cd[7];
#pragma unroll
      for (uint32_t t = 0; t < 7; ++t) cd[t] = s.codes[6 * tid + t];
      uint32_t fw[3][2] = {{0u, 0u}, {0u, 0u}, {0u, 0u}}, rv[3][2] = {{0u, 0u}, {0u, 0u}, {0u, 0u}};
      uint32_t fbad[3] = {0u, 0u, 0u}, rbad[3] = {0u, 0u, 0u};
#pragma unroll
      for (uint32_t i = 0; i < HG_TX_CHUNK; ++i) {
        const uint32_t b0 = (cd[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
        const uint32_t b1 = (cd[(i + 1) >> 2] >> (8u * ((i + 1) & 3u))) & 0xFFu;
        const uint32_t b2 = (cd[(i + 2) >> 2] >> (8u * ((i + 2) & 3u))) & 0xFFu;
        const bool x = ((b0 | b1 | b2) & HG_TX_NOT_A_BASE) != 0u;
        const uint32_t idx = ((b0 & 3u) << 4) | ((b1 & 3u) << 2) | (b2 & 3u);
        const uint32_t f = x ? HG_TX_X : s.tab[0][idx], r = x ? HG_TX_X : s.tab[1][idx];
        const uint32_t ph = i % 3u, jj = i / 3u, rj = 7u - jj;  // the reverse images run downwards
        fw[ph][jj >> 2] |= f << (8u * (jj & 3u));
        rv[ph][rj >> 2] |= r << (8u * (rj & 3u));
        fbad[ph] |= (uint32_t)(x || f == HG_TX_STOP) << jj;
        rbad[ph] |= (uint32_t)(x || r == HG_TX_STOP) << rj;
      }
      const uint32_t rc = HG_TX_CHUNKS - 1u - tid;  // the lane's place in the reverse images
#pragma unroll
      for (uint32_t ph = 0; ph < 3; ++ph) {
        s.img[ph][2 * tid] = fw[ph][0], s.img[ph][2 * tid + 1] = fw[ph][1];
        s.img[3 + ph][2 * rc] = rv[ph][0], s.img[3 + ph][2 * rc + 1] = rv[ph][1];
        reinterpret_cast<uint8_t *>(s.inv[ph])[tid] = (uint8_t)fbad[ph];
        reinterpret_cast<uint8_t *>(s.inv[3 + ph])[rc] = (uint8_t)rbad[ph];
      }
    }
    __syncthreads();
    // ---- the tile's starts p = 3j + r inside [tile0, item_end): phase r, lane tid takes j = tid + 256 i
    const uint64_t left_starts = item_end - tile0;  // > 0
    const uint32_t lim = left_starts < HG_TX_TILE ? (uint32_t)left_starts : HG_TX_TILE;
#pragma unroll 1
    for (uint32_t r = 0; r < 3; ++r) {
      const uint32_t nj = (lim + 2u - r) / 3u;  // starts of phase r below lim
      for (uint32_t j = tid; j < nj; j += WG) {
        sample_window<KW>(s, s.img[r], s.inv[r], j, wn, gm, g, hits, cnt);
        sample_window<KW>(s, s.img[3 + r], s.inv[3 + r], rev_top - j, wn, gm, g, hits, cnt);
      }
    }
  }
  flush_stage<WG>(s.stage, gm, g, hits, cnt);
}

}  // namespace

hipError_t hg_tx_launch_kmer_sample(hipStream_t st, const uint8_t *d_seq, const hg_genome_meta *d_meta, const uint32_t *d_item_genome,
                                    uint32_t n_items, uint32_t ksize, uint64_t threshold, uint64_t seed, uint64_t *d_hits, uint32_t *d_cnt) {
  if (n_items == 0) return hipSuccess;
  if (ksize < 1 || ksize > 32) return hipErrorInvalidValue;
  const uint32_t item_starts = hg_kmer_item_starts(ksize);  // the plan's
  HG_LAUNCH_BY_KW(tx_kmer_sample_kernel, ksize, n_items, WG, st, d_seq, d_meta, d_item_genome, ksize, item_starts, threshold, seed,
                  d_hits, d_cnt);
  return hipGetLastError();
}
