// hg_kmer_window.h -- the HIP-free part of what aa_kmer_sample_kernel and tx_kmer_sample_kernel share (not installed): the two
// kernels' tile geometry and the integer arithmetic of one window -- its masks, the test of its bits in a bit image and the
// gather of its bytes from a dword image -- as plain C++ for host and device.  g++ compiles this file without HIP, so a CPU
// program (tests/native/aa_window_driver.cpp) checks the very functions the kernels run, and their read extents against the
// sizes of the LDS images below.  The device-only rest (hit stage, sample step, launch) is hg_sample_core.h.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HG_WIN_HD __host__ __device__ __forceinline__
#else
#define HG_WIN_HD inline
#endif

// ---- geometry: amino-acid kernel (hg_aa_kernels.hip) ----------------------------------------------------------------------
constexpr uint32_t HG_AA_WG = 256;                        // lanes per workgroup
constexpr uint32_t HG_AA_BYTES = 16 * HG_AA_WG;           // staged bytes per tile: 16 per lane, one wide load
constexpr uint32_t HG_AA_TILE = HG_AA_BYTES - 64;         // k-mer starts per tile: the last start reads up to 40 bytes
constexpr uint32_t HG_AA_STAGE = 1024;                    // entries of the LDS hit stage
constexpr uint32_t HG_AA_IMG_WORDS = HG_AA_BYTES / 4;     // the byte image
constexpr uint32_t HG_AA_INV_WORDS = HG_AA_BYTES / 32 + 2;  // the bit image, two zero words of slack behind it
static_assert(HG_AA_TILE % 4 == 0 && HG_AA_TILE + 40 <= HG_AA_BYTES, "amino-acid tile geometry");

// ---- geometry: six-frame translated kernel (hg_tx_kernels.hip) -------------------------------------------------------------
constexpr uint32_t HG_TX_WG = 256;                   // lanes per workgroup
constexpr uint32_t HG_TX_BYTES = 16 * HG_TX_WG;      // staged nucleotides per tile: 16 per lane, one wide load
constexpr uint32_t HG_TX_TILE = HG_TX_BYTES - 96;    // nucleotide starts per tile: the last start's window spans 3 * 32 bytes
constexpr uint32_t HG_TX_STAGE = 1024;               // entries of the LDS hit stage
constexpr uint32_t HG_TX_CHUNK = 24;                 // codon starts one lane translates: 8 residues of each of the 3 phases
constexpr uint32_t HG_TX_CHUNKS = (HG_TX_BYTES + HG_TX_CHUNK - 1) / HG_TX_CHUNK;  // 171
constexpr uint32_t HG_TX_PHASE_LEN = 8 * HG_TX_CHUNKS;                            // residues of one phase image: 1 368
constexpr uint32_t HG_TX_IMG_WORDS = HG_TX_PHASE_LEN / 4 + 10;   // one phase image; a window's dword reads end at most 9 words behind its first
constexpr uint32_t HG_TX_INV_WORDS = HG_TX_PHASE_LEN / 32 + 4;   // one bit image; a window reads two words
static_assert(HG_TX_TILE % 4 == 0 && HG_TX_TILE + 96 <= HG_TX_BYTES, "translated tile geometry");
static_assert(HG_TX_CHUNKS <= HG_TX_WG, "one chunk per lane");

// ---- one window of k bytes, 1 <= k <= 32, KW = ceil(k / 8) -----------------------------------------------------------------
// the k bits of a window in a bit image, shifted down to bit 0
HG_WIN_HD uint32_t hg_win_mask(uint32_t ksize) { return ksize >= 32 ? ~0u : (1u << ksize) - 1u; }
// the bytes of the k-mer's last word (1..8) as a mask of that word
HG_WIN_HD uint64_t hg_win_tail_mask(uint32_t ksize, int kw) {
  const uint32_t tail_bytes = ksize - 8u * (uint32_t)(kw - 1);
  return tail_bytes >= 8 ? ~0ull : (1ull << (8u * tail_bytes)) - 1ull;
}

// whether a bit of [a, a + k) is set in the bit image: two words (a / 32 and the next, read whatever k is), one funnel shift
HG_WIN_HD bool hg_win_any_bit(const uint32_t *inv, uint32_t a, uint32_t win_mask) {
  const uint32_t dw = a >> 5, sh = a & 31u;
  const uint64_t two = (uint64_t)inv[dw] | ((uint64_t)inv[dw + 1] << 32);
  return ((uint32_t)(two >> sh) & win_mask) != 0u;
}

// The k bytes that start sh8 = 8 * (a mod 4) bits into d[0], d = image + a / 4, as the kw = ceil(k / 8) little-endian words
// w[0 .. kw), the bytes of the last word behind the k-mer zero.  Reads d[0 .. 2 kw] whatever k is.  sh8 is a parameter because
// the amino-acid kernel's lanes keep theirs for a whole launch.  kw is an argument and the loop has no unroll pragma on
// purpose: a kernel template passes its constant KW, and the compiler unrolls the loop where it meets that constant -- in the
// kernel for aa, in sample_window for tx -- which is what leaves both kernels' generated code as it was with the loop
// written out in place.
HG_WIN_HD void hg_win_gather(const uint32_t *d, uint32_t sh8, int kw, uint64_t tail_mask, uint64_t *w) {
  uint32_t lo = d[0];
  for (int i = 0; i < kw; ++i) {
    const uint32_t mid = d[2 * i + 1], hi = d[2 * i + 2];
    const uint32_t w_lo = (uint32_t)(((uint64_t)lo | ((uint64_t)mid << 32)) >> sh8);
    const uint32_t w_hi = (uint32_t)(((uint64_t)mid | ((uint64_t)hi << 32)) >> sh8);
    w[i] = (uint64_t)w_lo | ((uint64_t)w_hi << 32);
    lo = hi;
  }
  w[kw - 1] &= tail_mask;
}
