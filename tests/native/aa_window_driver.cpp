// AddressSanitizer + UBSan driver (CPU build) for the window arithmetic aa_kmer_sample_kernel and tx_kmer_sample_kernel
// share (hyper-gen_amd/csrc/hg_kmer_window.h, compiled here without HIP): the test of a window's bits in a bit image and the
// gather of its bytes from a dword image, for every k in 1..32 at every start byte 0..71 -- all four byte phases, all 32 bit
// phases, across a word of the bit image -- against byte-wise and bit-wise references; and the read extent of the largest
// start either kernel issues, with the images in heap blocks of exactly the size of the kernels' LDS members, so that a read
// behind the documented slack is an AddressSanitizer error.  The hash is not checked here (the GPU tests do, against the oracle).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

#include "../../hyper-gen_amd/csrc/hg_kmer_window.h"

#define CHECK(cond)                                                                                              \
  if (!(cond)) {                                                                                                 \
    std::printf("%s:%d: %s, k %u, start %u: %s\n", __FILE__, __LINE__, g_case, g_k, g_a, #cond), std::exit(1);   \
  }

namespace {

const char *g_case = "";
uint32_t g_k = 0, g_a = 0;

// a heap block of exactly `words` dwords (no vector: its capacity may exceed its size)
struct Words {
  size_t n;
  std::unique_ptr<uint32_t[]> own;
  uint32_t *p;
  explicit Words(size_t words) : n(words), own(new uint32_t[words]()), p(own.get()) {}
  void randomize(std::mt19937_64 &rng) {
    for (size_t i = 0; i < n; ++i) p[i] = (uint32_t)rng();
  }
  uint8_t byte(size_t i) const { return (uint8_t)(p[i / 4] >> (8 * (i % 4))); }  // little-endian, as the kernels store
  bool bit(size_t i) const { return (p[i / 32] >> (i % 32)) & 1u; }
};

// the gather of the k bytes from byte a of img against their byte-wise copy
void check_gather(const Words &img, uint32_t a, uint32_t k) {
  g_a = a, g_k = k;
  const int kw = (int)(k + 7) / 8;
  uint64_t got[4] = {0, 0, 0, 0};
  hg_win_gather(img.p + (a >> 2), 8u * (a & 3u), kw, hg_win_tail_mask(k, kw), got);
  uint64_t want[4] = {0, 0, 0, 0};  // the k bytes, zero-padded, as little-endian words
  for (uint32_t i = 0; i < k; ++i) want[i / 8] |= (uint64_t)img.byte(a + i) << (8 * (i % 8));
  CHECK(std::memcmp(got, want, sizeof want) == 0);
}

// the window test of bits [a, a + k) of inv against the bits one by one
void check_test(const Words &inv, uint32_t a, uint32_t k) {
  g_a = a, g_k = k;
  bool want = false;
  for (uint32_t i = 0; i < k; ++i) want = want || inv.bit(a + i);
  CHECK(hg_win_any_bit(inv.p, a, hg_win_mask(k)) == want);
}

// one largest start of a kernel: both images as large as the kernel's LDS members, random content
void check_extent(const char *name, size_t img_words, size_t inv_words, uint32_t a, uint32_t k, std::mt19937_64 &rng) {
  g_case = name;
  Words img(img_words), inv(inv_words);
  img.randomize(rng), inv.randomize(rng);
  check_gather(img, a, k);
  check_test(inv, a, k);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240607);
  constexpr uint32_t MAX_A = 71, MAX_K = 32;
  // blocks that end with the last dword a window may read: d[2 kw] of the gather, the second word of the test
  Words img((MAX_A >> 2) + 2 * ((MAX_K + 7) / 8) + 1), inv((MAX_A >> 5) + 2);
  size_t n = 0;
  for (int round = 0; round < 4; ++round) {
    img.randomize(rng);
    for (uint32_t k = 1; k <= MAX_K; ++k)
      for (uint32_t a = 0; a <= MAX_A; ++a) {
        g_case = "gather";
        check_gather(img, a, k);
        g_case = "test, random bits";
        inv.randomize(rng);
        check_test(inv, a, k);
        if (round) continue;
        g_case = "test, no bit";
        std::memset(inv.p, 0, inv.n * 4);
        CHECK(!hg_win_any_bit(inv.p, a, hg_win_mask(k)));
        g_case = "test, one bit";
        for (uint32_t b = a ? a - 1 : 0; b <= a + k; ++b) {  // from the bit before the window to the bit behind it
          std::memset(inv.p, 0, inv.n * 4);
          inv.p[b / 32] = 1u << (b % 32);
          CHECK(hg_win_any_bit(inv.p, a, hg_win_mask(k)) == (b >= a && b < a + k));
          ++n;
        }
      }
  }
  // the largest starts the kernels issue (hg_aa_kernels.hip, hg_tx_kernels.hip), at the smallest and the largest k
  const uint32_t tx_last_fwd = (HG_TX_TILE + 2) / 3 - 1;  // the last start of phase 0 in a full tile
  for (uint32_t k : {1u, MAX_K}) {
    check_extent("aa, last start of a tile", HG_AA_IMG_WORDS, HG_AA_INV_WORDS, HG_AA_TILE - 1, k, rng);
    check_extent("tx, last forward start", HG_TX_IMG_WORDS, HG_TX_INV_WORDS, tx_last_fwd, k, rng);
    check_extent("tx, first reverse window", HG_TX_IMG_WORDS, HG_TX_INV_WORDS, HG_TX_PHASE_LEN - k, k, rng);
  }
  std::printf("aa window driver ok (%zu single-bit cases)\n", n);
  return 0;
}
