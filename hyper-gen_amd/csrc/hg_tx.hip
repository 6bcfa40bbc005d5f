// hg_tx.hip -- the C ABI of include/hypergen_tx.h (libhypergen_tx.so): six-frame translated protein sketches from DNA.
// The library adds one kernel (hg_tx_kernels.hip) and borrows the rest through the companion entry points of hg_companion.h:
// its hook tells the plan that a window spans 3 * ksize bytes and that a start yields two k-mers.  hg_tx_translate_frame is
// the host's reading of the specification, through the functions the kernel's tables are filled from (hg_tx.h).
#include "../../include/hypergen_tx.h"
#include "hg_companion.h"
#include "hg_tx.h"

namespace {

const char *const KERNEL_NAMES[4] = {"tx_kmer_sample_kernel<1>", "tx_kmer_sample_kernel<2>", "tx_kmer_sample_kernel<3>",
                                     "tx_kmer_sample_kernel<4>"};
// a codon per residue, both strands
const hg_companion TX{hg_tx_launch_kmer_sample, hg_tx_kernel_name, 3, 2, "translated k-mers", "genomes"};

}  // namespace

extern "C" const char *hg_tx_kernel_name(uint32_t ksize) { return ksize >= 1 && ksize <= 32 ? KERNEL_NAMES[(ksize + 7) / 8 - 1] : ""; }
extern "C" uint32_t hg_tx_tile_starts(void) { return HG_TX_TILE; }
extern "C" uint32_t hg_tx_item_starts(uint32_t ksize) { return ksize >= 1 && ksize <= 32 ? hg_kmer_item_starts(ksize) : 0u; }

extern "C" hg_status hg_tx_sketch_batch_dev(hg_ctx *c, const uint8_t *d_seq, const uint64_t *offsets, const uint64_t *lens, size_t n,
                                            const hg_sketch_params *p, int16_t *d_hv, int32_t *d_norm2, uint32_t *d_nhash) {
  return hg_companion_sketch_batch_dev(c, TX, d_seq, offsets, lens, n, p, d_hv, d_norm2, d_nhash);
}

extern "C" hg_status hg_tx_sketch_batch(hg_ctx *c, const uint8_t *const *seqs, const size_t *lens, size_t n, const hg_sketch_params *p,
                                        int16_t *hv_out, int32_t *norm2_out, uint32_t *nhash_out) {
  return hg_companion_sketch_batch(c, TX, seqs, lens, n, p, hv_out, norm2_out, nhash_out);
}

extern "C" hg_status hg_tx_hash_sample(hg_ctx *c, const uint8_t *seq, size_t n, uint32_t ksize, uint64_t threshold, uint64_t seed,
                                       uint64_t *out_hashes, size_t cap, size_t *n_out) {
  return hg_companion_hash_sample(c, TX, seq, n, ksize, threshold, seed, out_hashes, cap, n_out);
}

// ---- the plan of a translated batch as numbers (host only), and whether a ctx ever had to regrow one ---------------------------
extern "C" hg_status hg_tx_plan_describe(const uint64_t *offsets, const uint64_t *lens, size_t n, uint32_t ksize, uint64_t scaled,
                                         uint64_t counts[6]) {
  if ((n && (!offsets || !lens)) || !counts || ksize < 1 || ksize > 32 || scaled < 1) return HG_ERR_INVALID;
  hg_batch_tables t;
  const hg_status s = hg_plan_build(nullptr, {nullptr, offsets, lens, nullptr, n, false}, ksize, scaled, nullptr, t,
                                    hg_plan_shape{TX.span_per_k * ksize, TX.per_start});
  if (s != HG_OK) return s;
  uint64_t min_cap = n ? UINT64_MAX : 0;
  for (size_t g = 0; g < n; ++g) min_cap = std::min<uint64_t>(min_cap, t.meta[g].hit_cap);
  counts[0] = t.n_items, counts[1] = t.total_slots, counts[2] = t.max_cap, counts[3] = min_cap, counts[4] = t.max_expect;
  counts[5] = hg_kmer_item_starts(ksize);
  return HG_OK;
}
extern "C" uint64_t hg_tx_plan_regrows(const hg_ctx *c) { return c ? c->n_plan_regrows : 0; }

// ---- one reading frame on the host ----------------------------------------------------------------------------------------
extern "C" hg_status hg_tx_translate_frame(const uint8_t *seq, size_t n, uint32_t frame, uint8_t *out, size_t cap, size_t *n_out) {
  if (!n_out || frame > 5 || (n && !seq)) return HG_ERR_INVALID;
  const uint32_t f = frame % 3;
  const size_t n_res = n >= f ? (n - f) / 3 : 0;
  *n_out = n_res;
  if (n_res > cap) return HG_ERR_CAPACITY;
  if (n_res && !out) return HG_ERR_INVALID;
  for (size_t j = 0; j < n_res; ++j) {
    // the codon's first base on the forward strand, or its LAST one: residue j of frame 3 + f reads s[n - 1 - f - 3j] downwards
    const size_t q = frame < 3 ? f + 3 * j : n - 3 - f - 3 * j;
    const uint32_t c0 = hg_tx_base_code(seq[q]), c1 = hg_tx_base_code(seq[q + 1]), c2 = hg_tx_base_code(seq[q + 2]);
    if ((c0 | c1 | c2) & HG_TX_NOT_A_BASE) {
      out[j] = HG_TX_X;
      continue;
    }
    const uint32_t i = 16u * c0 + 4u * c1 + c2;
    out[j] = frame < 3 ? hg_tx_table_fwd(i) : hg_tx_table_rev(i);
  }
  return HG_OK;
}
