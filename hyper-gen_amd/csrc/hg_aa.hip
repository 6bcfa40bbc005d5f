// hg_aa.hip -- the C ABI of include/hypergen_aa.h (libhypergen_aa.so): amino-acid k-mer sketches.
// The library adds one kernel (hg_aa_kernels.hip) and borrows the rest through the companion entry points of hg_companion.h;
// the protein FASTA reader is its own.
#include <zlib.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/hypergen_aa.h"
#include "hg_aa.h"
#include "hg_companion.h"

namespace {

const char *const KERNEL_NAMES[4] = {"aa_kmer_sample_kernel<1>", "aa_kmer_sample_kernel<2>", "aa_kmer_sample_kernel<3>",
                                     "aa_kmer_sample_kernel<4>"};
// a window of k bytes, one k-mer per start: the plan is the nucleotide one
const hg_companion AA{hg_aa_launch_kmer_sample, hg_aa_kernel_name, 1, 1, "amino-acid k-mers", "proteomes"};

}  // namespace

extern "C" const char *hg_aa_kernel_name(uint32_t ksize) { return ksize >= 1 && ksize <= 32 ? KERNEL_NAMES[(ksize + 7) / 8 - 1] : ""; }
extern "C" uint32_t hg_aa_tile_starts(void) { return HG_AA_TILE; }
extern "C" uint32_t hg_aa_item_starts(uint32_t ksize) { return ksize >= 1 && ksize <= 32 ? hg_kmer_item_starts(ksize) : 0u; }

extern "C" hg_status hg_aa_sketch_batch_dev(hg_ctx *c, const uint8_t *d_seq, const uint64_t *offsets, const uint64_t *lens, size_t n,
                                            const hg_sketch_params *p, int16_t *d_hv, int32_t *d_norm2, uint32_t *d_nhash) {
  return hg_companion_sketch_batch_dev(c, AA, d_seq, offsets, lens, n, p, d_hv, d_norm2, d_nhash);
}

extern "C" hg_status hg_aa_sketch_batch(hg_ctx *c, const uint8_t *const *seqs, const size_t *lens, size_t n, const hg_sketch_params *p,
                                        int16_t *hv_out, int32_t *norm2_out, uint32_t *nhash_out) {
  return hg_companion_sketch_batch(c, AA, seqs, lens, n, p, hv_out, norm2_out, nhash_out);
}

extern "C" hg_status hg_aa_hash_sample(hg_ctx *c, const uint8_t *seq, size_t n, uint32_t ksize, uint64_t threshold, uint64_t seed,
                                       uint64_t *out_hashes, size_t cap, size_t *n_out) {
  return hg_companion_hash_sample(c, AA, seq, n, ksize, threshold, seed, out_hashes, cap, n_out);
}

// ---- protein FASTA -> one proteome (host only) ------------------------------------------------------------------------
extern "C" hg_status hg_aa_read_fasta(const char *path, uint8_t **pbuf, size_t *pcap, size_t *pn) {
  if (!path || !pbuf || !pcap || !pn) return HG_ERR_INVALID;
  *pn = 0;
  gzFile f = gzopen(path, "rb");  // (reads a file that is not gzip as it is)
  if (!f) return HG_ERR_IO;
  (void)gzbuffer(f, 1u << 18);
  uint8_t *buf = *pbuf;
  size_t cap = buf ? *pcap : 0, w = 0;
  std::vector<uint8_t> chunk((size_t)1 << 20);
  bool line_start = true, header = false;
  hg_status st = HG_OK;
  for (;;) {
    const int got = gzread(f, chunk.data(), (unsigned)chunk.size());
    if (got < 0) {
      st = HG_ERR_IO;
      break;
    }
    if (got == 0) break;
    if (w + (size_t)got > cap) {  // (every input byte yields at most one output byte)
      const size_t want = std::max(w + (size_t)got + 64, cap + cap / 2);
      uint8_t *nb = static_cast<uint8_t *>(std::realloc(buf, want));
      if (!nb) {
        st = HG_ERR_OOM;
        break;
      }
      buf = nb, cap = want;
    }
    for (int i = 0; i < got; ++i) {
      const uint8_t ch = chunk[(size_t)i];
      if (header) {
        if (ch == '\n') header = false, line_start = true;
        continue;
      }
      if (ch == '\n') {
        line_start = true;
        continue;
      }
      if (line_start && ch == '>') {  // a record starts: one '*', the rest of the line is its name
        buf[w++] = '*';
        header = true, line_start = false;
        continue;
      }
      line_start = false;
      if (ch == '\r' || ch == ' ' || ch == '\t') continue;
      buf[w++] = ch;
    }
  }
  gzclose(f);
  *pbuf = buf, *pcap = cap;
  if (st != HG_OK) return st;
  *pn = w;
  return HG_OK;
}
