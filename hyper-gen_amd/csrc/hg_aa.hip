// hg_aa.hip -- the C ABI of include/hypergen_aa.h (libhypergen_aa.so): amino-acid k-mer sketches.
// The library adds one kernel (hg_aa_kernels.hip) and borrows the rest: every entry point sets the ctx's hash + sample hook
// (hg_ctx::kmer_hook, read by hg_sketch_front), runs the nucleotide library's synchronous sketch path -- plan, hit regions,
// overflow-and-regrow, sort / unique, encoders, norm -- and clears the hook again.  Never the deferred step: its re-run would
// come from a later call that knows nothing of the hook.
#include <zlib.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/hypergen_aa.h"
#include "hg_aa.h"
#include "hg_sketch.h"

namespace {

const char *const KERNEL_NAMES[4] = {"aa_kmer_sample_kernel<1>", "aa_kmer_sample_kernel<2>", "aa_kmer_sample_kernel<3>",
                                     "aa_kmer_sample_kernel<4>"};

// the hook while an entry point of this library runs the synchronous path
struct AaHook {
  hg_ctx *c;
  AaHook(hg_ctx *ctx, uint32_t ksize) : c(ctx) { c->kmer_hook = hg_aa_launch_kmer_sample, c->kmer_hook_name = hg_aa_kernel_name(ksize); }
  ~AaHook() { c->kmer_hook = nullptr, c->kmer_hook_name = nullptr; }
};

hg_status check_params(hg_ctx *c, const hg_sketch_params *p) {
  const hg_status s = hg_check_sketch_params(c, p);
  if (s != HG_OK) return s;
  if (p->ksize > 32) return hg_fail(c, HG_ERR_UNSUPPORTED, "amino-acid k-mers: ksize must be <= 32");
  if (p->min_count > 1) return hg_fail(c, HG_ERR_UNSUPPORTED, "amino-acid k-mers: min_count above 1 is not supported");
  if (p->norm_mode != HG_NORM_ACGT) return hg_fail(c, HG_ERR_INVALID, "amino-acid k-mers: norm_mode must be 0");
  return HG_OK;
}

}  // namespace

extern "C" const char *hg_aa_kernel_name(uint32_t ksize) { return ksize >= 1 && ksize <= 32 ? KERNEL_NAMES[(ksize + 7) / 8 - 1] : ""; }
extern "C" uint32_t hg_aa_tile_starts(void) { return HG_AA_TILE; }
extern "C" uint32_t hg_aa_item_starts(uint32_t ksize) { return ksize >= 1 && ksize <= 32 ? hg_kmer_item_starts(ksize) : 0u; }

extern "C" hg_status hg_aa_sketch_batch_dev(hg_ctx *c, const uint8_t *d_seq, const uint64_t *offsets, const uint64_t *lens, size_t n,
                                            const hg_sketch_params *p, int16_t *d_hv, int32_t *d_norm2, uint32_t *d_nhash) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_params(c, p);
  if (s != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!d_seq || !offsets || !lens || !d_hv || !d_norm2 || !d_nhash) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (n > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "more than 2^31 proteomes in one batch");
  HG_ENTER(c);  // (a deferred nucleotide step of the ctx is resolved here, with no hook set)
  hg_sketch_params q = *p;
  q.canonical = 0, q.min_count = 1;
  const hg_genome_batch b{d_seq, offsets, lens, nullptr, n, false};
  const AaHook hook(c, q.ksize);
  return hg_sketch_batch_sync(c, b, &q, hg_sketch_out{d_hv, d_norm2, d_nhash});
}

extern "C" hg_status hg_aa_sketch_batch(hg_ctx *c, const uint8_t *const *seqs, const size_t *lens, size_t n, const hg_sketch_params *p,
                                        int16_t *hv_out, int32_t *norm2_out, uint32_t *nhash_out) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_params(c, p);
  if (s != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!seqs || !lens || !hv_out || !norm2_out || !nhash_out) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (n > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "more than 2^31 proteomes in one batch");
  HG_ENTER(c);
  // device layout: every proteome at a multiple of 64 with at least 32 bytes behind it
  std::vector<uint64_t> offs(n), l64(n);
  uint64_t total = 0;
  for (size_t g = 0; g < n; ++g) {
    if (lens[g] && !seqs[g]) return hg_fail(c, HG_ERR_INVALID, "NULL sequence");
    offs[g] = total, l64[g] = lens[g];
    total += ((uint64_t)lens[g] + 32 + 63) & ~(uint64_t)63;
  }
  const size_t hv_bytes = n * (size_t)p->hv_d * sizeof(int16_t);
  if ((s = hg_ensure(c, c->w_seq, total + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_hv, hv_bytes + n * 8 + 64)) != HG_OK) return s;
  auto *d_seq = static_cast<uint8_t *>(c->w_seq.p);
  auto *d_hv = static_cast<int16_t *>(c->w_hv.p);
  auto *d_n2 = reinterpret_cast<int32_t *>(static_cast<uint8_t *>(c->w_hv.p) + ((hv_bytes + 15) & ~(size_t)15));
  auto *d_nh = reinterpret_cast<uint32_t *>(d_n2 + n);
  for (size_t g = 0; g < n; ++g)
    if (lens[g]) HG_HIP(c, hipMemcpyAsync(d_seq + offs[g], seqs[g], lens[g], hipMemcpyHostToDevice, c->stream));
  if ((s = hg_aa_sketch_batch_dev(c, d_seq, offs.data(), l64.data(), n, p, d_hv, d_n2, d_nh)) != HG_OK) return s;
  HG_HIP(c, hipMemcpyAsync(hv_out, d_hv, hv_bytes, hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(norm2_out, d_n2, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(nhash_out, d_nh, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

extern "C" hg_status hg_aa_hash_sample(hg_ctx *c, const uint8_t *seq, size_t n, uint32_t ksize, uint64_t threshold, uint64_t seed,
                                       uint64_t *out_hashes, size_t cap, size_t *n_out) {
  if (!c) return HG_ERR_INVALID;
  if (!n_out) return hg_fail(c, HG_ERR_INVALID, "n_out == NULL");
  *n_out = 0;
  if (ksize < 1) return hg_fail(c, HG_ERR_INVALID, "ksize must be >= 1");
  if (ksize > 32) return hg_fail(c, HG_ERR_UNSUPPORTED, "amino-acid k-mers: ksize must be <= 32");
  if (n && !seq) return hg_fail(c, HG_ERR_INVALID, "NULL sequence");
  if (n < ksize) return HG_OK;
  HG_ENTER(c);
  const std::vector<uint64_t> offs{0}, l64{n};
  hg_status s = hg_ensure(c, c->w_seq, n + 64);
  if (s != HG_OK) return s;
  HG_HIP(c, hipMemcpyAsync(c->w_seq.p, seq, n, hipMemcpyHostToDevice, c->stream));
  // the plan's capacities want "scaled": from the threshold (threshold = MAX / scaled)
  uint64_t scaled = threshold ? UINT64_MAX / threshold : UINT64_MAX;
  if (scaled < 1) scaled = 1;
  const hg_genome_batch b{static_cast<uint8_t *>(c->w_seq.p), offs.data(), l64.data(), nullptr, 1, false};
  const hg_sketch_params p{ksize, 0, scaled, seed, 0, 0, HG_NORM_ACGT, 1};  // (no encode)
  hg_batch_tables pl;
  uint32_t *d_nd = nullptr;
  hg_sample_fetch fetch;
  fetch.max_hashes = out_hashes ? cap : 0;
  {
    const AaHook hook(c, ksize);
    s = hg_sample_batch_sync(c, b, &p, threshold, pl, false, &d_nd, &fetch);
  }
  if (s != HG_OK) return s;
  if (fetch.valid) {  // count and hashes came back with the path's own synchronisation
    *n_out = fetch.nd;
    if (fetch.nd) std::memcpy(out_hashes, fetch.h_hashes, fetch.nd * sizeof(uint64_t));
    return HG_OK;
  }
  uint32_t nd = 0;
  HG_HIP(c, hipMemcpyAsync(&nd, d_nd, sizeof nd, hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  *n_out = nd;
  if (nd > cap) return hg_fail(c, HG_ERR_CAPACITY, "out_hashes too small");
  if (nd) {
    if (!out_hashes) return hg_fail(c, HG_ERR_INVALID, "out_hashes == NULL");
    HG_HIP(c, hipMemcpyAsync(out_hashes, static_cast<uint64_t *>(c->w_hits.p) + pl.meta[0].hit_off, nd * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, c->stream));
    HG_HIP(c, hipStreamSynchronize(c->stream));
  }
  return HG_OK;
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
