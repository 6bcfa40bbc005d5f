// hg_companion.h -- the entry points a companion library builds around its hash + sample kernel (not installed; shared by
// libhypergen_aa.so and libhypergen_tx.so, compiled into each).  A companion adds one kernel and borrows the rest: every entry
// point sets the ctx's hash + sample hook (hg_ctx::kmer_hook, read by hg_sketch_front), runs the nucleotide library's
// synchronous sketch path -- plan, hit regions, overflow-and-regrow, sort / unique, encoders, norm -- and clears the hook
// again.  Never the deferred step: its re-run would come from a later call that knows nothing of the hook.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "hg_sketch.h"

// one companion kernel family: its launcher, what the plan must know of it, and how its messages name things
struct hg_companion {
  hg_kmer_hook launch;
  const char *(*kernel_name)(uint32_t ksize);
  uint32_t span_per_k;  // bytes of a k-mer window per unit of ksize (the window spans span_per_k * ksize bytes)
  uint32_t per_start;   // k-mers one start yields
  const char *what;     // "amino-acid k-mers"
  const char *units;    // "proteomes"
};

// the hook while an entry point of a companion runs the synchronous path
struct hg_companion_hook {
  hg_ctx *c;
  hg_companion_hook(hg_ctx *ctx, const hg_companion &k, uint32_t ksize) : c(ctx) {
    c->kmer_hook = k.launch, c->kmer_hook_name = k.kernel_name(ksize);
    c->kmer_hook_span = k.span_per_k == 1 ? 0 : k.span_per_k * ksize, c->kmer_hook_per_start = k.per_start;
  }
  ~hg_companion_hook() { c->kmer_hook = nullptr, c->kmer_hook_name = nullptr, c->kmer_hook_span = 0, c->kmer_hook_per_start = 1; }
};

inline hg_status hg_companion_check_params(hg_ctx *c, const hg_companion &k, const hg_sketch_params *p) {
  const hg_status s = hg_check_sketch_params(c, p);
  if (s != HG_OK) return s;
  const std::string what = k.what;
  if (p->ksize > 32) return hg_fail(c, HG_ERR_UNSUPPORTED, what + ": ksize must be <= 32");
  if (p->min_count > 1) return hg_fail(c, HG_ERR_UNSUPPORTED, what + ": min_count above 1 is not supported");
  if (p->norm_mode != HG_NORM_ACGT) return hg_fail(c, HG_ERR_INVALID, what + ": norm_mode must be 0");
  return HG_OK;
}

inline hg_status hg_companion_sketch_batch_dev(hg_ctx *c, const hg_companion &k, const uint8_t *d_seq, const uint64_t *offsets,
                                               const uint64_t *lens, size_t n, const hg_sketch_params *p, int16_t *d_hv,
                                               int32_t *d_norm2, uint32_t *d_nhash) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_companion_check_params(c, k, p);
  if (s != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!d_seq || !offsets || !lens || !d_hv || !d_norm2 || !d_nhash) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (n > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, std::string("more than 2^31 ") + k.units + " in one batch");
  HG_ENTER(c);  // (a deferred nucleotide step of the ctx is resolved here, with no hook set)
  hg_sketch_params q = *p;
  q.canonical = 0, q.min_count = 1;
  const hg_genome_batch b{d_seq, offsets, lens, nullptr, n, false};
  const hg_companion_hook hook(c, k, q.ksize);
  return hg_sketch_batch_sync(c, b, &q, hg_sketch_out{d_hv, d_norm2, d_nhash});
}

inline hg_status hg_companion_sketch_batch(hg_ctx *c, const hg_companion &k, const uint8_t *const *seqs, const size_t *lens, size_t n,
                                           const hg_sketch_params *p, int16_t *hv_out, int32_t *norm2_out, uint32_t *nhash_out) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_companion_check_params(c, k, p);
  if (s != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!seqs || !lens || !hv_out || !norm2_out || !nhash_out) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (n > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, std::string("more than 2^31 ") + k.units + " in one batch");
  HG_ENTER(c);
  // device layout: every sequence at a multiple of 64 with at least 32 bytes behind it
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
  if ((s = hg_companion_sketch_batch_dev(c, k, d_seq, offs.data(), l64.data(), n, p, d_hv, d_n2, d_nh)) != HG_OK) return s;
  HG_HIP(c, hipMemcpyAsync(hv_out, d_hv, hv_bytes, hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(norm2_out, d_n2, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(nhash_out, d_nh, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

inline hg_status hg_companion_hash_sample(hg_ctx *c, const hg_companion &k, const uint8_t *seq, size_t n, uint32_t ksize,
                                          uint64_t threshold, uint64_t seed, uint64_t *out_hashes, size_t cap, size_t *n_out) {
  if (!c) return HG_ERR_INVALID;
  if (!n_out) return hg_fail(c, HG_ERR_INVALID, "n_out == NULL");
  *n_out = 0;
  if (ksize < 1) return hg_fail(c, HG_ERR_INVALID, "ksize must be >= 1");
  if (ksize > 32) return hg_fail(c, HG_ERR_UNSUPPORTED, std::string(k.what) + ": ksize must be <= 32");
  if (n && !seq) return hg_fail(c, HG_ERR_INVALID, "NULL sequence");
  if (n < (size_t)k.span_per_k * ksize) return HG_OK;
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
    const hg_companion_hook hook(c, k, ksize);
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
