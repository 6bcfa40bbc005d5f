// hg_sketch.h -- seams between the translation units of the sketch path (not installed):
//   hg_sketch_plan.hip  batch geometry -> hit regions + work items; the plan kept by the ctx (hg_plan_get), its upload
//   hg_sketch_step.hip  the sync-free step (hash + sample -> sort / unique -> encode queued back to back, one check word
//                       read a call late), hg_sketch_resolve, and hg_sketch_front, the first kernels of both paths
//   hg_sketch_rare.hip  the synchronous path: counters read back, overflow retry, multi-workgroup sorts, split encode
//   hg_api_sketch.hip   the C ABI entry points (device-resident, host-fed, one genome per call)
// A batch travels between them as one hg_genome_batch (hg_internal.h), its outputs as one hg_sketch_out.
#pragma once
#include <utility>

#include "hg_internal.h"

// Host tables of one batch: what the kernels read (uploaded to w_gmeta / w_items) and what the synchronous path learns
// from the raw counters.
struct hg_batch_tables {
  std::vector<hg_genome_meta> meta;   // (a plan taken from the ctx's cache fills hit_cap / hit_off only)
  std::vector<uint32_t> item_genome;  // work item -> genome (empty for a cached plan)
  std::vector<uint32_t> group_first;  // workgroup -> its first work item, n_groups + 1 entries (empty for a cached plan / k > 32)
  size_t n_groups = 0;
  uint64_t total_slots = 0;
  uint32_t max_cap = 0, max_expect = 0;
  size_t n_items = 0;
  bool reused = false;      // taken from the ctx's cached plan (its tables are on the device)
  uint32_t max_hits = ~0u;  // largest stored raw hit count of the batch (upper bound of the distinct counts)
  std::vector<std::pair<uint32_t, uint32_t>> big;  // (genome, stored raw hits) with more than HG_ENC_SLAB hits
};

hg_status hg_check_sketch_params(hg_ctx *c, const hg_sketch_params *p);
// where the group table lies in w_items: behind the n_items item words, 16-byte aligned
inline size_t hg_plan_group_offset(size_t n_items) { return (n_items + 3) & ~(size_t)3; }
inline const uint32_t *hg_plan_group_table(const hg_ctx *c, size_t n_items, size_t n_groups) {
  return n_groups ? static_cast<const uint32_t *>(c->w_items.p) + hg_plan_group_offset(n_items) : nullptr;
}

// What the hash + sample kernel makes of a genome, as far as the plan's sizes go: a k-mer window spans `span` bytes (0: ksize
// of them) and every start yields `per_start` k-mers.  (ksize, 1) for the nucleotide kernels and the amino-acid hook; a hook
// that says otherwise sets hg_ctx::kmer_hook_span / kmer_hook_per_start.  A genome of n bytes then has n - span + 1 starts,
// (n - span + 1) * per_start k-mers -- the bound of its hit region -- and that many / scaled expected hits.
struct hg_plan_shape {
  uint32_t span = 0, per_start = 1;
};
inline hg_plan_shape hg_ctx_plan_shape(const hg_ctx *c) {
  return c->kmer_hook ? hg_plan_shape{c->kmer_hook_span, c->kmer_hook_per_start} : hg_plan_shape{};
}

// want_caps: optional per-genome minimum capacities (retry after overflow); c may be nullptr (hg_sketch_plan_describe)
hg_status hg_plan_build(hg_ctx *c, const hg_genome_batch &b, uint32_t ksize, uint64_t scaled,
                        const std::vector<uint32_t> *want_caps, hg_batch_tables &t, hg_plan_shape shape = {});
// The batch's plan: the ctx's cached one when the geometry matches (t.reused; with_meta = false: the totals only -- the
// sync-free step reads no per-genome record on the host, 400 000 genomes are 16 MB of them), else built afresh.
// The shape is part of the geometry: a plan cached for another shape does not match.
hg_status hg_plan_get(hg_ctx *c, const hg_genome_batch &b, uint32_t ksize, uint64_t scaled, hg_batch_tables &t, bool with_meta = true,
                      hg_plan_shape shape = {});
// the cached plan's capacities and hit offsets into t.meta (a reused plan's records, for the synchronous path)
void hg_plan_tables_from_cache(const hg_sketch_plan &pl, size_t n, hg_batch_tables &t, bool with_meta = true);
// A freshly built plan (not t.reused) goes to w_gmeta / w_items through the page-locked plan staging (stream-ordered,
// returns at once) and becomes the ctx's cached plan.
hg_status hg_plan_commit(hg_ctx *c, const hg_batch_tables &t, const hg_genome_batch &b, uint32_t ksize, uint64_t scaled,
                         hg_plan_shape shape = {});

// ASCII genomes -> hg_pack2 blobs on the device (synchronises the stream before and after: it uses the ctx's scratch)
hg_status hg_pack_batch(hg_ctx *c, const uint8_t *d_seq, const uint64_t *seq_offs, const uint64_t *lens, size_t n,
                        uint32_t norm_mode, uint8_t *d_blobs, const uint64_t *blob_offs);

// One-genome callers that want the sorted hash list on the host (hg_kmer_hash_sample): the distinct count and the first
// max_hashes hashes ride back with the counter copy the synchronous path waits for anyway -- one synchronisation per call
// instead of three.  valid is set when the list the LDS sort produced is final (no overflow, no second sort pass).
struct hg_sample_fetch {
  size_t max_hashes = 0;
  const uint64_t *h_hashes = nullptr;  // in the ctx's page-locked scratch: consume before the next call on the ctx
  uint32_t nd = 0;
  bool valid = false;
};

// Both paths start here: counters zeroed, k-mer launch, first sort / unique launch (its size in *sort_cap).  sync_free: the
// sort flags what it cannot take in the step's flag word (zeroed with the counters), and the capacity-sized second sort
// launch follows; else the synchronous path reads the counters back.
hg_status hg_sketch_front(hg_ctx *c, const hg_genome_batch &b, const hg_sketch_params *p, uint64_t threshold,
                          const hg_batch_tables &t, bool sync_free, uint32_t *sort_cap);

// The synchronous path.  Runs hash + sample and sort / unique; on return (stream synchronised) the device hit buffer holds
// each genome's ascending distinct hashes at t.meta[g].hit_off and *d_ndistinct_out the counts.  planned: t already holds
// the batch's plan with its records (hg_plan_get); else it is looked up here.  p->scaled sizes the plan; threshold samples.
hg_status hg_sample_batch_sync(hg_ctx *c, const hg_genome_batch &b, const hg_sketch_params *p, uint64_t threshold,
                               hg_batch_tables &t, bool planned, uint32_t **d_ndistinct_out, hg_sample_fetch *fetch);
// ... followed by the encoders (several workgroups for the genomes with very large sets); returns with the encoders
// queued, everything before them finished.
hg_status hg_sketch_batch_sync(hg_ctx *c, const hg_genome_batch &b, const hg_sketch_params *p, const hg_sketch_out &out,
                               hg_batch_tables *planned = nullptr);

// One sketch step on device-resident genomes: sync-free when the batch allows it, else the synchronous path.
hg_status hg_sketch_step(hg_ctx *c, const hg_genome_batch &b, const hg_sketch_params *p, const hg_sketch_out &out);
