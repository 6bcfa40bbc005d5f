/*
 * hypergen.h -- C ABI of libhypergen_hip.so, the MI355X (gfx950) implementation of
 * the HyperGen sketch + ANI hot path.
 *
 * This is the drop-in boundary.  Each entry point names the reference interface
 * (wh-xu/Hyper-Gen, file:line) it replaces; INTEGRATION.md shows the Rust
 * `extern "C"` block a maintainer would add in src/sketch_cuda.rs / src/dist.rs.
 *
 * Conventions
 *   - plain C types only; every call returns an hg_status (the reference
 *     .unwrap()s and aborts, src/sketch_cuda.rs:134-156 -- here the caller decides);
 *   - `hg_ctx` owns one device, one stream and growable device workspaces; a ctx is
 *     NOT thread-safe, create one per host thread (the reference binds one shared
 *     CudaDevice per rayon worker, src/sketch_cuda.rs:82);
 *   - "host" entry points take host pointers and stage through the ctx;
 *     "_dev" entry points take device pointers (HBM resident, no PCIe traffic);
 *   - outputs are caller allocated with explicit capacities;
 *   - there is NO CPU fallback: without a usable HIP device hg_ctx_create fails.
 */
#ifndef HYPERGEN_H
#define HYPERGEN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hg_ctx hg_ctx;

typedef enum {
  HG_OK = 0,
  HG_ERR_INVALID = 1,     /* bad argument                                          */
  HG_ERR_NO_DEVICE = 2,   /* no HIP device / device id out of range                */
  HG_ERR_HIP = 3,         /* a HIP runtime call failed (see hg_last_error)         */
  HG_ERR_OOM = 4,         /* device or host allocation failed                      */
  HG_ERR_CAPACITY = 5,    /* caller's output buffer too small; *n_out = needed     */
  HG_ERR_UNSUPPORTED = 6, /* parameter combination not implemented on the device   */
  HG_ERR_IO = 7,          /* file could not be read / written / parsed             */
  HG_ERR_INEXACT = 8      /* integer dot products cannot be evaluated exactly      */
} hg_status;

const char *hg_status_str(hg_status s);
/* message of the last failing call on this ctx (or on ctx creation if ctx == NULL) */
const char *hg_last_error(const hg_ctx *ctx);
/* library version string */
const char *hg_version(void);

/* ---- context ------------------------------------------------------------------
 * replaces CudaDevice::new(0) + load_ptx(..) + bind_to_thread()
 * (src/sketch_cuda.rs:52-60,82).  Kernels are linked into the library, there is no
 * PTX/code-object loading step. */
hg_status hg_ctx_create(int device_id, hg_ctx **out);
void hg_ctx_destroy(hg_ctx *ctx);
/* run all subsequent work on an existing hipStream_t (e.g. torch's current stream).  The handle is used as
 * given: NULL is HIP's default (null) stream -- which IS torch's current stream unless the caller changed
 * it -- so that the ctx's kernels are ordered with the caller's own work on that stream.
 * hg_ctx_reset_stream goes back to the ctx's private non-blocking stream (the state after hg_ctx_create).
 * Both first wait for the work already queued on the stream being left (the ctx workspaces are ordered by
 * one stream at a time). */
hg_status hg_ctx_set_stream(hg_ctx *ctx, void *hip_stream);
hg_status hg_ctx_reset_stream(hg_ctx *ctx);
hg_status hg_ctx_sync(hg_ctx *ctx);
/* How many sketch steps (hg_sketch_batch_dev / _packed calls, sub-batches of the host-fed entry points) the ctx has queued
 * without a host round trip, how many it ran through the synchronous path, and how many of the former it had to run again
 * because their check word asked for it (see "Completion of hg_sketch_batch_dev" below).  NULL pointers are skipped. */
hg_status hg_ctx_sketch_step_counts(hg_ctx *ctx, uint64_t *sync_free, uint64_t *synchronous, uint64_t *redone);
int hg_device_count(void);
/* development / test hook (no reference counterpart): force an internal code path of THIS ctx.
 * keys: "dist_tile" = "" | "small" | "big" | "wide"      (GEMM tile geometry)
 *       "dist_path" = "" | "f16" | "i8" | "cen"            (operand format of the ANI GEMM: raw values as f16 only / try byte
 *                                                           operands / try centred counts as f16 -- also on small problems)
 *       "dist_order" = "" | "plain" | "legacy"             ("plain": a self-comparison does not run its diagonal tiles first;
 *                                                           "legacy": workgroups derive their tile from blockIdx instead of
 *                                                           reading the host's balanced slot -> tile table)
 *       "ham_path"  = "" | "popc" | "mfma" | "fp4"         (Hamming search: xor + popcount, +-1 byte GEMM, +-1 e2m1 GEMM)
 *       "kmer_input" = "" | "packed"                       ("packed": batches that arrive as ASCII are 2-bit packed on the
 *                                                           device first and take the packed-input kernels)
 *       "hostfed" = "" | "ascii" | "packed"                (what hg_sketch_batch / hg_kmer_hash_sample send over the link:
 *                                                           the library's choice / always ASCII / always 2-bit packed on the host)
 *       "sort_test_buckets" = "<n>"   (bucket count of the large-set sort; 0 = automatic)
 *       "pair_limit" = "<n>"          (pairs one launch of a thresholded comparison / search may enumerate before the call is
 *                                      split into blocks of reference rows; 0 = 2^32 - 1, the reach of the hit counter)
 *       "cluster_hit_cap" = "<n>"     (hits the scratch list of hg_cluster_dev starts with -- small forces its grow path;
 *                                      0 = the ctx's own size)
 *       "greedy_rounds" = "<n>"       (rounds hg_cluster_greedy* queue before they read the count of undecided nodes back;
 *                                      0 = the default, 4.  Any value gives the same result: tests run 1 and the default)
 *       "setcover_rounds" = "<n>"     (rounds hg_cluster_setcover* queue before they read the count of undecided nodes back;
 *                                      0 = the default, 4.  Any value gives the same result: tests run 1 and the default)
 *       "tree_rounds" = "<n>"         (rounds hg_cluster_tree* queue before they read the count of selecting roots back;
 *                                      0 = the default, 4.  Any value gives the same result: tests run 1 and the default)
 *       "average_rounds" = "<n>"      (rounds hg_cluster_average* queue before they read the round's merge count back;
 *                                      0 = the default, 4.  Any value gives the same result: tests run 1 and the default)
 *       "average_block_rows" = "<n>"  (rows per block of the ANI matrix in hg_cluster_average_dev; 0 = automatic, from
 *                                      HG_SEARCH_BLOCK_BYTES)
 *       "complete_rounds" = "<n>"     (rounds hg_cluster_complete* queue before they read the round's merge count back;
 *                                      0 = the default, 4.  Any value gives the same result: tests run 1 and the default)
 *       "complete_block_rows" = "<n>" (rows per block of the ANI matrix in hg_cluster_complete_dev; 0 = automatic, from
 *                                      HG_SEARCH_BLOCK_BYTES)
 *       "complete_rescan" = "" | "all" ("all": hg_cluster_complete* scan every live row in every round instead of only the
 *                                      rows a merge invalidated.  Both give the same result and the same round count)
 *       "nj_block_rows" = "<n>"       (rows per block of the ANI matrix in hg_nj_dev; 0 = automatic, from
 *                                      HG_SEARCH_BLOCK_BYTES)
 *       "stats_block_rows" = "<n>"    (rows per block of the ANI matrix in hg_cluster_stats_dev; 0 = automatic, from
 *                                      HG_SEARCH_BLOCK_BYTES)
 *       "search_block_rows" = "<n>"   (reference rows per matrix block of hg_search_topk*; 0 = automatic, from
 *                                      HG_SEARCH_BLOCK_BYTES)
 *       "hostfed_stage_bytes" = "<n>" (bytes of sequence at which hg_sketch_batch closes a sub-batch, twice as many when the
 *                                      batch goes over 2-bit packed; 0 = the default, 64 MiB.  Any value gives the same result)
 * Nothing in the library reads environment variables. */
hg_status hg_ctx_set_debug(hg_ctx *ctx, const char *key, const char *value);

/* per-kernel device timing: when enabled, every kernel launch of the sketch / dist entry
 * points is bracketed by HIP events on the ctx's stream.  hg_ctx_timings waits for the last
 * bracket and returns, per kernel class, the SUM of the launch durations (ms) and the number
 * of launches since the previous hg_ctx_timings call. */
#define HG_T_KMER 0      /* k-mer hash + sample            */
#define HG_T_SORT 1      /* sort + unique                  */
#define HG_T_ENCODE 2    /* HV encode + norm               */
#define HG_T_DIST_PREP 3 /* i16 -> f16 + exactness bounds  */
#define HG_T_DIST 4      /* ANI GEMM (MFMA or integer)     */
#define HG_T_COUNT 5
hg_status hg_ctx_enable_timing(hg_ctx *ctx, int on);
hg_status hg_ctx_timings(hg_ctx *ctx, float ms_sum[HG_T_COUNT], uint32_t launches[HG_T_COUNT]);
/* name of the kernel the last call launched for timing class `cls` (HG_T_KMER, HG_T_DIST), spelled as rocprofv3
 * prints it ("kmer_sample_shared<21, true, false>", "dist_mfma_kernel<false, false, true, true, 5, true, false, false, false>");
 * "" if none.  A measurement harness uses it to check that a committed profile belongs to the kernel that ran.
 * HG_T_DIST after a bit-packed Hamming call: the GEMM's dist_mfma_kernel instantiation when the search ran on the matrix pipe,
 * "hamming_kernel<1>", "<2>" or "<8>" (16, 32 or 128 query columns per tile) when the xor + popcount kernel did the work.
 * HG_T_SORT / HG_T_ENCODE: every kernel the last sketch step (or hg_kmer_hash_sample's sort, hg_hv_encode's encode) queued
 * for the class, in launch order, joined by " + " ("sort_unique_kernel<true> + sort_unique_rest_kernel",
 * "encode_wave_kernel + sketch_finish_kernel"); a step run again later through the synchronous path reports that run.
 * With min_count > 1 the sort class names the min_count_* kernels that ran in place of sort_unique_* / bucket_sort_kernel. */
const char *hg_ctx_last_kernel(const hg_ctx *ctx, int cls);

/* minimal device-memory helpers for callers that have no HIP binding of their own
 * (cudarc's htod_copy / alloc_zeros / sync_reclaim, src/sketch_cuda.rs:134,138,156) */
hg_status hg_dev_alloc(hg_ctx *ctx, size_t bytes, void **dptr);
hg_status hg_dev_free(hg_ctx *ctx, void *dptr);
hg_status hg_copy_h2d(hg_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
hg_status hg_copy_d2h(hg_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* ---- parameters --------------------------------------------------------------- */
#define HG_LAYOUT_SCALAR 0u /* encode_hash_hd       src/hd.rs:94-112               */
#define HG_LAYOUT_AVX2 1u   /* encode_hash_hd_avx2  src/hd.rs:14-92 (x86-64 output) */
#define HG_NORM_ACGT 0u     /* only ACGTacgt are bases (src/cuda_kernel.cu:277-296) */
#define HG_NORM_U2T 1u      /* additionally u/U -> T (needletail normalize)         */

/* mirrors SketchParams (src/types.rs:83-113); defaults k=21 scaled=1500 seed=123
 * canonical=1 hv_d=4096 */
typedef struct {
  uint32_t ksize;     /* 1..255 (u8 in the reference): 1..32 kmer_sample_shared, 33..64 kmer_sample_long<k>, 65..255 run-time k */
  uint32_t canonical; /* 0/1 (honoured like src/cuda_kernel.cu:306-314)             */
  uint64_t scaled;    /* threshold = UINT64_MAX / scaled (src/sketch.rs:73)          */
  uint64_t seed;
  uint32_t hv_d;      /* HV dimension; chunks of 64 are filled (src/hd.rs:34,102)    */
  uint32_t hv_layout; /* HG_LAYOUT_*                                                 */
  uint32_t norm_mode; /* HG_NORM_*                                                   */
  uint32_t min_count; /* keep a sampled k-mer only if it occurs at least this often; 0 and 1: every sampled k-mer (see below) */
} hg_sketch_params;

/* min_count (no reference counterpart; the field was `reserved` and never read).  Let raw be the multiset of sampled hashes of
 * a genome / read set, one per sampled k-mer POSITION, and m = max(1, min_count):
 *     kept = { h : multiplicity of h in raw >= m }, ascending
 * nhash = |kept|; the HV and its norm are the encoder's output for kept.  m = 1 is the reference's HashSet<u64>
 * (src/sketch.rs:93), bit for bit -- what a zero-initialised struct and hg_sketch_params_default (it writes 0) ask for.
 * m >= 2 is for raw READS (Mash's -m): every sequencing error makes up to k k-mers that occur once, and at 30x coverage
 * they outnumber the genome's own.  With canonical != 0 both strands of a k-mer have one hash and count together.  An empty
 * kept gives nhash = 0 and the encoder's row for the empty set.  Counts are taken on the complete raw multiset only: a hit
 * region that overflows is grown and the step run again exactly as for m = 1, before anything is filtered.
 * Honoured by every entry point that takes hg_sketch_params: hg_sketch_batch_dev, hg_sketch_batch_dev_packed, hg_sketch_batch,
 * hg_sketch_batch_multi, hg_sketch_stream_open (every push form), and a sync-free step that is run again synchronously.
 * The .sketch container does not record it. */

void hg_sketch_params_default(hg_sketch_params *p);

/* ---- k-mer hash + FracMinHash sample --------------------------------------------
 * replaces extract_kmer_t1ha2_cuda + kernel cuda_kmer_t1ha2
 * (src/sketch_cuda.rs:120-166, src/cuda_kernel.cu:250-321; CPU twin
 * extract_kmer_hash, src/sketch.rs:71-98).
 * seq   : read_merge_seq layout (src/fastx_reader.rs:6-29), host memory.
 * output: the DISTINCT sampled hashes, ascending (HashSet semantics, lossless: no
 *         per-thread slot cap, hash value 0 is kept).
 * If more than `cap` distinct hashes exist: HG_ERR_CAPACITY and *n_out = count. */
hg_status hg_kmer_hash_sample(hg_ctx *ctx, const uint8_t *seq, size_t n_bps,
                              uint32_t ksize, uint64_t threshold, uint64_t seed,
                              int canonical, uint32_t norm_mode, uint64_t *out_hashes,
                              size_t cap, size_t *n_out);
/* The same with the min_count filter of hg_sketch_params: output = the sampled hashes that occur at least max(1, min_count)
 * times among the sequence's sampled k-mer positions, ascending.  Same capacity rule: HG_ERR_CAPACITY and *n_out = the number
 * of hashes kept.  min_count <= 1 is hg_kmer_hash_sample. */
hg_status hg_kmer_hash_sample_min_count(hg_ctx *ctx, const uint8_t *seq, size_t n_bps,
                                        uint32_t ksize, uint64_t threshold, uint64_t seed,
                                        int canonical, uint32_t norm_mode, uint32_t min_count,
                                        uint64_t *out_hashes, size_t cap, size_t *n_out);

/* ---- HV encode -------------------------------------------------------------------
 * replaces hd::encode_hash_hd{,_avx2} + dist::compute_hv_l2_norm
 * (src/hd.rs:14-112, src/dist.rs:132-137).  `hashes` must be distinct (host). */
hg_status hg_hv_encode(hg_ctx *ctx, const uint64_t *hashes, size_t n, uint32_t hv_d,
                       uint32_t hv_layout, int16_t *hv_out, int32_t *norm2_out);

/* ---- whole-batch sketch ------------------------------------------------------------
 * what the rayon loop body of src/sketch.rs:35-48 / src/sketch_cuda.rs:79-96 does per
 * file (hash+sample -> set -> HV encode -> norm), for n genomes in one call.
 *
 * _dev: d_seq holds all genomes (device memory); genome i occupies
 * [offsets[i], offsets[i] + lens[i]) (host arrays).  offsets must be multiples of 4
 * and the allocation must be readable for 32 bytes past every genome's end.
 * d_hv      : n * hv_d int16 (device), d_norm2 : n int32 (device),
 * d_nhash   : n uint32 (device) = number of distinct sampled hashes. */
hg_status hg_sketch_batch_dev(hg_ctx *ctx, const uint8_t *d_seq, const uint64_t *offsets,
                              const uint64_t *lens, size_t n, const hg_sketch_params *p,
                              int16_t *d_hv, int32_t *d_norm2, uint32_t *d_nhash);
/* Completion of hg_sketch_batch_dev / _packed.  The call queues the whole step -- hash + sample, sort / unique, encode --
 * on the ctx's stream and returns; no host round trip separates the kernels.  What the host used to read back between
 * them (did a genome outgrow its hit region -- more than twice its expected number of sampled k-mers + 1 024, the
 * signature of a sampled k-mer repeated thousands of times -- or the one-workgroup sort) comes back as ONE check word
 * behind the last kernel, and the library reads it when the NEXT call on the ctx, or hg_ctx_sync, arrives: a step that
 * reported such a genome is then run again through the synchronous path (exact capacities, multi-workgroup sort), before
 * that call does anything else.  Hence:
 *   - d_seq, d_hv, d_norm2, d_nhash belong to the library until the next call on the ctx or hg_ctx_sync has returned;
 *   - results are FINAL after hg_ctx_sync (or any later call on the ctx) has returned.  A consumer that orders itself
 *     behind the call on the stream alone sees final rows too, except for the genomes of such a step: their d_nhash holds
 *     HG_NHASH_PENDING (and their HV rows are untouched) until the library has redone the step;
 *   - an error of the re-run is returned by the call that triggered it.
 * Batches whose genomes are EXPECTED to exceed the one-workgroup sort (more than ~7 000 sampled k-mers: 10 Mbp at
 * scaled = 1 500) take the synchronous path at once and are final in stream order; hg_ctx_set_debug(ctx, "sketch_path",
 * "sync") sends every batch that way (the behaviour up to round 5: counters read back between sort and encode).
 * All of this is the same for every p->min_count: the check word is raised by RAW counts (before the filter), pending rows
 * carry HG_NHASH_PENDING, and results are final after hg_ctx_sync. */
#define HG_NHASH_PENDING 0xFFFFFFFFu
/* How the library would lay a batch out for the k-mer launch (host arithmetic only; no ctx, no device): counts[0] = work items
 * (pieces of 27 432 k-mer starts for k <= 21, 27 324 for k <= 32, 12 288 beyond), [1] = workgroups -- for k <= 32 the work
 * items of consecutive SMALL genomes share a workgroup, up to three full items' worth of tiles --, [2] = hit slots, [3] = largest
 * hit region, [4] = largest expected sampled count of a genome, [5] = tiles of a full work item (0 for k > 32).  group_first
 * (optional, cap entries): first work item of every workgroup, then the item count (counts[1] + 1 entries; k <= 32 only). */
hg_status hg_sketch_plan_describe(const uint64_t *offsets, const uint64_t *lens, size_t n, uint32_t ksize, uint64_t scaled,
                                  uint64_t counts[6], uint32_t *group_first, size_t cap);
/* The same batch with the genomes resident as 2-bit PACKED bases: genome i is the hg_pack2 blob (layout below:
 * 4 bases per byte + the not-a-base bitmap, 0.375 bytes per base in HBM instead of 1) at d_blobs + offsets[i]
 * (multiples of 16; 32 readable bytes behind every blob), n_bps[i] = its number of bases.  The k-mer kernels read the
 * codes as they lie -- no ASCII copy exists on the device -- and the result is bit-identical to hg_sketch_batch_dev on
 * the sequences the blobs were packed from (under the norm_mode they were packed with; p->norm_mode is not applied
 * again).  The pattern of the reference's second kernel (src/cuda_kernel.cu:15-69 on NT4 codes, src/sketch_cuda.rs:23-32). */
hg_status hg_sketch_batch_dev_packed(hg_ctx *ctx, const uint8_t *d_blobs, const uint64_t *offsets,
                                     const uint64_t *n_bps, size_t n, const hg_sketch_params *p,
                                     int16_t *d_hv, int32_t *d_norm2, uint32_t *d_nhash);
/* host buffers in, host results out.  The sequences cross the link in sub-batches that upload while the previous one is
 * sketched.  What crosses is the library's choice and never changes a result bit: a batch of >= 32 MB on a host with >= 4
 * usable cores is 2-bit packed by up to 16 host threads of the call (hg_pack2 blobs, 0.375 bytes per base, in pieces of
 * 1 Mbase into page-locked staging; the packed-input kernels sketch them) -- 2.3x the ASCII rate on the measured box,
 * where host DRAM (114 GB/s of packing reads) then limits instead of PCIe; the first sub-batch is timed and the rest goes
 * as ASCII when the host packs slower than the link carries.  A call with n = 1 packs on the calling thread when the
 * source is pageable memory, or when >= 3 other host-fed calls of the process are in flight (the reference's
 * one-call-per-genome pattern from a thread pool, src/sketch_cuda.rs:79-96: the calls share one link) and the calling
 * threads together pack fast enough for that to pay -- their rate is measured in the packed calls; when it falls short
 * (a host whose memory is busy) the following calls go as ASCII for a while before packing is tried again.  Debug key
 * "hostfed" = "ascii" | "packed" pins the choice.  The same rule applies to hg_kmer_hash_sample. */
hg_status hg_sketch_batch(hg_ctx *ctx, const uint8_t *const *seqs, const size_t *lens,
                          size_t n, const hg_sketch_params *p, int16_t *hv_out,
                          int32_t *norm2_out, uint32_t *nhash_out);

/* ---- ANI ------------------------------------------------------------------------------
 * replaces dist::compute_hv_ani / compute_pairwise_ani (src/dist.rs:139-161,231-294).
 * ref_hv: R x hv_d int16 row-major (decompressed sketches), qry_hv: Q x hv_d.
 * ani_out[r * Q + q] = ANI in percent (0..100), float32 arithmetic in the reference's
 * operation order, INCLUDING its logarithm: Rust's f32::ln is the C library's logf, and the device evaluates glibc's logf
 * algorithm (sysdeps/ieee754/flt-32/e_logf.c) operation for operation (csrc/hg_logf.h), so an ANI value is the float the
 * reference computes for the same dot product and norms, bit for bit -- and with it the third decimal of a TSV line, the
 * side of `ani >= ani_th` and the order of near-ties.  Dot products are exact integers (HG_ERR_INEXACT is never a silent
 * rounding: it is returned only if no exact device path applies). */
hg_status hg_dist_full(hg_ctx *ctx, const int16_t *ref_hv, const int32_t *ref_norm2,
                       size_t R, const int16_t *qry_hv, const int32_t *qry_norm2, size_t Q,
                       uint32_t hv_d, uint32_t ksize, float *ani_out);
hg_status hg_dist_full_dev(hg_ctx *ctx, const int16_t *d_ref_hv, const int32_t *d_ref_norm2,
                           size_t R, const int16_t *d_qry_hv, const int32_t *d_qry_norm2,
                           size_t Q, uint32_t hv_d, uint32_t ksize, float *d_ani_out);
/* Completion of the *_dev entry points: their device inputs are read, and their device outputs written,
 * in stream order on the ctx's stream (hg_ctx_set_stream), so work the caller queues on that stream before
 * / after the call is ordered with it.  When hg_dist_dev / hg_hamming_search_dev (and their _block forms) return, every
 * kernel queued on the stream before and by the call has finished (the hit count comes back through a page-locked
 * block the last kernel writes and the host polls for a bounded time before it falls back to a blocking stream
 * synchronisation); one 64-byte hipMemsetAsync that re-zeroes the call's counter words may still be pending on the
 * stream -- it touches nothing the caller sees.  hg_dist_full_dev may return with its last kernels still running --
 * hg_ctx_sync (or the caller's own stream synchronisation) completes them; for hg_sketch_batch_dev see "Completion of
 * hg_sketch_batch_dev" above. */
/* The ANI formula's two pieces on their own (diagnostics): d_out[i] = the library's logf of d_x[i] -- or, with d_x ==
 * NULL, of the float whose bit pattern is first_bits + i (an exhaustive sweep needs no input array); d_ani[i] = the tail
 * of compute_pairwise_ani (src/dist.rs:153-160) for the integer dot product d_dot[i] and the norms.  Stream-ordered. */
hg_status hg_logf_dev(hg_ctx *ctx, const float *d_x, uint32_t first_bits, size_t n, float *d_out);
hg_status hg_ani_from_dots_dev(hg_ctx *ctx, const int32_t *d_dot, const int32_t *d_norm2_r, const int32_t *d_norm2_q,
                               size_t n, uint32_t ksize, float *d_ani);

/* ANI metric of a ctx (no reference counterpart; the reference computes HG_ANI_MASH only, src/dist.rs:153-160).  With
 * J = dot / (nr + nq - dot) and k = ksize, every metric is ani = 1 + ln(x) / k -> NaN to 0, clamped to [0, 1], x 100, f32
 * arithmetic in this order and the device's logf bit for bit, where x is
 *   HG_ANI_MASH            : 2 / (1 / J + 1)        (the default; symmetric)
 *   HG_ANI_CONTAINMENT     : dot / nq               (the share of the QUERY's hashes found in the reference; directional)
 *   HG_ANI_MAX_CONTAINMENT : dot / min(nr, nq)      (i32 min of the norms as passed; symmetric)
 * Containment estimates the identity of a fragment (a partial MAG, a plasmid, a draft) with a larger genome, where J --
 * and with it the Mash-style value -- falls with the difference in size.  With equal norms all three agree up to rounding.
 * dot <= 0 gives 0, a zero denominator 0 (dot = 0) or 100 (dot > 0), dot > denominator 100.
 * hg_ctx_set_ani_metric: host-side state of the ctx like its stream, read when each call is made; HG_ERR_INVALID for any other
 * value.  It applies to hg_dist_full{,_dev}, hg_dist{,_dev}, hg_dist_block_dev, hg_dist_block_ops_dev, hg_dist_multi{,_dev}
 * (hg_multi_set_ani_metric sets every shard's ctx), hg_search_topk{,_dev,_block_dev,_multi_dev}, hg_cluster{,_dev},
 * hg_cluster_greedy{,_dev}, hg_cluster_setcover{,_dev}, hg_cluster_tree{,_dev}, hg_cluster_average{,_dev}, hg_cluster_complete{,_dev}, hg_cluster_stats{,_dev} and hg_ani_from_dots_dev.  symmetric != 0 under
 * HG_ANI_CONTAINMENT is HG_ERR_INVALID (the metric is directional: call without it for every ordered pair); hg_cluster{,_dev},
 * hg_cluster_greedy{,_dev}, hg_cluster_setcover{,_dev}, hg_cluster_tree{,_dev}, hg_cluster_average{,_dev}, hg_cluster_complete{,_dev} and hg_cluster_stats{,_dev}
 * accept HG_ANI_MASH and HG_ANI_MAX_CONTAINMENT only.  hg_cluster_add_hits_dev, hg_cluster_greedy_hits_dev, hg_cluster_setcover_hits_dev and
 * hg_cluster_tree_hits_dev (they take hits), hg_cluster_average_matrix_dev, hg_cluster_complete_matrix_dev and hg_cluster_stats_matrix_dev (they take the matrix), hg_dist_prep_ops_dev, the
 * sort / top-k calls, hg_ani_pairs{,_dev} (its columns name their metrics) and the Hamming search do not depend on it.  hg_nj{,_dev}
 * read it and accept the two symmetric metrics as clustering does; hg_nj_matrix_dev and hg_nj_newick do not depend on it.
 * hg_ctx_ani_metric: HG_ANI_MASH on a fresh ctx. */
#define HG_ANI_MASH 0
#define HG_ANI_CONTAINMENT 1
#define HG_ANI_MAX_CONTAINMENT 2
hg_status hg_ctx_set_ani_metric(hg_ctx *ctx, int metric);
int hg_ctx_ani_metric(const hg_ctx *ctx);

/* one reported pair: what dump_ani_file prints per line (src/utils.rs:275-285) */
typedef struct {
  uint32_t ref_idx;
  uint32_t qry_idx;
  float ani;
} hg_ani_hit;

/* thresholded form: pairs with ani >= ani_th.  symmetric != 0 enumerates only
 * ref_idx < qry_idx (src/dist.rs:243-265).  Hits come back in no particular order
 * (hg_sort_ani_hits gives the reference's file order).  *n_out = number of hits found;
 * if it exceeds cap only cap are stored and HG_ERR_CAPACITY is returned.
 * `out` is host memory for hg_dist and device memory for hg_dist_dev.
 * A set compared with itself (the reference's path_r == path_q case, src/dist.rs:13) is recognised by identical
 * pointers and row counts on both sides: hg_dist uploads it once, and the device path prepares its operands once
 * and runs the tiles on the matrix diagonal -- where such a comparison has its dense blocks of hits -- first.  The
 * result is the same set of hits either way.
 * The kernels count hits in 32 bits: a call of more than 2^32 - 1 pairs (66 000 x 66 000 and up) runs as blocks of
 * reference rows of fewer pairs each (hg_dist_block_dev does that by itself); counts add up in 64 bits, and once `out` is
 * full the remaining blocks only count.  hg_hamming_search(_block)_dev likewise. */
hg_status hg_dist(hg_ctx *ctx, const int16_t *ref_hv, const int32_t *ref_norm2, size_t R,
                  const int16_t *qry_hv, const int32_t *qry_norm2, size_t Q, uint32_t hv_d,
                  uint32_t ksize, int symmetric, float ani_th, hg_ani_hit *out, size_t cap,
                  size_t *n_out);
hg_status hg_dist_dev(hg_ctx *ctx, const int16_t *d_ref_hv, const int32_t *d_ref_norm2,
                      size_t R, const int16_t *d_qry_hv, const int32_t *d_qry_norm2, size_t Q,
                      uint32_t hv_d, uint32_t ksize, int symmetric, float ani_th,
                      hg_ani_hit *d_out, size_t cap, size_t *n_out);

/* One block of a larger R x Q matrix (multi-GPU decomposition): rows ref_off.. and columns
 * qry_off.. of the global enumeration.  Hits carry GLOBAL indices and `symmetric` keeps global ref < global qry,
 * so the union over the blocks of a partition equals the one-call result. */
hg_status hg_dist_block_dev(hg_ctx *ctx, const int16_t *d_ref_hv, const int32_t *d_ref_norm2, size_t R,
                            size_t ref_off, const int16_t *d_qry_hv, const int32_t *d_qry_norm2, size_t Q,
                            size_t qry_off, uint32_t hv_d, uint32_t ksize, int symmetric, float ani_th,
                            hg_ani_hit *d_out, size_t cap, size_t *n_out);

/* ---- sharded dist: reference operands prepared where the rows live -----------------------------------
 * hg_dist_block_dev needs every reference row as i16 (8 KiB at D = 4096) and converts ALL of them to its byte operands
 * itself: with the references spread over N GPUs that is an exchange of R x D x 2 bytes and an N-fold repeated prepass.
 * Here the rank that OWNS a row prepares it once -- hg_dist_prep_ops_dev: the centred byte operand (src/hd.rs:29,84-87:
 * hv = 2 * count - n, so (hv + e) >> 1 fits a byte), 4 KiB + 128 at D = 4096, and a 72-byte control record -- and the
 * exchange moves those (half the bytes; the reference's i16 rows never travel).  hg_dist_block_ops_dev is
 * hg_dist_block_dev with the reference side given that way; the query side is still the caller's own i16 rows.
 *   d_ops   : rows x hg_dist_ops_row_bytes(hv_d) bytes;  d_meta : rows x hg_dist_ops_meta_bytes() bytes (opaque);
 *   d_flag  : ONE device word per prepared block: 0 = every row fits the byte scheme.  The consumer passes the flag
 *             words of all blocks it gathered (d_flags, n_flags).
 *   d_ref_ops (consumer): room for hg_dist_ops_padded_rows(R) rows -- the tiles overhang, the call zeroes the rows behind R.
 *   d_ref_index: NULL (row i is global reference ref_off + i) or the global index of every row, for a gathered block
 *             whose rows are not one contiguous range (chunked exchanges); not with `symmetric`.
 * Returns HG_ERR_INEXACT, with nothing reported, when an owner's flag is set or the call's own query rows do not fit
 * the scheme (sketches beyond ~6 000 hashes at D = 4096): the caller then gathers the i16 rows and uses
 * hg_dist_block_dev -- same hits either way.  hv_d <= 8192, hv_d % 8 == 0. */
size_t hg_dist_ops_row_bytes(uint32_t hv_d);
size_t hg_dist_ops_meta_bytes(void);
size_t hg_dist_ops_padded_rows(size_t rows);
hg_status hg_dist_prep_ops_dev(hg_ctx *ctx, const int16_t *d_hv, size_t rows, uint32_t hv_d, uint8_t *d_ops,
                               uint8_t *d_meta, uint32_t *d_flag);
hg_status hg_dist_block_ops_dev(hg_ctx *ctx, const uint8_t *d_ref_ops, const uint8_t *d_ref_meta, const int32_t *d_ref_norm2,
                                size_t R, size_t ref_off, const uint32_t *d_ref_index, const uint32_t *d_flags,
                                size_t n_flags, const int16_t *d_qry_hv, const int32_t *d_qry_norm2, size_t Q,
                                size_t qry_off, uint32_t hv_d, uint32_t ksize, int symmetric, float ani_th,
                                hg_ani_hit *d_out, size_t cap, size_t *n_out);

/* Which exact operand path the last hg_dist / hg_dist_dev / hg_dist_block_dev call of this ctx took (all give the same
 * integers): 0 = the raw values as f16 operands on v_mfma_f32_16x16x32_f16 (exact f32 windows), 1 = centred i8 operands on
 * v_mfma_i32_16x16x64_i8 (sketches of up to ~6 000 hashes at D = 4096; decided on the device), 2 = integer VALU fallback,
 * 3 = the centred counts as f16 operands (one exact f32 window up to ~16 000 hashes per sketch at D = 4096: where byte
 * operands stop); -1 = none yet. */
int hg_ctx_last_dist_path(const hg_ctx *ctx);

/* order of dump_ani_file (src/utils.rs:262-269): stable ascending sort by ANI over the
 * reference's pair enumeration, then reversed.  Host side. */
void hg_sort_ani_hits(hg_ani_hit *hits, size_t n, size_t Q, int symmetric);

/* the same order produced on the device (stable radix passes over the enumeration key, then the ANI), in place on
 * a device-resident hit list; stream-ordered, returns without synchronising.  _staged: host list in and out through
 * the ctx (upload, device sort, download) -- a 10^6-hit list orders in ~1 ms instead of ~100 ms of host sort. */
hg_status hg_sort_ani_hits_dev(hg_ctx *ctx, hg_ani_hit *d_hits, size_t n, size_t Q);
hg_status hg_sort_ani_hits_staged(hg_ctx *ctx, hg_ani_hit *hits, size_t n, size_t Q);

/* `search` (an empty stub in the reference, src/main.rs:22-24; defined here): per query the k best references of
 * a hit list (e.g. the output of hg_dist_dev), descending ANI, ties by ascending reference index.
 * d_out: Q * k entries, query q's results at d_out[q*k ..], unused slots have ref_idx = 0xFFFFFFFF;
 * d_counts[q] = number of valid entries (<= k).  Device pointers; stream-ordered. */
hg_status hg_topk_per_query_dev(hg_ctx *ctx, const hg_ani_hit *d_hits, size_t n, size_t Q, uint32_t k,
                                hg_ani_hit *d_out, uint32_t *d_counts);

/* ANI of listed pairs (no reference counterpart): every metric of pair (ref_idx, qry_idx) of a list, from one exact dot per
 * pair -- without the R x Q comparison.  ani_pairs_kernel: one wave per pair streams both rows (16-byte loads when
 * hv_d % 8 == 0, 2-byte loads otherwise; nothing behind a row's end is read), forms the wrapping i32 dot like
 * dist_skinny_kernel and finishes it with the formulas of hg_ctx_set_ani_metric.
 *   d_pairs : n_pairs records hg_ani_hit; the `ani` field is ignored, so the output of hg_dist_dev, hg_sort_ani_hits_dev,
 *             hg_topk_per_query_dev, hg_search_topk* and hg_cluster_tree* goes in as it lies.  Duplicates, any order and
 *             ref_idx == qry_idx with identical buffers are allowed.  A record with ref_idx == HG_PAIRS_EMPTY is an empty slot
 *             (the top-k layout's): its floats and its dot are 0.  Any other record with ref_idx >= R or qry_idx >= Q makes the
 *             call HG_ERR_INVALID (its rows are not read, the outputs' contents are unspecified, the next call starts clean).
 *   columns : a mask of HG_PAIRS_*, < 16.  d_ani holds n_pairs x popcount(columns) floats, pair-major, a pair's values in
 *             ascending order of the column bits.  The value of (r, q) under a column is, bit for bit, what hg_dist_full_dev
 *             writes at [r, q] under the corresponding ctx metric; under HG_PAIRS_CONTAINMENT_REF what it writes at [q, r] with
 *             the two sets exchanged under HG_ANI_CONTAINMENT.  The call does not depend on hg_ctx_set_ani_metric.
 *   d_dot   : NULL or n_pairs wrapped i32 dots.  columns == 0 is allowed with d_dot (d_ani may then be NULL); columns == 0
 *             without d_dot and columns >= 16 are HG_ERR_INVALID.
 * n_pairs == 0: HG_OK, nothing is written; n_pairs >= 2^32: HG_ERR_UNSUPPORTED; R, Q, hv_d (1..65536) and ksize as for
 * hg_dist_dev; NULL d_pairs, row or norm pointers with n_pairs > 0: HG_ERR_INVALID.  d_ani and d_dot must not overlap d_pairs.
 * Inputs are read in stream order on the ctx's stream; results are final on return, as for hg_dist_dev (the error word comes
 * back the way its hit count does).  With timing on the launch counts under HG_T_DIST.
 *   hg_ani_pairs : host arrays in and out, staged through the ctx like hg_dist. */
#define HG_PAIRS_MASH 1u            /* 2 / (1 / J + 1)       = HG_ANI_MASH            */
#define HG_PAIRS_CONTAINMENT 2u     /* dot / nq              = HG_ANI_CONTAINMENT     */
#define HG_PAIRS_MAX_CONTAINMENT 4u /* dot / min(nr, nq)     = HG_ANI_MAX_CONTAINMENT */
#define HG_PAIRS_CONTAINMENT_REF 8u /* dot / nr: the share of the REFERENCE's hashes found in the query
                                       (HG_ANI_CONTAINMENT with the two sides exchanged)              */
#define HG_PAIRS_EMPTY 0xFFFFFFFFu  /* ref_idx of an empty slot (the top-k layout's)                   */
hg_status hg_ani_pairs_dev(hg_ctx *ctx, const int16_t *d_ref_hv, const int32_t *d_ref_norm2, size_t R,
                           const int16_t *d_qry_hv, const int32_t *d_qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize,
                           const hg_ani_hit *d_pairs, size_t n_pairs, uint32_t columns, float *d_ani, int32_t *d_dot);
hg_status hg_ani_pairs(hg_ctx *ctx, const int16_t *ref_hv, const int32_t *ref_norm2, size_t R, const int16_t *qry_hv,
                       const int32_t *qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, const hg_ani_hit *pairs,
                       size_t n_pairs, uint32_t columns, float *ani, int32_t *dot);

/* search: exact top-k per query in bounded memory (no reference counterpart, like hg_topk_per_query_dev).  The same result
 * as hg_dist_dev(ani_th) followed by hg_topk_per_query_dev -- per query the k references with the highest ANI among those with
 * ani >= ani_th (the float comparison of hg_dist_dev), descending ANI, ties by ascending GLOBAL reference index -- without the
 * hit list: the ANI matrix is computed in blocks of reference rows (hg_dist_full_dev into a scratch block of the ctx, at most
 * HG_SEARCH_BLOCK_BYTES unless one row is larger; debug key "search_block_rows" forces the row count), each block goes
 * through search_topk_select_kernel (a sorted list of k keys per thread in LDS; one compare against the k-th key rejects)
 * and search_topk_merge_kernel (slice lists into the running Q x k state).  Device memory: one block + its slice lists (32 MiB
 * at most unless Q * k * 8 is larger) + Q * k * 8 bytes, whatever the number of pairs at or above the threshold.  The order is
 * total, so the output does not depend on block size, slices or scheduling.  k <= HG_SEARCH_TOPK_MAX (HG_ERR_UNSUPPORTED
 * beyond); k == 0 or Q == 0: HG_OK, nothing is written; R == 0: every count 0, every slot empty; NULL pointers:
 * HG_ERR_INVALID; errors of the dist call (HG_ERR_INEXACT ...) pass through.  Honours hg_ctx_set_ani_metric.
 * Output layout of hg_topk_per_query_dev: d_out holds Q * k hg_ani_hit, query q's results at d_out[q * k ..], best first,
 * unused slots have ref_idx = 0xFFFFFFFF (qry_idx = 0xFFFFFFFF, ani = 0); d_counts[q] <= k.
 *   hg_search_topk_dev       : device pointers; stream-ordered, returns without synchronising (the dist call's operand
 *                              prepass reads a few statistics words back per block; nothing else waits for the device).
 *   hg_search_topk_block_dev : the same on rows ref_off.. / columns qry_off.. of a larger problem: hits carry global indices.
 *   hg_search_topk           : host arrays in and out, staged through the ctx like hg_dist.
 *   hg_search_topk_merge     : host side, no ctx: n_lists results of the layout above (lists[l], counts[l]; the same Q and
 *                              k, disjoint references) merged by the same order into out / counts_out.
 *   hg_search_topk_multi_dev : references sharded by rows -- shard s holds ref_rows[s] consecutive rows at d_ref_hv[s] /
 *                              d_ref_norm2[s] on its device, global row order = shard order -- and ALL Q query rows on every
 *                              shard (d_qry_hv[s] / d_qry_norm2[s]: the small side is broadcast, like
 *                              hg_hamming_search_multi; no reference row moves).  Every shard runs
 *                              hg_search_topk_block_dev; the lists are merged on the host into out / counts (host memory). */
#define HG_SEARCH_TOPK_MAX 64u
#define HG_SEARCH_BLOCK_BYTES ((size_t)256 << 20) /* budget of the scratch block of the ANI matrix: 256 MiB */
hg_status hg_search_topk_dev(hg_ctx *ctx, const int16_t *d_ref_hv, const int32_t *d_ref_norm2, size_t R,
                             const int16_t *d_qry_hv, const int32_t *d_qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize,
                             float ani_th, uint32_t k, hg_ani_hit *d_out, uint32_t *d_counts);
hg_status hg_search_topk_block_dev(hg_ctx *ctx, const int16_t *d_ref_hv, const int32_t *d_ref_norm2, size_t R, size_t ref_off,
                                   const int16_t *d_qry_hv, const int32_t *d_qry_norm2, size_t Q, size_t qry_off,
                                   uint32_t hv_d, uint32_t ksize, float ani_th, uint32_t k, hg_ani_hit *d_out,
                                   uint32_t *d_counts);
hg_status hg_search_topk(hg_ctx *ctx, const int16_t *ref_hv, const int32_t *ref_norm2, size_t R, const int16_t *qry_hv,
                         const int32_t *qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, float ani_th, uint32_t k,
                         hg_ani_hit *out, uint32_t *counts);
hg_status hg_search_topk_merge(const hg_ani_hit *const *lists, const uint32_t *const *counts, size_t n_lists, size_t Q,
                               uint32_t k, hg_ani_hit *out, uint32_t *counts_out);

/* `cluster` (no reference counterpart; its users cluster dump_ani_file's TSV, src/utils.rs:262-285, in another tool):
 * single-linkage clustering at an ANI threshold.  The graph has an edge {i, j} for every pair i < j with ani >= ani_th
 * (the ANI of hg_dist_dev, the side of the threshold exactly as there).  For every sketch i:
 *   rep[i]     = the smallest index of i's connected component (i itself without edges);
 *   cluster[i] = the component's dense id: 0, 1, ... in increasing order of rep (the file order of the clusters' first members);
 *   *n_clusters = the number of components.
 * The result depends on the graph alone -- not on scheduling, blocks, hit order or how many calls delivered the hits.
 * d_rep / d_cluster: n uint32 of device memory, n < 2^32 (hg_cluster_dev / hg_cluster: n < 2^31).
 * Step by step, on a hit list the caller has (e.g. of hg_dist_dev at a low threshold, clustered at several higher ones
 * without another GEMM; or of several hg_dist_block_dev calls / GPUs):
 *   hg_cluster_init_dev     : d_rep[i] = i.  Stream-ordered.
 *   hg_cluster_add_hits_dev : unions the hits with ani >= ani_th (self-pairs ignored) into d_rep; any number of calls,
 *                             stream-ordered.  A hit with an index >= n is skipped and remembered.
 *   hg_cluster_finish_dev   : d_rep[i] = the component minimum, d_cluster, *n_clusters; final when it returns (like
 *                             hg_dist_dev once its count is back).  HG_ERR_INVALID if a hit given since the init had an
 *                             index >= n.
 * That error word is kept by the ctx: one step-by-step clustering at a time per ctx. */
hg_status hg_cluster_init_dev(hg_ctx *ctx, uint32_t *d_rep, size_t n);
hg_status hg_cluster_add_hits_dev(hg_ctx *ctx, uint32_t *d_rep, size_t n, const hg_ani_hit *d_hits, size_t n_hits,
                                  float ani_th);
hg_status hg_cluster_finish_dev(hg_ctx *ctx, uint32_t *d_rep, size_t n, uint32_t *d_cluster, size_t *n_clusters);
/* The whole job on resident sketches (d_hv: n x hv_d int16, d_norm2: n): init, the symmetric comparison in blocks of rows
 * [r0, r0 + rows) x columns [r0, n) into a scratch hit list the ctx owns, each block unioned before the next one runs
 * (the hits of the whole matrix are never held at once -- past 66 000 sketches their count can pass 2^32), finish.  The
 * scratch list grows to a block's hit count when it overflows, and the block runs again (debug key "cluster_hit_cap"
 * sets the size it starts with).  hg_cluster: host arrays in and out, staged through the ctx. */
hg_status hg_cluster_dev(hg_ctx *ctx, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                         float ani_th, uint32_t *d_rep, uint32_t *d_cluster, size_t *n_clusters);
hg_status hg_cluster(hg_ctx *ctx, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                     float ani_th, uint32_t *rep, uint32_t *cluster, size_t *n_clusters);

/* Greedy representative clustering (no reference counterpart; what dereplication tools do -- CD-HIT's incremental scheme):
 * one representative per cluster and every other sketch within the threshold of ITS representative, neither of which
 * single linkage gives (a chain 0 - 1 - 2 with ani(0, 2) < ani_th is one component there).  Input: n sketches in
 * processing order 0 .. n - 1 and a symmetric ANI (HG_ANI_MASH or HG_ANI_MAX_CONTAINMENT; HG_ANI_CONTAINMENT is
 * HG_ERR_INVALID as for hg_cluster_dev); the side of the threshold is the float comparison ani >= ani_th of hg_dist_dev.
 * Going through i = 0, 1, ...:
 *   i is a REPRESENTATIVE iff no representative j < i has ani(j, i) >= ani_th;
 *   otherwise i is a MEMBER of the representative j < i with the highest ani(j, i) (float comparison, ties to the smallest
 *   j).  Only earlier representatives count: a later one that is within the threshold of i does not take it over.
 *   A member covers nobody: if 1 is a member of 0 and 2 is within the threshold of 1 only, 2 is a representative.
 * So representatives are pairwise below the threshold and every member is at or above it with its own representative.
 *   rep[i]      = i for a representative, its representative for a member;
 *   cluster[i]  = the dense id of rep[i]: 0, 1, ... in increasing order of the representatives' indices;
 *   *n_clusters = the number of representatives;
 *   ani[i]      = 100.0f for a representative, the ANI of the pair (rep[i], i) for a member (optional: may be NULL).
 * The result depends on the graph and its ANI values alone -- not on block size, hit order, scheduling or the number of
 * rounds.  n < 2^31; n == 0: HG_OK, *n_clusters = 0; NULL rep / cluster / n_clusters: HG_ERR_INVALID; results are final on
 * return, as for hg_cluster_dev.
 * On the device the walk is resolved in rounds (hg_cluster_greedy.hip): greedy_mark_kernel, one lane per hit -- a
 * representative makes its later neighbours members, two undecided ends block the later one for the round -- then
 * greedy_decide_kernel, one lane per node -- undecided and not blocked: representative; the smallest undecided node is
 * decided in every round.  The host queues "greedy_rounds" rounds (hg_ctx_set_debug; default 4) per readback of the
 * undecided count and stops at 0.  Dense groups resolve in about two rounds; the worst case, a path 0 - 1 - 2 - ...,
 * takes about n / 2 rounds (accepted).  greedy_assign_kernel then gives every covered node its best representative (a 64-bit
 * atomic max), and the dense ids come from hg_cluster_finish_dev's kernels.
 *   hg_cluster_greedy_dev : resident sketches; the symmetric comparison in the row blocks of hg_cluster_dev (scratch list,
 *                           "pair_limit", "cluster_hit_cap" and its grow path as there), each block resolved before the next.
 *   hg_cluster_greedy     : host arrays in and out, staged through the ctx. */
/* complete hit list of the caller (e.g. hg_dist_dev at a low threshold, resolved at several higher ones): either orientation,
 * duplicates and self-pairs allowed (self-pairs ignored, a pair given twice counts with each ANI; the highest wins);
 * hits below ani_th ignored; an index >= n (at any ANI): HG_ERR_INVALID, nothing reported, the next call starts clean */
hg_status hg_cluster_greedy_hits_dev(hg_ctx *ctx, size_t n, const hg_ani_hit *d_hits, size_t n_hits, float ani_th,
                                     uint32_t *d_rep, uint32_t *d_cluster, float *d_ani, size_t *n_clusters);
hg_status hg_cluster_greedy_dev(hg_ctx *ctx, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d,
                                uint32_t ksize, float ani_th, uint32_t *d_rep, uint32_t *d_cluster, float *d_ani,
                                size_t *n_clusters);
hg_status hg_cluster_greedy(hg_ctx *ctx, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                            float ani_th, uint32_t *rep, uint32_t *cluster, float *ani, size_t *n_clusters);
/* rounds of the last greedy call on this ctx, summed over its blocks (diagnostic; 0 = none yet) */
uint64_t hg_ctx_cluster_greedy_rounds(const hg_ctx *ctx);

/* Greedy set-cover clustering (no reference counterpart; the scheme MMseqs2 and Linclust cluster with by default): the
 * guarantees of hg_cluster_greedy -- representatives pairwise below the threshold, every member at or above it with its own
 * representative -- with the representative chosen by coverage instead of by position: a star whose centre is the last sketch
 * is n - 1 greedy clusters and one here, a chain 0 - 1 - 2 two greedy clusters and one here, around sketch 1.
 * Input: n sketches, hit records {ref_idx, qry_idx, ani} and ani_th.  A record COUNTS iff ani >= ani_th (the float comparison
 * of hg_dist_dev: NaN never counts) and ref_idx != qry_idx; a counting record is an edge between its two indices, in either
 * orientation.  An index >= n in any record, at any ANI: HG_ERR_INVALID, nothing reported, the next call on the ctx starts
 * clean.  U is the set of undecided nodes, at first all of them.  While U is not empty:
 *   1. deg(v) = the number of counting records with v at one end and the other end in U, for every v in U;
 *   2. v* = the node of U with the largest deg, ties to the smallest index: it becomes a REPRESENTATIVE;
 *   3. every u in U with a counting record {v*, u} becomes a MEMBER of v*; ani[u] = the highest ANI among those records;
 *   4. v* and its new members leave U.
 * Degrees count records -- a pair given twice counts twice; the symmetric output of hg_dist_dev has each pair once, so there
 * deg is the number of undecided neighbours, and a list that holds every pair the same number of times resolves identically.
 * A node of degree 0 is thereby a representative of itself.  A member never covers anybody and never changes representative.
 *   rep[i]      = i for a representative, its representative for a member (which may have a larger index than i);
 *   cluster[i]  = the dense id of rep[i]: 0, 1, ... in increasing order of the representatives' indices;
 *   ani[i]      = 100.0f for a representative, the pair's ANI for a member (optional: may be NULL);
 *   *n_clusters = the number of representatives.
 * The result depends on the multiset of counting records alone -- not on hit order, orientation, block sizes, rounds per
 * readback or scheduling.  n < 2^31 (HG_ERR_UNSUPPORTED beyond); n == 0: HG_OK, *n_clusters = 0; NULL rep / cluster /
 * n_clusters: HG_ERR_INVALID; HG_ANI_CONTAINMENT: HG_ERR_INVALID as for hg_cluster_dev; results are final on return.
 * On the device the rule is resolved in rounds over the live records -- both ends undecided -- (hg_cluster_setcover.hip):
 * setcover_count_kernel, one lane per record, integer atomic adds into deg; setcover_spread_kernel twice, a 64-bit atomic
 * max per record end -- first of key(v) = deg(v) << 32 | (0xFFFFFFFF - v), then of the maxima so found: the largest key
 * within two live hops of every node; setcover_select_kernel, one lane per node -- the strict maximum of its two hops is a
 * representative: the sequential walk chooses it with exactly the cover set it has now, and the nodes chosen in one round
 * are more than two hops apart; setcover_cover_kernel, one lane per record {representative, undecided}, an atomic max of
 * (ani, -representative) into the undecided end; setcover_settle_kernel, one lane per node -- covered: member.  The
 * global maximum is chosen in every round.  The host queues "setcover_rounds" rounds (hg_ctx_set_debug; default 4) per
 * readback of the undecided count and stops at 0.  Dense groups resolve in a few rounds; the worst case, a path
 * 0 - 1 - 2 - ..., takes about n / 3 rounds (accepted).  The dense ids come from hg_cluster_finish_dev's kernels.
 *   hg_cluster_setcover_hits_dev : a complete hit list of the caller, n_hits < 2^32 (HG_ERR_UNSUPPORTED beyond).
 *   hg_cluster_setcover_dev : resident sketches.  UNLIKE hg_cluster_greedy_dev and hg_cluster_tree_dev it cannot resolve a
 *                           row block before it has seen them all -- the rule is global: the first representative is the
 *                           best-covering node of the whole graph.  It runs the symmetric comparison in the row blocks of
 *                           hg_cluster_dev ("pair_limit" as there), APPENDS every block's hits to one scratch list and
 *                           resolves once at the end: the list costs 12 bytes per hit above the threshold.
 *                           "cluster_hit_cap" sets the list's first size; when a block overflows it, the list grows to what
 *                           is needed, the hits of earlier blocks are kept, and the block runs again.  A total of 2^32 - 1
 *                           hits or more: HG_ERR_UNSUPPORTED (the hit list does not fit; a higher threshold would).
 *   hg_cluster_setcover     : host arrays in and out, staged through the ctx. */
hg_status hg_cluster_setcover_hits_dev(hg_ctx *ctx, size_t n, const hg_ani_hit *d_hits, size_t n_hits, float ani_th,
                                       uint32_t *d_rep, uint32_t *d_cluster, float *d_ani, size_t *n_clusters);
hg_status hg_cluster_setcover_dev(hg_ctx *ctx, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d,
                                  uint32_t ksize, float ani_th, uint32_t *d_rep, uint32_t *d_cluster, float *d_ani,
                                  size_t *n_clusters);
hg_status hg_cluster_setcover(hg_ctx *ctx, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                              float ani_th, uint32_t *rep, uint32_t *cluster, float *ani, size_t *n_clusters);
/* rounds of the last set-cover call on this ctx (diagnostic; 0 = none yet) */
uint64_t hg_ctx_cluster_setcover_rounds(const hg_ctx *ctx);

/* The single-linkage tree (no reference counterpart): every threshold of single linkage from ONE comparison.  The
 * maximum-ANI spanning forest of the hit graph at a floor ani_th has at most n - 1 edges -- 12 (n - 1) bytes however many
 * pairs lie above the floor, where the hit list itself can pass 2^32 entries -- and is an exact summary of it:
 *   - cut at any t >= ani_th it gives exactly the components of the full graph at t.  Cutting needs no new call:
 *     hg_cluster_init_dev + hg_cluster_add_hits_dev(d_tree, n_edges, t) + hg_cluster_finish_dev, once per level;
 *   - its edges, strongest first, are the merge order of single-linkage clustering (the dendrogram).
 * Which hits count: ani >= ani_th (the float comparison of hg_dist_dev: NaN never counts) and ref_idx != qry_idx.  A hit is
 * the edge {lo, hi} = {min, max} of its indices: either orientation, duplicates allowed (a pair given with several ANIs has
 * several edges, the strongest decides).  Edge e is STRONGER than f iff ani(e) > ani(f) as floats (-0 = +0), or the ANIs
 * are equal and lo(e) < lo(f), or those are equal too and hi(e) < hi(f); edges equal in all three are the same edge.
 * The tree is what Kruskal builds: the edges strongest first, an edge kept iff it joins two different components.
 *   d_tree      : *n_edges = n - *n_clusters records {ref_idx = lo, qry_idx = hi, ani}, strongest first;
 *   rep, cluster: what hg_cluster_dev gives at ani_th (optional: both NULL for the tree alone); *n_clusters is always set.
 * The result depends on the edge set and its ANI values alone -- not on hit order, block size, rounds per readback or
 * scheduling.  tree_cap < n - 1: HG_ERR_CAPACITY with *n_edges = n - 1, nothing launched.  n == 0: HG_OK, zero counts;
 * n >= 2^31: HG_ERR_UNSUPPORTED; NULL d_tree / n_edges / n_clusters, or one of rep / cluster without the other:
 * HG_ERR_INVALID.  Results are final on return, as for hg_cluster_dev.
 * On the device (hg_cluster_tree.hip) the tree is resolved as Boruvka rounds over a candidate list: tree_best_ani_kernel and
 * tree_best_pair_kernel, one lane per candidate -- the strongest edge leaving each component, by an atomic max of the ANI
 * key and an atomic min of lo << 32 | hi among its ties; tree_select_kernel, one lane per node -- a root emits its edge
 * (once when both ends chose it); tree_hook_kernel and tree_compress_kernel unite the components.  Every live component
 * merges in every round: at most ceil(log2 n) + 1 rounds per block.  The host queues "tree_rounds" rounds (hg_ctx_set_debug;
 * default 4) per readback of the count of selecting roots and stops at 0.
 *   hg_cluster_tree_hits_dev : a complete hit list of the caller; an index >= n (at any ANI): HG_ERR_INVALID, nothing
 *                              reported, the next call starts clean.
 *   hg_cluster_tree_dev      : resident sketches (HG_ANI_MASH or HG_ANI_MAX_CONTAINMENT); the symmetric comparison in the row
 *                              blocks of hg_cluster_dev (scratch list, "pair_limit", "cluster_hit_cap" and its grow path as
 *                              there).  A block's candidates are the forest of the blocks before it and its own hits -- at most
 *                              n - 1 edges + one block's hits are ever held.
 *   hg_cluster_tree          : host arrays in and out, staged through the ctx. */
hg_status hg_cluster_tree_hits_dev(hg_ctx *ctx, size_t n, const hg_ani_hit *d_hits, size_t n_hits, float ani_th,
                                   hg_ani_hit *d_tree, size_t tree_cap, size_t *n_edges, uint32_t *d_rep, uint32_t *d_cluster,
                                   size_t *n_clusters);
hg_status hg_cluster_tree_dev(hg_ctx *ctx, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                              float ani_th, hg_ani_hit *d_tree, size_t tree_cap, size_t *n_edges, uint32_t *d_rep,
                              uint32_t *d_cluster, size_t *n_clusters);
hg_status hg_cluster_tree(hg_ctx *ctx, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                          float ani_th, hg_ani_hit *tree, size_t tree_cap, size_t *n_edges, uint32_t *rep, uint32_t *cluster,
                          size_t *n_clusters);
/* rounds of the last tree call on this ctx, summed over its blocks (diagnostic; 0 = none yet) */
uint64_t hg_ctx_cluster_tree_rounds(const hg_ctx *ctx);

/* Average linkage, UPGMA (no reference counterpart): the hierarchical clustering genome pipelines run on an ANI matrix --
 * dRep's primary clustering, scipy's linkage(method="average").  The pairs below the threshold enter the averages, so the
 * scheme works on the dense matrix, not on a hit list.  Input: n items and ani(i, j) for i < j -- the float
 * hg_dist_full_dev writes at [i, j] (reference i, query j) -- and ani_th.  Everything is decided on integers:
 *   m(i, j)  = the integer `dist` prints for the pair, in thousandths: NaN and negative values 0, values above 100 100,
 *              then rint((double)ani * 1000.0): 0 .. 100 000;
 *   th_milli = the same of ani_th.  A NaN threshold merges nothing, a threshold above 100 merges nothing, ani_th <= 0
 *              merges everything into one cluster;
 *   a cluster is named by its smallest member, c(A) is its size, S(A, B) the sum of m(a, b) over a in A, b in B;
 *   pair {A, B} is BETTER than {C, D} iff S(A,B) c(C) c(D) > S(C,D) c(A) c(B), compared exactly; on equality the pair
 *   with the smaller lower name wins, then the pair with the smaller higher name;
 *   while the best pair has S(A,B) >= th_milli c(A) c(B): merge it.  The merged cluster keeps the smaller name and
 *   S(K, A u B) = S(K,A) + S(K,B).
 * Results: rep[i] = the smallest index of i's cluster, cluster[i] = its dense id in increasing order of rep (the layout of
 * hg_cluster_dev), *n_clusters their number.  The dendrogram, three optional arrays of n entries (each may be NULL): for a
 * name B that was absorbed into A, into[B] = A, level[B] = (float)(((double)S / (double)(c(A) c(B))) / 1000.0) -- two IEEE
 * double divisions and one conversion, nothing contracted --, size[B] = c(A) + c(B) right after the merge; for a name never
 * absorbed into[i] = i, level[i] = 0, size[i] = the final size of its cluster.  The averages along a root path never
 * increase (UPGMA is monotone): sorted by (level descending, size ascending, into, index) the absorbed entries list the
 * merges with every child before its parent.
 * Only integers are added and the comparisons are exact (128-bit cross products): the result depends on the matrix alone
 * -- not on scheduling, block size or the rounds per readback -- and anyone can reproduce it from a `dist -a 0` TSV.
 * On the device (hg_cluster_average.hip) the rule is resolved in rounds on a dense n x n matrix of u64 sums: every pair of
 * mutual best partners merges at once, which is the sequential result because average linkage is reducible.  Per round
 * average_best_kernel (one workgroup per live row: its best partner among the pairs that meet the threshold),
 * average_pair_kernel (one lane per node: mutual pairs merge), average_rows_kernel (row A += row B) and
 * average_cols_kernel (M[R][A] += M[R][B] in every surviving row).  The host queues "average_rounds" rounds
 * (hg_ctx_set_debug; default 4) per readback of the round's merge count and stops at a round that merged nothing.  Groups
 * of near-equal members take some tens of rounds; the worst case, a chain whose neighbour similarities fall with the index,
 * takes O(n) rounds, and is accepted as the greedy resolution's path is.
 * n <= HG_CLUSTER_AVERAGE_MAX_N (the matrix is 34 GB there; 800 MB at 10 000): beyond it HG_ERR_UNSUPPORTED before anything
 * is allocated; a failed allocation is HG_ERR_OOM; the matrix is released before the call returns.  n == 0: HG_OK with
 * *n_clusters = 0.  NULL rep, cluster or n_clusters: HG_ERR_INVALID.  Results are final on return; one clustering at a
 * time per ctx.  Launches count under HG_T_DIST when timing is on.
 *   hg_cluster_average_matrix_dev : d_ani, n x n floats, row-major; only [i, j] with i < j is read.  Independent of the
 *                                   ctx's ANI metric.
 *   hg_cluster_average_dev        : resident sketches (HG_ANI_MASH or HG_ANI_MAX_CONTAINMENT); the matrix is filled from
 *                                   row blocks of hg_dist_full_dev -- rows [r0, r1) x columns [r0, n) in a scratch block of
 *                                   at most HG_SEARCH_BLOCK_BYTES; debug key "average_block_rows" forces the row count.
 *   hg_cluster_average            : host arrays in and out, staged through the ctx. */
#define HG_CLUSTER_AVERAGE_MAX_N 65536u
hg_status hg_cluster_average_matrix_dev(hg_ctx *ctx, const float *d_ani, size_t n, float ani_th, uint32_t *d_rep,
                                        uint32_t *d_cluster, uint32_t *d_into, float *d_level, uint32_t *d_size, size_t *n_clusters);
hg_status hg_cluster_average_dev(hg_ctx *ctx, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                 float ani_th, uint32_t *d_rep, uint32_t *d_cluster, uint32_t *d_into, float *d_level,
                                 uint32_t *d_size, size_t *n_clusters);
hg_status hg_cluster_average(hg_ctx *ctx, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                             float ani_th, uint32_t *rep, uint32_t *cluster, uint32_t *into, float *level, uint32_t *size,
                             size_t *n_clusters);
/* rounds of the last average-linkage call on this ctx, the one that merged nothing included (diagnostic; 0 = none yet) */
uint64_t hg_ctx_cluster_average_rounds(const hg_ctx *ctx);

/* Complete linkage (no reference counterpart): the hierarchical clustering in which EVERY pair inside a cluster is at
 * least the threshold -- dRep's --clusterAlg complete, scipy's linkage(method="complete") on an ANI matrix; what "a species
 * cluster at 95" means when it is meant strictly.  Single linkage chains, the representative schemes bound a member
 * against its representative only, average linkage bounds an average; this scheme bounds the lowest ANI within.  Input as
 * for average linkage: n items, ani(i, j) for i < j, and ani_th.  Everything is decided on integers:
 *   m(i, j)  = the m of average linkage above (hg_avg_milli: NaN and negative values 0, values above 100 100 000, else
 *              rint((double)ani * 1000.0)): it fits 32 bits;
 *   th_milli = the same of ani_th.  A NaN threshold merges nothing, a threshold above 100 merges nothing, ani_th <= 0
 *              merges everything into one cluster, pairs of ANI 0 or NaN included;
 *   a cluster is named by its smallest member, W(A, B) is the minimum of m(a, b) over a in A, b in B;
 *   pair {A, B} is BETTER than {C, D} iff W(A, B) > W(C, D); on equality the pair with the smaller lower name wins, then
 *   the pair with the smaller higher name;
 *   while the best pair has W(A, B) >= th_milli: merge it.  The merged cluster keeps the smaller name and
 *   W(K, A u B) = min(W(K, A), W(K, B)).
 * Results: exactly the outputs of hg_cluster_average*: rep, cluster (dense ids in increasing order of rep), *n_clusters, and
 * the three optional arrays of the dendrogram (each may be NULL).  For a name B that was absorbed into A, into[B] = A,
 * level[B] = (float)((double)W / 1000.0) of its merge, size[B] = the merged size; for a name never absorbed into[i] = i,
 * level[i] = 0, size[i] = the final size of its cluster.  Levels never rise towards the root (a minimum over more pairs is
 * not larger): sorted by (level descending, size ascending, into, index) the absorbed entries list the merges with every
 * child before its parent.
 * Only integer min and compares occur: the result depends on the matrix alone -- not on scheduling, block size or the
 * rounds per readback -- and anyone can reproduce it from a `dist -a 0` TSV.
 * On the device (hg_cluster_complete.hip) the rule is resolved in rounds on a dense matrix of u32 minima, n rows of n
 * rounded up to a multiple of 4: every pair of mutual best partners merges at once, which is the sequential result because
 * complete linkage is reducible.  The tie-break survives a merge: the key of K in row A is (W(A, K), -K); the key of
 * C u D, C < D, is (min(W(A, C), W(A, D)), -C), which is key(C) or strictly smaller in its first component, so a partner
 * that beat both C and D still beats their union; the global best pair is mutual, so every round but the last one merges.
 * complete_fill_kernel quantises the upper triangle, complete_mirror_kernel transposes it; per round complete_best_kernel
 * (one workgroup per live row: its best partner among the pairs with m >= th_milli, as one 64-bit maximum
 * m << 32 | 0xFFFFFFFF - j), complete_pair_kernel (one lane per node: mutual pairs merge), complete_rows_kernel
 * (row A = min(row A, row B)) and complete_cols_kernel (M[R][A] = min(M[R][A], M[R][B]) in every surviving row).
 * Similarities between clusters only ever fall, so from round 2 on complete_best_kernel keeps a live row's partner without
 * a scan when the row has none (it is retired: it never gets one again) or when neither the row nor its partner took part
 * in a merge of the previous round (the partner is still the best); debug key "complete_rescan" = "all" scans every live
 * row every round, with identical results and round counts.  The host queues "complete_rounds" rounds (hg_ctx_set_debug;
 * default 4) per readback of the round's merge count and stops at a round that merged nothing.  The worst case, a chain
 * whose neighbour similarities fall with the index, takes O(n) rounds.
 * n <= HG_CLUSTER_COMPLETE_MAX_N (the matrix is 17 GB there; 400 MB at 10 000): beyond it HG_ERR_UNSUPPORTED before anything
 * is allocated, and the next call starts clean; a failed allocation is HG_ERR_OOM; the matrix is released before the call
 * returns.  n == 0: HG_OK with *n_clusters = 0.  NULL rep, cluster or n_clusters: HG_ERR_INVALID.  Results are final on
 * return; one clustering at a time per ctx.  Launches count under HG_T_DIST when timing is on.
 *   hg_cluster_complete_matrix_dev : d_ani, n x n floats, row-major; only [i, j] with i < j is read.  Independent of the
 *                                    ctx's ANI metric.
 *   hg_cluster_complete_dev        : resident sketches (HG_ANI_MASH or HG_ANI_MAX_CONTAINMENT); the matrix is filled from
 *                                    row blocks of hg_dist_full_dev -- rows [r0, r1) x columns [r0, n) in a scratch block of
 *                                    at most HG_SEARCH_BLOCK_BYTES; debug key "complete_block_rows" forces the row count.
 *   hg_cluster_complete            : host arrays in and out, staged through the ctx. */
#define HG_CLUSTER_COMPLETE_MAX_N 65536u
hg_status hg_cluster_complete_matrix_dev(hg_ctx *ctx, const float *d_ani, size_t n, float ani_th, uint32_t *d_rep,
                                         uint32_t *d_cluster, uint32_t *d_into, float *d_level, uint32_t *d_size, size_t *n_clusters);
hg_status hg_cluster_complete_dev(hg_ctx *ctx, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                  float ani_th, uint32_t *d_rep, uint32_t *d_cluster, uint32_t *d_into, float *d_level,
                                  uint32_t *d_size, size_t *n_clusters);
hg_status hg_cluster_complete(hg_ctx *ctx, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                              float ani_th, uint32_t *rep, uint32_t *cluster, uint32_t *into, float *level, uint32_t *size,
                              size_t *n_clusters);
/* rounds of the last complete-linkage call on this ctx, the one that merged nothing included (diagnostic; 0 = none yet) */
uint64_t hg_ctx_cluster_complete_rounds(const hg_ctx *ctx);

/* Neighbour joining (no reference counterpart): the distance tree people draw from an all-pairs Mash / ANI table --
 * mashtree, `mash triangle | rapidnj`, the dendrogram step of pyani and dRep reports.  UPGMA (hg_cluster_average*) assumes a
 * clock and yields a merge table; neighbour joining does not, and yields an unrooted tree with branch lengths.  Input: n
 * items and ani(i, j) for i < j -- the float hg_dist_full_dev writes at [i, j].  Everything is decided on integers:
 *   m(i, j) = the m of average linkage above (hg_avg_milli: NaN and negative values 0, values above 100 100 000, else
 *             rint((double)ani * 1000.0)): the integer `dist` prints, in thousandths;
 *   d(i, j) = (100 000 - m(i, j)) << HG_NJ_FRAC_BITS, d(i, i) = 0: a fixed-point distance, one unit = 2^-15 thousandths of
 *             an ANI percent.  Every d stays in [0, 100 000 << 15], below 2^32: the matrix is u32;
 *   a node is named by an index; a joined node keeps the smaller of its two children's names; c = the live count, n at first.
 *   While c >= 3:
 *     1. r(i) = the sum of d(i, k) over live k != i (integers: the order of summation is irrelevant);
 *     2. Q(i, j) = (c - 2) d(i, j) - r(i) - r(j) in signed 64 bits (its magnitude is below 2^50 at n = 65 536);
 *     3. the pair to join is the minimum of (Q, i, j) over live i < j, compared lexicographically and exactly: ties go to
 *        the smaller lower name, then to the smaller higher name;
 *     4. for the joined pair a < b and D = d(a, b): len_a = floor(((c - 2) D + r(a) - r(b)) / (2 (c - 2))) -- a floor
 *        towards minus infinity, not a truncation --, len_b = D - len_a.  Either may be negative; neither is clamped;
 *     5. for every live k other than a and b: d(a, k) = d(k, a) = max(0, (d(a, k) + d(b, k) - D) >> 1), an arithmetic
 *        shift (floor).  Then b dies and c becomes c - 1.
 *   At c = 2 the two live names a < b give the last join (a, b, len_a = d(a, b), len_b = 0).
 * Result: joins[0 .. n - 2] in this order, hg_nj_join {a, b, len_a, len_b} (24 bytes), lengths in units of 2^-15
 * thousandths; *n_joins = n - 1 for n >= 2 and 0 for n <= 1.
 * The result depends on the matrix alone -- not on scheduling or block size -- and anyone can reproduce it from a
 * `dist -a 0` TSV.  The floor of step 5 loses at most half a unit per update: over 65 535 nested joins the drift is at most
 * one thousandth of a percent.  The clamp at 0 never acts on an additive (tree) matrix, and an additive matrix whose path
 * lengths are integers in thousandths is recovered exactly: topology and every branch.
 * On the device (hg_nj.hip; the three formulas once, in hg_nj_math.h) the matrix is n rows of n rounded up to a multiple
 * of 4: nj_fill_kernel quantises the upper triangle, nj_mirror_kernel transposes it, nj_rsum_kernel sums the rows.
 * Neighbour joining is not reducible, so there is one join per round: n - 2 rounds and the last join are queued ahead
 * without a readback (c is a launch argument).  Per round nj_best_kernel (one workgroup per live row i: the minimum of
 * (c - 2) d - r(j) over the live columns j > i, ties to the smaller j, from 16-byte loads of the row and of the live marks),
 * nj_pick_kernel (one workgroup: the minimum of (Q, i) over the rows, the join, b dies) and nj_update_kernel (one lane per
 * k: row and column a, r(k), and r(a) by one 64-bit atomic add per workgroup).  Scanning only the columns above the row
 * halves the traffic; the scan still reads about n^3 / 4 words over the whole call, dead columns included.
 * n <= HG_NJ_MAX_N (the matrix is 17 GB there; 400 MB at 10 000): beyond it HG_ERR_UNSUPPORTED before anything is
 * allocated; a failed allocation is HG_ERR_OOM; the matrix is released before the call returns and the ctx is usable
 * afterwards.  n == 0 and n == 1: HG_OK with *n_joins = 0.  NULL joins or n_joins (or inputs): HG_ERR_INVALID.  Results are
 * final on return.  Launches count under HG_T_DIST when timing is on.
 *   hg_nj_matrix_dev : d_ani, n x n floats, row-major; only [i, j] with i < j is read.  Independent of the ctx's ANI metric.
 *   hg_nj_dev        : resident sketches (HG_ANI_MASH or HG_ANI_MAX_CONTAINMENT; the directional metric is HG_ERR_INVALID as
 *                      in clustering); the matrix is filled from row blocks of hg_dist_full_dev -- rows [r0, r1) x columns
 *                      [r0, n) in a scratch block of at most HG_SEARCH_BLOCK_BYTES; debug key "nj_block_rows" forces the
 *                      row count.
 *   hg_nj            : host arrays in and out, staged through the ctx.
 *   hg_nj_newick     : host only, no ctx.  joins[0 .. n - 2] of n >= 1 items and their n names -> the unrooted tree in Newick
 *                      form, a NUL-terminated string in *out (hg_free releases it), its length without the NUL in *len (len
 *                      may be NULL).  Every label is single-quoted, an inner ' doubled.  An inner node is
 *                      (sub(a):len_a,sub(b):len_b), a first.  n = 1: 'name';  n = 2: ('a':L,'b':0.00000000);  n >= 3: the top
 *                      level is a trifurcation of the two children of the second-to-last join and the other side of the last
 *                      join, each with its length, in increasing order of their names (a subtree's name is its smallest leaf
 *                      index).  A length is printed in substitutions per site, 1 - ANI / 100, with eight decimals, by
 *                      integers only: t = (|len| * 1000 + 16384) >> 15, then an optional '-' (only if len < 0 and t != 0),
 *                      t / 10^8, '.', and t % 10^8 zero-padded.  A join list that is not a valid sequence (a >= b, a name
 *                      >= n, a dead name reused), n == 0 or a NULL argument: HG_ERR_INVALID, never a read out of bounds. */
#define HG_NJ_FRAC_BITS 15
#define HG_NJ_MAX_N 65536u
typedef struct {
  uint32_t a, b;        /* the joined names, a < b; the joined node is called a */
  int64_t len_a, len_b; /* their branches to the joined node, in units of 2^-15 thousandths of an ANI percent */
} hg_nj_join;
hg_status hg_nj_matrix_dev(hg_ctx *ctx, const float *d_ani, size_t n, hg_nj_join *d_joins, size_t *n_joins);
hg_status hg_nj_dev(hg_ctx *ctx, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                    hg_nj_join *d_joins, size_t *n_joins);
hg_status hg_nj(hg_ctx *ctx, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                hg_nj_join *joins, size_t *n_joins);
hg_status hg_nj_newick(const hg_nj_join *joins, size_t n, const char *const *names, char **out, size_t *len);

/* Cluster statistics (no reference counterpart): how good a clustering is -- per cluster the medoid, the cohesion (sum and
 * minimum of the within-cluster ANI) and the separation (the nearest item outside), the figures dRep, skDER and galah
 * report or use -- from the dense ANI matrix and a cluster assignment.  Input: n items, ani(i, j) -- the float
 * hg_dist_full_dev writes at [i, j] (reference i, query j) -- and cluster[i] < n_clusters in ANY labelling: it need not come
 * from this library, and ids without members are allowed.  Everything is decided on integers:
 *   m(i, j) = the integer `dist` prints for the pair, in thousandths (the m of average linkage above): NaN and negative
 *             values 0, values above 100 100 000, else rint((double)ani * 1000.0);
 *   the row of i uses row i of the matrix only, the diagonal is never read, and nothing assumes symmetry: an asymmetric
 *   matrix has one defined answer.
 * Per node, hg_node_stat (24 bytes):
 *   within_sum                      the sum of m(i, j) over j != i in i's cluster;
 *   within_min, within_min_idx      the smallest m(i, j) over j != i in i's cluster and the smallest j that attains it;
 *                                   HG_STATS_NONE twice for a singleton;
 *   outside_max, outside_max_idx    the largest m(i, j) over j outside i's cluster and the smallest j that attains it;
 *                                   HG_STATS_NONE twice when there is no item outside.
 * Per cluster id, hg_cluster_stat (48 bytes):
 *   within_sum                      the sum of the members' within_sum: the ordered pairs, size (size - 1) of them;
 *   size, first                     the number of members and the smallest member;
 *   medoid                          the member with the largest within_sum, ties to the smallest index (a singleton is its
 *                                   own medoid);
 *   within_min, _a, _b              the minimum of the members' within_min, the smallest member that attains it and that
 *                                   member's within_min_idx;
 *   outside_max, outside_member,    the maximum of the members' outside_max, the smallest member that attains it and that
 *   outside_idx                     member's outside_max_idx;
 *   reserved                        0.
 * HG_STATS_NONE marks an absent value; an id without members has size = 0, within_sum = 0 and HG_STATS_NONE in every index
 * and value field.  The mean within-cluster ANI of a cluster is (float)(((double)within_sum / (double)(size (size - 1))) /
 * 1000.0).  Only integer add, min and max are used: the result depends on the matrix and the assignment alone -- not on
 * block size, scheduling or the order of atomics.
 * On the device (hg_cluster_stats.hip): cluster_stats_rows_kernel, one workgroup per row of a block of the matrix (16-byte
 * loads, head and tail of a row peeled, a reduction by wave shuffles and LDS); cluster_stats_fold_kernel and
 * cluster_stats_medoid_kernel, one lane per node, 64-bit atomics per cluster id; cluster_stats_emit_kernel, one lane per
 * cluster id.  Memory: 48 bytes per cluster id, 24 per node when d_node is NULL, and in hg_cluster_stats_dev one block of
 * the matrix; no n x n matrix is held.
 * d_node or d_stat may be NULL, not both (HG_ERR_INVALID).  n == 0: HG_OK, the n_clusters records are written as empty.
 * n >= 2^31: HG_ERR_UNSUPPORTED.  NULL cluster (n > 0): HG_ERR_INVALID.  A cluster[i] >= n_clusters fails the call with
 * HG_ERR_INVALID -- it indexes nothing, and the next call on the ctx starts clean.  Results are final on return.  Launches
 * count under HG_T_DIST when timing is on.
 *   hg_cluster_stats_matrix_dev : d_ani, n x n floats, row-major.  Independent of the ctx's ANI metric.
 *   hg_cluster_stats_dev        : resident sketches (HG_ANI_MASH or HG_ANI_MAX_CONTAINMENT); the matrix is streamed as rows
 *                                 [r0, r1) x all n columns from hg_dist_full_dev in a scratch block of at most
 *                                 HG_SEARCH_BLOCK_BYTES; debug key "stats_block_rows" forces the row count.
 *   hg_cluster_stats            : host arrays in and out, staged through the ctx. */
#define HG_STATS_NONE 0xFFFFFFFFu
typedef struct {
  uint64_t within_sum;
  uint32_t within_min, within_min_idx;
  uint32_t outside_max, outside_max_idx;
} hg_node_stat;
typedef struct {
  uint64_t within_sum;
  uint32_t size, first, medoid;
  uint32_t within_min, within_min_a, within_min_b;
  uint32_t outside_max, outside_member, outside_idx;
  uint32_t reserved;
} hg_cluster_stat;
hg_status hg_cluster_stats_matrix_dev(hg_ctx *ctx, const float *d_ani, size_t n, const uint32_t *d_cluster, size_t n_clusters,
                                      hg_node_stat *d_node, hg_cluster_stat *d_stat);
hg_status hg_cluster_stats_dev(hg_ctx *ctx, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                               const uint32_t *d_cluster, size_t n_clusters, hg_node_stat *d_node, hg_cluster_stat *d_stat);
hg_status hg_cluster_stats(hg_ctx *ctx, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                           const uint32_t *cluster, size_t n_clusters, hg_node_stat *node, hg_cluster_stat *stat);

/* ---- sketch compression (host side; src/hd.rs:114-232) -------------------------------- */
uint32_t hg_hv_quant_bits(const int16_t *hv, uint32_t hv_d);
/* packed holds hg_hv_packed_bytes(hv_d, quant_bits) = quant_bits * (hv_d >> 3) bytes (src/hd.rs:146).  Like the
 * reference, only whole blocks of 256 dimensions are packed (src/hd.rs:147): for hv_d % 256 != 0 the bytes behind
 * them are zero and hg_hv_unpack gives every dimension behind the last whole block the value -2^(quant_bits-1)
 * (src/hd.rs:194,206-212) -- the round trip is lossless only for multiples of 256.  quant_bits = 16 reproduces the
 * reference's sign-extension spill (src/hd.rs:140-141) bit for bit. */
size_t hg_hv_packed_bytes(uint32_t hv_d, uint32_t quant_bits);
hg_status hg_hv_pack(const int16_t *hv, uint32_t hv_d, uint32_t quant_bits, uint8_t *packed);
hg_status hg_hv_unpack(const uint8_t *packed, uint32_t hv_d, uint32_t quant_bits, int16_t *hv);
/* The OTHER payload layout: what the reference writes and reads on a host WITHOUT AVX2 (src/hd.rs:158-166, 213-231).
 * (quant_bits * hv_d + 16) / 16 int16 words -- always one word more than the bits need when that product is a multiple
 * of 16 -- holding the low quant_bits bits of every value LSB first, NO offset added.  Decoding follows the reference
 * to the letter: `if v > (1 << (q-1)) { v - (1 << q) }` in i16 -- strictly greater, so -2^(q-1) (low bits 100..0) comes
 * back as +2^(q-1), and at quant_bits = 16 (`1 << 15` = -32768, `1 << 16` wraps to 1) every value but -32768 comes back
 * one lower: the reference's naive round trip is lossy exactly there, and so is this one.
 * The two layouts never have the same payload length (the naive one is longer by at least one word), which is how
 * hg_hv_payload_layout -- and through it `hyper-gen dist` / `search` -- tells them apart: HG_PAYLOAD_BITPACKER8X,
 * HG_PAYLOAD_NAIVE, or -1 for a length that is neither.  `hyper-gen sketch` writes the naive layout only behind
 * `--pack_layout naive` (an extension flag; the default is what the reference writes on every AVX2 host). */
enum { HG_PAYLOAD_BITPACKER8X = 0, HG_PAYLOAD_NAIVE = 1 };
size_t hg_hv_packed_bytes_naive(uint32_t hv_d, uint32_t quant_bits);
hg_status hg_hv_pack_naive(const int16_t *hv, uint32_t hv_d, uint32_t quant_bits, uint8_t *packed);
hg_status hg_hv_unpack_naive(const uint8_t *packed, uint32_t hv_d, uint32_t quant_bits, int16_t *hv);
int hg_hv_payload_layout(uint32_t hv_d, uint32_t quant_bits, size_t payload_bytes);
/* decompress_file_sketch (src/hd.rs:171-180: one rayon task per sketch) on the device: n payloads, payload i at
 * d_payloads + offsets[i] (byte offsets of any alignment into a device buffer of payloads_bytes bytes -- e.g. the image of
 * a .sketch file, see hg_sketch_file_payload_offset; host array) in layout layouts[i] with quant_bits[i] (host arrays;
 * layouts == NULL: all BitPacker8x), decoded to row i of the n x hv_d int16 matrix d_hv -- the same integers as
 * hg_hv_unpack / hg_hv_unpack_naive, rows and dimensions behind the last whole block included.  The payloads are 4.6 KB
 * per sketch at quant_bits = 9 against 8 KB of int16: `hyper-gen dist` uploads the file's payload bytes as they are and
 * decodes them here instead of unpacking on host threads and uploading the matrix.  Stream-ordered; the host arrays are
 * consumed before the call returns.  (hg_hv_unpack_kernel) */
hg_status hg_hv_unpack_batch_dev(hg_ctx *ctx, const uint8_t *d_payloads, size_t payloads_bytes, const uint64_t *offsets,
                                 const uint8_t *quant_bits, const uint8_t *layouts, size_t n, uint32_t hv_d, int16_t *d_hv);

/* ---- .sketch files (host side; src/types.rs:224-235, src/utils.rs:234-258) ------------ */
typedef struct {
  uint8_t ksize;
  uint8_t canonical;
  uint8_t hv_quant_bits;
  uint8_t pad;
  int32_t hv_norm_2;
  uint64_t scaled;
  uint64_t seed;
  uint64_t hv_d;
  const char *file_str; /* UTF-8, NUL terminated                                      */
  const int16_t *hv;    /* payload exactly as stored (packed when hv_quant_bits < 16) */
  uint64_t hv_len;      /* number of int16 in the payload                             */
} hg_file_sketch;

typedef struct hg_sketch_file hg_sketch_file; /* owns the records of a loaded file */

hg_status hg_sketch_file_write(const char *path, const hg_file_sketch *recs, size_t n);
hg_status hg_sketch_file_read(const char *path, hg_sketch_file **out);
/* The same parse without the payload copies: the records' `hv` are NULL (hv_len is set), the file's bytes stay in one
 * buffer (hg_sketch_file_image) and record i's payload starts at hg_sketch_file_payload_offset(f, i) in it -- upload the
 * image once and decode on the device with hg_hv_unpack_batch_dev (what `hyper-gen dist` / `search` do). */
hg_status hg_sketch_file_read_image(const char *path, hg_sketch_file **out);
const uint8_t *hg_sketch_file_image(const hg_sketch_file *f, size_t *bytes);
uint64_t hg_sketch_file_payload_offset(const hg_sketch_file *f, size_t i);
size_t hg_sketch_file_count(const hg_sketch_file *f);
const hg_file_sketch *hg_sketch_file_get(const hg_sketch_file *f, size_t i);
void hg_sketch_file_free(hg_sketch_file *f);

/* ---- continuous host-fed sketching ------------------------------------------------------------------------
 * The streaming form of hg_sketch_batch for hosts that produce genomes one at a time (reader threads walking a
 * file list, src/sketch_cuda.rs:120-166): one uploader and one compute thread per device keep the PCIe link and the
 * kernels busy without the caller collecting batches.  Results are bit-identical to hg_sketch_batch.
 *   open    one engine per entry of device_ids (an id may repeat); params are fixed for the stream's lifetime
 *   push    any thread; `seq` must stay valid and unchanged until the genome's result has been popped; page-locked
 *           memory (hg_read_fastx_pinned) is fetched by DMA at the link rate, other memory is staged by the runtime;
 *           BLOCKS while hg_sketch_stream_max_pending (4096) results are outstanding -- back-pressure for reader
 *           threads; a caller that pushes and pops on ONE thread must use hg_sketch_stream_try_push instead, which
 *           returns HG_ERR_CAPACITY ("would block": pop some results first) and never waits
 *   pop     any thread; blocks until a result is ready (completion order, identified by `tag`); *got = 0 with
 *           HG_OK once hg_sketch_stream_finish was called and every pushed genome has been popped; hv_out holds
 *           hv_d int16, any output pointer may be NULL
 *   finish  no more pushes; partial chunks are flushed
 *   close   joins the threads and frees everything (outstanding results are dropped)
 * After a failure every call returns its status; hg_sketch_stream_last_error has the text. */
typedef struct hg_sketch_stream hg_sketch_stream;
hg_status hg_sketch_stream_open(const int *device_ids, int n_devices, const hg_sketch_params *p, hg_sketch_stream **out);
hg_status hg_sketch_stream_push(hg_sketch_stream *s, const uint8_t *seq, size_t n_bps, uint64_t tag);
/* the same genome as a hg_pack2 blob (3 bits per base over the link instead of 8; the chunk's blobs go to the
 * packed-input kernels as they arrive, hg_sketch_batch_dev_packed: results are bit-identical).  The blob must have been
 * packed with the stream's norm_mode. */
hg_status hg_sketch_stream_push_packed(hg_sketch_stream *s, const uint8_t *blob, size_t n_bps, uint64_t tag);
/* ... or as a hg_pack2s blob: the codes plus a TABLE of the not-a-base runs instead of the bitmap -- 0.25 bytes per base
 * over the link for an ordinary assembly; the device rebuilds the bitmap.  Results are bit-identical.  blob_bytes = the
 * size of the caller's buffer: the run count is read and hg_pack2s_size(n_bps, n_runs) bytes are uploaded only if they lie
 * inside it, and a table whose runs are not ascending, disjoint, non-empty and inside the sequence is refused
 * (HG_ERR_INVALID) before anything reaches the device. */
hg_status hg_sketch_stream_push_packed_sparse(hg_sketch_stream *s, const uint8_t *blob, size_t blob_bytes, size_t n_bps, uint64_t tag);
/* non-blocking push of any form (packed: 0 = ASCII, 1 = `data` is a hg_pack2 blob, 2 = a hg_pack2s blob -- its run table
 * is validated like above, the buffer's size is the caller's word); HG_ERR_CAPACITY = would block */
hg_status hg_sketch_stream_try_push(hg_sketch_stream *s, const uint8_t *data, size_t n_bps, uint64_t tag, int packed);
size_t hg_sketch_stream_max_pending(const hg_sketch_stream *s);
hg_status hg_sketch_stream_pop(hg_sketch_stream *s, uint64_t *tag, int16_t *hv_out, int32_t *norm2_out,
                               uint32_t *nhash_out, int *got);
hg_status hg_sketch_stream_finish(hg_sketch_stream *s);
const char *hg_sketch_stream_last_error(hg_sketch_stream *s);
/* diagnostics of one engine, seconds since open: out[0] uploader waiting for input, [1] uploader waiting for a free
 * chunk (the kernels lag), [2] uploader inside the copy calls, [3] compute thread waiting for a chunk, [4] compute
 * thread from "chunk taken" to "results queued" (includes waiting for the chunk's upload); out[5] = chunks so far */
hg_status hg_sketch_stream_stats(hg_sketch_stream *s, int engine, double out[6]);
void hg_sketch_stream_close(hg_sketch_stream *s);

/* ---- 2-bit packing for the PCIe link (optional) ----------------------------------------------------
 * hg_pack2 writes hg_pack2_size(n_bps) bytes: 2-bit codes (A,C,G,T = 0..3, 4 bases per byte, LSB first) padded to
 * 16 bytes, then a not-a-base bit per position padded to 16 bytes.  Bases are what the kernels accept under
 * `norm_mode` (ACGTacgt, plus Uu -> T under HG_NORM_U2T).  `out` may equal `seq` when the buffer holds
 * max(n_bps, hg_pack2_size(n_bps)) bytes.  hg_unpack2_dev is the device inverse ('A','C','G','T' / 'N'; 16-byte
 * aligned device pointers, d_seq_out with room for n_bps rounded up to 16), in stream order on the ctx's stream. */
size_t hg_pack2_size(size_t n_bps);
hg_status hg_pack2(const uint8_t *seq, size_t n_bps, uint32_t norm_mode, uint8_t *out);
hg_status hg_unpack2_dev(hg_ctx *ctx, const uint8_t *d_blob, size_t n_bps, uint8_t *d_seq_out);
/* The sparse form for the link: [codes as in hg_pack2, padded to 16 bytes][uint32 n_runs, uint32 0, n_runs x {uint32 first
 * position, uint32 length} of the maximal runs of not-a-base positions, ascending, padded to 16 bytes].  hg_pack2s
 * writes hg_pack2s_size(n_bps, n_runs) bytes to `out` (*size_out) if they fit `cap`; HG_ERR_CAPACITY (*size_out = needed)
 * if not -- a sequence littered with non-bases is better served by hg_pack2 --, HG_ERR_UNSUPPORTED for n_bps >= 2^32.
 * `out` may equal `seq` (cap >= the blob). */
size_t hg_pack2s_size(size_t n_bps, size_t n_runs);
hg_status hg_pack2s(const uint8_t *seq, size_t n_bps, uint32_t norm_mode, uint8_t *out, size_t cap, size_t *size_out);
/* hg_pack2 on the device, byte for byte the host's output: ASCII genomes already in HBM (d_seq + offsets[i], multiples
 * of 4, lens[i] bases) become blobs at d_blobs + blob_offsets[i] (multiples of 16, hg_pack2_size(lens[i]) bytes each) --
 * the input form of hg_sketch_batch_dev_packed.  Host offset arrays, device data; complete on return.
 * hg_pack2_dev: one genome (d_seq 4-byte, d_blob 16-byte aligned). */
hg_status hg_pack2_batch_dev(hg_ctx *ctx, const uint8_t *d_seq, const uint64_t *offsets, const uint64_t *lens, size_t n,
                             uint32_t norm_mode, uint8_t *d_blobs, const uint64_t *blob_offsets);
hg_status hg_pack2_dev(hg_ctx *ctx, const uint8_t *d_seq, size_t n_bps, uint32_t norm_mode, uint8_t *d_blob);

/* ---- FASTA ingest (host side; src/fastx_reader.rs:6-29) ------------------------------- */
/* read_merge_seq: returns a malloc'ed buffer (free with hg_free) and its length */
hg_status hg_read_merge_seq(const char *path, uint8_t **out, size_t *n_bps);
/* same, into a caller-owned growable buffer: *buf (NULL or from malloc/realloc) of *cap bytes is reused when
 * large enough and realloc'ed otherwise -- a reader thread that recycles its buffers avoids one 5 MB
 * mmap / page-fault / munmap cycle per file */
hg_status hg_read_merge_seq_into(const char *path, uint8_t **buf, size_t *cap, size_t *n_bps);
/* mode HG_READ_MERGE: exactly read_merge_seq (every line that does not start with '>' is sequence).
 * mode HG_READ_NEEDLETAIL: what the reference's CPU path sees through needletail 0.5.1 (src/sketch.rs:76-87):
 * FASTA or FASTQ chosen by the first byte ('>' / '@'), four-line FASTQ records (only the sequence line is kept),
 * blanks, tabs and CRs inside sequence lines dropped (`normalize`); still one 'N' per record start.  Both modes
 * inflate gzip input transparently. */
#define HG_READ_MERGE 0u
#define HG_READ_NEEDLETAIL 1u
/* OR-ed into the mode: the buffer comes back as the hg_pack2 blob of the merged sequence (*n_bps = its bases),
 * packed for HG_NORM_ACGT, or for HG_NORM_U2T with HG_READ_PACK2_U2T as well -- for hg_sketch_stream_push_packed */
#define HG_READ_PACK2 16u
#define HG_READ_PACK2_U2T 32u
hg_status hg_read_fastx_into(const char *path, uint32_t mode, uint8_t **buf, size_t *cap, size_t *n_bps);
/* same, but the buffer is page-locked host memory owned by the library (hipHostMalloc, visible to every device;
 * *buf NULL or from an earlier call, release with hg_pinned_free): hg_sketch_batch uploads such sequences by DMA at
 * the PCIe rate, while malloc'ed memory goes through the runtime's bounce buffer at a fraction of it.  Needs a HIP
 * device like every compute entry point. */
hg_status hg_read_fastx_pinned(const char *path, uint32_t mode, uint8_t **buf, size_t *cap, size_t *n_bps);
void hg_pinned_free(void *p);
/* The order in which a dist / Hamming launch with tiles_m x tiles_n tiles of tile_rows x tile_cols walks its tiles (host
 * code only, no device needed; for inspection and for the tests): workgroup slot b runs tile out[b] = tm | tn << 16, or
 * no tile where out[b] == 0xFFFFFFFF.  The hardware deals slot b to XCD b % 8, so the slots b = x, x + 8, ... are XCD
 * x's queue: every tile that has work (with `symmetric`: not entirely on or below the diagonal of the global
 * enumeration, row 0 = ref_off, column 0 = qry_off) exactly once; the XCDs' tile counts differ by at most one; each
 * queue walks 8 x 8 super-tiles in halves of 4 x 8 tiles (the tiles resident on an XCD share 4 + 8 operand blocks through
 * its L2); with diagonal_first the tiles that straddle the diagonal (a database compared with itself has its hits
 * there) lead the queues.  *n_slots = the launch's grid size; HG_ERR_CAPACITY (with *n_slots set) if cap is too small. */
hg_status hg_dist_tile_order(uint32_t tiles_m, uint32_t tiles_n, uint32_t tile_rows, uint32_t tile_cols, int diagonal_first,
                             int symmetric, uint64_t ref_off, uint64_t qry_off, uint32_t *out, size_t cap, size_t *n_slots);
/* NUMA node of a device (-1 unknown): host threads that fill page-locked buffers for it should run there */
int hg_device_numa_node(int device_id);
/* Restricts the CALLING thread to the CPUs of a NUMA node (the ones it may already run on), unless the node has fewer of
 * them than `threads_sharing` (never oversubscribe a node).  Returns 1 when the thread was bound, 0 otherwise (unknown
 * node, nothing readable under /sys, too few CPUs).  Page-locked memory from the HIP runtime lies on the DEVICE's node
 * wherever the allocating thread ran: host threads that read or write such buffers -- the readers of the CLI, the
 * threads of a one-call-per-genome pool, which 2-bit pack into the context's staging buffer -- run ~1.5x faster there
 * than on the other socket (measured: 76-86 against 52-58 GB/s of packing reads, 16 threads). */
int hg_bind_thread_to_numa_node(int node, unsigned threads_sharing);
void hg_free(void *p);

/* ---- bit-packed hypervectors + Hamming search (extension: BASELINE.json configs[4]) ------------
 * No reference counterpart exists (the reference's `search` is an empty stub, src/main.rs:22-24);
 * the semantics are defined here (and restated on the CPU by the test oracle): bit d = (hv[d] >= 0), uint32 word w holds
 * dims 32w..32w+31 LSB first ((hv_d+31)/32 words per vector), distance = popcount(xor).
 * All pointers are device pointers; hv_d must be a multiple of 128 for the search. */
typedef struct {
  uint32_t ref_idx;
  uint32_t qry_idx;
  uint32_t dist;
} hg_ham_hit;
hg_status hg_hv_binarize_dev(hg_ctx *ctx, const int16_t *d_hv, size_t n, uint32_t hv_d, uint32_t *d_bits);
hg_status hg_hamming_full_dev(hg_ctx *ctx, const uint32_t *d_ref_bits, size_t R, const uint32_t *d_qry_bits,
                              size_t Q, uint32_t hv_d, uint32_t *d_dist_out);
/* all pairs with distance <= max_dist, in no particular order; *n_out = found (HG_ERR_CAPACITY if > cap) */
hg_status hg_hamming_search_dev(hg_ctx *ctx, const uint32_t *d_ref_bits, size_t R, const uint32_t *d_qry_bits,
                                size_t Q, uint32_t hv_d, uint32_t max_dist, hg_ham_hit *d_out, size_t cap,
                                size_t *n_out);

/* Searches of 2^24 pairs or more, and every hv_d that is not a multiple of 128, run as an exact GEMM on the matrix pipe
 * with the bits expanded to +-1.0 e2m1 nibbles (G = D - 2 * distance on v_mfma_scale_f32_16x16x128_f8f6f4 with unit
 * block scales; the ANI kernel's tiles and hit lists), smaller ones on the xor + popcount kernel; the +-1 BYTE GEMM
 * (v_mfma_i32_16x16x64_i8) stays reachable through the "ham_path" = "mfma" hook.  All three give the same integers.
 * hg_ctx_last_hamming_path: 0 = xor + popcount, 1 = byte GEMM, 2 = e2m1 (FP4) GEMM (the default for large searches);
 * -1 = none yet. */
int hg_ctx_last_hamming_path(const hg_ctx *ctx);
/* one shard of a sharded reference database: hits carry ref_off + local row, qry_off + local column */
hg_status hg_hamming_search_block_dev(hg_ctx *ctx, const uint32_t *d_ref_bits, size_t R, size_t ref_off,
                                      const uint32_t *d_qry_bits, size_t Q, size_t qry_off, uint32_t hv_d,
                                      uint32_t max_dist, hg_ham_hit *d_out, size_t cap, size_t *n_out);

/* ---- several GPUs in one process -------------------------------------------------------------------
 * The reference drives one CudaDevice::new(0) from all rayon workers (src/sketch_cuda.rs:52,82).  hg_multi
 * owns one hg_ctx per entry of device_ids (1..8 GPUs of one node; ids may repeat -- two logical shards on one
 * GPU, which is how a single-GPU box tests the sharded path) and one host thread per shard for the duration
 * of each call.  Partitioning follows SURVEY.md 8(e):
 *   sketch : genomes are independent units -> contiguous genome blocks per shard, no exchange;
 *   dist   : every shard needs ALL reference HVs -> the shards' row blocks are all-gathered device to
 *            device (hipMemcpyPeerAsync: every GPU pulls its 7 peers' blocks over its 7 xGMI links at
 *            once), then shard s computes the block (all refs) x (its query rows); hits are merged on
 *            the host with global indices;
 *   search : the bit-packed reference database is sharded by rows, the (small) query set is broadcast,
 *            per-shard hits are merged on the host.
 * Results equal the single-ctx calls (same kernels, same arithmetic); hit order is unspecified. */
typedef struct hg_multi hg_multi;
hg_status hg_multi_create(const int *device_ids, int n, hg_multi **out);
void hg_multi_destroy(hg_multi *m);
int hg_multi_size(const hg_multi *m);
hg_ctx *hg_multi_ctx(hg_multi *m, int shard); /* borrowed: valid until hg_multi_destroy */
const char *hg_multi_last_error(const hg_multi *m);
/* what hipDeviceEnablePeerAccess said when the shards were opened ("peer access enabled for 56 of 56 ordered device
 * pairs", or the pairs that fall back to host-staged copies and why) */
const char *hg_multi_peer_report(const hg_multi *m);
/* The exchange step of dist (the reference has none: src/dist.rs:231-294 runs on one host).
 *   HG_GATHER_PEER (default): direct hipMemcpyPeerAsync pulls, one per peer block;
 *   HG_GATHER_RCCL          : ncclAllGather (equal row blocks) / grouped ncclBroadcast per owner over one RCCL
 *                             communicator per shard (ncclCommInitAll).  Needs distinct device ids; librccl is opened
 *                             with dlopen at this call (HG_ERR_UNSUPPORTED if it is absent).
 * Both give the same gathered matrix, hence the same hits.  hg_multi_gather_report: how the last exchange ran. */
enum { HG_GATHER_PEER = 0, HG_GATHER_RCCL = 1 };
hg_status hg_multi_set_gather(hg_multi *m, int mode);
/* hg_ctx_set_ani_metric on every shard's ctx (see there): the metric of hg_dist_multi{,_dev} */
hg_status hg_multi_set_ani_metric(hg_multi *m, int metric);
int hg_multi_gather_mode(const hg_multi *m);
const char *hg_multi_gather_report(const hg_multi *m);
/* contiguous block [*lo, *hi) of n units owned by `shard` of n_shards; sizes differ by at most one */
void hg_shard_range(size_t n, int shard, int n_shards, size_t *lo, size_t *hi);

/* hg_sketch_batch over all shards: genome g goes to the shard whose hg_shard_range contains g */
hg_status hg_sketch_batch_multi(hg_multi *m, const uint8_t *const *seqs, const size_t *lens, size_t n,
                                const hg_sketch_params *p, int16_t *hv_out, int32_t *norm2_out,
                                uint32_t *nhash_out);
/* hg_dist over all shards, host buffers in and out.  Each reference row crosses PCIe once (to its shard's
 * GPU) and is replicated over xGMI; query rows go to their shard only.  qry_hv == ref_hv with Q == R is the
 * all-vs-all case: every GPU then holds every row, and with `symmetric` the column ranges are balanced by
 * pair count (boundaries at Q * sqrt(s / n)) instead of by row count. */
hg_status hg_dist_multi(hg_multi *m, const int16_t *ref_hv, const int32_t *ref_norm2, size_t R,
                        const int16_t *qry_hv, const int32_t *qry_norm2, size_t Q, uint32_t hv_d,
                        uint32_t ksize, int symmetric, float ani_th, hg_ani_hit *out, size_t cap,
                        size_t *n_out);
/* the same for sketches that are already resident: shard s holds ref_rows[s] consecutive reference rows at
 * d_ref_hv[s] / d_ref_norm2[s] on ITS device (e.g. the output of hg_sketch_batch_dev on hg_multi_ctx(m, s)),
 * global row order = shard order.  d_qry_hv == NULL: the query set is the reference set (all-vs-all). */
hg_status hg_dist_multi_dev(hg_multi *m, const int16_t *const *d_ref_hv, const int32_t *const *d_ref_norm2,
                            const size_t *ref_rows, const int16_t *const *d_qry_hv,
                            const int32_t *const *d_qry_norm2, const size_t *qry_rows, uint32_t hv_d,
                            uint32_t ksize, int symmetric, float ani_th, hg_ani_hit *out, size_t cap,
                            size_t *n_out);
/* bit-packed database search (host buffers): ref_bits is R x words, qry_bits Q x words, words = hv_d / 32 */
hg_status hg_hamming_search_multi(hg_multi *m, const uint32_t *ref_bits, size_t R, const uint32_t *qry_bits,
                                  size_t Q, uint32_t hv_d, uint32_t max_dist, hg_ham_hit *out, size_t cap,
                                  size_t *n_out);

/* hg_search_topk_dev over all shards (see "search: exact top-k per query" above); out: Q * k hg_ani_hit and counts: Q uint32
 * of HOST memory.  The metric is the shards' (hg_multi_set_ani_metric). */
hg_status hg_search_topk_multi_dev(hg_multi *m, const int16_t *const *d_ref_hv, const int32_t *const *d_ref_norm2,
                                   const size_t *ref_rows, const int16_t *const *d_qry_hv, const int32_t *const *d_qry_norm2,
                                   size_t Q, uint32_t hv_d, uint32_t ksize, float ani_th, uint32_t k, hg_ani_hit *out,
                                   uint32_t *counts);

/* ---- synthetic genomes (benchmark / test utility, not part of the reference surface) -----
 * Genome g = first_genome + i is written at d_out + i * stride as 'N' followed by L bases
 * (the read_merge_seq layout of a one-record FASTA).  Cluster c = g / cluster_size is an iid
 * uniform ACGT root; member m = g % cluster_size has iid substitutions at rate
 * m * sub_ppm_per_member / 1e6.  stride >= L + 1; n <= 65535 per call. */
hg_status hg_synth_genomes_dev(hg_ctx *ctx, uint64_t first_genome, size_t n, uint64_t L,
                               uint32_t cluster_size, uint32_t sub_ppm_per_member, uint64_t stride,
                               uint8_t *d_out);

#ifdef __cplusplus
}
#endif
#endif /* HYPERGEN_H */
