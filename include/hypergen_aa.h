/*
 * hypergen_aa.h -- C ABI of libhypergen_aa.so: amino-acid k-mer sketches (AAI) on the MI355X (gfx950).
 *
 * The companion of libhypergen_hip.so (hypergen.h) for protein input.  It holds the one kernel the nucleotide library has no
 * counterpart of -- k-mer hash + FracMinHash sample over the 20-letter alphabet, one strand -- and drives the other
 * library's plan, hit regions, sort / unique kernels, encoders and norm for everything behind it: a protein sketch is a set
 * of 64-bit hashes with a ksize like any other, so the .sketch container, hg_dist*, hg_search* and hg_cluster* take it as
 * it is and their ANI formula reads as AAI.  (Mash -a, sourmash protein and Dashing 2 --protein are the same idea.)
 *
 * Semantics (there is no counterpart in the reference, this is the specification)
 *   - a residue is one of ACDEFGHIKLMNPQRSTVWY in either case; every other byte value is not a residue (B J O U X Z * - .,
 *     digits, blanks, bytes >= 128).  N is a residue (asparagine), unlike on the nucleotide path;
 *   - a k-mer is k consecutive residues, 1 <= k <= 32; a window that holds a non-residue yields nothing; no reverse
 *     complement, no canonical choice;
 *   - hash = t1ha2_atonce(the k bytes upper-cased, seed), what src/sketch.rs:90 computes for those bytes; a k-mer is kept
 *     iff hash < threshold, threshold = UINT64_MAX / scaled (src/sketch.rs:73); hash value 0 is kept;
 *   - output: the distinct kept hashes, ascending; the HV is hg_hv_encode's row for that set, norm2 and nhash as on the
 *     nucleotide path.
 * The contexts are hypergen.h's (hg_ctx_create); the conventions and statuses too.  Link both libraries.
 */
#ifndef HYPERGEN_AA_H
#define HYPERGEN_AA_H

#include "hypergen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The distinct sampled hashes of one residue sequence (host memory), ascending: the twin of hg_kmer_hash_sample, with the
 * threshold itself.  If more than `cap` distinct hashes exist: HG_ERR_CAPACITY and *n_out = count.  ksize > 32:
 * HG_ERR_UNSUPPORTED. */
hg_status hg_aa_hash_sample(hg_ctx *ctx, const uint8_t *seq, size_t n, uint32_t ksize, uint64_t threshold, uint64_t seed,
                            uint64_t *out_hashes, size_t cap, size_t *n_out);

/* Whole-batch sketch of n proteomes in device memory: the buffer rules of hg_sketch_batch_dev (proteome i occupies
 * [offsets[i], offsets[i] + lens[i]) of d_seq, offsets multiples of 4, 32 readable bytes behind every proteome; d_hv n * hv_d
 * int16, d_norm2 n int32, d_nhash n uint32, all device).  The results are final in stream order when the call returns: it
 * never takes the deferred step, and it first resolves a deferred nucleotide step pending on the ctx, as every call on a ctx
 * does.  p->canonical is ignored; p->norm_mode must be 0 (HG_ERR_INVALID otherwise); p->min_count > 1 and p->ksize > 32 are
 * HG_ERR_UNSUPPORTED. */
hg_status hg_aa_sketch_batch_dev(hg_ctx *ctx, const uint8_t *d_seq, const uint64_t *offsets, const uint64_t *lens, size_t n,
                                 const hg_sketch_params *p, int16_t *d_hv, int32_t *d_norm2, uint32_t *d_nhash);
/* host buffers in, host results out: one upload, hg_aa_sketch_batch_dev, one download (nothing is packed) */
hg_status hg_aa_sketch_batch(hg_ctx *ctx, const uint8_t *const *seqs, const size_t *lens, size_t n, const hg_sketch_params *p,
                             int16_t *hv_out, int32_t *norm2_out, uint32_t *nhash_out);

/* A protein FASTA file (plain or gzip) as one proteome: the sequence bytes of all records with line ends, blanks, tabs and
 * CRs dropped, one '*' byte at every record start, so that no window spans two records.  *buf / *cap: NULL / 0 or a malloc'ed
 * buffer from an earlier call, grown when it is too small, as hg_read_fastx_into does; release with hg_free.  Needs no GPU. */
hg_status hg_aa_read_fasta(const char *path, uint8_t **buf, size_t *cap, size_t *n);

/* Name of the kernel that hashes k-mers of this length, as rocprofv3 and hg_ctx_last_kernel(ctx, HG_T_KMER) spell it
 * ("" for a ksize outside 1..32).  The string lives as long as the library. */
const char *hg_aa_kernel_name(uint32_t ksize);
/* Geometry of that kernel, for callers that size batches and for tests: k-mer starts one workgroup stages per tile, and
 * starts per work item (the plan's, shared with the nucleotide kernels). */
uint32_t hg_aa_tile_starts(void);
uint32_t hg_aa_item_starts(uint32_t ksize);

#ifdef __cplusplus
}
#endif
#endif
