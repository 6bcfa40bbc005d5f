/*
 * hypergen_tx.h -- C ABI of libhypergen_tx.so: six-frame translated protein sketches from DNA on the MI355X (gfx950).
 *
 * The second companion of libhypergen_hip.so (hypergen.h), beside libhypergen_aa.so (hypergen_aa.h).  It sketches the
 * amino-acid k-mers of all six reading frames of nucleotide input, so AAI needs no gene caller in front of it (sourmash
 * `sketch translate` is the same idea).  It holds one kernel -- codon lookup on both strands, k-mer hash + FracMinHash sample
 * over residues gathered at stride 3 -- and drives the other library's plan, hit regions, sort / unique kernels, encoders and
 * norm for everything behind it.  A translated sketch hashes the bytes a protein sketch hashes: the k-mers of a genome's real
 * proteins are a subset of its six-frame k-mers, so the containment of an hg_aa_* sketch in an hg_tx_* sketch says whether
 * those proteins are encoded in that assembly.
 *
 * Semantics (there is no counterpart in the reference, this is the specification)
 *   - a base is one of ACGT in either case; every other byte is not a base (N, IUPAC codes, U, blanks, bytes >= 128);
 *   - codons translate by the standard genetic code (NCBI table 1): with bases ordered T, C, A, G and index
 *     16 b1 + 4 b2 + b3 the residues are FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG, '*' a stop; a codon
 *     holding a non-base translates to 'X'; 'X' and '*' are not residues;
 *   - frame f = 0, 1, 2 of a sequence s of n bytes is the string whose residue j is the translation of s[f + 3j .. f + 3j + 2],
 *     j < floor((n - f) / 3); frames 3, 4, 5 are frames 0, 1, 2 of the reverse complement of the whole of s (a non-base stays a
 *     non-base at its mirrored place);
 *   - a k-mer is k consecutive residues of one frame string, 1 <= k <= 32; a window holding '*' or 'X' yields nothing; no
 *     canonical choice, both strands contribute.  Equivalently every nucleotide start p <= n - 3k yields up to two k-mers, the
 *     forward one and the one of the reverse complement of s[p, p + 3k); a sequence shorter than 3k yields nothing;
 *   - hash = t1ha2_atonce(the k residue letters, upper case, seed) -- what hg_aa_* hashes for the same protein; a k-mer is kept
 *     iff hash < threshold, threshold = UINT64_MAX / scaled; hash value 0 is kept;
 *   - output: the distinct kept hashes over all six frames, ascending; the HV is hg_hv_encode's row for that set, norm2 and
 *     nhash as on the other paths.  ksize counts residues, in the .sketch container too.
 * The contexts are hypergen.h's (hg_ctx_create); the conventions and statuses too.  Link both libraries.
 */
#ifndef HYPERGEN_TX_H
#define HYPERGEN_TX_H

#include "hypergen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The distinct sampled hashes of the six frames of one nucleotide sequence (host memory, ASCII), ascending: the twin of
 * hg_aa_hash_sample, with the threshold itself.  If more than `cap` distinct hashes exist: HG_ERR_CAPACITY and *n_out =
 * count.  ksize > 32: HG_ERR_UNSUPPORTED. */
hg_status hg_tx_hash_sample(hg_ctx *ctx, const uint8_t *seq, size_t n, uint32_t ksize, uint64_t threshold, uint64_t seed,
                            uint64_t *out_hashes, size_t cap, size_t *n_out);

/* Whole-batch sketch of n genomes in device memory, ASCII nucleotides only: the buffer rules of hg_sketch_batch_dev (genome i
 * occupies [offsets[i], offsets[i] + lens[i]) of d_seq, offsets multiples of 4, 32 readable bytes behind every genome; d_hv
 * n * hv_d int16, d_norm2 n int32, d_nhash n uint32, all device).  The results are final in stream order when the call
 * returns: it never takes the deferred step, and it first resolves a deferred nucleotide step pending on the ctx, as every
 * call on a ctx does.  p->canonical is ignored; p->norm_mode must be 0 (HG_ERR_INVALID otherwise); p->min_count > 1 and
 * p->ksize > 32 are HG_ERR_UNSUPPORTED.  The plan is sized for windows of 3 * ksize bytes and two k-mers per start, so a
 * dense call (scaled = 1) fits its hit regions at the first attempt. */
hg_status hg_tx_sketch_batch_dev(hg_ctx *ctx, const uint8_t *d_seq, const uint64_t *offsets, const uint64_t *lens, size_t n,
                                 const hg_sketch_params *p, int16_t *d_hv, int32_t *d_norm2, uint32_t *d_nhash);
/* host buffers in, host results out: one upload, hg_tx_sketch_batch_dev, one download (nothing is packed) */
hg_status hg_tx_sketch_batch(hg_ctx *ctx, const uint8_t *const *seqs, const size_t *lens, size_t n, const hg_sketch_params *p,
                             int16_t *hv_out, int32_t *norm2_out, uint32_t *nhash_out);

/* Reading frame `frame` (0..5) of the n bytes of seq as defined above, stops as '*' and codons with a non-base as 'X':
 * floor((n - frame mod 3) / 3) residues into out (cap bytes; no terminator), their number into *n_out.  HG_ERR_CAPACITY with
 * *n_out = that number when cap is too small, HG_ERR_INVALID for a frame above 5 or a NULL argument.  Host only, needs no
 * GPU; it runs the classification and codon functions the kernel's tables are filled from. */
hg_status hg_tx_translate_frame(const uint8_t *seq, size_t n, uint32_t frame, uint8_t *out, size_t cap, size_t *n_out);

/* The plan of a translated batch as numbers (host only, no device involved), for tests and for callers that size a batch: the
 * twin of hg_sketch_plan_describe for windows of 3 * ksize bytes and two k-mers per start.  counts[0..5] = work items, hit slots
 * of the batch, largest and smallest hit region, largest expected sampled count (2 * starts / scaled), starts per work item.
 * A genome of n bytes has n - 3 * ksize + 1 starts; its region holds min(2 * expected + 1024, 2 * starts) hashes, at least 1,
 * rounded up to a power of two when it is beyond the one-workgroup sort. */
hg_status hg_tx_plan_describe(const uint64_t *offsets, const uint64_t *lens, size_t n, uint32_t ksize, uint64_t scaled,
                              uint64_t counts[6]);
/* How often the synchronous sketch path of this ctx -- under any library -- found a hit region too small and built the plan
 * again with larger ones.  A translated call never needs to: its plan holds two k-mers per start.  For tests. */
uint64_t hg_tx_plan_regrows(const hg_ctx *ctx);

/* Name of the kernel that hashes k-mers of this length, as rocprofv3 and hg_ctx_last_kernel(ctx, HG_T_KMER) spell it
 * ("" for a ksize outside 1..32).  The string lives as long as the library. */
const char *hg_tx_kernel_name(uint32_t ksize);
/* Geometry of that kernel, for callers that size batches and for tests: nucleotide starts one workgroup stages per tile, and
 * starts per work item (the plan's, shared with the nucleotide kernels; 0 for a ksize outside 1..32). */
uint32_t hg_tx_tile_starts(void);
uint32_t hg_tx_item_starts(uint32_t ksize);

#ifdef __cplusplus
}
#endif
#endif
