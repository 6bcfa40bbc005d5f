/*
 * hypergen_frag.h -- C ABI of libhypergen_frag.so: fragment-wise ANI and aligned fraction on the MI355X (gfx950).
 *
 * The fourth companion of libhypergen_hip.so (hypergen.h), beside libhypergen_aa.so, libhypergen_tx.so and libhypergen_rec.so.
 * One sketch per genome gives one number per pair, which mixes how similar the shared part of two genomes is with how much
 * of them is shared.  FastANI, skani, dRep's secondary clustering and GTDB's species rule report the two apart: the ANI
 * over the aligned part and the aligned fraction (AF).  They cut the query into fragments and keep each fragment's best hit
 * in the reference.  This library does that on sketches: the genome is cut into windows (hg_frag_plan), every window is
 * sketched from the one resident sequence (hg_frag_sketch_seq_dev), and the (reference windows x query fragments) ANI matrix
 * is reduced, while its row blocks stream past, to one record per pair of genomes (hg_frag_ani*).
 *
 * Window shapes.  With both sides cut into disjoint windows of L bases a query fragment usually straddles two reference
 * windows.  Reference windows of W = 2 L that start every S = L bases contain every colinear L-base stretch whole: under
 * HG_ANI_CONTAINMENT the best window's value is then the fragment's identity estimate, undiluted.
 *
 * Semantics of the reduction (there is no counterpart in the reference, this is the specification).  Rows are reference
 * windows, columns query fragments, ani[r * Q + q]; ref_first / qry_first cut the rows / columns into genomes.
 *   m(r, q)    = the integer of the cluster statistics (hypergen.h): NaN and negative values 0, values above 100 100 000,
 *                else rint((double)ani * 1000.0);
 *   m_th       = rint((double)frag_th * 1000.0) clamped to 0..100 000 (a NaN threshold: 0);
 *   best(g, q) = the maximum of m(r, q) over the rows r of reference genome g, `row` the smallest r that attains it; a
 *                genome without rows gives m = 0, row = HG_FRAG_NONE;
 *   pair(g, h) : total = the fragments of query genome h, matched = those with best(g, q) >= m_th, sum = the sum of
 *                those bests.  With m_th = 0 every fragment matches.
 * Only integer max and add are used and ties go to the smaller row: the result depends on the matrix and the offsets
 * alone, not on block_rows, the grid or the order of the atomics.
 * Edge cases: R = 0, Q = 0, n_ref = 0 or n_qry = 0 return HG_OK with the records written as empty -- total as defined, sum
 * and matched 0, every best {0, HG_FRAG_NONE}.  Offsets that do not start at 0, are not ascending or do not end at R / Q:
 * HG_ERR_INVALID.  R or Q >= 2^31: HG_ERR_UNSUPPORTED.
 * The genome ANI a caller prints is (2 sum + matched) / (2 matched) in integer division, in thousandths; AF is matched / total.
 *
 * The contexts are hypergen.h's (hg_ctx_create); the conventions and statuses too.  Link both libraries.
 */
#ifndef HYPERGEN_FRAG_H
#define HYPERGEN_FRAG_H

#include "hypergen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HG_FRAG_NONE 0xFFFFFFFFu

typedef struct {
  uint64_t sum;     /* sum of best(g, q) over the matched fragments of h, in thousandths */
  uint32_t matched; /* fragments of h with best(g, q) >= m_th */
  uint32_t total;   /* fragments of h */
} hg_frag_pair;     /* 16 bytes */

typedef struct {
  uint32_t m;   /* best(g, q) in thousandths */
  uint32_t row; /* the smallest reference row that attains it, HG_FRAG_NONE for a genome without rows */
} hg_frag_best; /* 8 bytes */

/* The windows of a sequence of len bases (host arithmetic, no device).  window and step are multiples of 4 (the offsets of
 * hg_sketch_batch_dev are) with 4 <= step <= window, anything else is HG_ERR_INVALID.  len <= window: one window [0, len) --
 * also for len = 0, so that the genome stays present.  Otherwise 1 + ceil((len - window) / step) windows, window j =
 * [j step, min(j step + window, len)); a last window shorter than window / 2 is dropped (never with step <= window / 2; with
 * step = window a short tail is, as in FastANI).  *n = the number of windows; cap < *n: HG_ERR_CAPACITY and nothing beyond
 * cap is written (starts and lens may be NULL when cap is 0). */
hg_status hg_frag_plan(uint64_t len, uint64_t window, uint64_t step, uint64_t *starts, uint64_t *lens, size_t cap, size_t *n);

/* Called by hg_frag_sketch_seq_dev once per sub-batch: the m windows [first, first + m) of the plan with their starts and
 * lengths and their rows (hv: m * hv_d int16; norm2 and nhash: m entries; all host memory that is reused after the call
 * returns).  A return value other than 0 ends the sketching with HG_ERR_INVALID. */
typedef int (*hg_frag_rows_fn)(void *user, const uint64_t *starts, const uint64_t *lens, size_t first, size_t m, const int16_t *hv,
                               const int32_t *norm2, const uint32_t *nhash);

/* One sketch per window of the genome at d_seq: n_bps bytes in hg_read_merge_seq layout on the device, at an address that is
 * a multiple of 4, with 32 readable bytes behind them.  hg_sketch_batch_dev runs over the planned windows as offsets into
 * that one buffer -- overlapping windows read the same bytes, nothing is copied -- in sub-batches of at most 65 536 windows,
 * hg_ctx_sync behind each before a row is read, and `rows` gets every sub-batch.  A window's sketch is bit for bit what
 * hg_sketch_batch_dev gives for its bytes as a genome of their own: a genome's end, not the buffer's, masks the k-mers.
 * *n_windows = windows of the plan. */
hg_status hg_frag_sketch_seq_dev(hg_ctx *ctx, const uint8_t *d_seq, uint64_t n_bps, const hg_sketch_params *p, uint64_t window,
                                 uint64_t step, hg_frag_rows_fn rows, void *user, size_t *n_windows);

/* The reduction of an ANI matrix that lies on the device: d_ani, R x Q floats, row-major.  ref_first (host): n_ref + 1
 * ascending row offsets, [0] = 0, [n_ref] = R; qry_first (host): likewise over the columns.  d_pair (device, 8-byte aligned):
 * n_ref * n_qry records, [g * n_qry + h].  d_best (device, 8-byte aligned, may be NULL): n_ref * Q records, [g * Q + q].
 * Independent of the ctx's ANI metric.  Results are final on return.  Launches count under HG_T_DIST when timing is on. */
hg_status hg_frag_ani_matrix_dev(hg_ctx *ctx, const float *d_ani, size_t R, size_t Q, const uint32_t *ref_first, size_t n_ref,
                                 const uint32_t *qry_first, size_t n_qry, float frag_th, hg_frag_pair *d_pair, hg_frag_best *d_best);

/* The same from resident sketches: the matrix under the ctx's ANI metric (all three are accepted) arrives as row blocks
 * from hg_dist_full_dev in a scratch block of at most HG_SEARCH_BLOCK_BYTES; block_rows > 0 forces the rows per block (a
 * test makes a genome straddle blocks), 0 leaves the choice to the library.  No R x Q matrix is held.  Without d_best the
 * table of bests, 8 bytes x n_ref x Q, is processed in groups of reference genomes that fit the same bound. */
hg_status hg_frag_ani_dev(hg_ctx *ctx, const int16_t *d_ref_hv, const int32_t *d_ref_norm2, size_t R, const int16_t *d_qry_hv,
                          const int32_t *d_qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, const uint32_t *ref_first, size_t n_ref,
                          const uint32_t *qry_first, size_t n_qry, float frag_th, size_t block_rows, hg_frag_pair *d_pair,
                          hg_frag_best *d_best);

/* host arrays in and out (best may be NULL), staged through the ctx: uploads, hg_frag_ani_dev, downloads. */
hg_status hg_frag_ani(hg_ctx *ctx, const int16_t *ref_hv, const int32_t *ref_norm2, size_t R, const int16_t *qry_hv,
                      const int32_t *qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, const uint32_t *ref_first, size_t n_ref,
                      const uint32_t *qry_first, size_t n_qry, float frag_th, hg_frag_pair *pair, hg_frag_best *best);

/* Geometry, for tests that place segment sizes on its boundaries: rows of one genome a workgroup of frag_best_kernel
 * reduces, columns it covers, lanes of a wave (the first reduction step of frag_fold_kernel) and lanes of its workgroup. */
uint32_t hg_frag_row_chunk(void);
uint32_t hg_frag_col_tile(void);
uint32_t hg_frag_wave(void);
uint32_t hg_frag_fold_threads(void);
/* The library's kernels as rocprofv3 spells them, in launch order, separated by '\n'.  The string lives as long as the library. */
const char *hg_frag_kernel_names(void);
/* How often this process has launched each of them so far, in the order of hg_frag_kernel_names (cap entries at most; returns
 * the number of kernels).  For tests. */
uint32_t hg_frag_launch_counts(uint64_t *counts, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif
