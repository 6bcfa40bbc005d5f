/*
 * hypergen_hist.h -- C ABI of libhypergen_hist.so: the distribution of the ANI values of a whole comparison on the MI355X (gfx950).
 *
 * The fifth companion of libhypergen_hip.so (hypergen.h), beside libhypergen_aa.so, libhypergen_tx.so, libhypergen_rec.so and
 * libhypergen_frag.so.  A comparison of 100 000 x 100 000 sketches has 10^10 pairs: what clears a threshold, the best N and
 * the clusters can be asked of it, its TSV at -a 0 cannot be written.  The histogram of all its ANI values -- the plot behind
 * the "95 % species gap", and the only way to learn how many pairs a threshold will produce before it is run -- is at most
 * 100 001 integers.  This library reduces the matrix to that table of counts while its row blocks stream past.
 *
 * Semantics (there is no counterpart in the reference, this is the specification).
 *   m(r, q)    = the integer of the cluster statistics (hypergen.h), the ANI as dist prints it, in thousandths: NaN and
 *                negative values 0, values above 100 100 000, else rint((double)ani * 1000.0).  Range 0..100 000.
 *   bin_milli  = w, the width of a bin in thousandths, 1..100 000.
 *   n_bins     = 100 000 / w + 1 in integer division (hg_hist_bins).
 *   A pair falls into bin m / w: bin b holds the printed values [b w, min((b + 1) w - 1, 100 000)].
 *   pairs      = which entries count, by global row index i and global column index j: HG_HIST_ALL every (i, j),
 *                HG_HIST_UPPER i < j, HG_HIST_OFFDIAG i != j -- the three enumerations dist has: two files; one file under
 *                a symmetric metric; one file under containment.
 *   counts[b]  = the number of selected pairs in bin b (64 bits).
 * The histogram of a comparison is the histogram of the third field of its `dist -a 0` TSV and can be reproduced from one.
 * Only integer adds are used: the result depends on the matrix alone, not on block_rows, the grid or the order of the
 * atomics.
 *
 * What the counts do NOT say.  The sum of the counts from a bin's lower edge upwards is the number of TSV lines that PRINT
 * at least that value.  It is not the hit count of `dist -a x`, which compares the float: a pair at 94.9996 prints 95.000
 * and fails >= 95.
 *
 * Cost.  One workgroup's table in LDS covers hg_hist_lds_bins() bins.  A histogram of more bins is counted in slices of that
 * many bins, each slice by workgroups of its own that read the block again: the matrix is read ceil(n_bins / table) times --
 * once at w >= 13 with a table of 8 192 bins (the CLI's default w = 100 has 1 001 bins), 13 times at w = 1.
 *
 * The contexts are hypergen.h's (hg_ctx_create); the conventions and statuses too.  Link both libraries.
 */
#ifndef HYPERGEN_HIST_H
#define HYPERGEN_HIST_H

#include "hypergen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HG_HIST_ALL 0u     /* every (i, j) */
#define HG_HIST_UPPER 1u   /* i < j */
#define HG_HIST_OFFDIAG 2u /* i != j */
#define HG_HIST_MILLI_MAX 100000u

/* n_bins of a bin width, or 0 for a width outside 1..100 000.  Host arithmetic only. */
uint32_t hg_hist_bins(uint32_t bin_milli);

/* ADDS the selected pairs of one block of a matrix to d_counts: hg_hist_bins(bin_milli) 64-bit counts on the device, 8-byte
 * aligned, zeroed by the caller before the first block.  d_ani[r * pitch + c] is the value of the global pair (row0 + r,
 * col0 + c), r < rows, c < cols; pitch >= cols, in floats; d_ani may have any 4-byte alignment.  Stream-ordered on the ctx's
 * stream (nothing is final before hg_ctx_sync), independent of the ctx's ANI metric.  rows == 0 or cols == 0: HG_OK, nothing
 * added.  A block that lies wholly outside the selection launches nothing.  Unknown `pairs`, a width outside 1..100 000, a
 * NULL or misaligned pointer, pitch < cols: HG_ERR_INVALID.  A global index >= 2^31: HG_ERR_UNSUPPORTED.  Launches count
 * under HG_T_DIST when timing is on. */
hg_status hg_hist_add_matrix_dev(hg_ctx *ctx, const float *d_ani, size_t rows, size_t cols, size_t pitch, size_t row0, size_t col0,
                                 uint32_t pairs, uint32_t bin_milli, uint64_t *d_counts);

/* The histogram of a comparison of resident sketches: d_counts is zeroed, then the matrix under the ctx's ANI metric (all
 * three are accepted) arrives as row blocks from hg_dist_full_dev in a scratch block of at most HG_SEARCH_BLOCK_BYTES and
 * every block is counted; block_rows > 0 forces the rows per block (for tests), 0 leaves the choice to the library.  No
 * R x Q matrix is held.  HG_HIST_UPPER and HG_HIST_OFFDIAG need the same set on both sides -- identical pointers and R == Q --
 * anything else is HG_ERR_INVALID; HG_HIST_UPPER computes only the columns >= the block's first row, and under
 * HG_ANI_CONTAINMENT it is HG_ERR_INVALID (the metric is directional: the rule of hg_dist_dev's `symmetric`).  R == 0 or
 * Q == 0: HG_OK, all counts 0.  Results are final on return. */
hg_status hg_hist_dev(hg_ctx *ctx, const int16_t *d_ref_hv, const int32_t *d_ref_norm2, size_t R, const int16_t *d_qry_hv,
                      const int32_t *d_qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, uint32_t pairs, uint32_t bin_milli,
                      size_t block_rows, uint64_t *d_counts);

/* host arrays in and out, staged through the ctx: uploads, hg_hist_dev, download.  The same set on both sides is the same
 * host pointers and R == Q: it is uploaded once. */
hg_status hg_hist(hg_ctx *ctx, const int16_t *ref_hv, const int32_t *ref_norm2, size_t R, const int16_t *qry_hv, const int32_t *qry_norm2,
                  size_t Q, uint32_t hv_d, uint32_t ksize, uint32_t pairs, uint32_t bin_milli, uint64_t *counts);

/* Geometry, for tests that place values and sizes on its boundaries: the bins one workgroup's LDS table covers (a histogram
 * of more bins is counted in slices of this many; one of at most half as many keeps several copies of its table, one per
 * wave), the rows and the columns of a workgroup's tile, and the lanes of a workgroup (a lane of a wave owns four consecutive
 * columns, the waves take the tile's rows in turn). */
uint32_t hg_hist_lds_bins(void);
uint32_t hg_hist_tile_rows(void);
uint32_t hg_hist_tile_cols(void);
uint32_t hg_hist_threads(void);
/* The library's kernels as rocprofv3 spells them, separated by '\n'.  The string lives as long as the library. */
const char *hg_hist_kernel_names(void);
/* How often this process has launched each of them so far, in the order of hg_hist_kernel_names (cap entries at most; returns
 * the number of kernels).  For tests. */
uint32_t hg_hist_launch_counts(uint64_t *counts, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif
