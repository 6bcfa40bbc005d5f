/*
 * hypergen_tri.h -- C ABI of libhypergen_tri.so: the ANI matrix of all pairs of one set of sketches as fixed-width text,
 * formatted on the MI355X (gfx950).
 *
 * The sixth companion of libhypergen_hip.so (hypergen.h), beside libhypergen_aa.so, libhypergen_tx.so, libhypergen_rec.so,
 * libhypergen_frag.so and libhypergen_hist.so.  Tree builders, R's as.dist, heat maps and ordination scripts read the matrix
 * of all pairs (Mash and skani `triangle`, sourmash `compare`, FastANI --matrix write it).  `dist -a 0` prints every pair
 * too, but as one line per pair with both names in it, formatted on the host.  This library turns the blocks of the float
 * matrix into text on the device and hands the text to the host while the next block is computed.
 *
 * Semantics (there is no counterpart in the reference, this is the specification).
 *   m(i, j)  = the integer dist prints for the pair, in thousandths (hypergen_hist.h): NaN and negative values 0, values
 *              above 100 100 000, else rint((double)ani * 1000.0).  Range 0..100 000.
 *   A FIELD is HG_TRI_FIELD_BYTES = 8 bytes: m / 1000 right-aligned in three characters, padded with spaces; '.';
 *   m % 1000 as three digits ("  0.000", " 95.123", "100.000"); then one separator, '\n' behind the last field of a row and
 *   '\t' behind every other one.
 *   HG_TRI_LOWER : row i carries the fields j = 0..i-1, no diagonal; row 0 carries none.  The fields of row i start at
 *                  byte 8 i (i - 1) / 2 of the field text.
 *   HG_TRI_FULL  : row i carries all `cols` fields, the diagonal as computed.  The fields of row i start at byte 8 i cols.
 * Every field has the same width, so every offset is closed-form: blocks of rows can be written independently and a reader
 * can seek to the pair (i, j).  All offsets are 64-bit: 8 i (i - 1) / 2 passes 2^32 near i = 33 000.
 *
 * The FIELD TEXT of a block of rows [row0, row0 + rows) is the concatenation of its rows' fields,
 * hg_tri_text_bytes(layout, row0, rows, cols) bytes.  The PHYLIP-like file `hyper-gen triangle` writes is "n\n", then per
 * row its name, '\t' (or '\n' for a row without fields) and the row's fields; the names are the caller's.
 *
 * The contexts are hypergen.h's (hg_ctx_create); the conventions and statuses too.  Link both libraries.
 */
#ifndef HYPERGEN_TRI_H
#define HYPERGEN_TRI_H

#include "hypergen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HG_TRI_LOWER 0u /* j < i */
#define HG_TRI_FULL 1u  /* every j */
#define HG_TRI_FIELD_BYTES 8u

/* The bytes of the field text of the rows [row0, row0 + rows): LOWER 8 (T(row0 + rows) - T(row0)) with T(i) = i (i - 1) / 2
 * (cols is not used), FULL 8 rows cols.  0 for an unknown layout.  Host arithmetic only, 64 bits. */
uint64_t hg_tri_text_bytes(uint32_t layout, uint64_t row0, uint64_t rows, uint64_t cols);
/* The offset of the field of the pair (i, j), i a GLOBAL row >= row0, in the field text of a block that starts at row0:
 * LOWER 8 (T(i) - T(row0) + j), FULL 8 ((i - row0) cols + j).  With row0 = 0 it is the offset in the whole field text.
 * 0 for an unknown layout.  Host arithmetic only, 64 bits. */
uint64_t hg_tri_field_offset(uint32_t layout, uint64_t row0, uint64_t i, uint64_t j, uint64_t cols);

/* Formats one block of an ANI matrix that lies on the device and whose columns start at global column 0:
 * d_ani[r * pitch + c] is the value of the pair (row0 + r, c), r < rows, c < cols; pitch >= cols, in floats; d_ani may have
 * any 4-byte alignment.  d_text, 8-byte aligned, receives exactly hg_tri_text_bytes(layout, row0, rows, cols) bytes; nothing
 * beyond them is touched.  HG_TRI_LOWER needs cols >= row0 + rows - 1 and reads and writes only the pairs j < i.
 * Stream-ordered on the ctx's stream (nothing is final before hg_ctx_sync), independent of the ctx's ANI metric.
 * rows == 0 or cols == 0, or a LOWER block of row 0 alone: HG_OK, nothing written.  Unknown layout, a NULL or misaligned
 * pointer, pitch < cols, a LOWER block with too few columns: HG_ERR_INVALID.  A global index >= 2^31: HG_ERR_UNSUPPORTED.
 * Launches count under HG_T_DIST when timing is on. */
hg_status hg_tri_format_dev(hg_ctx *ctx, const float *d_ani, size_t rows, size_t cols, size_t pitch, size_t row0, uint32_t layout,
                            char *d_text);

/* The whole field text of one resident set of n sketches, under the ctx's ANI metric, into d_text on the device
 * (hg_tri_text_bytes(layout, 0, n, n) bytes, 8-byte aligned).  The matrix arrives as row blocks of hg_dist_full_dev in the
 * scratch block the search and matrix calls of the ctx use, and every block is formatted behind its GEMM; under HG_TRI_LOWER
 * only the columns in front of the block's last row are computed.  block_rows > 0 forces the rows per block (for tests), 0
 * leaves the choice to the library (HG_SEARCH_BLOCK_BYTES of floats at the most).  HG_TRI_LOWER under HG_ANI_CONTAINMENT is
 * HG_ERR_INVALID (the metric is directional).  n == 0, and n == 1 under LOWER: HG_OK, nothing written.  n >= 2^31:
 * HG_ERR_UNSUPPORTED.  Results are final on return. */
hg_status hg_tri_dev(hg_ctx *ctx, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize, uint32_t layout,
                     size_t block_rows, char *d_text);

/* What hg_tri_stream_dev hands over: the field text of the rows [row0, row0 + rows), `bytes` of it, in page-locked host
 * memory that is the library's again once the call returns.  Blocks arrive in ascending order, on the calling thread; a block
 * without fields (row 0 under LOWER) arrives with bytes == 0.  A return other than 0 ends the call. */
typedef int (*hg_tri_sink)(void *user, const char *text, size_t bytes, size_t row0, size_t rows);

/* The same text without holding it on the device: block b is formatted into one of two device buffers, copied into one of two
 * page-locked host buffers on a second stream and handed to `sink`; while the sink runs, block b + 1 is computed, formatted
 * and copied into the other pair.  A block holds 64 MiB of text at the most (one row where a row is longer).  The
 * concatenation of the blocks is hg_tri_dev's text.  A sink that returns non-zero ends the call
 * with HG_ERR_IO once the work in flight has drained; the ctx is usable afterwards.  NULL sink: HG_ERR_INVALID.  Otherwise as
 * hg_tri_dev. */
hg_status hg_tri_stream_dev(hg_ctx *ctx, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                            uint32_t layout, size_t block_rows, hg_tri_sink sink, void *user);

/* host arrays in, host text out (hg_tri_text_bytes(layout, 0, n, n) bytes), staged through the ctx: upload, hg_tri_dev,
 * download. */
hg_status hg_tri(hg_ctx *ctx, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize, uint32_t layout, char *text);

/* Geometry, for tests that place sizes on its boundaries: the rows and the columns of a workgroup's tile and the lanes of a
 * workgroup (a lane of a wave owns four consecutive columns, the waves take the tile's rows in turn). */
uint32_t hg_tri_tile_rows(void);
uint32_t hg_tri_tile_cols(void);
uint32_t hg_tri_threads(void);
/* The library's kernels as rocprofv3 spells them, separated by '\n'.  The string lives as long as the library. */
const char *hg_tri_kernel_names(void);
/* How often this process has launched each of them so far, in the order of hg_tri_kernel_names (cap entries at most; returns
 * the number of kernels).  For tests. */
uint32_t hg_tri_launch_counts(uint64_t *counts, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif
