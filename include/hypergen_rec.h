/*
 * hypergen_rec.h -- C ABI of libhypergen_rec.so: one multi-FASTA text split into its records on the MI355X (gfx950).
 *
 * The third companion of libhypergen_hip.so (hypergen.h), beside libhypergen_aa.so and libhypergen_tx.so.  Plasmid and viral
 * databases and the contigs of a metagenome assembly come as ONE file of thousands to millions of records; Mash -i, sourmash
 * --singleton and skani -i read such a file directly.  This library is the step in front of hg_sketch_batch_dev for it: the
 * text goes to the device once, a few streaming kernels find the records and write their sequences as the batch layout that
 * call takes -- offsets that are multiples of 4, no line ends -- and the unchanged sketch step runs on that batch.
 *
 * Semantics (there is no counterpart in the reference, this is the specification; the line rule is read_merge_seq's,
 * src/fastx_reader.rs:6-29)
 *   - the text is n bytes.  Lines end at LF; the last line may lack one.  A line's content is its bytes without the LF and
 *     without one CR directly before the LF; for an unterminated last line a CR as the very last byte of the text is dropped
 *     too.  Any other CR stays;
 *   - a header line is a line whose content starts with '>'.  An empty line is not a header; a '>' anywhere but at the first
 *     byte of a line is an ordinary sequence byte;
 *   - record r is the r-th header line.  Its sequence is the concatenation of the contents of the non-header lines behind it
 *     and before the next header; it may be empty.  No byte is classified or normalised: that stays with the k-mer kernels;
 *   - a non-header line with non-empty content before the first header is HG_ERR_IO ("sequence data before the first
 *     header"; a FASTQ file falls under this).  Empty lines before the first header are allowed;
 *   - the identifier of a record is the longest prefix of the header content behind the '>' made of bytes above 0x20.  It
 *     may be empty: the library reports its length, the caller decides what an empty one means;
 *   - 'N' + sequence, joined over all records in order, is exactly what hg_read_merge_seq returns for the file.
 *
 * Layout of the result
 *   - record r occupies [seq_off[r], seq_off[r] + seq_len[r]) of the sequence buffer; seq_off[0] = 0 and seq_off[r + 1] is
 *     seq_off[r] + seq_len[r] rounded up to a multiple of 4; the 0 to 3 bytes between two records are written as 'N';
 *   - seq_bytes is the end of the last record, rounded up the same way (0 without records).  The caller's buffer must hold
 *     seq_bytes + 32 bytes -- the 32 readable bytes behind every genome of hg_sketch_batch_dev; bytes from seq_bytes on are
 *     not written;
 *   - the record table has one hg_rec_entry per record.
 * The contexts are hypergen.h's (hg_ctx_create); the conventions and statuses too.  Link both libraries.
 */
#ifndef HYPERGEN_REC_H
#define HYPERGEN_REC_H

#include "hypergen.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint64_t hdr_off; /* where the '>' is in the text                      */
  uint32_t hdr_len; /* length of the header content, with the '>'        */
  uint32_t id_len;  /* length of the identifier (it starts at hdr_off + 1) */
  uint64_t seq_off; /* where the sequence starts in the sequence buffer  */
  uint64_t seq_len;
} hg_rec_entry;

/* Number of records and size of the sequence layout of the n bytes at d_text (device memory, 16-byte aligned, readable up to
 * n rounded up to 16; whatever lies behind byte n is ignored).  n >= 2^32: HG_ERR_UNSUPPORTED; sequence data before the first
 * header: HG_ERR_IO; n == 0: zero counts.  Complete on return. */
hg_status hg_rec_count_dev(hg_ctx *ctx, const uint8_t *d_text, size_t n, size_t *n_recs, size_t *seq_bytes);

/* The split itself: the layout above into d_seq (device, 16-byte aligned, seq_cap bytes) and d_recs (device, 16-byte aligned,
 * rec_cap entries).  rec_cap < *n_recs or seq_cap < *seq_bytes + 32: HG_ERR_CAPACITY with both needed sizes in *n_recs and
 * *seq_bytes, and nothing is written beyond the capacities.  The other statuses are hg_rec_count_dev's.  The result is
 * complete in stream order on the ctx's stream when the call returns. */
hg_status hg_rec_split_dev(hg_ctx *ctx, const uint8_t *d_text, size_t n, uint8_t *d_seq, size_t seq_cap, hg_rec_entry *d_recs,
                           size_t rec_cap, size_t *n_recs, size_t *seq_bytes);

/* host memory in, host results out: one upload, hg_rec_split_dev, one download.  seq_out and recs_out may be NULL when their
 * capacity is 0 (the call then reports the sizes with HG_ERR_CAPACITY). */
hg_status hg_rec_split(hg_ctx *ctx, const uint8_t *text, size_t n, uint8_t *seq_out, size_t seq_cap, hg_rec_entry *recs_out,
                       size_t rec_cap, size_t *n_recs, size_t *seq_bytes);

/* The same outputs from one host thread, no GPU involved: the yardstick of tools/rec_split_bench.py and what makes the
 * semantics testable without a device.  Not a fallback: nothing in the library or the command line calls it.  The capacity
 * rule is hg_rec_split_dev's; what fits the capacities may have been written when HG_ERR_CAPACITY is returned. */
hg_status hg_rec_split_host(const uint8_t *text, size_t n, uint8_t *seq_out, size_t seq_cap, hg_rec_entry *recs_out,
                            size_t rec_cap, size_t *n_recs, size_t *seq_bytes);

/* The bytes of a file, gzip inflated transparently, in page-locked memory (*buf NULL or from an earlier call, *cap its size;
 * release with hg_pinned_free): the pattern of hg_read_fastx_pinned.  At least 64 zero bytes follow the *n bytes of text, so
 * that n rounded up to 16 may be uploaded.  A file of 2^32 bytes or more after inflation: HG_ERR_UNSUPPORTED. */
hg_status hg_rec_read_text(const char *path, uint8_t **buf, size_t *cap, size_t *n);

/* Called by hg_rec_sketch_text_dev: first once with m == 0 when the record table is known, then once per sub-batch with the
 * rows of m records: row i belongs to record which[i] of recs (hv: m * hv_d int16; norm2 and nhash: m entries; all host
 * memory that is reused after the call returns).  A return value other than 0 ends the sketching with HG_ERR_INVALID. */
typedef int (*hg_rec_rows_fn)(void *user, const hg_rec_entry *recs, size_t n_recs, const uint32_t *which, size_t m,
                              const int16_t *hv, const int32_t *norm2, const uint32_t *nhash);

/* One sketch per record of the text at d_text (as for hg_rec_count_dev): count, allocate, split, download the table, then
 * hg_sketch_batch_dev over consecutive ranges of the records with at least min_length sequence bytes -- sub-batches of at most
 * 65 536 records or 1 GiB of sequence, hg_ctx_sync behind each before a row is read -- and `rows` for every sub-batch.  A
 * record shorter than p->ksize is sketched like any other and has nhash 0.  *n_recs = records of the text, *n_kept = records
 * sketched.  2^31 records or more: HG_ERR_UNSUPPORTED. */
hg_status hg_rec_sketch_text_dev(hg_ctx *ctx, const uint8_t *d_text, size_t n, const hg_sketch_params *p, uint64_t min_length,
                                 hg_rec_rows_fn rows, void *user, size_t *n_recs, size_t *n_kept);

/* Bytes of text one workgroup of the per-block kernels reads, for tests that place bytes on a block boundary. */
uint32_t hg_rec_block_bytes(void);
/* The library's kernels as rocprofv3 spells them, in launch order, separated by '\n'.  The string lives as long as the library. */
const char *hg_rec_kernel_names(void);
/* How often this process has launched each of them so far, in the order of hg_rec_kernel_names (cap entries at most; returns
 * the number of kernels).  For tests. */
uint32_t hg_rec_launch_counts(uint64_t *counts, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif
