// hg_rec.h -- what hg_rec.hip (host entry points) and hg_rec_kernels.hip (kernels) of libhypergen_rec.so share: the summary a
// stretch of FASTA text is reduced to, the geometry of the passes and the launchers.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hypergen_rec.h"

// ---- geometry ------------------------------------------------------------------------------------------------------------
constexpr uint32_t HG_REC_THREADS = 256;                       // every kernel of the library
constexpr uint32_t HG_REC_LANE_BYTES = 16;                     // one 16-byte load per lane
constexpr uint32_t HG_REC_BLOCK = HG_REC_THREADS * HG_REC_LANE_BYTES;  // bytes of text per workgroup: 4096
constexpr uint32_t HG_REC_TILE_ITEMS = 4;                      // block summaries per thread of the two scan kernels
constexpr uint32_t HG_REC_TILE = HG_REC_THREADS * HG_REC_TILE_ITEMS;   // blocks per tile: 1024 (n < 2^32: at most 1024 tiles)
constexpr uint32_t HG_REC_PAD_ITEMS = 8;                       // records per thread of the pad kernels
constexpr uint32_t HG_REC_PAD_TILE = HG_REC_THREADS * HG_REC_PAD_ITEMS;  // records per tile: 2048
constexpr uint32_t HG_REC_IMAGE = HG_REC_BLOCK + 64;           // LDS image of one block's output: its bytes, <= 8 pad bytes more, 16 of alignment
constexpr uint32_t HG_REC_NONE = 0xFFFFFFFFu;                  // "no such position" (positions are below 2^32 - 1)

// ---- the summary of a stretch of text ---------------------------------------------------------------------------------
// Whether a byte is sequence depends on whether the line it lies in started with '>', and that line start may be many blocks
// back.  A stretch of text -- a lane's 16 bytes, a block, a tile of blocks -- is therefore reduced to what the text behind it
// needs to know of it, and to its own counts as far as they do not depend on the text in front of it:
//   flags    HG_REC_LS: a line starts inside the stretch; HG_REC_HDR: the last such line is a header line
//   ls_pos   where that last line starts
//   ctl_pos  first byte <= 0x20 behind that line start (in the whole stretch when no line starts in it), HG_REC_NONE without:
//            where the identifier of a header ends
//   n_hdr    header lines that start in the stretch
//   pre      sequence bytes in front of the first line start: they count only if the stretch is entered inside a sequence line
//   post     sequence bytes of the non-header lines that start in the stretch
// hg_rec_combine(a, b) is the summary of a followed by b; it is associative, with hg_rec_identity() as its neutral element.
enum : uint32_t { HG_REC_LS = 1, HG_REC_HDR = 2 };
struct hg_rec_sum {
  uint32_t flags, ls_pos, ctl_pos, n_hdr, pre, post;
};

__host__ __device__ inline hg_rec_sum hg_rec_identity() { return hg_rec_sum{0, 0, HG_REC_NONE, 0, 0, 0}; }

__host__ __device__ inline hg_rec_sum hg_rec_combine(const hg_rec_sum &a, const hg_rec_sum &b) {
  const bool al = (a.flags & HG_REC_LS) != 0, bl = (b.flags & HG_REC_LS) != 0;
  hg_rec_sum r;
  r.flags = bl ? b.flags : a.flags;
  r.ls_pos = bl ? b.ls_pos : a.ls_pos;
  r.ctl_pos = bl ? b.ctl_pos : (a.ctl_pos != HG_REC_NONE ? a.ctl_pos : b.ctl_pos);
  r.n_hdr = a.n_hdr + b.n_hdr;
  r.pre = a.pre + (al ? 0u : b.pre);
  r.post = a.post + b.post + (al && !(a.flags & HG_REC_HDR) ? b.pre : 0u);
  return r;
}
// a prefix summary taken from the first byte of the text (which is a line start, and the text is entered outside a header):
// is the byte behind it inside a header line, and how many sequence bytes precede it
__host__ __device__ inline bool hg_rec_in_header(const hg_rec_sum &x) { return (x.flags & (HG_REC_LS | HG_REC_HDR)) == (HG_REC_LS | HG_REC_HDR); }
__host__ __device__ inline uint32_t hg_rec_seq_before(const hg_rec_sum &x) { return x.pre + x.post; }

// ---- result words (device, read back by the host) ------------------------------------------------------------------------
enum : uint32_t {
  HG_REC_RES_NRECS = 0,   // header lines of the text
  HG_REC_RES_TOTAL = 1,   // sequence bytes of the text, those before the first header included
  HG_REC_RES_LEAD = 2,    // sequence bytes before the first header (when there is one)
  HG_REC_RES_PAD_LO = 4,  // sum of the pads behind all records, 64 bits
  HG_REC_RES_PAD_HI = 5,
  HG_REC_RES_WORDS = 8
};

// ---- launchers (hg_rec_kernels.hip), all on `st`, in the order a split queues them ---------------------------------------
enum : uint32_t {
  HG_REC_K_SUMMARY, HG_REC_K_TILE_REDUCE, HG_REC_K_PREFIX, HG_REC_K_MARK, HG_REC_K_PAD_REDUCE, HG_REC_K_PAD_SCAN,
  HG_REC_K_OFFSETS, HG_REC_K_SCATTER, HG_REC_N_KERNELS
};
// how often the process has launched kernel k so far (hg_rec_launch_counts)
uint64_t hg_rec_launches(uint32_t kernel);
// blocks of text -> one summary each
hipError_t hg_rec_launch_summary(hipStream_t st, const uint8_t *d_text, uint64_t n, hg_rec_sum *d_blk, uint32_t n_blk);
// tiles of block summaries -> one summary each
hipError_t hg_rec_launch_tile_reduce(hipStream_t st, const hg_rec_sum *d_blk, uint32_t n_blk, hg_rec_sum *d_tile, uint32_t n_tiles);
// block summaries -> the summary of everything in front of each block, in place; the text's totals into d_res
hipError_t hg_rec_launch_prefix(hipStream_t st, hg_rec_sum *d_blk, uint32_t n_blk, const hg_rec_sum *d_tile, uint32_t n_tiles, uint32_t *d_res);
// per header line: hdr_off, hdr_len, id_len (d_recs may be NULL) and the number of sequence bytes in front of it (d_cidx,
// n_recs + 1 entries: the last is the text's total)
hipError_t hg_rec_launch_mark(hipStream_t st, const uint8_t *d_text, uint64_t n, const hg_rec_sum *d_pre, uint32_t n_blk,
                              hg_rec_entry *d_recs, uint32_t *d_cidx, uint32_t n_recs, uint32_t *d_res);
// the pads behind the records, summed per tile of records / scanned over the tiles / scanned inside each tile: d_ps[r] = sum of
// the pads behind the records in front of r (n_recs + 1 entries); seq_off and seq_len of every record (d_recs may be NULL)
hipError_t hg_rec_launch_pad_reduce(hipStream_t st, const uint32_t *d_cidx, uint32_t n_recs, uint32_t *d_tsum, uint32_t n_tiles);
hipError_t hg_rec_launch_pad_scan(hipStream_t st, const uint32_t *d_tsum, uint64_t *d_tbase, uint32_t n_tiles, uint32_t *d_res);
hipError_t hg_rec_launch_offsets(hipStream_t st, const uint32_t *d_cidx, uint32_t n_recs, const uint64_t *d_tbase, uint64_t *d_ps,
                                 hg_rec_entry *d_recs);
// the sequence bytes and the 'N' pads into d_seq (seq_bytes: the size of the layout, nothing is written from there on)
hipError_t hg_rec_launch_scatter(hipStream_t st, const uint8_t *d_text, uint64_t n, const hg_rec_sum *d_pre, uint32_t n_blk,
                                 const uint64_t *d_ps, uint32_t n_recs, uint8_t *d_seq, uint64_t seq_bytes);
