// hg_stream_layout.h -- what a chunk of the streaming sketcher (hg_stream.hip) holds, where each genome's bytes go in its areas
// and when it closes.  Arithmetic only (no HIP, no threads): checked on the CPU by tests/native/stream_layout_driver.cpp.
#pragma once
#include <algorithm>
#include <vector>
#include "hg_pack2.h"

constexpr size_t CHUNK_BYTES = 64ull << 20;  // device bytes a chunk aims at (one larger genome still fits: the chunk grows)
constexpr size_t CHUNK_GENOMES = 4096;       // bounds the HV read-back of a chunk of tiny genomes (32 MiB at D = 4096)
constexpr size_t SMALL_BYTES = 256u << 10;   // genomes below this are packed into page-locked staging and uploaded together
constexpr size_t CHUNK_SLACK = 64;           // readable bytes an area keeps behind its last region
constexpr size_t TEXT_AREA_MIN = CHUNK_BYTES + CHUNK_SLACK;  // the ASCII buffer every chunk is opened with
constexpr size_t PACKED_AREA_MIN = CHUNK_BYTES * 3 / 2 + (1u << 20);  // (a chunk of blobs uploads up to CHUNK_BYTES; sparse ones add their rebuilt bitmaps)

enum : int { KIND_ASCII = 0, KIND_PACK2 = 1, KIND_PACK2S = 2 };
struct StreamItem {
  const uint8_t *seq;  // ASCII sequence, a hg_pack2 blob (KIND_PACK2) or a hg_pack2s blob (KIND_PACK2S)
  size_t len;          // bases
  uint64_t tag;
  int kind;
  size_t blob_bytes;   // KIND_PACK2S: bytes of the host blob (codes + run table)
  size_t padded() const { return (len + 15) & ~(size_t)15; }
  // what the genome moves over the link (and what a chunk of blobs is sized by): its ASCII bytes or its blob
  size_t link() const { return kind == KIND_ASCII ? padded() : kind == KIND_PACK2 ? hg_pack2_code_bytes(len) + hg_pack2_mask_bytes(len) : blob_bytes; }
};

// Chunk size ramp: after the input ran dry the first chunk of a new burst closes at CHUNK_BYTES / 8 and every
// further one at twice the previous size (up to CHUNK_BYTES), so that the kernels start ~0.15 ms after the burst
// does instead of after a whole 64 MB upload -- with a burst of a few hundred genomes that idle start was a fifth
// of the pass (256 genomes x 1.25 MB: 28.7 k genomes/s; the bench's packed_stream leg)
struct ChunkLimit {
  size_t bytes = CHUNK_BYTES / 8;
  void new_burst() { bytes = CHUNK_BYTES / 8; }  // (the uploader is about to wait with nothing open)
  void chunk_closed() { bytes = std::min(CHUNK_BYTES, 2 * bytes); }
};

struct ChunkPlace {  // where one genome's bytes go, and what the chunk's areas must hold before its copy is issued
  enum Area : int { NONE, STAGE, TEXT, PACKED } area = NONE;  // NONE: an empty genome; STAGE: the page-locked mirror of TEXT
  size_t off = 0, n = 0;  // the copy: n bytes to `off` of the area (STAGE: memcpy, zeros up to the next multiple of 16; TEXT: the pending run first)
  // An area smaller than `need` (0: the genome does not touch it) is replaced by one of `want` bytes that keeps the first `keep`
  // bytes.  The ASCII buffer has nothing to keep: it grows for one genome larger than the chunk, which the closing rule lets
  // only into a chunk without bytes.  The packed area of a chunk sized by its blobs grows before its first blob only; one sized
  // by ASCII bytes can outgrow it with blobs in place (a hg_pack2s run table may be several times the genome's ASCII).
  size_t text_need = 0, text_want = 0, packed_need = 0, packed_want = 0, packed_keep = 0;
};

struct ChunkLayout {
  std::vector<uint64_t> offs, lens, tags;    // per genome: its ASCII region in the sequence buffer (offs: padded to 16)
  std::vector<uint64_t> pk_offs, mask_offs;  // per genome: its codes / its not-a-base bitmap in the packed area (0: ASCII or empty)
  size_t bytes = 0;                // padded ASCII-equivalent bytes of all genomes, whatever they came as
  size_t pk_bytes = 0, link_bytes = 0;  // the packed area's fill; bytes this chunk moves over the link
  size_t run_lo = 0, run_hi = 0;   // pending run of small ASCII genomes in the staging mirror
  uint32_t n_jobs = 0, n_blocks = 0;    // UnpackJob records (one per non-empty blob) and the grid of unpack2_kernel
  uint32_t n_sjobs = 0, n_sblocks = 0;  // SparseJob records (hg_pack2s genomes) and the grid of expand_runs_kernel
  uint32_t n_text = 0;             // non-empty genomes that arrived as ASCII
  bool has_ascii = false;          // some genome arrived as ASCII, empty or not: the chunk is sized by `bytes`
  // A chunk of blobs only goes to the packed-input kernels as it is; one that mixes blobs and ASCII genomes has its
  // blobs expanded into the sequence buffer by unpack2_kernel first.  (Empty genomes have no bytes of either form.)
  bool packed_only() const { return n_jobs > 0 && n_text == 0; }

  // Does `it` close the chunk before it is added?  A chunk that holds (or is about to hold) ASCII genomes is bounded by
  // its ASCII buffer; a chunk of blobs only never touches that and is bounded by the bytes it uploads -- three to four
  // times as many genomes per chunk, so that the fixed cost of a chunk (two stream synchronisations, ~0.3 ms) is shared
  // by more of them
  bool closes_before(const StreamItem &it, const ChunkLimit &limit) const {
    return !tags.empty() && (has_ascii || it.kind == KIND_ASCII ? bytes + it.padded() : link_bytes + it.link()) > limit.bytes;
  }
  // ... and after the last add?  When it is full -- or when nothing else is waiting: the kernels start at once and the
  // next genome opens a new chunk.  (A/B: keeping the chunk open while the kernels are busy halves the number of
  // chunks and is 7-10 % slower end to end -- results come back later, the readers' buffers free up later.)
  bool closes_after(bool idle, const ChunkLimit &limit) const {
    return idle || (has_ascii ? bytes : link_bytes) >= limit.bytes || tags.size() >= CHUNK_GENOMES;
  }
  void take_run(size_t &lo, size_t &hi) { lo = run_lo, hi = run_hi, run_lo = run_hi = 0; }  // (the caller uploads it)
  // Adds a genome; a non-empty blob gets its record in jobs[] (and sjobs[]: CHUNK_GENOMES entries each).
  ChunkPlace add(const StreamItem &it, UnpackJob *jobs, SparseJob *sjobs) {
    ChunkPlace pl;
    const size_t padded = it.padded();
    uint64_t pk_off = 0, mask_off = 0;
    if (it.kind == KIND_ASCII) has_ascii = true;
    if (has_ascii) pl.text_need = bytes + padded + CHUNK_SLACK, pl.text_want = padded + padded / 8 + CHUNK_SLACK;
    if (it.len && it.kind != KIND_ASCII) {
      const size_t mbytes = hg_pack2_mask_bytes(it.len);
      // device region: hg_pack2 = [codes][bitmap]; hg_pack2s = [codes][run table][bitmap, rebuilt by expand_runs_kernel]
      const size_t blob = it.kind == KIND_PACK2 ? it.link() : it.blob_bytes + mbytes;
      pl.area = ChunkPlace::PACKED, pl.off = pk_bytes, pl.n = it.link();
      pl.packed_need = pk_bytes + blob + CHUNK_SLACK, pl.packed_want = std::max(pl.packed_need + blob / 8, PACKED_AREA_MIN), pl.packed_keep = pk_bytes;
      pk_off = pk_bytes, mask_off = pk_bytes + (blob - mbytes);
      jobs[n_jobs++] = UnpackJob{pk_off, bytes, it.len, mask_off, n_blocks, 0};
      n_blocks += hg_unpack2_blocks(it.len);
      if (it.kind == KIND_PACK2S) {
        sjobs[n_sjobs++] = SparseJob{pk_off, mask_off, it.len, n_sblocks, 0};
        n_sblocks += hg_expand_runs_blocks(it.len);
      }
      pk_bytes += blob;
    } else if (it.len) {
      pl.area = it.len < SMALL_BYTES && bytes + padded <= CHUNK_BYTES ? ChunkPlace::STAGE : ChunkPlace::TEXT;
      if (pl.area == ChunkPlace::STAGE) run_lo = run_hi == run_lo ? bytes : run_lo, run_hi = bytes + padded;  // (joins the run)
      pl.off = bytes, pl.n = it.len, ++n_text;
    }
    offs.push_back(bytes), lens.push_back(it.len), tags.push_back(it.tag), pk_offs.push_back(pk_off), mask_offs.push_back(mask_off);
    bytes += padded, link_bytes += it.link();
    return pl;
  }
};
