// hg_rec.hip -- the C ABI of include/hypergen_rec.h (libhypergen_rec.so): one multi-FASTA text split into its records.
// The kernels are hg_rec_kernels.hip's; here are the sequence they are queued in, the two places where the host must read a
// count back before it can go on (the number of records sizes the per-record scratch; the size of the layout is checked
// against the caller's buffer before a byte is scattered), the host's own reading of the specification, the file reader and
// the per-record sketch loop.  Scratch lives in workspaces of the ctx that only the search and matrix calls use otherwise.
#include <zlib.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hg_internal.h"
#include "hg_rec.h"

namespace {

const char *const KERNEL_NAMES =
    "rec_block_summary_kernel\nrec_tile_reduce_kernel\nrec_block_prefix_kernel\nrec_mark_kernel\nrec_pad_reduce_kernel\n"
    "rec_pad_scan_kernel\nrec_offsets_kernel\nrec_scatter_kernel";

constexpr uint64_t SUB_BATCH_RECORDS = 65536, SUB_BATCH_BYTES = (uint64_t)1 << 30;

inline uint64_t up4(uint64_t x) { return (x + 3) & ~(uint64_t)3; }
inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
inline uint32_t div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// what the count passes leave on the device for the scatter, and what the host has read of it
struct Split {
  uint32_t n_blk = 0;
  uint64_t n_recs = 0, total = 0, seq_bytes = 0;
  hg_rec_sum *d_pre = nullptr;  // per block: the summary of the text in front of it
  uint32_t *d_cidx = nullptr;   // per record: sequence bytes in front of it; [n_recs]: the text's
  uint64_t *d_ps = nullptr;     // per record: pads behind the records in front of it; [n_recs]: all pads
};

hg_status read_words(hg_ctx *c, uint32_t *host) {
  HG_HIP(c, hipMemcpyAsync(host, c->w_srch_state.p, HG_REC_RES_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

// summaries, their scan, the totals: n_recs and the number of sequence bytes (0 < n < 2^32)
hg_status count_blocks(hg_ctx *c, const uint8_t *d_text, size_t n, Split &sp) {
  sp.n_blk = div_up(n, HG_REC_BLOCK);
  const uint32_t n_tiles = div_up(sp.n_blk, HG_REC_TILE);
  hg_status s;
  if ((s = hg_ensure(c, c->w_srch_blk, ((size_t)sp.n_blk + n_tiles) * sizeof(hg_rec_sum))) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_srch_state, HG_REC_RES_WORDS * sizeof(uint32_t))) != HG_OK) return s;
  sp.d_pre = static_cast<hg_rec_sum *>(c->w_srch_blk.p);
  hg_rec_sum *d_tile = sp.d_pre + sp.n_blk;
  auto *d_res = static_cast<uint32_t *>(c->w_srch_state.p);
  HG_HIP(c, hg_rec_launch_summary(c->stream, d_text, n, sp.d_pre, sp.n_blk));
  HG_HIP(c, hg_rec_launch_tile_reduce(c->stream, sp.d_pre, sp.n_blk, d_tile, n_tiles));
  HG_HIP(c, hg_rec_launch_prefix(c->stream, sp.d_pre, sp.n_blk, d_tile, n_tiles, d_res));
  uint32_t w[HG_REC_RES_WORDS];
  if ((s = read_words(c, w)) != HG_OK) return s;
  sp.n_recs = w[HG_REC_RES_NRECS], sp.total = w[HG_REC_RES_TOTAL];
  if (!sp.n_recs && sp.total) return hg_fail(c, HG_ERR_IO, "sequence data before the first header");
  return HG_OK;
}

// the record table (d_recs may be NULL) and the offsets: seq_bytes (n_recs > 0)
hg_status count_records(hg_ctx *c, const uint8_t *d_text, size_t n, hg_rec_entry *d_recs, Split &sp) {
  const uint32_t n_recs = (uint32_t)sp.n_recs, n_tiles = div_up(n_recs, HG_REC_PAD_TILE);
  // cidx (n_recs + 1 words, rounded to 8 bytes), ps (n_recs + 1), tile bases (n_tiles), tile sums (n_tiles words)
  const size_t cidx_bytes = (((size_t)n_recs + 1) * 4 + 7) & ~(size_t)7;
  hg_status s = hg_ensure(c, c->w_srch_lists, cidx_bytes + ((size_t)n_recs + 1 + n_tiles) * 8 + (size_t)n_tiles * 4);
  if (s != HG_OK) return s;
  auto *base = static_cast<uint8_t *>(c->w_srch_lists.p);
  sp.d_cidx = reinterpret_cast<uint32_t *>(base);
  sp.d_ps = reinterpret_cast<uint64_t *>(base + cidx_bytes);
  uint64_t *d_tbase = sp.d_ps + n_recs + 1;
  uint32_t *d_tsum = reinterpret_cast<uint32_t *>(d_tbase + n_tiles);
  auto *d_res = static_cast<uint32_t *>(c->w_srch_state.p);
  HG_HIP(c, hg_rec_launch_mark(c->stream, d_text, n, sp.d_pre, sp.n_blk, d_recs, sp.d_cidx, n_recs, d_res));
  HG_HIP(c, hg_rec_launch_pad_reduce(c->stream, sp.d_cidx, n_recs, d_tsum, n_tiles));
  HG_HIP(c, hg_rec_launch_pad_scan(c->stream, d_tsum, d_tbase, n_tiles, d_res));
  HG_HIP(c, hg_rec_launch_offsets(c->stream, sp.d_cidx, n_recs, d_tbase, sp.d_ps, d_recs));
  uint32_t w[HG_REC_RES_WORDS];
  if ((s = read_words(c, w)) != HG_OK) return s;
  if (w[HG_REC_RES_LEAD]) return hg_fail(c, HG_ERR_IO, "sequence data before the first header");
  sp.seq_bytes = sp.total + (((uint64_t)w[HG_REC_RES_PAD_HI] << 32) | w[HG_REC_RES_PAD_LO]);
  return HG_OK;
}

hg_status check_text(hg_ctx *c, const uint8_t *d_text, size_t n, size_t *n_recs, size_t *seq_bytes) {
  if (!n_recs || !seq_bytes) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  *n_recs = 0, *seq_bytes = 0;
  if ((uint64_t)n >= ((uint64_t)1 << 32)) return hg_fail(c, HG_ERR_UNSUPPORTED, "a text of 2^32 bytes or more");
  if (n && !d_text) return hg_fail(c, HG_ERR_INVALID, "NULL text");
  if (reinterpret_cast<uintptr_t>(d_text) & 15) return hg_fail(c, HG_ERR_INVALID, "the text must be 16-byte aligned");
  return HG_OK;
}

// count, check the capacities, scatter: hg_rec_split_dev behind its argument checks and HG_ENTER
hg_status split_dev(hg_ctx *c, const uint8_t *d_text, size_t n, uint8_t *d_seq, size_t seq_cap, hg_rec_entry *d_recs, size_t rec_cap,
                    size_t *n_recs, size_t *seq_bytes) {
  Split sp;
  hg_status s = count_blocks(c, d_text, n, sp);
  if (s != HG_OK) return s;
  if (sp.n_recs && (s = count_records(c, d_text, n, sp.n_recs <= rec_cap ? d_recs : nullptr, sp)) != HG_OK) return s;
  *n_recs = sp.n_recs, *seq_bytes = sp.seq_bytes;
  if (sp.n_recs > rec_cap || sp.seq_bytes + 32 > seq_cap) return hg_fail(c, HG_ERR_CAPACITY, "record table or sequence buffer too small");
  if (sp.seq_bytes)
    HG_HIP(c, hg_rec_launch_scatter(c->stream, d_text, n, sp.d_pre, sp.n_blk, sp.d_ps, (uint32_t)sp.n_recs, d_seq, sp.seq_bytes));
  return HG_OK;
}

}  // namespace

extern "C" uint32_t hg_rec_block_bytes(void) { return HG_REC_BLOCK; }
extern "C" const char *hg_rec_kernel_names(void) { return KERNEL_NAMES; }
extern "C" uint32_t hg_rec_launch_counts(uint64_t *counts, uint32_t cap) {
  for (uint32_t k = 0; counts && k < HG_REC_N_KERNELS && k < cap; ++k) counts[k] = hg_rec_launches(k);
  return HG_REC_N_KERNELS;
}

extern "C" hg_status hg_rec_count_dev(hg_ctx *c, const uint8_t *d_text, size_t n, size_t *n_recs, size_t *seq_bytes) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_text(c, d_text, n, n_recs, seq_bytes);
  if (s != HG_OK || n == 0) return s;
  HG_ENTER(c);
  Split sp;
  if ((s = count_blocks(c, d_text, n, sp)) != HG_OK) return s;
  if (sp.n_recs && (s = count_records(c, d_text, n, nullptr, sp)) != HG_OK) return s;
  *n_recs = sp.n_recs, *seq_bytes = sp.seq_bytes;
  return HG_OK;
}

extern "C" hg_status hg_rec_split_dev(hg_ctx *c, const uint8_t *d_text, size_t n, uint8_t *d_seq, size_t seq_cap, hg_rec_entry *d_recs,
                                      size_t rec_cap, size_t *n_recs, size_t *seq_bytes) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_text(c, d_text, n, n_recs, seq_bytes);
  if (s != HG_OK) return s;
  if ((seq_cap && !d_seq) || (rec_cap && !d_recs)) return hg_fail(c, HG_ERR_INVALID, "NULL output");
  if ((reinterpret_cast<uintptr_t>(d_seq) | reinterpret_cast<uintptr_t>(d_recs)) & 15)
    return hg_fail(c, HG_ERR_INVALID, "the outputs must be 16-byte aligned");
  if (n == 0) return seq_cap < 32 ? hg_fail(c, HG_ERR_CAPACITY, "sequence buffer too small") : HG_OK;
  HG_ENTER(c);
  return split_dev(c, d_text, n, d_seq, seq_cap, d_recs, rec_cap, n_recs, seq_bytes);
}

extern "C" hg_status hg_rec_split(hg_ctx *c, const uint8_t *text, size_t n, uint8_t *seq_out, size_t seq_cap, hg_rec_entry *recs_out,
                                  size_t rec_cap, size_t *n_recs, size_t *seq_bytes) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_text(c, nullptr, 0, n_recs, seq_bytes);
  if (s != HG_OK) return s;
  if ((uint64_t)n >= ((uint64_t)1 << 32)) return hg_fail(c, HG_ERR_UNSUPPORTED, "a text of 2^32 bytes or more");
  if ((n && !text) || (seq_cap && !seq_out) || (rec_cap && !recs_out)) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (n == 0) return seq_cap < 32 ? hg_fail(c, HG_ERR_CAPACITY, "sequence buffer too small") : HG_OK;
  HG_ENTER(c);
  if ((s = hg_ensure(c, c->w_seq, up16(n) + 16)) != HG_OK) return s;
  auto *d_text = static_cast<uint8_t *>(c->w_seq.p);
  HG_HIP(c, hipMemcpyAsync(d_text, text, n, hipMemcpyHostToDevice, c->stream));
  // the counts first: they size the device side of the outputs
  Split sp;
  if ((s = count_blocks(c, d_text, n, sp)) != HG_OK) return s;
  hg_rec_entry *d_recs = nullptr;
  if (sp.n_recs && sp.n_recs <= rec_cap) {
    if ((s = hg_ensure(c, c->w_hv, sp.n_recs * sizeof(hg_rec_entry))) != HG_OK) return s;
    d_recs = static_cast<hg_rec_entry *>(c->w_hv.p);
  }
  if (sp.n_recs && (s = count_records(c, d_text, n, d_recs, sp)) != HG_OK) return s;
  *n_recs = sp.n_recs, *seq_bytes = sp.seq_bytes;
  if (sp.n_recs > rec_cap || sp.seq_bytes + 32 > seq_cap) return hg_fail(c, HG_ERR_CAPACITY, "record table or sequence buffer too small");
  if (!sp.n_recs) return HG_OK;
  if (sp.seq_bytes) {
    if ((s = hg_ensure(c, c->w_pk, sp.seq_bytes + 32)) != HG_OK) return s;
    auto *d_seq = static_cast<uint8_t *>(c->w_pk.p);
    HG_HIP(c, hg_rec_launch_scatter(c->stream, d_text, n, sp.d_pre, sp.n_blk, sp.d_ps, (uint32_t)sp.n_recs, d_seq, sp.seq_bytes));
    HG_HIP(c, hipMemcpyAsync(seq_out, d_seq, sp.seq_bytes, hipMemcpyDeviceToHost, c->stream));
  }
  HG_HIP(c, hipMemcpyAsync(recs_out, d_recs, sp.n_recs * sizeof(hg_rec_entry), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

// ---- one host thread (no device): the specification, line by line --------------------------------------------------------
extern "C" hg_status hg_rec_split_host(const uint8_t *text, size_t n, uint8_t *seq_out, size_t seq_cap, hg_rec_entry *recs_out,
                                       size_t rec_cap, size_t *n_recs, size_t *seq_bytes) {
  if (!n_recs || !seq_bytes) return HG_ERR_INVALID;
  *n_recs = 0, *seq_bytes = 0;
  if ((uint64_t)n >= ((uint64_t)1 << 32)) return HG_ERR_UNSUPPORTED;
  if ((n && !text) || (seq_cap && !seq_out) || (rec_cap && !recs_out)) return HG_ERR_INVALID;
  size_t r = 0;        // records so far
  uint64_t w = 0;      // end of the layout so far
  uint64_t start = 0;  // where the open record's sequence starts
  auto close_record = [&] {  // the open record's length, and the 'N's up to the next multiple of 4
    if (r <= rec_cap) recs_out[r - 1].seq_len = w - start;
    for (; w & 3; ++w)
      if (w < seq_cap) seq_out[w] = 'N';
  };
  for (size_t i = 0; i < n;) {
    const auto *nl = static_cast<const uint8_t *>(std::memchr(text + i, '\n', n - i));
    const size_t j = nl ? (size_t)(nl - text) : n;
    size_t e = j;
    if (e > i && text[e - 1] == '\r') --e;  // one CR in front of the LF, or as the text's very last byte
    if (e > i && text[i] == '>') {
      if (r) close_record();
      start = w;
      if (r < rec_cap) {
        size_t id = i + 1;
        while (id < e && text[id] > 0x20) ++id;
        recs_out[r] = hg_rec_entry{i, (uint32_t)(e - i), (uint32_t)(id - i - 1), w, 0};
      }
      ++r;
    } else if (e > i) {
      if (!r) return HG_ERR_IO;  // sequence data before the first header
      if (w + (e - i) <= seq_cap) std::memcpy(seq_out + w, text + i, e - i);
      w += e - i;
    }
    i = nl ? j + 1 : j;
  }
  if (r) close_record();
  *n_recs = r, *seq_bytes = w;
  return r > rec_cap || w + 32 > seq_cap ? HG_ERR_CAPACITY : HG_OK;
}

// ---- a file's bytes, gzip inflated, in page-locked memory -----------------------------------------------------------------
extern "C" hg_status hg_rec_read_text(const char *path, uint8_t **pbuf, size_t *pcap, size_t *pn) {
  if (!path || !pbuf || !pcap || !pn) return HG_ERR_INVALID;
  *pn = 0;
  gzFile f = gzopen(path, "rb");  // (reads a file that is not gzip as it is)
  if (!f) return HG_ERR_IO;
  (void)gzbuffer(f, 1u << 20);
  uint8_t *buf = *pbuf;
  size_t cap = buf ? *pcap : 0, n = 0;
  hg_status st = HG_OK;
  auto grow = [&](size_t want) {  // page-locked, the first n bytes kept
    void *nb = nullptr;
    if (hipHostMalloc(&nb, want, hipHostMallocPortable) != hipSuccess || !nb) return false;
    if (buf && n) std::memcpy(nb, buf, n);
    if (buf) (void)hipHostFree(buf);
    buf = static_cast<uint8_t *>(nb), cap = want;
    return true;
  };
  constexpr size_t TAIL = 64, LIMIT = (size_t)1 << 32;
  if (cap < ((size_t)16 << 20) + TAIL && !grow(((size_t)16 << 20) + TAIL)) st = HG_ERR_OOM;
  while (st == HG_OK) {
    if (n + TAIL == cap && !grow(2 * cap)) {
      st = HG_ERR_OOM;
      break;
    }
    const int got = gzread(f, buf + n, (unsigned)std::min<size_t>(cap - TAIL - n, 1u << 30));
    if (got < 0) st = HG_ERR_IO;
    if (got <= 0) break;
    n += (size_t)got;
    if (n >= LIMIT) st = HG_ERR_UNSUPPORTED;
  }
  gzclose(f);
  *pbuf = buf, *pcap = cap;  // the (possibly moved) buffer stays the caller's, also on error
  if (st != HG_OK) return st;
  std::memset(buf + n, 0, TAIL);
  *pn = n;
  return HG_OK;
}

// ---- one sketch per record ------------------------------------------------------------------------------------------------
namespace {
struct DevMem {  // hg_dev_alloc'ed, freed with the object
  hg_ctx *c;
  void *p = nullptr;
  explicit DevMem(hg_ctx *ctx) : c(ctx) {}
  ~DevMem() {
    if (p) (void)hg_dev_free(c, p);
  }
  hg_status alloc(size_t bytes) {
    if (p) (void)hg_dev_free(c, p);
    p = nullptr;
    return hg_dev_alloc(c, bytes, &p);
  }
};
}  // namespace

extern "C" hg_status hg_rec_sketch_text_dev(hg_ctx *c, const uint8_t *d_text, size_t n, const hg_sketch_params *p, uint64_t min_length,
                                            hg_rec_rows_fn rows, void *user, size_t *n_recs, size_t *n_kept) {
  if (!c) return HG_ERR_INVALID;
  if (!p || !rows || !n_recs || !n_kept) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  *n_recs = 0, *n_kept = 0;
  size_t seq_bytes = 0;
  hg_status s = hg_rec_count_dev(c, d_text, n, n_recs, &seq_bytes);
  if (s != HG_OK) return s;
  const size_t R = *n_recs;
  if (R >= ((size_t)1 << 31)) return hg_fail(c, HG_ERR_UNSUPPORTED, "2^31 records or more in one text");
  std::vector<hg_rec_entry> recs(R);
  if (!R) return rows(user, recs.data(), 0, nullptr, 0, nullptr, nullptr, nullptr) ? hg_fail(c, HG_ERR_INVALID, "the rows callback failed") : HG_OK;
  DevMem d_seq(c), d_recs(c), d_out(c);
  if ((s = d_seq.alloc(seq_bytes + 32)) != HG_OK || (s = d_recs.alloc(R * sizeof(hg_rec_entry))) != HG_OK) return s;
  size_t got_recs = 0, got_bytes = 0;
  s = hg_rec_split_dev(c, d_text, n, static_cast<uint8_t *>(d_seq.p), seq_bytes + 32, static_cast<hg_rec_entry *>(d_recs.p), R, &got_recs,
                       &got_bytes);
  if (s != HG_OK) return s;
  if ((s = hg_copy_d2h(c, recs.data(), d_recs.p, R * sizeof(hg_rec_entry))) != HG_OK) return s;
  if (rows(user, recs.data(), R, nullptr, 0, nullptr, nullptr, nullptr)) return hg_fail(c, HG_ERR_INVALID, "the rows callback failed");
  // the records that are sketched, decided on the host from the table
  std::vector<uint32_t> kept;
  for (size_t r = 0; r < R; ++r)
    if (recs[r].seq_len >= min_length) kept.push_back((uint32_t)r);
  *n_kept = kept.size();
  // consecutive ranges of them: at most SUB_BATCH_RECORDS records or SUB_BATCH_BYTES of sequence (a longer record goes alone)
  const size_t hv_d = p->hv_d;
  std::vector<uint64_t> offs, lens;
  std::vector<int16_t> hv;
  std::vector<int32_t> n2;
  std::vector<uint32_t> nh;
  size_t out_rows = 0;
  for (size_t k0 = 0; k0 < kept.size();) {
    offs.clear(), lens.clear();
    uint64_t bytes = 0;
    size_t k1 = k0;
    while (k1 < kept.size() && k1 - k0 < SUB_BATCH_RECORDS && (k1 == k0 || bytes + recs[kept[k1]].seq_len <= SUB_BATCH_BYTES)) {
      offs.push_back(recs[kept[k1]].seq_off), lens.push_back(recs[kept[k1]].seq_len);
      bytes += recs[kept[k1]].seq_len, ++k1;
    }
    const size_t m = k1 - k0, hv_bytes = (m * hv_d * sizeof(int16_t) + 15) & ~(size_t)15;
    if (m > out_rows) {
      if ((s = d_out.alloc(hv_bytes + m * 8 + 64)) != HG_OK) return s;
      out_rows = m;
    }
    auto *d_hv = static_cast<int16_t *>(d_out.p);
    auto *d_n2 = reinterpret_cast<int32_t *>(static_cast<uint8_t *>(d_out.p) + hv_bytes);
    auto *d_nh = reinterpret_cast<uint32_t *>(d_n2 + m);
    if ((s = hg_sketch_batch_dev(c, static_cast<const uint8_t *>(d_seq.p), offs.data(), lens.data(), m, p, d_hv, d_n2, d_nh)) != HG_OK) return s;
    if ((s = hg_ctx_sync(c)) != HG_OK) return s;  // the step is deferred: no row is final before this
    hv.resize(m * hv_d), n2.resize(m), nh.resize(m);
    if ((s = hg_copy_d2h(c, hv.data(), d_hv, m * hv_d * sizeof(int16_t))) != HG_OK) return s;
    if ((s = hg_copy_d2h(c, n2.data(), d_n2, m * sizeof(int32_t))) != HG_OK) return s;
    if ((s = hg_copy_d2h(c, nh.data(), d_nh, m * sizeof(uint32_t))) != HG_OK) return s;
    if (rows(user, recs.data(), R, kept.data() + k0, m, hv.data(), n2.data(), nh.data())) return hg_fail(c, HG_ERR_INVALID, "the rows callback failed");
    k0 = k1;
  }
  return HG_OK;
}
