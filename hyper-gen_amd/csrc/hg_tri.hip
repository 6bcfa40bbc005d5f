// hg_tri.hip -- the C ABI of include/hypergen_tri.h (libhypergen_tri.so): the ANI matrix of one set of sketches as fixed-width
// text.  The kernel is hg_tri_kernels.hip's; here are the offset arithmetic, the argument checks and the two drivers that walk
// the set in row blocks of hg_dist_full_dev in the scratch block the search and matrix calls of the ctx use, each block
// formatted behind its GEMM on the same stream: hg_tri_dev keeps the text on the device, hg_tri_stream_dev sends every block
// through one of two page-locked buffers to the caller while the next one is computed.
#include <algorithm>

#include "hg_internal.h"
#include "hg_tri.h"

namespace {

const char *const KERNEL_NAMES = "tri_format_kernel";

struct DevMem {  // hg_dev_alloc'ed, freed with the object
  hg_ctx *c;
  void *p = nullptr;
  explicit DevMem(hg_ctx *ctx) : c(ctx) {}
  ~DevMem() {
    if (p) (void)hg_dev_free(c, p);
  }
  hg_status alloc(size_t bytes) { return hg_dev_alloc(c, std::max<size_t>(bytes, 16), &p); }
};

uint64_t tri_fields(uint64_t i) { return i ? i * (i - 1) / 2 : 0; }  // the fields of the rows in front of row i under LOWER

hg_status check_text(hg_ctx *c, uint32_t layout, const void *text) {
  if (layout > HG_TRI_FULL) return hg_fail(c, HG_ERR_INVALID, "layout must be HG_TRI_LOWER or HG_TRI_FULL");
  if (!text) return hg_fail(c, HG_ERR_INVALID, "text == NULL");
  if (reinterpret_cast<uintptr_t>(text) & 7) return hg_fail(c, HG_ERR_INVALID, "the text must be 8-byte aligned");
  return HG_OK;
}

// what hg_tri_dev and hg_tri_stream_dev ask of the set (behind the check of their own output)
hg_status check_set(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize, uint32_t layout) {
  if (layout > HG_TRI_FULL) return hg_fail(c, HG_ERR_INVALID, "layout must be HG_TRI_LOWER or HG_TRI_FULL");
  if (n >= ((size_t)1 << 31)) return hg_fail(c, HG_ERR_UNSUPPORTED, "n must be < 2^31");
  if (hv_d == 0 || hv_d > 65536) return hg_fail(c, HG_ERR_UNSUPPORTED, "hv_d must be in 1..65536");
  if (ksize == 0) return hg_fail(c, HG_ERR_INVALID, "ksize must be >= 1");
  if (layout == HG_TRI_LOWER && c->ani_metric == HG_ANI_CONTAINMENT)
    return hg_fail(c, HG_ERR_INVALID, "HG_TRI_LOWER with HG_ANI_CONTAINMENT: the metric is directional");
  if (n && (!d_hv || !d_norm2)) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  return HG_OK;
}

// the rows of a block: the caller's, or as many as fit `budget` bytes at `per_pair` bytes a pair of a full-width row -- whole
// GEMM row tiles (256 rows) where several fit, one row at the least.  hg_tri_dev fills the scratch block of the matrix
// (HG_SEARCH_BLOCK_BYTES of floats, as hg_hist_dev does: the GEMM runs at its rate on blocks of thousands of rows and at less
// than half of it on blocks of 256); hg_tri_stream_dev is bound by the link and holds four buffers of a block's text, so its
// block is HG_TRI_TEXT_BLOCK_BYTES of text.
size_t rows_per_block(size_t n, size_t forced, size_t budget, size_t per_pair) {
  if (forced) return std::min(n, forced);
  size_t fit = std::max<size_t>(1, budget / (per_pair * n));
  if (fit >= 256) fit -= fit % 256;
  return std::min(n, fit);
}

// one block of the set behind the checks and HG_ENTER: its GEMM into d_blk, its text to d_text.  LOWER computes the columns in
// front of the block's last row only; the block of row 0 alone has none and queues nothing.
hg_status queue_block(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize, uint32_t layout, size_t r0,
                      size_t rows, float *d_blk, char *d_text) {
  const size_t cols = layout == HG_TRI_LOWER ? r0 + rows - 1 : n;
  if (!cols) return HG_OK;
  const hg_status s = hg_dist_full_dev(c, d_hv + r0 * (size_t)hv_d, d_norm2 + r0, rows, d_hv, d_norm2, cols, hv_d, ksize, d_blk);
  if (s != HG_OK) return s;
  hg_timed tm(c, HG_T_DIST);
  HG_HIP(c, hg_tri_launch_format(c->stream, d_blk, (uint32_t)rows, (uint32_t)cols, cols, (uint32_t)r0, layout, d_text));
  return HG_OK;
}

// the two buffers on either side of the link, the events between the streams: released with the object
struct StreamState {
  hg_ctx *c;
  DevMem d_text[2];
  char *h_text[2] = {nullptr, nullptr};
  hipEvent_t formatted[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
  explicit StreamState(hg_ctx *ctx) : c(ctx), d_text{DevMem(ctx), DevMem(ctx)} {}
  ~StreamState() {
    for (int k = 0; k < 2; ++k) {
      if (h_text[k]) (void)hipHostFree(h_text[k]);
      if (formatted[k]) (void)hipEventDestroy(formatted[k]);
      if (copied[k]) (void)hipEventDestroy(copied[k]);
    }
  }
  hg_status open(size_t bytes) {
    if (!c->copy_stream) HG_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (int k = 0; k < 2; ++k) {
      const hg_status s = d_text[k].alloc(bytes);
      if (s != HG_OK) return s;
      if (hipHostMalloc(reinterpret_cast<void **>(&h_text[k]), std::max<size_t>(bytes, 16), hipHostMallocDefault) != hipSuccess) {
        h_text[k] = nullptr;
        (void)hipGetLastError();
        return hg_fail(c, HG_ERR_OOM, "page-locked text buffer");
      }
      HG_HIP(c, hipEventCreateWithFlags(&formatted[k], hipEventDisableTiming));
      HG_HIP(c, hipEventCreateWithFlags(&copied[k], hipEventDisableTiming));
    }
    return HG_OK;
  }
};

}  // namespace

extern "C" uint64_t hg_tri_text_bytes(uint32_t layout, uint64_t row0, uint64_t rows, uint64_t cols) {
  if (layout == HG_TRI_LOWER) return HG_TRI_FIELD_BYTES * (tri_fields(row0 + rows) - tri_fields(row0));
  return layout == HG_TRI_FULL ? HG_TRI_FIELD_BYTES * rows * cols : 0;
}
extern "C" uint64_t hg_tri_field_offset(uint32_t layout, uint64_t row0, uint64_t i, uint64_t j, uint64_t cols) {
  if (layout == HG_TRI_LOWER) return HG_TRI_FIELD_BYTES * (tri_fields(i) - tri_fields(row0) + j);
  return layout == HG_TRI_FULL ? HG_TRI_FIELD_BYTES * ((i - row0) * cols + j) : 0;
}
extern "C" uint32_t hg_tri_tile_rows(void) { return HG_TRI_TILE_ROWS; }
extern "C" uint32_t hg_tri_tile_cols(void) { return HG_TRI_TILE_COLS; }
extern "C" uint32_t hg_tri_threads(void) { return HG_TRI_THREADS; }
extern "C" const char *hg_tri_kernel_names(void) { return KERNEL_NAMES; }
extern "C" uint32_t hg_tri_launch_counts(uint64_t *counts, uint32_t cap) {
  for (uint32_t k = 0; counts && k < HG_TRI_N_KERNELS && k < cap; ++k) counts[k] = hg_tri_launches(k);
  return HG_TRI_N_KERNELS;
}

extern "C" hg_status hg_tri_format_dev(hg_ctx *c, const float *d_ani, size_t rows, size_t cols, size_t pitch, size_t row0, uint32_t layout,
                                       char *d_text) {
  if (!c) return HG_ERR_INVALID;
  const hg_status s = check_text(c, layout, d_text);
  if (s != HG_OK) return s;
  const size_t lim = (size_t)1 << 31;
  if (rows > lim || cols > lim || row0 > lim || row0 + rows > lim) return hg_fail(c, HG_ERR_UNSUPPORTED, "global indices must be < 2^31");
  if (rows == 0 || cols == 0) return HG_OK;
  if (!d_ani) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (reinterpret_cast<uintptr_t>(d_ani) & 3) return hg_fail(c, HG_ERR_INVALID, "the matrix must be 4-byte aligned");
  if (pitch < cols) return hg_fail(c, HG_ERR_INVALID, "pitch < cols");
  if (layout == HG_TRI_LOWER && cols < row0 + rows - 1) return hg_fail(c, HG_ERR_INVALID, "HG_TRI_LOWER needs cols >= row0 + rows - 1");
  HG_ENTER(c);
  if (layout == HG_TRI_LOWER && row0 + rows == 1) return HG_OK;  // row 0 alone: no field
  hg_timed tm(c, HG_T_DIST);
  HG_HIP(c, hg_tri_launch_format(c->stream, d_ani, (uint32_t)rows, (uint32_t)cols, pitch, (uint32_t)row0, layout, d_text));
  return HG_OK;
}

extern "C" hg_status hg_tri_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize, uint32_t layout,
                                size_t block_rows, char *d_text) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_text(c, layout, d_text);
  if (s != HG_OK || (s = check_set(c, d_hv, d_norm2, n, hv_d, ksize, layout)) != HG_OK) return s;
  HG_ENTER(c);
  if (n) {
    const size_t rb = rows_per_block(n, block_rows, HG_SEARCH_BLOCK_BYTES, sizeof(float));
    if ((s = hg_ensure(c, c->w_srch_blk, rb * n * sizeof(float))) != HG_OK) return s;
    float *d_blk = static_cast<float *>(c->w_srch_blk.p);
    for (size_t r0 = 0; r0 < n; r0 += rb)
      if ((s = queue_block(c, d_hv, d_norm2, n, hv_d, ksize, layout, r0, std::min(rb, n - r0), d_blk, d_text + hg_tri_field_offset(layout, 0, r0, 0, n))) != HG_OK)
        return s;
  }
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

extern "C" hg_status hg_tri_stream_dev(hg_ctx *c, const int16_t *d_hv, const int32_t *d_norm2, size_t n, uint32_t hv_d, uint32_t ksize,
                                       uint32_t layout, size_t block_rows, hg_tri_sink sink, void *user) {
  if (!c) return HG_ERR_INVALID;
  if (!sink) return hg_fail(c, HG_ERR_INVALID, "sink == NULL");
  hg_status s = check_set(c, d_hv, d_norm2, n, hv_d, ksize, layout);
  if (s != HG_OK) return s;
  HG_ENTER(c);
  if (!n) return HG_OK;
  const size_t rb = rows_per_block(n, block_rows, HG_TRI_TEXT_BLOCK_BYTES, HG_TRI_FIELD_BYTES), n_blocks = (n + rb - 1) / rb;
  auto rows_of = [&](size_t b) { return std::min(rb, n - b * rb); };
  auto bytes_of = [&](size_t b) { return (size_t)hg_tri_text_bytes(layout, b * rb, rows_of(b), n); };
  // (the largest block: the first under FULL, one of the last two under LOWER)
  const size_t most = std::max(bytes_of(0), std::max(bytes_of(n_blocks - 1), bytes_of(n_blocks > 1 ? n_blocks - 2 : 0)));
  StreamState st(c);
  if ((s = st.open(most)) != HG_OK || (s = hg_ensure(c, c->w_srch_blk, rb * n * sizeof(float))) != HG_OK) return s;
  float *d_blk = static_cast<float *>(c->w_srch_blk.p);
  // block b: GEMM and format on the ctx's stream into d_text[b & 1], the copy into h_text[b & 1] on the copy stream behind
  // `formatted`.  Both buffers of a pair are free when this runs: the host has waited for `copied` of block b - 2 and its sink
  // has returned.
  auto queue = [&](size_t b) -> hg_status {
    const int k = (int)(b & 1);
    const hg_status qs = queue_block(c, d_hv, d_norm2, n, hv_d, ksize, layout, b * rb, rows_of(b), d_blk, static_cast<char *>(st.d_text[k].p));
    if (qs != HG_OK || !bytes_of(b)) return qs;
    HG_HIP(c, hipEventRecord(st.formatted[k], c->stream));
    HG_HIP(c, hipStreamWaitEvent(c->copy_stream, st.formatted[k], 0));
    HG_HIP(c, hipMemcpyAsync(st.h_text[k], st.d_text[k].p, bytes_of(b), hipMemcpyDeviceToHost, c->copy_stream));
    HG_HIP(c, hipEventRecord(st.copied[k], c->copy_stream));
    return HG_OK;
  };
  // whatever ends the loop, nothing of this call is in flight behind it: the buffers go with `st`
  auto drain = [&](hg_status out) {
    const hipError_t e1 = hipStreamSynchronize(c->stream), e2 = hipStreamSynchronize(c->copy_stream);
    if (out == HG_OK && (e1 != hipSuccess || e2 != hipSuccess))
      return hg_fail(c, HG_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    return out;
  };
  if ((s = queue(0)) != HG_OK) return drain(s);
  for (size_t b = 0; b < n_blocks; ++b) {
    if (b + 1 < n_blocks && (s = queue(b + 1)) != HG_OK) return drain(s);
    if (bytes_of(b)) {
      const hipError_t e = hipEventSynchronize(st.copied[b & 1]);
      if (e != hipSuccess) return drain(hg_fail(c, HG_ERR_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(e)));
    }
    if (sink(user, st.h_text[b & 1], bytes_of(b), b * rb, rows_of(b)) != 0) return drain(hg_fail(c, HG_ERR_IO, "the sink refused a block"));
  }
  return drain(HG_OK);
}

extern "C" hg_status hg_tri(hg_ctx *c, const int16_t *hv, const int32_t *norm2, size_t n, uint32_t hv_d, uint32_t ksize, uint32_t layout, char *text) {
  if (!c) return HG_ERR_INVALID;
  if (layout > HG_TRI_FULL) return hg_fail(c, HG_ERR_INVALID, "layout must be HG_TRI_LOWER or HG_TRI_FULL");
  if (!text) return hg_fail(c, HG_ERR_INVALID, "text == NULL");
  if (n >= ((size_t)1 << 31)) return hg_fail(c, HG_ERR_UNSUPPORTED, "n must be < 2^31");
  if (n && (!hv || !norm2)) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  const size_t text_bytes = (size_t)hg_tri_text_bytes(layout, 0, n, n);
  DevMem d_hv(c), d_n2(c), d_text(c);
  hg_status s;
  if ((s = d_hv.alloc(n * hv_d * sizeof(int16_t))) != HG_OK || (s = d_n2.alloc(n * sizeof(int32_t))) != HG_OK || (s = d_text.alloc(text_bytes)) != HG_OK)
    return s;
  if (n && ((s = hg_copy_h2d(c, d_hv.p, hv, n * hv_d * sizeof(int16_t))) != HG_OK || (s = hg_copy_h2d(c, d_n2.p, norm2, n * sizeof(int32_t))) != HG_OK))
    return s;
  s = hg_tri_dev(c, static_cast<int16_t *>(d_hv.p), static_cast<int32_t *>(d_n2.p), n, hv_d, ksize, layout, 0, static_cast<char *>(d_text.p));
  if (s != HG_OK || !text_bytes) return s;
  return hg_copy_d2h(c, text, d_text.p, text_bytes);
}
