// hg_hist.hip -- the C ABI of include/hypergen_hist.h (libhypergen_hist.so): the histogram of the ANI values of a comparison.
// The kernel is hg_hist_kernels.hip's; here are the argument checks, the test of a block against the selection and the
// driver that streams the matrix: row blocks of hg_dist_full_dev in the scratch block the search and matrix calls of the ctx
// use, each counted behind its GEMM on the same stream.
#include <algorithm>

#include "hg_hist.h"
#include "hg_internal.h"

namespace {

const char *const KERNEL_NAMES = "hist_count_kernel";

struct DevMem {  // hg_dev_alloc'ed, freed with the object
  hg_ctx *c;
  void *p = nullptr;
  explicit DevMem(hg_ctx *ctx) : c(ctx) {}
  ~DevMem() {
    if (p) (void)hg_dev_free(c, p);
  }
  hg_status alloc(size_t bytes) { return hg_dev_alloc(c, std::max<size_t>(bytes, 16), &p); }
};

hg_status check_table(hg_ctx *c, uint32_t pairs, uint32_t bin_milli, const void *counts) {
  if (pairs > HG_HIST_OFFDIAG) return hg_fail(c, HG_ERR_INVALID, "pairs must be HG_HIST_ALL, HG_HIST_UPPER or HG_HIST_OFFDIAG");
  if (!hg_hist_bins(bin_milli)) return hg_fail(c, HG_ERR_INVALID, "bin_milli must be in 1..100000");
  if (!counts) return hg_fail(c, HG_ERR_INVALID, "counts == NULL");
  if (reinterpret_cast<uintptr_t>(counts) & 7) return hg_fail(c, HG_ERR_INVALID, "the counts must be 8-byte aligned");
  return HG_OK;
}

// does the block of global rows [row0, row0 + rows) and columns [col0, col0 + cols), neither empty, hold a selected pair?
bool meets_selection(uint32_t pairs, size_t rows, size_t cols, size_t row0, size_t col0) {
  if (pairs == HG_HIST_UPPER) return row0 < col0 + cols - 1;                          // its first row against its last column
  if (pairs == HG_HIST_OFFDIAG) return !(rows == 1 && cols == 1 && row0 == col0);  // all of it on the diagonal: one element
  return true;
}

// one block behind the checks and HG_ENTER
hg_status add_block(hg_ctx *c, const float *d_ani, size_t rows, size_t cols, size_t pitch, size_t row0, size_t col0, uint32_t pairs,
                    uint32_t bin_milli, uint64_t *d_counts) {
  if (!meets_selection(pairs, rows, cols, row0, col0)) return HG_OK;
  hg_timed tm(c, HG_T_DIST);
  HG_HIP(c, hg_hist_launch_count(c->stream, d_ani, (uint32_t)rows, (uint32_t)cols, pitch, (uint32_t)row0, (uint32_t)col0, pairs, bin_milli,
                                 reinterpret_cast<unsigned long long *>(d_counts)));
  return HG_OK;
}

}  // namespace

extern "C" uint32_t hg_hist_bins(uint32_t bin_milli) { return bin_milli >= 1 && bin_milli <= HG_HIST_MILLI_MAX ? HG_HIST_MILLI_MAX / bin_milli + 1 : 0; }
extern "C" uint32_t hg_hist_lds_bins(void) { return HG_HIST_LDS_BINS; }
extern "C" uint32_t hg_hist_tile_rows(void) { return HG_HIST_TILE_ROWS; }
extern "C" uint32_t hg_hist_tile_cols(void) { return HG_HIST_TILE_COLS; }
extern "C" uint32_t hg_hist_threads(void) { return HG_HIST_THREADS; }
extern "C" const char *hg_hist_kernel_names(void) { return KERNEL_NAMES; }
extern "C" uint32_t hg_hist_launch_counts(uint64_t *counts, uint32_t cap) {
  for (uint32_t k = 0; counts && k < HG_HIST_N_KERNELS && k < cap; ++k) counts[k] = hg_hist_launches(k);
  return HG_HIST_N_KERNELS;
}

extern "C" hg_status hg_hist_add_matrix_dev(hg_ctx *c, const float *d_ani, size_t rows, size_t cols, size_t pitch, size_t row0, size_t col0,
                                            uint32_t pairs, uint32_t bin_milli, uint64_t *d_counts) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_table(c, pairs, bin_milli, d_counts);
  if (s != HG_OK) return s;
  const size_t lim = (size_t)1 << 31;
  if (rows > lim || cols > lim || row0 > lim || col0 > lim || row0 + rows > lim || col0 + cols > lim)
    return hg_fail(c, HG_ERR_UNSUPPORTED, "global indices must be < 2^31");
  if (rows == 0 || cols == 0) return HG_OK;
  if (!d_ani) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (reinterpret_cast<uintptr_t>(d_ani) & 3) return hg_fail(c, HG_ERR_INVALID, "the matrix must be 4-byte aligned");
  if (pitch < cols) return hg_fail(c, HG_ERR_INVALID, "pitch < cols");
  HG_ENTER(c);
  return add_block(c, d_ani, rows, cols, pitch, row0, col0, pairs, bin_milli, d_counts);
}

extern "C" hg_status hg_hist_dev(hg_ctx *c, const int16_t *d_ref_hv, const int32_t *d_ref_norm2, size_t R, const int16_t *d_qry_hv,
                                 const int32_t *d_qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, uint32_t pairs, uint32_t bin_milli,
                                 size_t block_rows, uint64_t *d_counts) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_table(c, pairs, bin_milli, d_counts);
  if (s != HG_OK) return s;
  if (R >= ((size_t)1 << 31) || Q >= ((size_t)1 << 31)) return hg_fail(c, HG_ERR_UNSUPPORTED, "R, Q must be < 2^31");
  if (hv_d == 0 || hv_d > 65536) return hg_fail(c, HG_ERR_UNSUPPORTED, "hv_d must be in 1..65536");
  if (ksize == 0) return hg_fail(c, HG_ERR_INVALID, "ksize must be >= 1");
  if (pairs != HG_HIST_ALL && !(d_ref_hv == d_qry_hv && d_ref_norm2 == d_qry_norm2 && R == Q))
    return hg_fail(c, HG_ERR_INVALID, "HG_HIST_UPPER and HG_HIST_OFFDIAG need the same set on both sides");
  if (pairs == HG_HIST_UPPER && c->ani_metric == HG_ANI_CONTAINMENT)
    return hg_fail(c, HG_ERR_INVALID, "HG_HIST_UPPER with HG_ANI_CONTAINMENT: the metric is directional");
  if (R && Q && (!d_ref_hv || !d_ref_norm2 || !d_qry_hv || !d_qry_norm2)) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  HG_HIP(c, hipMemsetAsync(d_counts, 0, (size_t)hg_hist_bins(bin_milli) * sizeof(uint64_t), c->stream));
  if (R && Q) {
    const size_t fit = std::max<size_t>(1, HG_SEARCH_BLOCK_BYTES / (sizeof(float) * Q));
    const size_t rb = std::min<size_t>(R, block_rows ? block_rows : fit);
    if ((s = hg_ensure(c, c->w_srch_blk, rb * Q * sizeof(float))) != HG_OK) return s;
    float *d_blk = static_cast<float *>(c->w_srch_blk.p);
    for (size_t r0 = 0; r0 < R; r0 += rb) {
      const size_t rows = std::min(rb, R - r0);
      // UPPER: the columns in front of the block's first row hold no i < j -- the GEMM starts at column r0
      const size_t q0 = pairs == HG_HIST_UPPER ? r0 : 0, cols = Q - q0;
      if (pairs == HG_HIST_UPPER && cols < 2) break;  // (the last row alone: only its own diagonal element is left)
      if ((s = hg_dist_full_dev(c, d_ref_hv + r0 * (size_t)hv_d, d_ref_norm2 + r0, rows, d_qry_hv + q0 * (size_t)hv_d, d_qry_norm2 + q0, cols,
                                hv_d, ksize, d_blk)) != HG_OK)
        return s;
      if ((s = add_block(c, d_blk, rows, cols, cols, r0, q0, pairs, bin_milli, d_counts)) != HG_OK) return s;
    }
  }
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

extern "C" hg_status hg_hist(hg_ctx *c, const int16_t *ref_hv, const int32_t *ref_norm2, size_t R, const int16_t *qry_hv,
                             const int32_t *qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, uint32_t pairs, uint32_t bin_milli,
                             uint64_t *counts) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_table(c, pairs, bin_milli, counts);
  if (s != HG_OK) return s;
  if (R >= ((size_t)1 << 31) || Q >= ((size_t)1 << 31)) return hg_fail(c, HG_ERR_UNSUPPORTED, "R, Q must be < 2^31");
  if (R && Q && (!ref_hv || !ref_norm2 || !qry_hv || !qry_norm2)) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  const bool same = ref_hv == qry_hv && ref_norm2 == qry_norm2 && R == Q;
  const size_t table_bytes = (size_t)hg_hist_bins(bin_milli) * sizeof(uint64_t);
  DevMem d_rh(c), d_rn(c), d_qh(c), d_qn(c), d_counts(c);
  if ((s = d_rh.alloc(R * hv_d * sizeof(int16_t))) != HG_OK || (s = d_rn.alloc(R * sizeof(int32_t))) != HG_OK ||
      (s = d_counts.alloc(table_bytes)) != HG_OK)
    return s;
  if (!same && ((s = d_qh.alloc(Q * hv_d * sizeof(int16_t))) != HG_OK || (s = d_qn.alloc(Q * sizeof(int32_t))) != HG_OK)) return s;
  if (R && Q) {
    if ((s = hg_copy_h2d(c, d_rh.p, ref_hv, R * hv_d * sizeof(int16_t))) != HG_OK || (s = hg_copy_h2d(c, d_rn.p, ref_norm2, R * sizeof(int32_t))) != HG_OK)
      return s;
    if (!same &&
        ((s = hg_copy_h2d(c, d_qh.p, qry_hv, Q * hv_d * sizeof(int16_t))) != HG_OK || (s = hg_copy_h2d(c, d_qn.p, qry_norm2, Q * sizeof(int32_t))) != HG_OK))
      return s;
  }
  const void *qh = same ? d_rh.p : d_qh.p, *qn = same ? d_rn.p : d_qn.p;
  s = hg_hist_dev(c, static_cast<int16_t *>(d_rh.p), static_cast<int32_t *>(d_rn.p), R, static_cast<const int16_t *>(qh),
                  static_cast<const int32_t *>(qn), Q, hv_d, ksize, pairs, bin_milli, 0, static_cast<uint64_t *>(d_counts.p));
  if (s != HG_OK) return s;
  return hg_copy_d2h(c, counts, d_counts.p, table_bytes);
}
