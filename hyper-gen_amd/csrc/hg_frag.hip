// hg_frag.hip -- the C ABI of include/hypergen_frag.h (libhypergen_frag.so): fragment-wise ANI and aligned fraction.
// The kernels are hg_frag_kernels.hip's; here are the window plan, the windowed sketch loop around hg_sketch_batch_dev and
// the driver of the reduction: the chunk table of the reference genomes, the groups of genomes whose bests fit the scratch
// bound, the row blocks of hg_dist_full_dev inside a group, the fold behind it.  Scratch lives in workspaces of the ctx that
// only the search and matrix calls use otherwise.
#include <algorithm>
#include <cmath>
#include <vector>

#include "hg_frag.h"
#include "hg_internal.h"

namespace {

const char *const KERNEL_NAMES = "frag_best_kernel\nfrag_fold_kernel";

constexpr uint64_t SUB_BATCH_WINDOWS = 65536;
constexpr uint32_t NO_MATCH = 0xFFFFFFFFu;  // an m_th no best reaches: the records of an empty comparison

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
    return hg_dev_alloc(c, std::max<size_t>(bytes, 16), &p);
  }
};

uint32_t milli_threshold(float th) {  // (hg_avg_milli's clamps, on the host)
  if (!(th >= 0.0f)) th = 0.0f;
  if (th > 100.0f) th = 100.0f;
  return (uint32_t)std::rint((double)th * 1000.0);
}

hg_status check_offsets(hg_ctx *c, const uint32_t *first, size_t n, size_t end, const char *what) {
  if (n == 0) return end == 0 ? HG_OK : hg_fail(c, HG_ERR_INVALID, std::string(what) + ": no genome, but rows or columns");
  if (!first) return hg_fail(c, HG_ERR_INVALID, std::string(what) + " == NULL");
  if (first[0] != 0 || first[n] != end) return hg_fail(c, HG_ERR_INVALID, std::string(what) + " must start at 0 and end at the matrix's size");
  for (size_t g = 0; g < n; ++g)
    if (first[g] > first[g + 1]) return hg_fail(c, HG_ERR_INVALID, std::string(what) + " must be ascending");
  return HG_OK;
}

hg_status check_args(hg_ctx *c, size_t R, size_t Q, const uint32_t *ref_first, size_t n_ref, const uint32_t *qry_first, size_t n_qry,
                     const void *d_pair, const void *d_best) {
  if (R >= ((size_t)1 << 31) || Q >= ((size_t)1 << 31)) return hg_fail(c, HG_ERR_UNSUPPORTED, "R, Q must be < 2^31");
  if (n_ref >= ((size_t)1 << 31) || n_qry >= ((size_t)1 << 31)) return hg_fail(c, HG_ERR_UNSUPPORTED, "n_ref, n_qry must be < 2^31");
  hg_status s;
  if ((s = check_offsets(c, ref_first, n_ref, R, "ref_first")) != HG_OK || (s = check_offsets(c, qry_first, n_qry, Q, "qry_first")) != HG_OK) return s;
  if (n_ref && n_qry && !d_pair) return hg_fail(c, HG_ERR_INVALID, "d_pair == NULL");
  if ((reinterpret_cast<uintptr_t>(d_pair) | reinterpret_cast<uintptr_t>(d_best)) & 7) return hg_fail(c, HG_ERR_INVALID, "the outputs must be 8-byte aligned");
  return HG_OK;
}

// where the rows of a block come from: the caller's matrix, or hg_dist_full_dev into the scratch block
struct Source {
  const float *d_ani = nullptr;  // the whole matrix, or nullptr:
  const int16_t *d_ref_hv = nullptr, *d_qry_hv = nullptr;
  const int32_t *d_ref_n2 = nullptr, *d_qry_n2 = nullptr;
  uint32_t hv_d = 0, ksize = 0;
  size_t block_rows = 0;
};

// the reduction behind the argument checks and HG_ENTER
hg_status reduce(hg_ctx *c, const Source &src, size_t R, size_t Q, const uint32_t *ref_first, size_t n_ref, const uint32_t *qry_first,
                 size_t n_qry, float frag_th, hg_frag_pair *d_pair, hg_frag_best *d_best) {
  hg_status s;
  if (n_ref == 0) {
    HG_HIP(c, hipStreamSynchronize(c->stream));
    return HG_OK;
  }
  const bool empty = R == 0 || Q == 0;  // every best is {0, HG_FRAG_NONE}, nothing matches
  const uint32_t m_th = empty ? NO_MATCH : milli_threshold(frag_th);
  // the chunk table, and behind it the column offsets (one query genome of no columns where there is none: the fold is not launched then)
  std::vector<hg_frag_chunk> chunks;
  std::vector<uint32_t> chunk_first(n_ref + 1, 0);  // a genome's first chunk
  for (size_t g = 0; g < n_ref; ++g) {
    chunk_first[g] = (uint32_t)chunks.size();
    for (uint32_t r = ref_first[g]; r < ref_first[g + 1]; r += HG_FRAG_ROW_CHUNK)
      chunks.push_back(hg_frag_chunk{r, std::min(HG_FRAG_ROW_CHUNK, ref_first[g + 1] - r), (uint32_t)g, 0u});
  }
  chunk_first[n_ref] = (uint32_t)chunks.size();
  const size_t chunk_bytes = chunks.size() * sizeof(hg_frag_chunk), qf_bytes = (n_qry + 1) * sizeof(uint32_t);
  if ((s = hg_ensure(c, c->w_srch_state, chunk_bytes + qf_bytes + 64)) != HG_OK) return s;
  auto *d_chunks = static_cast<hg_frag_chunk *>(c->w_srch_state.p);
  auto *d_qf = reinterpret_cast<uint32_t *>(static_cast<char *>(c->w_srch_state.p) + chunk_bytes);
  if (chunk_bytes) HG_HIP(c, hipMemcpyAsync(d_chunks, chunks.data(), chunk_bytes, hipMemcpyHostToDevice, c->stream));
  if (n_qry) HG_HIP(c, hipMemcpyAsync(d_qf, qry_first, qf_bytes, hipMemcpyHostToDevice, c->stream));

  // groups of reference genomes whose keys, 8 bytes x Q each, fit the scratch bound (the caller's d_best holds them all)
  const size_t per_genome = std::max<size_t>(Q, 1) * sizeof(uint64_t);
  const size_t group_max = std::min<size_t>(HG_FRAG_MAX_GRID_Y, d_best ? n_ref : std::max<size_t>(1, HG_SEARCH_BLOCK_BYTES / per_genome));
  unsigned long long *d_keys = nullptr;
  if (!d_best) {
    if ((s = hg_ensure(c, c->w_srch_lists, std::min(group_max, n_ref) * per_genome)) != HG_OK) return s;
    d_keys = static_cast<unsigned long long *>(c->w_srch_lists.p);
  }
  // rows per block of the matrix
  size_t rb = 0;
  float *d_blk = nullptr;
  if (!src.d_ani && !empty) {
    const size_t fit = std::max<size_t>(1, HG_SEARCH_BLOCK_BYTES / (sizeof(float) * Q));
    rb = std::min<size_t>(R, src.block_rows ? src.block_rows : std::min<size_t>(fit, HG_FRAG_MAX_GRID_Y));
    if ((s = hg_ensure(c, c->w_srch_blk, rb * Q * sizeof(float))) != HG_OK) return s;
    d_blk = static_cast<float *>(c->w_srch_blk.p);
  }
  for (size_t g0 = 0; g0 < n_ref; g0 += group_max) {
    const size_t g1 = std::min(n_ref, g0 + group_max), n_g = g1 - g0;
    unsigned long long *keys = d_best ? reinterpret_cast<unsigned long long *>(d_best) + g0 * Q : d_keys;
    if (Q) HG_HIP(c, hipMemsetAsync(keys, 0, n_g * Q * sizeof(uint64_t), c->stream));
    const size_t row_lo = ref_first[g0], row_hi = ref_first[g1];
    // the rows of the group: slabs of a matrix that is there, or blocks computed into the scratch block
    const size_t step = empty ? 0 : src.d_ani ? HG_FRAG_MAX_GRID_Y : rb;
    for (size_t r0 = row_lo; !empty && r0 < row_hi; r0 += step) {
      const size_t rows = std::min(step, row_hi - r0);
      const float *blk = src.d_ani ? src.d_ani + r0 * Q : d_blk;
      if (!src.d_ani &&
          (s = hg_dist_full_dev(c, src.d_ref_hv + r0 * (size_t)src.hv_d, src.d_ref_n2 + r0, rows, src.d_qry_hv, src.d_qry_n2, Q, src.hv_d, src.ksize,
                                d_blk)) != HG_OK)
        return s;
      // the chunks that meet [r0, r0 + rows): from the one that holds r0 to the one that holds the last row
      auto holds = [&](size_t row) {
        return (size_t)(std::upper_bound(chunks.begin() + chunk_first[g0], chunks.begin() + chunk_first[g1], row,
                                         [](size_t v, const hg_frag_chunk &ch) { return v < ch.row0; }) - chunks.begin()) - 1;
      };
      const size_t c_lo = holds(r0), c_hi = holds(r0 + rows - 1) + 1;
      hg_timed tm(c, HG_T_DIST);
      for (size_t c0 = c_lo; c0 < c_hi; c0 += HG_FRAG_MAX_GRID_Y)  // (a forced block of more rows than a grid has: several launches)
        HG_HIP(c, hg_frag_launch_best(c->stream, blk, (uint32_t)r0, (uint32_t)rows, (uint32_t)Q, d_chunks, (uint32_t)c0,
                                      (uint32_t)std::min<size_t>(HG_FRAG_MAX_GRID_Y, c_hi - c0), (uint32_t)g0, keys));
    }
    if (n_qry) {
      hg_timed tm(c, HG_T_DIST);
      HG_HIP(c, hg_frag_launch_fold(c->stream, keys, (uint32_t)g0, (uint32_t)n_g, (uint32_t)Q, d_qf, (uint32_t)n_qry, m_th, d_pair, d_best != nullptr));
    }
  }
  HG_HIP(c, hipStreamSynchronize(c->stream));  // (the host tables above were read by then, too)
  return HG_OK;
}

}  // namespace

extern "C" uint32_t hg_frag_row_chunk(void) { return HG_FRAG_ROW_CHUNK; }
extern "C" uint32_t hg_frag_col_tile(void) { return HG_FRAG_COL_TILE; }
extern "C" uint32_t hg_frag_wave(void) { return HG_FRAG_WAVE; }
extern "C" uint32_t hg_frag_fold_threads(void) { return HG_FRAG_FOLD_THREADS; }
extern "C" const char *hg_frag_kernel_names(void) { return KERNEL_NAMES; }
extern "C" uint32_t hg_frag_launch_counts(uint64_t *counts, uint32_t cap) {
  for (uint32_t k = 0; counts && k < HG_FRAG_N_KERNELS && k < cap; ++k) counts[k] = hg_frag_launches(k);
  return HG_FRAG_N_KERNELS;
}

// ---- the window plan (no device) --------------------------------------------------------------------------------------------
extern "C" hg_status hg_frag_plan(uint64_t len, uint64_t window, uint64_t step, uint64_t *starts, uint64_t *lens, size_t cap, size_t *n) {
  if (!n) return HG_ERR_INVALID;
  *n = 0;
  if ((window | step) & 3 || step < 4 || step > window) return HG_ERR_INVALID;
  if (cap && (!starts || !lens)) return HG_ERR_INVALID;
  uint64_t count = 1;
  if (len > window) {
    count = 1 + (len - window + step - 1) / step;
    const uint64_t last = len - (count - 1) * step;  // window - step < last <= window
    if (2 * last < window) --count;                   // (count >= 2 here: the first window is whole)
  }
  *n = (size_t)count;
  for (uint64_t j = 0; j < count && j < cap; ++j) starts[j] = j * step, lens[j] = std::min(window, len - j * step);
  return count > cap ? HG_ERR_CAPACITY : HG_OK;
}

// ---- one sketch per window --------------------------------------------------------------------------------------------------
extern "C" hg_status hg_frag_sketch_seq_dev(hg_ctx *c, const uint8_t *d_seq, uint64_t n_bps, const hg_sketch_params *p, uint64_t window,
                                            uint64_t step, hg_frag_rows_fn rows, void *user, size_t *n_windows) {
  if (!c) return HG_ERR_INVALID;
  if (!p || !rows || !n_windows) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  *n_windows = 0;
  if (n_bps && !d_seq) return hg_fail(c, HG_ERR_INVALID, "NULL sequence");
  if (reinterpret_cast<uintptr_t>(d_seq) & 3) return hg_fail(c, HG_ERR_INVALID, "the sequence must be 4-byte aligned");
  size_t n = 0;
  hg_status s = hg_frag_plan(n_bps, window, step, nullptr, nullptr, 0, &n);
  if (s != HG_OK && s != HG_ERR_CAPACITY) return hg_fail(c, s, "window and step must be multiples of 4 with 4 <= step <= window");
  if (n >= ((size_t)1 << 31)) return hg_fail(c, HG_ERR_UNSUPPORTED, "2^31 windows or more in one sequence");
  std::vector<uint64_t> starts(n), lens(n);
  if ((s = hg_frag_plan(n_bps, window, step, starts.data(), lens.data(), n, &n)) != HG_OK) return hg_fail(c, s, "window plan");
  *n_windows = n;
  const size_t hv_d = p->hv_d, m_max = (size_t)std::min<uint64_t>(n, SUB_BATCH_WINDOWS), hv_bytes = (m_max * hv_d * sizeof(int16_t) + 15) & ~(size_t)15;
  DevMem d_out(c);
  if ((s = d_out.alloc(hv_bytes + m_max * 8 + 64)) != HG_OK) return s;
  auto *d_hv = static_cast<int16_t *>(d_out.p);
  auto *d_n2 = reinterpret_cast<int32_t *>(static_cast<uint8_t *>(d_out.p) + hv_bytes);
  auto *d_nh = reinterpret_cast<uint32_t *>(d_n2 + m_max);
  std::vector<int16_t> hv(m_max * hv_d);
  std::vector<int32_t> n2(m_max);
  std::vector<uint32_t> nh(m_max);
  for (size_t k0 = 0; k0 < n; k0 += SUB_BATCH_WINDOWS) {
    const size_t m = (size_t)std::min<uint64_t>(SUB_BATCH_WINDOWS, n - k0);
    if ((s = hg_sketch_batch_dev(c, d_seq, starts.data() + k0, lens.data() + k0, m, p, d_hv, d_n2, d_nh)) != HG_OK) return s;
    if ((s = hg_ctx_sync(c)) != HG_OK) return s;  // the step is deferred: no row is final before this
    if ((s = hg_copy_d2h(c, hv.data(), d_hv, m * hv_d * sizeof(int16_t))) != HG_OK) return s;
    if ((s = hg_copy_d2h(c, n2.data(), d_n2, m * sizeof(int32_t))) != HG_OK) return s;
    if ((s = hg_copy_d2h(c, nh.data(), d_nh, m * sizeof(uint32_t))) != HG_OK) return s;
    if (rows(user, starts.data() + k0, lens.data() + k0, k0, m, hv.data(), n2.data(), nh.data())) return hg_fail(c, HG_ERR_INVALID, "the rows callback failed");
  }
  return HG_OK;
}

// ---- the reduction ------------------------------------------------------------------------------------------------------------
extern "C" hg_status hg_frag_ani_matrix_dev(hg_ctx *c, const float *d_ani, size_t R, size_t Q, const uint32_t *ref_first, size_t n_ref,
                                            const uint32_t *qry_first, size_t n_qry, float frag_th, hg_frag_pair *d_pair, hg_frag_best *d_best) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_args(c, R, Q, ref_first, n_ref, qry_first, n_qry, d_pair, d_best);
  if (s != HG_OK) return s;
  if (R && Q && !d_ani) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (reinterpret_cast<uintptr_t>(d_ani) & 3) return hg_fail(c, HG_ERR_INVALID, "the matrix must be 4-byte aligned");
  HG_ENTER(c);
  Source src;
  src.d_ani = d_ani;
  return reduce(c, src, R, Q, ref_first, n_ref, qry_first, n_qry, frag_th, d_pair, d_best);
}

extern "C" hg_status hg_frag_ani_dev(hg_ctx *c, const int16_t *d_ref_hv, const int32_t *d_ref_norm2, size_t R, const int16_t *d_qry_hv,
                                     const int32_t *d_qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, const uint32_t *ref_first, size_t n_ref,
                                     const uint32_t *qry_first, size_t n_qry, float frag_th, size_t block_rows, hg_frag_pair *d_pair,
                                     hg_frag_best *d_best) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_args(c, R, Q, ref_first, n_ref, qry_first, n_qry, d_pair, d_best);
  if (s != HG_OK) return s;
  if (hv_d == 0 || hv_d > 65536) return hg_fail(c, HG_ERR_UNSUPPORTED, "hv_d must be in 1..65536");
  if (ksize == 0) return hg_fail(c, HG_ERR_INVALID, "ksize must be >= 1");
  if (R && Q && (!d_ref_hv || !d_ref_norm2 || !d_qry_hv || !d_qry_norm2)) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  Source src;
  src.d_ref_hv = d_ref_hv, src.d_ref_n2 = d_ref_norm2, src.d_qry_hv = d_qry_hv, src.d_qry_n2 = d_qry_norm2;
  src.hv_d = hv_d, src.ksize = ksize, src.block_rows = block_rows;
  return reduce(c, src, R, Q, ref_first, n_ref, qry_first, n_qry, frag_th, d_pair, d_best);
}

extern "C" hg_status hg_frag_ani(hg_ctx *c, const int16_t *ref_hv, const int32_t *ref_norm2, size_t R, const int16_t *qry_hv,
                                 const int32_t *qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, const uint32_t *ref_first, size_t n_ref,
                                 const uint32_t *qry_first, size_t n_qry, float frag_th, hg_frag_pair *pair, hg_frag_best *best) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_args(c, R, Q, ref_first, n_ref, qry_first, n_qry, pair, nullptr);
  if (s != HG_OK) return s;
  if (R && Q && (!ref_hv || !ref_norm2 || !qry_hv || !qry_norm2)) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  const size_t pair_bytes = n_ref * n_qry * sizeof(hg_frag_pair), best_bytes = best ? n_ref * Q * sizeof(hg_frag_best) : 0;
  DevMem d_rh(c), d_rn(c), d_qh(c), d_qn(c), d_pair(c), d_best(c);
  if ((s = d_rh.alloc(R * hv_d * sizeof(int16_t))) != HG_OK || (s = d_rn.alloc(R * sizeof(int32_t))) != HG_OK ||
      (s = d_qh.alloc(Q * hv_d * sizeof(int16_t))) != HG_OK || (s = d_qn.alloc(Q * sizeof(int32_t))) != HG_OK ||
      (s = d_pair.alloc(pair_bytes)) != HG_OK || (best && (s = d_best.alloc(best_bytes)) != HG_OK))
    return s;
  if (R && Q) {
    if ((s = hg_copy_h2d(c, d_rh.p, ref_hv, R * hv_d * sizeof(int16_t))) != HG_OK || (s = hg_copy_h2d(c, d_rn.p, ref_norm2, R * sizeof(int32_t))) != HG_OK ||
        (s = hg_copy_h2d(c, d_qh.p, qry_hv, Q * hv_d * sizeof(int16_t))) != HG_OK || (s = hg_copy_h2d(c, d_qn.p, qry_norm2, Q * sizeof(int32_t))) != HG_OK)
      return s;
  }
  s = hg_frag_ani_dev(c, static_cast<int16_t *>(d_rh.p), static_cast<int32_t *>(d_rn.p), R, static_cast<int16_t *>(d_qh.p),
                      static_cast<int32_t *>(d_qn.p), Q, hv_d, ksize, ref_first, n_ref, qry_first, n_qry, frag_th, 0,
                      static_cast<hg_frag_pair *>(d_pair.p), best ? static_cast<hg_frag_best *>(d_best.p) : nullptr);
  if (s != HG_OK) return s;
  if (pair_bytes && (s = hg_copy_d2h(c, pair, d_pair.p, pair_bytes)) != HG_OK) return s;
  if (best_bytes && (s = hg_copy_d2h(c, best, d_best.p, best_bytes)) != HG_OK) return s;
  return HG_OK;
}
