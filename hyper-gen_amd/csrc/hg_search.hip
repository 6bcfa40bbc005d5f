// hg_search.hip -- `search` in bounded memory: per query the k best references, selected while blocks of the ANI matrix
// stream past (include/hypergen.h, "search: exact top-k per query").  No hit list is built: memory is one block of the
// matrix (HG_SEARCH_BLOCK_BYTES), the slice lists of one block and Q * k keys of running state.
//
// Order.  An entry is the u64 key  ani_bits << 32 | (0xFFFFFFFF - global reference index).  ANI is never negative, so its
// IEEE bit pattern is monotone and ONE unsigned compare gives "descending ANI, ties by ascending reference index" -- a total
// order (no two entries of a query share a reference), hence the result does not depend on block size, slice count or
// scheduling.  Key 0 marks an empty slot (a real entry's low word is >= 2^31: reference indices stay below 2^31).
//
// Per block of reference rows [r0, r0 + Rb):
//   hg_dist_full_dev          the Rb x Q float block into w_srch_blk
//   search_topk_select_kernel grid (column strips) x (row slices).  A strip is cw = min(64, Q rounded up to a power of two)
//                             query columns; thread t of a workgroup owns column t % cw and the rows t / cw, t / cw + nsub, ...
//                             of its slice (nsub = threads / cw), so a wave reads 64 / cw consecutive matrix rows of cw
//                             consecutive floats each: whole 256-byte lines for Q >= 64, and for Q < 64 several rows per
//                             read with enough slices to fill the chip.  Every thread keeps a sorted list of k keys in LDS,
//                             list[j * threads + t] (conflict-free 8-byte reads across a wave), and rejects a value with
//                             one float compare (the threshold) and one u64 compare against its k-th key -- which starts at
//                             the running state's k-th key, so after the first block insertions are rare.  The nsub lists
//                             of a column are then folded in LDS (log2 nsub rounds) and the slice writes ONE list per column.
//   search_topk_merge_kernel  one workgroup per strip, the same mapping with slice lists in the place of matrix rows: thread
//                             (column, sub) folds the slices sub, sub + nsub, ... into its list, sub 0 starts from the
//                             running state, the lists are folded in LDS and the state is rewritten.
// search_topk_emit_kernel turns the state into hg_ani_hit rows and counts.
#include <cstring>

#include "hg_internal.h"

namespace {

constexpr uint32_t SEL_UNROLL = 8;                      // matrix values a thread has in flight
constexpr size_t SEL_LIST_BYTES = (size_t)32 << 20;     // cap of one block's slice lists (fewer, longer slices beyond it)

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t topk_key(float ani, uint32_t ref) {
  return ((uint64_t)__float_as_uint(ani) << 32) | (uint64_t)(0xFFFFFFFFu - ref);
}

// list: this thread's k keys, descending, `stride` words apart; key > list[k - 1] (the caller checked)
__device__ __forceinline__ void topk_insert(uint64_t *list, uint32_t stride, uint32_t k, uint64_t key) {
  uint32_t j = k - 1;
  while (j > 0) {
    const uint64_t up = list[(size_t)(j - 1) * stride];
    if (up >= key) break;
    list[(size_t)j * stride] = up;
    --j;
  }
  list[(size_t)j * stride] = key;
}

// A descending list `src` (0 ends it) into the thread's own; entries at or below `floor` cannot reach the result
__device__ __forceinline__ void topk_absorb(uint64_t *mine, uint32_t stride, uint32_t k, uint64_t floor, const uint64_t *src,
                                            size_t src_stride, uint32_t n) {
  uint64_t kth = umax64(floor, mine[(size_t)(k - 1) * stride]);
  for (uint32_t j = 0; j < n; ++j) {
    const uint64_t key = src[(size_t)j * src_stride];
    if (key <= kth) break;
    topk_insert(mine, stride, k, key);
    kth = umax64(floor, mine[(size_t)(k - 1) * stride]);
  }
}

// The nsub = blockDim.x / cw lists of every column of the strip into the list of thread (column, sub 0)
__device__ __forceinline__ void topk_fold(uint64_t *lists, uint32_t cw, uint32_t k, uint64_t floor) {
  const uint32_t nthr = blockDim.x, t = threadIdx.x;
  for (uint32_t step = nthr / cw / 2; step >= 1; step >>= 1) {
    __syncthreads();
    if (t / cw < step) topk_absorb(lists + t, nthr, k, floor, lists + t + step * cw, nthr, k);
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void search_topk_select_kernel(const float *__restrict__ blk, uint32_t rows, uint64_t Q, uint32_t cw,
                                                                 uint32_t rows_per_slice, uint32_t k, float ani_th, uint32_t ref0,
                                                                 const uint64_t *__restrict__ state, uint64_t *__restrict__ slice_keys,
                                                                 uint32_t *__restrict__ slice_cnt) {
  extern __shared__ uint64_t s_lists[];
  const uint32_t nthr = blockDim.x, t = threadIdx.x, nsub = nthr / cw, sub = t / cw;
  const uint64_t q = (uint64_t)blockIdx.x * cw + (t & (cw - 1));
  const bool valid = q < Q;
  uint64_t *mine = s_lists + t;
  for (uint32_t j = 0; j < k; ++j) mine[(size_t)j * nthr] = 0;
  // (a column behind Q takes nothing: no key exceeds this floor)
  const uint64_t floor = valid ? state[(size_t)(k - 1) * Q + q] : ~0ull;
  const uint32_t r_begin = blockIdx.y * rows_per_slice, r_end = min(rows, r_begin + rows_per_slice);
  uint64_t kth = floor;
  for (uint32_t r = r_begin + sub; r < r_end; r += nsub * SEL_UNROLL) {
    float v[SEL_UNROLL];
#pragma unroll
    for (uint32_t u = 0; u < SEL_UNROLL; ++u) {
      const uint32_t rr = r + u * nsub;
      v[u] = (valid && rr < r_end) ? blk[(size_t)rr * Q + q] : __uint_as_float(0x7FC00000u);  // NaN fails every threshold
    }
#pragma unroll
    for (uint32_t u = 0; u < SEL_UNROLL; ++u) {
      if (v[u] >= ani_th) {
        const uint64_t key = topk_key(v[u], ref0 + r + u * nsub);
        if (key > kth) {
          topk_insert(mine, nthr, k, key);
          kth = umax64(floor, mine[(size_t)(k - 1) * nthr]);
        }
      }
    }
  }
  topk_fold(s_lists, cw, k, floor);
  if (sub == 0 && valid) {
    uint32_t n = 0;
    for (; n < k; ++n) {
      const uint64_t key = mine[(size_t)n * nthr];
      if (!key) break;
      slice_keys[((size_t)blockIdx.y * k + n) * Q + q] = key;
    }
    slice_cnt[(size_t)blockIdx.y * Q + q] = n;
  }
}

__global__ __launch_bounds__(256) void search_topk_merge_kernel(const uint64_t *__restrict__ slice_keys, const uint32_t *__restrict__ slice_cnt,
                                                                uint32_t n_slices, uint64_t Q, uint32_t cw, uint32_t k,
                                                                uint64_t *__restrict__ state) {
  extern __shared__ uint64_t s_lists[];
  const uint32_t nthr = blockDim.x, t = threadIdx.x, nsub = nthr / cw, sub = t / cw;
  const uint64_t q = (uint64_t)blockIdx.x * cw + (t & (cw - 1));
  const bool valid = q < Q;
  uint64_t *mine = s_lists + t;
  for (uint32_t j = 0; j < k; ++j) mine[(size_t)j * nthr] = (sub == 0 && valid) ? state[(size_t)j * Q + q] : 0;
  if (valid)
    for (uint32_t s = sub; s < n_slices; s += nsub)
      topk_absorb(mine, nthr, k, 0, slice_keys + (size_t)s * k * Q + q, Q, slice_cnt[(size_t)s * Q + q]);
  topk_fold(s_lists, cw, k, 0);
  if (sub == 0 && valid)
    for (uint32_t j = 0; j < k; ++j) state[(size_t)j * Q + q] = mine[(size_t)j * nthr];
}

// state[j * Q + q] -> d_out[q * k + j], d_counts[q]
__global__ __launch_bounds__(256) void search_topk_emit_kernel(const uint64_t *__restrict__ state, uint64_t Q, uint32_t k, uint32_t qry_off,
                                                               hg_ani_hit *__restrict__ out, uint32_t *__restrict__ counts) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)Q * k) return;
  const uint64_t q = i / k;
  const uint32_t j = (uint32_t)(i - q * k);
  const uint64_t key = state[(size_t)j * Q + q];
  if (!key) {
    out[i] = hg_ani_hit{0xFFFFFFFFu, 0xFFFFFFFFu, 0.f};
    if (j == 0) counts[q] = 0;
    return;
  }
  out[i] = hg_ani_hit{0xFFFFFFFFu - (uint32_t)key, qry_off + (uint32_t)q, __uint_as_float((uint32_t)(key >> 32))};
  if (j + 1 == k || state[(size_t)(j + 1) * Q + q] == 0) counts[q] = j + 1;
}

struct SearchPlan {
  uint32_t Rb, cw, nthr, rows_per_slice, max_slices;
};

uint32_t ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

SearchPlan plan_search(const hg_ctx *c, size_t R, size_t Q, uint32_t k) {
  SearchPlan p{};
  const uint64_t fit = std::max<uint64_t>(1, HG_SEARCH_BLOCK_BYTES / (sizeof(float) * (uint64_t)Q));
  uint64_t rb = c->dbg_search_block_rows ? c->dbg_search_block_rows : (fit > 256 ? fit & ~(uint64_t)255 : fit);
  p.Rb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(rb, std::max<size_t>(R, 1)));
  p.cw = 1;
  while (p.cw < 64 && p.cw < Q) p.cw *= 2;
  p.nthr = k > 32 ? 128 : 256;  // threads * k * 8 bytes of LDS: 64 KiB at most
  const uint32_t nsub = p.nthr / p.cw, strips = ceil_div(Q, p.cw);
  // slices: enough workgroups to fill the chip a few times over, at least SEL_UNROLL rows per thread, and lists within
  // SEL_LIST_BYTES
  const uint32_t want = std::max<uint32_t>(1, 8u * (uint32_t)c->n_cu / std::max(1u, strips));
  const uint64_t list_cap = std::max<uint64_t>(1, SEL_LIST_BYTES / ((uint64_t)Q * k * sizeof(uint64_t)));
  const uint32_t slices = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(want, list_cap), 4096);
  p.rows_per_slice = std::max(nsub * SEL_UNROLL, ceil_div(p.Rb, slices));
  p.max_slices = ceil_div(p.Rb, p.rows_per_slice);
  return p;
}

hg_status check_search(hg_ctx *c, size_t R, size_t ref_off, size_t Q, size_t qry_off, uint32_t hv_d, uint32_t ksize, uint32_t k) {
  if (k > HG_SEARCH_TOPK_MAX) return hg_fail(c, HG_ERR_UNSUPPORTED, "k exceeds HG_SEARCH_TOPK_MAX");
  if (R > 0x7FFFFFFFull || Q > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "R, Q must be < 2^31");
  if (ref_off + R > 0x7FFFFFFFull || qry_off + Q > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "global indices must be < 2^31");
  if (hv_d == 0 || hv_d > 65536) return hg_fail(c, HG_ERR_UNSUPPORTED, "hv_d must be in 1..65536");
  if (ksize == 0) return hg_fail(c, HG_ERR_INVALID, "ksize must be >= 1");
  // (a launch addresses fewer than 2^32 threads: one per slot in the emit kernel, 256 per 64 queries in the others)
  if ((uint64_t)Q * std::max(k, 4u) >= 0xFFFFFF00ull) return hg_fail(c, HG_ERR_UNSUPPORTED, "Q * k must be < 2^32");
  return HG_OK;
}

}  // namespace

extern "C" hg_status hg_search_topk_block_dev(hg_ctx *c, const int16_t *d_ref_hv, const int32_t *d_ref_norm2, size_t R, size_t ref_off,
                                              const int16_t *d_qry_hv, const int32_t *d_qry_norm2, size_t Q, size_t qry_off,
                                              uint32_t hv_d, uint32_t ksize, float ani_th, uint32_t k, hg_ani_hit *d_out,
                                              uint32_t *d_counts) {
  if (!c) return HG_ERR_INVALID;
  if (k == 0 || Q == 0) return HG_OK;
  hg_status s = check_search(c, R, ref_off, Q, qry_off, hv_d, ksize, k);
  if (s != HG_OK) return s;
  if (!d_out || !d_counts || !d_qry_hv || !d_qry_norm2 || (R && (!d_ref_hv || !d_ref_norm2))) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  const SearchPlan p = plan_search(c, R, Q, k);
  const size_t state_bytes = Q * (size_t)k * sizeof(uint64_t);
  const size_t keys_bytes = ((size_t)p.max_slices * k * Q * sizeof(uint64_t) + 255) & ~(size_t)255;
  if ((s = hg_ensure(c, c->w_srch_state, state_bytes)) != HG_OK) return s;
  auto *state = static_cast<uint64_t *>(c->w_srch_state.p);
  HG_HIP(c, hipMemsetAsync(state, 0, state_bytes, c->stream));
  if (R) {
    if ((s = hg_ensure(c, c->w_srch_blk, (size_t)p.Rb * Q * sizeof(float))) != HG_OK) return s;
    if ((s = hg_ensure(c, c->w_srch_lists, keys_bytes + (size_t)p.max_slices * Q * sizeof(uint32_t))) != HG_OK) return s;
  }
  auto *blk = static_cast<float *>(c->w_srch_blk.p);
  auto *keys = static_cast<uint64_t *>(c->w_srch_lists.p);
  auto *cnts = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(c->w_srch_lists.p) + keys_bytes);
  const uint32_t strips = ceil_div(Q, p.cw);
  const size_t lds = (size_t)p.nthr * k * sizeof(uint64_t);
  for (size_t r0 = 0; r0 < R; r0 += p.Rb) {
    const uint32_t rows = (uint32_t)std::min<size_t>(p.Rb, R - r0), n_slices = ceil_div(rows, p.rows_per_slice);
    if ((s = hg_dist_full_dev(c, d_ref_hv + r0 * (size_t)hv_d, d_ref_norm2 + r0, rows, d_qry_hv, d_qry_norm2, Q, hv_d, ksize, blk)) != HG_OK)
      return s;
    hipLaunchKernelGGL(search_topk_select_kernel, dim3(strips, n_slices), dim3(p.nthr), lds, c->stream, blk, rows, (uint64_t)Q, p.cw,
                       p.rows_per_slice, k, ani_th, (uint32_t)(ref_off + r0), state, keys, cnts);
    HG_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(search_topk_merge_kernel, dim3(strips), dim3(p.nthr), lds, c->stream, keys, cnts, n_slices, (uint64_t)Q, p.cw, k,
                       state);
    HG_HIP(c, hipGetLastError());
  }
  const size_t slots = Q * (size_t)k;
  hipLaunchKernelGGL(search_topk_emit_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, c->stream, state, (uint64_t)Q, k,
                     (uint32_t)qry_off, d_out, d_counts);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}

extern "C" hg_status hg_search_topk_dev(hg_ctx *c, const int16_t *d_ref_hv, const int32_t *d_ref_norm2, size_t R, const int16_t *d_qry_hv,
                                        const int32_t *d_qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, float ani_th, uint32_t k,
                                        hg_ani_hit *d_out, uint32_t *d_counts) {
  return hg_search_topk_block_dev(c, d_ref_hv, d_ref_norm2, R, 0, d_qry_hv, d_qry_norm2, Q, 0, hv_d, ksize, ani_th, k, d_out, d_counts);
}

extern "C" hg_status hg_search_topk(hg_ctx *c, const int16_t *ref_hv, const int32_t *ref_norm2, size_t R, const int16_t *qry_hv,
                                    const int32_t *qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, float ani_th, uint32_t k,
                                    hg_ani_hit *out, uint32_t *counts) {
  if (!c) return HG_ERR_INVALID;
  if (k == 0 || Q == 0) return HG_OK;
  hg_status s = check_search(c, R, 0, Q, 0, hv_d, ksize, k);
  if (s != HG_OK) return s;
  if (!out || !counts || !qry_hv || !qry_norm2 || (R && (!ref_hv || !ref_norm2))) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  const size_t rb = R * (size_t)hv_d * 2, qb = Q * (size_t)hv_d * 2, ob = Q * (size_t)k * sizeof(hg_ani_hit);
  if ((s = hg_ensure(c, c->w_hv, rb + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_hv2, qb + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_n2a, R * 4 + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_n2b, Q * 4 + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_srch_out, ob + Q * sizeof(uint32_t) + 64)) != HG_OK) return s;
  if (R) {
    HG_HIP(c, hipMemcpyAsync(c->w_hv.p, ref_hv, rb, hipMemcpyHostToDevice, c->stream));
    HG_HIP(c, hipMemcpyAsync(c->w_n2a.p, ref_norm2, R * 4, hipMemcpyHostToDevice, c->stream));
  }
  HG_HIP(c, hipMemcpyAsync(c->w_hv2.p, qry_hv, qb, hipMemcpyHostToDevice, c->stream));
  HG_HIP(c, hipMemcpyAsync(c->w_n2b.p, qry_norm2, Q * 4, hipMemcpyHostToDevice, c->stream));
  auto *d_out = static_cast<hg_ani_hit *>(c->w_srch_out.p);
  auto *d_cnt = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(c->w_srch_out.p) + ob);
  s = hg_search_topk_dev(c, static_cast<const int16_t *>(c->w_hv.p), static_cast<const int32_t *>(c->w_n2a.p), R,
                         static_cast<const int16_t *>(c->w_hv2.p), static_cast<const int32_t *>(c->w_n2b.p), Q, hv_d, ksize, ani_th, k,
                         d_out, d_cnt);
  if (s != HG_OK) return s;
  HG_HIP(c, hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(counts, d_cnt, Q * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}

extern "C" hg_status hg_search_topk_merge(const hg_ani_hit *const *lists, const uint32_t *const *counts, size_t n_lists, size_t Q,
                                          uint32_t k, hg_ani_hit *out, uint32_t *counts_out) {
  if (k == 0 || Q == 0) return HG_OK;
  if (k > HG_SEARCH_TOPK_MAX) return HG_ERR_UNSUPPORTED;
  if (!out || !counts_out || (n_lists && (!lists || !counts))) return HG_ERR_INVALID;
  for (size_t l = 0; l < n_lists; ++l)
    if (!lists[l] || !counts[l]) return HG_ERR_INVALID;
  auto key = [](const hg_ani_hit &h) {
    uint32_t bits;
    std::memcpy(&bits, &h.ani, 4);
    return ((uint64_t)bits << 32) | (uint64_t)(0xFFFFFFFFu - h.ref_idx);
  };
  std::vector<uint32_t> head(n_lists);
  for (size_t q = 0; q < Q; ++q) {
    std::fill(head.begin(), head.end(), 0u);
    uint32_t n = 0;
    for (; n < k; ++n) {  // every list is in the order itself: the best of the heads is next
      size_t best = n_lists;
      uint64_t best_key = 0;
      for (size_t l = 0; l < n_lists; ++l) {
        if (head[l] >= std::min(counts[l][q], k)) continue;
        const uint64_t kk = key(lists[l][q * k + head[l]]);
        if (best == n_lists || kk > best_key) best = l, best_key = kk;
      }
      if (best == n_lists) break;
      out[q * k + n] = lists[best][q * k + head[best]++];
    }
    counts_out[q] = n;
    for (uint32_t j = n; j < k; ++j) out[q * k + j] = hg_ani_hit{0xFFFFFFFFu, 0xFFFFFFFFu, 0.f};
  }
  return HG_OK;
}
