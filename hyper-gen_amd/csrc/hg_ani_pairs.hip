// hg_ani_pairs.hip -- ANI of the pairs a list names (hg_ani_pairs{,_dev}; no reference counterpart): every metric of a pair is a
// function of the same (dot, nr, nq), so one exact dot per listed pair gives any set of them -- without the R x Q comparison and
// its operand prepass, which a sparse list wastes.  The arithmetic is dist_skinny_kernel's (hg_dist_kernels.hip), indexed by a
// pair list instead of by a tile; the formulas are the copies of hg_dist_common.h.
#include <cstring>

#include "hg_dist_common.h"

namespace {

// One wave per pair, a wave-uniform grid-stride loop over the list.  hv_d % 8 == 0 (`vec`): both rows stream as 16-byte pieces
// per lane, AP_C pieces per row and pass -- a row of 4 096 dimensions is one pass of eight loads, sixteen in flight per lane for
// the pair; a lane whose piece index is past the row's end multiplies zeros.  Any other hv_d: 2 bytes per lane and step.
// Neither form reads a byte behind a row.  Exact wrapping i32 dots with v_dot2_i32_i16 (src/dist.rs:147-151), the wave total by
// __shfl_xor, lane 0 finishes the pair: the listed columns in ascending order of their bits, then the dot.
constexpr uint32_t AP_T = 256, AP_C = 8;  // threads of a workgroup, 16-byte pieces per lane, row and pass
typedef short short2s __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int32_t ap_dot8(const uint4 &a, const uint4 &b, int32_t t) {
  t = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2s, a.x), __builtin_bit_cast(short2s, b.x), t, false);
  t = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2s, a.y), __builtin_bit_cast(short2s, b.y), t, false);
  t = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2s, a.z), __builtin_bit_cast(short2s, b.z), t, false);
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2s, a.w), __builtin_bit_cast(short2s, b.w), t, false);
}

__global__ __launch_bounds__(AP_T) void ani_pairs_kernel(const int16_t *__restrict__ ref, const int32_t *__restrict__ ref_n2, uint32_t R,
                                                         const int16_t *__restrict__ qry, const int32_t *__restrict__ qry_n2, uint32_t Q,
                                                         uint32_t hv_d, float kf, int vec, const hg_ani_hit *__restrict__ pairs,
                                                         uint32_t n_pairs, uint32_t columns, float *__restrict__ ani,
                                                         int32_t *__restrict__ dot_out, uint32_t *__restrict__ err) {
  const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (AP_T / 64);
  const uint32_t n_cols = (uint32_t)__popc(columns);
  for (size_t p = blockIdx.x * (AP_T / 64) + (threadIdx.x >> 6); p < n_pairs; p += waves) {  // wave-uniform (64 bits: n_pairs may be 2^32 - 1)
    const uint32_t r = __builtin_amdgcn_readfirstlane(pairs[p].ref_idx), q = __builtin_amdgcn_readfirstlane(pairs[p].qry_idx);
    if (r == HG_PAIRS_EMPTY) {  // an unused slot of the top-k layout: zeros
      if (lane < n_cols) ani[p * n_cols + lane] = 0.0f;
      if (lane == 0 && dot_out) dot_out[p] = 0;
      continue;
    }
    if (r >= R || q >= Q) {  // the call fails; the rows are not read
      if (lane == 0) atomicOr(err, 1u);
      continue;
    }
    const int16_t *__restrict__ a = ref + (size_t)r * hv_d, *__restrict__ b = qry + (size_t)q * hv_d;
    int32_t acc = 0;
    if (vec) {
      const uint4 *__restrict__ a4 = reinterpret_cast<const uint4 *>(a), *__restrict__ b4 = reinterpret_cast<const uint4 *>(b);
      const uint32_t pieces = hv_d / 8;
      for (uint32_t p0 = 0; p0 < pieces; p0 += 64 * AP_C) {
        uint4 va[AP_C], vb[AP_C];
#pragma unroll
        for (uint32_t c = 0; c < AP_C; ++c) {
          const uint32_t i = p0 + c * 64 + lane;
          va[c] = i < pieces ? a4[i] : make_uint4(0, 0, 0, 0);
          vb[c] = i < pieces ? b4[i] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (uint32_t c = 0; c < AP_C; ++c) acc = ap_dot8(va[c], vb[c], acc);
      }
    } else {
      for (uint32_t i = lane; i < hv_d; i += 64) acc = (int32_t)((uint32_t)acc + (uint32_t)((int32_t)a[i] * (int32_t)b[i]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
      const int32_t nr = ref_n2[r], nq = qry_n2[q];
      float *out = ani + p * n_cols;
      if (columns & HG_PAIRS_MASH) *out++ = ani_from_dot(acc, nr, nq, kf);
      if (columns & HG_PAIRS_CONTAINMENT) *out++ = ani_from_dot_containment(true, acc, nr, nq, kf);
      if (columns & HG_PAIRS_MAX_CONTAINMENT) *out++ = ani_from_dot_containment(false, acc, nr, nq, kf);
      if (columns & HG_PAIRS_CONTAINMENT_REF) *out++ = ani_from_dot_containment(true, acc, nq, nr, kf);  // the sides exchanged
      if (dot_out) dot_out[p] = acc;
    }
  }
}

// the limits of check_dist (hg_api_dist.hip) without its rule for `symmetric`, and those of the list
hg_status check_pairs(hg_ctx *c, size_t R, size_t Q, uint32_t hv_d, uint32_t ksize, size_t n_pairs, uint32_t columns, bool want_dot) {
  if (R > 0x7FFFFFFFull || Q > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "R, Q must be < 2^31");
  if (hv_d == 0 || hv_d > 65536) return hg_fail(c, HG_ERR_UNSUPPORTED, "hv_d must be in 1..65536");
  if (ksize == 0) return hg_fail(c, HG_ERR_INVALID, "ksize must be >= 1");
  if (n_pairs > 0xFFFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "n_pairs must be < 2^32");
  if (columns >= 16u) return hg_fail(c, HG_ERR_INVALID, "columns: unknown bits (HG_PAIRS_*)");
  if (columns == 0 && !want_dot) return hg_fail(c, HG_ERR_INVALID, "columns == 0 without d_dot: nothing to compute");
  return HG_OK;
}
bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + nb && y < x + na;
}

}  // namespace

extern "C" hg_status hg_ani_pairs_dev(hg_ctx *c, const int16_t *d_ref_hv, const int32_t *d_ref_norm2, size_t R, const int16_t *d_qry_hv,
                                      const int32_t *d_qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, const hg_ani_hit *d_pairs,
                                      size_t n_pairs, uint32_t columns, float *d_ani, int32_t *d_dot) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_pairs(c, R, Q, hv_d, ksize, n_pairs, columns, d_dot != nullptr);
  if (s != HG_OK) return s;
  if (n_pairs == 0) return HG_OK;
  if (!d_pairs || !d_ref_hv || !d_ref_norm2 || !d_qry_hv || !d_qry_norm2 || (columns && !d_ani)) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  const size_t n_cols = (size_t)__builtin_popcount(columns);
  if (overlaps(d_pairs, n_pairs * sizeof(hg_ani_hit), d_ani, n_pairs * n_cols * sizeof(float)) ||
      overlaps(d_pairs, n_pairs * sizeof(hg_ani_hit), d_dot, n_pairs * sizeof(int32_t)))
    return hg_fail(c, HG_ERR_INVALID, "d_ani / d_dot overlap d_pairs");
  HG_ENTER(c);
  if ((s = hg_ensure(c, c->w_misc, 64)) != HG_OK) return s;
  auto *d_err = static_cast<uint32_t *>(c->w_misc.p);  // the error word: zero between calls (see hg_dist_block_dev)
  if (c->misc_zeroed != d_err) HG_HIP(c, hipMemsetAsync(d_err, 0, 64, c->stream));
  c->misc_zeroed = nullptr;
  // (16-byte loads need rows that start on 16 bytes: hv_d % 8 == 0 and both matrices aligned so, as every allocation is)
  const int vec = hv_d % 8 == 0 && ((uintptr_t)d_ref_hv | (uintptr_t)d_qry_hv) % 16 == 0;
  const size_t groups = (n_pairs + AP_T / 64 - 1) / (AP_T / 64);
  const uint32_t grid = (uint32_t)std::min<size_t>(groups, (size_t)c->n_cu * 4);  // 16 resident waves per CU, a pair (16 KB at D = 4096) in flight each
  {
    hg_timed tm(c, HG_T_DIST);
    c->last_kernel[HG_T_DIST] = "ani_pairs_kernel";
    hipLaunchKernelGGL(ani_pairs_kernel, dim3(grid), dim3(AP_T), 0, c->stream, d_ref_hv, d_ref_norm2, (uint32_t)R, d_qry_hv, d_qry_norm2,
                       (uint32_t)Q, hv_d, (float)ksize, vec, d_pairs, (uint32_t)n_pairs, columns, d_ani, d_dot, d_err);
    HG_HIP(c, hipGetLastError());
  }
  const uint32_t *h_res = nullptr;
  if ((s = hg_publish_words(c, d_err, 1, &h_res, 16)) != HG_OK) return s;  // (cleared behind the copy: the next call starts clean)
  c->misc_zeroed = d_err;
  if (h_res[0]) return hg_fail(c, HG_ERR_INVALID, "a listed pair has ref_idx >= R or qry_idx >= Q");
  return HG_OK;
}

extern "C" hg_status hg_ani_pairs(hg_ctx *c, const int16_t *ref_hv, const int32_t *ref_norm2, size_t R, const int16_t *qry_hv,
                                  const int32_t *qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize, const hg_ani_hit *pairs, size_t n_pairs,
                                  uint32_t columns, float *ani, int32_t *dot) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = check_pairs(c, R, Q, hv_d, ksize, n_pairs, columns, dot != nullptr);
  if (s != HG_OK) return s;
  if (n_pairs == 0) return HG_OK;
  if (!pairs || !ref_hv || !ref_norm2 || !qry_hv || !qry_norm2 || (columns && !ani)) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  // staged like hg_dist: a set paired with itself travels once; the list and both outputs share w_ani
  const bool same = ref_hv == qry_hv && ref_norm2 == qry_norm2 && R == Q;
  const size_t rb = R * (size_t)hv_d * 2, qb = Q * (size_t)hv_d * 2;
  const size_t pb = (n_pairs * sizeof(hg_ani_hit) + 63) / 64 * 64, ab = (n_pairs * (size_t)__builtin_popcount(columns) * sizeof(float) + 63) / 64 * 64;
  if ((s = hg_ensure(c, c->w_hv, rb + 64)) != HG_OK) return s;
  if (!same && (s = hg_ensure(c, c->w_hv2, qb + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_n2a, R * 4 + 64)) != HG_OK) return s;
  if (!same && (s = hg_ensure(c, c->w_n2b, Q * 4 + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_ani, pb + ab + n_pairs * sizeof(int32_t) + 64)) != HG_OK) return s;
  auto *d_pairs = static_cast<hg_ani_hit *>(c->w_ani.p);
  auto *d_ani = reinterpret_cast<float *>(static_cast<char *>(c->w_ani.p) + pb);
  auto *d_dot = reinterpret_cast<int32_t *>(static_cast<char *>(c->w_ani.p) + pb + ab);
  if (rb) HG_HIP(c, hipMemcpyAsync(c->w_hv.p, ref_hv, rb, hipMemcpyHostToDevice, c->stream));
  if (!same && qb) HG_HIP(c, hipMemcpyAsync(c->w_hv2.p, qry_hv, qb, hipMemcpyHostToDevice, c->stream));
  if (R) HG_HIP(c, hipMemcpyAsync(c->w_n2a.p, ref_norm2, R * 4, hipMemcpyHostToDevice, c->stream));
  if (!same && Q) HG_HIP(c, hipMemcpyAsync(c->w_n2b.p, qry_norm2, Q * 4, hipMemcpyHostToDevice, c->stream));
  HG_HIP(c, hipMemcpyAsync(d_pairs, pairs, n_pairs * sizeof(hg_ani_hit), hipMemcpyHostToDevice, c->stream));
  s = hg_ani_pairs_dev(c, static_cast<const int16_t *>(c->w_hv.p), static_cast<const int32_t *>(c->w_n2a.p), R,
                       static_cast<const int16_t *>(same ? c->w_hv.p : c->w_hv2.p), static_cast<const int32_t *>(same ? c->w_n2a.p : c->w_n2b.p),
                       Q, hv_d, ksize, d_pairs, n_pairs, columns, columns ? d_ani : nullptr, dot ? d_dot : nullptr);
  if (s != HG_OK) return s;
  if (columns) HG_HIP(c, hipMemcpyAsync(ani, d_ani, n_pairs * (size_t)__builtin_popcount(columns) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (dot) HG_HIP(c, hipMemcpyAsync(dot, d_dot, n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}
