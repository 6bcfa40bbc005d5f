// hg_dist_common.h -- what every part of the all-pairs ANI path shares (private to hg_dist_kernels.hip).
#pragma once
#include <type_traits>
#include <utility>

#include "hg_internal.h"
#include "hg_logf.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef int int4v __attribute__((ext_vector_type(4)));
typedef int int8v __attribute__((ext_vector_type(8)));
template <int... Js, class F>
__device__ __forceinline__ void dist_static_for(std::integer_sequence<int, Js...>, F &&f) {
  (f(std::integral_constant<int, Js>{}), ...);
}

// ---- ANI epilogue (src/dist.rs:153-160) -----------------------------------------------------
__device__ __forceinline__ float ani_from_dot(int32_t dot, int32_t nr, int32_t nq, float kf) {
  const int32_t den = (int32_t)((uint32_t)nr + (uint32_t)nq - (uint32_t)dot);  // i32 wrapping
  const float jaccard = (float)dot / (float)den;
  const float inner = 1.0f / jaccard + 1.0f;
  const float x = 2.0f / inner;
  float ani = 1.0f + hg_logf(x) / kf;  // (glibc's logf, bit for bit: hg_logf.h)
  if (ani != ani) return 0.0f;  // is_nan -> 0
  ani = fminf(ani, 1.0f);
  ani = fmaxf(ani, 0.0f);
  return ani * 100.0f;
}

// ---- the containment metrics (hg_ctx_set_ani_metric; include/hypergen.h) ---------------------------------------------------
// x = dot / nq (HG_ANI_CONTAINMENT: the share of the query's hashes found in the reference) or dot / min(nr, nq)
// (HG_ANI_MAX_CONTAINMENT), then exactly the tail of ani_from_dot: 1 + ln(x) / k, NaN -> 0, clamp to [0, 1], x 100, all of it
// f32 in this order (dot <= 0 -> 0; den = 0 -> NaN -> 0 or +inf -> 100; dot > den -> 100).  With equal norms
// 2J / (1 + J) = dot / n, so both reduce to the Mash-style value up to rounding.  `contain`: HG_ANI_CONTAINMENT.
__device__ __forceinline__ float ani_from_dot_containment(bool contain, int32_t dot, int32_t nr, int32_t nq, float kf) {
  const int32_t den = contain ? nq : (nr < nq ? nr : nq);
  const float x = (float)dot / (float)den;
  float ani = 1.0f + hg_logf(x) / kf;
  if (ani != ani) return 0.0f;
  ani = fminf(ani, 1.0f);
  ani = fmaxf(ani, 0.0f);
  return ani * 100.0f;
}
// any metric (a uniform value: the integer and streaming kernels, hg_ani_from_dots_dev)
__device__ __forceinline__ float ani_from_dot_metric(int metric, int32_t dot, int32_t nr, int32_t nq, float kf) {
  return metric == HG_ANI_MASH ? ani_from_dot(dot, nr, nq, kf) : ani_from_dot_containment(metric == HG_ANI_CONTAINMENT, dot, nr, nq, kf);
}

}  // namespace
