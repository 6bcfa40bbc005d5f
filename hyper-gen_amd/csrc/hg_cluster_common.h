// hg_cluster_common.h -- the device routines the clustering files share (hg_cluster.hip, hg_cluster_greedy.hip,
// hg_cluster_setcover.hip, hg_cluster_tree.hip): the lock-free union-find over rep[n], the order-preserving ANI key and the grid of a grid-stride
// launch.  One copy; each file's head comment says how it uses them.
#pragma once
#include <algorithm>

#include "hg_internal.h"

// Inside a hooking kernel other workgroups -- on other CUs, other XCDs -- move rep[] under our feet: a CU's L1 is never
// refreshed by another CU's stores and the XCDs' L2s are not coherent with each other, so a plain load could return a
// value that is stale for as long as the line stays cached, and a CAS loop fed by it would spin.  Every access of rep[] in
// such a kernel is therefore an agent-scope atomic (relaxed: each value read is used only for itself -- correctness needs
// no ordering between locations, see find_root and the hooking loops).
__device__ __forceinline__ uint32_t rep_load(uint32_t *rep, uint32_t x) {
  return __hip_atomic_load(rep + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rep_store(uint32_t *rep, uint32_t x, uint32_t v) {
  __hip_atomic_store(rep + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Invariants of rep[] (they hold for every value any lane can read, stale or fresh):
//   (1) rep[x] <= x, and rep[x] < x once x is not a root: only a CAS on a root writes a smaller index into it, path
//       halving writes into non-roots only, and always an ancestor, which is smaller;
//   (2) a non-root never becomes a root again (nothing writes x into rep[x] after init);
//   (3) an ancestor stays an ancestor: trees only merge.
// find_root terminates because x strictly decreases in every step (1).  A root it returns may be stale -- hooked meanwhile
// -- but is an ancestor of the argument (3); the CAS of the hooking loop finds out.
__device__ __forceinline__ uint32_t find_root(uint32_t *rep, uint32_t x) {
  uint32_t p = rep_load(rep, x);
  while (p != x) {
    const uint32_t g = rep_load(rep, p);
    if (g == p) return p;
    rep_store(rep, x, g);  // path halving: x skips its parent (x is a non-root, g an ancestor of it)
    x = g;
    p = rep_load(rep, x);
  }
  return x;
}

// The union of the trees of x and y.  Why the loop terminates: each round either hooks (CAS succeeds: done) or the CAS
// fails, which means `hi` is no longer a root -- another lane hooked it under a smaller index, which the CAS returns (1).
// The loop then goes on with the root of that index, which is < hi, in place of hi: a + b strictly decreases every round
// and is bounded below.  When a == b both ends share an ancestor, and by (3) they stay in one tree.
__device__ __forceinline__ void hook_roots(uint32_t *rep, uint32_t x, uint32_t y) {
  uint32_t a = find_root(rep, x), b = find_root(rep, y);
  while (a != b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    uint32_t seen = hi;
    if (__hip_atomic_compare_exchange_strong(rep + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      break;
    a = lo, b = find_root(rep, seen);  // hi was hooked under seen < hi
  }
}

// Any float -> a 32-bit key of the same order (negative values and both zeros included; -0.0f + 0.0f = +0.0f), and back.
// No float that is not a NaN has the key 0.
__device__ __forceinline__ uint32_t ani_key(float a) {
  const uint32_t b = __float_as_uint(a + 0.0f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_ani(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// workgroups of 256 lanes for a grid-stride loop over `items`
inline unsigned grid_for(hg_ctx *c, size_t items) {
  const size_t want = (items + 255) / 256, most = (size_t)c->n_cu * 16;
  return (unsigned)std::max<size_t>(1, std::min(want, most));
}
