// hg_nj_math.h -- the exact arithmetic of neighbour joining (hg_nj.hip), usable from host code too: the fixed-point
// distance, the criterion Q, the branch length of the lower name and the distance of the joined node.  One copy of each:
// the kernels use them, and tests/native/nj_driver.cpp runs them on the CPU at the bounds -- 65 536 live nodes, every
// distance at its maximum -- which no test on the device reaches.
#pragma once
#include <stdint.h>

#include "hg_average_cmp.h"

#define HG_NJ_MATH_FRAC_BITS 15                        // HG_NJ_FRAC_BITS of include/hypergen.h
#define HG_NJ_MATH_D_MAX ((uint32_t)100000u << HG_NJ_MATH_FRAC_BITS)  // 3 276 800 000 < 2^32

// d(i, j) of an ANI: (100 000 - m) << 15, m = the integer `dist` prints in thousandths (hg_avg_milli: 0 .. 100 000).
HG_AVG_HD inline uint32_t hg_nj_dist(float ani) { return (uint32_t)(100000u - (uint32_t)hg_avg_milli(ani)) << HG_NJ_MATH_FRAC_BITS; }

// Q(i, j) = (c - 2) d(i, j) - r(i) - r(j), c >= 2 live nodes.  r <= 65 535 d_max < 2^48 and (c - 2) d < 2^48: |Q| < 2^50.
// hg_nj_key is the part that varies along a row.
HG_AVG_HD inline int64_t hg_nj_key(uint32_t c, uint32_t d, int64_t rj) { return (int64_t)(c - 2u) * (int64_t)d - rj; }
HG_AVG_HD inline int64_t hg_nj_q(uint32_t c, uint32_t d, int64_t ri, int64_t rj) { return hg_nj_key(c, d, rj) - ri; }

// The branch from the lower name a to the joined node, c >= 3: floor(((c - 2) D + r(a) - r(b)) / (2 (c - 2))), a floor
// towards minus infinity -- the numerator may be negative, and so may the result.  len_b = D - len_a.
HG_AVG_HD inline int64_t hg_nj_len_a(uint32_t c, uint32_t D, int64_t ra, int64_t rb) {
  const int64_t den = 2 * (int64_t)(c - 2u), num = (int64_t)(c - 2u) * (int64_t)D + ra - rb;
  const int64_t q = num / den;  // (truncates towards 0)
  return q - (int64_t)(num % den != 0 && num < 0);
}

// d(a u b, k) = max(0, (d(a, k) + d(b, k) - D) >> 1): an arithmetic shift, the floor of the half.  Stays within d_max.
HG_AVG_HD inline uint32_t hg_nj_update(uint32_t dak, uint32_t dbk, uint32_t D) {
  const int64_t s = ((int64_t)dak + (int64_t)dbk - (int64_t)D) >> 1;
  return s < 0 ? 0u : (uint32_t)s;
}
