// hg_average_cmp.h -- the exact arithmetic of average linkage (hg_cluster_average.hip), usable from host code too: the
// quantised ANI and the comparison of two averages.  tests/native/average_cmp_driver.cpp runs it on the CPU against
// operands whose products differ only above bit 64 -- sizes no test on the device reaches.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HG_AVG_HD __host__ __device__
#else
#define HG_AVG_HD
#endif

// The integer `dist` prints for an ANI, in thousandths (hg_cli.cpp, put_ani): NaN and negative values 0, values above 100
// 100 000, else the product with 1000 -- exact in a double -- rounded to the nearest integer, ties to even.
HG_AVG_HD inline uint64_t hg_avg_milli(float ani) {
  if (!(ani >= 0.0f)) ani = 0.0f;  // NaN too
  if (ani > 100.0f) ani = 100.0f;
  return (uint64_t)__builtin_rint((double)ani * 1000.0);
}

// sa / da against sb / db (sums of milli over da = c(A) c(B) and db = c(C) c(D) pairs; both denominators > 0) without a
// division: the cross products, which outgrow 64 bits near n = 17 000, in 128 bits.  > 0: the first average is larger,
// < 0: the second, 0: they are equal.
HG_AVG_HD inline int hg_avg_compare(uint64_t sa, uint64_t da, uint64_t sb, uint64_t db) {
  const unsigned __int128 l = (unsigned __int128)sa * db, r = (unsigned __int128)sb * da;
  return l > r ? 1 : (l < r ? -1 : 0);
}
