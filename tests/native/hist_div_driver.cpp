// hist_div_driver.cpp -- the division by the run-time bin width of libhypergen_hist.so (hyper-gen_amd/csrc/hg_hist.h:
// hg_hist_magic, hg_hist_div) on the CPU.  For EVERY width w in 1..100 000 it checks every bin edge: hg_hist_div(b w) == b
// and hg_hist_div(b w - 1) == b - 1 for every bin b, and the last value, 100 000.  The helper is monotone in m (a product
// with a positive constant, shifted), so between two edges that are right nothing can be wrong.  About 2.4 million checks.
// tests/test_hist_native.py builds it with -fsanitize=address,undefined and reads the last line.
#include <cinttypes>
#include <cstdio>

#include "../../hyper-gen_amd/csrc/hg_hist.h"

int main() {
  const uint32_t M = 100000;
  uint64_t checks = 0, bad = 0;
  auto check = [&](uint32_t w, uint64_t magic, uint32_t m) {
    ++checks;
    if (hg_hist_div(m, magic) != m / w && bad++ < 10) std::printf("w = %u, m = %u: %u, not %u\n", w, m, hg_hist_div(m, magic), m / w);
  };
  for (uint32_t w = 1; w <= M; ++w) {
    const uint64_t magic = hg_hist_magic(w);
    for (uint32_t b = 0; b <= M / w; ++b) {
      check(w, magic, b * w);
      if (b) check(w, magic, b * w - 1);
    }
    check(w, magic, M);
  }
  // the largest product the helper forms, and that a product of that size still fits 64 bits with room
  const uint64_t top = (uint64_t)M * hg_hist_magic(1);
  if (top >> 58) ++bad, std::printf("m * magic reaches bit 58\n");
  std::printf("hist div driver %s: %" PRIu64 " checks, %" PRIu64 " wrong\n", bad ? "FAILED" : "ok", checks, bad);
  return bad ? 1 : 0;
}
