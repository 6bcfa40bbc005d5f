// tri_format_driver.cpp -- the field packer of libhypergen_tri.so (hyper-gen_amd/csrc/hg_tri.h: hg_tri_field) on the CPU.  For
// EVERY m in 0..100 000 the 64-bit word, read as eight bytes in memory order, is compared with snprintf("%7.3f") of m / 1000
// (m / 1000.0 is printed exactly as its three decimals: the nearest double of a decimal with three places rounds back to it)
// and with the integer form "%3u.%03u", under both separators.  200 002 checks.
// tests/test_tri_native.py builds it with -fsanitize=address,undefined and reads the last line.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../hyper-gen_amd/csrc/hg_tri.h"

int main() {
  const uint32_t M = 100000;
  uint64_t checks = 0, bad = 0;
  for (uint32_t m = 0; m <= M; ++m) {
    char want[16], ints[16];
    std::snprintf(want, sizeof want, "%7.3f", (double)m / 1000.0);
    std::snprintf(ints, sizeof ints, "%3u.%03u", m / 1000, m % 1000);
    for (const char sep : {'\t', '\n'}) {
      const uint64_t word = hg_tri_field(m, (uint32_t)(unsigned char)sep);
      char got[9] = {0};
      std::memcpy(got, &word, 8);  // (the kernel stores the word: little-endian, byte 0 first)
      ++checks;
      if (std::strlen(want) != 7 || std::memcmp(got, want, 7) != 0 || std::memcmp(got, ints, 7) != 0 || got[7] != sep) {
        if (bad++ < 10) std::printf("m = %u: \"%.7s\" + 0x%02x, not \"%s\" + 0x%02x\n", m, got, (unsigned)(unsigned char)got[7], want, (unsigned)sep);
      }
    }
  }
  std::printf("tri format driver %s: %" PRIu64 " checks, %" PRIu64 " wrong\n", bad ? "FAILED" : "ok", checks, bad);
  return bad ? 1 : 0;
}
