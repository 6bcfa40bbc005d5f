// average_cmp_driver.cpp -- the exact arithmetic of average linkage (hyper-gen_amd/csrc/hg_average_cmp.h) on the CPU, for
// operands no device test reaches.  Reads one request per line from stdin and answers one line each:
//   c <sa> <da> <sb> <db>   -> hg_avg_compare: 1, -1 or 0
//   m <float bits, hex>     -> hg_avg_milli
// tests/test_cluster_average_surface.py feeds it pairs whose cross products differ only above bit 64 and checks the answers
// against Python integers.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../hyper-gen_amd/csrc/hg_average_cmp.h"

int main() {
  char line[256];
  unsigned long n = 0;
  while (std::fgets(line, sizeof line, stdin)) {
    uint64_t sa, da, sb, db;
    uint32_t bits;
    if (std::sscanf(line, "c %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &sa, &da, &sb, &db) == 4) {
      std::printf("%d\n", hg_avg_compare(sa, da, sb, db));
    } else if (std::sscanf(line, "m %" SCNx32, &bits) == 1) {
      float f;
      std::memcpy(&f, &bits, 4);
      std::printf("%" PRIu64 "\n", hg_avg_milli(f));
    } else {
      std::fprintf(stderr, "bad request: %s", line);
      return 1;
    }
    ++n;
  }
  std::fprintf(stderr, "average cmp driver ok: %lu requests\n", n);
  return 0;
}
