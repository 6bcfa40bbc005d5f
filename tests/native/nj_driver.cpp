// nj_driver.cpp -- the host-side parts of neighbour joining under AddressSanitizer + UBSan (tests/test_nj_native.py builds it
// with g++ as a stand-alone program): hg_nj_math.h at the bounds no device test reaches -- 65 536 live nodes, every
// distance at its maximum or at 0, negative numerators of the floor -- against 128-bit arithmetic, and hg_nj_newick
// (hg_formats.cpp) on random valid join lists, on lists broken in one place and on random garbage.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../hyper-gen_amd/csrc/hg_nj_math.h"
#include "../../include/hypergen.h"

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

typedef __int128 i128;

static i128 floor_div(i128 num, i128 den) {  // den > 0
  i128 q = num / den;
  if (num % den != 0 && num < 0) --q;
  return q;
}
static i128 ref_len_a(uint32_t c, uint32_t D, int64_t ra, int64_t rb) { return floor_div((i128)(c - 2) * D + ra - rb, 2 * (i128)(c - 2)); }
static i128 ref_q(uint32_t c, uint32_t d, int64_t ri, int64_t rj) { return (i128)(c - 2) * d - ri - rj; }
static i128 ref_update(uint32_t dak, uint32_t dbk, uint32_t D) {
  const i128 s = floor_div((i128)dak + dbk - D, 2);
  return s < 0 ? 0 : s;
}

static void math_at_the_bounds() {
  static_assert(HG_NJ_MATH_FRAC_BITS == HG_NJ_FRAC_BITS, "one fixed point");
  const uint32_t DMAX = HG_NJ_MATH_D_MAX;
  CHECK(DMAX == 3276800000u && (uint64_t)DMAX == ((uint64_t)100000 << 15));
  // the distance of an ANI
  CHECK(hg_nj_dist(100.0f) == 0 && hg_nj_dist(250.0f) == 0 && hg_nj_dist(std::numeric_limits<float>::infinity()) == 0);
  CHECK(hg_nj_dist(0.0f) == DMAX && hg_nj_dist(-5.0f) == DMAX && hg_nj_dist(std::numeric_limits<float>::quiet_NaN()) == DMAX);
  CHECK(hg_nj_dist(99.999f) == (1u << 15) && hg_nj_dist(95.0f) == (5000u << 15) && hg_nj_dist(99.9996f) == 0);
  // Q with 65 536 live nodes: every distance at its maximum, and a pair at 0 among maxima; |Q| < 2^50
  const uint32_t C = HG_NJ_MAX_N;
  const int64_t RMAX = (int64_t)(C - 1) * DMAX;  // r of a node whose 65 535 distances are all at the maximum
  const i128 LIMIT = (i128)1 << 50;
  for (uint32_t c : {3u, 4u, 1000u, C - 1, C})
    for (uint32_t d : {0u, 1u, DMAX - 1, DMAX})
      for (int64_t ri : {(int64_t)0, (int64_t)d, RMAX})
        for (int64_t rj : {(int64_t)0, (int64_t)d, RMAX}) {
          const i128 want = ref_q(c, d, ri, rj);
          CHECK(want < LIMIT && want > -LIMIT);
          CHECK((i128)hg_nj_q(c, d, ri, rj) == want);
          CHECK((i128)hg_nj_key(c, d, rj) - ri == want);
        }
  CHECK(hg_nj_q(C, DMAX, RMAX, RMAX) == (int64_t)(C - 2) * DMAX - 2 * RMAX && hg_nj_q(C, DMAX, RMAX, RMAX) < 0);
  CHECK(hg_nj_q(C, 0, RMAX - DMAX, RMAX - DMAX) == -2 * (RMAX - (int64_t)DMAX));
  // the floor of the branch length: negative numerators round towards minus infinity
  CHECK(hg_nj_len_a(3, 0, 0, 1) == -1 && hg_nj_len_a(3, 0, 0, 2) == -1 && hg_nj_len_a(3, 0, 0, 3) == -2 && hg_nj_len_a(3, 0, 1, 0) == 0);
  CHECK(hg_nj_len_a(3, 3, 7, 9) == 0 && hg_nj_len_a(3, 3, 12, 7) == 4 && hg_nj_len_a(4, 1, 0, 7) == -2);  // floor(-5 / 4)
  CHECK(hg_nj_len_a(C, DMAX, RMAX, RMAX) == (int64_t)DMAX / 2 && hg_nj_len_a(C, DMAX, 0, RMAX) < 0);
  for (uint32_t c : {3u, 4u, 5u, 65535u, C})
    for (uint32_t D : {0u, 1u, 2u, DMAX - 1, DMAX})
      for (int64_t ra : {(int64_t)D, (int64_t)D + 1, RMAX / 3, RMAX - 1, RMAX})
        for (int64_t rb : {(int64_t)D, (int64_t)D + 2, RMAX / 7, RMAX - 1, RMAX}) {
          const int64_t la = hg_nj_len_a(c, D, ra, rb);
          CHECK((i128)la == ref_len_a(c, D, ra, rb));
          CHECK((i128)la + ((int64_t)D - la) == (i128)D);
        }
  // the distance of a joined node: floor of the half, clamped at 0, never above the maximum
  CHECK(hg_nj_update(0, 0, DMAX) == 0 && hg_nj_update(DMAX, DMAX, 0) == DMAX && hg_nj_update(DMAX, DMAX, DMAX) == DMAX / 2);
  CHECK(hg_nj_update(1, 0, 0) == 0 && hg_nj_update(3, 0, 0) == 1 && hg_nj_update(0, 0, 1) == 0 && hg_nj_update(2, 3, 0) == 2);
  CHECK(hg_nj_update(5, 0, 6) == 0 && hg_nj_update(5, 2, 6) == 0 && hg_nj_update(5, 3, 6) == 1);
  std::mt19937_64 rng(5);
  for (int k = 0; k < 200000; ++k) {
    const uint32_t c = 3 + (uint32_t)(rng() % (C - 2)), d = (uint32_t)(rng() % ((uint64_t)DMAX + 1)), e = (uint32_t)(rng() % ((uint64_t)DMAX + 1)),
                   D = (uint32_t)(rng() % ((uint64_t)DMAX + 1));
    const int64_t ra = (int64_t)(rng() % ((uint64_t)RMAX + 1)), rb = (int64_t)(rng() % ((uint64_t)RMAX + 1));
    CHECK((i128)hg_nj_q(c, d, ra, rb) == ref_q(c, d, ra, rb));
    CHECK((i128)hg_nj_len_a(c, D, ra, rb) == ref_len_a(c, D, ra, rb));
    CHECK((i128)hg_nj_update(d, e, D) == ref_update(d, e, D) && hg_nj_update(d, e, D) <= DMAX);
  }
}

// a random valid join list of n items: the lower of two live names stays
static std::vector<hg_nj_join> random_joins(std::mt19937_64 &rng, size_t n) {
  std::vector<uint32_t> live(n);
  for (size_t i = 0; i < n; ++i) live[i] = (uint32_t)i;
  std::vector<hg_nj_join> joins;
  static const int64_t odd[] = {0, 1, -1, 16, 17, -17, INT64_MAX, INT64_MIN, (int64_t)100000 << 15, -((int64_t)100000 << 15)};
  while (live.size() >= 2) {
    size_t x = rng() % live.size(), y = rng() % (live.size() - 1);
    if (y >= x) ++y;
    if (live[x] > live[y]) std::swap(x, y);
    auto length = [&] { return rng() % 4 == 0 ? odd[rng() % 10] : (int64_t)(rng() % ((uint64_t)1 << 33)) - (1 << 20); };
    joins.push_back(hg_nj_join{live[x], live[y], length(), length()});
    live.erase(live.begin() + (long)y);
  }
  return joins;
}

static void check_text(const char *text, size_t len, size_t n, const std::vector<std::string> &names) {
  CHECK(std::strlen(text) == len && len >= 2 && text[len - 1] == ';');
  // outside quoted labels: balanced parentheses, n - 2 inner nodes for n >= 3 (one for n = 2), n labels
  size_t open = 0, close = 0, labels = 0;
  long depth = 0;
  for (size_t i = 0; i < len; ++i) {
    if (text[i] == '\'') {
      std::string got;
      for (++i; i < len; ++i) {
        if (text[i] == '\'') {
          if (i + 1 < len && text[i + 1] == '\'') ++i;
          else break;
        }
        got += text[i];
      }
      CHECK(i < len);
      bool known = false;
      for (const std::string &nm : names) known = known || nm == got;
      CHECK(known);
      ++labels;
    } else if (text[i] == '(') {
      ++open, ++depth;
    } else if (text[i] == ')') {
      ++close, --depth;
      CHECK(depth >= 0);
    }
  }
  CHECK(depth == 0 && labels == n && open == close && open == (n >= 3 ? n - 2 : n - 1));
}

static void newick_lists() {
  std::mt19937_64 rng(9);
  // literals
  {
    const int64_t K = (int64_t)1000 << 15;
    const hg_nj_join five[] = {{0, 1, 2 * K, 3 * K}, {0, 2, 3 * K, 4 * K}, {0, 3, 2 * K, 2 * K}, {0, 4, 1 * K, 0}};
    const char *names[] = {"a", "b", "c", "d", "e"};
    char *out = nullptr;
    size_t len = 0;
    CHECK(hg_nj_newick(five, 5, names, &out, &len) == HG_OK);
    CHECK(std::string(out) == "((('a':0.02000000,'b':0.03000000):0.03000000,'c':0.04000000):0.02000000,'d':0.02000000,'e':0.01000000);");
    hg_free(out);
    CHECK(hg_nj_newick(nullptr, 1, names, &out, &len) == HG_OK && std::string(out) == "'a';" && len == 4);
    hg_free(out);
    const hg_nj_join neg[] = {{0, 1, -17, -16}};
    CHECK(hg_nj_newick(neg, 2, names, &out, nullptr) == HG_OK && std::string(out) == "('a':-0.00000001,'b':0.00000000);");
    hg_free(out);
  }
  for (int round = 0; round < 3000; ++round) {
    const size_t n = 1 + rng() % 60;
    std::vector<std::string> names(n);
    for (size_t i = 0; i < n; ++i) {
      static const char alphabet[] = "ab'():;, /._-Z9";
      const size_t l = rng() % 9;
      for (size_t k = 0; k < l; ++k) names[i] += alphabet[rng() % (sizeof alphabet - 1)];
    }
    std::vector<const char *> ptrs(n);
    for (size_t i = 0; i < n; ++i) ptrs[i] = names[i].c_str();
    std::vector<hg_nj_join> joins = random_joins(rng, n);
    CHECK(joins.size() == n - 1);
    // exactly n - 1 records are allocated: a read behind them is a report
    hg_nj_join *exact = static_cast<hg_nj_join *>(std::malloc((n - 1) * sizeof(hg_nj_join) + 1));
    if (n > 1) std::memcpy(exact, joins.data(), (n - 1) * sizeof(hg_nj_join));
    char *out = nullptr;
    size_t len = 0;
    CHECK(hg_nj_newick(exact, n, ptrs.data(), &out, &len) == HG_OK && out);
    check_text(out, len, n, names);
    hg_free(out);
    if (n >= 2) {
      // broken in one place: a >= b, a name >= n, a dead name reused
      const size_t t = rng() % (n - 1);
      const hg_nj_join keep = exact[t];
      const int how = (int)(rng() % 5);
      bool broken = true;
      if (how == 0) std::swap(exact[t].a, exact[t].b);
      else if (how == 1) exact[t].b = exact[t].a;
      else if (how == 2) exact[t].b = (uint32_t)n + (uint32_t)(rng() % 2) * 0x7FFFFFF0u;
      else if (how == 3) exact[t].a = 0xFFFFFFFFu;
      else if (t + 1 < n - 1) exact[t + 1].b = keep.b, exact[t + 1].a = std::min(exact[t + 1].a, keep.b - 1);  // (b of join t is dead)
      else broken = false;
      if (broken) {
        out = reinterpret_cast<char *>(1);
        len = 99;
        CHECK(hg_nj_newick(exact, n, ptrs.data(), &out, &len) == HG_ERR_INVALID && out == nullptr && len == 0);
      }
      // garbage: any status, never a read out of bounds
      for (size_t k = 0; k + 1 < n; ++k) exact[k] = hg_nj_join{(uint32_t)rng() % (uint32_t)(n + 2), (uint32_t)rng() % (uint32_t)(n + 2), (int64_t)rng(), (int64_t)rng()};
      out = nullptr;
      const hg_status s = hg_nj_newick(exact, n, ptrs.data(), &out, &len);
      CHECK(s == HG_OK || s == HG_ERR_INVALID);
      if (s == HG_OK) check_text(out, len, n, names);
      hg_free(out);
    }
    std::free(exact);
  }
  // NULL arguments and n = 0
  const char *two[] = {"a", "b"};
  const hg_nj_join one[] = {{0, 1, 5, 0}};
  char *out = nullptr;
  CHECK(hg_nj_newick(one, 2, two, nullptr, nullptr) == HG_ERR_INVALID);
  CHECK(hg_nj_newick(nullptr, 2, two, &out, nullptr) == HG_ERR_INVALID && hg_nj_newick(one, 2, nullptr, &out, nullptr) == HG_ERR_INVALID);
  CHECK(hg_nj_newick(one, 0, two, &out, nullptr) == HG_ERR_INVALID && out == nullptr);
  const char *hole[] = {"a", nullptr};
  CHECK(hg_nj_newick(one, 2, hole, &out, nullptr) == HG_ERR_INVALID);
}

int main() {
  math_at_the_bounds();
  newick_lists();
  std::printf("nj driver ok\n");
  return 0;
}
