// AddressSanitizer + UBSan driver (CPU build) for the layout of a host-fed batch (hyper-gen_amd/csrc/hg_hostfed_layout.h).
// The model is the pair of loops hg_sketch_batch had before the unit existed (cut / offs / boffs / sub_packed, pieces /
// task_first), written out here as they stood; every field of the unit is compared against it over seeded length lists, and
// the properties the uploader and the device side rely on are checked on their own.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../hyper-gen_amd/csrc/hg_hostfed_layout.h"

#define CHECK(cond)                                                               \
  do {                                                                            \
    if (!(cond)) {                                                                \
      std::printf("%s:%d: case %s: %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); \
      std::exit(1);                                                               \
    }                                                                             \
  } while (0)

namespace {

std::string g_case;
uint64_t al16(uint64_t x) { return (x + 15) / 16 * 16; }
uint64_t pack2_size(uint64_t n) { return al16((n + 3) / 4) + al16((n + 7) / 8); }  // hg_pack2_size, written out

struct Model {  // the loops of hg_sketch_batch before the unit, unchanged but for the two parameters
  std::vector<uint64_t> offs, boffs;
  std::vector<size_t> cut{0};
  std::vector<uint8_t> sub_packed;
  std::vector<uint64_t> sub_pk_bytes, sub_span;
  uint64_t total = 0;
  Model(const std::vector<size_t> &lens, bool want_pack, uint64_t stage_bytes, uint64_t pack_bytes) : offs(lens.size()), boffs(lens.size()) {
    const size_t n = lens.size();
    uint64_t in_chunk = 0;
    for (size_t g = 0; g < n; ++g) {
      if (in_chunk >= stage_bytes) cut.push_back(g), in_chunk = 0;
      offs[g] = total;
      const uint64_t padded = (lens[g] + 15) & ~(uint64_t)15;
      total += padded, in_chunk += padded;
    }
    cut.push_back(n);
    const size_t n_chunks = cut.size() - 1;
    sub_packed.assign(n_chunks, 0), sub_pk_bytes.assign(n_chunks, 0), sub_span.assign(n_chunks, 0);
    for (size_t k = 0; k < n_chunks; ++k) {
      const uint64_t span = offs[cut[k + 1] - 1] + ((lens[cut[k + 1] - 1] + 15) & ~(uint64_t)15) - offs[cut[k]];
      sub_span[k] = span;
      if (!want_pack) continue;
      uint64_t at = 0;
      for (size_t g = cut[k]; g < cut[k + 1]; ++g) boffs[g] = offs[cut[k]] + at, at += pack2_size(lens[g]);
      sub_pk_bytes[k] = at;
      sub_packed[k] = at <= pack_bytes && at <= span && at > 0;
    }
  }
};

void model_pieces(const std::vector<size_t> &lens, size_t g0, size_t g1, std::vector<std::pair<size_t, uint64_t>> &pieces,
                  std::vector<size_t> &task_first) {
  constexpr uint64_t PIECE = 1ull << 20;
  for (size_t g = g0; g < g1; ++g)
    for (uint64_t b = 0; b < lens[g]; b += PIECE) pieces.emplace_back(g, b);
  task_first.assign(1, 0);
  uint64_t in_task = 0;
  for (size_t i = 0; i < pieces.size(); ++i) {
    if (in_task >= (256u << 10)) task_first.push_back(i), in_task = 0;
    in_task += std::min<uint64_t>(lens[pieces[i].first] - pieces[i].second, PIECE);
  }
  task_first.push_back(pieces.size());
}

size_t n_packed_subs = 0, n_ascii_among_packed = 0, n_routes[3] = {0, 0, 0}, n_multi_task = 0;

void check(const std::vector<size_t> &lens, bool want_pack, uint64_t stage_bytes, uint64_t pack_bytes) {
  const size_t n = lens.size();
  HostfedLayout lay(lens.data(), n, want_pack, stage_bytes, pack_bytes);
  const Model m(lens, want_pack, stage_bytes, pack_bytes);
  // -- against the model
  CHECK(lay.total == m.total && lay.offs == m.offs && lay.boffs == m.boffs && lay.pack_bytes == pack_bytes);
  CHECK(lay.lens.size() == n && lay.subs.size() == m.cut.size() - 1);
  for (size_t g = 0; g < n; ++g) CHECK(lay.lens[g] == lens[g]);
  for (size_t k = 0; k < lay.subs.size(); ++k) {
    const HostfedSub &s = lay.subs[k];
    CHECK(s.g0 == m.cut[k] && s.g1 == m.cut[k + 1] && s.span == m.sub_span[k] && s.pk_bytes == m.sub_pk_bytes[k] && s.packed == (m.sub_packed[k] != 0));
    const uint64_t cnt = s.g1 - s.g0;
    const HostfedRoute want = m.sub_packed[k] ? HostfedRoute::PACKED
                              : cnt >= 16 && s.span / cnt < ((uint64_t)1 << 20) && s.span <= pack_bytes ? HostfedRoute::STAGED : HostfedRoute::DIRECT;
    CHECK(lay.route(k) == want);
    ++n_routes[(int)want];
  }
  // -- on their own: genome regions
  uint64_t end = 0;
  for (size_t g = 0; g < n; ++g) {
    CHECK(lay.offs[g] % 16 == 0 && lay.offs[g] == end);  // aligned, ascending, disjoint, no gaps
    end = lay.offs[g] + al16(lens[g]);
  }
  CHECK(lay.total == end);
  // -- sub-batches
  CHECK(!lay.subs.empty() && lay.subs.front().g0 == 0 && lay.subs.back().g1 == n);
  for (size_t k = 0; k < lay.subs.size(); ++k) {
    const HostfedSub &s = lay.subs[k];
    CHECK(s.g0 < s.g1 && (k == 0 || s.g0 == lay.subs[k - 1].g1));
    uint64_t bytes = 0;
    for (size_t g = s.g0; g < s.g1; ++g) bytes += al16(lens[g]);
    CHECK(s.span == bytes);
    if (k + 1 < lay.subs.size()) CHECK(bytes >= stage_bytes && bytes - al16(lens[s.g1 - 1]) < stage_bytes);
    if (!want_pack) CHECK(!s.packed && s.pk_bytes == 0);
    if (!s.packed) {
      n_ascii_among_packed += want_pack;
      if (lay.route(k) == HostfedRoute::STAGED) CHECK(s.span <= pack_bytes);  // (the staging buffer holds pack_bytes)
      continue;
    }
    ++n_packed_subs;
    // blobs: disjoint, ascending, inside the sub-batch's own ASCII region; the staging buffer holds them
    uint64_t at = lay.offs[s.g0];
    for (size_t g = s.g0; g < s.g1; ++g) {
      CHECK(lay.boffs[g] == at && at % 16 == 0);
      at += pack2_size(lens[g]);
    }
    CHECK(at - lay.offs[s.g0] == s.pk_bytes && s.pk_bytes > 0 && s.pk_bytes <= pack_bytes && at <= lay.offs[s.g0] + s.span);
    // packing work: against the model, then: every base exactly once, piece starts on multiples of 1 << 20, tasks of 256 kbase
    const HostfedPackWork w = lay.pack_work(k);
    std::vector<std::pair<size_t, uint64_t>> mp;
    std::vector<size_t> mt;
    model_pieces(lens, s.g0, s.g1, mp, mt);
    CHECK(w.pieces.size() == mp.size() && w.task_first == mt && w.tasks() == mt.size() - 1);
    size_t g = s.g0;
    uint64_t b = 0;
    for (size_t i = 0; i < w.pieces.size(); ++i) {
      const HostfedPackWork::Piece &pc = w.pieces[i];
      CHECK(pc.g == mp[i].first && pc.b0 == mp[i].second && pc.b1 == std::min<uint64_t>(lens[pc.g], pc.b0 + ((uint64_t)1 << 20)));
      while (g < s.g1 && b == lens[g]) ++g, b = 0;  // (genomes without bases have no piece)
      CHECK(pc.g == g && pc.b0 == b && pc.b0 % ((uint64_t)1 << 20) == 0 && pc.b1 > pc.b0 && pc.b1 <= lens[g]);
      b = pc.b1;
    }
    while (g < s.g1 && b == lens[g]) ++g, b = 0;
    CHECK(g == s.g1);
    CHECK(w.task_first.front() == 0 && w.task_first.back() == w.pieces.size());
    for (size_t t = 0; t < w.tasks(); ++t) {
      CHECK(w.task_first[t] < w.task_first[t + 1] || w.pieces.empty());
      uint64_t bases = 0;
      for (size_t i = w.task_first[t]; i < w.task_first[t + 1]; ++i) bases += w.pieces[i].b1 - w.pieces[i].b0;
      if (t + 1 < w.tasks()) CHECK(bases >= (256u << 10));
    }
    n_multi_task += w.tasks() > 1;
  }
  // -- demotion behind every k: 0..k untouched, the rest ASCII with its route read from the new flag
  for (size_t k = 0; k < lay.subs.size(); ++k) {
    HostfedLayout d = lay;
    d.demote_after(k);
    CHECK(d.offs == lay.offs && d.boffs == lay.boffs && d.total == lay.total && d.subs.size() == lay.subs.size());
    for (size_t j = 0; j < d.subs.size(); ++j) {
      const HostfedSub &a = d.subs[j], &b = lay.subs[j];
      CHECK(a.g0 == b.g0 && a.g1 == b.g1 && a.span == b.span && a.pk_bytes == b.pk_bytes);
      CHECK(a.packed == (j <= k && b.packed));
      if (j <= k) CHECK(d.route(j) == lay.route(j));
      else CHECK(d.route(j) != HostfedRoute::PACKED);
    }
  }
}

// the expression hg_sketch_batch had for the batch-level decision
void model_decide(unsigned P, uint64_t all_bytes, size_t n, int others, const std::string &dbg_hostfed, bool &want_pack, unsigned &threads) {
  want_pack = (P >= 4 && all_bytes >= (32ull << 20) && all_bytes / n >= (1u << 10) && dbg_hostfed != "ascii") || (n > 1 && dbg_hostfed == "packed");
  if (want_pack) P = std::max(1u, P / (unsigned)(1 + others));
  threads = P;
}

}  // namespace

int main() {
  static_assert(HG_STAGE_BYTES == 64ull << 20 && HG_PACK_BYTES == (66ull << 20) && HG_PACK_PIECE % 64 == 0, "constants of the unit");
  const uint64_t stages[] = {64, 4096, 1 << 20, 64 << 20}, packs[] = {4096, HG_PACK_BYTES};
  for (uint64_t seed = 1; seed <= 12; ++seed) {
    std::mt19937_64 rng(seed);
    for (uint64_t stage : stages) {
      std::vector<size_t> lens;
      const size_t n = 1 + rng() % (seed % 3 ? 400 : 40);
      bool above = false;
      for (size_t i = 0; i < n; ++i) {
        const unsigned kind = (unsigned)(rng() % 16);
        size_t len;
        if (kind < 2) len = 0;
        else if (kind < 7) len = 1 + rng() % 16;
        else if (kind < 12) len = 1000 + rng() % 8000;
        else if (kind < 15) len = (1u << 20) - 40 + rng() % 80;  // around 1 MiB
        else if (!above || stage <= (1 << 20)) len = stage + 1 + rng() % 3000, above = true;  // above stage_bytes (one at 64 MiB)
        else len = 3 * (1u << 20) + rng() % 1000;
        lens.push_back(len);
      }
      if (!above) lens.push_back(stage + 17);
      for (uint64_t pack : packs)
        for (int want = 0; want < 2; ++want) {
          g_case = "seed " + std::to_string(seed) + " stage " + std::to_string(stage) + " pack " + std::to_string(pack) + " want " + std::to_string(want);
          check(lens, want != 0, stage, pack);
          check(lens, want != 0, hostfed_stage_bytes(want != 0, stage), pack);  // (as the entry point calls it: doubled when packed)
        }
    }
  }
  CHECK(n_packed_subs > 100 && n_ascii_among_packed > 100 && n_routes[0] && n_routes[1] && n_routes[2] && n_multi_task > 0);

  // the three cases of tests/test_gpu_packed.py::test_hostfed_forced_packed_with_very_short_sequences, as the entry point lays
  // them out under "hostfed" = "packed"
  g_case = "very short sequences";
  {
    std::mt19937_64 rng(32);
    std::vector<size_t> tiny(3000);
    for (auto &l : tiny) l = 1 + rng() % 16;
    const uint64_t stage = hostfed_stage_bytes(true, 0);
    CHECK(stage == 2 * HG_STAGE_BYTES && hostfed_stage_bytes(false, 0) == HG_STAGE_BYTES && hostfed_stage_bytes(true, 4096) == 8192);
    HostfedLayout a(tiny.data(), tiny.size(), true, stage, HG_PACK_BYTES);
    CHECK(a.subs.size() == 1 && !a.subs[0].packed && a.route(0) == HostfedRoute::STAGED);
    tiny.push_back(200000);
    HostfedLayout b(tiny.data(), tiny.size(), true, stage, HG_PACK_BYTES);
    CHECK(b.subs.size() == 1 && b.subs[0].packed && b.route(0) == HostfedRoute::PACKED);
    const size_t nine = 9;
    HostfedLayout c(&nine, 1, true, stage, HG_PACK_BYTES);
    CHECK(c.subs.size() == 1 && !c.subs[0].packed && c.route(0) == HostfedRoute::DIRECT);
    check(tiny, true, stage, HG_PACK_BYTES);
  }

  // the batch-level decision against the expression it replaces
  g_case = "decision";
  const char *hooks[] = {"", "ascii", "packed"};
  for (unsigned P : {1u, 3u, 4u, 16u})
    for (uint64_t all_bytes : {(32ull << 20) - 1, 32ull << 20})
      for (int mean_at : {0, 1})    // mean length just below 1 KiB / at 1 KiB
        for (size_t one : {0, 1})   // ... and the single genome, whatever its length
          for (int others : {0, 1, 3, 7, 40})
            for (int h = 0; h < 3; ++h) {
              const size_t n = one ? 1 : (size_t)(all_bytes >> 10) + (mean_at ? 0 : 1);
              if (!one) CHECK((all_bytes / n >= 1024) == (mean_at == 1) && all_bytes / n >= 1023);
              bool want;
              unsigned threads;
              model_decide(P, all_bytes, n, others, hooks[h], want, threads);
              const HostfedDecision d = hostfed_decide(P, all_bytes, n, others, (HostfedHook)h);
              CHECK(d.want_pack == want && d.threads == threads);
            }
  CHECK(hostfed_decide(4, 32ull << 20, 32, 0, HOSTFED_AUTO).want_pack && !hostfed_decide(3, 32ull << 20, 32, 0, HOSTFED_AUTO).want_pack);
  CHECK(hostfed_decide(1, 10, 2, 0, HOSTFED_PACKED).want_pack && !hostfed_decide(1, 10, 1, 0, HOSTFED_PACKED).want_pack);
  std::printf("hostfed layout driver ok (%zu packed sub-batches, %zu left ASCII, routes %zu/%zu/%zu)\n", n_packed_subs,
              n_ascii_among_packed, n_routes[0], n_routes[1], n_routes[2]);
  return 0;
}
