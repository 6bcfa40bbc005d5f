// ThreadSanitizer driver (CPU build) for the host threads of a host-fed call: CallPool + hg_pack2_piece
// (hyper-gen_amd/csrc/hg_host.h, hg_formats.cpp) -- the way hg_sketch_batch packs a sub-batch -- against hg_pack2, and
// Handover, through which its uploader thread passes the sub-batches to the thread that sketches them.
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "../../hyper-gen_amd/csrc/hg_host.h"

// A producer fills slot k - 1 and publishes k = 1..N, or fails at a random k; the consumer waits for each k in turn and reads
// the slot (plain memory: the hand-over is what orders the two), as hg_sketch_batch reads the layout's flags.
static int handover_case() {
  std::mt19937_64 rng(11);
  for (int run = 0; run < 200; ++run) {
    const size_t N = 1 + rng() % 40, fail_at = run % 3 ? N : rng() % N;  // (fail_at == N: no failure)
    const int err = 1 + (int)(rng() % 1000);
    std::vector<uint64_t> slot(N, 0);
    Handover h;
    std::thread producer([&] {
      for (size_t k = 0; k < N; ++k) {
        if (k == fail_at) return h.fail(err);
        slot[k] = 1000 + k;
        h.publish(k + 1);
      }
    });
    size_t seen = 0;
    int got = 0;
    for (size_t k = 0; k < N && !(got = h.wait(k)); ++k, ++seen)
      if (slot[k] != 1000 + k) return 1;
    producer.join();
    if (fail_at == N ? (got != 0 || seen != N) : (got != err || seen > fail_at)) return 1;
    if (fail_at < N && h.wait(0) != err) return 1;  // (the error stays)
  }
  return 0;
}

int main() {
  if (handover_case()) {
    std::printf("hand-over: wrong order or error\n");
    return 4;
  }
  std::mt19937_64 rng(7);
  const char alpha[] = "ACGTacgtNnUuRY-";
  const size_t lens[] = {0, 1, 63, 64, 65, 1000, (1u << 20) - 1, 1u << 20, (1u << 20) + 1, 3 * (1u << 20) + 77, 2500000};
  std::vector<std::vector<uint8_t>> seqs;
  for (size_t n : lens) {
    std::vector<uint8_t> s(n);
    for (auto &c : s) c = (uint8_t)alpha[rng() % (sizeof alpha - 1)];
    if (n > 300) std::memset(s.data() + n / 3, 'N', 200);
    seqs.push_back(std::move(s));
  }
  for (unsigned threads : {1u, 2u, 7u}) {
    CallPool pool(threads);
    for (int round = 0; round < 3; ++round) {  // the pool is reused sub-batch after sub-batch
      for (uint32_t norm : {HG_NORM_ACGT, HG_NORM_U2T}) {
        std::vector<size_t> off;
        size_t total = 0;
        for (auto &s : seqs) off.push_back(total), total += hg_pack2_size(s.size());
        std::vector<uint8_t> got(total + 1, 0xEE), want(total + 1, 0xEE);
        constexpr size_t PIECE = 1u << 20;
        std::vector<std::pair<size_t, size_t>> pieces;
        for (size_t g = 0; g < seqs.size(); ++g)
          for (size_t b = 0; b < seqs[g].size(); b += PIECE) pieces.emplace_back(g, b);
        pool.run(pieces.size(), [&](size_t i) {
          const size_t g = pieces[i].first, b = pieces[i].second, n = seqs[g].size();
          hg_pack2_piece(seqs[g].data(), n, norm, got.data() + off[g], b, b + PIECE < n ? b + PIECE : n);
        });
        pool.run(0, [&](size_t) { std::abort(); });
        for (size_t g = 0; g < seqs.size(); ++g)
          if (hg_pack2(seqs[g].data(), seqs[g].size(), norm, want.data() + off[g]) != HG_OK) return 2;
        if (got != want) {
          std::printf("pieces differ from hg_pack2 (threads %u, norm %u)\n", threads, norm);
          return 3;
        }
      }
    }
  }
  std::printf("tsan driver ok\n");
  return 0;
}
