// hg_hostfed_layout.h -- the host-fed batch (hg_sketch_batch in hg_api_sketch.hip) as arithmetic: whether it crosses the link
// 2-bit packed, where every genome and every blob lies in the device buffer, where a sub-batch ends, which upload route it
// takes and how its packing is shared out.  No HIP, no threads: checked on the CPU by tests/native/hostfed_layout_driver.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>
#include "hg_pack2.h"

constexpr uint64_t HG_STAGE_BYTES = 64ull << 20;                   // padded ASCII bytes at which a sub-batch closes
constexpr uint64_t HG_PACK_BYTES = HG_STAGE_BYTES + (2ull << 20);  // a staging buffer: a sub-batch of genomes < 1 MiB each fits
constexpr uint64_t HG_PACK_PIECE = 1ull << 20;       // bases one hg_pack2_piece call packs (a multiple of 64, as that requires)
constexpr uint64_t HG_PACK_TASK_MIN = 256ull << 10;  // bases a task handed to the pool holds at least

enum HostfedHook : int { HOSTFED_AUTO = 0, HOSTFED_ASCII, HOSTFED_PACKED };  // debug key "hostfed"

// Does the batch cross the link packed, and with how many host threads?  The link is what limits the entry point (50 GB/s =
// 10 k genomes/s of 5 Mbp as ASCII): a batch that is worth it goes over as hg_pack2 blobs, 0.375 bytes per base, packed by a
// few host threads of the call while the previous sub-batch uploads.  Needs cores: with fewer than 4 usable ones the ASCII
// path stays, and so do batches of genomes below 1 kbp on average (blobs carry 32 bytes of padding each).  The threads are
// shared with the other host-fed calls in flight.
struct HostfedDecision {
  bool want_pack;
  unsigned threads;
};
inline HostfedDecision hostfed_decide(unsigned usable_threads, uint64_t all_bytes, size_t n, int others, HostfedHook hook) {
  const bool want = (usable_threads >= 4 && all_bytes >= (32ull << 20) && all_bytes / n >= (1u << 10) && hook != HOSTFED_ASCII) ||
                    (n > 1 && hook == HOSTFED_PACKED);
  return {want, want ? std::max(1u, usable_threads / (unsigned)(1 + others)) : usable_threads};
}
// bytes at which a sub-batch closes (hook: debug key "hostfed_stage_bytes", 0 = HG_STAGE_BYTES); packed: 48 MB per upload
inline uint64_t hostfed_stage_bytes(bool want_pack, uint64_t hook) { return (hook ? hook : HG_STAGE_BYTES) * (want_pack ? 2 : 1); }

struct HostfedSub {  // genomes [g0, g1)
  size_t g0, g1;
  uint64_t span;      // bytes of its ASCII region, from offs[g0]
  uint64_t pk_bytes;  // bytes of its blobs (0 unless the batch wants packing)
  bool packed;        // its blobs go over the link and lie at the start of its ASCII region
};
enum class HostfedRoute { PACKED, STAGED, DIRECT };
struct HostfedPackWork {  // the packing of one sub-batch: task t packs pieces [task_first[t], task_first[t + 1])
  struct Piece {
    size_t g;
    uint64_t b0, b1;  // bases [b0, b1) of genome g
  };
  std::vector<Piece> pieces;
  std::vector<size_t> task_first;
  size_t tasks() const { return task_first.size() - 1; }
};

struct HostfedLayout {
  std::vector<uint64_t> offs, lens, boffs;  // per genome: start of its ASCII region (16-byte aligned), bases, start of its blob
  std::vector<HostfedSub> subs;
  uint64_t total = 0;  // bytes of all ASCII regions; the device buffer holds 64 more
  uint64_t pack_bytes;

  static uint64_t padded(uint64_t len) { return (len + 15) & ~(uint64_t)15; }
  static uint64_t blob(uint64_t len) { return hg_pack2_code_bytes(len) + hg_pack2_mask_bytes(len); }  // hg_pack2_size

  HostfedLayout(const size_t *lens_, size_t n, bool want_pack, uint64_t stage_bytes, uint64_t pack_bytes_)
      : offs(n), lens(lens_, lens_ + n), boffs(n, 0), pack_bytes(pack_bytes_) {
    size_t g0 = 0;
    for (size_t g = 0; g < n; ++g) {  // a sub-batch is cut when its bytes have reached stage_bytes before the next genome
      if (total - offs[g0] >= stage_bytes) close(g0, g, want_pack), g0 = g;
      offs[g] = total, total += padded(lens[g]);
    }
    close(g0, n, want_pack);
  }
  // how sub-batch k goes over the link, as its `packed` stands now
  HostfedRoute route(size_t k) const {
    const HostfedSub &s = subs[k];
    if (s.packed) return HostfedRoute::PACKED;
    // many small genomes: through page-locked staging in the device layout, one upload -- a copy per 2 kbp genome costs more
    // than the genome
    const uint64_t m = s.g1 - s.g0;
    return m >= 16 && s.span / m < ((uint64_t)1 << 20) && s.span <= pack_bytes ? HostfedRoute::STAGED : HostfedRoute::DIRECT;
  }
  // every sub-batch behind k goes as ASCII (the host packs too slowly)
  void demote_after(size_t k) {
    for (size_t j = k + 1; j < subs.size(); ++j) subs[j].packed = false;
  }
  // Pieces of 1 Mbase, so that the threads finish together whatever the genome sizes, handed out in runs of at least
  // 256 kbase: a task per 5 kbp genome cost more in the pool's hand-overs than in packing (100 000 x 5 kbp: 107 ms packed
  // against 30 ms as ASCII through one staging copy)
  HostfedPackWork pack_work(size_t k) const {
    HostfedPackWork w;
    w.task_first.push_back(0);
    uint64_t in_task = 0;
    for (size_t g = subs[k].g0; g < subs[k].g1; ++g)
      for (uint64_t b = 0; b < lens[g]; b += HG_PACK_PIECE) {
        if (in_task >= HG_PACK_TASK_MIN) w.task_first.push_back(w.pieces.size()), in_task = 0;
        w.pieces.push_back({g, b, std::min(lens[g], b + HG_PACK_PIECE)});
        in_task += w.pieces.back().b1 - b;
      }
    w.task_first.push_back(w.pieces.size());
    return w;
  }

 private:
  // Blob g of a sub-batch lies at the sub-batch's own start in the device buffer + the blob sizes in front of it.  A
  // sub-batch whose blobs outgrow a staging buffer (one huge genome) stays ASCII, and so does one whose blobs outgrow its own
  // ASCII region (a blob of 1..16 bases has 32 bytes, their padded ASCII 16: a sub-batch of very short sequences) -- they would
  // run into the next sub-batch's region or, for the last one, past the end of the buffer.
  void close(size_t g0, size_t g1, bool want_pack) {
    HostfedSub s{g0, g1, total - offs[g0], 0, false};
    if (want_pack) {
      for (size_t g = g0; g < g1; ++g) boffs[g] = offs[g0] + s.pk_bytes, s.pk_bytes += blob(lens[g]);
      s.packed = s.pk_bytes > 0 && s.pk_bytes <= pack_bytes && s.pk_bytes <= s.span;
    }
    subs.push_back(s);
  }
};
