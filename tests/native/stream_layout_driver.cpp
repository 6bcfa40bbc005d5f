// AddressSanitizer + UBSan driver (CPU build) for the chunk layout of the streaming sketcher
// (hyper-gen_amd/csrc/hg_stream_layout.h): it plays the uploader of hg_stream.hip -- ask, hand over, open, add, grow --
// over seeded item sequences and checks, for every chunk, the properties the device side relies on.  No expected-output
// file: the block-count and size formulas below are written out independently of the header's.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "../../hyper-gen_amd/csrc/hg_stream_layout.h"

#define CHECK(cond)                                                               \
  do {                                                                            \
    if (!(cond)) {                                                                \
      std::printf("%s:%d: case %s: %s\n", __FILE__, __LINE__, g_case, #cond);     \
      std::exit(1);                                                               \
    }                                                                             \
  } while (0)

namespace {

const char *g_case = "";
size_t al16(size_t x) { return (x + 15) / 16 * 16; }
size_t codes_of(size_t n) { return al16((n + 3) / 4); }
size_t bitmap_of(size_t n) { return al16((n + 7) / 8); }
size_t link_of(const StreamItem &it) {
  return it.kind == KIND_ASCII ? al16(it.len) : it.kind == KIND_PACK2 ? codes_of(it.len) + bitmap_of(it.len) : it.blob_bytes;
}

struct Area {  // a device area as the uploader keeps it: replaced by `want` bytes when `need` exceeds it
  size_t cap;
  void grow(size_t need, size_t want) {
    if (need > cap) {
      CHECK(want >= need);
      cap = want;
    }
  }
};

struct Sim {
  ChunkLimit limit;
  ChunkLayout lay;
  bool open = false, was_idle = true;
  unsigned closed_in_burst = 0;
  Area text[3] = {{TEXT_AREA_MIN}, {TEXT_AREA_MIN}, {TEXT_AREA_MIN}}, packed[3] = {{0}, {0}, {0}};
  unsigned ci = 0;  // the chunks' resources are used in turn
  std::vector<UnpackJob> jobs = std::vector<UnpackJob>(CHUNK_GENOMES);
  std::vector<SparseJob> sjobs = std::vector<SparseJob>(CHUNK_GENOMES);
  std::vector<StreamItem> items;                     // of the open chunk
  std::vector<std::pair<size_t, size_t>> staged;     // regions in the staging mirror no run has taken up yet
  size_t n_chunks = 0, max_genomes = 0, kept_growths = 0, text_growths = 0;

  void run_goes_up(size_t lo, size_t hi) {
    CHECK(lo % 16 == 0 && hi % 16 == 0 && lo <= hi && hi <= CHUNK_BYTES);  // (the mirror has CHUNK_BYTES)
    for (auto &r : staged) CHECK(r.first >= lo && r.second <= hi);
    CHECK(staged.empty() == (lo == hi));
    staged.clear();
  }

  void close() {
    size_t lo, hi;
    lay.take_run(lo, hi);
    run_goes_up(lo, hi);
    const size_t m = items.size();
    CHECK(m >= 1 && m <= CHUNK_GENOMES && lay.n_jobs <= CHUNK_GENOMES && lay.n_sjobs <= CHUNK_GENOMES);
    CHECK(lay.offs.size() == m && lay.lens.size() == m && lay.tags.size() == m && lay.pk_offs.size() == m && lay.mask_offs.size() == m);
    size_t bytes = 0, link = 0, pk_end = 0, n_text = 0;
    uint32_t j = 0, sj = 0, blocks = 0, sblocks = 0;
    bool any_ascii = false;
    for (size_t g = 0; g < m; ++g) {
      const StreamItem &it = items[g];
      CHECK(lay.lens[g] == it.len && lay.tags[g] == it.tag);
      CHECK(lay.offs[g] == bytes && bytes % 16 == 0);  // ASCII regions: aligned, in order, disjoint
      any_ascii |= it.kind == KIND_ASCII;
      if (it.kind == KIND_ASCII || it.len == 0) {
        CHECK(lay.pk_offs[g] == 0 && lay.mask_offs[g] == 0);
        n_text += it.len != 0;
      } else {
        const size_t mb = bitmap_of(it.len), table = it.kind == KIND_PACK2S ? it.blob_bytes - codes_of(it.len) : 0;
        const UnpackJob &jb = jobs[j++];
        CHECK(jb.pk_off == lay.pk_offs[g] && jb.mask_off == lay.mask_offs[g] && jb.out_off == bytes && jb.n_bps == it.len);
        CHECK(jb.pk_off % 16 == 0 && jb.mask_off % 16 == 0 && jb.pk_off >= pk_end);  // blobs: aligned, in order, disjoint
        CHECK(jb.mask_off == jb.pk_off + codes_of(it.len) + table);  // the bitmap behind the codes (and the run table)
        pk_end = jb.mask_off + mb;
        CHECK(jb.first_block == blocks);
        blocks += (uint32_t)(((it.len + 15) / 16 + 1023) / 1024);
        if (it.kind == KIND_PACK2S) {
          const SparseJob &s = sjobs[sj++];
          CHECK(s.codes_off == jb.pk_off && s.mask_off == jb.mask_off && s.n_bps == it.len && s.first_block == sblocks);
          sblocks += (uint32_t)((mb / 4 + 1023) / 1024);
        }
      }
      bytes += al16(it.len), link += link_of(it);
    }
    CHECK(lay.bytes == bytes && lay.link_bytes == link && lay.pk_bytes == pk_end);
    CHECK(lay.n_jobs == j && lay.n_blocks == blocks && lay.n_sjobs == sj && lay.n_sblocks == sblocks);
    CHECK(lay.has_ascii == any_ascii && lay.packed_only() == (j > 0 && n_text == 0));
    // what the kernels touch fits the areas the layout asked for, less the slack
    CHECK(lay.packed_only() || any_ascii || j == 0);
    if (any_ascii) CHECK(bytes + CHUNK_SLACK <= text[ci].cap);
    if (j) CHECK(pk_end + CHUNK_SLACK <= packed[ci].cap);
    ++n_chunks, max_genomes = std::max(max_genomes, m);
    open = false, items.clear(), ci = (ci + 1) % 3;
    limit.chunk_closed(), ++closed_in_burst;
  }

  // waits: the uploader finds its queue still empty when it comes back for the next item (after an idle hand-over)
  void push(const StreamItem &it, bool idle_after, bool waits = true) {
    if (was_idle && waits) limit.new_burst(), closed_in_burst = 0;
    CHECK(limit.bytes == std::min(CHUNK_BYTES, (CHUNK_BYTES / 8) << std::min(closed_in_burst, 3u)));  // the ramp
    if (open && lay.closes_before(it, limit)) close();
    if (!open) lay = ChunkLayout{}, open = true;
    CHECK(!lay.closes_before(it, limit) || !items.empty());
    const size_t bytes0 = lay.bytes, pk0 = lay.pk_bytes;
    const ChunkPlace pl = lay.add(it, jobs.data(), sjobs.data());
    items.push_back(it);
    // the growth invariants: the ASCII buffer is replaced only while the chunk has no bytes, the packed area of a chunk
    // sized by its blobs only before its first blob
    if (pl.text_need > text[ci].cap) {
      CHECK(bytes0 == 0);
      ++text_growths;
    }
    if (pl.packed_need > packed[ci].cap) {
      CHECK(pl.packed_keep == pk0 && (lay.has_ascii || pk0 == 0));
      kept_growths += pk0 != 0;
    }
    text[ci].grow(pl.text_need, pl.text_want), packed[ci].grow(pl.packed_need, pl.packed_want);
    CHECK((pl.text_need != 0) == lay.has_ascii && (pl.packed_need != 0) == (pl.area == ChunkPlace::PACKED));
    if (pl.area == ChunkPlace::STAGE) {
      CHECK(pl.off == bytes0 && pl.n == it.len && it.len < SMALL_BYTES && bytes0 + al16(it.len) <= CHUNK_BYTES);
      staged.emplace_back(bytes0, bytes0 + al16(it.len));
    } else if (pl.area == ChunkPlace::TEXT) {
      CHECK(pl.off == bytes0 && pl.n == it.len);
      size_t lo, hi;
      lay.take_run(lo, hi);  // (the pending run goes up before a genome's own copy)
      run_goes_up(lo, hi);
    } else if (pl.area == ChunkPlace::PACKED) {
      CHECK(pl.off == pk0 && pl.n == link_of(it) && pl.off + pl.n <= lay.pk_bytes);
    } else {
      CHECK(it.len == 0);
    }
    // a chunk of several genomes stays within the limit under its own sizing rule
    if (items.size() > 1) CHECK((lay.has_ascii ? lay.bytes : lay.link_bytes) <= limit.bytes);
    if (lay.closes_after(idle_after, limit)) close();
    CHECK(!open || (!idle_after && items.size() < CHUNK_GENOMES));
    was_idle = idle_after;
  }
};

StreamItem item(int kind, size_t len, size_t n_runs, uint64_t tag) {
  return StreamItem{nullptr, len, tag, kind, kind == KIND_PACK2S && len ? codes_of(len) + al16(8 + 8 * n_runs) : 0};
}

}  // namespace

int main() {
  const size_t lens[] = {0, 1, 15, 16, 17, SMALL_BYTES - 1, SMALL_BYTES, SMALL_BYTES + 1, CHUNK_BYTES / 8 - 17,
                         CHUNK_BYTES / 8, CHUNK_BYTES / 8 + 1, CHUNK_BYTES + 12345};
  const size_t n_lens = sizeof lens / sizeof lens[0];
  size_t chunks = 0, text_growths = 0;
  g_case = "random";
  for (uint64_t seed = 1; seed <= 40; ++seed) {
    std::mt19937_64 rng(seed);
    Sim sim;
    const unsigned idle_one_in = 1u << (seed % 6), tiny_bias = seed % 3;  // idle after every item ... after one in 32
    for (int i = 0; i < 3000; ++i) {
      const size_t len = lens[rng() % (tiny_bias && rng() % 4 ? 5 : n_lens)];
      const int kind = (int)(rng() % 3);
      const size_t n_runs = len ? (rng() % 4 ? rng() % 50 : rng() % (len / 2 + 1)) : 0;  // (runs are disjoint and not adjacent)
      sim.push(item(kind, len, n_runs, (uint64_t)i), rng() % idle_one_in == 0, rng() % 2);
    }
    sim.push(item(KIND_ASCII, 5, 0, 0), true);  // the input ends: the open chunk goes
    CHECK(!sim.open);
    chunks += sim.n_chunks, text_growths += sim.text_growths;
  }
  CHECK(text_growths > 0);

  g_case = "5000 tiny";
  for (int only = -1; only < 3; ++only) {  // kinds mixed, then each alone
    Sim sim;
    for (int i = 0; i < 5000; ++i) sim.push(item(only < 0 ? i % 3 : only, lens[1 + i % 4], 1, (uint64_t)i), i == 4999);
    CHECK(!sim.open && sim.n_chunks == 2 && sim.max_genomes == CHUNK_GENOMES);
    chunks += sim.n_chunks;
  }

  // Why the packed area keeps its blobs when it grows: a chunk sized by ASCII bytes takes sparse genomes whose run tables
  // are several times their ASCII (a run per two bases), and outgrows PACKED_AREA_MIN with blobs in place.
  g_case = "run-heavy sparse genomes among ASCII";
  {
    Sim sim;
    for (int i = 0; i < 400; ++i) {
      const size_t len = i % 2 ? 4u << 20 : 1;
      sim.push(item(i % 2 ? KIND_PACK2S : KIND_ASCII, len, len / 2, (uint64_t)i), i == 399);
    }
    CHECK(!sim.open && sim.kept_growths > 0);
    chunks += sim.n_chunks;
  }
  std::printf("stream layout driver ok (%zu chunks)\n", chunks);
  return 0;
}
