// hg_stream.hip -- continuous host-fed sketching (hg_sketch_stream_*).
//
// hg_sketch_batch overlaps upload and kernels INSIDE one call; a host that produces genomes one at a time (reader
// threads parsing FASTA files: src/sketch_cuda.rs:120-166 walks its file list the same way) pays the ends of every
// call -- the first upload with nothing to overlap, the last sub-batch's kernels and read-back with the link idle
// (~0.4 ms per call) -- and must collect a batch before it can call at all.  Here the two halves never stop:
//   * one uploader thread per device appends the pushed genomes to a ring of device chunks (~64 MB each) on a copy
//     stream; a chunk is handed on when it is full or the moment the input runs dry;
//   * one compute thread per device runs hg_sketch_batch_dev on the chunks as their uploads complete (stream
//     event) and queues the results.
// The PCIe link therefore carries sequence all the time, the kernels (a tenth of the upload time per genome) hide
// under it, and chunk sizes adapt by themselves: when the kernels lag, chunks fill up while the uploader waits.
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "hg_internal.h"
#include "hg_stream_layout.h"

namespace {

constexpr int N_CHUNKS = 3;

struct Chunk {  // the resources of one chunk; what they hold at the moment is `lay`
  ChunkLayout lay;
  uint8_t *d = nullptr;  // device sequence buffer
  size_t cap = 0;
  uint8_t *stage = nullptr;  // page-locked mirror for runs of small genomes (lazily allocated, CHUNK_BYTES)
  hipEvent_t uploaded = nullptr;
  uint8_t *dpk = nullptr;  // hg_pack2 / hg_pack2s blobs (hg_sketch_stream_push_packed*): their own device area
  size_t pk_cap = 0;
  UnpackJob *h_jobs = nullptr, *d_jobs = nullptr;    // CHUNK_GENOMES entries each (page-locked / device), lazily allocated
  SparseJob *h_sjobs = nullptr, *d_sjobs = nullptr;  // hg_pack2s genomes: bitmap rebuild jobs
};

struct Done {  // the results of one chunk
  std::vector<uint64_t> tags;
  std::vector<int16_t> hv;
  std::vector<int32_t> n2;
  std::vector<uint32_t> nh;
  size_t next = 0;
};

}  // namespace

struct hg_sketch_stream {
  struct Engine {
    int device = 0;
    // the compute thread: its ctx (workspaces, stream) and result areas
    hg_ctx *ctx = nullptr;
    int16_t *d_hv = nullptr;  // (one device block: HV rows, norm2, nhash)
    int32_t *d_n2 = nullptr;
    uint32_t *d_nh = nullptr;
    uint8_t *h_res = nullptr;  // page-locked read-back area
    std::thread comp;
    hipStream_t copy = nullptr;
    // A second copy stream for the genomes' own uploads, used in turn with `copy`: a copy command costs ~7 us of link
    // idle time whatever it moves (ASCII 5 MB: 50 GB/s; hg_pack2 1.9 MB: 42; hg_pack2s 1.25 MB: 36 -- the bench's
    // packed_stream legs), and with two queues the command overhead of one runs under the transfer of the other.
    hipStream_t copy2 = nullptr;
    hipEvent_t copy2_done = nullptr;  // "everything queued on copy2 for the chunk being handed over"
    unsigned turn = 0;
    Chunk chunk[N_CHUNKS];
    std::deque<StreamItem> in;
    std::deque<int> free_chunks, full_chunks;
    size_t load = 0;  // bytes pushed to this engine whose results are not out yet
    bool uploader_done = false;
    std::thread up;
    // diagnostics (hg_sketch_stream_stats): seconds spent per phase, chunks handed over
    double t_up_idle = 0, t_up_nochunk = 0, t_up_copy = 0, t_comp_idle = 0, t_comp_run = 0;
    size_t n_chunks = 0;
  };
  std::vector<Engine *> eng;
  hg_sketch_params p{};
  std::mutex mu;
  std::condition_variable cv_in, cv_chunk, cv_out, cv_room;
  std::deque<Done> out;
  size_t pushed = 0, popped = 0, max_pending = 4096;
  bool finishing = false;
  hg_status err = HG_OK;
  std::string msg;
};

namespace {

using Engine = hg_sketch_stream::Engine;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void fail(hg_sketch_stream *s, hg_status st, const std::string &m) {
  std::lock_guard<std::mutex> lk(s->mu);
  if (s->err == HG_OK) s->err = st, s->msg = m;
  s->cv_in.notify_all(), s->cv_chunk.notify_all(), s->cv_out.notify_all(), s->cv_room.notify_all();
}

#define ST_HIP(s, expr)                                                                    \
  do {                                                                                     \
    hipError_t e__ = (expr);                                                               \
    if (e__ != hipSuccess) {                                                               \
      fail((s), HG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));           \
      return false;                                                                        \
    }                                                                                      \
  } while (0)

// the pending run of small genomes of chunk c goes up as one copy
bool flush_run(hg_sketch_stream *s, Engine &e, Chunk &c) {
  size_t lo, hi;
  c.lay.take_run(lo, hi);
  if (hi > lo) ST_HIP(s, hipMemcpyAsync(c.d + lo, c.stage + lo, hi - lo, hipMemcpyHostToDevice, e.copy));
  return true;
}

bool hand_over(hg_sketch_stream *s, Engine &e, int ci) {
  Chunk &c = e.chunk[ci];
  if (!flush_run(s, e, c)) return false;
  if (c.lay.n_jobs) ST_HIP(s, hipMemcpyAsync(c.d_jobs, c.h_jobs, c.lay.n_jobs * sizeof(UnpackJob), hipMemcpyHostToDevice, e.copy));
  if (c.lay.n_sjobs) ST_HIP(s, hipMemcpyAsync(c.d_sjobs, c.h_sjobs, c.lay.n_sjobs * sizeof(SparseJob), hipMemcpyHostToDevice, e.copy));
  ST_HIP(s, hipEventRecord(e.copy2_done, e.copy2));  // the chunk's uploads on the second stream join the first
  ST_HIP(s, hipStreamWaitEvent(e.copy, e.copy2_done, 0));
  ST_HIP(s, hipEventRecord(c.uploaded, e.copy));
  std::lock_guard<std::mutex> lk(s->mu);
  e.full_chunks.push_back(ci);
  s->cv_chunk.notify_all();
  return true;
}

// An area of a chunk grows (ChunkPlace).  Nothing to keep: the old block is idle and goes first; else the copies into it are awaited.
bool regrow(hg_sketch_stream *s, Engine &e, uint8_t *&p, size_t &cap, size_t want, size_t keep) {
  if (keep) {
    ST_HIP(s, hipStreamSynchronize(e.copy));
    ST_HIP(s, hipStreamSynchronize(e.copy2));
  } else if (p) {
    ST_HIP(s, hipFree(p));
    p = nullptr, cap = 0;
  }
  uint8_t *nb = nullptr;
  const hipError_t he = hipMalloc(reinterpret_cast<void **>(&nb), want);
  if (he != hipSuccess) {
    fail(s, HG_ERR_OOM, "hipMalloc(" + std::to_string(want) + "): " + hipGetErrorString(he));
    return false;
  }
  if (p) {
    ST_HIP(s, hipMemcpy(nb, p, keep, hipMemcpyDeviceToDevice));
    ST_HIP(s, hipFree(p));
  }
  p = nb, cap = want;
  return true;
}

void uploader(hg_sketch_stream *s, Engine *ep) {
  Engine &e = *ep;
  auto body = [&]() -> bool {
    ST_HIP(s, hipSetDevice(e.device));
    int cur = -1;
    ChunkLimit limit;
    auto close_chunk = [&] { return limit.chunk_closed(), hand_over(s, e, std::exchange(cur, -1)); };  // (the next one may be twice as large)
    for (;;) {
      StreamItem it{};
      bool idle_after;
      {
        const double tw = now_s();
        std::unique_lock<std::mutex> lk(s->mu);
        if (e.in.empty() && cur < 0) limit.new_burst();
        s->cv_in.wait(lk, [&] { return !e.in.empty() || s->finishing || s->err != HG_OK; });
        e.t_up_idle += now_s() - tw;
        if (s->err != HG_OK) return false;
        if (e.in.empty()) break;  // finishing
        it = e.in.front();
        e.in.pop_front();
        idle_after = e.in.empty();
      }
      if (cur >= 0 && e.chunk[cur].lay.closes_before(it, limit) && !close_chunk()) return false;
      if (cur < 0) {
        const double tw = now_s();
        std::unique_lock<std::mutex> lk(s->mu);
        s->cv_chunk.wait(lk, [&] { return !e.free_chunks.empty() || s->err != HG_OK; });
        e.t_up_nochunk += now_s() - tw;
        if (s->err != HG_OK) return false;
        cur = e.free_chunks.front();
        e.free_chunks.pop_front();
        e.chunk[cur].lay = ChunkLayout{};
      }
      Chunk &c = e.chunk[cur];
      if (it.len && it.kind != KIND_ASCII && !c.h_jobs) {
        ST_HIP(s, hipHostMalloc(reinterpret_cast<void **>(&c.h_jobs), CHUNK_GENOMES * sizeof(UnpackJob), hipHostMallocDefault));
        ST_HIP(s, hipMalloc(reinterpret_cast<void **>(&c.d_jobs), CHUNK_GENOMES * sizeof(UnpackJob)));
        ST_HIP(s, hipHostMalloc(reinterpret_cast<void **>(&c.h_sjobs), CHUNK_GENOMES * sizeof(SparseJob), hipHostMallocDefault));
        ST_HIP(s, hipMalloc(reinterpret_cast<void **>(&c.d_sjobs), CHUNK_GENOMES * sizeof(SparseJob)));
      }
      const ChunkPlace pl = c.lay.add(it, c.h_jobs, c.h_sjobs);
      if (pl.text_need > c.cap && !regrow(s, e, c.d, c.cap, pl.text_want, 0)) return false;
      const double tc = now_s();
      if (pl.packed_need > c.pk_cap && !regrow(s, e, c.dpk, c.pk_cap, pl.packed_want, pl.packed_keep)) return false;
      if (pl.area == ChunkPlace::PACKED) {  // (the genomes' own copies alternate between the two queues)
        ST_HIP(s, hipMemcpyAsync(c.dpk + pl.off, it.seq, pl.n, hipMemcpyHostToDevice, (e.turn++ & 1u) ? e.copy2 : e.copy));
      } else if (pl.area == ChunkPlace::TEXT) {
        if (!flush_run(s, e, c)) return false;
        ST_HIP(s, hipMemcpyAsync(c.d + pl.off, it.seq, pl.n, hipMemcpyHostToDevice, (e.turn++ & 1u) ? e.copy2 : e.copy));
      } else if (pl.area == ChunkPlace::STAGE) {
        if (!c.stage) ST_HIP(s, hipHostMalloc(reinterpret_cast<void **>(&c.stage), CHUNK_BYTES, hipHostMallocDefault));
        std::memcpy(c.stage + pl.off, it.seq, pl.n);
        std::memset(c.stage + pl.off + pl.n, 0, it.padded() - pl.n);
      }
      e.t_up_copy += now_s() - tc;
      if (c.lay.closes_after(idle_after, limit) && !close_chunk()) return false;
    }
    return cur < 0 || hand_over(s, e, cur);
  };
  (void)body();
  std::lock_guard<std::mutex> lk(s->mu);
  e.uploader_done = true;
  s->cv_chunk.notify_all();
}

// the chunk's m result rows come back into h_res
bool read_back(hg_sketch_stream *s, Engine &e, size_t m) {
  const size_t hvb_al = (CHUNK_GENOMES * s->p.hv_d * sizeof(int16_t) + 63) & ~(size_t)63;
  ST_HIP(s, hipMemcpyAsync(e.h_res, e.d_hv, m * s->p.hv_d * sizeof(int16_t), hipMemcpyDeviceToHost, e.ctx->stream));
  ST_HIP(s, hipMemcpyAsync(e.h_res + hvb_al, e.d_n2, m * 4, hipMemcpyDeviceToHost, e.ctx->stream));
  ST_HIP(s, hipMemcpyAsync(e.h_res + hvb_al + CHUNK_GENOMES * 4, e.d_nh, m * 4, hipMemcpyDeviceToHost, e.ctx->stream));
  ST_HIP(s, hipStreamSynchronize(e.ctx->stream));
  return true;
}

void computer(hg_sketch_stream *s, Engine *ep) {
  Engine &e = *ep;
  auto ctx_failed = [&](hg_status st) { return fail(s, st, std::string("device ") + std::to_string(e.device) + ": " + hg_last_error(e.ctx)), false; };
  auto body = [&]() -> bool {
    ST_HIP(s, hipSetDevice(e.device));
    const size_t D = s->p.hv_d;
    for (;;) {
      int ci;
      const double tw = now_s();
      {
        std::unique_lock<std::mutex> lk(s->mu);
        s->cv_chunk.wait(lk, [&] { return !e.full_chunks.empty() || e.uploader_done || s->err != HG_OK; });
        e.t_comp_idle += now_s() - tw;
        if (s->err != HG_OK) return false;
        if (e.full_chunks.empty()) break;  // the uploader is done and so are we
        ci = e.full_chunks.front();
        e.full_chunks.pop_front();
      }
      Chunk &c = e.chunk[ci];
      const ChunkLayout &lay = c.lay;  // (the uploader does not touch it before the chunk is free again)
      const size_t m = lay.tags.size();
      const double tr = now_s();
      ST_HIP(s, hipStreamWaitEvent(e.ctx->stream, c.uploaded, 0));
      hg_status st;
      if (lay.n_sjobs)  // the bitmaps of the genomes that came as codes + run table
        ST_HIP(s, hg_launch_expand_runs(e.ctx->stream, c.dpk, c.d_sjobs, lay.n_sjobs, lay.n_sblocks));
      if (lay.packed_only()) {
        // (empty genomes of an otherwise packed chunk have no blob: offset 0, length 0 -- nothing is read for them)
        st = hg_sketch_batch_dev_packed_masks(e.ctx, c.dpk, lay.pk_offs.data(), lay.mask_offs.data(), lay.lens.data(), m, &s->p, e.d_hv, e.d_n2, e.d_nh);
      } else {
        if (lay.n_jobs) ST_HIP(s, hg_launch_unpack2_jobs(e.ctx->stream, c.dpk, c.d, c.d_jobs, lay.n_jobs, lay.n_blocks));
        st = hg_sketch_batch_dev(e.ctx, c.d, lay.offs.data(), lay.lens.data(), m, &s->p, e.d_hv, e.d_n2, e.d_nh);
      }
      if (st != HG_OK) return ctx_failed(st);
      if (!read_back(s, e, m)) return false;
      // the step's check word: a chunk with a genome that outgrew its hit region is sketched again (synchronous path),
      // and the rows copied above are fetched once more
      bool redone = false;
      if ((st = hg_sketch_resolve(e.ctx, &redone)) != HG_OK) return ctx_failed(st);
      if (redone && !read_back(s, e, m)) return false;
      const size_t hvb_al = (CHUNK_GENOMES * D * sizeof(int16_t) + 63) & ~(size_t)63;
      Done d;
      d.tags = lay.tags;
      d.hv.assign(reinterpret_cast<int16_t *>(e.h_res), reinterpret_cast<int16_t *>(e.h_res) + m * D);
      d.n2.assign(reinterpret_cast<int32_t *>(e.h_res + hvb_al), reinterpret_cast<int32_t *>(e.h_res + hvb_al) + m);
      d.nh.assign(reinterpret_cast<uint32_t *>(e.h_res + hvb_al + CHUNK_GENOMES * 4),
                  reinterpret_cast<uint32_t *>(e.h_res + hvb_al + CHUNK_GENOMES * 4) + m);
      std::lock_guard<std::mutex> lk(s->mu);
      e.t_comp_run += now_s() - tr, ++e.n_chunks;
      e.load -= std::min(e.load, lay.bytes);
      s->out.push_back(std::move(d));
      e.free_chunks.push_back(ci);
      s->cv_chunk.notify_all(), s->cv_out.notify_all();
    }
    return true;
  };
  (void)body();
  std::lock_guard<std::mutex> lk(s->mu);
  s->cv_out.notify_all();
}

void destroy(hg_sketch_stream *s) {
  {
    std::lock_guard<std::mutex> lk(s->mu);
    s->finishing = true;
    if (s->err == HG_OK && s->popped < s->pushed) s->err = HG_ERR_INVALID, s->msg = "stream closed with results outstanding";
    s->cv_in.notify_all(), s->cv_chunk.notify_all(), s->cv_out.notify_all(), s->cv_room.notify_all();
  }
  for (Engine *e : s->eng) {
    if (e->up.joinable()) e->up.join();
    if (e->comp.joinable()) e->comp.join();
    if (!e->ctx) {  // never opened (bad device id): nothing to release, and no HIP call that would leave an error behind
      delete e;
      continue;
    }
    (void)hipSetDevice(e->device);
    for (hipStream_t q : {e->copy, e->copy2}) if (q) (void)hipStreamSynchronize(q);
    for (Chunk &c : e->chunk) {
      for (void *p : {(void *)c.d, (void *)c.dpk, (void *)c.d_jobs, (void *)c.d_sjobs}) if (p) (void)hipFree(p);
      for (void *p : {(void *)c.stage, (void *)c.h_jobs, (void *)c.h_sjobs}) if (p) (void)hipHostFree(p);
      if (c.uploaded) (void)hipEventDestroy(c.uploaded);
    }
    if (e->d_hv) (void)hipFree(e->d_hv);
    if (e->h_res) (void)hipHostFree(e->h_res);
    for (hipStream_t q : {e->copy, e->copy2}) if (q) (void)hipStreamDestroy(q);
    if (e->copy2_done) (void)hipEventDestroy(e->copy2_done);
    hg_ctx_destroy(e->ctx);
    delete e;
  }
  delete s;
}

}  // namespace

extern "C" hg_status hg_sketch_stream_open(const int *device_ids, int n_devices, const hg_sketch_params *p,
                                           hg_sketch_stream **out) {
  if (!out) return HG_ERR_INVALID;
  *out = nullptr;
  if (!device_ids || n_devices <= 0 || !p) return hg_fail(nullptr, HG_ERR_INVALID, "hg_sketch_stream_open: bad arguments");
  if (p->hv_d == 0 || p->hv_d > 32768) return hg_fail(nullptr, HG_ERR_UNSUPPORTED, "hv_d must be in 1..32768");
  hg_sketch_stream *s = new (std::nothrow) hg_sketch_stream();
  if (!s) return HG_ERR_OOM;
  s->p = *p;
  const size_t hvb_al = (CHUNK_GENOMES * p->hv_d * sizeof(int16_t) + 63) & ~(size_t)63;
  for (int i = 0; i < n_devices; ++i) {
    Engine *e = new (std::nothrow) Engine();
    if (!e) {
      destroy(s);
      return HG_ERR_OOM;
    }
    s->eng.push_back(e);
    e->device = device_ids[i];
    hg_status st = hg_ctx_create(device_ids[i], &e->ctx);
    hipError_t he = hipSuccess;
    if (st == HG_OK) {
      if ((he = hipSetDevice(e->device)) == hipSuccess)
        he = hipStreamCreateWithFlags(&e->copy, hipStreamNonBlocking);
      if (he == hipSuccess) he = hipStreamCreateWithFlags(&e->copy2, hipStreamNonBlocking);
      if (he == hipSuccess) he = hipEventCreateWithFlags(&e->copy2_done, hipEventDisableTiming);
      for (int k = 0; k < N_CHUNKS && he == hipSuccess; ++k) {
        if ((he = hipMalloc(reinterpret_cast<void **>(&e->chunk[k].d), TEXT_AREA_MIN)) == hipSuccess)
          e->chunk[k].cap = TEXT_AREA_MIN, he = hipEventCreateWithFlags(&e->chunk[k].uploaded, hipEventDisableTiming);
        e->free_chunks.push_back(k);
      }
      void *dres = nullptr;
      if (he == hipSuccess && (he = hipMalloc(&dres, hvb_al + CHUNK_GENOMES * 8)) == hipSuccess) {
        e->d_hv = static_cast<int16_t *>(dres);
        e->d_n2 = reinterpret_cast<int32_t *>(static_cast<uint8_t *>(dres) + hvb_al);
        e->d_nh = reinterpret_cast<uint32_t *>(e->d_n2 + CHUNK_GENOMES);
        he = hipHostMalloc(reinterpret_cast<void **>(&e->h_res), hvb_al + CHUNK_GENOMES * 8, hipHostMallocDefault);
      }
    }
    if (st != HG_OK || he != hipSuccess) {
      const std::string m = st != HG_OK ? std::string(hg_last_error(nullptr)) : std::string("stream setup: ") + hipGetErrorString(he);
      destroy(s);
      return hg_fail(nullptr, st != HG_OK ? st : HG_ERR_HIP, m);
    }
  }
  for (Engine *e : s->eng) {
    e->up = std::thread(uploader, s, e);
    // one compute thread (one ctx) per device.  A/B at 2 (+ a 4th chunk): 7.3-7.8 k files/s instead of 8.3-9.6 k -- two
    // contexts' small kernels and synchronisations get in each other's way
    e->comp = std::thread(computer, s, e);
  }
  *out = s;
  return HG_OK;
}

static hg_status push_item(hg_sketch_stream *s, const uint8_t *seq, size_t len, uint64_t tag, int kind, bool wait, size_t given_bytes = ~(size_t)0) {
  if (!s || (len && !seq)) return HG_ERR_INVALID;
  size_t blob_bytes = 0;
  if (kind == KIND_PACK2S && len) {  // the blob says how long its run table is -- nothing of it is believed unchecked:
    // the count is read only if the caller's buffer reaches that far, the blob must fit the buffer, and the table has to be
    // what expand_runs_kernel's binary search assumes (ascending, disjoint, non-empty runs inside the sequence)
    if (len >= ((size_t)1 << 32)) return HG_ERR_UNSUPPORTED;
    const size_t tab_off = hg_pack2_code_bytes(len);
    if (given_bytes < tab_off + 8) return HG_ERR_INVALID;
    uint32_t n_runs;
    std::memcpy(&n_runs, seq + tab_off, 4);
    if ((size_t)n_runs > len) return HG_ERR_INVALID;
    blob_bytes = hg_pack2s_size(len, n_runs);
    if (blob_bytes > given_bytes) return HG_ERR_INVALID;
    uint64_t prev_end = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
      uint32_t st_len[2];
      std::memcpy(st_len, seq + tab_off + 8 + (size_t)8 * r, 8);
      if (st_len[1] == 0 || (r && st_len[0] < prev_end) || (uint64_t)st_len[0] + st_len[1] > len) return HG_ERR_INVALID;
      prev_end = (uint64_t)st_len[0] + st_len[1];
    }
  }
  std::unique_lock<std::mutex> lk(s->mu);
  if (s->finishing) return HG_ERR_INVALID;
  if (!wait && s->err == HG_OK && s->pushed - s->popped >= s->max_pending) return HG_ERR_CAPACITY;  // would block
  s->cv_room.wait(lk, [&] { return s->pushed - s->popped < s->max_pending || s->err != HG_OK; });
  if (s->err != HG_OK) return s->err;
  Engine *best = s->eng[0];
  for (Engine *e : s->eng)
    if (e->load < best->load) best = e;
  best->in.push_back(StreamItem{seq, len, tag, kind, blob_bytes});
  best->load += (len + 15) & ~(size_t)15;
  ++s->pushed;
  s->cv_in.notify_all();
  return HG_OK;
}

extern "C" hg_status hg_sketch_stream_push(hg_sketch_stream *s, const uint8_t *seq, size_t len, uint64_t tag) {
  return push_item(s, seq, len, tag, KIND_ASCII, true);
}

extern "C" hg_status hg_sketch_stream_push_packed(hg_sketch_stream *s, const uint8_t *blob, size_t n_bps, uint64_t tag) {
  return push_item(s, blob, n_bps, tag, KIND_PACK2, true);
}

extern "C" hg_status hg_sketch_stream_push_packed_sparse(hg_sketch_stream *s, const uint8_t *blob, size_t blob_bytes, size_t n_bps, uint64_t tag) {
  return push_item(s, blob, n_bps, tag, KIND_PACK2S, true, blob_bytes);
}

extern "C" hg_status hg_sketch_stream_try_push(hg_sketch_stream *s, const uint8_t *data, size_t n_bps, uint64_t tag, int packed) {
  if (packed < 0 || packed > 2) return HG_ERR_INVALID;
  return push_item(s, data, n_bps, tag, packed, false);
}

extern "C" size_t hg_sketch_stream_max_pending(const hg_sketch_stream *s) { return s ? s->max_pending : 0; }

extern "C" hg_status hg_sketch_stream_finish(hg_sketch_stream *s) {
  if (!s) return HG_ERR_INVALID;
  std::lock_guard<std::mutex> lk(s->mu);
  s->finishing = true;
  s->cv_in.notify_all(), s->cv_out.notify_all();
  return s->err;
}

extern "C" hg_status hg_sketch_stream_pop(hg_sketch_stream *s, uint64_t *tag, int16_t *hv_out, int32_t *norm2_out,
                                          uint32_t *nhash_out, int *got) {
  if (!s || !got) return HG_ERR_INVALID;
  *got = 0;
  std::unique_lock<std::mutex> lk(s->mu);
  s->cv_out.wait(lk, [&] { return !s->out.empty() || s->err != HG_OK || (s->finishing && s->popped == s->pushed); });
  if (s->out.empty()) return s->err;  // failed, or finished and drained (HG_OK, *got == 0)
  Done &d = s->out.front();
  const size_t k = d.next++, D = s->p.hv_d;
  if (tag) *tag = d.tags[k];
  if (hv_out) std::memcpy(hv_out, d.hv.data() + k * D, D * sizeof(int16_t));
  if (norm2_out) *norm2_out = d.n2[k];
  if (nhash_out) *nhash_out = d.nh[k];
  if (d.next == d.tags.size()) s->out.pop_front();
  ++s->popped;
  *got = 1;
  s->cv_room.notify_all();
  if (s->finishing && s->popped == s->pushed) s->cv_out.notify_all();
  return HG_OK;
}

extern "C" const char *hg_sketch_stream_last_error(hg_sketch_stream *s) {
  if (!s) return "";
  std::lock_guard<std::mutex> lk(s->mu);
  return s->msg.c_str();
}

extern "C" hg_status hg_sketch_stream_stats(hg_sketch_stream *s, int engine, double out[6]) {
  if (!s || !out || engine < 0 || engine >= (int)s->eng.size()) return HG_ERR_INVALID;
  std::lock_guard<std::mutex> lk(s->mu);
  const Engine &e = *s->eng[engine];
  out[0] = e.t_up_idle, out[1] = e.t_up_nochunk, out[2] = e.t_up_copy, out[3] = e.t_comp_idle, out[4] = e.t_comp_run;
  out[5] = (double)e.n_chunks;
  return HG_OK;
}

extern "C" void hg_sketch_stream_close(hg_sketch_stream *s) {
  if (s) destroy(s);
}
