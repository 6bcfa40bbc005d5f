// hg_api_sketch.hip -- the C ABI of include/hypergen.h, part 2: the sketch path -- batch plans, hash + sample -> sort / unique ->
// encode over the genomes of a batch (device-resident, host-fed with uploads and host-side 2-bit packing under them, one
// genome per call), page-locked read buffers.  What src/sketch.rs:35-56 and src/sketch_cuda.rs:79-166 do per file.
// The host-fed batch reads top to bottom in hg_sketch_batch: decide and lay out (hg_hostfed_layout.h, arithmetic only), then an
// uploader with one function per upload route, a consumer and a closing read-back, the two threads joined by a Handover (hg_host.h).
#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <sched.h>
#include <string>
#include <thread>
#include <vector>

#include "hg_host.h"
#include "hg_hostfed_layout.h"

#include "hg_sketch.h"

static hg_status sketch_batch_dev_impl(hg_ctx *c, const uint8_t *d_seq, const uint64_t *offsets, const uint64_t *lens, size_t n,
                                       const hg_sketch_params *p, int16_t *d_hv, int32_t *d_norm2, uint32_t *d_nhash, bool packed,
                                       const uint64_t *mask_offs = nullptr) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_check_sketch_params(c, p);
  if (s != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!d_seq || !offsets || !lens || !d_hv || !d_norm2 || !d_nhash) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (n > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "more than 2^31 genomes in one batch");
  HG_HIP(c, hipSetDevice(c->device));  // (no HG_ENTER: hg_sketch_step reads the previous step's check word behind its own launches)
  hg_genome_batch b{d_seq, offsets, lens, mask_offs, n, packed};
  const hg_sketch_out out{d_hv, d_norm2, d_nhash};
  if (!packed && c->dbg_kmer_input == "packed") {
    // test hook: the batch arrived as ASCII -- pack it here and run the packed kernels on the blobs, so that every
    // ASCII entry point (and with it every parity test) can be driven through both input forms
    if ((s = hg_sketch_resolve(c)) != HG_OK) return s;
    std::vector<uint64_t> hook_offs(n);
    uint64_t total = 0;
    for (size_t g = 0; g < n; ++g) hook_offs[g] = total, total += hg_pack2_size(lens[g]);
    if ((s = hg_ensure(c, c->w_pk, total + 64)) != HG_OK) return s;
    if ((s = hg_pack_batch(c, d_seq, offsets, lens, n, p->norm_mode, static_cast<uint8_t *>(c->w_pk.p), hook_offs.data())) != HG_OK) return s;
    b.d_seq = static_cast<const uint8_t *>(c->w_pk.p), b.offsets = hook_offs.data(), b.packed = true;
    return hg_sketch_step(c, b, p, out);
  }
  return hg_sketch_step(c, b, p, out);
}

hg_status hg_sketch_batch_dev_packed_masks(hg_ctx *c, const uint8_t *d_blobs, const uint64_t *code_offs, const uint64_t *mask_offs,
                                           const uint64_t *n_bps, size_t n, const hg_sketch_params *p, int16_t *d_hv,
                                           int32_t *d_norm2, uint32_t *d_nhash) {
  return sketch_batch_dev_impl(c, d_blobs, code_offs, n_bps, n, p, d_hv, d_norm2, d_nhash, true, mask_offs);
}

extern "C" hg_status hg_sketch_batch_dev(hg_ctx *c, const uint8_t *d_seq, const uint64_t *offsets,
                                         const uint64_t *lens, size_t n, const hg_sketch_params *p,
                                         int16_t *d_hv, int32_t *d_norm2, uint32_t *d_nhash) {
  return sketch_batch_dev_impl(c, d_seq, offsets, lens, n, p, d_hv, d_norm2, d_nhash, false);
}

extern "C" hg_status hg_sketch_batch_dev_packed(hg_ctx *c, const uint8_t *d_blobs, const uint64_t *offsets,
                                                const uint64_t *n_bps, size_t n, const hg_sketch_params *p,
                                                int16_t *d_hv, int32_t *d_norm2, uint32_t *d_nhash) {
  if (c && offsets)
    for (size_t g = 0; g < n; ++g)
      if (offsets[g] & 15) return hg_fail(c, HG_ERR_INVALID, "blob offsets must be multiples of 16");
  return sketch_batch_dev_impl(c, d_blobs, offsets, n_bps, n, p, d_hv, d_norm2, d_nhash, true);
}

extern "C" hg_status hg_pack2_batch_dev(hg_ctx *c, const uint8_t *d_seq, const uint64_t *offsets, const uint64_t *lens, size_t n,
                                        uint32_t norm_mode, uint8_t *d_blobs, const uint64_t *blob_offsets) {
  if (!c) return HG_ERR_INVALID;
  if (n == 0) return HG_OK;
  if (!d_seq || !offsets || !lens || !d_blobs || !blob_offsets || norm_mode > HG_NORM_U2T) return hg_fail(c, HG_ERR_INVALID, "bad argument");
  if (n > 0x7FFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "more than 2^31 genomes in one batch");
  HG_ENTER(c);
  return hg_pack_batch(c, d_seq, offsets, lens, n, norm_mode, d_blobs, blob_offsets);
}

extern "C" hg_status hg_pack2_dev(hg_ctx *c, const uint8_t *d_seq, size_t n_bps, uint32_t norm_mode, uint8_t *d_blob) {
  if (!c) return HG_ERR_INVALID;
  if (((uintptr_t)d_seq & 3) || ((uintptr_t)d_blob & 15)) return hg_fail(c, HG_ERR_INVALID, "hg_pack2_dev: d_seq must be 4-byte, d_blob 16-byte aligned");
  const uint64_t zero = 0, len = n_bps;
  return hg_pack2_batch_dev(c, d_seq, &zero, &len, 1, norm_mode, d_blob, &zero);
}

// NUMA node the device hangs off (sysfs of its PCI function), -1 when unknown.  Page-locked buffers filled by
// threads of that node are fetched ~25 % faster than buffers on the other socket (2-socket EPYC host, measured).
extern "C" int hg_device_numa_node(int device_id) {
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device_id) != hipSuccess) return -1;
  for (char *q = bus; *q; ++q) *q = (char)std::tolower((unsigned char)*q);
  const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
  FILE *f = std::fopen(path.c_str(), "r");
  if (!f) return -1;
  int node = -1;
  if (std::fscanf(f, "%d", &node) != 1) node = -1;
  std::fclose(f);
  return node;
}

// ---- page-locked read buffers -----------------------------------------------------------------------------------
// A pageable hipMemcpyAsync goes through the runtime's bounce buffer and blocks its caller; sequence read straight
// into page-locked memory is DMA'd by hg_sketch_batch at the link rate instead.
namespace {
bool grow_pinned(uint8_t *&buf, size_t &cap, size_t need, size_t keep, void *) {
  if (need <= cap) return true;
  // recycled slots see files of similar but not equal sizes: round up so that they rarely move
  const size_t want = ((need + need / 8) + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
  void *nb = nullptr;
  if (hipHostMalloc(&nb, want, hipHostMallocPortable) != hipSuccess || !nb) return false;
  if (buf && keep) std::memcpy(nb, buf, std::min(keep, cap));
  if (buf) (void)hipHostFree(buf);
  buf = static_cast<uint8_t *>(nb), cap = want;
  return true;
}
}  // namespace

extern "C" hg_status hg_read_fastx_pinned(const char *path, uint32_t mode, uint8_t **buf, size_t *cap, size_t *n_bps) {
  return hg_read_fastx_impl(path, mode, buf, cap, n_bps, grow_pinned, nullptr);
}

extern "C" void hg_pinned_free(void *p) {
  if (p) (void)hipHostFree(p);
}

// Host threads the library may use for its own host-side work on a call (2-bit packing of a host-fed batch): the cores
// this process may run on, at most 16 -- the reference's default `-t` (src/utils.rs:54-56).
static unsigned host_threads() {
  unsigned n = std::thread::hardware_concurrency();
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::min<unsigned>(n ? n : 1u, (unsigned)CPU_COUNT(&set));
  return std::max(1u, std::min(n, 16u));
}

// Host-fed calls in flight in this process (hg_sketch_batch / hg_kmer_hash_sample, any context): the reference's pattern is
// one call per genome from a pool of host threads (src/sketch_cuda.rs:79-96), and then the calls share ONE link.
static std::atomic<int> g_hostfed_calls{0};
namespace {
struct HostfedCall {
  int others;
  HostfedCall() : others(g_hostfed_calls.fetch_add(1)) {}
  ~HostfedCall() { g_hostfed_calls.fetch_sub(1); }
};
}  // namespace
static bool host_pinned(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // (an ordinary malloc'ed pointer is "invalid value" to the runtime)
    return false;
  }
  return a.type == hipMemoryTypeHost;
}
// Whether ONE genome handed over by a host-fed call goes over the link 2-bit packed (by the calling thread into the
// context's page-locked staging buffer) instead of as ASCII.
//  * pageable source (>= 256 KB): packed -- the runtime would stage it through its own pinned buffers anyway;
//  * page-locked source, fewer than 3 other host-fed calls in flight: ASCII (a lone 5 Mbp call takes 0.18 ms as ASCII,
//    0.33 ms packed);
//  * page-locked source, the link shared by K >= 4 calls (the reference's one-call-per-genome pattern from a thread
//    pool): packed as long as the host keeps up.  With K calls sharing a link of L bytes/s a call waits n K / L for its
//    ASCII, or n / r + 0.375 n K / L packed at r bytes/s: packing pays while r > L / (0.625 K).  r is what the calling
//    threads really achieve TOGETHER (16 of them are bound by host DRAM: 7 GB/s each on a quiet box of the pool -- 17 k
//    genomes/s against 10 k --, 4 GB/s on one whose memory was busy -- 8.6 k against 10 k), so it is measured in the
//    packed calls themselves (decayed mean, kept per range of K: r falls as K grows); when it falls short, the next calls
//    of that range go as ASCII -- 256 of them, doubling each time packing fails again, up to 16 384 -- and then packing is
//    tried afresh.
// Hook: "hostfed" = "ascii" never, "packed" always.
namespace {
constexpr double HG_LINK_BYTES_PER_S = 50e9;  // what ASCII uploads from page-locked memory reach on Gen5 x16 (bench.py host_fed.ascii_link)
struct PackState {
  std::atomic<uint64_t> rate{0};       // decayed mean of the bytes/s one calling thread packed at, contended packed calls
  std::atomic<uint32_t> samples{0};    // ... and how many calls it has seen since packing was (re)started
  std::atomic<int32_t> ascii_left{0};  // > 0: contended calls still to go as ASCII before packing is tried again
  std::atomic<uint32_t> backoff{256};
};
PackState g_pack[6];  // by calls in flight: 4-5, 6-7, 8-11, 12-15, 16-23, 24 and more
inline PackState &pack_state(int sharing) {
  return g_pack[sharing < 6 ? 0 : sharing < 8 ? 1 : sharing < 12 ? 2 : sharing < 16 ? 3 : sharing < 24 ? 4 : 5];
}
struct SingleChoice {
  bool packed = false, measured = false;
  int sharing = 1;  // calls in flight, this one included
};
// after a measured call packed its genome: n bytes in sec seconds
void pack_measured(const SingleChoice &ch, uint64_t n, double sec) {
  if (!ch.measured || sec <= 0) return;
  PackState &st = pack_state(ch.sharing);
  const uint64_t rate = (uint64_t)((double)n / sec), old = st.rate.load(std::memory_order_relaxed);
  const uint64_t now = old ? old - old / 8 + rate / 8 : rate;  // (racing updates lose a sample at worst)
  st.rate.store(now, std::memory_order_relaxed);
  const uint32_t seen = st.samples.fetch_add(1, std::memory_order_relaxed) + 1;
  if (seen >= 8 && (double)now * 0.625 * ch.sharing < 0.9 * HG_LINK_BYTES_PER_S) {
    const uint32_t b = st.backoff.load(std::memory_order_relaxed);
    st.ascii_left.store((int32_t)b, std::memory_order_relaxed);
    st.backoff.store(std::min<uint32_t>(2 * b, 16384u), std::memory_order_relaxed);
    st.samples.store(0, std::memory_order_relaxed), st.rate.store(0, std::memory_order_relaxed);
  } else if (seen == 1024) {
    st.backoff.store(256, std::memory_order_relaxed);  // (a long run of packing that paid)
  }
}
}  // namespace
static SingleChoice pack_single(const hg_ctx *c, const void *seq, uint64_t n_bps, int others) {
  SingleChoice r;
  r.sharing = others + 1;
  if (c->dbg_hostfed == "ascii" || hg_pack2_size(n_bps) > HG_PACK_BYTES) return r;
  r.packed = true;
  if (c->dbg_hostfed == "packed") return r;
  r.packed = false;
  if (n_bps < (256u << 10)) return r;
  if (!host_pinned(seq)) {
    r.packed = true;
    return r;
  }
  if (others < 3) return r;
  PackState &st = pack_state(r.sharing);
  if (st.ascii_left.load(std::memory_order_relaxed) > 0) {
    st.ascii_left.fetch_sub(1, std::memory_order_relaxed);
    return r;
  }
  r.packed = r.measured = true;
  return r;
}

// Page-locked staging buffer b of the context with room for `need` bytes, free to be rewritten (the upload that last read
// it has passed).  Sized by need -- locking pages costs ~0.25 ms per MB, and a pool of one-call-per-genome contexts
// should not pin 66 MB each for 2 MB blobs.
static hipError_t pack_buf_for(hg_ctx *c, int b, size_t need) {
  hipError_t e = hipSuccess;
  if (c->pack_used[b]) e = hipEventSynchronize(c->pack_ev[b]);
  if (e != hipSuccess) return e;
  if (!c->pack_ev[b] && (e = hipEventCreateWithFlags(&c->pack_ev[b], hipEventDisableTiming)) != hipSuccess) return e;
  if (c->pack_cap[b] >= need) return hipSuccess;
  if (c->pack_buf[b]) (void)hipHostFree(c->pack_buf[b]);
  c->pack_buf[b] = nullptr, c->pack_cap[b] = 0, c->pack_used[b] = false;
  const size_t want = (need + need / 4 + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
  if ((e = hipHostMalloc(&c->pack_buf[b], want, hipHostMallocDefault)) != hipSuccess) return e;
  c->pack_cap[b] = want;
  return hipSuccess;
}

// One genome, 2-bit packed by the calling thread into staging buffer 0 (the whole genome as one piece, timed for
// pack_single()'s sake) and queued for d_dst on `stream`: hg_kmer_hash_sample and the n = 1 of hg_sketch_batch.
static hipError_t upload_one_packed(hg_ctx *c, const SingleChoice &single, const uint8_t *seq, uint64_t n_bps, uint32_t norm_mode,
                                    void *d_dst, hipStream_t stream) {
  const size_t bytes = hg_pack2_size(n_bps);
  hipError_t e = pack_buf_for(c, 0, bytes);
  if (e != hipSuccess) return e;
  const auto t0 = std::chrono::steady_clock::now();
  hg_pack2_piece(seq, n_bps, norm_mode, static_cast<uint8_t *>(c->pack_buf[0]), 0, n_bps);
  pack_measured(single, n_bps, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  if ((e = hipMemcpyAsync(d_dst, c->pack_buf[0], bytes, hipMemcpyHostToDevice, stream)) == hipSuccess) e = hipEventRecord(c->pack_ev[0], stream);
  c->pack_used[0] = true;
  return e;
}

// ---- host-fed batch -------------------------------------------------------------------------------------------------
// The batch is cut into sub-batches of about HG_STAGE_BYTES (hg_hostfed_layout.h: the decision to pack, the layout, the
// upload routes and the packing tasks, as arithmetic); a helper thread queues their uploads on the context's copy stream
// (one event per sub-batch) while the calling thread runs hash/sort/encode of the sub-batches already on the device, so PCIe
// transfer and kernels overlap for pinned and for pageable caller memory alike (a pageable hipMemcpyAsync blocks the thread
// that issues it).
namespace {
struct HostfedDev {  // the device side of a call
  uint8_t *seq;
  int16_t *hv;
  int32_t *n2;
  uint32_t *nh;
  size_t hv_bytes;
  hipStream_t up_stream;  // one sub-batch (the n = 1 of a one-call-per-genome pool above all): its upload goes on the context's
  bool one_stream;        // own stream, in front of its kernels -- no second stream, no event to wait for
};

// What the uploader reads.  It writes (1) lay->subs[j].packed of the sub-batches j behind the first, while it works on the
// first: the consumer reads subs[j] after done->wait(j) has returned; (2) the context's staging buffers (pack_buf, pack_cap,
// pack_ev, pack_used), which the calling thread touches again only after it has joined the uploader.
struct HostfedUpload {
  hg_ctx *c;
  const uint8_t *const *seqs;
  HostfedLayout *lay;
  HostfedDev dev;
  CallPool *pool;         // packed route (nullptr: `single` packs)
  uint32_t norm_mode;
  SingleChoice single;    // n = 1, packed by pack_single()'s choice
  bool src_pinned;
  int pack_node;          // NUMA node the pool's threads run on
  unsigned threads;
  Handover *done;
};

// 2-bit pack the sub-batch into page-locked staging (all host threads of the call), then ONE upload
hipError_t upload_packed(const HostfedUpload &u, size_t k) {
  hg_ctx *c = u.c;
  HostfedLayout &lay = *u.lay;
  const HostfedSub sub = lay.subs[k];
  const size_t n = lay.lens.size();
  if (u.single.packed) return upload_one_packed(c, u.single, u.seqs[0], lay.lens[0], u.norm_mode, u.dev.seq, u.dev.up_stream);
  const int b = (int)(k & 1);
  hipError_t e = pack_buf_for(c, b, n == 1 ? sub.pk_bytes : HG_PACK_BYTES);
  if (e != hipSuccess) return e;
  auto *pin = static_cast<uint8_t *>(c->pack_buf[b]);
  const HostfedPackWork w = lay.pack_work(k);
  const auto t0 = std::chrono::steady_clock::now();
  u.pool->run(w.tasks(), [&](size_t t) {
    for (size_t i = w.task_first[t]; i < w.task_first[t + 1]; ++i) {
      const HostfedPackWork::Piece &pc = w.pieces[i];
      hg_pack2_piece(u.seqs[pc.g], lay.lens[pc.g], u.norm_mode, pin + (lay.boffs[pc.g] - lay.boffs[sub.g0]), pc.b0, pc.b1);
    }
  });
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  // Packing has to outrun the link to be worth it: the first packed sub-batch is timed, and the rest goes as ASCII when the
  // host is too slow.  (Page-locked sources go at ~55 GB/s as ASCII; pageable ones through the runtime's bounce buffer at
  // ~12 GB/s: a host whose cores are capped by a cgroup quota -- host_threads() cannot see one -- may pack slower than even that)
  if (k == 0 && (double)sub.span < (u.src_pinned ? 55e9 : 12e9) * sec && c->dbg_hostfed != "packed") lay.demote_after(k);
  if ((e = hipMemcpyAsync(u.dev.seq + lay.boffs[sub.g0], pin, sub.pk_bytes, hipMemcpyHostToDevice, u.dev.up_stream)) == hipSuccess)
    e = hipEventRecord(c->pack_ev[b], u.dev.up_stream);
  c->pack_used[b] = true;
  return e;
}

// many small genomes: into page-locked staging in the device layout, then ONE upload
hipError_t upload_staged(const HostfedUpload &u, size_t k) {
  hg_ctx *c = u.c;
  const HostfedLayout &lay = *u.lay;
  const HostfedSub &sub = lay.subs[k];
  const int b = (int)(k & 1);
  hipError_t e = pack_buf_for(c, b, HG_PACK_BYTES);
  if (e != hipSuccess) return e;
  auto *pin = static_cast<uint8_t *>(c->pack_buf[b]);
  for (size_t g = sub.g0; g < sub.g1; ++g)
    if (lay.lens[g]) std::memcpy(pin + (lay.offs[g] - lay.offs[sub.g0]), u.seqs[g], lay.lens[g]);
  if ((e = hipMemcpyAsync(u.dev.seq + lay.offs[sub.g0], pin, sub.span, hipMemcpyHostToDevice, u.dev.up_stream)) == hipSuccess)
    e = hipEventRecord(c->pack_ev[b], u.dev.up_stream);
  c->pack_used[b] = true;
  return e;
}

// one copy per genome, from where the caller has it
hipError_t upload_direct(const HostfedUpload &u, size_t k) {
  const HostfedLayout &lay = *u.lay;
  hipError_t e = hipSuccess;
  for (size_t g = lay.subs[k].g0; g < lay.subs[k].g1 && e == hipSuccess; ++g)
    if (lay.lens[g]) e = hipMemcpyAsync(u.dev.seq + lay.offs[g], u.seqs[g], lay.lens[g], hipMemcpyHostToDevice, u.dev.up_stream);
  return e;
}

// The uploader: queues every sub-batch's upload (and its event) and publishes it; on an error it releases the consumer, which
// then reports it.  Runs on a thread of its own when there is more than one sub-batch.
void hostfed_upload(const HostfedUpload &u) {
  const size_t n_subs = u.lay->subs.size();
  hipError_t e = hipSetDevice(u.c->device);
  if (n_subs > 1) (void)hg_bind_thread_to_numa_node(u.pack_node, u.threads);  // (the helper thread only, never the caller's)
  for (size_t k = 0; k < n_subs && e == hipSuccess; ++k) {
    switch (u.lay->route(k)) {
      case HostfedRoute::PACKED: e = upload_packed(u, k); break;
      case HostfedRoute::STAGED: e = upload_staged(u, k); break;
      case HostfedRoute::DIRECT: e = upload_direct(u, k); break;
    }
    if (e == hipSuccess && !u.dev.one_stream) e = hipEventRecord(u.c->copy_events[k], u.dev.up_stream);
    if (e == hipSuccess) u.done->publish(k + 1);
  }
  if (e != hipSuccess) u.done->fail((int)e);
}

// device buffers for sequence and results; more than one sub-batch: the copy stream and an event per sub-batch
hg_status hostfed_ensure(hg_ctx *c, const HostfedLayout &lay, const hg_sketch_params *p, HostfedDev &dev) {
  const size_t n = lay.lens.size(), n_subs = lay.subs.size();
  hg_status s;
  dev.hv_bytes = n * (size_t)p->hv_d * sizeof(int16_t);
  if ((s = hg_ensure(c, c->w_seq, lay.total + 64)) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_hv, dev.hv_bytes + n * 8 + 64)) != HG_OK) return s;
  dev.seq = static_cast<uint8_t *>(c->w_seq.p);
  dev.hv = static_cast<int16_t *>(c->w_hv.p);
  dev.n2 = reinterpret_cast<int32_t *>(static_cast<uint8_t *>(c->w_hv.p) + ((dev.hv_bytes + 15) & ~(size_t)15));
  dev.nh = reinterpret_cast<uint32_t *>(dev.n2 + n);
  dev.one_stream = n_subs == 1;
  if (!dev.one_stream && !c->copy_stream) HG_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  dev.up_stream = dev.one_stream ? c->stream : c->copy_stream;
  while (!dev.one_stream && c->copy_events.size() < n_subs) {
    hipEvent_t e;
    HG_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->copy_events.push_back(e);
  }
  return HG_OK;
}

// The pool's threads run on the NUMA node the sequences lie on (page-locked memory from the HIP runtime: the device's node,
// like the staging buffers they write; packing from the other socket is ~1.5x slower), the uploader thread too.
int hostfed_pack_node(const hg_ctx *c, const uint8_t *const *seqs, const size_t *lens, size_t n) {
  for (size_t g = 0; g < n; ++g)
    if (lens[g]) {
      const int node = hg_numa_node_of(seqs[g]);
      if (node >= 0) return node;
    }
  return hg_device_numa_node(c->device);
}

// The consumer: sketches every sub-batch as its upload is queued and queues the copy of its HVs back
hg_status hostfed_consume(hg_ctx *c, const HostfedLayout &lay, const HostfedDev &dev, Handover &done, const hg_sketch_params *p,
                          int16_t *hv_out) {
  hg_status s = HG_OK;
  for (size_t k = 0; k < lay.subs.size() && s == HG_OK; ++k) {
    const int err = done.wait(k);
    if (err) return hg_fail(c, HG_ERR_HIP, std::string("sequence upload: ") + hipGetErrorString((hipError_t)err));
    const HostfedSub &sub = lay.subs[k];
    const size_t g0 = sub.g0, m = sub.g1 - g0, row = (size_t)p->hv_d;
    hipError_t e = dev.one_stream ? hipSuccess : hipStreamWaitEvent(c->stream, c->copy_events[k], 0);
    if (e != hipSuccess) return hg_fail(c, HG_ERR_HIP, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e));
    if (sub.packed)
      s = hg_sketch_batch_dev_packed(c, dev.seq, lay.boffs.data() + g0, lay.lens.data() + g0, m, p, dev.hv + g0 * row, dev.n2 + g0, dev.nh + g0);
    else
      s = hg_sketch_batch_dev(c, dev.seq, lay.offs.data() + g0, lay.lens.data() + g0, m, p, dev.hv + g0 * row, dev.n2 + g0, dev.nh + g0);
    if (s != HG_OK) return s;
    e = hipMemcpyAsync(hv_out + g0 * row, dev.hv + g0 * row, m * row * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) s = hg_fail(c, HG_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
  }
  return s;
}

// Closes the call: the last sub-batch's check word (the earlier ones were read as their successors were queued), all HVs
// again when a step was redone (it leaves stale rows in the copies queued behind it), norms and counts.
hg_status hostfed_finish(hg_ctx *c, const HostfedDev &dev, size_t n, uint64_t redone_before, int16_t *hv_out, int32_t *norm2_out,
                         uint32_t *nhash_out) {
  const hg_status s = hg_sketch_resolve(c);
  if (s != HG_OK) return s;
  if (c->n_redone_steps != redone_before) HG_HIP(c, hipMemcpyAsync(hv_out, dev.hv, dev.hv_bytes, hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(norm2_out, dev.n2, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(nhash_out, dev.nh, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}
}  // namespace

extern "C" hg_status hg_sketch_batch(hg_ctx *c, const uint8_t *const *seqs, const size_t *lens, size_t n,
                                     const hg_sketch_params *p, int16_t *hv_out, int32_t *norm2_out,
                                     uint32_t *nhash_out) {
  if (!c) return HG_ERR_INVALID;
  hg_status s = hg_check_sketch_params(c, p);
  if (s != HG_OK) return s;
  if (n == 0) return HG_OK;
  if (!seqs || !lens || !hv_out || !norm2_out || !nhash_out) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  uint64_t all_bytes = 0;
  for (size_t g = 0; g < n; ++g) {
    if (lens[g] && !seqs[g]) return hg_fail(c, HG_ERR_INVALID, "NULL sequence");
    all_bytes += lens[g];
  }
  // decide: packed or ASCII, with how many threads.  A call that hands over little (the n = 1 of the one-call-per-genome
  // pattern) packs on its own thread, when pack_single() says the link is contended.
  HostfedCall in_flight;
  const HostfedHook hook = c->dbg_hostfed == "ascii" ? HOSTFED_ASCII : c->dbg_hostfed == "packed" ? HOSTFED_PACKED : HOSTFED_AUTO;
  HostfedDecision d = hostfed_decide(host_threads(), all_bytes, n, in_flight.others, hook);
  SingleChoice single;
  if (!d.want_pack && n == 1 && (single = pack_single(c, seqs[0], lens[0], in_flight.others)).packed) d = {true, 1};
  HostfedLayout lay(lens, n, d.want_pack, hostfed_stage_bytes(d.want_pack, c->dbg_hostfed_stage_bytes), HG_PACK_BYTES);
  HostfedDev dev;
  if ((s = hostfed_ensure(c, lay, p, dev)) != HG_OK) return s;
  const int pack_node = d.want_pack && d.threads > 1 ? hostfed_pack_node(c, seqs, lens, n) : -1;
  std::unique_ptr<CallPool> pool;
  if (d.want_pack && !single.packed) pool.reset(new CallPool(d.threads, pack_node));  // (takes the threads it can get)
  const bool src_pinned = d.want_pack && n > 1 && host_pinned(seqs[0]);
  const uint64_t redone_before = c->n_redone_steps;
  Handover done;
  const HostfedUpload up{c, seqs, &lay, dev, pool.get(), p->norm_mode, single, src_pinned, pack_node, d.threads, &done};
  std::thread uploader;
  if (lay.subs.size() > 1) uploader = std::thread(hostfed_upload, std::cref(up));
  else hostfed_upload(up);
  s = hostfed_consume(c, lay, dev, done, p, hv_out);
  if (uploader.joinable()) uploader.join();
  if (!dev.one_stream) (void)hipStreamSynchronize(c->copy_stream);
  if (s != HG_OK) {
    (void)hipStreamSynchronize(c->stream);
    return s;
  }
  return hostfed_finish(c, dev, n, redone_before, hv_out, norm2_out, nhash_out);
}

extern "C" hg_status hg_kmer_hash_sample(hg_ctx *c, const uint8_t *seq, size_t n_bps, uint32_t ksize,
                                         uint64_t threshold, uint64_t seed, int canonical, uint32_t norm_mode,
                                         uint64_t *out_hashes, size_t cap, size_t *n_out) {
  return hg_kmer_hash_sample_min_count(c, seq, n_bps, ksize, threshold, seed, canonical, norm_mode, 1, out_hashes, cap, n_out);
}

extern "C" hg_status hg_kmer_hash_sample_min_count(hg_ctx *c, const uint8_t *seq, size_t n_bps, uint32_t ksize,
                                                   uint64_t threshold, uint64_t seed, int canonical, uint32_t norm_mode,
                                                   uint32_t min_count, uint64_t *out_hashes, size_t cap, size_t *n_out) {
  if (!c) return HG_ERR_INVALID;
  if (!n_out) return hg_fail(c, HG_ERR_INVALID, "n_out == NULL");
  *n_out = 0;
  if (ksize < 1) return hg_fail(c, HG_ERR_INVALID, "ksize must be >= 1");
  if (ksize > 255) return hg_fail(c, HG_ERR_UNSUPPORTED, "ksize must be <= 255 (the reference's -k is u8)");
  if (norm_mode > HG_NORM_U2T) return hg_fail(c, HG_ERR_INVALID, "bad norm mode");
  if (n_bps && !seq) return hg_fail(c, HG_ERR_INVALID, "NULL sequence");
  if (n_bps < ksize) return HG_OK;
  HG_ENTER(c);
  const std::vector<uint64_t> offs{0}, l64{n_bps};
  hg_status s = hg_ensure(c, c->w_seq, n_bps + 64);
  if (s != HG_OK) return s;
  // over the link as ASCII, or 2-bit packed by this thread when the link is shared with other calls (pack_single())
  HostfedCall in_flight;
  const SingleChoice single = pack_single(c, seq, n_bps, in_flight.others);
  const bool packed = single.packed;
  if (packed) HG_HIP(c, upload_one_packed(c, single, seq, n_bps, norm_mode, c->w_seq.p, c->stream));
  else HG_HIP(c, hipMemcpyAsync(c->w_seq.p, seq, n_bps, hipMemcpyHostToDevice, c->stream));
  // capacity heuristic wants "scaled"; derive it from the threshold (threshold = MAX / scaled)
  uint64_t scaled = threshold ? UINT64_MAX / threshold : UINT64_MAX;
  if (scaled < 1) scaled = 1;
  const hg_genome_batch b{static_cast<uint8_t *>(c->w_seq.p), offs.data(), l64.data(), nullptr, 1, packed};
  const hg_sketch_params p{ksize, canonical != 0, scaled, seed, 0, 0, norm_mode, min_count};  // (no encode)
  hg_batch_tables pl;
  uint32_t *d_nd = nullptr;
  hg_sample_fetch fetch;
  fetch.max_hashes = out_hashes ? cap : 0;
  s = hg_sample_batch_sync(c, b, &p, threshold, pl, false, &d_nd, &fetch);
  if (s != HG_OK) return s;
  if (fetch.valid) {  // count and hashes came back with sample_batch's own synchronisation
    *n_out = fetch.nd;
    if (fetch.nd) std::memcpy(out_hashes, fetch.h_hashes, fetch.nd * sizeof(uint64_t));
    return HG_OK;
  }
  uint32_t nd = 0;
  HG_HIP(c, hipMemcpyAsync(&nd, d_nd, sizeof nd, hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  *n_out = nd;
  if (nd > cap) return hg_fail(c, HG_ERR_CAPACITY, "out_hashes too small");
  if (nd) {
    if (!out_hashes) return hg_fail(c, HG_ERR_INVALID, "out_hashes == NULL");
    HG_HIP(c, hipMemcpyAsync(out_hashes, static_cast<uint64_t *>(c->w_hits.p) + pl.meta[0].hit_off,
                             nd * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HG_HIP(c, hipStreamSynchronize(c->stream));
  }
  return HG_OK;
}

extern "C" hg_status hg_hv_encode(hg_ctx *c, const uint64_t *hashes, size_t n, uint32_t hv_d, uint32_t hv_layout,
                                  int16_t *hv_out, int32_t *norm2_out) {
  if (!c) return HG_ERR_INVALID;
  if (hv_d == 0 || hv_d > 32768) return hg_fail(c, HG_ERR_UNSUPPORTED, "hv_d must be in 1..32768");
  if (hv_layout > HG_LAYOUT_AVX2) return hg_fail(c, HG_ERR_INVALID, "bad layout");
  if ((n && !hashes) || !hv_out || !norm2_out) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (n > 0xFFFFFFF0ull) return hg_fail(c, HG_ERR_UNSUPPORTED, "too many hashes");
  HG_ENTER(c);
  hg_status s;
  if ((s = hg_ensure(c, c->w_gmeta, sizeof(hg_genome_meta))) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_hits, (n + 1) * sizeof(uint64_t))) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_cnt, 2 * sizeof(uint32_t))) != HG_OK) return s;
  if ((s = hg_ensure(c, c->w_hv, (size_t)hv_d * sizeof(int16_t) + 64)) != HG_OK) return s;
  c->plan.reset();  // w_gmeta is about to be overwritten
  hg_genome_meta m{};
  m.hit_off = 0, m.hit_cap = (uint32_t)n;
  const uint32_t nd = (uint32_t)n;
  auto *d_hv = static_cast<int16_t *>(c->w_hv.p);
  auto *d_n2 = reinterpret_cast<int32_t *>(static_cast<uint8_t *>(c->w_hv.p) + (((size_t)hv_d * 2 + 15) & ~(size_t)15));
  HG_HIP(c, hipMemcpyAsync(c->w_gmeta.p, &m, sizeof m, hipMemcpyHostToDevice, c->stream));
  HG_HIP(c, hipMemcpyAsync(c->w_cnt.p, &nd, sizeof nd, hipMemcpyHostToDevice, c->stream));
  if (n) HG_HIP(c, hipMemcpyAsync(c->w_hits.p, hashes, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  c->last_kernel[HG_T_ENCODE].clear();
  HG_HIP(c, hg_launch_encode(c->stream, static_cast<hg_genome_meta *>(c->w_gmeta.p), 1,
                             static_cast<uint64_t *>(c->w_hits.p), static_cast<uint32_t *>(c->w_cnt.p), hv_d,
                             hv_layout, d_hv, d_n2, nullptr, nd, &c->last_kernel[HG_T_ENCODE]));
  HG_HIP(c, hipMemcpyAsync(hv_out, d_hv, (size_t)hv_d * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipMemcpyAsync(norm2_out, d_n2, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HG_HIP(c, hipStreamSynchronize(c->stream));
  return HG_OK;
}
