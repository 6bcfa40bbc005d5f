// hg_multi.hip -- several GPUs in one process behind the C ABI (include/hypergen.h, "several GPUs in one
// process").  Host code only: every shard is an ordinary hg_ctx and runs the single-GPU entry points; this file
// adds the partitioning of SURVEY.md 8(e), the device-to-device all-gather of the reference HV matrix and the
// merge of the per-shard hit lists.
//
// Exchange step.  MI355X boards are fully connected by xGMI (7 links per GPU), so the all-gather is done as
// direct pulls: every GPU copies each peer's row block straight into its own gathered matrix with
// hipMemcpyPeerAsync -- 7 concurrent transfers per GPU, one per link, each block crossing exactly one link.
// (A ring all-gather would push every block over n - 1 hops of a per-link-bound ring.)  Ordering is by events:
// a block is published by an event on its owner's stream, the puller's stream waits for that event.
//
// The same exchange through RCCL (hg_multi_set_gather(m, HG_GATHER_RCCL); SURVEY.md 8(e): "one ncclAllGather of
// the R x D i16 ref matrix + R i32 norms"): one communicator per shard from ncclCommInitAll, the collective queued
// on every shard's stream inside one ncclGroupStart/End -- ncclAllGather when the row blocks have equal sizes,
// one ncclBroadcast per owner otherwise (the all-gather-v idiom).  librccl is opened with dlopen the first time
// the mode is selected, so the library carries no link-time dependency on it (the Makefile links -ldl for dlopen itself:
// glibc < 2.34 keeps it in libdl), and no build-time one either: without the rccl-dev header the handful of
// declarations used here are restated from the public NCCL API.
#include <dlfcn.h>
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
extern "C" {
typedef struct ncclComm *ncclComm_t;
typedef enum { ncclSuccess = 0, ncclUnhandledCudaError = 1, ncclSystemError = 2, ncclInternalError = 3 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclUint8 = 1 } ncclDataType_t;
ncclResult_t ncclCommInitAll(ncclComm_t *comm, int ndev, const int *devlist);
ncclResult_t ncclCommDestroy(ncclComm_t comm);
ncclResult_t ncclAllGather(const void *sendbuff, void *recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm,
                           hipStream_t stream);
ncclResult_t ncclBroadcast(const void *sendbuff, void *recvbuff, size_t count, ncclDataType_t datatype, int root,
                           ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclGroupStart(void);
ncclResult_t ncclGroupEnd(void);
const char *ncclGetErrorString(ncclResult_t result);
ncclResult_t ncclGetVersion(int *version);
}
#endif

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "hg_internal.h"

namespace {
struct RcclApi {
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclBroadcast) Broadcast = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclGetVersion) GetVersion = nullptr;
  std::string why;  // why it is unusable, if it is
  bool ok = false;
};
const RcclApi &rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    void *h = nullptr;
    // a copy that is already in the process (PyTorch ships its own) is reused through the soname lookup
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
      if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) {
      const char *e = dlerror();
      api.why = std::string("librccl not loadable: ") + (e ? e : "?");
      return;
    }
    bool all = true;
    auto sym = [&](const char *n) {
      void *p = dlsym(h, n);
      if (!p) all = false, api.why = std::string("librccl lacks ") + n;
      return p;
    };
    api.CommInitAll = reinterpret_cast<decltype(api.CommInitAll)>(sym("ncclCommInitAll"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
    api.AllGather = reinterpret_cast<decltype(api.AllGather)>(sym("ncclAllGather"));
    api.Broadcast = reinterpret_cast<decltype(api.Broadcast)>(sym("ncclBroadcast"));
    api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
    api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
    api.GetVersion = reinterpret_cast<decltype(api.GetVersion)>(sym("ncclGetVersion"));
    api.ok = all;
  });
  return api;
}
}  // namespace

struct hg_multi {
  std::vector<hg_ctx *> ctx;
  std::vector<int> dev;
  std::string err;
  struct Shard {
    hg_ctx::Buf ref_all, n2_all;  // gathered reference matrix + norms (every shard holds all rows)
    hg_ctx::Buf mine, mine_n2;    // this shard's uploaded reference rows (host entry points)
    hg_ctx::Buf qry, qry_n2;      // this shard's query rows (host entry points)
    hg_ctx::Buf hits;             // per-shard hit list
    // the byte form's exchange of PREPARED operands (dist_form): this shard's own rows as byte operands + control records +
    // flag word, and what it gathers from all owners
    hg_ctx::Buf ops_mine, meta_mine, flag_mine, ops_all, meta_all, flags_all;
    hipEvent_t ready = nullptr;   // "this shard's published rows are complete"
  };
  std::vector<Shard> sh;
  int gather = HG_GATHER_PEER;
  std::vector<ncclComm_t> comm;  // one per shard once HG_GATHER_RCCL was selected
  std::string peer_report;       // what hipDeviceEnablePeerAccess said at creation
  std::string gather_report;     // how the last exchange step ran
};

namespace {

hg_status mfail(hg_multi *m, hg_status s, const std::string &msg) {
  if (m) m->err = msg;
  return s;
}

// run fn(shard) on one host thread per shard; the first failing status wins
template <class F>
hg_status for_each_shard(hg_multi *m, F &&fn) {
  const int n = (int)m->ctx.size();
  std::vector<hg_status> st(n, HG_OK);
  if (n == 1) {
    st[0] = fn(0);
  } else {
    std::vector<std::thread> th;
    th.reserve(n);
    for (int s = 0; s < n; ++s) th.emplace_back([&, s] { st[s] = fn(s); });
    for (auto &t : th) t.join();
  }
  for (int s = 0; s < n; ++s)
    if (st[s] != HG_OK && st[s] != HG_ERR_CAPACITY)
      return mfail(m, st[s], "shard " + std::to_string(s) + " (device " + std::to_string(m->dev[s]) + "): " +
                                 hg_last_error(m->ctx[s]));
  for (int s = 0; s < n; ++s)
    if (st[s] == HG_ERR_CAPACITY) return HG_ERR_CAPACITY;
  return HG_OK;
}

// dst (on shard d) <- src (on shard s), ordered on shard d's stream
hipError_t peer_copy(hg_multi *m, int d, void *dst, int s, const void *src, size_t bytes) {
  if (!bytes) return hipSuccess;
  if (m->dev[d] == m->dev[s]) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, m->ctx[d]->stream);
  return hipMemcpyPeerAsync(dst, m->dev[d], src, m->dev[s], bytes, m->ctx[d]->stream);
}

}  // namespace

extern "C" void hg_shard_range(size_t n, int shard, int n_shards, size_t *lo, size_t *hi) {
  if (n_shards < 1) n_shards = 1;
  if (shard < 0) shard = 0;
  if (shard >= n_shards) shard = n_shards - 1;
  const size_t base = n / (size_t)n_shards, rem = n % (size_t)n_shards, s = (size_t)shard;
  const size_t l = s * base + std::min(s, rem);
  if (lo) *lo = l;
  if (hi) *hi = l + base + (s < rem ? 1 : 0);
}

extern "C" hg_status hg_multi_create(const int *device_ids, int n, hg_multi **out) {
  if (!out) return HG_ERR_INVALID;
  *out = nullptr;
  if (!device_ids || n < 1 || n > 64) return hg_fail(nullptr, HG_ERR_INVALID, "device_ids: 1..64 entries");
  hg_multi *m = new (std::nothrow) hg_multi();
  if (!m) return hg_fail(nullptr, HG_ERR_OOM, "hg_multi allocation");
  m->sh.resize(n);
  for (int s = 0; s < n; ++s) {
    hg_ctx *c = nullptr;
    const hg_status st = hg_ctx_create(device_ids[s], &c);
    if (st != HG_OK) {
      hg_multi_destroy(m);
      return st;  // message already in the thread's creation-error slot
    }
    m->ctx.push_back(c), m->dev.push_back(device_ids[s]);
    if (hipSetDevice(device_ids[s]) != hipSuccess ||
        hipEventCreateWithFlags(&m->sh[s].ready, hipEventDisableTiming) != hipSuccess) {
      hg_multi_destroy(m);
      return hg_fail(nullptr, HG_ERR_HIP, "hg_multi: event creation failed");
    }
  }
  // direct xGMI access between distinct devices (hipMemcpyPeerAsync stages through the host without it).  The
  // outcome is kept for the caller (hg_multi_peer_report): a pair without peer access still works, at PCIe speed.
  int pairs = 0, enabled = 0;
  std::string failed;
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) {
      if (m->dev[a] == m->dev[b]) continue;
      bool seen = false;  // repeated ids: report every ordered device pair once
      for (int a2 = 0; a2 <= a && !seen; ++a2)
        for (int b2 = 0; b2 < (a2 == a ? b : n) && !seen; ++b2)
          seen = m->dev[a2] == m->dev[a] && m->dev[b2] == m->dev[b];
      if (seen) continue;
      ++pairs;
      int can = 0;
      hipError_t e = hipDeviceCanAccessPeer(&can, m->dev[a], m->dev[b]);
      if (e == hipSuccess && can) {
        (void)hipSetDevice(m->dev[a]);
        e = hipDeviceEnablePeerAccess(m->dev[b], 0);
        if (e == hipErrorPeerAccessAlreadyEnabled) e = hipSuccess, (void)hipGetLastError();
      } else if (e == hipSuccess) {
        e = hipErrorPeerAccessUnsupported;
      }
      if (e == hipSuccess) {
        ++enabled;
      } else {
        (void)hipGetLastError();
        failed += " " + std::to_string(m->dev[a]) + "->" + std::to_string(m->dev[b]) + " (" + hipGetErrorName(e) + ")";
      }
    }
  m->peer_report = "peer access enabled for " + std::to_string(enabled) + " of " + std::to_string(pairs) +
                   " ordered device pairs" + (failed.empty() ? std::string() : "; host-staged copies for:" + failed);
  *out = m;
  return HG_OK;
}

extern "C" const char *hg_multi_peer_report(const hg_multi *m) { return m ? m->peer_report.c_str() : ""; }
extern "C" const char *hg_multi_gather_report(const hg_multi *m) { return m ? m->gather_report.c_str() : ""; }
extern "C" int hg_multi_gather_mode(const hg_multi *m) { return m ? m->gather : -1; }

extern "C" hg_status hg_multi_set_ani_metric(hg_multi *m, int metric) {
  if (!m) return HG_ERR_INVALID;
  if (metric != HG_ANI_MASH && metric != HG_ANI_CONTAINMENT && metric != HG_ANI_MAX_CONTAINMENT)
    return mfail(m, HG_ERR_INVALID, "unknown ANI metric " + std::to_string(metric));
  for (hg_ctx *c : m->ctx) c->ani_metric = metric;  // (host-side state: no device involved)
  return HG_OK;
}

extern "C" hg_status hg_multi_set_gather(hg_multi *m, int mode) {
  if (!m) return HG_ERR_INVALID;
  if (mode == HG_GATHER_PEER) {
    m->gather = mode;
    return HG_OK;
  }
  if (mode != HG_GATHER_RCCL) return mfail(m, HG_ERR_INVALID, "gather mode: HG_GATHER_PEER or HG_GATHER_RCCL");
  const int n = (int)m->ctx.size();
  for (int a = 0; a < n; ++a)
    for (int b = a + 1; b < n; ++b)
      if (m->dev[a] == m->dev[b])
        return mfail(m, HG_ERR_UNSUPPORTED, "HG_GATHER_RCCL needs distinct devices (one communicator rank per GPU)");
  const RcclApi &r = rccl();
  if (!r.ok) return mfail(m, HG_ERR_UNSUPPORTED, r.why);
  if (m->comm.empty()) {
    for (int s = 0; s < n; ++s) (void)hipSetDevice(m->dev[s]), (void)hipStreamSynchronize(m->ctx[s]->stream);
    std::vector<ncclComm_t> comm(n, nullptr);
    const ncclResult_t e = r.CommInitAll(comm.data(), n, m->dev.data());
    if (e != ncclSuccess) return mfail(m, HG_ERR_HIP, std::string("ncclCommInitAll: ") + r.GetErrorString(e));
    m->comm = comm;
  }
  m->gather = mode;
  return HG_OK;
}

extern "C" void hg_multi_destroy(hg_multi *m) {
  if (!m) return;
  for (size_t s = 0; s < m->ctx.size(); ++s) {
    (void)hipSetDevice(m->dev[s]);
    (void)hipStreamSynchronize(m->ctx[s]->stream);
  }
  for (ncclComm_t c : m->comm)
    if (c) (void)rccl().CommDestroy(c);
  for (size_t s = 0; s < m->ctx.size(); ++s) {
    (void)hipSetDevice(m->dev[s]);
    hg_multi::Shard &x = m->sh[s];
    for (hg_ctx::Buf *b : {&x.ref_all, &x.n2_all, &x.mine, &x.mine_n2, &x.qry, &x.qry_n2, &x.hits, &x.ops_mine, &x.meta_mine,
                           &x.flag_mine, &x.ops_all, &x.meta_all, &x.flags_all})
      if (b->p) (void)hipFree(b->p);
  }
  for (size_t s = 0; s < m->sh.size(); ++s)
    if (m->sh[s].ready) (void)hipEventDestroy(m->sh[s].ready);
  for (hg_ctx *c : m->ctx) hg_ctx_destroy(c);
  delete m;
}

extern "C" int hg_multi_size(const hg_multi *m) { return m ? (int)m->ctx.size() : 0; }
extern "C" hg_ctx *hg_multi_ctx(hg_multi *m, int shard) {
  return (m && shard >= 0 && shard < (int)m->ctx.size()) ? m->ctx[shard] : nullptr;
}
extern "C" const char *hg_multi_last_error(const hg_multi *m) { return m ? m->err.c_str() : hg_last_error(nullptr); }

// ---- sketch: independent units, no exchange ---------------------------------------------------------------
extern "C" hg_status hg_sketch_batch_multi(hg_multi *m, const uint8_t *const *seqs, const size_t *lens, size_t n,
                                           const hg_sketch_params *p, int16_t *hv_out, int32_t *norm2_out,
                                           uint32_t *nhash_out) {
  if (!m) return HG_ERR_INVALID;
  if (!p) return mfail(m, HG_ERR_INVALID, "params == NULL");
  if (n == 0) return HG_OK;
  if (!seqs || !lens || !hv_out || !norm2_out || !nhash_out) return mfail(m, HG_ERR_INVALID, "NULL argument");
  const int ns = (int)m->ctx.size();
  return for_each_shard(m, [&](int s) -> hg_status {
    size_t lo, hi;
    hg_shard_range(n, s, ns, &lo, &hi);
    if (hi == lo) return HG_OK;
    return hg_sketch_batch(m->ctx[s], seqs + lo, lens + lo, hi - lo, p, hv_out + lo * (size_t)p->hv_d, norm2_out + lo,
                           nhash_out + lo);
  });
}

// ---- dist ------------------------------------------------------------------------------------------------------
namespace {

struct DistPlan {
  std::vector<size_t> rlo, rhi;  // reference rows owned (published) by each shard
  std::vector<size_t> clo, chi;  // query columns computed by each shard (global indices)
  size_t R = 0, Q = 0;
};

// every shard's stream idle: no copy queued by a call may outlive it (a peer pull still reading another shard's
// `mine` buffer while the caller's retry re-uploads into it)
void drain(hg_multi *m) {
  for (size_t s = 0; s < m->ctx.size(); ++s)
    if (hipSetDevice(m->dev[s]) == hipSuccess) (void)hipStreamSynchronize(m->ctx[s]->stream);
}
struct DrainOnExit {
  hg_multi *m;
  ~DrainOnExit() { drain(m); }
};

bool rccl_mode(const hg_multi *m) { return m->gather == HG_GATHER_RCCL && !m->comm.empty(); }
bool equal_blocks(const DistPlan &pl) {
  for (size_t t = 1; t < pl.rlo.size(); ++t)
    if (pl.rhi[t] - pl.rlo[t] != pl.rhi[0] - pl.rlo[0]) return false;
  return true;
}

// One array of the exchange step.  Owner t contributes its reference rows -- or, `one_each`, one unit (the byte form's flag
// word) -- of `unit` bytes at src[t]; receiver s holds owner t's block at dst[s] + first(t) * unit, first(t) being the units
// of the owners before t.
struct GatherArray {
  std::vector<const void *> src;  // per owner
  std::vector<void *> dst;        // per receiver
  size_t unit;
  bool one_each = false;
};

// The exchange step: every receiver gets every owner's block of every array.  Receivers are the shards with query columns;
// under RCCL every rank takes part in the collectives, so every shard's dst must be valid there.  Each receiver's stream
// first waits for every other owner's published data, so what the caller queues behind the exchange may read the owners'
// rows as well.  *cross += the bytes pulled between distinct devices.
hg_status exchange(hg_multi *m, const DistPlan &pl, const std::vector<GatherArray> &arrs, size_t *cross) {
  const int ns = (int)m->ctx.size();
  const bool use_rccl = rccl_mode(m);
  auto count = [&](const GatherArray &a, int t) { return a.one_each ? size_t(1) : pl.rhi[t] - pl.rlo[t]; };
  auto block = [&](const GatherArray &a, int s, int t) {
    return static_cast<uint8_t *>(a.dst[s]) + (a.one_each ? (size_t)t : pl.rlo[t]) * a.unit;
  };
  for (int s = 0; s < ns; ++s)
    if (hipSetDevice(m->dev[s]) != hipSuccess || hipEventRecord(m->sh[s].ready, m->ctx[s]->stream) != hipSuccess)
      return mfail(m, HG_ERR_HIP, "hg_dist_multi: event record failed");
  // each receiver waits for the other owners; the direct pulls: one copy per (array, owner), all queued at once on its stream
  for (int s = 0; s < ns; ++s) {
    if (pl.chi[s] == pl.clo[s]) continue;
    hg_ctx *c = m->ctx[s];
    HG_HIP(c, hipSetDevice(m->dev[s]));
    for (int t = 0; t < ns; ++t)
      if (t != s) HG_HIP(c, hipStreamWaitEvent(c->stream, m->sh[t].ready, 0));
    if (use_rccl) continue;
    for (const GatherArray &a : arrs)
      for (int t = 0; t < ns; ++t) {
        const size_t bytes = count(a, t) * a.unit;
        HG_HIP(c, peer_copy(m, s, block(a, s, t), t, a.src[t], bytes));
        if (m->dev[s] != m->dev[t]) *cross += bytes;
      }
  }
  if (!use_rccl) return HG_OK;
  // RCCL: ncclAllGather of equal blocks, one ncclBroadcast per non-empty owner otherwise (the all-gather-v idiom)
  const RcclApi &r = rccl();
  const bool equal = equal_blocks(pl);
  ncclResult_t e = r.GroupStart();
  for (int s = 0; s < ns && e == ncclSuccess; ++s) {
    if (hipSetDevice(m->dev[s]) != hipSuccess) e = ncclSystemError;  // (no return inside the group: GroupEnd closes it)
    const hipStream_t st = m->ctx[s]->stream;
    for (size_t i = 0; i < arrs.size() && e == ncclSuccess; ++i) {
      const GatherArray &a = arrs[i];
      if (a.one_each || equal)
        e = r.AllGather(a.src[s], a.dst[s], count(a, s) * a.unit, ncclUint8, m->comm[s], st);
      else
        for (int t = 0; t < ns && e == ncclSuccess; ++t)
          if (count(a, t)) e = r.Broadcast(a.src[s], block(a, s, t), count(a, t) * a.unit, ncclUint8, t, m->comm[s], st);
    }
  }
  const ncclResult_t e2 = r.GroupEnd();
  if (e == ncclSuccess) e = e2;
  if (e != ncclSuccess) return mfail(m, HG_ERR_HIP, std::string("RCCL all-gather: ") + r.GetErrorString(e));
  return HG_OK;
}

// shard lists back to back into the caller's buffer (hit order is unspecified by contract)
template <class Hit>
hg_status merge_hits(hg_multi *m, const std::vector<size_t> &found, hg_status st, Hit *out, size_t cap, size_t *n_out) {
  const int ns = (int)m->ctx.size();
  size_t total = 0;
  for (int s = 0; s < ns; ++s) total += found[s];
  *n_out = total;
  if (st != HG_OK && st != HG_ERR_CAPACITY) return st;
  if (total > cap) return mfail(m, HG_ERR_CAPACITY, "hit buffer too small");
  size_t at = 0;
  for (int s = 0; s < ns; ++s) {
    if (!found[s]) continue;
    hg_ctx *c = m->ctx[s];
    HG_HIP(c, hipSetDevice(m->dev[s]));
    HG_HIP(c, hipMemcpyAsync(out + at, m->sh[s].hits.p, found[s] * sizeof(Hit), hipMemcpyDeviceToHost, c->stream));
    at += found[s];
  }
  for (int s = 0; s < ns; ++s) {
    HG_HIP(m->ctx[s], hipSetDevice(m->dev[s]));
    HG_HIP(m->ctx[s], hipStreamSynchronize(m->ctx[s]->stream));
  }
  return HG_OK;
}

// One form of the exchange + compute.  The byte form (`ops`) exchanges PREPARED operands: every shard converts its own
// reference rows to centred byte operands + 72-byte control records once (hg_dist_prep_ops_dev), and the receivers gather
// those -- 4.3 KB per row at D = 4096 instead of 8 KB of i16, and no shard repeats another shard's prepass.  In the
// all-vs-all case a shard then pulls the i16 rows of its QUERY range from their owners (under `symmetric` the column ranges
// are balanced by pair count and do not coincide with the row blocks).  It returns HG_ERR_INEXACT, with nothing reported,
// when an owner's or a query side's rows do not fit the byte scheme.  The i16 form gathers the rows themselves.
hg_status dist_form(hg_multi *m, bool ops, const int16_t *const *d_ref, const int32_t *const *d_rn, const int16_t *const *d_qry,
                    const int32_t *const *d_qn, const DistPlan &pl, uint32_t hv_d, uint32_t ksize, int symmetric, float ani_th,
                    hg_ani_hit *out, size_t cap, size_t *n_out) {
  using Shard = hg_multi::Shard;
  const int ns = (int)m->ctx.size();
  const size_t rb = hg_dist_ops_row_bytes(hv_d), mb = hg_dist_ops_meta_bytes(), row16 = (size_t)hv_d * sizeof(int16_t);
  const bool use_rccl = rccl_mode(m);
  std::vector<size_t> found(ns, 0), caps(ns, 0);
  // phase 1 (one thread per shard): workspaces, and in the byte form the shard's own rows prepared on its stream
  hg_status st = for_each_shard(m, [&](int s) -> hg_status {
    hg_ctx *c = m->ctx[s];
    Shard &x = m->sh[s];
    const size_t rows = pl.rhi[s] - pl.rlo[s], qn_rows = pl.chi[s] - pl.clo[s];
    HG_HIP(c, hipSetDevice(m->dev[s]));
    hg_status e;
    if (qn_rows || use_rccl) {  // the gathered arrays
      if (ops) {
        if ((e = hg_ensure(c, x.ops_all, hg_dist_ops_padded_rows(pl.R) * rb + 64)) != HG_OK) return e;
        if ((e = hg_ensure(c, x.meta_all, pl.R * mb + 64)) != HG_OK) return e;
        if ((e = hg_ensure(c, x.flags_all, (size_t)ns * sizeof(uint32_t) + 64)) != HG_OK) return e;
      } else if ((e = hg_ensure(c, x.ref_all, pl.R * row16 + 64)) != HG_OK) {
        return e;
      }
      if ((e = hg_ensure(c, x.n2_all, pl.R * sizeof(int32_t) + 64)) != HG_OK) return e;
    }
    // capacity of this shard's list: its share of the caller's capacity can be exceeded by a skewed hit
    // distribution, so it gets the whole `cap`, bounded by its pair count
    caps[s] = (size_t)std::min<unsigned __int128>((unsigned __int128)pl.R * qn_rows, cap);
    if ((e = hg_ensure(c, x.hits, caps[s] * sizeof(hg_ani_hit) + 64)) != HG_OK) return e;
    if (!ops) return HG_OK;
    if (!d_qry && qn_rows) {  // all-vs-all: this shard's query rows, assembled below
      if ((e = hg_ensure(c, x.qry, qn_rows * row16 + 64)) != HG_OK) return e;
      if ((e = hg_ensure(c, x.qry_n2, qn_rows * sizeof(int32_t) + 64)) != HG_OK) return e;
    }
    if ((e = hg_ensure(c, x.ops_mine, rows * rb + 64)) != HG_OK) return e;
    if ((e = hg_ensure(c, x.meta_mine, rows * mb + 64)) != HG_OK) return e;
    if ((e = hg_ensure(c, x.flag_mine, 64)) != HG_OK) return e;
    HG_HIP(c, hipMemsetAsync(x.flag_mine.p, 0, 16, c->stream));
    return hg_dist_prep_ops_dev(c, d_ref[s], rows, hv_d, static_cast<uint8_t *>(x.ops_mine.p), static_cast<uint8_t *>(x.meta_mine.p),
                                static_cast<uint32_t *>(x.flag_mine.p));
  });
  if (st != HG_OK) return st;
  // phase 2 (this thread): the exchange, queued on the receivers' streams behind the owners' "ready" events
  auto mine = [&](hg_ctx::Buf Shard::*b) { std::vector<const void *> v; for (Shard &x : m->sh) v.push_back((x.*b).p); return v; };
  auto all = [&](hg_ctx::Buf Shard::*b) { std::vector<void *> v; for (Shard &x : m->sh) v.push_back((x.*b).p); return v; };
  const std::vector<const void *> ref(d_ref, d_ref + ns), rn(d_rn, d_rn + ns);
  std::vector<GatherArray> arrs;
  if (ops)
    arrs = {{mine(&Shard::ops_mine), all(&Shard::ops_all), rb},
            {mine(&Shard::meta_mine), all(&Shard::meta_all), mb},
            {rn, all(&Shard::n2_all), sizeof(int32_t)},
            {mine(&Shard::flag_mine), all(&Shard::flags_all), sizeof(uint32_t), true}};
  else
    arrs = {{ref, all(&Shard::ref_all), row16}, {rn, all(&Shard::n2_all), sizeof(int32_t)}};
  size_t cross = 0;
  if ((st = exchange(m, pl, arrs, &cross)) != HG_OK) return st;
  for (int s = 0; s < ns && ops && !d_qry; ++s) {  // all-vs-all byte form: the part of s's query range that owner t holds
    hg_ctx *c = m->ctx[s];
    Shard &x = m->sh[s];
    HG_HIP(c, hipSetDevice(m->dev[s]));
    for (int t = 0; t < ns; ++t) {
      const size_t lo = std::max(pl.clo[s], pl.rlo[t]), hi = std::min(pl.chi[s], pl.rhi[t]);
      if (lo >= hi) continue;
      HG_HIP(c, peer_copy(m, s, static_cast<int16_t *>(x.qry.p) + (lo - pl.clo[s]) * (size_t)hv_d, t,
                          d_ref[t] + (lo - pl.rlo[t]) * (size_t)hv_d, (hi - lo) * row16));
      HG_HIP(c, peer_copy(m, s, static_cast<int32_t *>(x.qry_n2.p) + (lo - pl.clo[s]), t, d_rn[t] + (lo - pl.rlo[t]),
                          (hi - lo) * sizeof(int32_t)));
      if (m->dev[s] != m->dev[t]) cross += (hi - lo) * (row16 + sizeof(int32_t));
    }
  }
  // phase 3 (one thread per shard): (all refs) x (this shard's query rows)
  std::vector<hg_status> sst(ns, HG_OK);
  st = for_each_shard(m, [&](int s) -> hg_status {
    hg_ctx *c = m->ctx[s];
    Shard &x = m->sh[s];
    const size_t qn_rows = pl.chi[s] - pl.clo[s];
    if (qn_rows == 0) return HG_OK;
    HG_HIP(c, hipSetDevice(m->dev[s]));
    const auto *g_hv = static_cast<const int16_t *>(x.ref_all.p);
    const auto *g_n2 = static_cast<const int32_t *>(x.n2_all.p);
    const int16_t *q_hv = d_qry ? d_qry[s] : ops ? static_cast<const int16_t *>(x.qry.p) : g_hv + pl.clo[s] * (size_t)hv_d;
    const int32_t *q_n2 = d_qry ? d_qn[s] : ops ? static_cast<const int32_t *>(x.qry_n2.p) : g_n2 + pl.clo[s];
    auto *hits = static_cast<hg_ani_hit *>(x.hits.p);
    if (!ops)
      return hg_dist_block_dev(c, g_hv, g_n2, pl.R, 0, q_hv, q_n2, qn_rows, pl.clo[s], hv_d, ksize, symmetric, ani_th, hits, caps[s],
                               &found[s]);
    sst[s] = hg_dist_block_ops_dev(c, static_cast<const uint8_t *>(x.ops_all.p), static_cast<const uint8_t *>(x.meta_all.p), g_n2,
                                   pl.R, 0, nullptr, static_cast<const uint32_t *>(x.flags_all.p), (size_t)ns, q_hv, q_n2, qn_rows,
                                   pl.clo[s], hv_d, ksize, symmetric, ani_th, hits, caps[s], &found[s]);
    return sst[s] == HG_ERR_INEXACT ? HG_OK : sst[s];
  });
  for (int s = 0; s < ns; ++s)
    if (sst[s] == HG_ERR_INEXACT) return HG_ERR_INEXACT;  // (an owner's veto is seen by every shard; a query side's by its own)
  // hg_multi_gather_report: how the exchange of the call that produced the hits ran
  size_t per_shard = 0;
  for (const GatherArray &a : arrs) per_shard += (a.one_each ? (size_t)ns : pl.R) * a.unit;
  std::string how = "peer pulls (hipMemcpyPeerAsync)";
  if (use_rccl) {
    int ver = 0;
    (void)rccl().GetVersion(&ver);
    how = std::string("rccl ") + (equal_blocks(pl) ? "ncclAllGather" : "grouped ncclBroadcast") + " over " + std::to_string(ns) +
          " ranks (version " + std::to_string(ver) + ")";
  }
  how += (ops ? ", prepared byte operands + control records: " : ", i16 rows: ") + std::to_string(per_shard) + " B per shard";
  if (ops) how += " instead of " + std::to_string(pl.R * (row16 + sizeof(int32_t))) + " B of i16 rows";
  m->gather_report = how + ", " + std::to_string(cross) + " B between distinct devices; " + m->peer_report;
  // phase 4: the per-shard lists into the caller's buffer
  return merge_hits(m, found, st, out, cap, n_out);
}

// d_ref / d_rn: shard s's reference rows on its device.  d_qry == nullptr: all-vs-all on the gathered matrix.
hg_status dist_core(hg_multi *m, const int16_t *const *d_ref, const int32_t *const *d_rn, const int16_t *const *d_qry,
                    const int32_t *const *d_qn, const DistPlan &pl, uint32_t hv_d, uint32_t ksize, int symmetric,
                    float ani_th, hg_ani_hit *out, size_t cap, size_t *n_out) {
  DrainOnExit drain_guard{m};  // every return below leaves all shard streams idle
  // the byte form first (half the bytes, no repeated prepass); a veto -- sketches that do not fit the byte scheme -- or
  // the "f16" hook on shard 0 brings the i16 form
  if (hv_d <= 8192 && hv_d % 8 == 0 && m->ctx[0]->dbg_dist_path != "f16") {
    const hg_status os = dist_form(m, true, d_ref, d_rn, d_qry, d_qn, pl, hv_d, ksize, symmetric, ani_th, out, cap, n_out);
    if (os != HG_ERR_INEXACT) return os;
    drain(m);
    *n_out = 0;
  }
  return dist_form(m, false, d_ref, d_rn, d_qry, d_qn, pl, hv_d, ksize, symmetric, ani_th, out, cap, n_out);
}

// column ranges of the all-vs-all case: by pair count under `symmetric` (column j pairs with j rows)
void all_vs_all_columns(size_t n, int ns, int symmetric, DistPlan &pl) {
  pl.clo.resize(ns), pl.chi.resize(ns);
  for (int s = 0; s < ns; ++s) {
    if (symmetric) {
      pl.clo[s] = (size_t)std::llround((double)n * std::sqrt((double)s / ns));
      pl.chi[s] = s + 1 == ns ? n : (size_t)std::llround((double)n * std::sqrt((double)(s + 1) / ns));
    } else {
      hg_shard_range(n, s, ns, &pl.clo[s], &pl.chi[s]);
    }
  }
}

// The checks the several-GPU entry points start with, in this order.  `empty`: nothing to compare -- HG_OK before any
// pointer is looked at (empty host matrices may come as NULL); `bad`: the entry point's own argument defect, if any.
hg_status check_args(hg_multi *m, size_t *n_out, bool empty, const char *bad, int symmetric) {
  if (!m) return HG_ERR_INVALID;
  if (!n_out) return mfail(m, HG_ERR_INVALID, "n_out == NULL");
  *n_out = 0;
  if (empty) return HG_OK;
  if (bad) return mfail(m, HG_ERR_INVALID, bad);
  if (symmetric && m->ctx[0]->ani_metric == HG_ANI_CONTAINMENT)
    return mfail(m, HG_ERR_INVALID, "symmetric != 0 with HG_ANI_CONTAINMENT: the metric is directional");
  return HG_OK;
}

// host rows [lo, hi) of `row_bytes` each -- and their norms, given n2_buf -- into a shard's buffers, queued on its stream
hg_status upload_rows(hg_ctx *c, hg_ctx::Buf &buf, const void *rows, size_t lo, size_t hi, size_t row_bytes,
                      hg_ctx::Buf *n2_buf = nullptr, const int32_t *n2 = nullptr) {
  const size_t n = hi - lo;
  hg_status e;
  if ((e = hg_ensure(c, buf, n * row_bytes + 64)) != HG_OK) return e;
  if (n2_buf && (e = hg_ensure(c, *n2_buf, n * sizeof(int32_t) + 64)) != HG_OK) return e;
  if (!n) return HG_OK;
  const auto *src = static_cast<const uint8_t *>(rows) + lo * row_bytes;
  HG_HIP(c, hipMemcpyAsync(buf.p, src, n * row_bytes, hipMemcpyHostToDevice, c->stream));
  if (n2_buf) HG_HIP(c, hipMemcpyAsync(n2_buf->p, n2 + lo, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  return HG_OK;
}

}  // namespace

extern "C" hg_status hg_dist_multi_dev(hg_multi *m, const int16_t *const *d_ref_hv, const int32_t *const *d_ref_norm2,
                                       const size_t *ref_rows, const int16_t *const *d_qry_hv,
                                       const int32_t *const *d_qry_norm2, const size_t *qry_rows, uint32_t hv_d,
                                       uint32_t ksize, int symmetric, float ani_th, hg_ani_hit *out, size_t cap,
                                       size_t *n_out) {
  const char *bad = !d_ref_hv || !d_ref_norm2 || !ref_rows || (cap && !out) ? "NULL argument"
                    : d_qry_hv && (!d_qry_norm2 || !qry_rows) ? "query shards need norms and row counts" : nullptr;
  hg_status st = check_args(m, n_out, false, bad, symmetric);
  if (st != HG_OK) return st;
  const int ns = (int)m->ctx.size();
  for (int s = 0; s < ns; ++s) {  // the shards' operands may be the outputs of a sketch step still queued on their ctx
    if (hipSetDevice(m->dev[s]) != hipSuccess) return mfail(m, HG_ERR_HIP, "hipSetDevice");
    if ((st = hg_sketch_resolve(m->ctx[s])) != HG_OK) return mfail(m, st, hg_last_error(m->ctx[s]));
  }
  DistPlan pl;
  pl.rlo.resize(ns), pl.rhi.resize(ns);
  for (int s = 0; s < ns; ++s) {
    pl.rlo[s] = pl.R, pl.R += ref_rows[s], pl.rhi[s] = pl.R;
    if (ref_rows[s] && (!d_ref_hv[s] || !d_ref_norm2[s])) return mfail(m, HG_ERR_INVALID, "NULL reference shard");
  }
  if (d_qry_hv) {
    pl.clo.resize(ns), pl.chi.resize(ns);
    for (int s = 0; s < ns; ++s) {
      pl.clo[s] = pl.Q, pl.Q += qry_rows[s], pl.chi[s] = pl.Q;
      if (qry_rows[s] && (!d_qry_hv[s] || !d_qry_norm2[s])) return mfail(m, HG_ERR_INVALID, "NULL query shard");
    }
  } else {
    pl.Q = pl.R;
    all_vs_all_columns(pl.R, ns, symmetric, pl);
  }
  if (pl.R == 0 || pl.Q == 0) return HG_OK;
  return dist_core(m, d_ref_hv, d_ref_norm2, d_qry_hv, d_qry_norm2, pl, hv_d, ksize, symmetric, ani_th, out, cap, n_out);
}

extern "C" hg_status hg_dist_multi(hg_multi *m, const int16_t *ref_hv, const int32_t *ref_norm2, size_t R,
                                   const int16_t *qry_hv, const int32_t *qry_norm2, size_t Q, uint32_t hv_d,
                                   uint32_t ksize, int symmetric, float ani_th, hg_ani_hit *out, size_t cap,
                                   size_t *n_out) {
  const char *bad = !ref_hv || !ref_norm2 || !qry_hv || !qry_norm2 || (cap && !out) ? "NULL argument"
                    : hv_d == 0 ? "hv_d == 0" : nullptr;
  const hg_status st = check_args(m, n_out, R == 0 || Q == 0, bad, symmetric);
  if (st != HG_OK || R == 0 || Q == 0) return st;
  const int ns = (int)m->ctx.size();
  const bool same = ref_hv == qry_hv && ref_norm2 == qry_norm2 && R == Q;
  const size_t row_bytes = (size_t)hv_d * sizeof(int16_t);
  DistPlan pl;
  pl.R = R, pl.Q = Q;
  pl.rlo.resize(ns), pl.rhi.resize(ns);
  for (int s = 0; s < ns; ++s) hg_shard_range(R, s, ns, &pl.rlo[s], &pl.rhi[s]);
  if (same) {
    all_vs_all_columns(R, ns, symmetric, pl);
  } else {
    pl.clo.resize(ns), pl.chi.resize(ns);
    for (int s = 0; s < ns; ++s) hg_shard_range(Q, s, ns, &pl.clo[s], &pl.chi[s]);
  }
  // upload: every reference row crosses PCIe once, to the GPU that publishes it; query rows go to their shard
  std::vector<const int16_t *> d_ref(ns), d_qry(ns);
  std::vector<const int32_t *> d_rn(ns), d_qn(ns);
  const hg_status up = for_each_shard(m, [&](int s) -> hg_status {
    hg_ctx *c = m->ctx[s];
    hg_multi::Shard &x = m->sh[s];
    HG_HIP(c, hipSetDevice(m->dev[s]));
    hg_status e = upload_rows(c, x.mine, ref_hv, pl.rlo[s], pl.rhi[s], row_bytes, &x.mine_n2, ref_norm2);
    if (e == HG_OK && !same) e = upload_rows(c, x.qry, qry_hv, pl.clo[s], pl.chi[s], row_bytes, &x.qry_n2, qry_norm2);
    d_ref[s] = static_cast<const int16_t *>(x.mine.p), d_rn[s] = static_cast<const int32_t *>(x.mine_n2.p);
    d_qry[s] = static_cast<const int16_t *>(x.qry.p), d_qn[s] = static_cast<const int32_t *>(x.qry_n2.p);
    return e;
  });
  if (up != HG_OK) return up;
  return dist_core(m, d_ref.data(), d_rn.data(), same ? nullptr : d_qry.data(), same ? nullptr : d_qn.data(), pl, hv_d,
                   ksize, symmetric, ani_th, out, cap, n_out);
}

// ---- bit-packed database search: references sharded, queries broadcast, hits merged ----------------------------
extern "C" hg_status hg_hamming_search_multi(hg_multi *m, const uint32_t *ref_bits, size_t R, const uint32_t *qry_bits,
                                             size_t Q, uint32_t hv_d, uint32_t max_dist, hg_ham_hit *out, size_t cap,
                                             size_t *n_out) {
  const char *bad = !ref_bits || !qry_bits || (cap && !out) ? "NULL argument" : nullptr;
  const hg_status chk = check_args(m, n_out, R == 0 || Q == 0, bad, 0);
  if (chk != HG_OK || R == 0 || Q == 0) return chk;
  const int ns = (int)m->ctx.size();
  const size_t row_bytes = (hv_d + 31) / 32 * sizeof(uint32_t);
  std::vector<size_t> found(ns, 0), caps(ns, 0);
  DrainOnExit drain_guard{m};  // every return below leaves all shard streams idle
  const hg_status st = for_each_shard(m, [&](int s) -> hg_status {
    size_t lo, hi;
    hg_shard_range(R, s, ns, &lo, &hi);
    if (hi == lo) return HG_OK;
    hg_ctx *c = m->ctx[s];
    hg_multi::Shard &x = m->sh[s];
    HG_HIP(c, hipSetDevice(m->dev[s]));
    caps[s] = (size_t)std::min<unsigned __int128>((unsigned __int128)(hi - lo) * Q, cap);
    hg_status e;
    if ((e = hg_ensure(c, x.hits, caps[s] * sizeof(hg_ham_hit) + 64)) != HG_OK) return e;
    if ((e = upload_rows(c, x.mine, ref_bits, lo, hi, row_bytes)) != HG_OK) return e;
    if ((e = upload_rows(c, x.qry, qry_bits, 0, Q, row_bytes)) != HG_OK) return e;  // broadcast: one PCIe link per GPU
    return hg_hamming_search_block_dev(c, static_cast<const uint32_t *>(x.mine.p), hi - lo, lo,
                                       static_cast<const uint32_t *>(x.qry.p), Q, 0, hv_d, max_dist,
                                       static_cast<hg_ham_hit *>(x.hits.p), caps[s], &found[s]);
  });
  return merge_hits(m, found, st, out, cap, n_out);
}

// ---- search top-k: references sharded by rows where they live, every shard holds all query rows, lists merged ---------
extern "C" hg_status hg_search_topk_multi_dev(hg_multi *m, const int16_t *const *d_ref_hv, const int32_t *const *d_ref_norm2,
                                              const size_t *ref_rows, const int16_t *const *d_qry_hv,
                                              const int32_t *const *d_qry_norm2, size_t Q, uint32_t hv_d, uint32_t ksize,
                                              float ani_th, uint32_t k, hg_ani_hit *out, uint32_t *counts) {
  if (!m) return HG_ERR_INVALID;
  if (k == 0 || Q == 0) return HG_OK;
  if (k > HG_SEARCH_TOPK_MAX) return mfail(m, HG_ERR_UNSUPPORTED, "k exceeds HG_SEARCH_TOPK_MAX");
  if (!d_ref_hv || !d_ref_norm2 || !ref_rows || !d_qry_hv || !d_qry_norm2 || !out || !counts) return mfail(m, HG_ERR_INVALID, "NULL argument");
  const int ns = (int)m->ctx.size();
  std::vector<size_t> first(ns + 1, 0);
  for (int s = 0; s < ns; ++s) {
    first[s + 1] = first[s] + ref_rows[s];
    if ((ref_rows[s] && (!d_ref_hv[s] || !d_ref_norm2[s])) || !d_qry_hv[s] || !d_qry_norm2[s]) return mfail(m, HG_ERR_INVALID, "NULL shard operand");
  }
  if (first[ns] > 0x7FFFFFFFull) return mfail(m, HG_ERR_UNSUPPORTED, "R must be < 2^31");
  const size_t slots = Q * (size_t)k, ob = slots * sizeof(hg_ani_hit);
  std::vector<std::vector<hg_ani_hit>> lists(ns, std::vector<hg_ani_hit>(slots));
  std::vector<std::vector<uint32_t>> cnts(ns, std::vector<uint32_t>(Q));
  DrainOnExit drain_guard{m};  // every return below leaves all shard streams idle
  const hg_status st = for_each_shard(m, [&](int s) -> hg_status {
    hg_ctx *c = m->ctx[s];
    hg_multi::Shard &x = m->sh[s];
    HG_HIP(c, hipSetDevice(m->dev[s]));
    hg_status e;
    if ((e = hg_ensure(c, x.hits, ob + Q * sizeof(uint32_t) + 64)) != HG_OK) return e;
    auto *d_out = static_cast<hg_ani_hit *>(x.hits.p);
    auto *d_cnt = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(x.hits.p) + ob);
    if ((e = hg_search_topk_block_dev(c, d_ref_hv[s], d_ref_norm2[s], ref_rows[s], first[s], d_qry_hv[s], d_qry_norm2[s], Q, 0, hv_d,
                                      ksize, ani_th, k, d_out, d_cnt)) != HG_OK)
      return e;
    HG_HIP(c, hipMemcpyAsync(lists[s].data(), d_out, ob, hipMemcpyDeviceToHost, c->stream));
    HG_HIP(c, hipMemcpyAsync(cnts[s].data(), d_cnt, Q * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HG_HIP(c, hipStreamSynchronize(c->stream));
    return HG_OK;
  });
  if (st != HG_OK) return st;
  std::vector<const hg_ani_hit *> lp(ns);
  std::vector<const uint32_t *> cp(ns);
  for (int s = 0; s < ns; ++s) lp[s] = lists[s].data(), cp[s] = cnts[s].data();
  return hg_search_topk_merge(lp.data(), cp.data(), (size_t)ns, Q, k, out, counts);
}
