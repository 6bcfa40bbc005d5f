// hg_sort_kernels.hip -- set semantics (sort + unique) on gfx950.
//
// sort_unique : the HashSet<u64> of src/sketch.rs:93 / src/sketch_cuda.rs:158-163, as an
//               ascending duplicate-free list per genome (bitonic sort in LDS, one workgroup
//               per genome; a global-memory variant covers genomes whose hit count exceeds
//               the LDS budget).
#include "hg_block_scan.h"
#include "hg_internal.h"

namespace {

constexpr int SORT_WG = 512;
constexpr uint32_t SORT_LDS_MAX_KEYS = HG_SORT_LDS_MAX_KEYS;  // 64 KiB of keys + 32 KiB of counters of the 160 KiB LDS

// one compare-exchange pass of the bitonic network over a[0..n2), n2 a power of two
template <class Ptr>
__device__ __forceinline__ void bitonic_sort(Ptr a, uint32_t n2, uint32_t tid, uint32_t nthr) {
  for (uint32_t k = 2; k <= n2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < (n2 >> 1); t += nthr) {
        // t-th pair of this stage
        uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        uint32_t hi = lo | j;
        bool up = (lo & k) == 0;
        uint64_t x = a[lo], y = a[hi];
        if ((x > y) == up) {
          a[lo] = y;
          a[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ uint32_t next_pow2(uint32_t v) {
  uint32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

constexpr uint32_t SORT_BUCKET_MAX_KEYS = 8192, SORT_BUCKET_LIMIT = 16, SORT_KPT = SORT_BUCKET_MAX_KEYS / SORT_WG;
static_assert(SORT_BUCKET_MAX_KEYS == SORT_LDS_MAX_KEYS, "every set the one-workgroup sort takes can take its counting sort");
constexpr size_t SORT_LDS_BYTES_MAX = (size_t)SORT_LDS_MAX_KEYS * (sizeof(uint64_t) + sizeof(uint32_t));  // keys + counters

// The counting sort of n keys (SORT_WG <= n2 = next_pow2(n) <= SORT_KPT * SORT_WG) into s_keys by the whole workgroup.
// The callers' keys are uniform over a known range, so a monotone map bucket_of: key -> [0, n2) puts 0.5-1 keys into each
// of n2 buckets on average.  Count (one returning LDS atomic per key: its rank inside the bucket), scan, scatter, then every
// thread orders the few keys of its n2 / SORT_WG buckets by insertion: five passes over the keys instead of the bitonic
// network's 66 (2 048 keys) to 78 (8 192) -- 3.4 -> ... ms for 50 M keys in 32 000 buckets of hg_launch_sort_large.
// s_bk: n2 words, the bucket counters and then the bucket starts.  Returns whether s_keys[0..n) is ordered.  A bucket with
// more than SORT_BUCKET_LIMIT keys (repeats: equal keys share a bucket) gives the sort up: false, and the keys are all in
// s_keys, padded with ~0 to n2, for the caller's bitonic_sort.  Ends on a barrier.
template <class BucketOf>
__device__ __forceinline__ bool counting_sort_lds(const uint64_t *__restrict__ src, const uint32_t n, const uint32_t n2,
                                                  uint64_t *s_keys, uint32_t *s_bk, uint32_t *s_scan, BucketOf bucket_of) {
  __shared__ uint32_t s_over;
  const uint32_t tid = threadIdx.x, per = n2 / SORT_WG;
  for (uint32_t i = tid; i < n2; i += SORT_WG) s_bk[i] = 0;
  if (tid == 0) s_over = 0;
  __syncthreads();
  uint64_t kk[SORT_KPT];
  uint32_t bb[SORT_KPT], rr[SORT_KPT];
#pragma unroll
  for (uint32_t u = 0; u < SORT_KPT; ++u) {
    const uint32_t i = tid + u * SORT_WG;
    if (i < n) {
      kk[u] = src[i];
      bb[u] = bucket_of(kk[u]);
      rr[u] = atomicAdd(&s_bk[bb[u]], 1u);
    }
  }
  __syncthreads();
  {  // exclusive scan of the counters: thread t owns buckets [t * per, (t + 1) * per)
    uint32_t c[SORT_KPT], sum = 0, mx = 0;
#pragma unroll
    for (uint32_t q = 0; q < SORT_KPT; ++q)
      if (q < per) c[q] = s_bk[tid * per + q], sum += c[q], mx = c[q] > mx ? c[q] : mx;
    if (mx > SORT_BUCKET_LIMIT) s_over = 1u;  // (same value from every writer)
    uint32_t total;
    uint32_t run = block_excl_scan<SORT_WG / 64>(sum, s_scan, &total);
#pragma unroll
    for (uint32_t q = 0; q < SORT_KPT; ++q)
      if (q < per) s_bk[tid * per + q] = run, run += c[q];
  }
  __syncthreads();
#pragma unroll
  for (uint32_t u = 0; u < SORT_KPT; ++u)
    if (tid + u * SORT_WG < n) s_keys[s_bk[bb[u]] + rr[u]] = kk[u];
  __syncthreads();
  const bool sorted = s_over == 0u;  // workgroup-uniform
  if (sorted) {
    for (uint32_t q = 0; q < per; ++q) {  // order the keys inside each of this thread's buckets
      const uint32_t b = tid * per + q, lo = s_bk[b], hi = b + 1 < n2 ? s_bk[b + 1] : n;
      for (uint32_t i = lo + 1; i < hi; ++i) {
        const uint64_t v = s_keys[i];
        uint32_t j = i;
        while (j > lo && s_keys[j - 1] > v) s_keys[j] = s_keys[j - 1], --j;
        s_keys[j] = v;
      }
    }
  } else {
    for (uint32_t i = n + tid; i < n2; i += SORT_WG) s_keys[i] = ~0ull;
  }
  __syncthreads();
  return sorted;
}

// unique: element i of the ascending list src[0..n) survives iff it differs from its predecessor; chunked keep-flag scan and
// scatter to dst by the whole workgroup.  Returns the distinct count.  IN_PLACE (dst == src): a chunk is read whole -- the
// i - 1 neighbour included -- before any of it is written, and written before the next is read; the destination index never
// exceeds the source index, so no unread element is overtaken.  Otherwise (LDS -> global memory) src is only read: the scan's
// own barriers are the only ones.
// MINC (min_count = m >= 2): the start of a run survives iff the run is at least m long -- in an ascending list, iff the element
// m - 1 places ahead equals it: one more read, ahead of the chunk.  IN_PLACE that read is safe for the reason above: every write
// of this and the earlier chunks went to an index below the running count `base` of survivors, and the elements from `base` on
// still hold what the sort left there (base <= c0 <= i, and where base == i every element so far survived and was written
// onto itself); the look-ahead only reads at i + m - 1 >= i, and the barrier between a chunk's reads and its writes covers it
// like the i - 1 read.
template <bool IN_PLACE, bool MINC = false>
__device__ __forceinline__ uint32_t unique_scatter(const uint64_t *src, const uint32_t n, uint64_t *dst, uint32_t *s_scan,
                                                   const uint32_t m = 1) {
  const uint32_t tid = threadIdx.x;
  uint32_t base = 0;
  for (uint32_t c0 = 0; c0 < n; c0 += SORT_WG) {
    const uint32_t i = c0 + tid;
    uint64_t v = 0;
    uint32_t keep = 0;
    if (i < n) {
      v = src[i];
      keep = (i == 0 || v != src[i - 1]) ? 1u : 0u;
      if constexpr (MINC) keep = (keep && m - 1 < n - i && src[i + (m - 1)] == v) ? 1u : 0u;
    }
    if (IN_PLACE) __syncthreads();
    uint32_t total;
    const uint32_t pos = block_excl_scan<SORT_WG / 64>(keep, s_scan, &total);
    if (keep) dst[base + pos] = v;
    base += total;
    if (IN_PLACE) __syncthreads();
  }
  return base;
}

// Up to 64 keys ordered and de-duplicated by ONE wave in registers (lane = the calling lane, 0..63): a 64-lane bitonic
// network over shuffles, no LDS, no barrier.  MINC: a run start survives iff the key m - 1 lanes up equals it (m > 64: none can).
template <bool MINC = false>
__device__ __forceinline__ void sort_unique_wave(uint64_t *__restrict__ region, const uint32_t n, const uint32_t lane,
                                                 uint32_t *__restrict__ nd_out, const uint32_t m = 1) {
  uint64_t key = lane < n ? region[lane] : ~0ull;  // hashes are < threshold < ~0
#pragma unroll
  for (uint32_t k = 2; k <= 64; k <<= 1)
#pragma unroll
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      const uint64_t other = ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), (int)j) << 32) |
                             (uint32_t)__shfl_xor((int)(uint32_t)key, (int)j);
      const bool lower = (lane & j) == 0, asc = (lane & k) == 0;
      const bool take_min = lower == asc;
      key = (take_min == (other < key)) ? other : key;
    }
  const uint64_t prev = ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(key >> 32), 1) << 32) | (uint32_t)__shfl_up((int)(uint32_t)key, 1);
  bool keep = lane < n && (lane == 0 || key != prev);
  if constexpr (MINC) {
    const int from = (int)((lane + m - 1) & 63u);  // (every lane takes part in the shuffle; the lanes it is meant for are picked below)
    const uint64_t ahead = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(key >> 32), from) << 32) | (uint32_t)__shfl((int)(uint32_t)key, from);
    keep = keep && m <= 64 && lane + m - 1 < n && ahead == key;
  }
  const unsigned long long kb = __ballot(keep);
  if (keep) region[__popcll(kb & ((1ull << lane) - 1ull))] = key;  // (every key was read before the first one is written)
  if (lane == 0) *nd_out = (uint32_t)__popcll(kb);
}

// The sort + unique of ONE genome by the calling workgroup (n = its stored raw hits).  USE_LDS: the keys are staged in dynamic
// LDS (lds_keys of them, then as many counters if bucket_mul != 0); otherwise the sort runs in place in the genome's hit region
// (which must have next_pow2(n) slots).  Returns early -- whole waves, or the whole workgroup -- on the paths that need no
// barrier; a caller that loops over genomes puts a barrier between them.
// MINC: only the keys that occur at least m (>= 2) times survive.  Sort first, then unique_scatter's look-ahead: a set this
// size is one workgroup's work either way, and the sort it has is the one the de-duplicating form is tuned with.
template <bool USE_LDS, bool MINC = false>
__device__ __forceinline__ void sort_unique_one(const uint32_t g, const hg_genome_meta &gm, const uint32_t n,
                                                uint64_t *__restrict__ hits, uint32_t *__restrict__ ndistinct,
                                                const uint32_t lds_keys, const uint64_t bucket_mul, const uint32_t m = 1) {
  extern __shared__ __attribute__((aligned(16))) uint64_t s_keys[];
  __shared__ uint32_t s_scan[SORT_WG / 64];
  uint64_t *region = hits + gm.hit_off;
  const uint32_t n2 = next_pow2(n);
  if (USE_LDS != (n2 <= lds_keys)) return;  // larger sets: bucketed sort (hg_launch_sort_large) or the in-place variant
  const uint32_t tid = threadIdx.x;

  if (n <= 1) {
    if (tid == 0) ndistinct[g] = (!MINC || n >= m) ? n : 0u;
    return;
  }
  uint32_t nd;
  if constexpr (USE_LDS) {
    if (n <= 64) {
      // A handful of hashes (plasmids, viral genomes, the 50 kbp genomes of bench.py's `many_small` leg: 33 hashes each): one
      // wave orders them in registers -- a 64-lane bitonic network over shuffles, no LDS, no barrier -- while the other waves
      // leave.  (Through the workgroup-wide network with its barrier per pass, 100 000 such genomes took 0.96 ms; the k-mer
      // kernel of the same batch 9.3 ms.)
      if (tid >= 64) return;  // whole waves
      sort_unique_wave<MINC>(region, n, tid, ndistinct + g, m);
      return;
    }
    if (bucket_mul != 0 && n >= (uint32_t)SORT_WG) {
      // sampled hashes are uniform below the threshold: bucket = floor(h * n2 / threshold), 0.8 keys each on average
      const uint32_t shift = (uint32_t)(__builtin_ctz(lds_keys) - __builtin_ctz(n2));
      const bool sorted = counting_sort_lds(region, n, n2, s_keys, reinterpret_cast<uint32_t *>(s_keys + lds_keys), s_scan,
                                            [=](uint64_t h) {
                                              const uint32_t b = (uint32_t)__umul64hi(h, bucket_mul) >> shift;
                                              return b < n2 ? b : n2 - 1;
                                            });
      if (!sorted) bitonic_sort(s_keys, n2, tid, SORT_WG);
    } else {
      for (uint32_t i = tid; i < n2; i += SORT_WG) s_keys[i] = (i < n) ? region[i] : ~0ull;
      __syncthreads();
      bitonic_sort(s_keys, n2, tid, SORT_WG);
    }
    nd = unique_scatter<false, MINC>(s_keys, n, region, s_scan, m);
  } else {
    for (uint32_t i = n + tid; i < n2; i += SORT_WG) region[i] = ~0ull;  // hashes are < threshold < ~0
    __syncthreads();
    bitonic_sort(region, n2, tid, SORT_WG);
    nd = unique_scatter<true, MINC>(region, n, region, s_scan, m);
  }
  if (tid == 0) ndistinct[g] = nd;
}

// The raw count n of genome g, clamped to its hit region's capacity (overflow is reported by the host from cnt[]).  In the
// sync-free step (flags != nullptr) nobody on the host looks at cnt[] before the encoders run: a genome this launch and its
// hg_launch_sort_unique_rest cannot finish is marked for them and reported through the step's flag word by the thread
// with tid == 0, and the return value is false -- the caller leaves.
__device__ __forceinline__ bool sort_step_guard(uint32_t &n, const uint32_t cap, uint32_t *__restrict__ flags, const uint32_t tid,
                                                uint32_t *__restrict__ nd_out) {
  if (flags) {
    const bool over = n > cap;
    if (over || n > SORT_LDS_MAX_KEYS) {
      if (tid == 0) atomicOr(flags, over ? HG_STEP_OVERFLOW : HG_STEP_LARGE_SET), *nd_out = HG_NHASH_PENDING;
      return false;
    }
  }
  if (n > cap) n = cap;
  return true;
}

// The kernels below come in two families with one body each: sort_unique_* / bucket_sort_kernel keep every key once
// (min_count <= 1, the reference's HashSet), min_count_* keep the keys that occur at least m >= 2 times.  The body is a
// device function with the MINC flag, so the first family compiles to what it was before the second existed.

// One workgroup per genome (of the todo list, if there is one).
template <bool USE_LDS, bool MINC>
__device__ __forceinline__ void sort_unique_body(const hg_genome_meta *__restrict__ meta, uint64_t *__restrict__ hits,
                                                 const uint32_t *__restrict__ cnt, uint32_t *__restrict__ ndistinct, uint32_t lds_keys,
                                                 const uint32_t *__restrict__ todo, uint64_t bucket_mul, uint32_t *__restrict__ flags,
                                                 const uint32_t m) {
  const uint32_t g = todo ? todo[blockIdx.x] : blockIdx.x;
  const hg_genome_meta gm = meta[g];
  uint32_t n = cnt[g];
  if (!sort_step_guard(n, gm.hit_cap, flags, threadIdx.x, ndistinct + g)) return;
  sort_unique_one<USE_LDS, MINC>(g, gm, n, hits, ndistinct, lds_keys, bucket_mul, m);
}
template <bool USE_LDS>
__global__ __launch_bounds__(SORT_WG) void sort_unique_kernel(
    const hg_genome_meta *__restrict__ meta, uint64_t *__restrict__ hits,
    const uint32_t *__restrict__ cnt, uint32_t *__restrict__ ndistinct, uint32_t lds_keys,
    const uint32_t *__restrict__ todo, uint64_t bucket_mul, uint32_t *__restrict__ flags) {
  sort_unique_body<USE_LDS, false>(meta, hits, cnt, ndistinct, lds_keys, todo, bucket_mul, flags, 1u);
}
template <bool USE_LDS>
__global__ __launch_bounds__(SORT_WG) void min_count_kernel(
    const hg_genome_meta *__restrict__ meta, uint64_t *__restrict__ hits,
    const uint32_t *__restrict__ cnt, uint32_t *__restrict__ ndistinct, uint32_t lds_keys,
    const uint32_t *__restrict__ todo, uint64_t bucket_mul, uint32_t *__restrict__ flags, uint32_t m) {
  sort_unique_body<USE_LDS, true>(meta, hits, cnt, ndistinct, lds_keys, todo, bucket_mul, flags, m);
}

// One WAVE per genome, four genomes per workgroup: the first sort launch of a batch whose genomes are EXPECTED to sample at
// most a few dozen k-mers (plasmids, viral genomes, contigs of a few kbp: 400 000 genomes of 2 kbp have 1.3 hashes each --
// there one 512-thread workgroup per genome, seven of whose eight waves leave at once, cost 0.74 ms against 2.25 ms for
// the k-mer kernel).  A genome with more than 64 raw hits is left to hg_launch_sort_unique_rest (skip_keys = 64).
template <bool MINC>
__device__ __forceinline__ void sort_unique_wave_body(const hg_genome_meta *__restrict__ meta, uint64_t *__restrict__ hits,
                                                      const uint32_t *__restrict__ cnt, uint32_t *__restrict__ ndistinct,
                                                      uint32_t n_genomes, uint32_t *__restrict__ flags, const uint32_t m) {
  const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
  if (g >= n_genomes) return;
  uint32_t n = cnt[g];
  if (!sort_step_guard(n, meta[g].hit_cap, flags, lane, ndistinct + g)) return;
  if (n > 64) return;
  if (n <= 1) {
    if (lane == 0) ndistinct[g] = (!MINC || n >= m) ? n : 0u;
    return;
  }
  sort_unique_wave<MINC>(hits + meta[g].hit_off, n, lane, ndistinct + g, m);
}
__global__ __launch_bounds__(256) void sort_unique_wave_kernel(
    const hg_genome_meta *__restrict__ meta, uint64_t *__restrict__ hits, const uint32_t *__restrict__ cnt,
    uint32_t *__restrict__ ndistinct, uint32_t n_genomes, uint32_t *__restrict__ flags) {
  sort_unique_wave_body<false>(meta, hits, cnt, ndistinct, n_genomes, flags, 1u);
}
__global__ __launch_bounds__(256) void min_count_wave_kernel(
    const hg_genome_meta *__restrict__ meta, uint64_t *__restrict__ hits, const uint32_t *__restrict__ cnt,
    uint32_t *__restrict__ ndistinct, uint32_t n_genomes, uint32_t *__restrict__ flags, uint32_t m) {
  sort_unique_wave_body<true>(meta, hits, cnt, ndistinct, n_genomes, flags, m);
}

// grid: SORT_WG genomes per workgroup.  The genomes whose raw count is in (skip_keys, lds_keys] -- what a launch of
// sort_unique_kernel with skip_keys of LDS left out -- are picked out of the counters by the workgroup itself and sorted
// one after the other (rare by construction: skip_keys is 1.125 times the expected count, or last run's largest).
template <bool MINC>
__device__ __forceinline__ void sort_unique_rest_body(const hg_genome_meta *__restrict__ meta, uint64_t *__restrict__ hits,
                                                      const uint32_t *__restrict__ cnt, uint32_t *__restrict__ ndistinct,
                                                      uint32_t n_genomes, uint32_t skip_keys, uint32_t lds_keys, uint64_t bucket_mul,
                                                      const uint32_t m) {
  __shared__ uint32_t s_list[SORT_WG], s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const uint32_t g = blockIdx.x * SORT_WG + threadIdx.x;
  if (g < n_genomes) {
    const uint32_t c = cnt[g];
    if (c > skip_keys && c <= lds_keys && c <= meta[g].hit_cap) s_list[atomicAdd(&s_n, 1u)] = g;
  }
  __syncthreads();
  const uint32_t todo = s_n;
  for (uint32_t i = 0; i < todo; ++i) {
    const uint32_t gi = s_list[i];
    const hg_genome_meta gm = meta[gi];
    sort_unique_one<true, MINC>(gi, gm, cnt[gi], hits, ndistinct, lds_keys, bucket_mul, m);
    __syncthreads();
  }
}
__global__ __launch_bounds__(SORT_WG) void sort_unique_rest_kernel(
    const hg_genome_meta *__restrict__ meta, uint64_t *__restrict__ hits, const uint32_t *__restrict__ cnt,
    uint32_t *__restrict__ ndistinct, uint32_t n_genomes, uint32_t skip_keys, uint32_t lds_keys, uint64_t bucket_mul) {
  sort_unique_rest_body<false>(meta, hits, cnt, ndistinct, n_genomes, skip_keys, lds_keys, bucket_mul, 1u);
}
__global__ __launch_bounds__(SORT_WG) void min_count_rest_kernel(
    const hg_genome_meta *__restrict__ meta, uint64_t *__restrict__ hits, const uint32_t *__restrict__ cnt,
    uint32_t *__restrict__ ndistinct, uint32_t n_genomes, uint32_t skip_keys, uint32_t lds_keys, uint64_t bucket_mul, uint32_t m) {
  sort_unique_rest_body<true>(meta, hits, cnt, ndistinct, n_genomes, skip_keys, lds_keys, bucket_mul, m);
}

__global__ __launch_bounds__(256) void sketch_finish_kernel(const uint32_t *__restrict__ ndistinct, uint32_t *__restrict__ nhash,
                                                            uint32_t n_genomes, const uint32_t *__restrict__ flags,
                                                            volatile uint32_t *h_slot, uint32_t seq) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g < n_genomes) nhash[g] = ndistinct[g];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    h_slot[0] = *flags;
    __threadfence_system();
    h_slot[1] = seq;
    __threadfence_system();
  }
}

// ---- large hash sets: bucket by value, sort + unique each bucket in LDS -----------------------------------
constexpr uint32_t BK_WG = 256;
__device__ __forceinline__ uint32_t bucket_of(uint64_t h, const hg_bucket_job &job) {
  const uint32_t b = (uint32_t)__umul64hi(h, job.mul);  // monotone in h
  return b < job.P ? b : job.P - 1;
}

// grid: key chunks.  bcount[bucket] += the chunk's keys of that bucket.  A chunk of 4 096 keys of a genome with up to
// BK_PRIV_MAX buckets counts in LDS first and adds its non-zero counters once (a global atomic per KEY on the genome's few
// counters ran at 0.38 TB/s of keys: 1.0 ms for 50 M keys); beyond that a key hits a bucket less than four times per chunk
// and goes straight to the global counter (no value returned: the waves do not wait).
constexpr uint32_t BK_PRIV_MAX = 2048, BK_KPT = HG_BUCKET_CHUNK / BK_WG;
static_assert(HG_BUCKET_CHUNK % BK_WG == 0, "whole keys per thread");
__global__ __launch_bounds__(BK_WG) void bucket_count_kernel(const hg_bucket_job *__restrict__ jobs,
                                                             const uint32_t *__restrict__ chunk_job,
                                                             const uint64_t *__restrict__ hits,
                                                             uint32_t *__restrict__ bcount) {
  __shared__ uint32_t s_h[BK_PRIV_MAX];
  const hg_bucket_job job = jobs[chunk_job[blockIdx.x]];
  const uint32_t k0 = (blockIdx.x - job.chunk_first) * HG_BUCKET_CHUNK;
  const uint32_t k1 = k0 + HG_BUCKET_CHUNK < job.n ? k0 + HG_BUCKET_CHUNK : job.n;
  if (job.P > BK_PRIV_MAX) {  // workgroup-uniform
    for (uint32_t i = k0 + threadIdx.x; i < k1; i += BK_WG)
      atomicAdd(&bcount[job.bucket_first + bucket_of(hits[job.hit_off + i], job)], 1u);
    return;
  }
  for (uint32_t b = threadIdx.x; b < job.P; b += BK_WG) s_h[b] = 0;
  __syncthreads();
  for (uint32_t i = k0 + threadIdx.x; i < k1; i += BK_WG) atomicAdd(&s_h[bucket_of(hits[job.hit_off + i], job)], 1u);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < job.P; b += BK_WG) {
    const uint32_t v = s_h[b];
    if (v) atomicAdd(&bcount[job.bucket_first + b], v);
  }
}

// grid: jobs.  out[b] = exclusive prefix of in[b] over the job's buckets; optionally the total per genome
__global__ __launch_bounds__(SORT_WG) void bucket_scan_kernel(const hg_bucket_job *__restrict__ jobs,
                                                              const uint32_t *__restrict__ in,
                                                              uint32_t *__restrict__ out,
                                                              uint32_t *__restrict__ total_per_genome) {
  __shared__ uint32_t s_scan[SORT_WG / 64];
  const hg_bucket_job job = jobs[blockIdx.x];
  uint32_t run = 0;
  for (uint32_t b0 = 0; b0 < job.P; b0 += SORT_WG) {
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t v = b < job.P ? in[job.bucket_first + b] : 0u;
    uint32_t total;
    const uint32_t pre = block_excl_scan<SORT_WG / 64>(v, s_scan, &total);
    if (b < job.P) out[job.bucket_first + b] = run + pre;
    run += total;
  }
  if (total_per_genome && threadIdx.x == 0) total_per_genome[job.genome] = run;
}

// grid: key chunks.  Every key moves to its bucket's range of the scratch buffer.  With up to BK_PRIV_MAX buckets the chunk
// ranks its keys per bucket in LDS (returning LDS atomics), reserves ONE run per non-empty bucket (a returning global atomic
// per bucket instead of per key: 2.1 -> ... ms for 50 M keys) and writes the keys, held in registers meanwhile, into the runs.
__global__ __launch_bounds__(BK_WG) void bucket_scatter_kernel(const hg_bucket_job *__restrict__ jobs,
                                                               const uint32_t *__restrict__ chunk_job,
                                                               const uint64_t *__restrict__ hits,
                                                               const uint32_t *__restrict__ bstart,
                                                               uint32_t *__restrict__ bcursor,
                                                               uint64_t *__restrict__ tmp) {
  __shared__ uint32_t s_h[BK_PRIV_MAX];
  const hg_bucket_job job = jobs[chunk_job[blockIdx.x]];
  const uint32_t k0 = (blockIdx.x - job.chunk_first) * HG_BUCKET_CHUNK;
  const uint32_t k1 = k0 + HG_BUCKET_CHUNK < job.n ? k0 + HG_BUCKET_CHUNK : job.n;
  if (job.P > BK_PRIV_MAX) {  // workgroup-uniform
    for (uint32_t i = k0 + threadIdx.x; i < k1; i += BK_WG) {
      const uint64_t h = hits[job.hit_off + i];
      const uint32_t gb = job.bucket_first + bucket_of(h, job);
      const uint32_t pos = atomicAdd(&bcursor[gb], 1u);
      tmp[job.hit_off + bstart[gb] + pos] = h;
    }
    return;
  }
  for (uint32_t b = threadIdx.x; b < job.P; b += BK_WG) s_h[b] = 0;
  __syncthreads();
  uint64_t kk[BK_KPT];
  uint32_t bb[BK_KPT], rr[BK_KPT];
#pragma unroll
  for (uint32_t u = 0; u < BK_KPT; ++u) {
    const uint32_t i = k0 + threadIdx.x + u * BK_WG;
    if (i < k1) {
      kk[u] = hits[job.hit_off + i];
      bb[u] = bucket_of(kk[u], job);
      rr[u] = atomicAdd(&s_h[bb[u]], 1u);  // rank among the chunk's keys of that bucket
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < job.P; b += BK_WG) {  // count -> where the chunk's run of bucket b starts in the scratch copy
    const uint32_t v = s_h[b], gb = job.bucket_first + b;
    if (v) s_h[b] = bstart[gb] + atomicAdd(&bcursor[gb], v);
  }
  __syncthreads();
#pragma unroll
  for (uint32_t u = 0; u < BK_KPT; ++u)
    if (k0 + threadIdx.x + u * BK_WG < k1) tmp[job.hit_off + s_h[bb[u]] + rr[u]] = kk[u];
}

// grid: buckets.  Sort + unique in LDS; the distinct keys go back to the start of the bucket's scratch range.
// A bucket with more keys than LDS holds (only possible when duplicates pile up: the map is balanced for
// distinct hashes) is first de-duplicated through an LDS hash set; if even its distinct keys do not fit the
// job is flagged and the caller sorts that genome in place instead.
// MINC: equal keys share a bucket, so a bucket sees every occurrence of its keys.  Here the order is count first, sort the
// survivors: every key goes into an LDS table of (key, occurrences) -- the hash set above with a counter per slot; the launch's
// LDS has 4 bytes of counters per key behind the keys --, the keys seen at least m times are compacted through the bucket's own
// scratch range (its raw keys are not needed again) and only those are sorted.  A read set is what this is for: at 30x coverage
// a bucket of ~800 raw keys holds ~30 genuine hashes of 20-35 copies each among ~200 singletons -- the counting sort gives up
// at 17 equal keys and the bitonic network would order all 1 024 (55 passes), the table orders ~30 (15).  The table has at
// least two slots per raw key, so it cannot overflow, up to cap_keys / 2 raw keys; from there it has cap_keys slots and takes
// up to 3/4 of that in DISTINCT keys.  Beyond: a bucket that fits LDS is sorted whole and filtered by unique_scatter's
// look-ahead (the keys are still in the scratch range), one that does not flags its job as above.
template <bool MINC>
__device__ __forceinline__ void bucket_sort_body(const hg_bucket_job *__restrict__ jobs, const uint32_t *__restrict__ bucket_job,
                                                 const uint32_t *__restrict__ bcount, const uint32_t *__restrict__ bstart,
                                                 uint64_t *__restrict__ tmp, uint32_t *__restrict__ bdist,
                                                 uint32_t *__restrict__ fail, const uint32_t cap_keys, const uint32_t m) {
  // cap_keys (a power of two, <= SORT_LDS_MAX_KEYS): keys the launch's LDS holds -- 12 bytes each, keys + counters.  The
  // launcher sizes it to four times the bucket size the plan aims at: 48 KiB for 512-1 024 expected keys, three workgroups
  // per CU (with the full 96 KiB in every launch one workgroup per CU sorted 1 500 keys at a time).
  extern __shared__ __attribute__((aligned(16))) uint64_t s_keys[];
  __shared__ uint32_t s_scan[SORT_WG / 64];
  __shared__ uint32_t s_distinct;
  [[maybe_unused]] __shared__ uint32_t s_kept;
  [[maybe_unused]] uint32_t *const s_occ = reinterpret_cast<uint32_t *>(s_keys + cap_keys);  // MINC: occurrences of the key in slot i
  const uint32_t gb = blockIdx.x, j = bucket_job[gb], tid = threadIdx.x;
  const hg_bucket_job job = jobs[j];
  const uint32_t n = bcount[gb];
  uint64_t *base = tmp + job.hit_off + bstart[gb];
  if (n == 0) {
    if (tid == 0) bdist[gb] = 0;
    return;
  }
  if (MINC || n > cap_keys) {
    uint32_t HSET_SLOTS = cap_keys;  // (a power of two)
    if constexpr (MINC)
      if (n <= cap_keys / 2) HSET_SLOTS = n <= 32 ? 64u : 2 * next_pow2(n);
    const uint32_t HSET_MAX = HSET_SLOTS / 4 * 3;
    for (uint32_t i = tid; i < HSET_SLOTS; i += SORT_WG) s_keys[i] = ~0ull;  // no hash equals ~0 (h < threshold)
    if (tid == 0) s_distinct = 0;
    if constexpr (MINC) {
      for (uint32_t i = tid; i < HSET_SLOTS; i += SORT_WG) s_occ[i] = 0;
      if (tid == 0) s_kept = 0;
    }
    __syncthreads();
    for (uint32_t i = tid; i < n; i += SORT_WG) {
      const uint64_t h = base[i];
      uint32_t slot = (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> 40) & (HSET_SLOTS - 1);
      for (;;) {
        if (s_distinct > HSET_MAX) break;  // hopeless: flagged below
        const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long *>(&s_keys[slot]), ~0ull, (unsigned long long)h);
        if (old == ~0ull) {
          atomicAdd(&s_distinct, 1u);
          if constexpr (MINC) atomicAdd(&s_occ[slot], 1u);
          break;
        }
        if (old == h) {
          if constexpr (MINC) atomicAdd(&s_occ[slot], 1u);
          break;
        }
        slot = (slot + 1) & (HSET_SLOTS - 1);
      }
    }
    __syncthreads();
    const bool overflow = s_distinct > HSET_MAX;  // workgroup-uniform
    if (overflow && n > cap_keys) {
      if (tid == 0) fail[j] = 1u, bdist[gb] = 0;
      return;
    }
    if constexpr (!MINC) {
      bitonic_sort(s_keys, HSET_SLOTS, tid, SORT_WG);  // empty slots (~0) sort to the end
      const uint32_t d = s_distinct;
      for (uint32_t i = tid; i < d; i += SORT_WG) base[i] = s_keys[i];
      if (tid == 0) bdist[gb] = d;
      return;
    } else if (!overflow) {  // (the table is complete: nobody gave up above)
      for (uint32_t i = tid; i < HSET_SLOTS; i += SORT_WG)
        if (s_keys[i] != ~0ull && s_occ[i] >= m) base[atomicAdd(&s_kept, 1u)] = s_keys[i];  // (kept <= distinct <= n: inside the bucket's range)
      __syncthreads();  // (orders the workgroup's global writes before its reads below, too)
      const uint32_t d = s_kept, d2 = next_pow2(d);
      for (uint32_t i = tid; i < d2; i += SORT_WG) s_keys[i] = i < d ? base[i] : ~0ull;
      __syncthreads();
      bitonic_sort(s_keys, d2, tid, SORT_WG);
      for (uint32_t i = tid; i < d; i += SORT_WG) base[i] = s_keys[i];
      if (tid == 0) bdist[gb] = d;
      return;
    }
    __syncthreads();  // MINC, more distinct keys than the table takes, but the bucket fits LDS: everyone has read s_distinct
  }
  const uint32_t n2 = next_pow2(n);
  bool sorted = false;  // workgroup-uniform
  if (n2 >= (uint32_t)SORT_WG) {
    // The bucket's keys are uniform over its value range: the counting sort one level down -- sub-bucket = the top bits of the
    // FRACTION of h * mul (its integer part is the bucket; the fraction grows with h inside it).  Keys the bucket map clamped
    // into the last bucket -- integer part >= P -- have no usable fraction: last sub-bucket.
    const uint32_t shift = 64u - (uint32_t)__builtin_ctz(n2);
    sorted = counting_sort_lds(base, n, n2, s_keys, reinterpret_cast<uint32_t *>(s_keys + cap_keys), s_scan, [=](uint64_t h) {
      return (uint32_t)__umul64hi(h, job.mul) >= job.P ? n2 - 1 : (uint32_t)((h * job.mul) >> shift);
    });
  } else {
    for (uint32_t i = tid; i < n2; i += SORT_WG) s_keys[i] = (i < n) ? base[i] : ~0ull;
    __syncthreads();
  }
  if (!sorted) bitonic_sort(s_keys, n2, tid, SORT_WG);
  const uint32_t run = unique_scatter<false, MINC>(s_keys, n, base, s_scan, m);
  if (tid == 0) bdist[gb] = run;
}
__global__ __launch_bounds__(SORT_WG) void bucket_sort_kernel(const hg_bucket_job *__restrict__ jobs,
                                                              const uint32_t *__restrict__ bucket_job,
                                                              const uint32_t *__restrict__ bcount,
                                                              const uint32_t *__restrict__ bstart,
                                                              uint64_t *__restrict__ tmp,
                                                              uint32_t *__restrict__ bdist,
                                                              uint32_t *__restrict__ fail, uint32_t cap_keys) {
  bucket_sort_body<false>(jobs, bucket_job, bcount, bstart, tmp, bdist, fail, cap_keys, 1u);
}
__global__ __launch_bounds__(SORT_WG) void min_count_bucket_kernel(const hg_bucket_job *__restrict__ jobs,
                                                                   const uint32_t *__restrict__ bucket_job,
                                                                   const uint32_t *__restrict__ bcount,
                                                                   const uint32_t *__restrict__ bstart,
                                                                   uint64_t *__restrict__ tmp,
                                                                   uint32_t *__restrict__ bdist,
                                                                   uint32_t *__restrict__ fail, uint32_t cap_keys, uint32_t m) {
  bucket_sort_body<true>(jobs, bucket_job, bcount, bstart, tmp, bdist, fail, cap_keys, m);
}

// grid: buckets.  Distinct keys of the bucket -> their final place in the genome's hit region.
__global__ __launch_bounds__(BK_WG) void bucket_copy_kernel(const hg_bucket_job *__restrict__ jobs,
                                                            const uint32_t *__restrict__ bucket_job,
                                                            const uint32_t *__restrict__ bstart,
                                                            const uint32_t *__restrict__ bdist,
                                                            const uint32_t *__restrict__ bout,
                                                            const uint32_t *__restrict__ fail,
                                                            const uint64_t *__restrict__ tmp,
                                                            uint64_t *__restrict__ hits) {
  const uint32_t gb = blockIdx.x;
  if (fail[bucket_job[gb]]) return;  // the genome's raw keys must survive for the in-place sort
  const hg_bucket_job job = jobs[bucket_job[gb]];
  const uint64_t *src = tmp + job.hit_off + bstart[gb];
  uint64_t *dst = hits + job.hit_off + bout[gb];
  for (uint32_t i = threadIdx.x; i < bdist[gb]; i += BK_WG) dst[i] = src[i];
}

}  // namespace

static hipError_t sort_lds_attr() {
  static std::atomic<uint64_t> done{0};
  if (attr_done_on_this_device(done, false)) return hipSuccess;
  // (keys + the counting sort's counters)
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&sort_unique_kernel<true>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, SORT_LDS_BYTES_MAX);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&bucket_sort_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, SORT_LDS_BYTES_MAX);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&sort_unique_rest_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, SORT_LDS_BYTES_MAX);
  for (const void *f : {reinterpret_cast<const void *>(&min_count_kernel<true>), reinterpret_cast<const void *>(&min_count_bucket_kernel),
                        reinterpret_cast<const void *>(&min_count_rest_kernel)})
    if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, SORT_LDS_BYTES_MAX);
  if (e == hipSuccess) attr_done_on_this_device(done, true);
  return e;
}

uint32_t hg_sort_lds_keys(uint32_t max_cap) {
  uint32_t keys = 1;
  while (keys < max_cap && keys < SORT_LDS_MAX_KEYS) keys <<= 1;
  return keys;
}

// What a launch of the LDS sort for hit regions of up to max_cap keys needs: the keys the LDS holds, the counting sort's
// bucket_mul for hashes below `threshold` and that many buckets -- ceil(keys * 2^64 / threshold); 0 without a threshold: no
// counting sort --, and the dynamic LDS: the keys, and the bucket counters where the counting sort applies.
struct sort_lds_plan {
  uint32_t keys;
  uint64_t bucket_mul;
  size_t lds_bytes;
  hipError_t err;  // of sort_lds_attr()
};
static sort_lds_plan sort_lds_plan_for(uint32_t max_cap, uint64_t threshold) {
  sort_lds_plan p;
  p.keys = hg_sort_lds_keys(max_cap);
  p.bucket_mul = 0;
  if (threshold != 0) {
    const unsigned __int128 q = (((unsigned __int128)p.keys << 64) + threshold - 1) / threshold;
    p.bucket_mul = q > (unsigned __int128)UINT64_MAX ? UINT64_MAX : (uint64_t)q;
  }
  p.lds_bytes = (size_t)p.keys * (sizeof(uint64_t) + (p.bucket_mul ? sizeof(uint32_t) : 0));
  p.err = sort_lds_attr();
  return p;
}

hipError_t hg_launch_sort_unique_todo(hipStream_t st, const hg_genome_meta *d_meta, const uint32_t *d_todo, uint32_t n_todo,
                                      uint64_t *d_hits, const uint32_t *d_cnt, uint32_t *d_ndistinct, uint32_t max_cap,
                                      uint64_t threshold, uint32_t min_count, std::string *launched) {
  if (n_todo == 0) return hipSuccess;
  const sort_lds_plan p = sort_lds_plan_for(max_cap, threshold);
  if (p.err != hipSuccess) return p.err;
  if (min_count > 1) {
    hipLaunchKernelGGL((min_count_kernel<true>), dim3(n_todo), dim3(SORT_WG), p.lds_bytes, st, d_meta, d_hits, d_cnt, d_ndistinct,
                       p.keys, d_todo, p.bucket_mul, (uint32_t *)nullptr, min_count);
    hg_note_launch(launched, "min_count_kernel<true>");
    return hipGetLastError();
  }
  hipLaunchKernelGGL((sort_unique_kernel<true>), dim3(n_todo), dim3(SORT_WG), p.lds_bytes, st, d_meta, d_hits, d_cnt, d_ndistinct,
                     p.keys, d_todo, p.bucket_mul, (uint32_t *)nullptr);
  hg_note_launch(launched, "sort_unique_kernel<true>");
  return hipGetLastError();
}

hipError_t hg_launch_sort_unique(hipStream_t st, const hg_genome_meta *d_meta, uint32_t n_genomes,
                                 uint64_t *d_hits, const uint32_t *d_cnt, uint32_t *d_ndistinct,
                                 uint32_t max_cap, uint64_t threshold, uint32_t min_count, uint32_t *d_flags,
                                 std::string *launched) {
  if (n_genomes == 0) return hipSuccess;
  const sort_lds_plan p = sort_lds_plan_for(max_cap, threshold);
  if (p.err != hipSuccess) return p.err;
  if (min_count > 1) {  // the same two launches, of the min_count family
    if (p.keys <= 64) {
      hipLaunchKernelGGL(min_count_wave_kernel, dim3((n_genomes + 3) / 4), dim3(256), 0, st, d_meta, d_hits, d_cnt, d_ndistinct,
                         n_genomes, d_flags, min_count);
      hg_note_launch(launched, "min_count_wave_kernel");
      return hipGetLastError();
    }
    hipLaunchKernelGGL((min_count_kernel<true>), dim3(n_genomes), dim3(SORT_WG), p.lds_bytes, st, d_meta, d_hits, d_cnt,
                       d_ndistinct, p.keys, (const uint32_t *)nullptr, p.bucket_mul, d_flags, min_count);
    hg_note_launch(launched, "min_count_kernel<true>");
    return hipGetLastError();
  }
  if (p.keys <= 64) {  // tiny sets: a wave per genome
    hipLaunchKernelGGL(sort_unique_wave_kernel, dim3((n_genomes + 3) / 4), dim3(256), 0, st, d_meta, d_hits, d_cnt, d_ndistinct,
                       n_genomes, d_flags);
    hg_note_launch(launched, "sort_unique_wave_kernel");
    return hipGetLastError();
  }
  // genomes whose hit count exceeds the LDS budget are skipped here: the caller learns the counts and
  // runs hg_launch_sort_large / hg_launch_sort_inplace for them (or, with d_flags, reads the step's flag word)
  hipLaunchKernelGGL((sort_unique_kernel<true>), dim3(n_genomes), dim3(SORT_WG), p.lds_bytes, st, d_meta,
                     d_hits, d_cnt, d_ndistinct, p.keys, (const uint32_t *)nullptr, p.bucket_mul, d_flags);
  hg_note_launch(launched, "sort_unique_kernel<true>");
  return hipGetLastError();
}

hipError_t hg_launch_sort_unique_rest(hipStream_t st, const hg_genome_meta *d_meta, uint32_t n_genomes, uint64_t *d_hits,
                                      const uint32_t *d_cnt, uint32_t *d_ndistinct, uint32_t done_cap, uint32_t max_cap,
                                      uint64_t threshold, uint32_t min_count, std::string *launched) {
  const uint32_t skip = hg_sort_lds_keys(done_cap);
  if (n_genomes == 0 || skip >= hg_sort_lds_keys(max_cap)) return hipSuccess;
  const sort_lds_plan p = sort_lds_plan_for(max_cap, threshold);
  if (p.err != hipSuccess) return p.err;
  if (min_count > 1) {
    hipLaunchKernelGGL(min_count_rest_kernel, dim3((n_genomes + SORT_WG - 1) / SORT_WG), dim3(SORT_WG), p.lds_bytes, st, d_meta,
                       d_hits, d_cnt, d_ndistinct, n_genomes, skip, p.keys, p.bucket_mul, min_count);
    hg_note_launch(launched, "min_count_rest_kernel");
    return hipGetLastError();
  }
  hipLaunchKernelGGL(sort_unique_rest_kernel, dim3((n_genomes + SORT_WG - 1) / SORT_WG), dim3(SORT_WG), p.lds_bytes, st, d_meta,
                     d_hits, d_cnt, d_ndistinct, n_genomes, skip, p.keys, p.bucket_mul);
  hg_note_launch(launched, "sort_unique_rest_kernel");
  return hipGetLastError();
}

hipError_t hg_launch_sketch_finish(hipStream_t st, const uint32_t *d_ndistinct, uint32_t *d_nhash, uint32_t n_genomes,
                                   const uint32_t *d_flags, uint32_t *h_slot, uint32_t seq, std::string *launched) {
  hipLaunchKernelGGL(sketch_finish_kernel, dim3((n_genomes + 255) / 256), dim3(256), 0, st, d_ndistinct, d_nhash, n_genomes,
                     d_flags, h_slot, seq);
  hg_note_launch(launched, "sketch_finish_kernel");
  return hipGetLastError();
}

hipError_t hg_launch_sort_inplace(hipStream_t st, const hg_genome_meta *d_meta, const uint32_t *d_todo,
                                  uint32_t n_todo, uint64_t *d_hits, const uint32_t *d_cnt, uint32_t *d_ndistinct,
                                  uint32_t min_count, std::string *launched) {
  if (n_todo == 0) return hipSuccess;
  if (min_count > 1) {
    hipLaunchKernelGGL((min_count_kernel<false>), dim3(n_todo), dim3(SORT_WG), 0, st, d_meta, d_hits, d_cnt,
                       d_ndistinct, SORT_LDS_MAX_KEYS, d_todo, (uint64_t)0, (uint32_t *)nullptr, min_count);
    hg_note_launch(launched, "min_count_kernel<false>");
    return hipGetLastError();
  }
  hipLaunchKernelGGL((sort_unique_kernel<false>), dim3(n_todo), dim3(SORT_WG), 0, st, d_meta, d_hits, d_cnt,
                     d_ndistinct, SORT_LDS_MAX_KEYS, d_todo, (uint64_t)0, (uint32_t *)nullptr);
  hg_note_launch(launched, "sort_unique_kernel<false>");
  return hipGetLastError();
}

hipError_t hg_launch_sort_large(hipStream_t st, const hg_bucket_job *d_jobs, uint32_t n_jobs,
                                const uint32_t *d_chunk_job, uint32_t n_chunks, const uint32_t *d_bucket_job,
                                uint32_t n_buckets, uint32_t *d_bk, uint64_t *d_hits, uint64_t *d_tmp,
                                uint32_t *d_ndistinct, uint32_t bucket_cap_keys, uint32_t min_count, std::string *launched) {
  if (n_jobs == 0) return hipSuccess;
  uint32_t cap_keys = (uint32_t)SORT_WG;  // (a power of two: the counting sort deals n2 / SORT_WG sub-buckets to a thread)
  while (cap_keys < bucket_cap_keys && cap_keys < SORT_LDS_MAX_KEYS) cap_keys <<= 1;
  hipError_t e = sort_lds_attr();
  if (e != hipSuccess) return e;
  uint32_t *bcount = d_bk, *bstart = d_bk + n_buckets, *bcursor = d_bk + 2 * (size_t)n_buckets;
  uint32_t *bdist = d_bk + 3 * (size_t)n_buckets, *bout = d_bk + 4 * (size_t)n_buckets, *fail = d_bk + 5 * (size_t)n_buckets;
  if ((e = hipMemsetAsync(d_bk, 0, (5 * (size_t)n_buckets + n_jobs) * sizeof(uint32_t), st)) != hipSuccess) return e;
  hipLaunchKernelGGL(bucket_count_kernel, dim3(n_chunks), dim3(BK_WG), 0, st, d_jobs, d_chunk_job, d_hits, bcount);
  hipLaunchKernelGGL(bucket_scan_kernel, dim3(n_jobs), dim3(SORT_WG), 0, st, d_jobs, bcount, bstart, (uint32_t *)nullptr);
  hipLaunchKernelGGL(bucket_scatter_kernel, dim3(n_chunks), dim3(BK_WG), 0, st, d_jobs, d_chunk_job, d_hits, bstart,
                     bcursor, d_tmp);
  // (only the per-bucket kernel knows about min_count: the buckets before it hold raw keys, the scan and copy behind it survivors)
  const size_t bucket_lds = (size_t)cap_keys * (sizeof(uint64_t) + sizeof(uint32_t));
  if (min_count > 1)
    hipLaunchKernelGGL(min_count_bucket_kernel, dim3(n_buckets), dim3(SORT_WG), bucket_lds, st, d_jobs, d_bucket_job, bcount, bstart,
                       d_tmp, bdist, fail, cap_keys, min_count);
  else
    hipLaunchKernelGGL(bucket_sort_kernel, dim3(n_buckets), dim3(SORT_WG), bucket_lds, st, d_jobs, d_bucket_job, bcount, bstart, d_tmp,
                       bdist, fail, cap_keys);
  hipLaunchKernelGGL(bucket_scan_kernel, dim3(n_jobs), dim3(SORT_WG), 0, st, d_jobs, bdist, bout, d_ndistinct);
  hipLaunchKernelGGL(bucket_copy_kernel, dim3(n_buckets), dim3(BK_WG), 0, st, d_jobs, d_bucket_job, bstart, bdist, bout,
                     fail, d_tmp, d_hits);
  for (const char *k : {"bucket_count_kernel", "bucket_scan_kernel", "bucket_scatter_kernel",
                        min_count > 1 ? "min_count_bucket_kernel" : "bucket_sort_kernel", "bucket_scan_kernel", "bucket_copy_kernel"})
    hg_note_launch(launched, k);
  return hipGetLastError();
}
