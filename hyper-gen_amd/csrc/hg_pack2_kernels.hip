// hg_pack2_kernels.hip -- hg_pack2 blobs on the device: ASCII -> blob (hg_pack2_batch_dev), blob -> ASCII (hg_unpack2_dev), and
// the streaming sketcher's two job-table kernels: a chunk's blobs -> ASCII, hg_pack2s genomes' bitmaps from their run tables.
#include "hg_internal.h"

namespace {
// the job a workgroup of a job-table kernel works on: the last one whose first block is <= blockIdx.x
template <class Job>
__device__ __forceinline__ Job job_of_block(const Job *__restrict__ jobs, uint32_t n_jobs) {
  uint32_t lo = 0, hi = n_jobs;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (jobs[mid].first_block <= blockIdx.x) lo = mid;
    else hi = mid;
  }
  return jobs[lo];
}

// 16 bases per step: 4 code bytes -> 16 ASCII bytes through a v_perm table ("ACGT"), non-bases -> 'N'
__device__ __forceinline__ void unpack2_group(const uint8_t *__restrict__ blob, const uint8_t *__restrict__ mask, uint8_t *__restrict__ out,
                                              uint64_t grp) {
  const uint32_t codes = *reinterpret_cast<const uint32_t *>(blob + 4 * grp);
  const uint32_t bad = *reinterpret_cast<const uint16_t *>(mask + 2 * grp);
  uint32_t w[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint32_t c = (codes >> (8 * b)) & 0xFFu;
    const uint32_t sel = (c & 3u) | ((c & 0xCu) << 6) | ((c & 0x30u) << 12) | ((c & 0xC0u) << 18);  // 2-bit fields -> bytes
    const uint32_t ascii = __builtin_amdgcn_perm(0u, 0x54474341u, sel);  // selector 0..3 -> 'A','C','G','T'
    const uint32_t m = ((((bad >> (4 * b)) & 0xFu) * 0x00204081u) & 0x01010101u) * 0xFFu;  // mask bits -> byte masks
    w[b] = (ascii & ~m) | (0x4E4E4E4Eu & m);
  }
  *reinterpret_cast<uint4 *>(out + 16 * grp) = make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(256) void unpack2_kernel(const uint8_t *__restrict__ pk, uint8_t *__restrict__ out,
                                                      const UnpackJob *__restrict__ jobs, uint32_t n_jobs) {
  const UnpackJob jb = job_of_block(jobs, n_jobs);
  const uint64_t groups = (jb.n_bps + 15) / 16;
  const uint64_t g0 = (uint64_t)(blockIdx.x - jb.first_block) * UNPACK_GROUPS_PER_BLOCK + threadIdx.x;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint64_t g = g0 + 256u * r;
    if (g < groups) unpack2_group(pk + jb.pk_off, pk + jb.mask_off, out + jb.out_off, g);
  }
}

// hg_pack2s genomes: the not-a-base bitmap of the hg_pack2 layout rebuilt from the run table that came over the link.
// One workgroup per 4 KiB slice of a genome's bitmap: zeroed in LDS, the runs that overlap it OR-ed in, written out
// once -- the chunk's memory is reused, so every word is written whether it has a bit or not.
__global__ __launch_bounds__(256) void expand_runs_kernel(uint8_t *__restrict__ pk, const SparseJob *__restrict__ jobs, uint32_t n_jobs) {
  __shared__ uint32_t s_bits[SLICE_WORDS];
  const SparseJob jb = job_of_block(jobs, n_jobs);
  const uint64_t cb = hg_pack2_code_bytes(jb.n_bps), words = hg_pack2_mask_bytes(jb.n_bps) / 4;
  const uint64_t w0 = (uint64_t)(blockIdx.x - jb.first_block) * SLICE_WORDS;
  if (w0 >= words) return;
  const uint32_t nw = (uint32_t)(words - w0 < SLICE_WORDS ? words - w0 : SLICE_WORDS);
  for (uint32_t i = threadIdx.x; i < nw; i += 256) s_bits[i] = 0u;
  __syncthreads();
  const uint32_t *__restrict__ tab = reinterpret_cast<const uint32_t *>(pk + jb.codes_off + cb);
  const uint32_t n_runs = tab[0];
  const uint64_t b0 = 32 * w0, b1 = b0 + 32ull * nw;
  uint32_t a = 0, z = n_runs;  // first run that ends behind b0 (runs are sorted and disjoint)
  while (a < z) {
    const uint32_t mid = (a + z) >> 1;
    if ((uint64_t)tab[2 + 2 * mid] + tab[3 + 2 * mid] > b0) z = mid;
    else a = mid + 1;
  }
  for (uint32_t r = a; r < n_runs; ++r) {  // uniform: a slice sees a handful of runs
    const uint64_t st = tab[2 + 2 * r], en = st + tab[3 + 2 * r];
    if (st >= b1) break;
    const uint64_t s_ = st > b0 ? st : b0, e_ = en < b1 ? en : b1;  // e_ > s_
    const uint32_t fw = (uint32_t)((s_ - b0) >> 5), lw = (uint32_t)((e_ - 1 - b0) >> 5);
    for (uint32_t w = fw + threadIdx.x; w <= lw; w += 256) {
      uint32_t m = ~0u;
      if (w == fw) m &= ~0u << (uint32_t)(s_ & 31);
      if (w == lw) m &= ~0u >> (31u - (uint32_t)((e_ - 1) & 31));
      atomicOr(&s_bits[w], m);
    }
  }
  __syncthreads();
  uint32_t *__restrict__ dst = reinterpret_cast<uint32_t *>(pk + jb.mask_off) + w0;
  for (uint32_t i = threadIdx.x; i < nw; i += 256) dst[i] = s_bits[i];
}

// ASCII -> hg_pack2 blob, 32 bases per lane (8 code bytes + 4 bitmap bytes), bit-identical to the host's hg_pack2
// (hg_formats.cpp): A,C,G,T = 0..3 in either case (+ u/U -> T under u2t), anything else code 0 + its not-a-base bit;
// the paddings of both areas (to 16 bytes) and everything behind the last base are zero.  tab: {seq_off, n_bps, blob_off}
// per genome; blockIdx.y = genome.
__global__ __launch_bounds__(256) void pack2_kernel(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ tab,
                                                    uint32_t u2t, uint8_t *__restrict__ blobs) {
  const uint64_t seq_off = tab[3 * blockIdx.y], n = tab[3 * blockIdx.y + 1], blob_off = tab[3 * blockIdx.y + 2];
  const uint64_t cb = hg_pack2_code_bytes(n), mb = hg_pack2_mask_bytes(n);
  const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x, i0 = 32 * q;
  if (4 * q >= mb) return;  // (the bitmap's padding reaches further than the codes')
  const uint8_t *__restrict__ src = seq + seq_off;
  uint32_t x[8];
  if (i0 + 32 <= n) {
    const uint32_t *s4 = reinterpret_cast<const uint32_t *>(src + i0);  // seq_off is a multiple of 4
#pragma unroll
    for (int t = 0; t < 8; ++t) x[t] = s4[t];
  } else {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      uint32_t w = 0;
      for (int b = 0; b < 4; ++b) {
        const uint64_t i = i0 + 4 * t + b;
        w |= (uint32_t)(i < n ? src[i] : (uint8_t)0) << (8 * b);
      }
      x[t] = w;
    }
  }
  uint32_t codes[2] = {0u, 0u}, bad = 0u;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    uint32_t xv = x[t];
    if (u2t) {  // u/U -> T ('U' ^ 'T' == 1)
      const uint32_t e = (xv & 0xDFDFDFDFu) ^ 0x55555555u;
      const uint32_t nz = ((e & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | e;  // bit 7 set <=> byte != 'U'
      xv ^= (~nz & 0x80808080u) >> 7;
    }
    const uint32_t tt = xv ^ (xv >> 1);
    uint32_t cd = (tt >> 1) & 0x03030303u;
    const uint32_t d = (xv & 0xDFDFDFDFu) ^ __builtin_amdgcn_perm(0u, 0x54474341u, cd);
    const uint32_t z = ((((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u) >> 7;  // 1 per byte that is not a base
    cd &= ~(z * 0xFFu);
    codes[t >> 2] |= ((cd | (cd >> 6) | (cd >> 12) | (cd >> 18)) & 0xFFu) << (8 * (t & 3));
    uint32_t nb = ((z * 0x01020408u) >> 24) & 0xFu;
    // positions at or behind the end are not flagged (the host leaves those bits zero)
    const uint64_t p0 = i0 + 4 * t;
    if (p0 + 4 > n) nb &= p0 >= n ? 0u : ((1u << (uint32_t)(n - p0)) - 1u);
    bad |= nb << (4 * t);
  }
  uint8_t *blob = blobs + blob_off;
  if (8 * q < cb) *reinterpret_cast<uint2 *>(blob + 8 * q) = make_uint2(codes[0], codes[1]);
  *reinterpret_cast<uint32_t *>(blob + cb + 4 * q) = bad;
}

__global__ __launch_bounds__(256) void unpack2_one_kernel(const uint8_t *__restrict__ blob, uint8_t *__restrict__ out, uint64_t n_bps) {
  const uint64_t groups = (n_bps + 15) / 16;
  const size_t code_bytes = hg_pack2_code_bytes(n_bps);
  const uint64_t g0 = (uint64_t)blockIdx.x * UNPACK_GROUPS_PER_BLOCK + threadIdx.x;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint64_t g = g0 + 256u * r;
    if (g < groups) unpack2_group(blob, blob + code_bytes, out, g);
  }
}
}  // namespace

hipError_t hg_launch_pack2(hipStream_t st, const uint8_t *d_seq, const uint64_t *d_tab, uint32_t n, uint32_t blocks_max,
                           uint32_t u2t, uint8_t *d_blobs) {
  for (uint32_t g0 = 0; g0 < n; g0 += 65535) {
    const uint32_t m = std::min<uint32_t>(65535u, n - g0);
    hipLaunchKernelGGL(pack2_kernel, dim3(blocks_max, m), dim3(256), 0, st, d_seq, d_tab + 3 * (size_t)g0, u2t, d_blobs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t hg_launch_unpack2_jobs(hipStream_t st, const uint8_t *d_pk, uint8_t *d_out, const UnpackJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks) {
  hipLaunchKernelGGL(unpack2_kernel, dim3(n_blocks), dim3(256), 0, st, d_pk, d_out, d_jobs, n_jobs);
  return hipGetLastError();
}

hipError_t hg_launch_expand_runs(hipStream_t st, uint8_t *d_pk, const SparseJob *d_jobs, uint32_t n_jobs, uint32_t n_blocks) {
  hipLaunchKernelGGL(expand_runs_kernel, dim3(n_blocks), dim3(256), 0, st, d_pk, d_jobs, n_jobs);
  return hipGetLastError();
}

extern "C" hg_status hg_unpack2_dev(hg_ctx *c, const uint8_t *d_blob, size_t n_bps, uint8_t *d_seq_out) {
  if (!c) return HG_ERR_INVALID;
  if (n_bps == 0) return HG_OK;
  if (!d_blob || !d_seq_out) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (((uintptr_t)d_blob | (uintptr_t)d_seq_out) & 15) return hg_fail(c, HG_ERR_INVALID, "hg_unpack2_dev: pointers must be 16-byte aligned");
  HG_ENTER(c);
  hipLaunchKernelGGL(unpack2_one_kernel, dim3(hg_unpack2_blocks(n_bps)), dim3(256), 0, c->stream, d_blob, d_seq_out, (uint64_t)n_bps);
  HG_HIP(c, hipGetLastError());
  return HG_OK;
}
