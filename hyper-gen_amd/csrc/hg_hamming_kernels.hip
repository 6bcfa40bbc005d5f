// hg_hamming_kernels.hip -- bit-packed hypervectors and XOR/popcount Hamming search on gfx950.
//
// Extension named by BASELINE.json configs[4] (D = 16384 sign-binarised HVs, database search); the
// reference has no such path, so the semantics are this repository's: bit d = (hv[d] >= 0), uint32
// word w holds dims 32w..32w+31 LSB first, distance = popcount(xor).  The CPU definition the tests
// compare with, bit for bit, lives with the test infrastructure.
//
// The search is HBM/L2 + VALU work (v_xor_b32 + v_bcnt_u32_b32 per 32 dims and pair), not a GEMM: a
// 128 x 128 tile of pairs per workgroup, 8 x 8 pairs per lane in registers, operand slices of 32
// words staged through LDS with padded rows (conflict-free ds_read_b128).
#include <algorithm>

#include "hg_internal.h"

namespace {

__global__ __launch_bounds__(256) void binarize_kernel(const int16_t *__restrict__ hv, uint32_t hv_d,
                                                       uint32_t words, uint32_t *__restrict__ bits) {
  const uint32_t g = blockIdx.y;
  const int16_t *__restrict__ src = hv + (size_t)g * hv_d;
  // one lane per dimension, one ballot per 64 dims -> two words
  for (uint32_t d0 = blockIdx.x * blockDim.x; d0 < words * 32; d0 += gridDim.x * blockDim.x) {
    const uint32_t d = d0 + threadIdx.x;
    const bool b = d < hv_d && src[d] >= 0;
    const unsigned long long m = __ballot(b);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = d >> 5;
    if (lane == 0 && w < words) bits[(size_t)g * words + w] = (uint32_t)m;
    if (lane == 32 && w < words) bits[(size_t)g * words + w] = (uint32_t)(m >> 32);
  }
}

constexpr int HT = 128;          // tile edge (pairs)
constexpr int HK = 32;           // words per K slice
constexpr int HROW = HK + 4;     // padded LDS row (words): 144 B, conflict-free ds_read_b128

struct HamArgs {
  const uint32_t *ref, *qry;
  uint32_t R, Q, words;
  uint32_t *dist_out;   // full matrix or nullptr
  hg_ham_hit *hits;
  uint32_t *hit_count;
  uint32_t hit_cap, max_dist;
  uint32_t ref_off, qry_off;  // global index of row 0 / column 0 (a shard of a larger database)
};

// JN: query columns per lane -- the tile is HT reference rows x 16 JN queries.  8 = the square tile; 2 and 1 serve searches
// with up to 32 / 16 queries (a handful of genomes against a large database: with the square tile 1 000 000 x 10 did the
// xor + popcount work of 128 query columns, 3.5 ms where the reference bits alone stream in 0.3).
template <int JN>
__global__ __launch_bounds__(256) void hamming_kernel(HamArgs a) {
  constexpr int HQ = 16 * JN;  // query columns of a tile
  __shared__ __attribute__((aligned(16))) uint32_t sAB[2 * HT * HROW];
  uint32_t *sA = sAB, *sB = sAB + HT * HROW;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t tx = tid & 15, ty = tid >> 4;  // 16 x 16 lanes, lane (ty,tx) owns rows ty+16i, cols tx+16j
  const uint32_t row0 = blockIdx.y * HT, col0 = blockIdx.x * HQ;
  uint32_t acc[8][JN];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j) acc[i][j] = 0;

  // staging: 128 rows x 32 words = 1024 pieces of 16 B per operand -> 4 per thread
  const uint32_t srow = tid >> 3, spc = tid & 7;
  for (uint32_t k0 = 0; k0 < a.words; k0 += HK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t r = srow + 32 * i, w = k0 + spc * 4;
      uint4 va = make_uint4(0, 0, 0, 0), vb = make_uint4(0, 0, 0, 0);
      if (row0 + r < a.R) {
        const uint32_t *p = a.ref + (size_t)(row0 + r) * a.words + w;
        if (w + 4 <= a.words) va = *reinterpret_cast<const uint4 *>(p);
        else {
          if (w < a.words) va.x = p[0];
          if (w + 1 < a.words) va.y = p[1];
          if (w + 2 < a.words) va.z = p[2];
        }
      }
      if (r < (uint32_t)HQ && col0 + r < a.Q) {
        const uint32_t *p = a.qry + (size_t)(col0 + r) * a.words + w;
        if (w + 4 <= a.words) vb = *reinterpret_cast<const uint4 *>(p);
        else {
          if (w < a.words) vb.x = p[0];
          if (w + 1 < a.words) vb.y = p[1];
          if (w + 2 < a.words) vb.z = p[2];
        }
      }
      *reinterpret_cast<uint4 *>(&sA[r * HROW + spc * 4]) = va;
      if (r < (uint32_t)HQ) *reinterpret_cast<uint4 *>(&sB[r * HROW + spc * 4]) = vb;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < HK; kk += 4) {
      uint4 rb[JN];  // the B quads stay in registers, the A quads stream through (keeps the kernel
                    // near 128 VGPRs instead of 240: 4 waves per SIMD instead of 2)
#pragma unroll
      for (int j = 0; j < JN; ++j) rb[j] = *reinterpret_cast<const uint4 *>(&sB[(tx + 16 * j) * HROW + kk]);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint4 ra = *reinterpret_cast<const uint4 *>(&sA[(ty + 16 * i) * HROW + kk]);
#pragma unroll
        for (int j = 0; j < JN; ++j) {
          acc[i][j] += __builtin_popcount(ra.x ^ rb[j].x);
          acc[i][j] += __builtin_popcount(ra.y ^ rb[j].y);
          acc[i][j] += __builtin_popcount(ra.z ^ rb[j].z);
          acc[i][j] += __builtin_popcount(ra.w ^ rb[j].w);
        }
      }
    }
  }
  __syncthreads();  // LDS is free now: per-wave hit staging (one global atomic per flush)
  constexpr uint32_t CAP = 512;
  hg_ham_hit *stage = reinterpret_cast<hg_ham_hit *>(sAB) + wave * CAP;  // 4 x 6 KiB <= 36 KiB
  static_assert(4 * CAP * sizeof(hg_ham_hit) <= 2 * HT * HROW * sizeof(uint32_t), "staging must fit the tiles");
  uint32_t staged = 0;
#define HG_HFLUSH()                                                                        \
  if (staged) {                                                                            \
    uint32_t base = 0;                                                                     \
    if (lane == 0) base = atomicAdd(a.hit_count, staged);                                  \
    base = __builtin_amdgcn_readfirstlane(base);                                           \
    for (uint32_t e = lane; e < staged; e += 64)                                           \
      if (base + e < a.hit_cap) a.hits[base + e] = stage[e];                               \
    staged = 0;                                                                            \
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t r = row0 + ty + 16 * i;
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      const uint32_t c = col0 + tx + 16 * j;
      const bool ok = r < a.R && c < a.Q;
      if (ok && a.dist_out) a.dist_out[(size_t)r * a.Q + c] = acc[i][j];
      const bool hit = ok && a.hit_count && acc[i][j] <= a.max_dist;
      const unsigned long long bal = __ballot(hit);
      if (bal) {
        const uint32_t pos =
            staged + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (hit) stage[pos] = hg_ham_hit{r + a.ref_off, c + a.qry_off, acc[i][j]};
        staged += (uint32_t)__popcll(bal);
        if (staged > CAP - 64) {
          HG_HFLUSH()
        }
      }
    }
  }
  HG_HFLUSH()
#undef HG_HFLUSH
}

}  // namespace

extern "C" hg_status hg_hv_binarize_dev(hg_ctx *c, const int16_t *d_hv, size_t n, uint32_t hv_d, uint32_t *d_bits) {
  if (!c) return HG_ERR_INVALID;
  if (n == 0) return HG_OK;
  if (!d_hv || !d_bits || hv_d == 0) return hg_fail(c, HG_ERR_INVALID, "bad binarize arguments");
  HG_ENTER(c);
  const uint32_t words = (hv_d + 31) / 32;
  for (size_t g0 = 0; g0 < n; g0 += 65535) {
    const uint32_t m = (uint32_t)std::min<size_t>(65535, n - g0);
    hipLaunchKernelGGL(binarize_kernel, dim3((words * 32 + 255) / 256, m), dim3(256), 0, c->stream,
                       d_hv + g0 * hv_d, hv_d, words, d_bits + g0 * words);
    HG_HIP(c, hipGetLastError());
  }
  return HG_OK;
}

static hg_status ham_launch(hg_ctx *c, const uint32_t *d_ref, size_t R, const uint32_t *d_qry, size_t Q,
                            uint32_t hv_d, uint32_t *d_dist, hg_ham_hit *d_hits, uint32_t *d_count, uint32_t cap,
                            uint32_t max_dist, uint32_t ref_off = 0, uint32_t qry_off = 0) {
  const uint32_t words = (hv_d + 31) / 32;
  if (words % 4) return hg_fail(c, HG_ERR_UNSUPPORTED, "hv_d must be a multiple of 128 for the packed path");
  HamArgs a{d_ref, d_qry, (uint32_t)R, (uint32_t)Q, words, d_dist, d_hits, d_count, cap, max_dist, ref_off, qry_off};
  const uint32_t cols = Q <= 16 ? 16u : Q <= 32 ? 32u : (uint32_t)HT;  // query columns per tile
  dim3 grid((unsigned)((Q + cols - 1) / cols), (unsigned)((R + HT - 1) / HT));
  if (grid.y > 65535) return hg_fail(c, HG_ERR_UNSUPPORTED, "too many reference rows for one launch");
  hg_timed tm(c, HG_T_DIST);
  if (cols == 16) hipLaunchKernelGGL(hamming_kernel<1>, grid, dim3(256), 0, c->stream, a);
  else if (cols == 32) hipLaunchKernelGGL(hamming_kernel<2>, grid, dim3(256), 0, c->stream, a);
  else hipLaunchKernelGGL(hamming_kernel<8>, grid, dim3(256), 0, c->stream, a);
  HG_HIP(c, hipGetLastError());
  c->last_kernel[HG_T_DIST] = cols == 16 ? "hamming_kernel<1>" : cols == 32 ? "hamming_kernel<2>" : "hamming_kernel<8>";
  return HG_OK;
}

extern "C" int hg_ctx_last_hamming_path(const hg_ctx *c) { return c ? c->last_ham_path : -1; }

extern "C" hg_status hg_hamming_full_dev(hg_ctx *c, const uint32_t *d_ref_bits, size_t R, const uint32_t *d_qry_bits,
                                         size_t Q, uint32_t hv_d, uint32_t *d_dist_out) {
  if (!c) return HG_ERR_INVALID;
  if (R == 0 || Q == 0) return HG_OK;
  if (!d_ref_bits || !d_qry_bits || !d_dist_out) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  HG_ENTER(c);
  return ham_launch(c, d_ref_bits, R, d_qry_bits, Q, hv_d, d_dist_out, nullptr, nullptr, 0, 0);
}

extern "C" hg_status hg_hamming_search_dev(hg_ctx *c, const uint32_t *d_ref_bits, size_t R, const uint32_t *d_qry_bits,
                                           size_t Q, uint32_t hv_d, uint32_t max_dist, hg_ham_hit *d_out, size_t cap,
                                           size_t *n_out) {
  return hg_hamming_search_block_dev(c, d_ref_bits, R, 0, d_qry_bits, Q, 0, hv_d, max_dist, d_out, cap, n_out);
}

static hg_status hamming_block_once(hg_ctx *c, const uint32_t *d_ref_bits, size_t R, size_t ref_off, const uint32_t *d_qry_bits, size_t Q,
                                    size_t qry_off, uint32_t hv_d, uint32_t max_dist, hg_ham_hit *d_out, size_t cap, size_t *n_out);

extern "C" hg_status hg_hamming_search_block_dev(hg_ctx *c, const uint32_t *d_ref_bits, size_t R, size_t ref_off,
                                                 const uint32_t *d_qry_bits, size_t Q, size_t qry_off, uint32_t hv_d,
                                                 uint32_t max_dist, hg_ham_hit *d_out, size_t cap, size_t *n_out) {
  // (32-bit hit counter: more than 2^32 - 1 pairs run as blocks of reference rows, see hg_dist_block_dev; rows of packed bits
  // are whole 32-bit words)
  if (c && n_out && Q && (uint64_t)R * (uint64_t)Q > hg_pair_limit(c)) {
    const size_t words = ((size_t)hv_d + 31) / 32;
    return hg_run_blocks(c, R, Q, d_out, cap, n_out, [&](size_t r0, size_t rows, hg_ham_hit *out, size_t room, size_t *got) {
      return hamming_block_once(c, d_ref_bits + r0 * words, rows, ref_off + r0, d_qry_bits, Q, qry_off, hv_d, max_dist, out, room, got);
    });
  }
  return hamming_block_once(c, d_ref_bits, R, ref_off, d_qry_bits, Q, qry_off, hv_d, max_dist, d_out, cap, n_out);
}

static hg_status hamming_block_once(hg_ctx *c, const uint32_t *d_ref_bits, size_t R, size_t ref_off, const uint32_t *d_qry_bits, size_t Q,
                                    size_t qry_off, uint32_t hv_d, uint32_t max_dist, hg_ham_hit *d_out, size_t cap, size_t *n_out) {
  if (!c) return HG_ERR_INVALID;
  if (!n_out) return hg_fail(c, HG_ERR_INVALID, "n_out == NULL");
  *n_out = 0;
  if (R == 0 || Q == 0) return HG_OK;
  if (!d_ref_bits || !d_qry_bits || (cap && !d_out)) return hg_fail(c, HG_ERR_INVALID, "NULL argument");
  if (ref_off + R > 0xFFFFFFFFull || qry_off + Q > 0xFFFFFFFFull) return hg_fail(c, HG_ERR_UNSUPPORTED, "global indices must fit 32 bits");
  HG_ENTER(c);
  hg_status s;
  if ((s = hg_ensure(c, c->w_misc, 64)) != HG_OK) return s;
  auto *d_count = static_cast<uint32_t *>(c->w_misc.p);
  if (c->misc_zeroed != d_count) HG_HIP(c, hipMemsetAsync(d_count, 0, 64, c->stream));  // (see hg_dist_block_dev)
  c->misc_zeroed = nullptr;
  // Large searches run as an exact +-1 GEMM on the matrix pipe (hg_run_hamming_mfma: G = D - 2 * distance, the ANI
  // kernel's tiles and hit lists) -- on e2m1 (FP4) operands, or on byte operands when the hook says "mfma" (the A/B
  // partner; hv_d % 128 == 0 only); small ones -- and everything when the hook says "popc" -- on the xor + popcount
  // kernel above.  All three give the same integers.
  const bool want_i8 = c->dbg_ham_path == "mfma" && hv_d % 128 == 0;
  // (up to 32 queries: the popcount kernel's narrow tiles stream the references once, whatever their number -- the matrix
  // pipe's 320 query columns per tile would be 3-10 % used)
  const bool skinny = Q <= 32 && ((hv_d + 31) / 32) % 4 == 0 && (R + HT - 1) / HT <= 65535 && c->dbg_ham_path.empty();
  const bool mfma = !skinny && c->dbg_ham_path != "popc" && hv_d <= 65536 && R < 0x7FFFFFFFull && Q < 0x7FFFFFFFull &&
                    ((uint64_t)R * Q >= (uint64_t)1 << 24 || want_i8 || c->dbg_ham_path == "fp4" ||
                     ((hv_d + 31) / 32) % 4 != 0 /* the popcount kernel reads rows in 16-byte pieces */);
  c->last_ham_path = mfma ? (want_i8 ? 1 : 2) : 0;
  if (mfma)
    s = hg_run_hamming_mfma(c, d_ref_bits, (uint32_t)R, d_qry_bits, (uint32_t)Q, hv_d, max_dist, d_out, d_count,
                            cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap, (uint32_t)ref_off, (uint32_t)qry_off,
                            c->last_ham_path);
  else
    s = ham_launch(c, d_ref_bits, R, d_qry_bits, Q, hv_d, nullptr, d_out, d_count,
                   cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap, max_dist, (uint32_t)ref_off, (uint32_t)qry_off);
  if (s != HG_OK) return s;
  const uint32_t *h_res = nullptr;
  if ((s = hg_publish_words(c, d_count, 1, &h_res, 16)) != HG_OK) return s;
  c->misc_zeroed = d_count;
  const uint32_t found = h_res[0];
  *n_out = found;
  if (found > cap) return hg_fail(c, HG_ERR_CAPACITY, "hit buffer too small");
  return HG_OK;
}
