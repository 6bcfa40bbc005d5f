// hg_encode_kernels.hip -- hypervector encode on gfx950.
//
// encode      : hd::encode_hash_hd{,_avx2} + dist::compute_hv_l2_norm
//               (src/hd.rs:14-112, src/dist.rs:132-137):
//                   hv[d] = 2 * #{h : bit_d(WyRng_h) = 1} - n      (i16 wrapping)
//               The WyRng stream is random-access (state_i = h + (i+1)*INC), so lane i of a
//               wave produces word i of every hash directly; the 64 bit-columns of that word
//               are counted with bit-sliced carry-save adders (a Harley-Seal tree over 16
//               hashes, ~6 logic ops per word instead of 128 per-bit adds), expanded once
//               per genome into LDS counters, and written out in the scalar or the AVX2
//               dimension order.
#include "hg_internal.h"

namespace {

constexpr int ENC_WG = 512;
constexpr int ENC_WAVES = ENC_WG / 64;
constexpr uint64_t WY_INC = 0xa0761d6478bd642full;
constexpr uint64_t WY_XOR = 0xe7037ed1a0b428dbull;

__device__ __forceinline__ uint64_t wy_word(uint64_t hash, uint64_t off) {
  // word (i) of WyRng seeded with `hash`: state = hash + (i+1)*INC, off = (i+1)*INC
  uint64_t s = hash + off;
  unsigned __int128 m = (unsigned __int128)(s ^ WY_XOR) * s;
  return (uint64_t)(m >> 64) ^ (uint64_t)m;
}

// carry-save adder on 64 independent bit columns
// (majority and three-way xor as ONE v_bitop3_b32 per 32-bit half each -- truth tables 0xE8 and 0x96 with a = 0xF0,
// b = 0xCC, c = 0xAA --: 4 instructions per adder instead of the 10 the compiler makes of and / or / xor)
__device__ __forceinline__ void csa(uint64_t &hi, uint64_t &lo, uint64_t a, uint64_t b, uint64_t c) {
  const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32), b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32);
  const uint32_t c0 = (uint32_t)c, c1 = (uint32_t)(c >> 32);
  const uint32_t h0 = __builtin_amdgcn_bitop3_b32(a0, b0, c0, 0xE8), h1 = __builtin_amdgcn_bitop3_b32(a1, b1, c1, 0xE8);
  const uint32_t l0 = __builtin_amdgcn_bitop3_b32(a0, b0, c0, 0x96), l1 = __builtin_amdgcn_bitop3_b32(a1, b1, c1, 0x96);
  hi = (uint64_t)h0 | ((uint64_t)h1 << 32);
  lo = (uint64_t)l0 | ((uint64_t)l1 << 32);
}

// Harley-Seal: 16 words into the bit-sliced counters pl[0..4) (ones, twos, fours, eights); returns the carry into the sixteens
__device__ __forceinline__ uint64_t harley_seal16(uint64_t *pl, const uint64_t (&x)[16]) {
  uint64_t twosA, twosB, foursA, foursB, eightsA, eightsB, sixteens;
  csa(twosA, pl[0], pl[0], x[0], x[1]);
  csa(twosB, pl[0], pl[0], x[2], x[3]);
  csa(foursA, pl[1], pl[1], twosA, twosB);
  csa(twosA, pl[0], pl[0], x[4], x[5]);
  csa(twosB, pl[0], pl[0], x[6], x[7]);
  csa(foursB, pl[1], pl[1], twosA, twosB);
  csa(eightsA, pl[2], pl[2], foursA, foursB);
  csa(twosA, pl[0], pl[0], x[8], x[9]);
  csa(twosB, pl[0], pl[0], x[10], x[11]);
  csa(foursA, pl[1], pl[1], twosA, twosB);
  csa(twosA, pl[0], pl[0], x[12], x[13]);
  csa(twosB, pl[0], pl[0], x[14], x[15]);
  csa(foursB, pl[1], pl[1], twosA, twosB);
  csa(eightsB, pl[2], pl[2], foursA, foursB);
  csa(sixteens, pl[3], pl[3], eightsA, eightsB);
  return sixteens;
}

constexpr int HI_PLANES = 10;  // counts up to 15 + 16*1023 per flush window

// One row by the ENC_WG threads of the workgroup: hv[d] = 2 * count - n (i16 wrapping) in `layout` order, *norm2 = sum hv^2
// (i32 wrapping).  count_of(w, j) is the count of bit j of word w.  Scalar order: bit j -> position j of its 64-block.
// AVX2 order (src/hd.rs:14-92): bit j -> position 4 * (j % 16) + j / 16, i.e. j = 16 * (pos % 4) + pos / 4.  Dimensions past
// the last whole 64-block carry no random bit: count 0.
template <class CountOf>
__device__ __forceinline__ void write_hv_row(uint32_t hv_d, uint32_t layout, uint32_t n, int16_t *__restrict__ out,
                                             int32_t *__restrict__ norm2, int32_t *s_red, CountOf count_of) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d_full = (hv_d / 64) * 64;
  uint32_t acc = 0;
  for (uint32_t d = tid; d < hv_d; d += ENC_WG) {
    uint32_t c = 0;
    if (d < d_full) {
      const uint32_t pos = d & 63;
      c = count_of(d >> 6, (layout == HG_LAYOUT_AVX2) ? (16 * (pos & 3) + (pos >> 2)) : pos);
    }
    const int16_t v = (int16_t)(uint16_t)(2u * c - n);
    out[d] = v;
    acc += (uint32_t)((int32_t)v * (int32_t)v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  if (lane == 0) s_red[wave] = (int32_t)acc;
  __syncthreads();
  if (tid == 0) {
    uint32_t s = 0;
    for (int w = 0; w < ENC_WAVES; ++w) s += (uint32_t)s_red[w];
    *norm2 = (int32_t)s;
  }
}

// One workgroup per genome.  hv_d/64 words are spread over lanes; when hv_d/64 < 64*ENC_WAVES
// several waves share a word and split the hashes.
// SPLIT = false: one workgroup per genome, writes the hypervector.  Genomes with more than `split_over`
// hashes are left to the split launch (split_over = ~0u: none are).
// SPLIT = true : one workgroup per (genome, slab of HG_ENC_SLAB hashes) item; the per-dimension counts are
// added into accum[slot][word * 64 + bit] and encode_finalize_kernel turns them into the hypervector --
// a 3 Gbp genome (2 M hashes) otherwise keeps one workgroup busy for 30 ms while hashing it takes 8.
template <bool SPLIT>
__global__ __launch_bounds__(ENC_WG) void encode_kernel(
    const hg_genome_meta *__restrict__ meta, const uint64_t *__restrict__ hits,
    const uint32_t *__restrict__ ndistinct, uint32_t hv_d, uint32_t layout,
    int16_t *__restrict__ hv_out, int32_t *__restrict__ norm2_out, uint32_t split_over,
    const uint2 *__restrict__ items, uint32_t *__restrict__ accum, uint32_t wave_max) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_cnt[];  // [64][n_words + 1]
  __shared__ int32_t s_red[ENC_WAVES];
  const uint32_t g = SPLIT ? items[blockIdx.x].x : blockIdx.x;
  const hg_genome_meta gm = meta[g];
  const uint32_t n_all = ndistinct[g];
  if (!SPLIT && (n_all > split_over || n_all <= wave_max || n_all == HG_NHASH_PENDING)) return;  // split launch / encode_wave_kernel / left to the redo
  const uint32_t slab = SPLIT ? (items[blockIdx.x].y & 0xffffu) : 0u, slot = SPLIT ? (items[blockIdx.x].y >> 16) : 0u;
  const uint32_t h0 = SPLIT ? slab * HG_ENC_SLAB : 0u;
  if (SPLIT && h0 >= n_all) return;  // the plan was made from the raw (pre-unique) count
  const uint32_t n = SPLIT ? (n_all - h0 < HG_ENC_SLAB ? n_all - h0 : HG_ENC_SLAB) : n_all;  // hashes of this workgroup
  const uint64_t *__restrict__ hs = hits + gm.hit_off + h0;
  const uint32_t n_words = hv_d / 64;
  const uint32_t stride = n_words + 1;  // +1: conflict-free column writes and row reads
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform => scalar hash loads

  for (uint32_t i = tid; i < 64 * stride; i += ENC_WG) s_cnt[i] = 0;
  __syncthreads();

  // word groups of 64 words; (group, hash-slice) pairs are dealt round-robin to the waves
  const uint32_t n_groups = (n_words + 63) / 64;
  const uint32_t slices = (n_groups == 0 || n_groups >= (uint32_t)ENC_WAVES) ? 1u : (uint32_t)ENC_WAVES / n_groups;
  for (uint32_t job = wave; job < n_groups * slices; job += ENC_WAVES) {
    const uint32_t grp = job / slices, slice = job % slices;
    const uint32_t w = grp * 64 + lane;  // this lane's word index
    const bool w_ok = w < n_words;
    const uint64_t off = (uint64_t)(w + 1) * WY_INC;
    // hashes of this slice: blocks of 16, block b belongs to slice (b % slices)
    uint64_t pl[4 + HI_PLANES];  // ones, twos, fours, eights, then the 16s planes
#pragma unroll
    for (int p = 0; p < 4 + HI_PLANES; ++p) pl[p] = 0;
    uint32_t blocks_in_window = 0;

    auto flush = [&]() {
      // expand the bit-sliced counters of this lane's word into the LDS counters
      if (w_ok) {
#pragma unroll 4
        for (uint32_t j = 0; j < 64; ++j) {
          uint32_t c = 0;
#pragma unroll
          for (int p = 0; p < 4 + HI_PLANES; ++p) c |= (uint32_t)((pl[p] >> j) & 1) << p;
          if (c) atomicAdd(&s_cnt[j * stride + w], c);
        }
      }
#pragma unroll
      for (int p = 0; p < 4 + HI_PLANES; ++p) pl[p] = 0;
      blocks_in_window = 0;
    };

    for (uint32_t b0 = slice * 16; b0 < n; b0 += slices * 16) {
      uint64_t x[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const uint32_t idx = b0 + t;
        x[t] = (idx < n) ? wy_word(hs[idx], off) : 0ull;  // hs[idx] is wave-uniform
      }
      uint64_t carry = harley_seal16(pl, x);  // ripple into the high planes
#pragma unroll
      for (int p = 0; p < HI_PLANES; ++p) {
        uint64_t t = pl[4 + p] & carry;
        pl[4 + p] ^= carry;
        carry = t;
      }
      if (++blocks_in_window == (1u << HI_PLANES) - 1) flush();
    }
    flush();
  }
  __syncthreads();

  if (SPLIT) {
    uint32_t *__restrict__ a = accum + (size_t)slot * hv_d;
    for (uint32_t i = tid; i < n_words * 64; i += ENC_WG) {
      const uint32_t w = i >> 6, j = i & 63, c = s_cnt[j * stride + w];
      if (c) atomicAdd(&a[i], c);  // no value returned: nothing waits for it
    }
    return;
  }
  write_hv_row(hv_d, layout, n, hv_out + (size_t)g * hv_d, norm2_out + g, s_red,
               [&](uint32_t w, uint32_t j) { return s_cnt[j * stride + w]; });
}

typedef short short2v __attribute__((ext_vector_type(2)));

// The lane's 64 bit-column counts, held bit-sliced in planes pl[0..P) (count < 2^P), as its 64 outputs 2 * count - n in the
// AVX2 dimension order, two per dword, + their squares into acc.  Output position p of the 64-block holds bit
// j = 16 * (p % 4) + p / 4 (src/hd.rs:14-92), so the pair (2 m, 2 m + 1) holds bits (b, b + 16) of ONE 32-bit half of the
// planes, b = m / 2 of the low half for even m, of the high half for odd m: one shift and one v_and_or per plane moves
// both bits of plane k to bit k of their 16-bit fields -- 2 P instructions per pair, then packed 16-bit arithmetic
// (v_pk_lshlrev_b16, v_pk_sub_i16, v_dot2c_i32_i16).  (The generic form below extracts every bit of every plane on its own:
// 2 900 instructions per lane for P = 14 against 32 (2 P + 3).)
template <int P>
__device__ __forceinline__ void expand_pairs_avx2(const uint64_t *pl, uint32_t n, uint32_t (&packed)[32], uint32_t &acc) {
  const short2v nv = {(short)(uint16_t)n, (short)(uint16_t)n};
#pragma unroll
  for (int m = 0; m < 32; ++m) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const int t = m >> 1;
      const uint32_t xw = (m & 1) ? (uint32_t)(pl[k] >> 32) : (uint32_t)pl[k];
      const uint32_t sh = t >= k ? xw >> (t - k) : xw << (k - t);
      c |= sh & (0x00010001u << k);
    }
    const short2v cv = __builtin_bit_cast(short2v, c), v = cv + cv - nv;  // i16 wrapping, like the reference's i16 sums
    acc = (uint32_t)__builtin_amdgcn_sdot2(v, v, (int)acc, false);  // (no clamp: wraps like the i32 sum)
    packed[m] = __builtin_bit_cast(uint32_t, v);
  }
}

// One WAVE per genome (four genomes per workgroup) for hash sets of at most HG_ENC_WAVE_MAX hashes -- every
// ordinary genome.  Lane i owns word i of the random stream (hv_d / 64 <= 64 words per pass), so the 64 bit
// columns of that word are counted entirely inside the lane: bit-sliced carry-save planes over all hashes,
// expanded once at the end straight into the output row.  No atomics, no barrier; the
// eight-waves-per-genome kernel above (LDS counters, one flush per wave and word) remains for larger sets.
// (Which genomes it takes: hg_launch_encode.)  A genome of a few kbp has 1-30 hashes: there the expansion IS the kernel,
// and it is specialised on the number of planes the counts can occupy (4 for n < 16).
__global__ __launch_bounds__(256) void encode_wave_kernel(
    const hg_genome_meta *__restrict__ meta, const uint64_t *__restrict__ hits,
    const uint32_t *__restrict__ ndistinct, uint32_t n_genomes, uint32_t hv_d, uint32_t layout,
    int16_t *__restrict__ hv_out, int32_t *__restrict__ norm2_out, uint32_t wave_max) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (g >= n_genomes) return;
  const uint32_t n = ndistinct[g];
  if (n > wave_max) return;  // encode_kernel handles this genome
  const uint64_t *__restrict__ hs = hits + meta[g].hit_off;
  const uint32_t n_words = hv_d / 64;
  int16_t *__restrict__ out = hv_out + (size_t)g * hv_d;
  const bool vec_ok = (hv_d % 8 == 0) && ((reinterpret_cast<uintptr_t>(hv_out) & 15) == 0);
  // A lane holds 128 consecutive bytes of the row: stored from the registers, every store instruction of the wave touches 64
  // different 128-byte lines, 16 bytes of each.  For the shortest sets (n < 16: a genome of a few kbp), where the 8 KB row
  // IS the genome's cost, the pass goes through the wave's 8 KB of LDS instead -- lane l's q-th 16 bytes at slot
  // 8 l + (q ^ (l & 7)) -- and leaves with the lanes on consecutive addresses: 400 000 sets of 1-2 hashes 1.16 -> 0.78 ms
  // (4.2 TB/s of rows).  Taken for n < 64 as well, the kernel needs 181 registers instead of 121 and every larger set pays
  // (0.34 -> 0.46 ms at 33 hashes, 1.46 -> 2.14 at 3 300): not taken.
  __shared__ uint4 s_rows[4][512];
  uint4 *const s_row = s_rows[threadIdx.x >> 6];
  const bool via_lds = vec_ok && n < 16 && layout == HG_LAYOUT_AVX2;  // wave-uniform
  uint32_t acc = 0;
  for (uint32_t grp = 0; grp * 64 < n_words; ++grp) {
    const uint32_t w = grp * 64 + lane;
    const uint64_t off = (uint64_t)(w + 1) * WY_INC;
    uint64_t pl[4 + HI_PLANES];  // ones, twos, fours, eights, then the 16s planes
#pragma unroll
    for (int p = 0; p < 4 + HI_PLANES; ++p) pl[p] = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 16) {
      // (the sixteen hashes are wave-uniform scalar loads, all issued before the first is used: the index is clamped
      // instead of the load being skipped, which would put every load of a short set behind its own branch and wait)
      uint64_t h[16], x[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) h[t] = hs[b0 + t < n ? b0 + t : n - 1];
#pragma unroll
      for (int t = 0; t < 16; ++t) x[t] = (b0 + t < n) ? wy_word(h[t], off) : 0ull;
      const uint64_t sixteens = harley_seal16(pl, x);
      if (n >= 16) {  // (wave-uniform; fewer than 16 hashes never carry out of the eights)
        uint64_t carry = sixteens;
#pragma unroll
        for (int p = 0; p < HI_PLANES; ++p) {
          const uint64_t t = pl[4 + p] & carry;
          pl[4 + p] ^= carry;
          carry = t;
        }
      }
    }
    if (via_lds) {  // wave-uniform
      if (w < n_words) {
        uint32_t packed[32];
        expand_pairs_avx2<4>(pl, n, packed, acc);
#pragma unroll
        for (int q = 0; q < 8; ++q)
          s_row[8 * lane + ((uint32_t)q ^ (lane & 7u))] = make_uint4(packed[4 * q], packed[4 * q + 1], packed[4 * q + 2], packed[4 * q + 3]);
      }
      // (the wave's own LDS operations complete in order; the fences keep the compiler from moving them across each other)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const uint32_t pass_words = n_words - grp * 64 < 64u ? n_words - grp * 64 : 64u;
      uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)grp * 64 * 64);
#pragma unroll 2
      for (uint32_t sidx = 0; sidx < 8; ++sidx) {
        const uint32_t i = sidx * 64 + lane, l = i >> 3, q = i & 7u;
        if (l < pass_words) {  // (written once, read by nobody on this device soon: past the caches)
          typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
          const uint4 v = s_row[8 * l + (q ^ (l & 7u))];
          __builtin_nontemporal_store(u32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4 *>(dst + i));
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the next pass writes the same slots)
      __builtin_amdgcn_wave_barrier();
    } else if (w < n_words) {
      uint32_t packed[32];
      if (layout == HG_LAYOUT_AVX2) {  // wave-uniform, and so is the choice of the plane count
        if (n < 16) expand_pairs_avx2<4>(pl, n, packed, acc);
        else if (n < 64) expand_pairs_avx2<6>(pl, n, packed, acc);
        else if (n < 256) expand_pairs_avx2<8>(pl, n, packed, acc);
        else expand_pairs_avx2<4 + HI_PLANES>(pl, n, packed, acc);
      } else {  // scalar order: output position p holds bit p
#pragma unroll
        for (int p = 0; p < 64; ++p) {
          uint32_t c = 0;
#pragma unroll
          for (int q = 0; q < 4 + HI_PLANES; ++q) c |= (uint32_t)((pl[q] >> p) & 1) << q;
          const int16_t v = (int16_t)(uint16_t)(2u * c - n);
          acc += (uint32_t)((int32_t)v * (int32_t)v);
          if (p & 1) packed[p >> 1] |= (uint32_t)(uint16_t)v << 16;
          else packed[p >> 1] = (uint32_t)(uint16_t)v;
        }
      }
      int16_t *dst = out + (size_t)w * 64;
      if (vec_ok) {
#pragma unroll
        for (int q = 0; q < 8; ++q)  // (NOT past the caches like the LDS pass above: a lane's eight 16-byte stores lie in ONE 128-byte line the
                                     // L2 puts together -- written non-temporally they reach HBM as partial lines, 0.33 -> 1.68 ms at 33 hashes)
          reinterpret_cast<uint4 *>(dst)[q] = make_uint4(packed[4 * q], packed[4 * q + 1], packed[4 * q + 2], packed[4 * q + 3]);
      } else {
#pragma unroll
        for (int q = 0; q < 32; ++q) dst[2 * q] = (int16_t)(packed[q] & 0xffffu), dst[2 * q + 1] = (int16_t)(packed[q] >> 16);
      }
    }
  }
  // dimensions past the last whole 64-block carry no random bit: count 0
  for (uint32_t d = n_words * 64 + lane; d < hv_d; d += 64) {
    const int16_t v = (int16_t)(uint16_t)(0u - n);
    out[d] = v;
    acc += (uint32_t)((int32_t)v * (int32_t)v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  if (lane == 0) norm2_out[g] = (int32_t)acc;
}

// grid: split genomes.  accum[slot][word * 64 + bit] -> hv (layout, i16 wrapping) + norm
__global__ __launch_bounds__(ENC_WG) void encode_finalize_kernel(const uint32_t *__restrict__ genomes,
                                                                 const uint32_t *__restrict__ ndistinct,
                                                                 const uint32_t *__restrict__ accum, uint32_t hv_d,
                                                                 uint32_t layout, int16_t *__restrict__ hv_out,
                                                                 int32_t *__restrict__ norm2_out) {
  __shared__ int32_t s_red[ENC_WAVES];
  const uint32_t g = genomes[blockIdx.x];
  const uint32_t *__restrict__ a = accum + (size_t)blockIdx.x * hv_d;
  write_hv_row(hv_d, layout, ndistinct[g], hv_out + (size_t)g * hv_d, norm2_out + g, s_red,
               [&](uint32_t w, uint32_t j) { return a[w * 64 + j]; });
}

}  // namespace

static hipError_t encode_attr() {
  static std::atomic<uint64_t> done{0};
  if (attr_done_on_this_device(done, false)) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&encode_kernel<false>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&encode_kernel<true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
  if (e == hipSuccess) attr_done_on_this_device(done, true);
  return e;
}

hipError_t hg_launch_encode(hipStream_t st, const hg_genome_meta *d_meta, uint32_t n_genomes,
                            const uint64_t *d_hits, const uint32_t *d_ndistinct, uint32_t hv_d,
                            uint32_t layout, int16_t *d_hv, int32_t *d_norm2, const hg_encode_split *split,
                            uint32_t max_hashes, std::string *launched) {
  if (n_genomes == 0) return hipSuccess;
  const size_t lds = (size_t)64 * (hv_d / 64 + 1) * sizeof(uint32_t);
  if (lds > 150 * 1024) return hipErrorInvalidValue;  // hv_d up to ~38k
  hipError_t e = encode_attr();
  if (e != hipSuccess) return e;
  const bool sp = split && split->n_items;
  // One wave per genome does less work per genome (no LDS counters, no per-wave flush) but runs a genome's
  // hashes serially: it takes everything when the batch alone fills the SIMDs several times over, and only the
  // tiny sets (where the eight-wave kernel is all overhead) otherwise.  1 000 x 3 333 hashes: 0.18 ms with eight
  // waves per genome, 0.39 ms with one; 100 000 x 20 hashes: 4.4 ms vs 0.7 ms.
  const uint32_t wave_max = n_genomes >= 8192 ? (uint32_t)HG_ENC_WAVE_MAX : 256u;
  hipLaunchKernelGGL(encode_wave_kernel, dim3((n_genomes + 3) / 4), dim3(256), 0, st, d_meta, d_hits, d_ndistinct, n_genomes,
                     hv_d, layout, d_hv, d_norm2, wave_max);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hg_note_launch(launched, "encode_wave_kernel");
  if (max_hashes > wave_max) {  // some genome may exceed what the wave kernel takes
    hipLaunchKernelGGL(encode_kernel<false>, dim3(n_genomes), dim3(ENC_WG), lds, st, d_meta, d_hits, d_ndistinct, hv_d,
                       layout, d_hv, d_norm2, sp ? (uint32_t)HG_ENC_SLAB : ~0u, (const uint2 *)nullptr, (uint32_t *)nullptr,
                       wave_max);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hg_note_launch(launched, "encode_kernel<false>");
  }
  if (!sp) return e;
  if ((e = hipMemsetAsync(split->d_accum, 0, (size_t)split->n_genomes * hv_d * sizeof(uint32_t), st)) != hipSuccess) return e;
  hipLaunchKernelGGL(encode_kernel<true>, dim3(split->n_items), dim3(ENC_WG), lds, st, d_meta, d_hits, d_ndistinct, hv_d,
                     layout, d_hv, d_norm2, ~0u, reinterpret_cast<const uint2 *>(split->d_items), split->d_accum, 0u);
  hipLaunchKernelGGL(encode_finalize_kernel, dim3(split->n_genomes), dim3(ENC_WG), 0, st, split->d_genomes, d_ndistinct,
                     split->d_accum, hv_d, layout, d_hv, d_norm2);
  hg_note_launch(launched, "encode_kernel<true>");
  hg_note_launch(launched, "encode_finalize_kernel");
  return hipGetLastError();
}
