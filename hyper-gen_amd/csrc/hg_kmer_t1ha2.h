// hg_kmer_t1ha2.h -- t1ha2_atonce as the k-mer kernels compute it: the primes, the hand-written 64 x 64 -> 128 bit products,
// mixup64 / final64, the whole hash for k <= 16 bytes (t1ha2_fixed_w) and for more than 32 bytes read from an LDS phase
// image (t1ha2_long), and the bounds under which the first mixup of k = 17..32 runs its shorter text (hg_kmer_asm.h).
// Included by hg_kmer_kernels.hip only.  Expects: <cstdint> and <utility>, device compilation for gfx950.
#pragma once
namespace {

// t1ha2 primes (src/cuda_kernel.cu:71-77)
constexpr uint64_t P0 = 0xEC99BF0D8372CAABull;
constexpr uint64_t P1 = 0x82434FE90EDCEF39ull;
constexpr uint64_t P2 = 0xD4F06DB99D67BE4Bull;
constexpr uint64_t P3 = 0xBD9CACC22C6E9571ull;
constexpr uint64_t P4 = 0x9C06FAF4D023E3ABull;
constexpr uint64_t P5 = 0xC060724A8424F345ull;
constexpr uint64_t P6 = 0xCB5AF53AE3AAAC31ull;

// The schoolbook 64 x 64 product below sums its two cross products and the carry dword of the low one in 64 bits:
// W = x0 p1 + x1 p0 + hi32(x0 p0) <= (2^32 - 1) (p0 + p1) + p0 - 1.  Where that worst case stays below 2^64 -- in effect
// p0 + p1 < 2^32 -- the sum has no carry-out for ANY x, and the v_addc that would fold it into the high dword of the
// result adds zero.  True for P1 (largest W = 0.567 x 2^64) and P3 (0.914), false for P2 (1.447), P4 (1.423) and P5 (1.268).
constexpr bool mul128_cross_fits(uint64_t P) {
  const unsigned __int128 m = 0xFFFFFFFFull, p0 = (uint32_t)P, p1 = P >> 32;
  return ((m * p1 + m * p0 + ((m * p0) >> 32)) >> 64) == 0;
}
static_assert(mul128_cross_fits(P1) && mul128_cross_fits(P3), "the mixups with P1 and P3 run without the carry op");
static_assert(!mul128_cross_fits(P2) && !mul128_cross_fits(P4) && !mul128_cross_fits(P5), "P2, P4 and P5 need the carry op");

__device__ __forceinline__ uint64_t mk64(uint32_t lo, uint32_t hi) {
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
// rotate right; by a constant: two v_alignbit_b32 (the compiler's own form is a 64-bit shift + shift + or)
__device__ __forceinline__ uint64_t rot64(uint64_t v, unsigned s) {
  if (__builtin_constant_p(s) && s > 0 && s < 64 && s != 32) {
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    return s < 32 ? mk64(__builtin_amdgcn_alignbit(hi, lo, s), __builtin_amdgcn_alignbit(lo, hi, s))
                  : mk64(__builtin_amdgcn_alignbit(lo, hi, s - 32), __builtin_amdgcn_alignbit(hi, lo, s - 32));
  }
  return (v >> s) | (v << (64 - s));
}
// rot64 whose result is opaque to the optimiser.  `x + rot64(y, s)`: the compiler sees the rotate as {lo} | {hi << 32}, turns
// the or of disjoint halves into an add, and adds the two halves SEPARATELY -- two 64-bit adds and two v_mov (zero halves) per
// rotate where one add would do; eight rotates per k-mer in the long-input round.  The empty asm makes the pair one value.
__device__ __forceinline__ uint64_t rot64p(uint64_t v, unsigned s) {
  uint64_t r = rot64(v, s);
  asm("" : "+v"(r));
  return r;
}

// lo64(x * P) returned, hi64(x * P) + addend stored in hi_plus.
// Schoolbook product on 32-bit halves with four v_mad_u64_u32.  Written by hand because the
// compiler's expansion of a 128-bit multiply spends 5 v_mov + one 64-bit add on zero-extending
// partial words; here the third product takes the second as its 64-bit addend and hands its carry
// out in an SGPR pair, and that carry plus the caller's addend are folded into the addend of the
// last product with three 32-bit ops.  A prime whose cross sum fits 64 bits (mul128_cross_fits: P1, P3) has no such carry:
// the third product's carry-out is dead, and neither the v_addc nor, with a zero addend, the v_cndmask is there.
template <uint64_t P, bool ZERO_ADDEND = false, bool UNI_ADDEND = false>
__device__ __forceinline__ uint64_t mul128_lo_hiadd(uint64_t x, uint64_t addend, uint64_t &hi_plus) {
  constexpr uint32_t p0 = (uint32_t)P, p1 = (uint32_t)(P >> 32);
  const uint32_t x0 = (uint32_t)x, x1 = (uint32_t)(x >> 32);
  const uint64_t A = (uint64_t)x0 * p0;
  const uint64_t T = (uint64_t)x1 * p0 + (A >> 32);  // cannot overflow
  uint64_t W, cm;                                     // W = x0*p1 + T (mod 2^64), cm = carry-out lanes
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(W), "=s"(cm) : "v"(x0), "s"(p1), "v"(T));
  constexpr bool CARRY = !mul128_cross_fits(P);       // else W is the whole sum: cm is zero in every lane and unused
  if (ZERO_ADDEND) {
    uint32_t shi = 0;                                 // S = {hi32(W), carry}
    if constexpr (CARRY) asm("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(shi) : "s"(cm));
    hi_plus = (uint64_t)x1 * p1 + mk64((uint32_t)(W >> 32), shi);
  } else {
    // hi64 + addend = x1*p1 + (addend + hi32(W)) + (carry << 32): the 64-bit sum addend + hi32(W) is ONE
    // v_mad_u64_u32 (hi32(W) * 1 + addend; it lands in an aligned register pair, which three 32-bit carry ops
    // do not -- the compiler then paid v_movs to pair them), and the carry goes into the high half of the last
    // product with one v_addc that takes it straight from the SGPR pair.  All of this is mod 2^64, like b += hi.
    // (UNI_ADDEND: the addend is wave-uniform -- the seed in the first mixup -- and is read from its SGPR pair)
    uint64_t t, junk;
    if (UNI_ADDEND)
      asm("v_mad_u64_u32 %0, %1, %2, 1, %3" : "=v"(t), "=s"(junk) : "v"((uint32_t)(W >> 32)), "s"(addend));
    else
      asm("v_mad_u64_u32 %0, %1, %2, 1, %3" : "=v"(t), "=s"(junk) : "v"((uint32_t)(W >> 32)), "v"(addend));
    const uint64_t hp = (uint64_t)x1 * p1 + t;
    uint32_t hph = (uint32_t)(hp >> 32);
    if constexpr (CARRY) asm("v_addc_co_u32_e64 %0, %1, %0, 0, %1" : "+v"(hph), "+s"(cm));
    hi_plus = mk64((uint32_t)hp, hph);
  }
  return mk64((uint32_t)A, (uint32_t)W);
}

// src/cuda_kernel.cu:136-141 with the prime as a template argument (UNI_B: b is wave-uniform)
template <uint64_t P, bool UNI_B = false>
__device__ __forceinline__ void mixup64(uint64_t &a, uint64_t &b, uint64_t v) {
  uint64_t nb;
  a ^= mul128_lo_hiadd<P, false, UNI_B>(b + v, b, nb);
  b = nb;
}
// lo64(x * P).  The compiler's form is one v_mad_u64_u32 + two v_mul_lo_u32 + v_add3 (four slow-class
// instructions); here the two cross products are chained through one 64-bit accumulator -- three v_mad_u64_u32 and a
// plain add.
template <uint64_t P>
__device__ __forceinline__ uint64_t lo64mul(uint64_t x) {
  constexpr uint32_t p0 = (uint32_t)P, p1 = (uint32_t)(P >> 32);
  const uint32_t x0 = (uint32_t)x, x1 = (uint32_t)(x >> 32);
  const uint64_t t = (uint64_t)x0 * p0;
  uint64_t w1, w, junk;
  asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(w1), "=s"(junk) : "v"(x0), "s"(p1));
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(w), "=s"(junk) : "v"(x1), "s"(p0), "v"(w1));
  return mk64((uint32_t)t, (uint32_t)(t >> 32) + (uint32_t)w);
}
// src/cuda_kernel.cu:143-153
__device__ __forceinline__ uint64_t final64(uint64_t a, uint64_t b) {
  const uint64_t x = lo64mul<P0>(a + rot64(b, 41));
  const uint64_t y = lo64mul<P6>(rot64(a, 23) + b);
  uint64_t hi;
  const uint64_t lo = mul128_lo_hiadd<P5, true>(x ^ y, 0, hi);
  return lo ^ hi;
}

// t1ha2_atonce for a compile-time length K <= 16 on 8-byte little-endian words w[0..ceil(K/8)) with the unused bytes
// of the last word zero (tail switch of src/cuda_kernel.cu:205-245).  k = 17..32 is the text of hg_kmer_asm.h.
template <int K>
__device__ __forceinline__ uint64_t t1ha2_fixed_w(const uint64_t *w, uint64_t seed) {
  static_assert(K >= 1 && K <= 16, "one or two words");
  // the first mixup's `b` operand is wave-uniform (the seed or the length)
  uint64_t a = seed, b = (uint64_t)K;
  int i = 0;
  if (K > 8) mixup64<P2, true>(a, b, w[i++]);
  mixup64<P1, (K <= 8)>(b, a, w[i++]);
  return final64(a, b);
}

// A k-mer of the long-k kernel as t1ha2_long reads it: a run of dwords in an LDS phase image
struct LdsStrand {
  const uint32_t *base;  // dword 0 of the k-mer in the phase image of its start (image (byte0 & 3), dword byte0 >> 2)
  uint32_t d0, d1;       // its first two dwords when `cached` (the strand choice has read them already)
  bool cached;           // (always true in kmer_sample_long; without the field, k = 53..55 compile to other instructions)
  __device__ __forceinline__ uint32_t dword(uint32_t i) const {  // bytes [byte0 + 4i, byte0 + 4i + 4)
    if (cached && __builtin_constant_p(i) && i == 0) return d0;
    if (cached && __builtin_constant_p(i) && i == 1) return d1;
    return base[i];
  }
  __device__ __forceinline__ uint64_t word(uint32_t byte_off, uint32_t nbytes) const {  // little endian, byte_off % 8 == 0
    uint32_t lo = dword(byte_off / 4), hi = nbytes > 4 ? dword(byte_off / 4 + 1) : 0u;
    if (nbytes < 4) lo &= (1u << (8 * nbytes)) - 1;
    else if (nbytes > 4 && nbytes < 8) hi &= (1u << (8 * (nbytes - 4))) - 1;
    return mk64(lo, hi);
  }
};

// t1ha2_atonce of `len` > 32 bytes (published t1ha2: lanes c, d, 32 bytes per round, squash, then the tail switch of
// src/cuda_kernel.cu:207-245).  LEN > 0: len == LEN is a compile-time constant and everything below unrolls.
template <uint32_t LEN>
__device__ __forceinline__ uint64_t t1ha2_long(const LdsStrand &sb, uint32_t len_rt, uint64_t seed) {
  const uint32_t len0 = LEN ? LEN : len_rt;
  uint64_t a = seed, b = (uint64_t)len0;
  uint32_t off = 0, len = len0;
  {
    uint64_t c = rot64((uint64_t)len, 23) + ~seed;
    uint64_t d = ~(uint64_t)len + rot64(seed, 19);
    auto round = [&]() __attribute__((always_inline)) {
      const uint64_t w0 = sb.word(off, 8), w1 = sb.word(off + 8, 8), w2 = sb.word(off + 16, 8), w3 = sb.word(off + 24, 8);
      off += 32;
      const uint64_t d02 = w0 + rot64p(w2 + d, 56);
      const uint64_t c13 = w1 + rot64p(w3 + c, 19);
      d ^= b + rot64p(w1, 38);
      c ^= a + rot64p(w0, 57);
      b ^= lo64mul<P6>(c13 + w2);
      a ^= lo64mul<P5>(d02 + w3);
    };
    if constexpr (LEN != 0) {
      static_assert(LEN > 32 && LEN <= 64, "compile-time lengths: one or two rounds");
      round();
      if constexpr (LEN == 64) round();  // (data < detent  <=>  off + 31 < len)
    } else {
      do round();
      while (off + 31 < len);
    }
    a ^= lo64mul<P6>(c + rot64p(d, 23));
    b ^= lo64mul<P5>(rot64p(c, 19) + d);
    len &= 31;
  }
  uint32_t rem = len;
  if (rem > 24) { mixup64<P4>(a, b, sb.word(off, 8)); off += 8, rem -= 8; }
  if (rem > 16) { mixup64<P3>(b, a, sb.word(off, 8)); off += 8, rem -= 8; }
  if (rem > 8) { mixup64<P2>(a, b, sb.word(off, 8)); off += 8, rem -= 8; }
  if (rem > 0) mixup64<P1>(b, a, sb.word(off, rem));
  return final64(a, b);
}

// The bounded first mixup of k = 17..32 (HG_KS_MUL128_BOUNDED, hg_kmer_asm.h) at its worst case: both dwords of w0 are
// "TTTT" -- every staged byte of a kept k-mer is one of ACGT -- and s (operand and addend of the stage: the seed for
// k <= 24, K for k >= 25) is the largest one admitted.  Every term grows with x0, x1 and s, so the maxima decide.
constexpr uint64_t FIRST_SEED_END = 1ull << 28;  // k = 17..24: seeds from here on take the general text (they hold up to 0x66C7395F)
constexpr bool first_mixup_bounded(uint64_t P, uint64_t s) {
  const uint64_t p0 = (uint32_t)P, p1 = P >> 32, x1 = 0x54545454ull, x0 = x1 + s;
  if (s >> 32 || x0 >> 32) return false;                                              // x0 = w0.lo + s is a 32-bit add
  const unsigned __int128 W = (unsigned __int128)x0 * p1 + (unsigned __int128)x1 * p0 + ((x0 * p0) >> 32);
  if (W >> 64) return false;                                                           // no carry out of the third product
  const uint64_t z = (uint64_t)(W >> 32) + s;
  if (z >> 32) return false;                                                           // hi32(W) + s is a 32-bit add
  return (((unsigned __int128)x1 * p1 + z) >> 64) == 0;                               // hi64 + s < 2^64
}
template <int... Ks>
constexpr bool first_mixup_bounded_k25_32(std::integer_sequence<int, Ks...>) {
  return (first_mixup_bounded(P4, 25 + Ks) && ...);
}
static_assert(first_mixup_bounded(P3, FIRST_SEED_END - 1), "k = 17..24: first mixup's bounds at the largest admitted seed");
static_assert(first_mixup_bounded_k25_32(std::make_integer_sequence<int, 8>{}), "k = 25..32: first mixup's bounds with s = K");
static_assert(first_mixup_bounded(P3, 0x66C7395Full) && !first_mixup_bounded(P3, 0x66C73960ull), "where the k = 17..24 bounds end");
}  // namespace
