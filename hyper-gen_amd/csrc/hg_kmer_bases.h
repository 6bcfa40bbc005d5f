// hg_kmer_bases.h -- four bases at a time: SWAR classification of a dword of ASCII, as both k-mer kernels stage it.
// Included by hg_kmer_kernels.hip only.  Expects: <cstdint>, device compilation for gfx950.
#pragma once
namespace {

// needletail normalize: u/U -> T  ('U' ^ 'T' == 1)
__device__ __forceinline__ uint32_t u2t_rewrite(uint32_t x) {
  const uint32_t e = (x & 0xDFDFDFDFu) ^ 0x55555555u;
  const uint32_t nz = ((e & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | e;  // bit 7 set <=> byte != 'U'
  return x ^ ((~nz & 0x80808080u) >> 7);
}
// dword of ASCII -> cd: 2-bit code per byte (A,C,G,T -> 0,1,2,3, whatever the case; any other byte gets some code too),
// fa: "ACGT"[code], ca: "TGCA"[code].  A byte is a base iff its upper-cased value equals fa's: see not_a_base4.
__device__ __forceinline__ void classify4(uint32_t x, uint32_t &cd, uint32_t &fa, uint32_t &ca) {
  const uint32_t tt = x ^ (x >> 1);
  cd = (tt >> 1) & 0x03030303u;
  fa = __builtin_amdgcn_perm(0u, 0x54474341u, cd);
  ca = __builtin_amdgcn_perm(0u, 0x41434754u, cd);
}
// bit 7 of a byte set <=> that byte of x is not the base classify4 made of it (fa)
__device__ __forceinline__ uint32_t not_a_base4(uint32_t x, uint32_t fa) {
  const uint32_t d = (x & 0xDFDFDFDFu) ^ fa;
  return (((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;
}
}  // namespace
