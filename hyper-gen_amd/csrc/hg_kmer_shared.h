// hg_kmer_shared.h -- kmer_sample_shared: the shared-image k-mer kernel, compile-time k in [1, 32], both strand modes, ASCII
// or hg_pack2 input.  Its tile geometry (GeoS), the two staging front ends, the code window and strand choice, the two
// k-mer loops, the kernel.  Included by hg_kmer_kernels.hip only.  Expects: WG (the .hip), hg_kmer_t1ha2.h, hg_kmer_asm.h,
// hg_kmer_bases.h, hg_kmer_hits.h.
#pragma once
namespace {

// The WORKGROUP keeps one image of its tile in LDS in all four byte phases -- F_phi[i] = bytes [4 i + phi, 4 i + phi + 4) of
// the tile, phi = 0..3 -- and the same for the reverse complement R[q] = comp(F[N - 1 - q]).  A lane owns M = 12 consecutive
// starts p = 12 tid + j, so the phase of k-mer j is j & 3 on the forward strand and, with N chosen such that
// (N - K) & 3 == 3, 3 - (j & 3) on the reverse strand: compile-time per j.  Both strands' hash words are then whole dwords at
// [base + imm(j) + 4 m]: ONE v_cndmask picks the base (forward: FB + 12 tid; reverse: one of three per-lane constants
// RB' - 12 tid - 8 (j >> 2)), the immediates imm(j) = S (j & 3) + 4 (j >> 2) are shared by both strands (reverse phase psi
// is stored at S (3 - psi) for that), and the ds_reads deliver the words straight into the register pairs the multiplies
// take -- no VALU instruction touches the bytes.  The images are written once per tile by the lanes that load the bases
// (12 bases + one lookahead dword per lane: every base is classified once); the 2-bit codes for the strand compare and
// the validity bits go through LDS as well (768 + 1 036 bytes).  Two barriers per tile; 28 KB of LDS per workgroup
// (5 workgroups per CU).  What the kernels before this one paid instead: DESIGN.md 4.1.

template <int... Js, class F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, Js...>, F &&f) {
  (f(std::integral_constant<int, Js>{}), ...);
}

template <int K>
struct GeoS {
  static constexpr int M = 12;                      // starts per lane and tile (multiple of 4: the phase of start j is j & 3)
  static constexpr int DW = M / 4;
  // Every lane stages one unit of M bases; the k-mers of the last lanes' windows would need bases behind the staged
  // area, so the last LOOK_UNITS lanes hash nothing and the tile advances by (WG - LOOK_UNITS) * M starts: 0.8 % of the
  // hashing slots of one wave idle -- against a second, three-lane staging pass on the way to the barrier (+2 %)
  static constexpr int WIN = K <= 21 ? 32 : 48;     // bases of a lane's code window (its M starts + K - 1 more): 64 / 96 bits
  static constexpr int LOOK_UNITS = (WIN - M + M - 1) / M;  // the last hashing lane's window ends inside the staged area: 2 / 3 units
  static constexpr int TILE = (WG - LOOK_UNITS) * M;  // 3 048 / 3 036 starts
  static constexpr int TILES = 9;
  static constexpr int ITEM = TILE * TILES;         // 27 432 / 27 324 starts per work item
  static constexpr int UNITS = WG;
  static constexpr int NB_T = UNITS * M;            // staged bases (3 072)
  static constexpr int N_R = NB_T + ((K + 3 - NB_T) & 3);  // length the reverse strand is indexed in: (N_R - K) & 3 == 3
  static constexpr int S = 4 * (NB_T / 4 + 3);      // bytes per phase image
  static constexpr int ND = (K + 3) / 4, NB = K - 4 * (ND - 1), NW = (K + 7) / 8;
  static_assert(M + K - 1 <= WIN && K <= 32, "a lane's k-mers live in its code window; 2 K bits fit a 64-bit compare");
  static_assert(((N_R - K) & 3) == 3, "reverse phase of start j is 3 - (j & 3)");
  // A tile is INTERIOR when every byte a lane of it fetches holds bases of the genome: the last lane's window ends at
  // tile_start + (UNITS - 1) M + WIN (packed: WIN codes, and the bitmap word's bits up to the 64th matter only below
  // WIN) resp. + 4 (DW + 1) (ASCII), both <= tile_start + SPAN.  Its staging addresses are a scalar base plus a lane
  // constant, which rests on:
  static constexpr int SPAN = NB_T + WIN;           // a tile at tile_start is interior iff tile_start + SPAN <= n_bps
  static constexpr int PAR8 = (TILE % 8) / 4;       // 1: tile_start & 7 alternates between 0 and 4 from tile to tile
  static_assert(TILE % 4 == 0 && ITEM % 4 == 0, "a tile starts at a whole code byte and an aligned ASCII dword");
  static_assert(TILE % 8 == 0 || TILE % 8 == 4, "a tile starts at bit 0 or bit 4 of a bitmap byte");
  static_assert(4 * (DW + 1) <= WIN && (UNITS - 1) * M + WIN <= SPAN, "SPAN covers the last lane's fetches");
  static_assert(SPAN - (UNITS - 1) * M >= WIN && SPAN - (UNITS - 1) * M >= M, "no lane of an interior tile has a base behind the end in its window");
  static_assert(SPAN - K + 1 > (WG - 64) * M, "every wave of an interior tile has k-mer starts");
  typedef typename std::conditional<(WIN > 32), uint64_t, uint32_t>::type inv_t;  // validity bits of a code window
};
// (hg_kmer_tile_starts / hg_kmer_item_tiles give the host ONE geometry per code-window class)
template <int... Ks>
constexpr bool geos_one_geometry_per_class(std::integer_sequence<int, Ks...>) {
  return ((GeoS<Ks + 1>::TILE == GeoS<(Ks + 1 <= 21 ? 21 : 32)>::TILE && GeoS<Ks + 1>::TILES == GeoS<21>::TILES &&
           GeoS<Ks + 1>::SPAN == GeoS<(Ks + 1 <= 21 ? 21 : 32)>::SPAN) && ...);
}
static_assert(geos_one_geometry_per_class(std::make_integer_sequence<int, 32>{}), "TILE, TILES and SPAN depend on K only through WIN");

using lds_u8p = __attribute__((address_space(3))) const uint8_t *;
using lds_u16p = __attribute__((address_space(3))) const uint16_t *;
using lds_u32p = __attribute__((address_space(3))) const uint32_t *;
using glb_u8p = __attribute__((address_space(1))) const uint8_t *;
using glb_u32p = __attribute__((address_space(1))) const uint32_t *;
using glb_u32up = __attribute__((address_space(1))) const uint32_t __attribute__((aligned(1))) *;
using glb_u64up = __attribute__((address_space(1))) const uint64_t __attribute__((aligned(1))) *;

// ---- staging ---------------------------------------------------------------------------------------------------------
// A tile's scalar load base, as a global-memory pointer.  The empty statement pins it to a scalar register pair inside
// the tile loop: left alone, the compiler adds the lane's offset to the genome's base once per item instead and carries
// a 64-bit vector address that it advances per tile -- the arithmetic the interior front end is there to avoid.  With
// a 32-bit lane offset the loads take the form global_load v, v_off, s[base:base+1].  The lane offsets are constants of
// the lane, kept in io_seq / io_mask and passed through an empty statement at the top of every tile, so that what is
// carried from tile to tile is the 32-bit value and not its 64-bit extension.
__device__ __forceinline__ glb_u8p tile_base(const uint8_t *p) {
  uint64_t a = (uint64_t)(uintptr_t)p;
  asm volatile("" : "+s"(a));
  return (glb_u8p)a;
}
// "some base of this tile is not ACGT / lies behind the genome end" (wave-uniform branch; same value from every writer)
__device__ __forceinline__ void raise_dirty(bool dirty, uint32_t *flag) {
  if ((threadIdx.x & 63) == 0 || dirty) *flag = 1u;
}
// forward phase images of unit u: F_phi[DW u + t] = bytes [4 t + phi, 4 t + phi + 4) of the unit (+ lookahead)
template <int K>
__device__ __forceinline__ void store_forward_phases(uint32_t *s_f, uint32_t u, const uint32_t (&FA)[GeoS<K>::DW + 1]) {
  constexpr int DW = GeoS<K>::DW, S = GeoS<K>::S;
  uint32_t *const f0 = s_f + DW * u;
#pragma unroll
  for (int t = 0; t < DW; ++t) {
    f0[t] = FA[t];
    f0[S / 4 + t] = __builtin_amdgcn_alignbyte(FA[t + 1], FA[t], 1);
    f0[2 * (S / 4) + t] = __builtin_amdgcn_alignbyte(FA[t + 1], FA[t], 2);
    f0[3 * (S / 4) + t] = __builtin_amdgcn_alignbyte(FA[t + 1], FA[t], 3);
  }
}
// reverse phase images of unit u: the forward bytes [s, s + 4), s = 4 i + phi', complemented and byte-reversed, are dword
// j = JB(phi') - i of reverse phase psi = (N_R - phi') & 3, which lives at S (3 - psi).  X[t] carries the complements of
// the unit's dword t in the front end's own form, and rev(phi', X[i], X[i + 1]) makes the image dword of it.  (phi' is a
// compile-time constant, handed to rev as a type: with a run-time loop that the optimiser unrolls, the stores' address
// arithmetic compiled to other instructions than it had when both front ends carried this loop themselves.)
template <int K, class Rev>
__device__ __forceinline__ void store_reverse_phases(uint32_t *s_r, uint32_t u, const uint32_t (&X)[GeoS<K>::DW + 1], Rev rev) {
  constexpr int DW = GeoS<K>::DW, S = GeoS<K>::S, N_R = GeoS<K>::N_R;
  static_for(std::make_integer_sequence<int, 4>{}, [&](auto phc) {
    constexpr int ph = decltype(phc)::value, psi = (N_R - ph) & 3, JB = (N_R - 4 - psi - ph) / 4;
    uint32_t *const r0 = s_r + (3 - psi) * (S / 4) + JB - (int)(DW * u);
#pragma unroll
    for (int t = 0; t < DW; ++t) r0[-t] = rev(phc, X[t], X[t + 1]);
    // i = -1: the bytes in front of the tile do not exist; what follows them (the tile's first ph bases) does
    if (ph > 0 && u == 0) r0[1] = rev(phc, 0u, X[0]);
  });
}

// Stage unit u of the tile from ASCII: bases [M u, M u + M) at genome position P, one lookahead dword.  Two front ends: a
// lane of an INTERIOR tile (GeoS::SPAN) loads from the tile's scalar base plus its constant 32-bit offset io_seq and has
// no base behind the genome end; an edge tile does the arithmetic per lane.  Behind the loads they are the same code.
// Writes the unit's part of the phase images s_f / s_r, its 2-bit codes (s_code) and validity bits (s_val[u]).
// (io_seq, and io_mask below, are the kernel's own variables, taken by reference: they pass through an empty asm statement
// per tile -- see tile_base -- and as value arguments the packed kernels' tile loop compiled to four more instructions.)
template <int K, bool CANON, bool INTERIOR>
__device__ __forceinline__ void stage_unit(uint32_t u, uint64_t tile_start, const uint8_t *__restrict__ gseq, uint64_t n_bps,
                                           uint32_t u2t, const uint32_t &io_seq, uint32_t *s_f, uint32_t *s_r, uint8_t *s_code,
                                           uint32_t *s_val, uint32_t *dirty_flag) {
  using G = GeoS<K>;
  constexpr int M = G::M, DW = G::DW;
  const uint64_t P = tile_start + (uint64_t)u * M;
  uint32_t x[DW + 1];
  const int64_t rem64 = INTERIOR ? (int64_t)M : (int64_t)n_bps - (int64_t)P;  // bases of the genome from P on (interior: M or more)
  if constexpr (INTERIOR) {
    const glb_u32p src = (glb_u32p)(tile_base(gseq + tile_start) + io_seq);
#pragma unroll
    for (int t = 0; t <= DW; ++t) x[t] = src[t];
  } else if (rem64 + 32 >= 4 * (DW + 1)) {  // the caller provides 32 readable bytes behind every genome
    const uint32_t *src = reinterpret_cast<const uint32_t *>(gseq + P);
#pragma unroll
    for (int t = 0; t <= DW; ++t) x[t] = src[t];
  } else {
#pragma unroll
    for (int t = 0; t <= DW; ++t) {
      uint32_t w = 0;
      for (int bb = 0; bb < 4; ++bb) {
        const int64_t o = 4 * t + bb;
        w |= (uint32_t)(o < rem64 ? gseq[P + o] : (uint8_t)'N') << (8 * bb);
      }
      x[t] = w;
    }
  }
  if (u2t) {  // one uniform branch
#pragma unroll
    for (int t = 0; t <= DW; ++t) x[t] = u2t_rewrite(x[t]);
  }
  uint32_t FA[DW + 1], CA[DW + 1];
  uint32_t dacc = 0, codes = 0;
#pragma unroll
  for (int t = 0; t <= DW; ++t) {
    uint32_t cd;
    classify4(x[t], cd, FA[t], CA[t]);
    if (t < DW) {
      dacc |= (x[t] & 0xDFDFDFDFu) ^ FA[t];
      if (CANON) codes |= __builtin_amdgcn_udot4(cd, 0x40100401u, 0u, false) << (8 * t);  // c0 | c1<<2 | c2<<4 | c3<<6
    }
  }
  // validity of the unit's own M bases
  uint32_t inv = 0;
  const bool dirty = dacc != 0 || rem64 < M;
  if (__any(dirty)) {
#pragma unroll
    for (int t = 0; t < DW; ++t) inv |= ((((not_a_base4(x[t], FA[t]) >> 7) * 0x01020408u) >> 24) & 0xFu) << (4 * t);
    if (rem64 < M) inv |= rem64 <= 0 ? ~0u : (~0u << (uint32_t)rem64);
    inv &= (1u << M) - 1;
    raise_dirty(dirty, dirty_flag);
  }
  s_val[u] = inv;
  store_forward_phases<K>(s_f, u, FA);
  if constexpr (CANON) {
    // 2-bit codes: M / 4 bytes at byte M u / 4
#pragma unroll
    for (int t = 0; t < DW; ++t) s_code[DW * u + t] = (uint8_t)(codes >> (8 * t));
    // CA[t]: byte k = complement of base 4 t + k
    store_reverse_phases<K>(s_r, u, CA, [](auto phc, uint32_t lo, uint32_t hi) {
      constexpr uint32_t ph = decltype(phc)::value, sel = (ph + 3) | ((ph + 2) << 8) | ((ph + 1) << 16) | (ph << 24);
      return __builtin_amdgcn_perm(hi, lo, sel);
    });
  }
}

// Stage unit u of the tile from a hg_pack2 blob (include/hypergen.h: 2-bit codes, 4 bases per byte, then the not-a-base
// bitmap; 0.375 bytes per base in HBM instead of 1).  No classification at all: the lane fetches its whole 32- / 48-base
// code window (c0 = bases [P, P + 16): its own M bases + the lookahead dword; c1, c2 = the rest of its WIN-base window: the
// canonical compare's operand, as loaded) and the window's validity bits invw with two unaligned loads, and the forward /
// reverse-complement ASCII of four bases comes out of ONE 8-byte LDS table read indexed by the code byte (s_lut: 256
// entries x {ASCII, complement ASCII byte-reversed}) -- the pattern of the reference's second kernel
// (src/cuda_kernel.cu:15-69, NT4 codes from src/sketch_cuda.rs:23-32), not its data path.  Positions behind the genome end
// are invalid whatever the blob's padding says.
template <int K, bool CANON, bool INTERIOR>
__device__ __forceinline__ void stage_unit_packed(uint32_t u, uint64_t tile_start, const uint8_t *__restrict__ gseq,
                                                  const uint8_t *__restrict__ gmask, uint64_t n_bps, const uint32_t &io_seq,
                                                  const uint32_t &io_mask, uint32_t *s_f, uint32_t *s_r, const uint2 *s_lut,
                                                  uint32_t *dirty_flag, uint32_t &c0, uint32_t &c1, uint32_t &c2,
                                                  typename GeoS<K>::inv_t &invw) {
  using G = GeoS<K>;
  typedef typename G::inv_t inv_t;
  constexpr int M = G::M, DW = G::DW, WIN = G::WIN;
  if constexpr (INTERIOR) {
    // interior tile (GeoS::SPAN): P = tile_start + M u lies at code byte (tile_start >> 2) + 3 u and at bitmap bit
    // 4 q of byte tile_start >> 3, q = 3 u + (tile_start >> 2 & 1) -- scalar bases, 32-bit lane offsets, and no base of
    // the window lies behind the genome end
    const glb_u8p cp = tile_base(gseq + (tile_start >> 2)) + io_seq;
    c0 = *(glb_u32up)cp;
    c1 = *(glb_u32up)(cp + 4);
    c2 = WIN > 32 ? *(glb_u32up)(cp + 8) : 0u;
    const uint32_t q = 3u * u + (G::PAR8 ? (uint32_t)(tile_start >> 2) & 1u : 0u);
    const uint64_t mb = *(glb_u64up)(tile_base(gmask + (tile_start >> 3)) + (G::PAR8 ? q >> 1 : io_mask));
    const uint32_t sh = (q & 1u) << 2;
    if constexpr (WIN > 32) invw = (inv_t)(mb >> sh);
    else invw = __builtin_amdgcn_alignbit((uint32_t)(mb >> 32), (uint32_t)mb, sh);
  } else {
    typedef uint32_t __attribute__((aligned(1))) u32u;
    typedef uint64_t __attribute__((aligned(1))) u64u;
    const uint64_t P = tile_start + (uint64_t)u * M;  // a multiple of 4: whole code bytes
    const int64_t rem64 = (int64_t)n_bps - (int64_t)P;
    const uint64_t Pc = rem64 > 0 ? P : 0;            // (a window that starts behind the end reads the blob's first bytes: all invalid anyway)
    // the blob (codes padded to 16 bytes + >= 16 bytes of bitmap) and the 32 readable bytes the caller leaves behind it cover
    // every byte fetched here
    const uint8_t *cp = gseq + (Pc >> 2);
    c0 = *reinterpret_cast<const u32u *>(cp);
    c1 = *reinterpret_cast<const u32u *>(cp + 4);
    c2 = WIN > 32 ? *reinterpret_cast<const u32u *>(cp + 8) : 0u;
    const uint64_t mb = *reinterpret_cast<const u64u *>(gmask + (Pc >> 3));
    invw = (inv_t)(mb >> (uint32_t)(Pc & 7));
    if (rem64 < WIN) invw |= rem64 <= 0 ? ~(inv_t)0 : (inv_t)(~(inv_t)0 << (uint32_t)rem64);
  }
  const bool dirty = invw != 0;
  if (__any(dirty)) raise_dirty(dirty, dirty_flag);
  uint32_t FA[DW + 1], RW[DW + 1];  // RW[t]: byte k = complement of base 4 t + 3 - k
#pragma unroll
  for (int t = 0; t <= DW; ++t) {
    const uint2 e = s_lut[(c0 >> (8 * t)) & 0xFFu];
    FA[t] = e.x, RW[t] = e.y;
  }
  store_forward_phases<K>(s_f, u, FA);
  if constexpr (CANON) {
    // dword JB - (DW u + t) of phase psi holds the complements of bases 4 t + ph + 3 .. 4 t + ph -- bytes [4 - ph, 8 - ph) of
    // {RW[t] : RW[t + 1]}
    store_reverse_phases<K>(s_r, u, RW, [](auto phc, uint32_t lo, uint32_t hi) {
      constexpr int ph = decltype(phc)::value;
      return ph == 0 ? lo : __builtin_amdgcn_alignbyte(lo, hi, 4 - ph);
    });
  }
}

// ---- the code window and the strand choice ---------------------------------------------------------------------------
// A lane's code window: WIN bases from its first start on, two bits each.  LSB-first complement stream (read upwards it IS
// the reverse strand) and MSB-first forward stream (base 0 in the top two bits), as 64-bit values (WIN = 32: Gc, Gm) or
// dwords (WIN = 48: wc, gf)
struct CodeWindow {
  uint64_t Gm = 0, Gc = 0;
  uint32_t gf[3] = {0, 0, 0}, wc[3] = {0, 0, 0};
};
// from the window's codes as loaded: base b at bits 2 b .. 2 b + 1 of {wl, wh, w2}
template <int K>
__device__ __forceinline__ CodeWindow code_window(uint32_t wl, uint32_t wh, uint32_t w2) {
  CodeWindow w;
  auto pairrev = [](uint32_t v) {
    const uint32_t br = __builtin_bitreverse32(v);
    return ((br >> 1) & 0x55555555u) | ((br & 0x55555555u) << 1);
  };
  if constexpr (GeoS<K>::WIN == 32) {
    w.Gc = ~mk64(wl, wh);
    w.Gm = mk64(pairrev(wh), pairrev(wl));
  } else {
    w.wc[0] = ~wl, w.wc[1] = ~wh, w.wc[2] = ~w2;
    w.gf[0] = pairrev(wl), w.gf[1] = pairrev(wh), w.gf[2] = pairrev(w2);
  }
  return w;
}

// the chosen strand's base address for k-mer jj (aF: forward, aR[jj >> 2]: reverse complement): forward < reverse
// complement as one compare of 2-bit codes (32-bit for odd K, 64-bit for even K)
template <int K, bool CANON, int jj>
__device__ __forceinline__ uint32_t strand_base(const CodeWindow &cw, uint32_t aF, const uint32_t (&aR)[GeoS<K>::M / 4]) {
  constexpr int WIN = GeoS<K>::WIN;
  const uint64_t Gm = cw.Gm, Gc = cw.Gc;
  const uint32_t(&gf)[3] = cw.gf, (&wc)[3] = cw.wc;
  uint32_t base = aF;
  if constexpr (CANON && (K & 1) != 0) {
    // odd K: the TOP dwords decide -- the first 16 bases of the forward k-mer against the first 16 of its reverse
    // complement.  They always differ: base (K - 1) / 2 (<= 15) is the middle of both strands, code c on one and
    // 3 - c on the other (the complement is the bitwise NOT of the code, whatever the byte was).  So the 64-bit shifts
    // and compare of the whole values reduce to one v_alignbit per strand (none where the shift is 0) and a 32-bit
    // compare.
    uint32_t fh, rh;
    if constexpr (WIN == 32) {
      // top dwords of Gm << 2 jj and Gc << 2 (32 - K - jj)
      constexpr int SF = 2 * jj, SR = 2 * (32 - K - jj);
      const uint32_t gmh = (uint32_t)(Gm >> 32), gml = (uint32_t)Gm, gch = (uint32_t)(Gc >> 32), gcl = (uint32_t)Gc;
      fh = SF == 0 ? gmh : __builtin_amdgcn_alignbit(gmh, gml, 32 - SF);
      if constexpr (SR == 0) rh = gch;
      else if constexpr (SR < 32) rh = __builtin_amdgcn_alignbit(gch, gcl, 32 - SR);
      else rh = gcl << (SR - 32);  // (K < 16)
    } else {
      // 96-bit streams: the MSB-first forward stream from bit 2 jj (from the top); bits [e + 32, e + 64) of the LSB-first
      // complement stream, e = 2 jj + 2 K - 64 (zeros below bit 0)
      constexpr int o = 2 * jj;
      fh = o == 0 ? gf[0] : __builtin_amdgcn_alignbit(gf[0], gf[1], 32 - o);
      constexpr int e = 2 * jj + 2 * K - 64, off = e + 32, a = off >> 5, sft = off & 31;
      static_assert(off >= 0 && a <= 1, "window inside [0, wc0, wc1, wc2]");
      const uint32_t x_[4] = {0u, wc[0], wc[1], wc[2]};
      rh = sft == 0 ? x_[a + 1] : __builtin_amdgcn_alignbit(x_[a + 2], x_[a + 1], sft);
    }
    uint64_t lt;
    asm("v_cmp_lt_u32_e64 %0, %1, %2" : "=s"(lt) : "v"(rh), "v"(fh));
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(base) : "v"(aF), "v"(aR[jj >> 2]), "s"(lt));
  } else if constexpr (CANON) {
    // even K: the whole 2 K bits, bottom-aligned (WIN = 32) or top-aligned with what lies below them cut off
    uint64_t fv, rv;
    if constexpr (WIN == 32) {
      constexpr uint64_t MASK2K = (1ull << (2 * K)) - 1;
      fv = (Gm >> (2 * (32 - K - jj))) & MASK2K;
      rv = (Gc >> (2 * jj)) & MASK2K;
    } else {
      // 96-bit streams: both values TOP-aligned in 64 bits.  Forward: the MSB-first stream from bit 2 jj (from the
      // top).  Reverse: bits [e, e + 64) of the LSB-first complement stream, e = 2 jj + 2 K - 64 (zeros below
      // bit 0).
      constexpr int o = 2 * jj;
      uint32_t fh, fl;
      if constexpr (o == 0) fh = gf[0], fl = gf[1];
      else fh = __builtin_amdgcn_alignbit(gf[0], gf[1], 32 - o), fl = __builtin_amdgcn_alignbit(gf[1], gf[2], 32 - o);
      constexpr int e = 2 * jj + 2 * K - 64, off = e + 32, a = off >> 5, sft = off & 31;
      static_assert(off >= 0 && a <= 1, "window inside [0, wc0, wc1, wc2]");
      const uint32_t x_[4] = {0u, wc[0], wc[1], wc[2]};
      uint32_t rl, rh;
      if constexpr (sft == 0) rl = x_[a], rh = x_[a + 1];
      else rl = __builtin_amdgcn_alignbit(x_[a + 1], x_[a], sft), rh = __builtin_amdgcn_alignbit(x_[a + 2], x_[a + 1], sft);
      if constexpr (K < 32) {
        constexpr uint32_t LOWCUT = ~((1u << (64 - 2 * K)) - 1u);
        fl &= LOWCUT, rl &= LOWCUT;
      }
      fv = mk64(fl, fh), rv = mk64(rl, rh);
    }
    uint64_t lt;
    asm("v_cmp_lt_u64_e64 %0, %1, %2" : "=s"(lt) : "v"(rv), "v"(fv));
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(base) : "v"(aF), "v"(aR[jj >> 2]), "s"(lt));
  }
  return base;
}

// ---- the kernel ------------------------------------------------------------------------------------------------------
template <int K, bool CANON, bool PACKED>
__global__ __launch_bounds__(WG) void kmer_sample_shared(
    const uint8_t *__restrict__ seq, const hg_genome_meta *__restrict__ meta,
    const uint32_t *__restrict__ item_genome, uint64_t threshold, uint64_t seed, uint32_t u2t,
    uint64_t *__restrict__ hits, uint32_t *__restrict__ cnt, uint32_t stage_cap, const uint32_t *__restrict__ group_first) {
  using G = GeoS<K>;
  typedef typename G::inv_t inv_t;
  constexpr int M = G::M, DW = G::DW, S = G::S, ND = G::ND, NB = G::NB, NW = G::NW, N_R = G::N_R, WIN = G::WIN;
  constexpr inv_t MASKK = (inv_t)(((uint64_t)1 << K) - 1);

  // A workgroup takes the work items [item_lo, item_hi) one after the other: ONE item of a genome that fills it (TILES
  // tiles), or the items of several consecutive SMALL genomes, TILES tiles between them (the host's plan groups them:
  // hg_sketch_plan.hip) -- a genome of a few kbp is one or two tiles, and a workgroup of its own paid the launch, the
  // dependent loads of its records and the table set-up below for 6 us of hashing.
  const uint32_t tid = threadIdx.x;
  const uint32_t item_lo = group_first ? group_first[blockIdx.x] : blockIdx.x;
  const uint32_t item_hi = group_first ? group_first[blockIdx.x + 1] : blockIdx.x + 1;
  uint32_t g = 0;
  hg_genome_meta gm{};
  uint64_t n_bps = 0, n_starts = 0, item_start = 0;
  const uint8_t *__restrict__ gseq = seq, *__restrict__ gmask = seq;
  uint32_t tile_no = 0;  // tiles this workgroup has done (parity of the "dirty" flags)

  __shared__ HitStage stage;
  __shared__ __attribute__((aligned(16))) uint32_t s_f[4 * S / 4];                 // forward phase images
  __shared__ __attribute__((aligned(16))) uint32_t s_r[CANON ? 4 * S / 4 : 4];     // reverse phase images (psi at S (3 - psi))
  __shared__ __attribute__((aligned(16))) uint8_t s_code[(CANON && !PACKED) ? G::NB_T / 4 + 16 : 16];  // 2-bit codes, base b at bits 2b..2b+1
  __shared__ uint32_t s_val[PACKED ? 4 : G::UNITS + 4];   // per unit of M bases: bit b set <=> base b cannot be part of a k-mer
  __shared__ uint32_t s_dirty[2];            // "some base of this tile is not ACGT / lies behind the genome end", by tile parity
  __shared__ __attribute__((aligned(8))) uint2 s_lut[PACKED ? 256 : 1];  // code byte -> {ASCII of its 4 bases, complement ASCII byte-reversed}
  if (tid == 0) stage.n = 0, s_dirty[0] = 0, s_dirty[1] = 0;
  if constexpr (!PACKED) {
    if (tid < 4) s_val[G::UNITS + tid] = 0;
  } else {
    static_assert(WG == 256, "one table entry per lane");
    uint32_t f = 0, r = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t cd = (tid >> (2 * b)) & 3u;
      f |= ((0x54474341u >> (8 * cd)) & 0xFFu) << (8 * b);        // "ACGT"[code]
      r |= ((0x41434754u >> (8 * cd)) & 0xFFu) << (8 * (3 - b));  // "TGCA"[code], base b at byte 3 - b
    }
    s_lut[tid] = make_uint2(f, r);
  }
  __syncthreads();

  // per-lane read bases (they do not depend on the tile) and staging offsets (tile_base)
  const uint32_t aF = (uint32_t)(uintptr_t)(lds_u8p)(reinterpret_cast<const uint8_t *>(s_f)) + M * tid;
  uint32_t aR[M / 4];
#pragma unroll
  for (int gq = 0; gq < M / 4; ++gq)
    aR[gq] = (uint32_t)(uintptr_t)(lds_u8p)(reinterpret_cast<const uint8_t *>(s_r)) + 4u * ((uint32_t)(N_R - K) >> 2) - M * tid - 8u * gq;
  uint32_t io_seq = (PACKED ? 3u : (uint32_t)M) * tid;  // the lane's unit from the tile's base: code bytes / ASCII bytes
  uint32_t io_mask = (3u * tid) >> 1;                   // its bitmap byte, in a tile that starts at bit 0 of one

  // (the next item's records are requested while this one is hashed: two dependent scalar loads otherwise in front of
  // every small genome)
  uint32_t g_next = item_genome[item_lo];
  hg_genome_meta gm_next = meta[g_next];
#pragma unroll 1
  for (uint32_t item = item_lo; item < item_hi; ++item) {
    g = g_next;
    gm = gm_next;
    if (item + 1 < item_hi) {
      g_next = item_genome[item + 1];
      gm_next = meta[g_next];
    }
    n_bps = gm.n_bps;
    if (n_bps < (uint64_t)K) continue;  // (uniform; such a genome has no work item anyway)
    n_starts = n_bps - K + 1;
    gseq = seq + gm.seq_off;
    gmask = seq + gm.mask_off;
    item_start = (uint64_t)(item - gm.item_first) * G::ITEM;
    // (uniform; the plan makes no item behind the last start.  One of a foreign plan that does lie there has no tile and
    // stages no hit, so it also skips the flush of an empty list at the loop's end, like the genome shorter than K above; the
    // subtraction below must not wrap into "interior")
    if (item_start >= n_starts) continue;
    // bases from the item's start to the genome's end, saturated: tile t of the item is interior iff t TILE + SPAN <= item_rem
    const uint64_t item_rem64 = n_bps - item_start;
    const uint32_t item_rem = (item_rem64 >> 32) != 0 ? ~0u : (uint32_t)item_rem64;
#pragma unroll 1
    for (int tile = 0; tile < G::TILES; ++tile, ++tile_no) {
      const uint64_t tile_start = item_start + (uint64_t)tile * G::TILE;
      if ((uint32_t)tile * (uint32_t)G::TILE + (uint32_t)(K - 1) >= item_rem) break;  // tile_start >= n_starts; uniform
      const uint32_t par = tile_no & 1u;

      // ---- stage: every lane its unit.  An interior tile (scalar test) takes the front end without address or tail
      // arithmetic, and all its waves stage and hash.  In an edge tile, a wave whose units all lie behind everything a live
      // lane's window can reach -- the last k-mer start + WIN bases -- stages nothing (wave-uniform; its slots of the images
      // keep what an earlier tile left there and nobody reads them), and a wave whose 64 x M starts all lie behind the
      // genome's last k-mer hashes nothing: a 2 kbp genome fills three of its one tile's four waves, the last tile of a
      // 10 kbp genome two -- the idle wave only meets the others at the barriers, and its issue slots go to the other
      // workgroups of the CU (2 kbp genomes: 0.27 -> 0.4 of the per-base rate).
      uint32_t pc0 = 0, pc1 = 0, pc2 = 0;
      inv_t pinv = 0;
      asm volatile("" : "+v"(io_seq), "+v"(io_mask));
      const bool interior = (uint32_t)tile * (uint32_t)G::TILE + (uint32_t)G::SPAN <= item_rem;
      bool wave_live = true;
      if (interior) {
        if constexpr (PACKED) stage_unit_packed<K, CANON, true>(tid, tile_start, gseq, gmask, n_bps, io_seq, io_mask, s_f, s_r, s_lut, &s_dirty[par], pc0, pc1, pc2, pinv);
        else stage_unit<K, CANON, true>(tid, tile_start, gseq, n_bps, u2t, io_seq, s_f, s_r, s_code, s_val, &s_dirty[par]);
      } else {
        const uint64_t wave_start = tile_start + (uint64_t)(tid & ~63u) * M;
        if (wave_start < n_starts + (uint64_t)WIN) {
          if constexpr (PACKED) stage_unit_packed<K, CANON, false>(tid, tile_start, gseq, gmask, n_bps, io_seq, io_mask, s_f, s_r, s_lut, &s_dirty[par], pc0, pc1, pc2, pinv);
          else stage_unit<K, CANON, false>(tid, tile_start, gseq, n_bps, u2t, io_seq, s_f, s_r, s_code, s_val, &s_dirty[par]);
        }
        wave_live = wave_start < n_starts;
      }
      __syncthreads();

      // ---- window: the validity bits (read only where the tile has any set) and the 2-bit codes of the lane's WIN bases
      const bool tile_dirty = s_dirty[par] != 0u;  // workgroup-uniform
      inv_t inv_w = 0;
      if constexpr (PACKED) {
        if (tile_dirty) inv_w = pinv;
      } else if (tile_dirty) {
        if constexpr (WIN > 32)
          inv_w = (inv_t)((uint64_t)s_val[tid] | ((uint64_t)s_val[tid + 1] << M) | ((uint64_t)s_val[tid + 2] << (2 * M)) |
                          ((uint64_t)s_val[tid + 3] << (3 * M)));
        else
          inv_w = (inv_t)(s_val[tid] | (s_val[tid + 1] << M) | (s_val[tid + 2] << (2 * M)));
      }
      CodeWindow cw;
      if constexpr (CANON) {
        uint32_t wl, wh, w2 = 0;
        if constexpr (PACKED) {
          wl = pc0, wh = pc1, w2 = pc2;  // the window as loaded
        } else {  // from bit 2 M tid = byte (M / 4) tid of the code image
          const uint32_t bo = (uint32_t)DW * tid;
          const uint32_t *cp = reinterpret_cast<const uint32_t *>(s_code) + (bo >> 2);
          const uint32_t c0 = cp[0], c1 = cp[1], c2 = cp[2], sh = 8u * (bo & 3u);
          wl = __builtin_amdgcn_alignbit(c1, c0, sh), wh = __builtin_amdgcn_alignbit(c2, c1, sh);
          if constexpr (WIN > 32) w2 = __builtin_amdgcn_alignbit(cp[3], c2, sh);
        }
        cw = code_window<K>(wl, wh, w2);
      }

      // ---- hash the lane's M starts.  CHECK: the tile has bytes that are no bases, and a k-mer with one in its window
      // (inv_w) is dropped.  The two loops stay lambdas of the kernel: as function templates they compile to other code.
      const bool hashing = tid < (uint32_t)(WG - G::LOOK_UNITS);  // (the last lanes' windows leave the staged area)
      // k = 17..32: the statements of hg_kmer_asm.h, which lists the local names they use.  FB: the first mixup's bounded text
      uint64_t w0a = 0, w0b = 0, w0c = 0, w0d = 0, w1a = 0, w1b = 0, w1c = 0, w1d = 0;
      uint64_t hmask = 0, hjunk = 0;
      uint32_t hlo0 = 0, hlo1 = 0, hhi = 0;
      uint64_t zpair = 0;  // every asm statement rewrites its low half only, so the zero in the high half is carried as a value
      constexpr int KCASE = 10 * ND + NB;
      auto kmers_asm = [&](auto checkc, auto boundedc) __attribute__((always_inline)) {
        constexpr bool CHECK = decltype(checkc)::value;
        constexpr bool FB = decltype(boundedc)::value;
        if constexpr (NW >= 3) {
          {
            const uint32_t base = strand_base<K, CANON, 0>(cw, aF, aR);
            constexpr int IMM = 0;
            HG_KS_ALL_CASES(HG_KS_FIRST)
          }
          static_for(std::make_integer_sequence<int, M>{}, [&](auto jc) {
            constexpr int j = decltype(jc)::value;
            const bool valid = !CHECK || ((inv_w >> j) & MASKK) == 0;
            if constexpr (j + 1 < M) {
              const uint32_t base = strand_base<K, CANON, j + 1>(cw, aF, aR);
              constexpr int IMM = S * ((j + 1) & 3) + 4 * ((j + 1) >> 2);
              if constexpr ((j & 1) == 0) {
                HG_KS_ALL_CASES(HG_KS_EVEN)
              } else {
                HG_KS_ALL_CASES(HG_KS_ODD)
              }
            } else {
              static_assert((M & 1) == 0, "the last k-mer's words are in the parity-1 buffer");
              HG_KS_ALL_CASES(HG_KS_LAST)
            }
            if (hmask != 0) {  // wave-uniform: some lane is a candidate (1 k-mer in `scaled`); the exact test
              const uint64_t h = mk64(hlo0 ^ hlo1, hhi);
              if (h < threshold && valid && hashing) stage_hit(stage, stage_cap, h, gm, g, hits, cnt);
            }
          });
        }
      };
      // k <= 16: the compiler's code for t1ha2_fixed_w; the words of k-mer j + 1 are fetched in front of the hash of k-mer j
      auto fetch_words = [&](auto jjc, uint64_t *w) __attribute__((always_inline)) {
        constexpr int jj = decltype(jjc)::value;
        const uint32_t base = strand_base<K, CANON, jj>(cw, aF, aR);
        constexpr int IMM = S * (jj & 3) + 4 * (jj >> 2);
        const lds_u32p src = (lds_u32p)(uintptr_t)(base + (uint32_t)IMM);
        uint32_t d[2 * NW];
#pragma unroll
        for (int m = 0; m < 2 * NW; ++m) {
          if (m < ND - 1 || (m == ND - 1 && NB == 4)) d[m] = src[m];
          else if (m == ND - 1 && NB == 1) d[m] = *(lds_u8p)(uintptr_t)(base + (uint32_t)(IMM + 4 * m));
          else if (m == ND - 1 && NB == 2) d[m] = *(lds_u16p)(uintptr_t)(base + (uint32_t)(IMM + 4 * m));
          else if (m == ND - 1) d[m] = src[m] & 0xFFFFFFu;
          else d[m] = 0;
        }
#pragma unroll
        for (int m = 0; m < NW; ++m) w[m] = mk64(d[2 * m], d[2 * m + 1]);
      };
      uint64_t wq[2][NW];
      auto run_kmers = [&](auto checkc) __attribute__((always_inline)) {
        constexpr bool CHECK = decltype(checkc)::value;
        if constexpr (NW <= 2) {
          static_for(std::make_integer_sequence<int, M>{}, [&](auto jc) {
            constexpr int j = decltype(jc)::value;
            const bool valid = !CHECK || ((inv_w >> j) & MASKK) == 0;
            if constexpr (j == 0) fetch_words(jc, wq[0]);
            if constexpr (j + 1 < M) fetch_words(std::integral_constant<int, j + 1>{}, wq[(j + 1) & 1]);
            const uint64_t h = t1ha2_fixed_w<K>(wq[j & 1], seed);
            if (valid && hashing && h < threshold) stage_hit(stage, stage_cap, h, gm, g, hits, cnt);
          });
        }
      };
      if (wave_live) {
        if constexpr (NW >= 3) {  // K = 17..32
          // The first mixup's bounded text holds for every seed where its s is K (K >= 25) and for seeds below
          // FIRST_SEED_END where s is the seed (K <= 24); a larger seed takes the general text.  A scalar test of the kernel
          // argument once per tile and a second pair of loop copies in the K <= 24 kernels -- not an instantiation picked at
          // launch: the set of compiled kernels, their names and the launch table stay what they are, the object grows by
          // the same two loop copies either way, and the test costs a scalar compare and branch per 3 048 k-mers.
          constexpr bool ANY_SEED = NW == 4;  // one text serves every seed
          if (ANY_SEED || seed < FIRST_SEED_END) {
            if (!tile_dirty) kmers_asm(std::false_type{}, std::true_type{});
            else kmers_asm(std::true_type{}, std::true_type{});
          } else if constexpr (!ANY_SEED) {
            if (!tile_dirty) kmers_asm(std::false_type{}, std::false_type{});
            else kmers_asm(std::true_type{}, std::false_type{});
          }
        } else {
          if (!tile_dirty) run_kmers(std::false_type{});
          else run_kmers(std::true_type{});
        }
      }
      __syncthreads();  // every read of the images is done: the next tile may overwrite them
      if (tid == 0) s_dirty[par] = 0u;  // (raised again in two tiles' time at the earliest, behind the next tile's barriers)
      // (the staged count is workgroup-uniform behind the barrier above)
      if (dense_sampling(threshold)) flush_hits_if_filling(stage, stage_cap, gm, g, hits, cnt);
    }
    // the item's hits to its genome's region (the list is empty again for the next item of the group: its first tile's
    // barrier lies between this call's reads of the list and the next writes)
    if (item + 1 < item_hi) flush_hits<true>(stage, stage_cap, gm, g, hits, cnt);
    else flush_hits(stage, stage_cap, gm, g, hits, cnt);
  }
}
}  // namespace
