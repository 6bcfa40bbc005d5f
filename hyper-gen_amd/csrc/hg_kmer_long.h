// hg_kmer_long.h -- kmer_sample_long: the k-mer kernel for k = 33..255 (the CPU path's t1ha2 long-input loop;
// src/cuda_kernel.cu has none).  Included by hg_kmer_kernels.hip only.  Expects: WG, GEN_ITEM (the .hip), hg_kmer_t1ha2.h
// (LdsStrand, t1ha2_long), hg_kmer_bases.h, hg_kmer_hits.h.
#pragma once
namespace {

// A workgroup stages 2 048 bytes of sequence per tile -- 1 536 k-mer starts and the up to 254 bytes behind the last one --
// into LDS as the normalised forward strand (upper-case ASCII, 0 for anything that is not a base) and its reverse
// complement (so that the reverse strand of a k-mer is an ascending byte range too), each in all four byte phases (image
// phi holds bytes [4 i + phi, 4 i + phi + 4) at dword i: every dword of a k-mer that starts at ANY byte is one aligned read
// of the image of its start's phase -- the pattern of kmer_sample_shared), plus one validity bit per byte.  A lane stages
// eight bytes: it loads them with the dword in front and the dword behind (16 bytes), classifies all four dwords, and
// writes its two dwords of all eight images itself -- the forward phases need the NEXT dword, the reverse-complement phases
// the PREVIOUS one -- so a tile has two barriers and no pass over LDS (DESIGN.md has what the five-barrier form cost).
// Each lane then takes six starts.  KC = 0: run-time k (65..255).  KC = 33..64: k is a compile-time constant -- the validity
// test is two funnel shifts on the bit image, the strand choice one 64-bit compare of the first eight bases (the byte
// strings differ there for all but one k-mer in 65 536), and t1ha2 is straight-line code: one round of its 32-byte loop
// (two for k = 64) and a tail of k - 32 bytes.
constexpr uint32_t LONG_TILE = 1536;                 // k-mer starts per tile (6 per lane)
constexpr uint32_t LONG_BYTES = 2048;                // staged bytes per tile (>= LONG_TILE + 254), 8 per lane
// dwords between two phase images: the tile + slack.  Consecutive lanes take consecutive starts, so a wave reads 16
// consecutive dwords of each of the four images at once; with the images 16 banks apart (pitch == 16 mod 32) every LDS bank
// serves exactly two lanes, with 516 dwords (pitch 4) up to four.  Measured at k = 33: 18.4 against 18.1 ms -- no gain, the
// kernel is VALU-bound (SQ_LDS_BANK_CONFLICT is 61 % of its LDS cycles either way, the LDS is busy 59 % of the time); 16 it
// is.  An A/B of this pitch, of the clean-tile shortcut (tile_dirty), of the cached first dwords (LdsStrand) or of the
// k-mer loop left rolled is a build of the parent commit with that line changed (tools/build_variant.sh).
constexpr uint32_t LONG_DW = LONG_BYTES / 4 + 16;
static_assert(GEN_ITEM % LONG_TILE == 0 && LONG_TILE % 8 == 0 && LONG_BYTES == 8 * WG && LONG_TILE + 254 <= LONG_BYTES, "long-k tile geometry");

// four bases as ASCII -> {normalised forward ASCII, complement ASCII, invalid bytes as 0xFF}; bytes that are not a base
// (after the optional u/U -> T) are 0 in both strands
__device__ __forceinline__ void long_classify_ascii(uint32_t x, uint32_t u2t, uint32_t &fa, uint32_t &ca, uint32_t &bad) {
  if (u2t) x = u2t_rewrite(x);
  uint32_t cd, f, c;
  classify4(x, cd, f, c);
  bad = (not_a_base4(x, f) >> 7) * 0xFFu;
  fa = f & ~bad, ca = c & ~bad;
}
// four bases as 2-bit codes (low byte of `codes`) + their four not-a-base bits
__device__ __forceinline__ void long_classify_codes(uint32_t codes, uint32_t inv4, uint32_t &fa, uint32_t &ca, uint32_t &bad) {
  const uint32_t cd = (codes & 3u) | ((codes & 0xCu) << 6) | ((codes & 0x30u) << 12) | ((codes & 0xC0u) << 18);
  bad = (((inv4 & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu;
  fa = __builtin_amdgcn_perm(0u, 0x54474341u, cd) & ~bad;
  ca = __builtin_amdgcn_perm(0u, 0x41434754u, cd) & ~bad;
}

template <int KC, bool PACKED>  // (PACKED last: a profiler's name of a packed-input kernel ends in "true>" for both kernels)
__global__ __launch_bounds__(WG) void kmer_sample_long(
    const uint8_t *__restrict__ seq, const hg_genome_meta *__restrict__ meta,
    const uint32_t *__restrict__ item_genome, uint32_t ksize_rt, uint64_t threshold, uint64_t seed,
    uint32_t canonical, uint32_t u2t, uint64_t *__restrict__ hits, uint32_t *__restrict__ cnt, uint32_t stage_cap) {
  __shared__ HitStage stage;
  __shared__ uint32_t s_f[4 * LONG_DW], s_rc[4 * LONG_DW];  // forward / reverse-complement strand, four byte phases each
  __shared__ uint32_t s_inv[LONG_BYTES / 32 + 12];          // bit i set <=> staged byte i is not a base (zero slack behind)
  __shared__ uint32_t s_anybad[2];                          // "this tile holds a byte that is not a base", by tile parity
  const uint32_t ksize = KC ? (uint32_t)KC : ksize_rt;
  const uint32_t item = blockIdx.x, tid = threadIdx.x;
  const uint32_t g = item_genome[item];
  const hg_genome_meta gm = meta[g];
  const uint64_t n_bps = gm.n_bps;
  if (n_bps < ksize) return;
  const uint64_t n_starts = n_bps - ksize + 1;
  const uint8_t *__restrict__ gseq = seq + gm.seq_off;
  const uint8_t *__restrict__ gmask = seq + gm.mask_off;  // PACKED: the genome's not-a-base bitmap
  const uint64_t item_start = (uint64_t)(item - gm.item_first) * GEN_ITEM;
  if (tid == 0) stage.n = 0;
  if (tid < 4) s_f[tid * LONG_DW + LONG_BYTES / 4] = 0u, s_rc[tid * LONG_DW + LONG_BYTES / 4] = 0u;  // (read by a k-mer's last, masked dword)
  if (tid < 12) s_inv[LONG_BYTES / 32 + tid] = 0u;
  if (tid < 2) s_anybad[tid] = 0u;
  typedef uint32_t __attribute__((aligned(1))) u32u_t;
  uint32_t tile_par = 0;

  for (uint64_t tile0 = item_start; tile0 < item_start + GEN_ITEM && tile0 < n_starts; tile0 += LONG_TILE, tile_par ^= 1u) {
    __syncthreads();  // previous tile's readers are done
    if (tid == 0) s_anybad[tile_par ^ 1u] = 0u;  // (the flag of the tile before: read by everyone in front of the barrier above)
    if (dense_sampling(threshold)) flush_hits_if_filling(stage, stage_cap, gm, g, hits, cnt);
    // ---- stage: the lane's eight bytes [pos0, pos0 + 8) with the four bytes in front of and behind them
    {
      const uint64_t pos0 = tile0 + (uint64_t)tid * 8;  // a multiple of 8
      uint32_t fa[4], ca[4], bad[4];                     // dwords at pos0 - 4, pos0, pos0 + 4, pos0 + 8
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int64_t q = (int64_t)pos0 + 4 * t - 4;    // first base of this dword
        fa[t] = ca[t] = 0u, bad[t] = ~0u;
        if (q >= 0 && (uint64_t)q < n_bps) {             // (the caller leaves 32 readable bytes behind every genome)
          if constexpr (PACKED) {
            const uint32_t codes = gseq[(uint64_t)q >> 2];  // q is a multiple of 4: one code byte
            const uint32_t inv4 = (uint32_t)gmask[(uint64_t)q >> 3] >> ((uint32_t)q & 4u);
            long_classify_codes(codes, inv4, fa[t], ca[t], bad[t]);
          } else {
            long_classify_ascii(*reinterpret_cast<const u32u_t *>(gseq + q), u2t, fa[t], ca[t], bad[t]);
          }
          const uint64_t left = n_bps - (uint64_t)q;     // bases of the genome from q on: what lies behind them is not sequence
          if (left < 4) {
            const uint32_t keep = (1u << (8 * (uint32_t)left)) - 1u;
            fa[t] &= keep, ca[t] &= keep, bad[t] |= ~keep;
          }
        }
      }
      // forward images: dwords 2 tid and 2 tid + 1 of every phase
#pragma unroll
      for (uint32_t ph = 0; ph < 4; ++ph) {
        s_f[ph * LONG_DW + 2 * tid] = ph ? __builtin_amdgcn_alignbyte(fa[2], fa[1], ph) : fa[1];
        s_f[ph * LONG_DW + 2 * tid + 1] = ph ? __builtin_amdgcn_alignbyte(fa[3], fa[2], ph) : fa[2];
      }
      // reverse complement: byte LONG_BYTES - 1 - i holds the complement of forward byte i, so forward dword f is dword
      // LONG_BYTES / 4 - 1 - f byte-reversed, and its successor in the image is the forward dword IN FRONT of it
      const uint32_t r0 = __builtin_bswap32(ca[0]), r1 = __builtin_bswap32(ca[1]), r2 = __builtin_bswap32(ca[2]);
      const uint32_t j1 = LONG_BYTES / 4 - 1 - 2 * tid;  // image dword of forward dword 2 tid (j1 - 1: of 2 tid + 1)
#pragma unroll
      for (uint32_t ph = 0; ph < 4; ++ph) {
        s_rc[ph * LONG_DW + j1] = ph ? __builtin_amdgcn_alignbyte(r0, r1, ph) : r1;
        s_rc[ph * LONG_DW + j1 - 1] = ph ? __builtin_amdgcn_alignbyte(r1, r2, ph) : r2;
      }
      // validity bits of the lane's eight bytes: byte tid of the bit image
      const uint32_t b8 = ((((bad[1] & 0x01010101u) * 0x01020408u) >> 24) & 15u) | (((((bad[2] & 0x01010101u) * 0x01020408u) >> 24) & 15u) << 4);
      reinterpret_cast<uint8_t *>(s_inv)[tid] = (uint8_t)b8;
      if (b8 != 0u) s_anybad[tile_par] = 1u;  // (same value from every writer)
    }
    __syncthreads();
    const bool tile_dirty = s_anybad[tile_par] != 0u;  // workgroup-uniform: a clean tile (nearly all of them) tests no window
    // ---- the lane's six starts p = tid + 256 j.  256 is a multiple of 4, so the byte phase of a lane's starts is the same for
    // all j on both strands and the k-mer's first dword moves by 64 dwords per j: two pointers that step, no address arithmetic
    // per start (forward: byte p; reverse complement: byte LONG_BYTES - p - k)
    const uint64_t left_starts = n_starts - tile0;  // > 0
    const uint32_t lim = left_starts < LONG_TILE ? (uint32_t)left_starts : LONG_TILE;
    const uint32_t jn = lim > tid ? (lim - tid + WG - 1) / WG : 0u;  // this lane's starts inside the genome
    const uint32_t rb0 = LONG_BYTES - ksize - tid;
    const uint32_t *fp = s_f + (tid & 3u) * LONG_DW + (tid >> 2);
    const uint32_t *rp = s_rc + (rb0 & 3u) * LONG_DW + (rb0 >> 2);
#pragma unroll 1
    for (uint32_t j = 0; j < jn; ++j, fp += WG / 4, rp -= WG / 4) {
      if (tile_dirty) {  // a non-base inside the window [p, p + k)?
        const uint32_t p = tid + WG * j, dw = p >> 5, sh = p & 31u;
        bool any_bad;
        if constexpr (KC != 0) {
          const uint32_t d0 = s_inv[dw], d1 = s_inv[dw + 1], d2 = s_inv[dw + 2];
          const uint32_t w0 = __builtin_amdgcn_alignbit(d1, d0, sh), w1 = __builtin_amdgcn_alignbit(d2, d1, sh);  // bits p .. p + 63
          constexpr uint32_t M1 = KC >= 64 ? ~0u : (1u << (KC - 32)) - 1u;
          any_bad = (w0 | (w1 & M1)) != 0u;
        } else {
          uint32_t acc = 0;
          for (uint32_t t = 0; 32 * t < ksize; ++t) {
            const uint32_t w = __builtin_amdgcn_alignbit(s_inv[dw + t + 1], s_inv[dw + t], sh);
            const uint32_t left = ksize - 32 * t;
            acc |= left >= 32 ? w : w & ((1u << left) - 1u);
          }
          any_bad = acc != 0u;
        }
        if (any_bad) continue;
      }
      // the lexicographically smaller byte string (canonical): big-endian compare of the first eight bytes, then the rest; the
      // forward strand's first two dwords are read in any case -- they are the hash's first word (plain values: a struct that
      // is written after its construction goes to scratch)
      const uint32_t fd0 = fp[0], fd1 = fp[1];
      uint32_t rd0 = 0, rd1 = 0;
      bool use_rc = false;
      if (canonical) {
        rd0 = rp[0], rd1 = rp[1];
        const uint64_t fw = mk64(__builtin_bswap32(fd1), __builtin_bswap32(fd0));
        const uint64_t rw = mk64(__builtin_bswap32(rd1), __builtin_bswap32(rd0));
        if (fw != rw) {
          use_rc = rw < fw;
        } else {
          for (uint32_t t = 2; 4 * t < ksize; ++t) {
            uint32_t fd = __builtin_bswap32(fp[t]), rd = __builtin_bswap32(rp[t]);
            const uint32_t left = ksize - 4 * t;
            if (left < 4) fd &= ~0u << (8 * (4 - left)), rd &= ~0u << (8 * (4 - left));
            if (fd != rd) {
              use_rc = rd < fd;
              break;
            }
          }
        }
      }
      const LdsStrand sel{use_rc ? rp : fp, use_rc ? rd0 : fd0, use_rc ? rd1 : fd1, true};
      const uint64_t h = t1ha2_long<(uint32_t)KC>(sel, ksize, seed);
      if (h < threshold) stage_hit(stage, stage_cap, h, gm, g, hits, cnt);
    }
  }
  flush_hits(stage, stage_cap, gm, g, hits, cnt);
}
}  // namespace
