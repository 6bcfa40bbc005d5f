// hg_rec_kernels.hip -- the kernels of libhypergen_rec.so: one multi-FASTA text into records, a segmented stream compaction.
//
// A split is eight launches on one stream.  No workgroup waits for another: what a block needs of the blocks in front of it is
// carried from launch to launch as a scanned summary (hg_rec.h: hg_rec_sum), never by polling memory.
//   rec_block_summary_kernel   4096 bytes of text per workgroup, 16 per lane -> the block's summary
//   rec_tile_reduce_kernel     1024 block summaries per workgroup -> the tile's summary
//   rec_block_prefix_kernel    per tile: the summary of the tiles in front of it, then every block's exclusive prefix, in place
//   rec_mark_kernel            the text again: the lane that holds a header line's LF (or the text's last byte) writes the
//                              record's hdr_off, hdr_len, id_len and the number of sequence bytes in front of it
//   rec_pad_reduce_kernel      2048 records per workgroup: the sum of their pads (0..3 bytes each to the next multiple of 4)
//   rec_pad_scan_kernel        one workgroup: the exclusive scan of those sums
//   rec_offsets_kernel         per record: the pads in front of it, hence seq_off; seq_len
//   rec_scatter_kernel         the text a third time: sequence bytes and 'N' pads into an LDS image of the block's stretch of
//                              the output, which leaves as 16-byte stores (byte stores for the <= 15 bytes at either end)
// The output is the text's sequence bytes in text order with the pad of record r - 1 placed where header r starts, so the place
// of a byte is (sequence bytes in front of it) + (pads behind the records in front of its record): both are known per lane
// from the block's prefix and the lane scan, and the image needs no second scan.
#include <atomic>

#include "hg_block_scan.h"
#include "hg_rec.h"

namespace {

constexpr uint32_t WAVES = HG_REC_THREADS / 64;

__device__ __forceinline__ uint32_t below(uint32_t k) { return (1u << k) - 1u; }  // bits 0 .. k - 1 (k <= 31)
__device__ __forceinline__ uint32_t upto(uint32_t k) { return (2u << k) - 1u; }   // bits 0 .. k (k <= 30)

// A lane's 16 bytes as bit masks (bit k: byte i0 + k of the text); bytes from n on are in none of them.
struct LaneText {
  uint32_t w[4];
  uint32_t nv;    // bytes of the lane in front of n
  uint32_t v;     // below(nv)
  uint32_t lf;    // LF
  uint32_t cr;    // CR
  uint32_t ls;    // first byte of a line: byte 0 of the text or the byte behind an LF
  uint32_t hs;    // first byte of a header line
  uint32_t ctl;   // <= 0x20
  uint32_t seqc;  // neither an LF nor a CR in front of an LF or of the text's end: a sequence byte if its line is no header
  uint32_t prev;  // the byte in front of the lane (LF in front of the text)
};

__device__ __forceinline__ LaneText rec_load_lane(const uint8_t *__restrict__ text, uint64_t n, uint64_t i0) {
  LaneText t;
  uint4 q = make_uint4(0, 0, 0, 0);
  if (i0 < n) q = *reinterpret_cast<const uint4 *>(text + i0);  // (readable up to n rounded up to 16)
  t.w[0] = q.x, t.w[1] = q.y, t.w[2] = q.z, t.w[3] = q.w;
  // the byte in front of the lane (look-behind of the header rule) and the one behind it (look-ahead of the CR rule): the
  // neighbours' through the wave, from memory at the wave's two ends
  const uint32_t lane = threadIdx.x & 63;
  uint32_t prev = __shfl_up(q.w >> 24, 1), next = __shfl_down(q.x & 0xFFu, 1);
  if (lane == 0) prev = i0 > 0 && i0 < n ? text[i0 - 1] : '\n';
  if (lane == 63) next = i0 + 16 < n ? text[i0 + 16] : '\n';
  const bool next_lf = i0 + 16 >= n || next == '\n';  // the end of the text ends a line like an LF does
  t.prev = prev;
  t.nv = i0 >= n ? 0u : (n - i0 >= 16 ? 16u : (uint32_t)(n - i0));
  t.v = below(t.nv);
  uint32_t lf = 0, cr = 0, gt = 0, ctl = 0;
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) {
    const uint32_t c = (t.w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    lf |= (uint32_t)(c == '\n') << k, cr |= (uint32_t)(c == '\r') << k, gt |= (uint32_t)(c == '>') << k, ctl |= (uint32_t)(c <= 0x20u) << k;
  }
  t.lf = lf & t.v, t.cr = cr & t.v, t.ctl = ctl & t.v;
  t.ls = ((t.lf << 1) | (uint32_t)(prev == '\n')) & t.v;
  t.hs = t.ls & gt;
  const uint32_t next_ends = (((t.lf | ~t.v) & 0xFFFFu) >> 1) | ((uint32_t)next_lf << 15);  // bit k: byte k + 1 is an LF or behind the text
  t.seqc = t.v & ~t.lf & ~(t.cr & next_ends);
  return t;
}

// the bytes of the header lines that start in the lane
__device__ __forceinline__ uint32_t rec_header_bytes(const LaneText &t) {
  uint32_t h = 0;
  for (uint32_t m = t.ls; m;) {
    const uint32_t p = __builtin_ctz(m);
    m &= m - 1;
    const uint32_t q = m ? __builtin_ctz(m) : 16u;
    if ((t.hs >> p) & 1u) h |= below(q) & ~below(p);
  }
  return h & t.v;
}

// the lane's summary; positions are the text's
__device__ __forceinline__ hg_rec_sum rec_lane_sum(const LaneText &t, uint32_t i0, uint32_t hdr_bytes) {
  hg_rec_sum s;
  uint32_t ctl = t.ctl;
  if (t.ls) {
    const uint32_t last = 31u - __builtin_clz(t.ls);
    s.flags = HG_REC_LS | ((t.hs >> last) & 1u ? HG_REC_HDR : 0u), s.ls_pos = i0 + last;
    ctl &= ~upto(last);
  } else {
    s.flags = 0, s.ls_pos = 0;
  }
  s.ctl_pos = ctl ? i0 + __builtin_ctz(ctl) : HG_REC_NONE;
  s.n_hdr = __builtin_popcount(t.hs);
  const uint32_t front = t.ls ? below(__builtin_ctz(t.ls)) : 0xFFFFu;
  s.pre = __builtin_popcount(t.seqc & front);
  s.post = __builtin_popcount(t.seqc & ~front & ~hdr_bytes);
  return s;
}

__device__ __forceinline__ hg_rec_sum shfl_up_sum(const hg_rec_sum &s, uint32_t o) {
  hg_rec_sum r;
  r.flags = __shfl_up(s.flags, o), r.ls_pos = __shfl_up(s.ls_pos, o), r.ctl_pos = __shfl_up(s.ctl_pos, o);
  r.n_hdr = __shfl_up(s.n_hdr, o), r.pre = __shfl_up(s.pre, o), r.post = __shfl_up(s.post, o);
  return r;
}

// block_excl_scan (hg_block_scan.h) for summaries: the combination of the threads in front of this one, in thread order;
// *total = that of the whole workgroup
__device__ __forceinline__ hg_rec_sum rec_block_scan(const hg_rec_sum &v, hg_rec_sum *s_wave /* WAVES */, hg_rec_sum *total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  hg_rec_sum inc = v;
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const hg_rec_sum up = shfl_up_sum(inc, o);
    if (lane >= o) inc = hg_rec_combine(up, inc);
  }
  hg_rec_sum ex = shfl_up_sum(inc, 1);
  if (lane == 0) ex = hg_rec_identity();
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  hg_rec_sum before = hg_rec_identity(), all = hg_rec_identity();
#pragma unroll
  for (uint32_t w = 0; w < WAVES; ++w) {
    const hg_rec_sum t = s_wave[w];
    if (w < wave) before = hg_rec_combine(before, t);
    all = hg_rec_combine(all, t);
  }
  __syncthreads();  // (s_wave may be reused by the caller's next round)
  *total = all;
  return hg_rec_combine(before, ex);
}

// ---- the three passes over the summaries -------------------------------------------------------------------------------
__global__ __launch_bounds__(HG_REC_THREADS) void rec_block_summary_kernel(const uint8_t *__restrict__ text, uint64_t n,
                                                                           hg_rec_sum *__restrict__ blk) {
  __shared__ hg_rec_sum s_wave[WAVES];
  const uint64_t i0 = (uint64_t)blockIdx.x * HG_REC_BLOCK + threadIdx.x * HG_REC_LANE_BYTES;
  const LaneText t = rec_load_lane(text, n, i0);
  hg_rec_sum total;
  (void)rec_block_scan(rec_lane_sum(t, (uint32_t)i0, rec_header_bytes(t)), s_wave, &total);
  if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ __launch_bounds__(HG_REC_THREADS) void rec_tile_reduce_kernel(const hg_rec_sum *__restrict__ blk, uint32_t n_blk,
                                                                         hg_rec_sum *__restrict__ tile) {
  __shared__ hg_rec_sum s_wave[WAVES];
  const uint32_t first = blockIdx.x * HG_REC_TILE + threadIdx.x * HG_REC_TILE_ITEMS;
  hg_rec_sum acc = hg_rec_identity();
#pragma unroll
  for (uint32_t j = 0; j < HG_REC_TILE_ITEMS; ++j)
    if (first + j < n_blk) acc = hg_rec_combine(acc, blk[first + j]);
  hg_rec_sum total;
  (void)rec_block_scan(acc, s_wave, &total);
  if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

__global__ __launch_bounds__(HG_REC_THREADS) void rec_block_prefix_kernel(hg_rec_sum *__restrict__ blk, uint32_t n_blk,
                                                                          const hg_rec_sum *__restrict__ tile, uint32_t n_tiles,
                                                                          uint32_t *__restrict__ res) {
  __shared__ hg_rec_sum s_wave[WAVES];
  // the tiles in front of this one (at most 1024: four per thread)
  hg_rec_sum acc = hg_rec_identity();
#pragma unroll
  for (uint32_t j = 0; j < HG_REC_TILE_ITEMS; ++j) {
    const uint32_t idx = threadIdx.x * HG_REC_TILE_ITEMS + j;
    if (idx < blockIdx.x && idx < n_tiles) acc = hg_rec_combine(acc, tile[idx]);
  }
  hg_rec_sum front;
  (void)rec_block_scan(acc, s_wave, &front);
  // this tile's blocks: every block summary becomes the summary of all the text in front of the block
  const uint32_t first = blockIdx.x * HG_REC_TILE + threadIdx.x * HG_REC_TILE_ITEMS;
  hg_rec_sum item[HG_REC_TILE_ITEMS];
  acc = hg_rec_identity();
#pragma unroll
  for (uint32_t j = 0; j < HG_REC_TILE_ITEMS; ++j) {
    item[j] = first + j < n_blk ? blk[first + j] : hg_rec_identity();
    acc = hg_rec_combine(acc, item[j]);
  }
  hg_rec_sum all;
  hg_rec_sum run = hg_rec_combine(front, rec_block_scan(acc, s_wave, &all));
#pragma unroll
  for (uint32_t j = 0; j < HG_REC_TILE_ITEMS; ++j) {
    if (first + j < n_blk) blk[first + j] = run;
    run = hg_rec_combine(run, item[j]);
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {  // the last tile knows the whole text
    const hg_rec_sum whole = hg_rec_combine(front, all);
    for (uint32_t k = 0; k < HG_REC_RES_WORDS; ++k) res[k] = 0;
    res[HG_REC_RES_NRECS] = whole.n_hdr, res[HG_REC_RES_TOTAL] = hg_rec_seq_before(whole);
  }
}

// ---- the lane's view of the text once the prefix is known ---------------------------------------------------------------
struct LaneState {
  hg_rec_sum x;      // the summary of all the text in front of the lane
  bool in_hdr;       // the lane is entered inside a header line
  uint32_t seq;      // the lane's sequence bytes
  uint32_t cb;       // sequence bytes in front of the lane
};

__device__ __forceinline__ LaneState rec_lane_state(const LaneText &t, const hg_rec_sum &x, uint32_t hdr_bytes) {
  LaneState s;
  s.x = x, s.in_hdr = hg_rec_in_header(x);
  const uint32_t front = t.ls ? below(__builtin_ctz(t.ls)) : 0xFFFFu;
  s.seq = t.seqc & ~(hdr_bytes | (s.in_hdr ? front : 0u));
  s.cb = hg_rec_seq_before(x);
  return s;
}

// The line that ends at byte k of the lane -- with its LF there or, at the text's last byte, with the text: the index of its
// record if it is a header line, -1 if not
__device__ __forceinline__ int64_t rec_line_record(const LaneText &t, const LaneState &s, uint32_t k) {
  const uint32_t starts = t.ls & upto(k);
  const bool is_hdr = starts ? ((t.hs >> (31u - __builtin_clz(starts))) & 1u) != 0 : s.in_hdr;
  return is_hdr ? (int64_t)s.x.n_hdr + __builtin_popcount(t.hs & upto(k)) - 1 : -1;
}

// ---- per header line: where it is, how long, how long its identifier, how much sequence precedes it --------------------
__global__ __launch_bounds__(HG_REC_THREADS) void rec_mark_kernel(const uint8_t *__restrict__ text, uint64_t n,
                                                                  const hg_rec_sum *__restrict__ pre, hg_rec_entry *__restrict__ recs,
                                                                  uint32_t *__restrict__ cidx, uint32_t n_recs, uint32_t *__restrict__ res) {
  __shared__ hg_rec_sum s_wave[WAVES];
  const uint64_t i0 = (uint64_t)blockIdx.x * HG_REC_BLOCK + threadIdx.x * HG_REC_LANE_BYTES;
  const LaneText t = rec_load_lane(text, n, i0);
  const uint32_t hdr_bytes = rec_header_bytes(t);
  hg_rec_sum total;
  const hg_rec_sum ex = rec_block_scan(rec_lane_sum(t, (uint32_t)i0, hdr_bytes), s_wave, &total);
  if (!t.nv) return;
  const LaneState s = rec_lane_state(t, hg_rec_combine(pre[blockIdx.x], ex), hdr_bytes);
  const uint32_t p0 = (uint32_t)i0;
  const bool owns_end = i0 + t.nv == n;                                     // the lane holds the text's last byte
  const bool open_end = owns_end && !((t.lf >> (t.nv - 1)) & 1u);           // ... and that byte is no LF: the text ends the line
  // every line end of the lane: its LFs, and the text's end behind an unterminated last line
  for (uint32_t m = t.lf | (open_end ? 1u << (t.nv - 1) : 0u); m;) {
    const uint32_t k = __builtin_ctz(m);
    m &= m - 1;
    const int64_t r = rec_line_record(t, s, k);
    if (r < 0 || r >= (int64_t)n_recs) continue;
    const bool at_text_end = !((t.lf >> k) & 1u);
    const uint32_t starts = t.ls & upto(k);
    uint32_t start, id_end;  // where the header line starts; the first byte <= 0x20 behind its '>', the text's end without one
    if (starts) {
      const uint32_t sl = 31u - __builtin_clz(starts);
      const uint32_t cand = t.ctl & ~upto(sl) & upto(k);
      start = p0 + sl, id_end = cand ? p0 + __builtin_ctz(cand) : (uint32_t)n;
    } else {
      const uint32_t cand = t.ctl & upto(k);
      start = s.x.ls_pos, id_end = s.x.ctl_pos != HG_REC_NONE ? s.x.ctl_pos : (cand ? p0 + __builtin_ctz(cand) : (uint32_t)n);
    }
    // the content ends in front of the LF, or with the text; one CR directly in front of that is not part of it
    const uint32_t end = at_text_end ? p0 + k + 1 : p0 + k;
    const bool cr = at_text_end ? ((t.cr >> k) & 1u) != 0 : (k ? ((t.cr >> (k - 1)) & 1u) != 0 : t.prev == '\r');
    const uint32_t c = s.cb + __builtin_popcount(s.seq & below(k));  // (a header line holds no sequence byte)
    if (recs) *reinterpret_cast<uint4 *>(&recs[r]) = make_uint4(start, 0u, end - start - (cr ? 1u : 0u), id_end - start - 1u);
    cidx[r] = c;
    if (r == 0) res[HG_REC_RES_LEAD] = c;
  }
  if (owns_end) {
    const uint32_t nr = s.x.n_hdr + __builtin_popcount(t.hs);
    if (nr == n_recs) cidx[nr] = s.cb + __builtin_popcount(s.seq);
  }
}

// ---- the pads behind the records ----------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rec_pad(uint32_t len) { return (0u - len) & 3u; }

__global__ __launch_bounds__(HG_REC_THREADS) void rec_pad_reduce_kernel(const uint32_t *__restrict__ cidx, uint32_t n_recs,
                                                                        uint32_t *__restrict__ tsum) {
  __shared__ uint32_t s_wave[WAVES];
  const uint64_t first = (uint64_t)blockIdx.x * HG_REC_PAD_TILE + threadIdx.x * HG_REC_PAD_ITEMS;
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < HG_REC_PAD_ITEMS; ++j)
    if (first + j < n_recs) sum += rec_pad(cidx[first + j + 1] - cidx[first + j]);
  uint32_t total;
  (void)block_excl_scan<WAVES>(sum, s_wave, &total);
  if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// one workgroup: a tile sum is at most 3 * 2048, a round of 2048 tiles fits 32 bits, the running base is 64 bits
__global__ __launch_bounds__(HG_REC_THREADS) void rec_pad_scan_kernel(const uint32_t *__restrict__ tsum, uint64_t *__restrict__ tbase,
                                                                      uint32_t n_tiles, uint32_t *__restrict__ res) {
  __shared__ uint32_t s_wave[WAVES];
  uint64_t carry = 0;
  for (uint64_t base = 0; base < n_tiles; base += HG_REC_PAD_TILE) {
    const uint64_t first = base + threadIdx.x * HG_REC_PAD_ITEMS;
    uint32_t v[HG_REC_PAD_ITEMS], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < HG_REC_PAD_ITEMS; ++j) sum += v[j] = first + j < n_tiles ? tsum[first + j] : 0u;
    uint32_t total;
    uint64_t run = carry + block_excl_scan<WAVES>(sum, s_wave, &total);
#pragma unroll
    for (uint32_t j = 0; j < HG_REC_PAD_ITEMS; ++j) {
      if (first + j < n_tiles) tbase[first + j] = run;
      run += v[j];
    }
    carry += total;
  }
  if (threadIdx.x == 0) res[HG_REC_RES_PAD_LO] = (uint32_t)carry, res[HG_REC_RES_PAD_HI] = (uint32_t)(carry >> 32);
}

__global__ __launch_bounds__(HG_REC_THREADS) void rec_offsets_kernel(const uint32_t *__restrict__ cidx, uint32_t n_recs,
                                                                     const uint64_t *__restrict__ tbase, uint64_t *__restrict__ ps,
                                                                     hg_rec_entry *__restrict__ recs) {
  __shared__ uint32_t s_wave[WAVES];
  const uint64_t first = (uint64_t)blockIdx.x * HG_REC_PAD_TILE + threadIdx.x * HG_REC_PAD_ITEMS;
  uint32_t at[HG_REC_PAD_ITEMS], len[HG_REC_PAD_ITEMS], sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < HG_REC_PAD_ITEMS; ++j) {
    at[j] = len[j] = 0;
    if (first + j < n_recs) at[j] = cidx[first + j], len[j] = cidx[first + j + 1] - at[j];
    sum += rec_pad(len[j]);
  }
  uint32_t total;
  uint64_t run = tbase[blockIdx.x] + block_excl_scan<WAVES>(sum, s_wave, &total);
#pragma unroll
  for (uint32_t j = 0; j < HG_REC_PAD_ITEMS; ++j) {
    const uint64_t r = first + j;
    if (r >= n_recs) break;
    ps[r] = run;
    if (recs) {
      const uint64_t off = (uint64_t)at[j] + run;
      *(reinterpret_cast<uint4 *>(&recs[r]) + 1) = make_uint4((uint32_t)off, (uint32_t)(off >> 32), len[j], 0u);
    }
    run += rec_pad(len[j]);
    if (r == n_recs - 1) ps[n_recs] = run;
  }
}

// ---- sequence bytes and pads into the layout ---------------------------------------------------------------------------
// where the output stands in front of a place of the text whose prefix summary is x: the sequence bytes in front of it, and the
// pads placed so far -- the '>' of header r places the pad of record r - 1
__device__ __forceinline__ uint64_t rec_out_at(const hg_rec_sum &x, const uint64_t *__restrict__ ps) {
  return (uint64_t)hg_rec_seq_before(x) + ps[x.n_hdr ? x.n_hdr - 1 : 0];
}

__global__ __launch_bounds__(HG_REC_THREADS) void rec_scatter_kernel(const uint8_t *__restrict__ text, uint64_t n,
                                                                     const hg_rec_sum *__restrict__ pre, uint32_t n_blk,
                                                                     const uint64_t *__restrict__ ps, uint32_t n_recs,
                                                                     uint8_t *__restrict__ seq, uint64_t seq_bytes) {
  __shared__ hg_rec_sum s_wave[WAVES];
  __shared__ __attribute__((aligned(16))) uint8_t img[HG_REC_IMAGE];
  const uint64_t i0 = (uint64_t)blockIdx.x * HG_REC_BLOCK + threadIdx.x * HG_REC_LANE_BYTES;
  const LaneText t = rec_load_lane(text, n, i0);
  const uint32_t hdr_bytes = rec_header_bytes(t);
  hg_rec_sum total;
  const hg_rec_sum ex = rec_block_scan(rec_lane_sum(t, (uint32_t)i0, hdr_bytes), s_wave, &total);
  // the block's stretch of the output, [o_base, o_end): image byte shift + i is output byte o_base + i, so that 16-byte
  // chunks of the image are 16-byte chunks of the output
  const hg_rec_sum xb = pre[blockIdx.x];
  const uint64_t o_base = rec_out_at(xb, ps);
  const uint64_t o_end = blockIdx.x + 1 < n_blk ? rec_out_at(pre[blockIdx.x + 1], ps) : seq_bytes;
  const uint32_t shift = (uint32_t)(o_base & 15u);
  auto put = [&](uint64_t o, uint8_t c) {
    const uint64_t at = o - o_base + shift;
    if (at < HG_REC_IMAGE) img[at] = c;
  };
  if (t.nv) {
    const LaneState s = rec_lane_state(t, hg_rec_combine(xb, ex), hdr_bytes);
    // sequence bytes: byte k of record r goes to (sequence bytes in front of it) + ps[r]
    uint32_t cur = 0;  // headers in front of the byte whose ps is loaded (0: none yet)
    uint64_t cur_ps = 0;
    for (uint32_t m = s.seq; m;) {
      const uint32_t k = __builtin_ctz(m);
      m &= m - 1;
      const uint32_t hdrs = s.x.n_hdr + __builtin_popcount(t.hs & below(k));
      if (!hdrs) continue;  // (sequence before the first header: such a text is not scattered)
      if (hdrs != cur) cur = hdrs, cur_ps = ps[hdrs - 1];
      put((uint64_t)s.cb + __builtin_popcount(s.seq & below(k)) + cur_ps, (uint8_t)(t.w[k >> 2] >> (8 * (k & 3))));
    }
    // pads: where header line r >= 1 starts, the pad of record r - 1; where the text ends, the pad of the last record
    for (uint32_t m = t.hs; m;) {
      const uint32_t k = __builtin_ctz(m);
      m &= m - 1;
      const uint32_t r = s.x.n_hdr + __builtin_popcount(t.hs & below(k));
      if (r < 1 || r >= n_recs) continue;
      const uint64_t c = (uint64_t)s.cb + __builtin_popcount(s.seq & below(k));
      for (uint64_t o = c + ps[r - 1]; o < c + ps[r]; ++o) put(o, 'N');
    }
    if (i0 + t.nv == n && n_recs) {
      const uint64_t c = (uint64_t)s.cb + __builtin_popcount(s.seq);
      for (uint64_t o = c + ps[n_recs - 1]; o < c + ps[n_recs]; ++o) put(o, 'N');
    }
  }
  __syncthreads();
  if (o_end <= o_base) return;
  const uint64_t count = o_end - o_base;
  const uint32_t lo = shift, hi = shift + (count < HG_REC_IMAGE - 16 ? (uint32_t)count : HG_REC_IMAGE - 16);
  uint8_t *out = seq + (o_base - shift);  // (16-byte aligned: seq is, and o_base - shift is a multiple of 16)
  for (uint32_t j = threadIdx.x * 16; j < hi; j += HG_REC_THREADS * 16) {
    if (j >= lo && j + 16 <= hi) {
      *reinterpret_cast<uint4 *>(out + j) = *reinterpret_cast<const uint4 *>(img + j);
    } else {  // the block's first and last chunk: the bytes of them that are the block's
      for (uint32_t b = j > lo ? j : lo; b < j + 16 && b < hi; ++b) out[b] = img[b];
    }
  }
}

std::atomic<uint64_t> g_launches[HG_REC_N_KERNELS];

inline uint32_t div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

}  // namespace

uint64_t hg_rec_launches(uint32_t kernel) { return kernel < HG_REC_N_KERNELS ? g_launches[kernel].load() : 0; }

hipError_t hg_rec_launch_summary(hipStream_t st, const uint8_t *d_text, uint64_t n, hg_rec_sum *d_blk, uint32_t n_blk) {
  ++g_launches[HG_REC_K_SUMMARY];
  rec_block_summary_kernel<<<n_blk, HG_REC_THREADS, 0, st>>>(d_text, n, d_blk);
  return hipGetLastError();
}
hipError_t hg_rec_launch_tile_reduce(hipStream_t st, const hg_rec_sum *d_blk, uint32_t n_blk, hg_rec_sum *d_tile, uint32_t n_tiles) {
  ++g_launches[HG_REC_K_TILE_REDUCE];
  rec_tile_reduce_kernel<<<n_tiles, HG_REC_THREADS, 0, st>>>(d_blk, n_blk, d_tile);
  return hipGetLastError();
}
hipError_t hg_rec_launch_prefix(hipStream_t st, hg_rec_sum *d_blk, uint32_t n_blk, const hg_rec_sum *d_tile, uint32_t n_tiles, uint32_t *d_res) {
  ++g_launches[HG_REC_K_PREFIX];
  rec_block_prefix_kernel<<<n_tiles, HG_REC_THREADS, 0, st>>>(d_blk, n_blk, d_tile, n_tiles, d_res);
  return hipGetLastError();
}
hipError_t hg_rec_launch_mark(hipStream_t st, const uint8_t *d_text, uint64_t n, const hg_rec_sum *d_pre, uint32_t n_blk,
                              hg_rec_entry *d_recs, uint32_t *d_cidx, uint32_t n_recs, uint32_t *d_res) {
  ++g_launches[HG_REC_K_MARK];
  rec_mark_kernel<<<n_blk, HG_REC_THREADS, 0, st>>>(d_text, n, d_pre, d_recs, d_cidx, n_recs, d_res);
  return hipGetLastError();
}
hipError_t hg_rec_launch_pad_reduce(hipStream_t st, const uint32_t *d_cidx, uint32_t n_recs, uint32_t *d_tsum, uint32_t n_tiles) {
  ++g_launches[HG_REC_K_PAD_REDUCE];
  rec_pad_reduce_kernel<<<n_tiles, HG_REC_THREADS, 0, st>>>(d_cidx, n_recs, d_tsum);
  return hipGetLastError();
}
hipError_t hg_rec_launch_pad_scan(hipStream_t st, const uint32_t *d_tsum, uint64_t *d_tbase, uint32_t n_tiles, uint32_t *d_res) {
  ++g_launches[HG_REC_K_PAD_SCAN];
  rec_pad_scan_kernel<<<1, HG_REC_THREADS, 0, st>>>(d_tsum, d_tbase, n_tiles, d_res);
  return hipGetLastError();
}
hipError_t hg_rec_launch_offsets(hipStream_t st, const uint32_t *d_cidx, uint32_t n_recs, const uint64_t *d_tbase, uint64_t *d_ps,
                                 hg_rec_entry *d_recs) {
  ++g_launches[HG_REC_K_OFFSETS];
  rec_offsets_kernel<<<div_up(n_recs, HG_REC_PAD_TILE), HG_REC_THREADS, 0, st>>>(d_cidx, n_recs, d_tbase, d_ps, d_recs);
  return hipGetLastError();
}
hipError_t hg_rec_launch_scatter(hipStream_t st, const uint8_t *d_text, uint64_t n, const hg_rec_sum *d_pre, uint32_t n_blk,
                                 const uint64_t *d_ps, uint32_t n_recs, uint8_t *d_seq, uint64_t seq_bytes) {
  ++g_launches[HG_REC_K_SCATTER];
  rec_scatter_kernel<<<n_blk, HG_REC_THREADS, 0, st>>>(d_text, n, d_pre, n_blk, d_ps, n_recs, d_seq, seq_bytes);
  return hipGetLastError();
}
