// hg_kmer_asm.h -- the k-mer body of kmer_sample_shared for k = 17..32 as assembly text: the word reads of the next k-mer,
// three (k <= 24) or four mixup64 stages, final64 and the candidate compare on fixed register pairs, and the asm
// statements built from that text.  Macros only.  Included by hg_kmer_kernels.hip only.  Expects: P0..P6 (hg_kmer_t1ha2.h)
// for the operand lists, and at the place of use the local names listed at "the statements" below.
#pragma once

// The compiler's code for the same arithmetic (t1ha2_fixed_w's form) spends 10 v_mov and 3 v_add_u32 per hash on moving
// 32-bit halves into the even-aligned register pairs v_mad_u64_u32 / v_lshl_add_u64 take (inline asm operands cannot name the halves of a
// 64-bit operand, so every product's halves travel as separate values and get re-paired), plus nops behind every carry
// that goes through an SGPR pair.  Here all temporaries are fixed physical registers, every result is produced in the
// pair that consumes it, carries go through VCC into a VOP2 v_addc (no SGPR read hazard), and what is left is what the
// ISA forces: the high dword of a product is an ODD register and a 64-bit addend has to start at an EVEN one -- one
// v_mov per 128-bit product (into the pair Z = {x, 0}).  56 vector instructions per hash + candidate compare instead of 64
// (55 with the bounded first mixup, HG_KS_MUL128_BOUNDED below; 54 without the carry op of the P1 stage, HG_KS_MUL128_NC).
// HG_KS_MUL128: lo64(x P) -> {v74, v76}, hi64(x P) + ADDEND -> OUT; 7 instructions, the carry of the cross sum through VCC.
//   v[56:61] / v[62:67]  hash words of k-mer j / j+1 (filled by HG_KS_READ one k-mer ahead)
//   Z v[68:69]  H v71 (hash high dword)  X v[72:73]  A v[74:75]  T v[76:77]  U v[78:79]  S1 v[80:81]  S2 v[82:83]  R v[84:85]
//   Y v[86:87]  C v[88:89]
#define HG_KS_MUL128(XLO, XHI, PLO, PHI, ADDEND, OUT, OUTHI)                                   \
  "v_mad_u64_u32 v[74:75], %[junk], " XLO ", " PLO ", 0\n\t"                                   \
  "v_mov_b32 v68, v75\n\t"                                                                     \
  "v_mad_u64_u32 v[76:77], %[junk], " XHI ", " PLO ", v[68:69]\n\t"                            \
  "v_mad_u64_u32 v[76:77], vcc, " XLO ", " PHI ", v[76:77]\n\t"                                \
  "v_mad_u64_u32 " OUT ", %[junk], v77, 1, " ADDEND "\n\t"                                     \
  "v_mad_u64_u32 " OUT ", %[junk], " XHI ", " PHI ", " OUT "\n\t"                              \
  "v_addc_co_u32_e32 " OUTHI ", vcc, 0, " OUTHI ", vcc\n\t"
// The same product for a prime whose cross sum fits 64 bits (mul128_cross_fits): the third product's carry-out is zero
// for every operand, so it goes to %[junk], VCC is not touched and the v_addc is not there -- 6 instructions, not 7.
#define HG_KS_MUL128_NC(XLO, XHI, PLO, PHI, ADDEND, OUT, OUTHI)                                \
  "v_mad_u64_u32 v[74:75], %[junk], " XLO ", " PLO ", 0\n\t"                                   \
  "v_mov_b32 v68, v75\n\t"                                                                     \
  "v_mad_u64_u32 v[76:77], %[junk], " XHI ", " PLO ", v[68:69]\n\t"                            \
  "v_mad_u64_u32 v[76:77], %[junk], " XLO ", " PHI ", v[76:77]\n\t"                            \
  "v_mad_u64_u32 " OUT ", %[junk], v77, 1, " ADDEND "\n\t"                                     \
  "v_mad_u64_u32 " OUT ", %[junk], " XHI ", " PHI ", " OUT "\n\t"
// The stages name their prime through these, so that the text without the carry cannot meet another prime than the
// two the predicate admits: P1 (the last stage) and P3 (the general first mixup of k <= 24, the second stage of k >= 25).
static_assert(mul128_cross_fits(P1), "HG_KS_MUL128_P1 drops the carry op");
static_assert(mul128_cross_fits(P3), "HG_KS_MUL128_P3 drops the carry op");
#define HG_KS_MUL128_P1(XLO, XHI, ADDEND, OUT, OUTHI) HG_KS_MUL128_NC(XLO, XHI, "%[p1l]", "%[p1h]", ADDEND, OUT, OUTHI)
#define HG_KS_MUL128_P3(XLO, XHI, ADDEND, OUT, OUTHI) HG_KS_MUL128_NC(XLO, XHI, "%[p3l]", "%[p3h]", ADDEND, OUT, OUTHI)
// The FIRST mixup's multiplicand is x = s + w0 with s wave-uniform and small (the seed, k <= 24; the length K, k >= 25)
// and w0 eight staged bytes, each one of "ACGT" in every k-mer that is KEPT: both phase images are written from the
// code -> ASCII lookups, whatever the input byte was, so w0.lo, w0.hi <= 0x54545454.  (Lanes whose k-mers are discarded
// anyway -- lookahead lanes, slots a dead wave did not stage -- may multiply anything: the stage is arithmetic only, no
// address depends on it.)  With s below FIRST_SEED_END (first_mixup_bounded(), hg_kmer_t1ha2.h, evaluates the worst case):
//   * no carry leaves the low dword of s + w0: x0 = w0.lo + s is one 32-bit add and x1 is w0.hi as read;
//   * W = x0 p1 + x1 p0 + hi32(x0 p0) < 2^64: the third product has no carry-out, so the v_addc goes.  For P3 (k <= 24)
//     that needs no bound at all -- mul128_cross_fits(P3) holds for every operand; for P4 (k >= 25), whose cross sum can
//     reach 1.423 x 2^64, it is the bound on x0 and x1 that does it;
//   * hi32(W) + s < 2^32 (the stage's addend is s as well): the "x 1" product is one 32-bit add into Z's low half, and
//     the last product takes Z as its addend, as HG_KS_FINAL's does.
// One v_lshl_add_u64, one v_mad_u64_u32 and one v_addc_co_u32 become two v_add_u32: 7 instructions instead of 8.
// ADD32: s as a 32-bit operand (an SGPR or an inline constant).  Z's high half stays 0.
#define HG_KS_MUL128_BOUNDED(W0L, W0H, PLO, PHI, ADD32, OUT)                                   \
  "v_add_u32_e32 v72, " ADD32 ", " W0L "\n\t"                                                  \
  "v_mad_u64_u32 v[74:75], %[junk], v72, " PLO ", 0\n\t"                                       \
  "v_mov_b32 v68, v75\n\t"                                                                     \
  "v_mad_u64_u32 v[76:77], %[junk], " W0H ", " PLO ", v[68:69]\n\t"                            \
  "v_mad_u64_u32 v[76:77], %[junk], v72, " PHI ", v[76:77]\n\t"                                \
  "v_add_u32_e32 v68, " ADD32 ", v77\n\t"                                                      \
  "v_mad_u64_u32 " OUT ", %[junk], " W0H ", " PHI ", v[68:69]\n\t"
// lo64(x * P) -> {OLO, OHI} (a pair): three chained products and one add into the pair's own high half
#define HG_KS_LO64(XLO, XHI, PLO, PHI, OUT, OLO_UNUSED, OHI)                                   \
  "v_mad_u64_u32 " OUT ", %[junk], " XLO ", " PLO ", 0\n\t"                                    \
  "v_mad_u64_u32 v[76:77], %[junk], " XLO ", " PHI ", 0\n\t"                                   \
  "v_mad_u64_u32 v[76:77], %[junk], " XHI ", " PLO ", v[76:77]\n\t"                            \
  "v_add_u32_e32 " OHI ", " OHI ", v76\n\t"

// ---- the word reads ------------------------------------------------------------------------------------------------
// request the words of one k-mer into one buffer (registers R0..R7 = four pairs; three of them for K <= 24): whole
// dwords of the strand's phase image and the last 1..4 bytes.  A case is (D, B) = (dwords, bytes in the last dword):
// K = 17..20: (5, 1..4), 21..24: (6, 1..4), 25..28: (7, 1..4), 29..32: (8, 1..4).
// (dword reads: a ds_read_b64 at an address that is a multiple of 4 but not of 8 is as slow as a byte-aligned one --
// measured 18.8 ms against 8.5 for the whole kernel -- and ds_read2_b32's 8-bit offsets cannot hold the phase image's)
#define HG_KS_RD(R, O) "ds_read_b32 v" R ", %[base] offset:%[" O "]\n\t"
#define HG_KS_RD4(R, O) "ds_read_b32 v" R ", %[base] offset:%[" O "] + 4\n\t"
#define HG_KS_HEAD2(R0, R1, R2, R3) HG_KS_RD(R0, "o0") HG_KS_RD4(R1, "o0") HG_KS_RD(R2, "o1") HG_KS_RD4(R3, "o1")
#define HG_KS_HEAD3(R0, R1, R2, R3, R4, R5) HG_KS_HEAD2(R0, R1, R2, R3) HG_KS_RD(R4, "o2") HG_KS_RD(R5, "o3")
// the last pair: odd dword count (low half only, high half zero) / even (a whole dword + the rest)
#define HG_KS_TAIL_O1(RL, RH, OL, OH) "ds_read_u8 v" RL ", %[base] offset:%[" OL "]\n\tv_mov_b32 v" RH ", 0"
#define HG_KS_TAIL_O2(RL, RH, OL, OH) "ds_read_u16 v" RL ", %[base] offset:%[" OL "]\n\tv_mov_b32 v" RH ", 0"
#define HG_KS_TAIL_O3(RL, RH, OL, OH) "ds_read_b32 v" RL ", %[base] offset:%[" OL "]\n\tv_mov_b32 v" RH ", 0"
#define HG_KS_TAIL_O4(RL, RH, OL, OH) HG_KS_TAIL_O3(RL, RH, OL, OH)
#define HG_KS_TAIL_E1(RL, RH, OL, OH) HG_KS_RD(RL, OL) "ds_read_u8 v" RH ", %[base] offset:%[" OH "]"
#define HG_KS_TAIL_E2(RL, RH, OL, OH) HG_KS_RD(RL, OL) "ds_read_u16 v" RH ", %[base] offset:%[" OH "]"
#define HG_KS_TAIL_E3(RL, RH, OL, OH) HG_KS_RD(RL, OL) "ds_read_b32 v" RH ", %[base] offset:%[" OH "]"
#define HG_KS_TAIL_E4(RL, RH, OL, OH) HG_KS_TAIL_E3(RL, RH, OL, OH)
// by dword count D: the head, the last pair (B pasted onto its parity) and the register of the last dword
#define HG_KS_HEAD_5(R0, R1, R2, R3, R4, R5, R6, R7) HG_KS_HEAD2(R0, R1, R2, R3)
#define HG_KS_HEAD_6(R0, R1, R2, R3, R4, R5, R6, R7) HG_KS_HEAD2(R0, R1, R2, R3)
#define HG_KS_HEAD_7(R0, R1, R2, R3, R4, R5, R6, R7) HG_KS_HEAD3(R0, R1, R2, R3, R4, R5)
#define HG_KS_HEAD_8(R0, R1, R2, R3, R4, R5, R6, R7) HG_KS_HEAD3(R0, R1, R2, R3, R4, R5)
#define HG_KS_TAIL_5(B, R0, R1, R2, R3, R4, R5, R6, R7) HG_KS_TAIL_O##B(R4, R5, "o2", "o3")
#define HG_KS_TAIL_6(B, R0, R1, R2, R3, R4, R5, R6, R7) HG_KS_TAIL_E##B(R4, R5, "o2", "o3")
#define HG_KS_TAIL_7(B, R0, R1, R2, R3, R4, R5, R6, R7) HG_KS_TAIL_O##B(R6, R7, "o4", "o5")
#define HG_KS_TAIL_8(B, R0, R1, R2, R3, R4, R5, R6, R7) HG_KS_TAIL_E##B(R6, R7, "o4", "o5")
#define HG_KS_LASTDW_5(R0, R1, R2, R3, R4, R5, R6, R7) R4
#define HG_KS_LASTDW_6(R0, R1, R2, R3, R4, R5, R6, R7) R5
#define HG_KS_LASTDW_7(R0, R1, R2, R3, R4, R5, R6, R7) R6
#define HG_KS_LASTDW_8(R0, R1, R2, R3, R4, R5, R6, R7) R7
#define HG_KS_READ_TEXT(D, B, ...) HG_KS_HEAD_##D(__VA_ARGS__) HG_KS_TAIL_##D(B, __VA_ARGS__)
// wait for the words requested one hash ago; K % 4 == 3: the last dword carries a byte of the next base
#define HG_KS_W "s_waitcnt lgkmcnt(0)\n\t"
#define HG_KS_WM(R) HG_KS_W "v_and_b32 v" R ", 0xffffff, v" R "\n\t"
#define HG_KS_WAIT_B1(R) HG_KS_W
#define HG_KS_WAIT_B2(R) HG_KS_W
#define HG_KS_WAIT_B3(R) HG_KS_WM(R)
#define HG_KS_WAIT_B4(R) HG_KS_W
#define HG_KS_WAIT_TEXT(D, B, ...) HG_KS_WAIT_B##B(HG_KS_LASTDW_##D(__VA_ARGS__))
// the two word buffers: R0..R7 and the same as register pairs; K <= 24 uses the first three pairs
#define HG_KS_REGS0 "56", "57", "58", "59", "60", "61", "90", "91"
#define HG_KS_REGS1 "62", "63", "64", "65", "66", "67", "92", "93"
// (in front: the first word's two dwords by name, for the bounded first mixup)
#define HG_KS_PAIRS0 "v56", "v57", "v[56:57]", "v[58:59]", "v[60:61]", "v[90:91]"
#define HG_KS_PAIRS1 "v62", "v63", "v[62:63]", "v[64:65]", "v[66:67]", "v[92:93]"
#define HG_KS_APPLY(M, ...) M(__VA_ARGS__)  // (the lists above are expanded before M sees them)

// ---- the hash ------------------------------------------------------------------------------------------------------
// final64(a, b): x = (a + rot64(b, 41)) * P0, y = (rot64(a, 23) + b) * P6 (low halves), z = x ^ y, mux64(z, P5), compare.
// The compare only marks CANDIDATES: hi32(h) <= hi32(threshold), one 32-bit compare on the high dword's v_xor instead of
// the low dword's v_xor and a 64-bit compare.  The hash's low dword stays recoverable -- its two product dwords v74 / v78
// are outputs -- and the exact h < threshold is decided in the wave-uniform hit path (1 k-mer in `scaled`, plus the
// k-mers whose high dword equals the threshold's: 2^-32 of them).
#define HG_KS_FINAL(AP, AL, AH, BP, BL, BH)                                                                          \
  "v_alignbit_b32 v86, " BL ", " BH ", 9\n\t"                                                                        \
  "v_alignbit_b32 v87, " BH ", " BL ", 9\n\t"                                                                        \
  "v_lshl_add_u64 v[72:73], v[86:87], 0, " AP "\n\t"                                                                 \
  "v_alignbit_b32 v86, " AH ", " AL ", 23\n\t"                                                                       \
  "v_alignbit_b32 v87, " AL ", " AH ", 23\n\t"                                                                       \
  "v_lshl_add_u64 v[88:89], v[86:87], 0, " BP "\n\t"                                                                 \
  HG_KS_LO64("v72", "v73", "%[p0l]", "%[p0h]", "v[74:75]", "v74", "v75")                                             \
  HG_KS_LO64("v88", "v89", "%[p6l]", "%[p6h]", "v[84:85]", "v84", "v85")                                             \
  "v_xor_b32_e32 v72, v74, v84\n\t"                                                                                  \
  "v_xor_b32_e32 v73, v75, v85\n\t"                                                                                  \
  "v_mad_u64_u32 v[74:75], %[junk], v72, %[p5l], 0\n\t"                                                              \
  "v_mov_b32 v68, v75\n\t"                                                                                           \
  "v_mad_u64_u32 v[76:77], %[junk], v73, %[p5l], v[68:69]\n\t"                                                       \
  "v_mad_u64_u32 v[76:77], vcc, v72, %[p5h], v[76:77]\n\t"                                                           \
  "v_mov_b32 v68, v77\n\t"                                                                                           \
  "v_mad_u64_u32 v[78:79], %[junk], v73, %[p5h], v[68:69]\n\t"                                                       \
  "v_addc_co_u32_e32 v79, vcc, 0, v79, vcc\n\t"                                                                      \
  "v_xor_b32_e32 v71, v76, v79\n\t"                                                                                  \
  "v_cmp_ge_u32_e64 %[mask], %[thrh], v71"
// The first mixup: lo64 -> {v74, v76}, hi64 + s -> U.  HG_KS_FIRST_n: the bounded text; HG_KS_FIRST_FULL_n: the general
// text for any 64-bit seed, which seeds of FIRST_SEED_END and more take.
//   17 <= K <= 24, mixup64<P3>(b, a, w0): x = seed + w0; b = K ^ lo; a = seed + hi
//   25 <= K <= 32, mixup64<P4>(a, b, w0): x = K + w0; a = seed ^ lo; b = K + hi
#define HG_KS_FIRST_FULL_3(W0L, W0H, W0)                                                                             \
  "v_lshl_add_u64 v[72:73], " W0 ", 0, %[seed]\n\t"                                                                  \
  HG_KS_MUL128_P3("v72", "v73", "%[seed]", "v[78:79]", "v79")
#define HG_KS_FIRST_FULL_4(W0L, W0H, W0)                                                                             \
  "v_lshl_add_u64 v[72:73], " W0 ", 0, %[kk]\n\t"                                                                    \
  HG_KS_MUL128("v72", "v73", "%[p4l]", "%[p4h]", "%[kk]", "v[78:79]", "v79")
#define HG_KS_FIRST_3(W0L, W0H, W0) HG_KS_MUL128_BOUNDED(W0L, W0H, "%[p3l]", "%[p3h]", "%[seedl]", "v[78:79]")
#define HG_KS_FIRST_4(W0L, W0H, W0) HG_KS_MUL128_BOUNDED(W0L, W0H, "%[p4l]", "%[p4h]", "%[kk]", "v[78:79]")
// 17 <= K <= 24: three stages
#define HG_KS_REST_3(W1, W2, W3)                                                                                     \
  "v_xor_b32_e32 v80, %[kk], v74\n\t"                                                                                \
  "v_mov_b32 v81, v76\n\t"                                                                                           \
  /* mixup64<P2>(a, b, w1): x = b + w1; a ^= lo; b += hi   (a = U, b = S1 -> a = S2, b = R) */                       \
  "v_lshl_add_u64 v[72:73], v[80:81], 0, " W1 "\n\t"                                                                 \
  HG_KS_MUL128("v72", "v73", "%[p2l]", "%[p2h]", "v[80:81]", "v[84:85]", "v85")                                      \
  "v_xor_b32_e32 v82, v78, v74\n\t"                                                                                  \
  "v_xor_b32_e32 v83, v79, v76\n\t"                                                                                  \
  /* mixup64<P1>(b, a, w2): x = a + w2; b ^= lo; a += hi   (a = S2, b = R -> b = S1, a = U) */                       \
  "v_lshl_add_u64 v[72:73], v[82:83], 0, " W2 "\n\t"                                                                 \
  HG_KS_MUL128_P1("v72", "v73", "v[82:83]", "v[78:79]", "v79")                                                       \
  "v_xor_b32_e32 v80, v84, v74\n\t"                                                                                  \
  "v_xor_b32_e32 v81, v85, v76\n\t"                                                                                  \
  HG_KS_FINAL("v[78:79]", "v78", "v79", "v[80:81]", "v80", "v81")
#define HG_KS_HASH_TEXT_3(W0L, W0H, W0, W1, W2, W3) HG_KS_FIRST_3(W0L, W0H, W0) HG_KS_REST_3(W1, W2, W3)
#define HG_KS_HASH_FULL_TEXT_3(W0L, W0H, W0, W1, W2, W3) HG_KS_FIRST_FULL_3(W0L, W0H, W0) HG_KS_REST_3(W1, W2, W3)
// 25 <= K <= 32: four stages (the first one's b is the length, a small constant)
#define HG_KS_REST_4(W1, W2, W3)                                                                                     \
  /* (first mixup: -> a = S1, b = U) */                                                                              \
  "v_xor_b32_e32 v80, %[seedl], v74\n\t"                                                                             \
  "v_xor_b32_e32 v81, %[seedh], v76\n\t"                                                                             \
  /* mixup64<P3>(b, a, w1): x = a + w1; b ^= lo; a += hi   (a = S1, b = U -> b = S2, a = R) */                       \
  "v_lshl_add_u64 v[72:73], v[80:81], 0, " W1 "\n\t"                                                                 \
  HG_KS_MUL128_P3("v72", "v73", "v[80:81]", "v[84:85]", "v85")                                                       \
  "v_xor_b32_e32 v82, v78, v74\n\t"                                                                                  \
  "v_xor_b32_e32 v83, v79, v76\n\t"                                                                                  \
  /* mixup64<P2>(a, b, w2): x = b + w2; a ^= lo; b += hi   (a = R, b = S2 -> a = S1, b = U) */                       \
  "v_lshl_add_u64 v[72:73], v[82:83], 0, " W2 "\n\t"                                                                 \
  HG_KS_MUL128("v72", "v73", "%[p2l]", "%[p2h]", "v[82:83]", "v[78:79]", "v79")                                      \
  "v_xor_b32_e32 v80, v84, v74\n\t"                                                                                  \
  "v_xor_b32_e32 v81, v85, v76\n\t"                                                                                  \
  /* mixup64<P1>(b, a, w3): x = a + w3; b ^= lo; a += hi   (a = S1, b = U -> b = S2, a = R) */                       \
  "v_lshl_add_u64 v[72:73], v[80:81], 0, " W3 "\n\t"                                                                 \
  HG_KS_MUL128_P1("v72", "v73", "v[80:81]", "v[84:85]", "v85")                                                       \
  "v_xor_b32_e32 v82, v78, v74\n\t"                                                                                  \
  "v_xor_b32_e32 v83, v79, v76\n\t"                                                                                  \
  HG_KS_FINAL("v[84:85]", "v84", "v85", "v[82:83]", "v82", "v83")
#define HG_KS_HASH_TEXT_4(W0L, W0H, W0, W1, W2, W3) HG_KS_FIRST_4(W0L, W0H, W0) HG_KS_REST_4(W1, W2, W3)
#define HG_KS_HASH_FULL_TEXT_4(W0L, W0H, W0, W1, W2, W3) HG_KS_FIRST_FULL_4(W0L, W0H, W0) HG_KS_REST_4(W1, W2, W3)
#define HG_KS_HASH_INPUTS                                                                                            \
  [seed] "s"(seed), [thrh] "s"((uint32_t)(threshold >> 32)), [kk] "n"(K), [p0l] "s"((uint32_t)P0), [p0h] "s"((uint32_t)(P0 >> 32)),     \
      [p1l] "s"((uint32_t)P1), [p1h] "s"((uint32_t)(P1 >> 32)), [p2l] "s"((uint32_t)P2), [p2h] "s"((uint32_t)(P2 >> 32)), \
      [p3l] "s"((uint32_t)P3), [p3h] "s"((uint32_t)(P3 >> 32)), [p5l] "s"((uint32_t)P5), [p5h] "s"((uint32_t)(P5 >> 32)), \
      [p6l] "s"((uint32_t)P6), [p6h] "s"((uint32_t)(P6 >> 32)), [p4l] "s"((uint32_t)P4), [p4h] "s"((uint32_t)(P4 >> 32)),   \
      [seedl] "s"((uint32_t)seed), [seedh] "s"((uint32_t)(seed >> 32))
#define HG_KS_HASH_CLOBBERS                                                                                          \
  "vcc", "v72", "v73", "v75", "v76", "v77", "v79", "v80", "v81", "v82", "v83", "v84",                 \
      "v85", "v86", "v87", "v88", "v89"

// ---- the statements --------------------------------------------------------------------------------------------------
// One asm statement per k-mer: wait for this k-mer's words (requested a whole hash earlier), request the next
// k-mer's into the other buffer (whole dwords of the chosen strand's phase image: two 8-byte reads at 4-byte aligned
// addresses, one dword and the last 1..4 bytes), hash, compare with the threshold.  The buffers are bound to fixed
// registers on both sides, so the compiler sees ordinary values and never copies them.
// Local names the statements use, all of the k-mer loop they stand in (kmers_asm in kmer_sample_shared): K, seed, threshold
// (kernel arguments); base, IMM (the next k-mer's strand base address and its compile-time offset into the phase images);
// KCASE (10 * dwords + bytes in the last dword: a statement is compiled for its own case); FB (first mixup: the bounded
// text); hmask, hjunk (candidate lanes / the SGPR pair of unused carry-outs); hlo0, hlo1, hhi (the hash: {hlo0 ^ hlo1, hhi});
// zpair (Z = {x, 0}, carried as a value); w0a..w0d, w1a..w1d (the word buffers: v[56:61] + v[90:91], v[62:67] + v[92:93]).
#define HG_KS_OFFS [o0] "n"(IMM), [o1] "n"(IMM + 8), [o2] "n"(IMM + 16), [o3] "n"(IMM + 20), [o4] "n"(IMM + 24), [o5] "n"(IMM + 28)
#define HG_KS_OUT0 "={v[56:57]}"(w0a), "={v[58:59]}"(w0b), "={v[60:61]}"(w0c), "={v[90:91]}"(w0d)
#define HG_KS_OUT1 "={v[62:63]}"(w1a), "={v[64:65]}"(w1b), "={v[66:67]}"(w1c), "={v[92:93]}"(w1d)
#define HG_KS_IN0 "{v[56:57]}"(w0a), "{v[58:59]}"(w0b), "{v[60:61]}"(w0c), "{v[90:91]}"(w0d)
#define HG_KS_IN1 "{v[62:63]}"(w1a), "{v[64:65]}"(w1b), "{v[66:67]}"(w1c), "{v[92:93]}"(w1d)
// cases (D, B, stages): HG_KS_FIRST requests k-mer 0's words; _EVEN / _ODD hash k-mer j from buffer j & 1 and request k-mer
// j + 1's into the other one; _LAST hashes the last k-mer
#define HG_KS_FIRST(D, B, N)                                                                                          \
  if constexpr (KCASE == 10 * D + B)                                                                                  \
    asm volatile(HG_KS_APPLY(HG_KS_READ_TEXT, D, B, HG_KS_REGS0) : HG_KS_OUT0 : [base] "v"(base), HG_KS_OFFS);
// (each k-mer statement twice: the first mixup's bounded text, FB, and the general one; one of them is compiled)
#define HG_KS_EVEN(D, B, N) HG_KS_EVEN1(D, B, HG_KS_HASH_TEXT_##N, FB) HG_KS_EVEN1(D, B, HG_KS_HASH_FULL_TEXT_##N, !FB)
#define HG_KS_ODD(D, B, N) HG_KS_ODD1(D, B, HG_KS_HASH_TEXT_##N, FB) HG_KS_ODD1(D, B, HG_KS_HASH_FULL_TEXT_##N, !FB)
#define HG_KS_LAST(D, B, N) HG_KS_LAST1(D, B, HG_KS_HASH_TEXT_##N, FB) HG_KS_LAST1(D, B, HG_KS_HASH_FULL_TEXT_##N, !FB)
#define HG_KS_HASH_OUTPUTS [mask] "=s"(hmask), [junk] "=&s"(hjunk), "=&{v74}"(hlo0), "=&{v78}"(hlo1), "=&{v71}"(hhi), "={v[68:69]}"(zpair)
#define HG_KS_EVEN1(D, B, HASH, COND)                                                                                 \
  if constexpr (KCASE == 10 * D + B && (COND))                                                                        \
    asm volatile(HG_KS_APPLY(HG_KS_WAIT_TEXT, D, B, HG_KS_REGS0) HG_KS_APPLY(HG_KS_READ_TEXT, D, B, HG_KS_REGS1) "\n\t" \
                 HG_KS_APPLY(HASH, HG_KS_PAIRS0)                                                                      \
                 : HG_KS_HASH_OUTPUTS, HG_KS_OUT1                                                                     \
                 : HG_KS_HASH_INPUTS, "{v[68:69]}"(zpair), [base] "v"(base), HG_KS_OFFS, HG_KS_IN0                    \
                 : HG_KS_HASH_CLOBBERS);
#define HG_KS_ODD1(D, B, HASH, COND)                                                                                  \
  if constexpr (KCASE == 10 * D + B && (COND))                                                                        \
    asm volatile(HG_KS_APPLY(HG_KS_WAIT_TEXT, D, B, HG_KS_REGS1) HG_KS_APPLY(HG_KS_READ_TEXT, D, B, HG_KS_REGS0) "\n\t" \
                 HG_KS_APPLY(HASH, HG_KS_PAIRS1)                                                                      \
                 : HG_KS_HASH_OUTPUTS, HG_KS_OUT0                                                                     \
                 : HG_KS_HASH_INPUTS, "{v[68:69]}"(zpair), [base] "v"(base), HG_KS_OFFS, HG_KS_IN1                    \
                 : HG_KS_HASH_CLOBBERS);
#define HG_KS_LAST1(D, B, HASH, COND)                                                                                 \
  if constexpr (KCASE == 10 * D + B && (COND))                                                                        \
    asm volatile(HG_KS_APPLY(HG_KS_WAIT_TEXT, D, B, HG_KS_REGS1) HG_KS_APPLY(HASH, HG_KS_PAIRS1)                      \
                 : HG_KS_HASH_OUTPUTS                                                                                 \
                 : HG_KS_HASH_INPUTS, "{v[68:69]}"(zpair), HG_KS_IN1                                                  \
                 : HG_KS_HASH_CLOBBERS);
#define HG_KS_ALL_CASES(X) X(5, 1, 3) X(5, 2, 3) X(5, 3, 3) X(5, 4, 3) X(6, 1, 3) X(6, 2, 3) X(6, 3, 3) X(6, 4, 3) \
                           X(7, 1, 4) X(7, 2, 4) X(7, 3, 4) X(7, 4, 4) X(8, 1, 4) X(8, 2, 4) X(8, 3, 4) X(8, 4, 4)
