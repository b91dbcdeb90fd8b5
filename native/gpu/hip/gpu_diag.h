// C ABI of the MI355X (gfx950) health-diagnostic kernels (libbgc_gpu_diag.so).
//
// The reference has no GPU code; these kernels implement the north
// star's "GPU discovery, health" for the node agent: before a GPU is advertised as
// schedulable `amd.com/gpu`, its HBM3E is pattern-tested at streaming bandwidth and
// every CU's matrix cores are checked with exact-integer MFMA tiles.  The library is
// dlopen()ed by the node agent and by the Python bindings so CPU-only hosts never need
// a HIP runtime.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BGC_DIAG_ABI_VERSION 15
#define BGC_DIAG_MAX_CU_KEYS 2048

// The data the diagnostics generate for themselves.  All arithmetic is modulo 2^32 (mix32) or
// 2^64 (mix64); u32(x) is the low 32 bits of x.
//
//   mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
//   mix64(x): x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33
//   trit(h):  (h mod 3) - 1, a value in {-1, 0, 1}
//
//  * HBM stream (bgc_diag_hbm).  A buffer is 16-byte elements i = 0.. of four 32-bit words each.
//    With pattern seed s, word c (0..3) of element i is mix32((w + c) ^ s) where
//    w = u32(4 i) ^ (u32(i >> 30) * 0x9e3779b9).  Timed iteration `it` (0-based) fills, copies and
//    checks with s = mix32(seed + (it + 1) * 0x9e3779b9); the untimed warm-up fill uses
//    s = mix32(seed).  The seeds of one run are pairwise distinct, so every word of an iteration's
//    pattern differs from the same word of any other iteration's and of the warm-up's: a fill or a
//    copy that wrote nothing cannot pass on what was there before.  Both buffers are set to 0xFF
//    bytes once after allocation.
//  * HBM walk (bgc_diag_hbm_walk).  key = mix64(0x9e3779b97f4a7c15 ^ seed).  In the first pass the
//    64-bit word at device address a holds a ^ key, in the second a ^ ~key.
//  * PCIe (bgc_diag_pcie).  64-bit word i of the transfer is mix32(u32(i) ^ seed) << 32 |
//    mix32(u32(i) ^ ~seed).  A transfer is at most 16 GiB, so u32(i) is all of i and both halves
//    take a different value in every word.
//  * GEMM soak (bgc_diag_gemm_soak).  Element i (row-major) of an operand with operand seed s is
//    trit(mix32(u32(i) ^ mix32(u32(i >> 32) + s))) as bf16; A[m][k] uses s = seed, Bt[n][k] (B
//    transposed) s = seed ^ 0xB7B7B7B7.  The reference checksums are rref = A (B 1), the row sums
//    of C, and cref = (1^T A) B, its column sums.
//  * Matrix-core tiles (bgc_diag_mfma, bgc_diag_mfma_lowp, bgc_diag_mfma_classic, bgc_diag_burn_dtype).
//    h(s, tile, r, c, which) = mix32(s ^ mix32(tile * 0x9e3779b9 + which) ^ u32(128 r + c)) and
//    op(s, tile, r, c, which) = trit(h(s, tile, r, c, which)).  A check wave w takes tiles
//    w * rounds .. w * rounds + rounds - 1, a throughput wave w tile w.
//  * Dense tiles: bf16 (16x16x32) and the classic fp16 (16x16x32), int8 (16x16x64), fp32 and fp64
//    (16x16x4).  A[row][k] = v(h(seed, tile, row, k, 0xA)) and B[k][col] = v(h(seed, tile, k, col, 0xB)) in
//    the path's element type.  v = trit, so the elements are op(), in the bf16 check and in every
//    path's throughput phase.  In a classic path's check phase v uses the width of the path's
//    multipliers, and every partial sum of a dot product, in any summation order, is an integer that
//    the accumulator holds exactly:
//      fp16:  v(h) = (h mod 1025) - 512, |v| <= 2^9 (exact in fp16: 11 significand bits);
//             |sum| <= 32 * 2^18 = 2^23 < 2^24, exact in the fp32 accumulator;
//      int8:  v(h) = int8(h & 0xff), |v| <= 2^7; |sum| <= 64 * 2^14 = 2^20, i32 accumulator;
//      fp32:  v(h) = (h mod 4095) - 2047; |sum| <= 4 * 2047^2 = 16760836 < 2^24;
//      fp64:  v(h) = int(h >> 6) - 2^25, |v| <= 2^25; |sum| <= 4 * 2^50 = 2^52 < 2^53.
//    The check recomputes each dot product in integer arithmetic (64-bit for fp64), converts it once
//    and compares for equality.  Lane l = 16 g + rc holds, of A row rc and of B column rc: bf16 and
//    fp16, k = 8 g + j in element j of 8; int8, k = 16 g + j in byte j of 16; fp32 and fp64, the single
//    element k = g.  The result lane l holds C[4 g + i][rc] in accumulator element i, except fp64,
//    whose lane holds C[g + 4 i][rc].
//  * MX tiles (16x16x128): A[row][k] = op(seed, tile, row, c(k), 0xA), B[k][col] =
//    op(seed, tile, col, c(k), 0xB), as e4m3 codes 0x38 / 0x00 / 0xB8 or e2m1 codes 0x2 / 0x0 / 0xA for
//    1 / 0 / -1.  c(k) numbers the elements in the order the lanes hold them (below): fp4, c(k) = k;
//    fp8, c(k) = 32 ((k mod 64) / 16) + 16 (k / 64) + k mod 16.  Scale exponents (E8M0 byte 127 + e)
//    of the K-block blk = k / 32: ea[row][blk] = op(seed ^ 0x5ca1e, tile, row, blk, 0xA), eb[col][blk] =
//    op(seed ^ 0x5ca1e, tile, col, blk, 0xB) in the scaled variants, 0 otherwise.  The exact result is
//    C[row][col] = sum_blk 2^(ea[row][blk] + eb[col][blk]) sum_{k in blk} A[row][k] B[k][col].
//    Lane l = 16 g + rc of the wave holds, of A row rc and of B column rc: fp8, K 16 g .. 16 g + 15 in
//    bytes 0..15 and K 64 + 16 g .. in bytes 16..31; fp4, K 32 g .. 32 g + 31 in 16 bytes, the even k in
//    the low nibble; the scale byte of (rc, block g).  The result lane l holds C[4 g + i][rc] in
//    accumulator element i.
//  * LDS march and rate (bgc_diag_lds).  A workgroup holds its CU's whole LDS as BGC_LDS_WORDS 32-bit
//    words.  For workgroup b of a launch, s_b = mix32(seed + (b + 1) * 0x9e3779b9); word j holds
//    P(b, j) = mix32(j ^ s_b) in pass 0 and ~P(b, j) in pass 1; the rate phase reads P.  mix32 is a
//    bijection, so the words of a workgroup are pairwise distinct, and the s_b of one launch are
//    pairwise distinct, so no word equals the same word of any other workgroup: a write that lands
//    at the wrong address reads back as a wrong value elsewhere, what the previous workgroup left on
//    the CU cannot pass, and every cell is checked holding both 0 and 1.
//  * L2 march and rate (bgc_diag_cache).  The L2 buffer is `grid` regions of region_words =
//    region_bytes / 4 32-bit words, `grid` being the device's CU count.  In round r (0-based) of the
//    march, workgroup b works on region (b + r) mod grid with s = mix32(seed + (r * grid + b + 1) *
//    0x9e3779b9); word j of the region holds mix32(j ^ s) in pass 0 and its inverse in pass 1.  The
//    rate phase uses the seed of round `rounds`: workgroup b fills region b with mix32(j ^ s),
//    s = mix32(seed + (rounds * grid + b + 1) * 0x9e3779b9).  The seeds of one run are pairwise
//    distinct, so what another round or another workgroup left in a region cannot pass.  A word of
//    the march is named by its index in the whole buffer, region * region_words + j.
//  * Infinity Cache (bgc_diag_cache).  Word i of the buffer holds mix32(u32(i) ^ mix32(~seed)); S is
//    the sum of all its words modulo 2^32.
//  * Vector ALU (bgc_diag_valu).  Every wave computes the same values; lane l (0..63) of a wave has its own
//    operands.  Operand word k of (class cls, round r, lane l) is
//      w(cls, r, k, l) = mix32(seed ^ mix32(cls << 24 | r << 16 | k << 8 | l)),   w_k for short.
//    Floating-point operands keep the hash's sign and all of its significand bits and bound the exponent:
//      f32(h)  = bits (h & 0x807fffff) | (127 + BGC_VALU_F32_EMIN + ((h >> 23) & 15)) << 23:  |x| in [2^-8, 2^8);
//      f16(h)  = of the low 16 bits of h, (h & 0x83ff) | (15 + BGC_VALU_F16_EMIN + ((h >> 10) & 7)) << 10:  |x| in
//                [2^-4, 2^4);  f16x2(h) = f16(h & 0xffff) | f16(h >> 16) << 16;
//      f64(hi, lo) = bits (hi & 0x800fffff) << 32 | (1023 + BGC_VALU_F32_EMIN + ((hi >> 20) & 15)) << 52 | lo.
//    With these ranges no operand and no correctly rounded result is a NaN, an infinity or a denormal, so the
//    verdict does not depend on the denormal mode.  fp32 and fp64: a product lies in [2^-16, 2^16) and a sum of a
//    product and an operand below 2^17; the operands are multiples of 2^-31 (2^-60) and their products of 2^-62
//    (2^-120), so a sum or difference that is not 0 is at least that, far above the smallest normal number 2^-126
//    (2^-1022); an exact 0 is allowed.  fp16: the operands are multiples of 2^-14, the smallest normal half, so a
//    sum that is not 0 is a normal number below 2^5; a product lies in [2^-8, 2^8); the FMA's addend takes the
//    sign of the product, so |a b + c| lies in [2^-4, 2^9), below the largest half 65504.  a b is a multiple of
//    2^-28 below 2^8 and c of 2^-14 below 2^4, so a b + c takes at most 37 bits and the host's double arithmetic
//    is exact: rounding it once to a half (to nearest even) is the fused result.  Conversions: f32 -> i32 takes
//    |x| < 2^8; f32 -> f16 and bf16 take |x| in [2^-8, 2^8), normal in both formats.
//    A round of a class produces these 32-bit result words, in this order (40 in all; BGC_VALU_ROUND_WORDS):
//      int32 (13), a = w_0, b = w_1, c = w_2, all modulo 2^32:  a + b;  a - b;  a b;  (a b) >> 32;
//        (a mod 2^24)(b mod 2^24) + c;  a << (c & 31);  a >> (c & 31);  a >> (c & 31) arithmetically;
//        (a >> (c & 31)) & (2^((c >> 8) & 31) - 1);  the bytes of the 64-bit a:b (b the low half) that the four
//        bytes of c & 0x07070707 select, byte i of the result by byte i of the selector;  (a:b >> (c & 31)) mod 2^32;
//        the number of 1 bits of a;  the number of leading 0 bits of a (32 for 0).
//      fp32 (6), x_k = f32(w_k):  fma(x_0, x_1, x_2);  fma(x_3, x_5, x_1) and fma(x_4, x_0, x_2) as one packed
//        FMA;  p = x_3 x_4;  p + x_5 (two roundings);  x_0 - x_4.
//      fp16 (3), packed halves A = f16x2(w_0), B = f16x2(w_1), C = (f16x2(w_2) & 0x7fff7fff) | ((A ^ B) &
//        0x80008000):  fma(A, B, C);  A + B;  A B, each on both halves, the low half in the low 16 bits.
//      fp64 (6), x_k = f64(w_2k, w_2k+1):  fma(x_0, x_1, x_2);  x_0 + x_1;  x_0 x_1, each as its low word, then
//        its high word.
//      cvt (5):  f32(w_0) to i32, truncated;  w_1 as an i32 to f32;  f32(w_2) to f16, zero-extended;  f16(w_3) to
//        f32;  bf16 of f32(w_4) | bf16 of f32(w_5) << 16.  All to nearest even where they round.
//      dot (2), a = w_0, b = w_1:  the sum of the four products of the signed bytes of a and b, plus w_2 >> 8
//        arithmetically;  the same of the unsigned bytes, plus w_2 >> 8.
//      trans (5):  2^x of x = f32 bits (w_0 & 0x807fffff) | (125 + ((w_0 >> 23) & 7)) << 23;  log2 of the positive
//        x with the significand of w_1 and exponent t - 5 for t = (w_1 >> 23) & 7 below 4, else t - 3 (so x lies
//        outside (0.5, 2) and |log2 x| >= 1);  1 / f32(w_2);  1 / sqrt|f32(w_3)|;  sqrt|f32(w_4)|.
//    Digest: d(cls, l) starts at 0x9e3779b9 + cls, and every result word v, round after round, is folded as
//    d = mix32(d ^ v).  mix32 is a bijection, so one changed word always changes the final digest.  The six
//    classes before trans are exact: every result is an integer or an IEEE result rounded to nearest even, and
//    the host compares all digests with its own.  The transcendental instructions are not bit-specified: their
//    digests are judged by consensus of the waves, and the raw results of one wave that holds the consensus
//    against double-precision libm, within BGC_VALU_*_ULPS units in the last place of the fp32 result.
//    Rate phase: 8 chains per lane, `rate_iters` iterations.  fp32 (chains of 2 packed components), fp16 (2
//    packed halves) and fp64 (1): x = fma(x, -1, 2047) from x = 1 + l + 64 k for component k = 2 chain + j (fp64:
//    k = chain), so x alternates between two integers below 2^11, exact in all three formats.  int32: x =
//    (x mod 2^24) * 0x5bd1e9 + 0x9e3779b9 from x = mix32(seed ^ (chain << 8 | l)).  trans: x = 2^x * 0.5 from
//    x = 0.25 + (l + 64 chain) / 1024, which settles at 1.  The end digest of a lane starts at 0x85ebca6b + rate
//    class and folds chain 0's words, then chain 1's, ... (fp32: component 0, component 1; fp16: one packed word;
//    fp64: low, high); the host computes it for the four exact classes and takes the waves' consensus for trans.
//  * Atomics (bgc_diag_atomic).  A launch is `grid` workgroups of four waves; wave w = 4 * workgroup + wave of the
//    workgroup, pair p = w * rounds + r for round r, P = 4 * grid * rounds pairs in all.  Operand word k of
//    (class cls, wave w, round r, lane l) is
//      a(cls, k, w, r, l) = mix32(mix32(seed ^ mix32(cls << 4 | k)) ^ (w << 12 | r << 6 | l)).
//    Every operation is chosen so that the final value of an element does not depend on the order in which its
//    operations arrive.  A class's table is rows of 64 elements.  In placement OWN it has 2 * grid rows and (w, r)
//    works on row 2 * workgroup + (w + r) mod 2, so the 2 * rounds pairs of one workgroup share a row; in placement
//    SHARED it has rows_cls = ceil(P / N_cls) rows and (w, r) works on row p mod rows_cls, so no element has more
//    than N_cls operations (N: int32, int64, f32 and f64 4096, pk16 128, cas and ticket 64).  Lane l works on
//    element l of the row.  Word k of a 32-bit class's element is at (k * rows + row) * 64 + l words into the class's
//    table, a 64-bit class's element at (row * 64 + l) * 2.
//      int32 (6 words), a_k = a(0, k, ..):  word 0 += a_0 modulo 2^32 from 0;  word 1 = min of the a_1 as signed
//        from 0x7fffffff;  word 2 = max of the a_2 as unsigned from 0;  word 3 &= a_3 from 0xffffffff;  word 4 |= a_4
//        from 0;  word 5 ^= a_5 from 0.
//      int64:  += a(1, 1, ..) << 32 | a(1, 0, ..) modulo 2^64 from 0.
//      f32:  += (a mod 4095) - 2047 as a float from 0.  |sum| <= 2047 * 4096 < 2^24 at any point of any order, so
//        every partial sum is exact.
//      f64:  += int(a >> 6) - 2^25 as a double from 0; |sum| <= 2^25 * 4096 = 2^37 < 2^53.
//      pk16 (2 words):  word 0 += (trit(a(4, 0, ..)), trit(a(4, 0, ..) >> 16)) as packed bf16, the first in the low
//        half;  word 1 the same of a(4, 1, ..) as packed fp16.  At most 128 operations, so every partial sum is an
//        integer of magnitude <= 128, exact in bf16 (8 significand bits) and in fp16.
//      cas:  every lane tries once to replace BGC_ATOMIC_EMPTY by its id = p * 64 + l and the wave stores the
//        ballot of the lanes that succeeded.  Exactly one of an element's contenders wins, and the element holds
//        the winner's id; which one wins is the hardware's choice.
//      ticket:  every lane adds 1 to the element, a counter from 0, takes the value before as its ticket and writes
//        id + 1 to slot `ticket` of the element's order array (capacity: OWN and LDS 2 * rounds, SHARED
//        ceil(P / rows)), if the ticket is below the capacity.  The counter ends at its number of pullers and the
//        order array is a permutation of their id + 1.
//      lds (9 words, OWN only, the table in the workgroup's LDS and copied out at the end), a_k = a(7, k, ..):
//        word 0 += a_0;  word 1 a ticket counter as above;  word 2 max unsigned of a_2;  word 3 min signed of a_3;
//        word 4 &= a_4;  word 5 |= a_5;  word 6 ^= a_6;  word 7 += (a_7 mod 4095) - 2047 as a float;  word 8 a cas
//        as above.  Initial values as in int32.
//    Rate phase: `rate_grid` workgroups (a multiple of 8), group g = (workgroup / 8) * 4 + wave of the workgroup, so
//    a group has the 8 waves of equal number of 8 consecutive workgroups.  A group owns 64 rows of 64 32-bit words;
//    in iteration i its waves add to row i mod 64, lane l to word l, for the visit j = i / 64.  With
//    h(cls, w, l) = mix32(mix32(seed ^ mix32(0x100 | cls)) ^ (w << 6 | l)):  f32 adds (-1)^j trit(h) as a float;  pk
//    bf16 adds (-1)^j (trit(h), trit(h >> 16)) as packed bf16;  u32 adds h + i * 0x9e3779b9 modulo 2^32;  rtn: lane
//    0 adds 1 to the group's head and sums the values it gets back.  The sign follows the visit, so whatever an
//    adder has added to one word is 0 or its trit at any time, a word's partial sums stay within +-8 in any order,
//    and a word ends at the sum of the trits of its adders if it was visited an odd number of times, else at 0.
//    A head ends at n = 8 * iters and the group's sums total n (n - 1) / 2.
//  * Register file (bgc_diag_regfile; regfile_ref.h holds this once).  Registers are numbered r = 0..511: v0..v255,
//    then a0..a255 as 256..511.  Wave w (global wave index) has the seed ws = mix32(seed + (w + 1) * 0x9e3779b9) and
//    lane l the hash h = mix32(ws + l).  A fill writes h + r * 0x61c88647 into register r of lane l, pass 1 of the
//    march the inverse.  Layout 0 leaves out v0..v7 and layout 1 v248..v255.  The rotate fills the ring v8..v255,
//    a0..a255 (ring index i is register 8 + i, 504 in all) as pass 0 does; a sweep moves the word at index i + 1 to
//    index i and the one at index 0 to the last, so after s sweeps index i holds the fill of index (i + s) mod 504.
//  * Cross-lane (bgc_diag_xlane; xlane_ref.h holds this once).  Every wave computes the same values.  Operand word k
//    of (class cls, round r, lane l) is the vector ALU's hash, w_k = mix32(seed ^ mix32(cls << 24 | r << 16 | k << 8 |
//    l)); a wave-uniform word is the hash of lane 64, which no wave has: u_k = w(cls, r, k, 64).  The model of the
//    instructions, written from the ISA manual and held to the MI355X by the GPU tests:
//      DPP gate.  Lane l is in row l / 16 and bank (l mod 16) / 4.  If its row_mask bit or its bank_mask bit is 0, or
//        EXEC disables it, the lane keeps `old` (the destination register's content).  Otherwise it takes the source
//        lane s; if s is invalid or disabled by EXEC it takes 0 with bound_ctrl:1 and keeps `old` with bound_ctrl:0.
//      DPP source lanes.  quad_perm: (l & ~3) + sel[l & 3].  row_shr:n: l - n, row_shl:n: l + n, both invalid outside
//        the row.  row_ror:n: the row's base + ((l mod 16) - n) mod 16.  wave_shr:1: l - 1, lane 0 invalid; wave_ror:1:
//        (l - 1) mod 64; wave_shl:1: l + 1, lane 63 invalid; wave_rol:1: (l + 1) mod 64.  row_mirror: base + 15 - l mod
//        16.  row_half_mirror: (l & ~7) + 7 - (l & 7).  row_bcast:15: lane 15 of the previous row; a lane of row 0
//        reads itself.  row_bcast:31: lane 31 for rows 2 and 3; a lane of rows 0 and 1 reads itself.  (Measured on the
//        MI355X with bound_ctrl:0: those rows are not invalid, they receive their own source and not `old`.)
//      A VOP2 with a DPP operand, v_add_u32_dpp vdst, src0, src1: vdst = dpp(src0) + src1 under the same gate, a lane
//        that is not written keeping vdst.
//      v_permlane32_swap vdst, src: lanes 32..63 of vdst swap with lanes 0..31 of src.  v_permlane16_swap: rows 1 and
//        3 of vdst swap with rows 0 and 2 of src.
//      ds_bpermute: dst[l] = src[(addr[l] >> 2) & 63]; an inactive source lane gives 0, an inactive lane is not
//        written.  ds_permute: dst[(addr[l] >> 2) & 63] = src[l].
//      ds_swizzle, bit mode: within each 32-lane half s = ((l & and) | or) ^ xor, the fields being offset bits 4:0,
//        9:5 and 14:10.  Quad mode (bit 15 set): offset bits 7:0 act as a quad_perm.
//      v_readfirstlane: the lowest lane set in EXEC.  v_mbcnt_lo then _hi: the number of set mask bits below the lane.
//    A round of a class produces these 32-bit result words, in this order (47 in all; BGC_XLANE_ROUND_WORDS).  Unless
//    said otherwise the source is w_0, `old` is w_1, both masks are 0xf and bound_ctrl is 0.
//      row (12), v_mov_b32_dpp:  quad_perm:[3,2,1,0];  [1,0,3,2];  [2,2,0,0];  row_shl:1;  row_shl:7;  row_shr:1;
//        row_shr:12;  row_ror:1;  row_ror:8;  row_ror:15;  row_mirror;  row_half_mirror.
//      wave (6), alike:  wave_shl:1;  wave_rol:1;  wave_shr:1;  wave_ror:1;  row_bcast:15;  row_bcast:31.
//      mask (6), alike:  row_shr:1 bound_ctrl:1;  wave_shl:1 bound_ctrl:1;  row_ror:3 row_mask:0xa;  row_ror:3
//        bank_mask:0x5;  row_bcast:15 row_mask:0xa;  row_shr:3 row_mask:0x6 bank_mask:0x9 bound_ctrl:1.
//      alu (3), all modulo 2^32:  v_add_u32_dpp row_shr:1 bound_ctrl:1 of w_0 and w_1 into a register that holds w_2;
//        v_min_u32_dpp row_ror:8 alike;  the inclusive prefix sum of w_2 over the 64 lanes by the DPP scan: acc =
//        dpp(x) + x with row_shr:1, acc += dpp(x) with row_shr:2 and row_shr:3 (all three bound_ctrl:1), then acc +=
//        dpp(acc) with row_shr:4 bank_mask:0xe, row_shr:8 bank_mask:0xc, row_bcast:15 row_mask:0xa and row_bcast:31
//        row_mask:0xc.
//      swap (4), vdst = w_0, src = w_1:  vdst, then src after v_permlane16_swap_b32;  the same after
//        v_permlane32_swap_b32 of the original two.
//      lds (6):  ds_bpermute_b32 with address (w_1 & 63) << 2;  ds_bpermute_b32 with address ((l + 1 + u_0 mod 63) &
//        63) << 2, a rotation by 1..63;  ds_permute_b32 with address (((u_1 | 1) l + u_2) & 63) << 2, a bijection;
//        ds_swizzle_b32 with and 0x1b, or 0x04, xor 0x11;  with and 0x0f, or 0x10, xor 0x0a;  in quad mode with
//        [1,3,0,2].
//      lane (6):  v_readlane_b32 of lane u_0 & 63 of w_0, in every lane;  v_readfirstlane_b32 of w_1, alike;  w_2 with
//        u_1 in lane u_2 & 63 by v_writelane_b32;  the low word of the ballot of w_0 & 1, in every lane;  its high
//        word;  v_mbcnt_lo then v_mbcnt_hi of that ballot.
//      exec (4), under the EXEC mask M = ((u_1 << 32 | u_0) | 1 << on) & ~(1 << off) with on = u_2 & 63 and off = (on +
//        1 + u_3 mod 63) & 63:  v_mov_b32_dpp wave_ror:1;  the same with bound_ctrl:1;  ds_bpermute_b32 with address
//        (w_2 & 63) << 2.  A lane that M disables holds `old`, w_1, in these three.  Then v_readfirstlane_b32 under M,
//        a scalar that every lane folds once EXEC is restored.
//    Digest: d(cls, l) starts at 0x9e3779b9 + cls and folds every result word v as d = mix32(d ^ v), as the vector
//    ALU's.  All eight classes are exact: the host compares every digest with its own, and there is no consensus.
//    Rate phase: 8 chains per lane, chain c of lane l filled with mix32(seed ^ (0x10000 | c << 8 | l)).  Every step is a
//    permutation of the wave's 8 * 64 values: dpp moves every chain by v_mov_b32_dpp row_ror:1;  swap exchanges
//    chains 2 j and 2 j + 1 by v_permlane32_swap_b32;  bpermute reads lane (l + 1) mod 64 by ds_bpermute_b32;
//    swizzle reads lane l ^ 0x15 of its half by ds_swizzle_b32 (and 0x1f, or 0, xor 0x15).  After `rate_iters` steps a
//    chain holds the fill moved by that permutation's rate_iters-th power.  The end digest of a lane starts at
//    0x85ebca6b + rate class and folds chain 0's word, then chain 1's, ...

typedef struct {
  uint64_t bytes;          // buffer size tested
  int iters;               // timed iterations per phase
  double write_gbps;       // pattern fill (store-only)
  double read_gbps;        // verify pass (load-only, compare in registers)
  double copy_gbps;        // device-to-device copy kernel (load+store bytes)
  uint64_t mismatches;     // 32-bit words that failed the pattern check, summed over `iters` (the
                           // counters are not reset between iterations)
  uint64_t first_bad_word; // index of the first failing 32-bit word (UINT64_MAX if none)
  double elapsed_ms;
} bgc_hbm_result;

typedef struct {
  uint64_t tiles_checked;   // 16x16x32 bf16 MFMA tiles verified element-wise
  uint64_t mismatches;      // output elements that differed from the exact result
  int cus_seen;             // distinct (XCC, SE, SH, CU) that executed the test
  int bad_cus;              // CUs with >= 1 mismatch
  int xccs_seen;            // distinct XCC ids
  double tflops;            // dense bf16 MFMA rate of the throughput phase
  int throughput_ok;        // throughput phase accumulators matched exactly
  double elapsed_ms;
  int bad_cu_keys[64];      // first bad CU keys (xcc<<8 | se<<5 | sh<<4 | cu)
  int xcc_waves[8];         // throughput-phase waves that ran on each XCC
  double xcc_wave_us[8];    // their mean duration (constant 100 MHz clock)
  double xcc_balance;       // fastest / slowest XCC mean wave time (1.0 = balanced)
} bgc_mfma_result;

int bgc_diag_abi_version(void);
int bgc_diag_device_count(void);
// Returns 0 on success, non-zero on HIP error (message via bgc_diag_last_error()).
int bgc_diag_hbm(int device, uint64_t bytes, int iters, uint32_t seed, bgc_hbm_result* out);
int bgc_diag_mfma(int device, int waves_per_cu, int throughput_iters, uint32_t seed, bgc_mfma_result* out);
typedef struct {
  uint64_t tiles_checked;         // 16x16x128 MX tiles verified element-wise (all four variants)
  uint64_t fp8_mismatches;        // e4m3 operands, unit E8M0 scales
  uint64_t fp8_scaled_mismatches; // e4m3 operands, per-32-element-block scales in {1/2, 1, 2}
  uint64_t fp4_mismatches;        // e2m1 operands, unit scales
  uint64_t fp4_scaled_mismatches; // e2m1 operands, block scales
  int cus_seen;
  int bad_cus;                    // CUs with >= 1 mismatch in any variant
  double fp8_tflops;              // dense MX-fp8 rate (v_mfma_scale_f32_16x16x128_f8f6f4)
  double fp4_tflops;              // dense MX-fp4 rate, same instruction
  int throughput_ok;              // both rate phases' accumulators matched exactly
  double elapsed_ms;
  int bad_cu_keys[64];
} bgc_lowp_result;

// The block-scaled low-precision matrix-core path (the one fp8/fp4 inference uses), which
// the bf16 checks above never exercise: exact-integer fp8 and fp4 tiles with and without
// E8M0 block scales on every CU, then the dense fp8 and fp4 rates.
int bgc_diag_mfma_lowp(int device, int waves_per_cu, int throughput_iters, uint32_t seed, bgc_lowp_result* out);
// The classic matrix-core paths, in the order of every [4] below and of `path` arguments.
#define BGC_CLASSIC_FP16 0  // v_mfma_f32_16x16x32_f16
#define BGC_CLASSIC_INT8 1  // v_mfma_i32_16x16x64_i8
#define BGC_CLASSIC_FP32 2  // v_mfma_f32_16x16x4_f32
#define BGC_CLASSIC_FP64 3  // v_mfma_f64_16x16x4_f64
typedef struct {
  uint64_t tiles_checked;   // 16x16xK tiles verified element-wise, all four paths
  uint64_t mismatches[4];   // output elements that differed from the exact result, by path
  int cus_seen;             // the smallest, over the four paths, of the distinct CUs that ran that path's check
  int bad_cus;              // CUs with >= 1 mismatch on any path
  double rate[4];           // dense rate of each path's throughput launch: TFLOP/s, int8 in TOP/s
  double rate_ms[4];        // device time of that launch
  int throughput_ok;        // every throughput launch's accumulators matched exactly
  double elapsed_ms;        // the check launches and the four timed launches
  int bad_cu_keys[64];
} bgc_classic_result;

// The fp16, int8, fp32-input and fp64 matrix-core paths, which differ from the bf16 one by more
// than an opcode (i32 accumulation, fp64's own multipliers and C/D map, one element per lane):
// exact tiles with full-width operands on every CU (`waves_per_cu` 1..64), then each path's dense
// rate over `throughput_iters` (1..65536) iterations of four MFMA chains per wave.
int bgc_diag_mfma_classic(int device, int waves_per_cu, int throughput_iters, uint32_t seed, bgc_classic_result* out);
// C[m,n] (double) = A[m,k] * B[k,n] on classic path `path`: A and B row-major in the path's element
// type (IEEE half bits, int8, float, double).  m, n multiples of 16 up to 4096; k a multiple of the
// path's K (32, 64, 4, 4) up to 8192.  Lets a test check each path's operand and result layout.
int bgc_diag_gemm_dtype(int device, int path, int m, int n, int k, const void* a, const void* b, double* c);
typedef struct {
  int launches;             // throughput kernels run back to back
  double elapsed_ms;        // wall time of the burn (device events)
  double tflops_mean;       // dense bf16 MFMA rate over the whole burn
  double tflops_min;        // slowest launch
  double tflops_first;      // first launch (includes the clock ramp from idle)
  double tflops_last;       // last launch vs the best one: a drop means the GPU throttled
  double tflops_max;
  uint64_t mismatches;      // accumulator errors over all launches
} bgc_burn_result;

// Sustained MFMA load for `duration_ms` (back-to-back throughput kernels of ~10 ms each):
// the node agent samples power, clocks, temperatures and throttle residency meanwhile.
// The first launch runs 2048 iterations; the later ones run the count that its time puts at ~10 ms,
// at least 64 and at most the largest with K * iters <= 2^23 (2^18 for bf16, K = 32; 2^16 for the MX
// tiles, K = 128).  The throughput kernel compares acc == iters * tile + c (c <= 3) in fp32, and a
// tile element is at most K in magnitude, so up to that count every value on either side is an
// integer below 2^24 and the comparison is exact; bgc_diag_mfma and bgc_diag_mfma_lowp take at most
// the same counts.
int bgc_diag_burn(int device, int duration_ms, int waves_per_cu, uint32_t seed, bgc_burn_result* out);
// The same load on another matrix-core path: BGC_BURN_FP8 / BGC_BURN_FP4 run the MX
// block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 rate kernel (rates in that dtype's FLOP/s).
#define BGC_BURN_BF16 0
#define BGC_BURN_FP8 1
#define BGC_BURN_FP4 2
int bgc_diag_burn_dtype(int device, int duration_ms, int waves_per_cu, uint32_t seed, int dtype, bgc_burn_result* out);
// C[m,n] (fp32) = A[m,k] * B[k,n], A/B bf16 bit patterns, row-major, via MFMA; the host
// compares C with its own fp32 product (m, n multiples of 16; k a multiple of 32).
int bgc_diag_gemm(int device, int m, int n, int k, const uint16_t* a_bf16, const uint16_t* b_bf16, float* c);
typedef struct {
  uint64_t bytes;           // transfer size (pinned host buffers)
  int iters;
  double h2d_gbps;          // best host -> device rate
  double d2h_gbps;          // best device -> host rate
  double bidir_gbps;        // both directions at once on two streams (sum of the two)
  uint64_t mismatches;      // 64-bit words that did not survive the H2D + D2H round trip
  double elapsed_ms;
} bgc_pcie_result;

// Host <-> device DMA over the GPU's PCIe link: a link that trained narrow or slow, or
// that replays, shows up here before a training job's data loader notices.
int bgc_diag_pcie(int device, uint64_t bytes, int iters, uint32_t seed, bgc_pcie_result* out);
typedef struct {
  int m, n, k;              // C[m,n] = A[m,k] * B[k,n], bf16 in, fp32 out
  int launches;             // back-to-back GEMMs
  double elapsed_ms;        // sum of the launches (device events)
  double tflops_mean;       // over all launches
  double tflops_best;
  uint64_t row_mismatches;  // C rows whose sum differs from A (B 1) or that hold an element that is not
                            // an exact integer (NaN and Inf included)  (after the first and the last launch)
  uint64_t col_mismatches;  // C columns alike, against (1^T A) B
  int tile;                 // 256 (256x256 tile, 8 waves) or 128 (128x128, 4 waves)
  int kernel;               // 2: 8-phase ping-pong (K % 128 == 0), 1: double-buffered
} bgc_soak_result;

// GEMM soak: an LDS-tiled (global_load_lds double buffering, XOR-swizzled LDS) bf16 MFMA
// GEMM run `launches` times back to back on operands in {-1, 0, 1}, checked by exact
// row/column checksums (ABFT).  m, n multiples of 128; k a multiple of 64.
int bgc_diag_gemm_soak(int device, int m, int n, int k, int launches, uint32_t seed, bgc_soak_result* out);
// The soak's GEMM kernel on caller operands: C[m,n] (fp32) = A[m,k] * Bt[n,k]^T, A/Bt bf16
// bit patterns, row-major (so both are K-contiguous, as the kernel reads them); same shape
// rules as bgc_diag_gemm_soak.  Lets a test compare the LDS-tiled kernel on random data
// with an independent fp32 product.
int bgc_diag_gemm_tiled(int device, int m, int n, int k, const uint16_t* a_bf16, const uint16_t* bt_bf16, float* c);
// The MX block-scaled matrix-core path (v_mfma_scale_f32_16x16x128_f8f6f4) on caller
// operands: C[m,n] (fp32) = sum_k a(m,k) 2^(sa(m,k/32)-127) * bt(n,k) 2^(sb(n,k/32)-127).
// fmt 0: fp8 e4m3 (OCP), one byte per element; fmt 4: fp4 e2m1, two per byte (element 2i in
// the low nibble).  a is m x k, bt is n x k (row-major, K-contiguous), the E8M0 scales are
// m x k/32 and n x k/32 bytes.  m, n multiples of 16; k a multiple of 128.  Lets a test
// check the hardware's operand and scale layout against an independent decode.
int bgc_diag_mx_gemm(int device, int fmt, int m, int n, int k, const uint8_t* a, const uint8_t* a_scales,
                     const uint8_t* bt, const uint8_t* bt_scales, float* c);

typedef struct {
  uint64_t free_bytes;        // hipMemGetInfo before the walk
  uint64_t total_bytes;
  uint64_t target_bytes;      // fraction * free_bytes
  uint64_t bytes_covered;     // allocated and written + verified with both patterns
  int chunks;                 // device allocations the walk spans
  int passes;                 // completed passes (2 = address pattern, then its inverse)
  uint64_t mismatches;        // 64-bit words that read back wrong
  uint64_t first_bad_addr;    // device address of the lowest failing word (0 = none)
  uint64_t first_bad_xor;     // expected ^ found at that word: the flipped bits
  double write_gbps;          // fill rate over the covered bytes
  double read_gbps;           // verify rate
  double alloc_ms;            // of which: allocating the chunks
  double elapsed_ms;          // wall time of the walk (allocation included)
  int budget_hit;             // 1 when the time budget ended the walk before both passes
} bgc_hbm_walk_result;

// Pattern walk of (nearly) all free HBM: allocates `fraction` of the free VRAM in chunks of
// `chunk_bytes`, writes every 64-bit word with its own device address XOR a seed-derived
// key, verifies all of it only after every chunk was written (a write that lands on the
// wrong row or stack shows up as a wrong address elsewhere), then repeats with the inverse
// so every cell is checked holding both 0 and 1.  Stops early after `budget_ms`.
int bgc_diag_hbm_walk(int device, double fraction, uint64_t chunk_bytes, int budget_ms, uint32_t seed,
                      bgc_hbm_walk_result* out);
#define BGC_LDS_WORDS 40960  // 163840 B: all of a CU's Local Data Share
typedef struct {
  int cus;                  // CUs of the device
  int cus_seen;             // distinct CUs that ran a march workgroup
  int bad_cus;
  uint64_t words_checked;   // 2 * BGC_LDS_WORDS per workgroup
  uint64_t mismatches;      // 32-bit words that read back wrong, both passes
  int first_bad_cu_key;     // lowest bad CU key, -1 if none
  uint32_t first_bad_word;  // lowest failing word index on that CU
  uint32_t bad_bits;        // OR of expected ^ found over all failures
  double read_tbps;         // rate phase: bytes read from LDS / device time, all CUs
  int rate_ok;              // every thread's sum matched
  int slowest_cu_key;       // CU whose rate workgroup took longest (constant clock), -1 if none ran
  double cu_balance;        // fastest / slowest CU time of the rate phase (1.0 = balanced)
  double elapsed_ms;
  int bad_cu_keys[64];
} bgc_lds_result;

// Every CU's Local Data Share, which the other checks never cover as a whole: a march of all
// 160 KiB per CU by `wgs_per_cu` (1..64) workgroups per CU, each of which fills the whole array and
// so is alone on its CU (16-byte stores, then the inverse as strided dword stores; verified with
// 16- and 8-byte loads), attributed to (XCC, SE, SH, CU); then `rate_iters` (1..65536) sweeps of
// conflict-free 16-byte reads over the array by one workgroup per CU, for the LDS read rate.
int bgc_diag_lds(int device, int wgs_per_cu, int rate_iters, uint32_t seed, bgc_lds_result* out);
#define BGC_L2_REGION_BYTES (96u << 10)  // default region of an L2 workgroup: 32 of them hold 3 MiB of an XCD's 4 MiB
#define BGC_L2_SLAB_BYTES (32u << 10)    // a region is 1..4 of these: 256 threads x 16 B x 8 loads in flight
typedef struct {
  int cus;                     // CUs of the device: workgroups of every L2 launch, regions of the L2 buffer
  int xccs_seen;               // distinct XCCs that ran a march workgroup
  int rounds;
  uint32_t region_bytes;
  uint64_t l2_words_checked;   // 2 * region words per workgroup and round
  uint64_t l2_mismatches;      // 32-bit words that read back wrong from L2, both passes, all rounds
  int l2_bad_xccs;             // XCCs with >= 1 mismatch
  uint64_t xcc_mismatches[8];  // by the XCC the workgroup ran on
  int first_bad_xcc;           // lowest bad XCC, -1 if none
  uint64_t first_bad_word;     // lowest failing word on that XCC, as an index in the whole L2 buffer
  uint32_t l2_bad_bits;        // OR of expected ^ found over all failures
  double l2_read_tbps;         // rate phase: bytes read through L2 / device time, all XCCs
  int l2_rate_ok;              // every thread's sum matched
  int xcc_wgs[8];              // rate workgroups that ran on each XCC
  double xcc_us[8];            // mean time of their loops (constant 100 MHz clock)
  int slowest_xcc;             // -1 if none ran
  double xcc_balance;          // fastest / slowest XCC mean loop time (1.0 = balanced)
  uint64_t ic_bytes;           // Infinity-Cache phase: buffer size, 0 when the phase is off
  uint64_t ic_words_checked;   // 2 * ic_bytes / 4: once after the fill, once after the timed sweeps
  uint64_t ic_mismatches;      // both checks summed
  uint64_t ic_first_bad_word;  // lowest failing 32-bit word of the buffer (UINT64_MAX if none)
  uint32_t ic_bad_bits;
  double ic_read_tbps;         // bytes of the timed sweeps / device time
  int ic_rate_ok;              // their 32-bit total was ic_sweeps * S (1 when the phase is off)
  double elapsed_ms;
} bgc_cache_result;

// The two SRAM levels between the LDS and HBM, which the other checks pass through without
// holding anything in them: each XCD's 4 MiB L2 and the 256 MiB Infinity Cache.
//  * L2: one workgroup per CU owns a region of `region_bytes` (32, 64, 96 or 128 KiB) of a buffer
//    sized for all of them.  `rounds` (1..16) march launches, each a fill with plain stores, a
//    verify with L1-bypassing loads, then the inverse (dword stores, 8-byte loads), attributed to
//    the XCC the workgroup ran on; the regions rotate over the workgroups from round to round.  Then
//    `l2_sweeps` (1..65536) L1-bypassing sweeps of each region, for the aggregate L2 read rate.
//  * Infinity Cache: off when `ic_bytes` is 0, else a buffer of `ic_bytes` (a multiple of 1 MiB, at
//    most 1 GiB) is filled, checked word by word, swept `ic_sweeps` (1..4096) times under a 32-bit
//    sum with every sweep's reads coming from another XCD than the last, and checked again.
int bgc_diag_cache(int device, int rounds, uint32_t region_bytes, int l2_sweeps, uint64_t ic_bytes, int ic_sweeps,
                   uint32_t seed, bgc_cache_result* out);
// The vector ALU's instruction classes, in the order of every [7] below and of a plant's `cls`.
#define BGC_VALU_INT32 0  // add, sub, v_mul_lo_u32, v_mul_hi_u32, 24-bit mad, shifts, v_bfe_u32, v_perm_b32, v_alignbit_b32, bit counts
#define BGC_VALU_FP32 1   // v_fma_f32 (issued in its v_fmac_f32 form), v_pk_fma_f32, v_mul_f32, v_add_f32, v_sub_f32
#define BGC_VALU_FP16 2   // v_pk_fma_f16, v_pk_add_f16, v_pk_mul_f16
#define BGC_VALU_FP64 3   // v_fma_f64 (issued in its v_fmac_f64 form), v_add_f64, v_mul_f64
#define BGC_VALU_CVT 4    // v_cvt_i32_f32, v_cvt_f32_i32, v_cvt_f16_f32, v_cvt_f32_f16, v_cvt_pk_bf16_f32
#define BGC_VALU_DOT 5    // v_dot4c_i32_i8, v_dot4_u32_u8
#define BGC_VALU_TRANS 6  // v_exp_f32, v_log_f32, v_rcp_f32, v_rsq_f32, v_sqrt_f32
#define BGC_VALU_CLASSES 7
#define BGC_VALU_ROUND_WORDS 40  // 32-bit result words of a lane per round: 13 + 6 + 3 + 6 + 5 + 2 + 5
// The rate phase's classes, in the order of every [5] below.
#define BGC_VALU_RATE_FP32 0   // v_pk_fma_f32, TFLOP/s (an FMA counts 2)
#define BGC_VALU_RATE_FP16 1   // v_pk_fma_f16, TFLOP/s
#define BGC_VALU_RATE_FP64 2   // v_fma_f64, TFLOP/s
#define BGC_VALU_RATE_INT32 3  // v_mad_u32_u24, TOP/s (a mad counts 2)
#define BGC_VALU_RATE_TRANS 4  // v_exp_f32, T instructions/s
#define BGC_VALU_RATE_CLASSES 5
// Smallest exponent of the fp32 / fp64 and of the fp16 operands; each range spans 16 (8) binades (derived above).
#define BGC_VALU_F32_EMIN (-8)
#define BGC_VALU_F16_EMIN (-4)
// Accuracy bounds of the transcendental instructions against double-precision libm, in units of the last place of the
// fp32 result: the largest error measured on the MI355X over seed 0x5eed and 16 other seeds at 64 rounds (69632 values
// per instruction; profiles/valu_diag/trans_ulps.json), rounded up to a whole unit, plus 1 for the host libm's own error.
#define BGC_VALU_EXP_ULPS 2.0   // v_exp_f32: measured 0.767
#define BGC_VALU_LOG_ULPS 2.0   // v_log_f32: measured 0.997
#define BGC_VALU_RCP_ULPS 2.0   // v_rcp_f32: measured 0.867
#define BGC_VALU_RSQ_ULPS 2.0   // v_rsq_f32: measured 0.821
#define BGC_VALU_SQRT_ULPS 2.0  // v_sqrt_f32: measured 0.906
typedef struct {
  int cus;                     // CUs of the device
  int cus_seen;                // distinct CUs that ran a check wave
  int simds_seen;              // distinct (CU, SIMD) that ran one
  uint64_t values_checked;     // result words folded into digests: waves * 64 * rounds * BGC_VALU_ROUND_WORDS
  uint64_t mismatches[7];      // (wave, lane) digests that differ from the host's (trans: from the consensus), by class
  int consensus_ok;            // more than half of the waves hold the same 64 trans digests
  uint64_t trans_out_of_bound; // raw trans results of one consensus wave beyond BGC_VALU_*_ULPS of libm
  int bad_cus;                 // CUs with >= 1 mismatch
  int bad_simds;               // (CU, SIMD) with >= 1 mismatch
  int first_bad_cu_key;        // the mismatch with the lowest (CU key, SIMD, wave, class, lane); each -1 if none
  int first_bad_simd;          // 0..3
  int first_bad_lane;
  int first_bad_class;
  uint64_t bad_lanes;          // bit l: lane l mismatched in some wave
  double rate[5];              // each rate class's launch: TFLOP/s, TOP/s or T instructions/s
  double rate_ms[5];           // device time of that launch
  int rate_ok;                 // every lane's end digest of every rate launch matched
  int slowest_cu_key;          // CU whose rate waves took longest in the mean over the five launches, -1 if none ran
  double cu_balance;           // fastest / slowest CU mean wave time (1.0 = balanced)
  double elapsed_ms;           // the check launch and the five timed launches
  int bad_cu_keys[64];
} bgc_valu_result;

// The vector ALU, which does every softmax, normalisation, activation, conversion and optimizer step and which
// referees every other check here: cus * `waves_per_simd` (1..8) workgroups of four waves, normally one per SIMD
// of a CU, each run `rounds` (1..64) rounds of a fixed sequence of integer, fp32, fp16, fp64, conversion, integer
// dot and transcendental instructions on per-lane operands and write one digest per lane and class with the CU
// and SIMD they ran on.  The device compares nothing: the host recomputes the exact classes and judges the
// transcendentals by consensus and against libm.  Then one timed launch per rate class, `rate_iters`
// (1..65536) iterations of 8 chains per lane.  Not covered: the scalar ALU, the floating-point dot products
// (their internal rounding is unspecified), fp8 conversions and the register file as a memory.
int bgc_diag_valu(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, bgc_valu_result* out);
// The atomic check's placements and classes, in the order of mismatches[2][8] below and of a plant's fields.
#define BGC_ATOMIC_OWN 0     // a table of the workgroup's own: its 4 waves contend, a wrong element names the CU
#define BGC_ATOMIC_SHARED 1  // one table for the launch: waves of workgroups far apart contend
#define BGC_ATOMIC_INT32 0   // global_atomic_add, _smin, _umax, _and, _or, _xor
#define BGC_ATOMIC_INT64 1   // global_atomic_add_x2
#define BGC_ATOMIC_F32 2     // global_atomic_add_f32
#define BGC_ATOMIC_F64 3     // global_atomic_add_f64
#define BGC_ATOMIC_PK16 4    // global_atomic_pk_add_bf16, global_atomic_pk_add_f16
#define BGC_ATOMIC_CAS 5     // global_atomic_cmpswap, returning, one try per lane
#define BGC_ATOMIC_TICKET 6  // global_atomic_add, returning
#define BGC_ATOMIC_LDS 7     // ds_add_u32, ds_add_rtn_u32, ds_max_u32, ds_min_i32, ds_and_b32, ds_or_b32, ds_xor_b32, ds_add_f32, ds_cmpst_rtn_b32; OWN only
#define BGC_ATOMIC_CLASSES 8
#define BGC_ATOMIC_EMPTY 0xffffffffu  // a cas element nobody has claimed
// The rate phase's classes, in the order of every [4] below.
#define BGC_ATOMIC_RATE_F32 0      // global_atomic_add_f32 without return, TB/s of added bytes
#define BGC_ATOMIC_RATE_PK_BF16 1  // global_atomic_pk_add_bf16 without return, TB/s of added bytes
#define BGC_ATOMIC_RATE_U32 2      // global_atomic_add without return, TB/s of added bytes
#define BGC_ATOMIC_RATE_RTN 3      // global_atomic_add with return by lane 0 of each wave, 1e9 adds/s
#define BGC_ATOMIC_RATE_CLASSES 4
typedef struct {
  int cus;                       // CUs of the device
  int cus_seen;                  // distinct CUs that ran a check workgroup
  uint64_t values_checked;       // 32-bit words of both tables and slots of the order arrays that the host judged
  uint64_t mismatches[2][8];     // [placement][class]: wrong words (64-bit classes: values; cas, ticket: elements)
  int bad_cus;                   // CUs whose workgroup has a wrong OWN or LDS element
  int first_bad_placement;       // the first wrong value in the order OWN, SHARED and class, word, row, lane; each -1 if none
  int first_bad_class;
  int first_bad_op;              // word of the element
  int64_t first_bad_element;     // row * 64 + lane in the class's table
  uint64_t first_bad_xor;        // expected ^ found (cas, ticket: 0)
  int64_t first_bad_delta;       // found - expected of an add word: modulo 2^32 or 2^64 as signed, a float's as an integer
                                 // (pk16: of the low half, of the high half if the low one is right); else 0
  uint64_t tickets_out_of_range; // tickets at or beyond their order array's capacity: counted, nothing stored
  double rate[4];                // each rate class's timed launch: TB/s of added bytes, rtn 1e9 adds/s
  double rate_ms[4];             // device time of that launch
  int rate_ok;                   // every end value of every rate launch matched its closed form
  int xcc_waves[8];              // rate waves that ran on each XCC, the four timed launches together
  double xcc_us[8];              // mean time of their loops (constant 100 MHz clock)
  int slowest_xcc;               // -1 if none ran
  double xcc_balance;            // fastest / slowest XCC mean loop time (1.0 = balanced)
  double elapsed_ms;             // the check launch and the four timed launches
  int bad_cu_keys[64];
} bgc_atomic_result;

// Atomic read-modify-writes, which every scatter, index_add, split-K and attention-backward accumulation, histogram
// and cross-workgroup ticket or claim relies on: cus * `wgs_per_cu` (1..8) workgroups of four waves each run `rounds`
// (1..64) rounds of every class above on hashed operands, in a table of their own and in one shared by the launch
// ("Atomics", above).  No wave waits for another, no operation is tried again, and a returned ticket is used as an
// index only below the capacity of its array.  The device compares nothing: the final tables go to the host, which
// recomputes them (atomic_ref.h).  Then a warm-up and a timed launch per rate class, `rate_iters` (1..65536)
// iterations, each wave instruction 256 contiguous bytes, 8 adders per word, the end values checked against their
// closed forms and the waves' loop times binned by XCC (reported only).  Agent scope and device memory only.
int bgc_diag_atomic(int device, int wgs_per_cu, int rounds, int rate_iters, uint32_t seed, bgc_atomic_result* out);
// The register-file check.  Registers are numbered 0..511 (v0..v255, then a0..a255 as 256..511); phases 0..3 are the
// march's (layout = phase >> 1, pass = phase & 1) and BGC_REGFILE_PHASE_ROTATE is the rotate.
#define BGC_REGFILE_REGS 512
#define BGC_REGFILE_TEMPS 8  // registers a march layout (and the rotate) keeps for the check's own use
#define BGC_REGFILE_PHASE_ROTATE 4
#define BGC_REGFILE_PHASES 5
#define BGC_REGFILE_PLANT_SLOTS 8
// The registers a value plant can name, by slot: the first and last of each half, one in the middle of each, and two
// of each layout's own eight, which only the other layout verifies.
#define BGC_REGFILE_PLANT_REGS {0, 5, 128, 250, 255, 256, 384, 511}
typedef struct {
  int cus;                     // CUs of the device
  int cus_seen;                // distinct CUs that ran a march wave
  int simds;                   // 4 * cus
  int simds_seen;              // distinct (CU, SIMD) that ran one
  int regs_marched;            // registers of a lane that some layout marches: 512
  int ring_regs;               // registers of the rotate's ring: 504
  uint64_t words_checked;      // waves * 64 * (2 layouts * 2 passes * 504 + ring_regs)
  uint64_t mismatches;         // vgpr_mismatches + agpr_mismatches + rotate_mismatches
  uint64_t vgpr_mismatches;    // wrong words of the march in v0..v255
  uint64_t agpr_mismatches;    // and in a0..a255
  uint64_t rotate_mismatches;  // wrong words of the ring after the timed rotate
  int bad_simds;               // (CU, SIMD) with >= 1 wrong word
  uint32_t bad_bits;           // OR of expected ^ found
  uint64_t bad_lane_mask;      // bit l: lane l held a wrong word
  int first_bad_cu_key;        // the lowest (CU key, SIMD) with a wrong word in the march, else in the rotate, and its
  int first_bad_simd;          // lowest (phase, register, lane); each -1 if none
  int first_bad_reg;           // 0..511
  int first_bad_lane;
  int first_bad_phase;
  double mov_tops;             // 1e12 lane-moves per second of the timed rotate: waves * 64 * ring_regs * sweeps / rotate_ms
  int rate_ok;                 // no rotate verify failed
  double simd_balance;         // fastest / slowest (CU, SIMD) mean loop time of the rotate (1.0 = balanced)
  int slowest_cu_key;          // the (CU, SIMD) whose rotate waves took longest in the mean; -1 if none ran
  int slowest_simd;
  double march_ms, rotate_ms;  // device time of the march launch and of the timed rotate launch
  double elapsed_ms;           // their sum
} bgc_regfile_result;

// The vector register file as a memory, 128 KiB per SIMD, which every operand of every other check passes through:
// cus * `wgs_per_cu` (1..8) workgroups of four waves whose kernel allocates all 512 registers of a lane, so that each
// wave is alone on a SIMD and its registers are that SIMD's whole file.  The march writes a per-wave pattern into
// every register of one layout (all but eight), verifies it, writes the inverse and verifies again, then does the same
// in a second layout that keeps eight other registers: together all 512.  The rotate fills a ring of 504 registers,
// moves it by one place `sweeps` (1..65536) times between two reads of the constant clock, and verifies where every
// word arrived: a moving-data check and the move rate.  A wrong word names its CU, SIMD, register, lane and phase.
// Not covered: the scalar registers, registers under matrix-core traffic, retention over time.
int bgc_diag_regfile(int device, int wgs_per_cu, int sweeps, uint32_t seed, bgc_regfile_result* out);
// The cross-lane check's instruction classes, in the order of every [8] below and of a plant's `cls`.
#define BGC_XLANE_ROW 0   // v_mov_b32_dpp: quad_perm, row_shl, row_shr, row_ror, row_mirror, row_half_mirror
#define BGC_XLANE_WAVE 1  // v_mov_b32_dpp: wave_shl, wave_rol, wave_shr, wave_ror, row_bcast:15, row_bcast:31
#define BGC_XLANE_MASK 2  // v_mov_b32_dpp with row_mask, bank_mask and bound_ctrl
#define BGC_XLANE_ALU 3   // v_add_u32_dpp, v_min_u32_dpp, the DPP prefix scan
#define BGC_XLANE_SWAP 4  // v_permlane16_swap_b32, v_permlane32_swap_b32
#define BGC_XLANE_LDS 5   // ds_bpermute_b32, ds_permute_b32, ds_swizzle_b32: the LDS crossbar, no LDS memory
#define BGC_XLANE_LANE 6  // v_readlane_b32, v_readfirstlane_b32, v_writelane_b32, the ballot (v_cmp), v_mbcnt_lo / _hi
#define BGC_XLANE_EXEC 7  // v_mov_b32_dpp, ds_bpermute_b32 and v_readfirstlane_b32 under a partial EXEC mask
#define BGC_XLANE_CLASSES 8
#define BGC_XLANE_ROUND_WORDS 47  // 32-bit result words of a lane per round: 12 + 6 + 6 + 3 + 4 + 6 + 6 + 4
// The rate phase's classes, in the order of every [4] below; all in 1e12 lane-moves per second (a 32-bit value
// arriving in a lane; a swap writes two registers and counts 128 a wave).
#define BGC_XLANE_RATE_DPP 0       // v_mov_b32_dpp row_ror:1
#define BGC_XLANE_RATE_SWAP 1      // v_permlane32_swap_b32
#define BGC_XLANE_RATE_BPERMUTE 2  // ds_bpermute_b32
#define BGC_XLANE_RATE_SWIZZLE 3   // ds_swizzle_b32
#define BGC_XLANE_RATE_CLASSES 4
typedef struct {
  int cus;                     // CUs of the device
  int cus_seen;                // distinct CUs that ran a check wave
  int simds_seen;              // distinct (CU, SIMD) that ran one
  uint64_t values_checked;     // result words folded into digests: waves * 64 * rounds * BGC_XLANE_ROUND_WORDS
  uint64_t mismatches[8];      // (wave, lane) digests that differ from the host's, by class
  int bad_cus;                 // CUs with >= 1 mismatch
  int bad_simds;               // (CU, SIMD) with >= 1 mismatch
  int first_bad_cu_key;        // the mismatch with the lowest (CU key, SIMD, wave, class, lane); each -1 if none
  int first_bad_simd;          // 0..3
  int first_bad_lane;          // the destination lane
  int first_bad_class;
  uint64_t bad_lanes;          // bit l: destination lane l mismatched in some wave
  double rate[4];              // each rate class's launch, 1e12 lane-moves per second
  double rate_ms[4];           // device time of that launch
  int rate_ok;                 // every lane's end digest of every rate launch matched
  int slowest_cu_key;          // CU whose rate waves took longest in the mean over the four launches, -1 if none ran
  double cu_balance;           // fastest / slowest CU mean wave time (1.0 = balanced)
  double elapsed_ms;           // the check launch and the four timed launches
  int bad_cu_keys[64];
} bgc_xlane_result;

// The paths that move a value from one lane of a wave to another, which carry every wave reduction (softmax and
// layer-norm row sums, __shfl_*, ballots, readfirstlane broadcasts, the matrix-core epilogue transposes): the DPP
// network of each SIMD's vector ALU, the swap path between half-waves, the LDS crossbar and the path between vector
// lanes and scalar registers.  cus * `waves_per_simd` (1..8) workgroups of four waves, normally one per SIMD of a CU,
// each run `rounds` (1..64) rounds of the fixed sequence above ("Cross-lane") on hashed operands and write one digest
// per lane and class with the CU and SIMD they ran on.  The results are pure data movement, so the device compares
// nothing and the host recomputes every digest (xlane_ref.h).  Then a warm-up and a timed launch per rate class,
// `rate_iters` (1..65536) steps of 8 chains per lane, the end values checked in closed form.  Not covered: DPP on
// 64-bit and 16-bit operands, SDWA, ds_swizzle's other modes, the cross-lane moves inside the matrix cores.
int bgc_diag_xlane(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, bgc_xlane_result* out);
// ---------------------------------------------------------------------------------------------
// Planted variants: FOR TESTS ONLY.  Each runs the same implementation as the entry point it is
// named after, with a list of deliberately wrong values ("plants") written into the diagnostic's
// own buffers or accumulators between the phase that produces the data and the phase that checks
// it, so a test can show that a wrong value reaches the counters; the *_delayed variants plant time
// instead, so a test can show that a slow wave or launch reaches the rates.  An empty list is the
// production behaviour.  Every plant is in bounds: a position outside the buffer, or a wave, lane, round,
// chain or element index out of range, a negative count or more than BGC_DIAG_MAX_PLANTS is
// refused with "invalid arguments" before the device is touched (only `wave` has to wait for the
// device's CU count).  The node agent and the diag worker never load these symbols.
#define BGC_DIAG_MAX_PLANTS 4096
#define BGC_PLANT_ALL_WAVES (-1)
#define BGC_MFMA_CHECK_ROUNDS 8  // tiles per wave of bgc_diag_mfma's check phase
#define BGC_LOWP_CHECK_ROUNDS 2  // and of each bgc_diag_mfma_lowp variant
#define BGC_CLASSIC_CHECK_ROUNDS 4  // and of each bgc_diag_mfma_classic path

typedef struct {
  uint64_t word32_index;  // 32-bit word of the buffer
  uint32_t xor_mask;
} bgc_hbm_plant;
// One fill, one copy, the plants XORed into the copy in order, one check.  The rates are those of
// that single cold iteration: no measurement.
int bgc_diag_hbm_planted(int device, uint64_t bytes, uint32_t seed, const bgc_hbm_plant* plants, int n,
                         bgc_hbm_result* out);

typedef struct {
  int pass;                // 0: address pattern, 1: its inverse
  int chunk;               // allocation, in the order they were made
  uint64_t word64_offset;  // 64-bit word inside that chunk
  uint64_t xor_mask;
} bgc_walk_plant;
typedef struct {
  uint64_t base;   // device address
  uint64_t bytes;
} bgc_walk_chunk;
// The walk over `bytes` (rounded down to 2 MiB) in chunks of `chunk_bytes`, without a time
// budget; each plant is applied after its pass's fill and before its check.  The first
// min(out->chunks, max_chunks) allocations are returned in `chunks`.  Fails if the device cannot
// allocate the chunks as `bytes` and `chunk_bytes` imply them.
int bgc_diag_hbm_walk_planted(int device, uint64_t bytes, uint64_t chunk_bytes, uint32_t seed,
                              const bgc_walk_plant* plants, int n, bgc_walk_chunk* chunks, int max_chunks,
                              bgc_hbm_walk_result* out);

typedef struct {
  uint64_t word64_index;  // 64-bit word of the transfer
  uint64_t xor_mask;
} bgc_pcie_plant;
// One timed iteration; the plants are XORed into the device buffer after the first upload and
// before the device-to-device and device-to-host copies of the round-trip check.
int bgc_diag_pcie_planted(int device, uint64_t bytes, uint32_t seed, const bgc_pcie_plant* plants, int n,
                          bgc_pcie_result* out);

// acc[i] of `lane` += delta in the check phase, before round `round`'s comparison, in wave `wave`
// (global wave index: block * 4 + wave of the block) or in every wave (BGC_PLANT_ALL_WAVES).  A
// delta that makes the value NaN counts as a mismatch like any other.
typedef struct {
  int wave, round, lane, i;
  float delta;
} bgc_mfma_check_plant;
// acc[chain][i] of `lane` += delta in the throughput phase, after the loop and before the comparison.
typedef struct {
  int wave, lane, chain, i;
  float delta;
} bgc_mfma_rate_plant;
int bgc_diag_mfma_planted(int device, int waves_per_cu, int throughput_iters, uint32_t seed,
                          const bgc_mfma_check_plant* check, int n_check, const bgc_mfma_rate_plant* rate, int n_rate,
                          bgc_mfma_result* out);
typedef struct {
  int variant;  // 0 fp8, 1 fp8 scaled, 2 fp4, 3 fp4 scaled
  bgc_mfma_check_plant at;
} bgc_lowp_check_plant;
typedef struct {
  int fmt;  // 0 fp8, 1 fp4
  bgc_mfma_rate_plant at;
} bgc_lowp_rate_plant;
int bgc_diag_mfma_lowp_planted(int device, int waves_per_cu, int throughput_iters, uint32_t seed,
                               const bgc_lowp_check_plant* check, int n_check, const bgc_lowp_rate_plant* rate,
                               int n_rate, bgc_lowp_result* out);
// The classic run takes the same plants with `variant` and `fmt` both naming the path
// (BGC_CLASSIC_*).  `delta` is converted to the path's accumulator type; on the int8 path a delta
// that is not a finite integer below 2^31 in magnitude is refused with "invalid arguments".
int bgc_diag_mfma_classic_planted(int device, int waves_per_cu, int throughput_iters, uint32_t seed,
                                  const bgc_lowp_check_plant* check, int n_check, const bgc_lowp_rate_plant* rate,
                                  int n_rate, bgc_classic_result* out);

// Delay plants: time instead of values.  Wave `wave` (global wave index, or BGC_PLANT_ALL_WAVES) of a
// throughput launch reaches the plant point after its loop and before its comparison, where the
// value plants above are applied.  There it waits until `ticks` of the constant clock (wall_clock64(),
// 100 MHz: the clock xcc_wave_us is measured with) have passed since it reached that point, and goes
// on; the wait is a loop on the clock difference with s_sleep between the reads and nothing else, so
// it ends after `ticks` whatever else happens, and the wave's values are untouched.  A wave that
// several plants name waits for the largest of their `ticks`.  `ticks` is 1..BGC_DIAG_MAX_DELAY_TICKS
// (100 ms at 100 MHz); 0, more, or `wave` < BGC_PLANT_ALL_WAVES is refused with "invalid arguments"
// before the device is touched.
#define BGC_DIAG_MAX_DELAY_TICKS 10000000u
typedef struct {
  int wave;
  uint32_t ticks;
} bgc_mfma_delay_plant;
// bgc_diag_mfma with `delays` applied in the timed throughput launch only: the warm-up launch and the
// check phase take none.  So the delayed waves' time shows in tflops, xcc_wave_us and xcc_balance, and
// nothing else of the result moves.
int bgc_diag_mfma_delayed(int device, int waves_per_cu, int throughput_iters, uint32_t seed,
                          const bgc_mfma_delay_plant* delays, int n, bgc_mfma_result* out);
// bgc_diag_burn_dtype with every wave of every launch whose index (0-based) is at least
// `first_delayed_launch` (>= 0) delayed by `ticks`; a `first_delayed_launch` the burn never reaches
// is a clean burn.  The MX rate kernels do not time themselves, which is why the delay counts from
// the plant point and not from the kernel's start.
int bgc_diag_burn_delayed(int device, int duration_ms, int waves_per_cu, uint32_t seed, int dtype,
                          int first_delayed_launch, uint32_t ticks, bgc_burn_result* out);
// bgc_diag_burn_dtype with value plants: launch `launch` (0-based) of the burn applies the plants that
// name it, after its loop and before its comparison; every other launch is the production kernel.  So
// each plant that changes a value adds one to `mismatches`, whichever launch it is in, and nothing
// else of the result moves.  A `launch` the burn never reaches has no effect; `launch` < 0 is refused
// with "invalid arguments" before the device is touched.
typedef struct {
  int launch;
  bgc_mfma_rate_plant at;
} bgc_burn_plant;
int bgc_diag_burn_planted(int device, int duration_ms, int waves_per_cu, uint32_t seed, int dtype,
                          const bgc_burn_plant* plants, int n, bgc_burn_result* out);

// C[row][col] += delta after launch `launch` and before its checksums.  Only the first and the
// last launch are verified: a plant on any other launch is invalid.
typedef struct {
  int launch, row, col;
  float delta;
} bgc_soak_plant;
int bgc_diag_gemm_soak_planted(int device, int m, int n, int k, int launches, uint32_t seed,
                               const bgc_soak_plant* plants, int n_plants, bgc_soak_result* out);

// lds[word] ^= xor_mask in march workgroup `wg` (or in every one, BGC_PLANT_ALL_WAVES), by its thread 0
// after pass `pass`'s fill and before its verify.  pass 0 or 1, word < BGC_LDS_WORDS, a non-zero
// mask, wg below the march's grid (CUs * wgs_per_cu).  The rate phase takes no plant.
typedef struct {
  int wg;
  int pass;
  uint32_t word;
  uint32_t xor_mask;
} bgc_lds_plant;
int bgc_diag_lds_planted(int device, int wgs_per_cu, int rate_iters, uint32_t seed, const bgc_lds_plant* plants, int n,
                         bgc_lds_result* out);

// region[word] ^= xor_mask in march workgroup `wg` (or in every one, BGC_PLANT_ALL_WAVES) of round
// `round`, by its thread 0 with a plain store after pass `pass`'s fill barrier and before its verify,
// so the line changes in the L2 that holds it.  round < rounds, pass 0 or 1, word < region_bytes / 4,
// a non-zero mask, wg below the grid (the CU count).  The rate phase takes no value plant.
typedef struct {
  int round;
  int wg;
  int pass;
  uint32_t word;
  uint32_t xor_mask;
} bgc_l2_plant;
// buffer[word] ^= xor_mask from the host: `when` 0 after the fill and before the first check (so
// both checks and the sweeps' sum see it), 1 after the timed sweeps and before the last check.
// word < ic_bytes / 4, a non-zero mask.
typedef struct {
  int when;
  uint64_t word;
  uint32_t xor_mask;
} bgc_ic_plant;
int bgc_diag_cache_planted(int device, int rounds, uint32_t region_bytes, int l2_sweeps, uint64_t ic_bytes, int ic_sweeps,
                           uint32_t seed, const bgc_l2_plant* l2_plants, int n_l2, const bgc_ic_plant* ic_plants, int n_ic,
                           bgc_cache_result* out);
// Workgroup `wg` (or every one, BGC_PLANT_ALL_WAVES) of the timed L2 rate launch waits `ticks`
// (1..BGC_DIAG_MAX_DELAY_TICKS) of the constant clock after its loop and before it reads its end time,
// as the matrix-core delay plants below do.  The warm-up launch, the march and the Infinity-Cache
// phase take none, and no value is touched: the time shows in l2_read_tbps, xcc_us, slowest_xcc and
// xcc_balance only.
typedef struct {
  int wg;
  uint32_t ticks;
} bgc_cache_delay_plant;
int bgc_diag_cache_delayed(int device, int rounds, uint32_t region_bytes, int l2_sweeps, uint64_t ic_bytes, int ic_sweeps,
                           uint32_t seed, const bgc_cache_delay_plant* delays, int n, bgc_cache_result* out);

// Result word `op` (below the class's count) of `lane` in round `round` of class `cls` ^= xor_mask before it is
// folded, in check wave `wave` (global wave index: workgroup * 4 + wave of the workgroup) or in every wave
// (BGC_PLANT_ALL_WAVES).  round < rounds, a non-zero mask, wave below the launch's cus * waves_per_simd * 4.
typedef struct {
  int wave, cls, round, lane, op;
  uint32_t xor_mask;
} bgc_valu_plant;
// The first word of chain `chain` (0..7) of `lane` ^= xor_mask after the loop of rate class `cls`'s timed launch.
typedef struct {
  int wave, cls, lane, chain;
  uint32_t xor_mask;
} bgc_valu_rate_plant;
int bgc_diag_valu_planted(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, const bgc_valu_plant* check,
                          int n_check, const bgc_valu_rate_plant* rate, int n_rate, bgc_valu_result* out);
// Wave `wave` (or every one) of rate class `cls`'s timed launch waits `ticks` (1..BGC_DIAG_MAX_DELAY_TICKS) of the
// constant clock after its loop and before it reads its end time.  No value is touched: the time shows in rate,
// rate_ms, slowest_cu_key and cu_balance only.
typedef struct {
  int wave, cls;
  uint32_t ticks;
} bgc_valu_delay_plant;
int bgc_diag_valu_delayed(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, const bgc_valu_delay_plant* delays,
                          int n, bgc_valu_result* out);

// Lane `lane` of check wave `wave` (global wave index, below the launch's cus * wgs_per_cu * 4) issues the atomic
// of word `op` (below the class's word count; 0 for int64, f32, f64, cas and ticket) of class `cls` in placement
// `placement` in round `round` `times` times instead of once: 0 is a lost update, 2 a doubled one, 1 with a non-zero
// mask a wrong operand.  The operand word (the hash a(cls, op, ..), of int64 its low word; the id of cas and ticket)
// is XORed with the mask.  Of several plants on one atomic the first in the list applies.  times 0..2, and a zero
// mask with times 1 is refused; LDS takes placement OWN only.
typedef struct {
  int placement, cls, op, wave, round, lane, times;
  uint32_t xor_mask;
} bgc_atomic_plant;
// Lane `lane` (rtn: 0) of wave `wave` of rate class `cls`'s timed launch issues the atomic of its last iteration
// `times` (0 or 2) times.
typedef struct {
  int cls, wave, lane, times;
} bgc_atomic_rate_plant;
int bgc_diag_atomic_planted(int device, int wgs_per_cu, int rounds, int rate_iters, uint32_t seed, const bgc_atomic_plant* plants, int n,
                            const bgc_atomic_rate_plant* rate, int n_rate, bgc_atomic_result* out);
// Wave `wave` (or every one, BGC_PLANT_ALL_WAVES) of rate class `cls`'s timed launch waits `ticks`
// (1..BGC_DIAG_MAX_DELAY_TICKS) of the constant clock after its loop and before it reads its end time.  No value is
// touched: the time shows in rate, rate_ms, xcc_us, slowest_xcc and xcc_balance only.
typedef struct {
  int cls, wave;
  uint32_t ticks;
} bgc_atomic_delay_plant;
int bgc_diag_atomic_delayed(int device, int wgs_per_cu, int rounds, int rate_iters, uint32_t seed, const bgc_atomic_delay_plant* delays,
                            int n, bgc_atomic_result* out);

// Register BGC_REGFILE_PLANT_REGS[slot] of `lane` ^= xor_mask in wave `wave` (global wave index, or every wave with
// BGC_PLANT_ALL_WAVES) after the fill of `phase` and before its verify; in BGC_REGFILE_PHASE_ROTATE before the sweeps,
// so the wrong word travels with the ring.  slot below BGC_REGFILE_PLANT_SLOTS, lane 0..63, a non-zero mask, and the
// phase must hold a pattern in that register (not one of its own eight), else "invalid arguments".
typedef struct {
  int wave, phase, slot, lane;
  uint32_t xor_mask;
} bgc_regfile_plant;
int bgc_diag_regfile_planted(int device, int wgs_per_cu, int sweeps, uint32_t seed, const bgc_regfile_plant* plants, int n,
                             bgc_regfile_result* out);
// Wave `wave` (or every one) of the timed rotate launch waits `ticks` (1..BGC_DIAG_MAX_DELAY_TICKS) of the constant
// clock after its loop and before it reads its end time.  No value is touched: the time shows in mov_tops, rotate_ms,
// slowest_cu_key, slowest_simd and simd_balance only.
typedef struct {
  int wave;
  uint32_t ticks;
} bgc_regfile_delay_plant;
int bgc_diag_regfile_delayed(int device, int wgs_per_cu, int sweeps, uint32_t seed, const bgc_regfile_delay_plant* delays, int n,
                             bgc_regfile_result* out);

// Result word `op` (below the class's count) of destination lane `lane` in round `round` of cross-lane class `cls`
// ^= xor_mask before it is folded, in check wave `wave` (global wave index) or in every wave (BGC_PLANT_ALL_WAVES):
// there is no consensus, so a plant on every wave is caught like any other.  round < rounds, a non-zero mask, wave
// below the launch's cus * waves_per_simd * 4.
typedef struct {
  int wave, cls, round, lane, op;
  uint32_t xor_mask;
} bgc_xlane_plant;
// The end value of chain `chain` (0..7) of `lane` ^= xor_mask after the loop of rate class `cls`'s timed launch.
typedef struct {
  int wave, cls, lane, chain;
  uint32_t xor_mask;
} bgc_xlane_rate_plant;
int bgc_diag_xlane_planted(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, const bgc_xlane_plant* check,
                           int n_check, const bgc_xlane_rate_plant* rate, int n_rate, bgc_xlane_result* out);
// Wave `wave` (or every one) of rate class `cls`'s timed launch waits `ticks` (1..BGC_DIAG_MAX_DELAY_TICKS) of the
// constant clock after its loop and before it reads its end time.  No value is touched: the time shows in rate,
// rate_ms, slowest_cu_key and cu_balance only.
typedef struct {
  int wave, cls;
  uint32_t ticks;
} bgc_xlane_delay_plant;
int bgc_diag_xlane_delayed(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, const bgc_xlane_delay_plant* delays,
                           int n, bgc_xlane_result* out);

// ---------------------------------------------------------------------------------------------
// Generated data: FOR TESTS ONLY, never loaded by the node agent or the diag worker.  Each runs
// the same implementation as the entry point it is named after and then copies the data that
// run generated ("the data the diagnostics generate", above) to host memory of the caller, so a
// test can compare it with an independent reference.  A null destination, or a run whose copies
// to the host exceed BGC_DIAG_MAX_DATA_BYTES in all, is refused with "invalid arguments" before
// the device is touched.
#define BGC_DIAG_MAX_DATA_BYTES (128ULL << 20)

// bgc_diag_hbm, then the copy buffer as the last iteration left it: `bytes` rounded down to 16,
// to `data`.
int bgc_diag_hbm_data(int device, uint64_t bytes, int iters, uint32_t seed, void* data, bgc_hbm_result* out);
// bgc_diag_hbm_walk_planted without plants, ended after `passes` (1 or 2) passes; then every
// chunk's contents, in the order of `chunks` and without gaps, to `data` (`bytes` rounded down to
// 2 MiB).  All chunks are returned: max_chunks must cover them.
int bgc_diag_hbm_walk_data(int device, uint64_t bytes, uint64_t chunk_bytes, int passes, uint32_t seed,
                           bgc_walk_chunk* chunks, int max_chunks, void* data, bgc_hbm_walk_result* out);
// bgc_diag_pcie with one iteration; the host buffer that the round-trip check compared with the
// pattern (`bytes` rounded down to 8) to `data`.
int bgc_diag_pcie_data(int device, uint64_t bytes, uint32_t seed, void* data, bgc_pcie_result* out);
typedef struct {
  uint16_t* a;    // m x k bf16 bit patterns
  uint16_t* bt;   // n x k
  int64_t* rref;  // m reference row checksums
  int64_t* cref;  // n reference column checksums
  float* c;       // m x n, after the launch
} bgc_soak_data;
// bgc_diag_gemm_soak with one launch; all five destinations are required.
int bgc_diag_gemm_soak_data(int device, int m, int n, int k, uint32_t seed, const bgc_soak_data* data,
                            bgc_soak_result* out);
#define BGC_TILE_BF16 0
#define BGC_TILE_FP8 1
#define BGC_TILE_FP4 2
typedef struct {
  uint32_t a[8], b[8];  // the lane's A and B fragment as the MFMA takes it (bf16 and fp4: 4 dwords, the rest 0)
  int32_t ea, eb;       // its scale exponents (E8M0 byte - 127)
  float acc[4];         // what the matrix core returned
  float expect[4];      // the check's own value of the same elements
} bgc_tile_lane;
// One wave runs the check's tile functions (pack, scale exponents, MFMA, expected values) on tile
// `tile` of matrix-core path `path` (BGC_TILE_*), with block scales if `scaled` (MX paths only),
// and every lane writes what it holds to lanes[0..63].
int bgc_diag_mfma_tile(int device, int path, int scaled, uint32_t seed, uint32_t tile, bgc_tile_lane* lanes);
typedef struct {
  uint32_t a[4], b[4];  // the lane's A and B fragment as the MFMA takes it (fp32: 1 dword, fp64: 2, the rest 0)
  double acc[4];        // what the matrix core returned
  double expect[4];     // the check's own value of the same elements
} bgc_classic_tile_lane;
// The same for check tile `tile` of classic path `path` (BGC_CLASSIC_*).
int bgc_diag_mfma_classic_tile(int device, int path, uint32_t seed, uint32_t tile, bgc_classic_tile_lane* lanes);
// The march with `grid` (1..4096) workgroups; workgroup `wg` (< grid) copies its whole array, as it
// is after pass `pass`'s (0 or 1) verify, to `data` (BGC_LDS_WORDS words).
int bgc_diag_lds_data(int device, uint32_t seed, int wg, int pass, int grid, void* data);
// bgc_diag_cache with the march ended after `passes` (1 or 2) passes of its last round; then the
// whole L2 buffer as the march left it (out->cus * region_bytes bytes) to `l2_data`, which holds
// `l2_capacity` bytes, and the Infinity-Cache buffer as the last check saw it (ic_bytes) to
// `ic_data`, which may be null when ic_bytes is 0.  l2_capacity + ic_bytes may not exceed
// BGC_DIAG_MAX_DATA_BYTES; a device whose L2 buffer exceeds l2_capacity is refused once its CU count
// is known.
int bgc_diag_cache_data(int device, int rounds, uint32_t region_bytes, int passes, int l2_sweeps, uint64_t ic_bytes,
                        int ic_sweeps, uint32_t seed, void* l2_data, uint64_t l2_capacity, void* ic_data,
                        bgc_cache_result* out);

// What one check wave produced, or what the host referee expects of every wave.
typedef struct {
  int cu_key, simd;                      // where the wave ran in the check launch; -1 in the host's expectation
  int rate_cu_key[BGC_VALU_RATE_CLASSES];  // the CU it ran on in each rate class's timed launch; -1 likewise
  uint32_t digests[BGC_VALU_CLASSES][64];  // [class][lane]
  uint32_t raw[64 * BGC_VALU_ROUND_WORDS * 64];  // [round][word][lane], the classes' words in class order; `rounds` rounds
} bgc_valu_wave;
// bgc_diag_valu with the plants of bgc_diag_valu_planted and the delays of bgc_diag_valu_delayed (any list may be empty),
// then wave `wave` (below the launch's wave count, refused once the CU count is known): where it ran, in the check launch
// and in every timed rate launch of this very run, since the dispatcher places a wave anew in every launch; its digests as
// it wrote them; and every result word as it folded it, plants applied.  So a test can compare the place that a planted or
// delayed run names with the place of the wave it planted.
int bgc_diag_valu_data(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, int wave, const bgc_valu_plant* check,
                       int n_check, const bgc_valu_rate_plant* rate, int n_rate, const bgc_valu_delay_plant* delays, int n_delay,
                       bgc_valu_wave* data, bgc_valu_result* out);
// The host referee's values for (seed, rounds): the digests it compares with, and every result word (trans: double
// libm rounded to float, which no digest is compared with).  Touches no device.
int bgc_diag_valu_expected(uint32_t seed, int rounds, bgc_valu_wave* data);

// Where everything of an atomic check with `grid` workgroups, `rounds` rounds and a rate phase of `rate_grid`
// workgroups lies ("Atomics", above), and the data the two entries below return: 32-bit words in this order, each
// section at data_off[] words from the start.
#define BGC_ATOMIC_DATA_OWN 0           // the OWN table: class cls at table_off[0][cls] words, rows[0][cls] rows
#define BGC_ATOMIC_DATA_SHARED 1        // the SHARED table alike, with [1]
#define BGC_ATOMIC_DATA_BALLOTS 2       // 64-bit winners' ballots of the cas: [OWN, SHARED, LDS][pair]
#define BGC_ATOMIC_DATA_ORDER_OWN 3     // (row * 64 + lane) * order_cap[0] + ticket
#define BGC_ATOMIC_DATA_ORDER_SHARED 4  // alike with order_cap[1]
#define BGC_ATOMIC_DATA_ORDER_LDS 5     // alike with order_cap[2]
#define BGC_ATOMIC_DATA_CU_KEYS 6       // the CU key each check workgroup recorded
#define BGC_ATOMIC_DATA_RATE_CU_KEYS 7  // [rate class][workgroup of the timed rate launch]
#define BGC_ATOMIC_DATA_SECTIONS 8
typedef struct {
  int grid, rate_grid, rounds, waves;
  uint32_t pairs;              // waves * rounds
  uint32_t rows[2][8];         // rows of a class's table (SHARED LDS: 0)
  uint32_t order_cap[3];       // slots of an element's order array: OWN, SHARED, LDS
  uint64_t table_off[2][8];    // first word of a class in its placement's table
  uint64_t data_off[8];
  uint64_t data_words[8];
  uint64_t total_words;
} bgc_atomic_layout;
// grid 1..16384, rate_grid a multiple of 8 in 8..4096, rounds 1..64.  Touches no device.
int bgc_diag_atomic_layout(int grid, int rate_grid, int rounds, bgc_atomic_layout* out);
// bgc_diag_atomic with the plants of bgc_diag_atomic_planted and the delays of bgc_diag_atomic_delayed (any list may
// be empty); then the final tables, the ballots, the order arrays and the CU keys of that very run to `data`, which
// holds `capacity` bytes (at most BGC_DIAG_MAX_DATA_BYTES; a device whose data exceeds it is refused once its CU
// count is known).
int bgc_diag_atomic_data(int device, int wgs_per_cu, int rounds, int rate_iters, uint32_t seed, const bgc_atomic_plant* plants, int n,
                         const bgc_atomic_rate_plant* rate, int n_rate, const bgc_atomic_delay_plant* delays, int n_delay, void* data,
                         uint64_t capacity, bgc_atomic_result* out);
// The host referee's tables for a launch of `grid` workgroups with `plants` applied, in the same layout (rate_grid
// taken as 8, the CU keys -1).  Of what the hardware's order decides it gives one admissible outcome: every cas goes
// to the contender with the lowest pair and every ticket is drawn in the order of the pairs.  Touches no device.
int bgc_diag_atomic_expected(uint32_t seed, int grid, int rounds, const bgc_atomic_plant* plants, int n, void* data, uint64_t capacity);
// The rate phase's end values for `rate_grid` workgroups: the groups' rows, (group * 64 + row) * 64 + lane, of classes
// f32, pk bf16 and u32 (rate_grid / 8 * 4 * 4096 words), the groups' heads of rtn (rate_grid / 8 * 4 words).
int bgc_diag_atomic_rate_expected(uint32_t seed, int rate_grid, int rate_iters, int cls, uint32_t* out, uint64_t capacity_words);

// Where a wave recorded that it ran.
typedef struct {
  int cu_key, simd;
} bgc_regfile_place;
// bgc_diag_regfile with the plants of bgc_diag_regfile_planted and the delays of bgc_diag_regfile_delayed (either list
// may be empty); then wave `wave`'s whole file as phase `phase` had it, words[register * 64 + lane]: after the fill and
// the plants of a march phase, or after the timed rotate's sweeps (the phase's own eight registers are 0); and the place
// every wave recorded in the march launch and in the timed rotate launch of this very run, march_places[wave] and
// rotate_places[wave], each with room for `max_waves`.  The copies, 128 KiB and 16 bytes a wave, may not exceed
// BGC_DIAG_MAX_DATA_BYTES; a launch of more than max_waves waves is refused once the CU count is known.
int bgc_diag_regfile_data(int device, int wgs_per_cu, int sweeps, uint32_t seed, int wave, int phase, const bgc_regfile_plant* plants, int n,
                          const bgc_regfile_delay_plant* delays, int n_delay, uint32_t* words, bgc_regfile_place* march_places,
                          bgc_regfile_place* rotate_places, int max_waves, bgc_regfile_result* out);
// The layouts (regfile_ref.h).  Touches no device.
typedef struct {
  int regs, lanes, temps, ring_regs, plant_slots;
  uint8_t marched[2][BGC_REGFILE_REGS];             // [layout][register]: 1 if the layout marches it
  int temp_regs[2][BGC_REGFILE_TEMPS];              // the registers a layout keeps; the rotate keeps layout 0's
  int ring[BGC_REGFILE_REGS];                       // ring index -> register, ring_regs entries
  int plant_regs[BGC_REGFILE_PLANT_SLOTS];
  uint8_t plant_phase_ok[BGC_REGFILE_PLANT_SLOTS][BGC_REGFILE_PHASES];  // 1 if a plant of that slot may name the phase
} bgc_regfile_layout;
int bgc_diag_regfile_layout(bgc_regfile_layout* out);
// What wave `wave` (>= 0) holds when phase `phase` is dumped in a run with `sweeps` sweeps and these plants, as
// bgc_diag_regfile_data returns it: after `sweeps` sweeps ring index i holds what the fill and the plants put at index
// (i + sweeps) mod ring_regs, so a planted word is found `sweeps` places down the ring.  Touches no device.
int bgc_diag_regfile_expected(uint32_t seed, int wave, int phase, int sweeps, const bgc_regfile_plant* plants, int n, uint32_t* words);

// What one cross-lane check wave produced, or what the host referee expects of every wave.
typedef struct {
  int cu_key, simd;                           // where the wave ran in the check launch; -1 in the host's expectation
  int rate_cu_key[BGC_XLANE_RATE_CLASSES];    // the CU it ran on in each rate class's timed launch; -1 likewise
  uint32_t digests[BGC_XLANE_CLASSES][64];    // [class][lane]
  uint32_t raw[64 * BGC_XLANE_ROUND_WORDS * 64];  // [round][word][lane], the classes' words in class order; `rounds` rounds
} bgc_xlane_wave;
// bgc_diag_xlane with the plants of bgc_diag_xlane_planted and the delays of bgc_diag_xlane_delayed (any list may be
// empty), then wave `wave` (below the launch's wave count, refused once the CU count is known): where it ran in the
// check launch and in every timed rate launch of this very run, its digests as it wrote them, and every result word
// as it folded it, plants applied.
int bgc_diag_xlane_data(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, int wave, const bgc_xlane_plant* check,
                        int n_check, const bgc_xlane_rate_plant* rate, int n_rate, const bgc_xlane_delay_plant* delays, int n_delay,
                        bgc_xlane_wave* data, bgc_xlane_result* out);
// The host referee's values for (seed, rounds): the digests it compares with and every result word.  Touches no device.
int bgc_diag_xlane_expected(uint32_t seed, int rounds, bgc_xlane_wave* data);

// PCI bus id of a HIP device ("0000:05:00.0", lower-case hex) — the key the node agent and
// the RCCL probe use to match a HIP device (renumbered inside a container) to amdsmi.
int bgc_diag_device_bdf(int device, char* buf, size_t len);
// Device name / gfx arch string, e.g. "gfx950".
int bgc_diag_device_arch(int device, char* buf, size_t len);
const char* bgc_diag_last_error(void);

#ifdef __cplusplus
}
#endif
