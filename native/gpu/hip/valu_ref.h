// The vector-ALU check's operands, its instruction sequence and the host's reference arithmetic
// (gpu_diag.h, "Vector ALU").  No HIP dependency: valu.hip includes it for both sides, and a plain
// C++17 program can include it alone to run the host referee, under a sanitizer for instance.
//
//  * The sequence of a round is written once, valu_round<Alu>(): the device runs it with an Alu of
//    gfx950 builtins (valu.hip), the host with HostAlu below, whose every operation is IEEE
//    round-to-nearest-even or integer arithmetic that owes nothing to the device: fmaf / fma for
//    the fused operations, exact double arithmetic and one rounding for fp16, plain integer code
//    for the rest.  Only the transcendentals are not bit-specified: HostAlu gives double-precision
//    libm rounded to float, which the referee uses for the accuracy bound and never for equality.
//  * Contraction is off in this header: a host compiler that fused `p + c` behind `p = a * b`
//    would compute another value than the two roundings the sequence asks for.
//  * Hazards on the host are shifts and signed overflow: every shift count is masked below the
//    width, every product and sum that may wrap is unsigned, and the float-to-int conversion takes
//    operands below 2^8.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gpu_diag.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")  // GCC ignores the STDC pragma and contracts by default where the target has an FMA
#else
#pragma STDC FP_CONTRACT OFF
#endif

#if defined(__HIPCC__)
#define BGC_VALU_HD __host__ __device__ __forceinline__
#else
#define BGC_VALU_HD inline
#endif

namespace bgc_valu {

constexpr int kClasses = BGC_VALU_CLASSES;
constexpr int kRoundWords = BGC_VALU_ROUND_WORDS;
// 32-bit result words of a class per round, and where a class starts among the 40 of a round
BGC_VALU_HD constexpr int class_words(int cls) {
  constexpr int words[kClasses] = {13, 6, 3, 6, 5, 2, 5};
  return words[cls];
}
BGC_VALU_HD constexpr int word_base(int cls) {
  int base = 0;
  for (int c = 0; c < cls; ++c) base += class_words(c);
  return base;
}
static_assert(word_base(kClasses) == kRoundWords, "the classes' words fill a round");

BGC_VALU_HD uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// operand word k of (class, round, lane)
BGC_VALU_HD uint32_t operand(uint32_t seed, int cls, int round, int k, int lane) {
  return mix32(seed ^ mix32(static_cast<uint32_t>(cls) << 24 | static_cast<uint32_t>(round) << 16 | static_cast<uint32_t>(k) << 8 |
                            static_cast<uint32_t>(lane)));
}

BGC_VALU_HD uint32_t digest_start(int cls) { return 0x9e3779b9U + static_cast<uint32_t>(cls); }

BGC_VALU_HD float f32_of(uint32_t bits) { return __builtin_bit_cast(float, bits); }
BGC_VALU_HD uint32_t bits_of(float x) { return __builtin_bit_cast(uint32_t, x); }
BGC_VALU_HD double f64_of(uint64_t bits) { return __builtin_bit_cast(double, bits); }
BGC_VALU_HD uint64_t bits_of(double x) { return __builtin_bit_cast(uint64_t, x); }

// Operand ranges (derived in gpu_diag.h): sign and significand of the hash, exponent emin + (field & mask).
BGC_VALU_HD uint32_t f32_bits(uint32_t h, int emin, uint32_t mask) {
  return (h & 0x807fffffU) | static_cast<uint32_t>(127 + emin + static_cast<int>((h >> 23) & mask)) << 23;
}
BGC_VALU_HD float f32_operand(uint32_t h) { return f32_of(f32_bits(h, BGC_VALU_F32_EMIN, 15)); }
BGC_VALU_HD uint32_t f16_bits(uint32_t h16) {  // of the low 16 bits of h16
  return (h16 & 0x83ffU) | ((static_cast<uint32_t>(15 + BGC_VALU_F16_EMIN) + ((h16 >> 10) & 7)) << 10);
}
BGC_VALU_HD uint32_t f16x2_bits(uint32_t h) { return f16_bits(h & 0xffffU) | f16_bits(h >> 16) << 16; }
BGC_VALU_HD double f64_operand(uint32_t hi, uint32_t lo) {
  const uint64_t field = static_cast<uint64_t>(1023 + BGC_VALU_F32_EMIN + static_cast<int>((hi >> 20) & 15));
  return f64_of(static_cast<uint64_t>(hi & 0x800fffffU) << 32 | field << 52 | lo);
}
// the log's operand: positive, exponent -5..-2 or 1..4, so outside (0.5, 2)
BGC_VALU_HD float log_operand(uint32_t h) {
  const int t = static_cast<int>((h >> 23) & 7);
  return f32_of((h & 0x007fffffU) | static_cast<uint32_t>(127 + (t < 4 ? t - 5 : t - 3)) << 23);
}

// The seven classes of one round for one lane.  put(word, bits) takes each 32-bit result word in
// order, word counting from 0 within the class; a 64-bit result is its low word, then its high.
template <class Alu, class Put>
BGC_VALU_HD void valu_int32(uint32_t seed, int round, int lane, Put&& put) {
  const uint32_t a = operand(seed, BGC_VALU_INT32, round, 0, lane), b = operand(seed, BGC_VALU_INT32, round, 1, lane),
                 c = operand(seed, BGC_VALU_INT32, round, 2, lane);
  put(0, a + b);
  put(1, a - b);
  put(2, a * b);
  put(3, Alu::mul_hi(a, b));
  put(4, Alu::mad24(a, b, c));
  put(5, a << (c & 31));
  put(6, a >> (c & 31));
  put(7, static_cast<uint32_t>(static_cast<int32_t>(a) >> (c & 31)));
  put(8, Alu::bfe(a, c & 31, (c >> 8) & 31));
  put(9, Alu::perm(a, b, c & 0x07070707U));
  put(10, Alu::alignbit(a, b, c & 31));
  put(11, Alu::popcount(a));
  put(12, Alu::clz(a));
}

template <class Alu, class Put>
BGC_VALU_HD void valu_fp32(uint32_t seed, int round, int lane, Put&& put) {
  float x[6];
  for (int k = 0; k < 6; ++k) x[k] = f32_operand(operand(seed, BGC_VALU_FP32, round, k, lane));
  put(0, bits_of(Alu::fma(x[0], x[1], x[2])));
  const float pa[2] = {x[3], x[4]}, pb[2] = {x[5], x[0]}, pc[2] = {x[1], x[2]};
  float pr[2];
  Alu::pk_fma(pa, pb, pc, pr);
  put(1, bits_of(pr[0]));
  put(2, bits_of(pr[1]));
  const float p = Alu::mul(x[3], x[4]);
  put(3, bits_of(p));
  put(4, bits_of(Alu::add(p, x[5])));  // two roundings: a contracted multiply-add would differ
  put(5, bits_of(Alu::sub(x[0], x[4])));
}

template <class Alu, class Put>
BGC_VALU_HD void valu_fp16(uint32_t seed, int round, int lane, Put&& put) {
  const uint32_t a = f16x2_bits(operand(seed, BGC_VALU_FP16, round, 0, lane)), b = f16x2_bits(operand(seed, BGC_VALU_FP16, round, 1, lane));
  // the addend takes the sign of the product, half by half: no cancellation, so no denormal result
  const uint32_t c = (f16x2_bits(operand(seed, BGC_VALU_FP16, round, 2, lane)) & 0x7fff7fffU) | ((a ^ b) & 0x80008000U);
  put(0, Alu::pk_fma_f16(a, b, c));
  put(1, Alu::pk_add_f16(a, b));
  put(2, Alu::pk_mul_f16(a, b));
}

template <class Alu, class Put>
BGC_VALU_HD void valu_fp64(uint32_t seed, int round, int lane, Put&& put) {
  double x[3];
  for (int k = 0; k < 3; ++k) {
    x[k] = f64_operand(operand(seed, BGC_VALU_FP64, round, 2 * k, lane), operand(seed, BGC_VALU_FP64, round, 2 * k + 1, lane));
  }
  const uint64_t r[3] = {bits_of(Alu::fma(x[0], x[1], x[2])), bits_of(Alu::add(x[0], x[1])), bits_of(Alu::mul(x[0], x[1]))};
  for (int k = 0; k < 3; ++k) {
    put(2 * k, static_cast<uint32_t>(r[k]));
    put(2 * k + 1, static_cast<uint32_t>(r[k] >> 32));
  }
}

template <class Alu, class Put>
BGC_VALU_HD void valu_cvt(uint32_t seed, int round, int lane, Put&& put) {
  uint32_t w[6];
  for (int k = 0; k < 6; ++k) w[k] = operand(seed, BGC_VALU_CVT, round, k, lane);
  put(0, static_cast<uint32_t>(Alu::f32_to_i32(f32_operand(w[0]))));
  put(1, bits_of(Alu::i32_to_f32(static_cast<int32_t>(w[1]))));
  put(2, Alu::f32_to_f16(f32_operand(w[2])));
  put(3, bits_of(Alu::f16_to_f32(f16_bits(w[3] & 0xffffU))));
  put(4, Alu::pk_bf16(f32_operand(w[4]), f32_operand(w[5])));
}

template <class Alu, class Put>
BGC_VALU_HD void valu_dot(uint32_t seed, int round, int lane, Put&& put) {
  const uint32_t a = operand(seed, BGC_VALU_DOT, round, 0, lane), b = operand(seed, BGC_VALU_DOT, round, 1, lane),
                 c = operand(seed, BGC_VALU_DOT, round, 2, lane);
  // accumulators of 24 bits: no sum reaches the overflow that a clamp would decide
  put(0, static_cast<uint32_t>(Alu::sdot4(static_cast<int32_t>(a), static_cast<int32_t>(b), static_cast<int32_t>(c) >> 8)));
  put(1, Alu::udot4(a, b, c >> 8));
}

// operand of transcendental `op` (kExp2 .. kSqrt)
BGC_VALU_HD float trans_operand(uint32_t seed, int round, int lane, int op) {
  const uint32_t w = operand(seed, BGC_VALU_TRANS, round, op, lane);
  switch (op) {
    case 0: return f32_of(f32_bits(w, -2, 7));  // |x| in [2^-2, 2^6): 2^x is a normal number
    case 1: return log_operand(w);
    case 2: return f32_operand(w);
    default: return f32_of(f32_bits(w, BGC_VALU_F32_EMIN, 15) & 0x7fffffffU);
  }
}

template <class Alu, class Put>
BGC_VALU_HD void valu_trans(uint32_t seed, int round, int lane, Put&& put) {
  put(0, bits_of(Alu::exp2(trans_operand(seed, round, lane, 0))));
  put(1, bits_of(Alu::log2(trans_operand(seed, round, lane, 1))));
  put(2, bits_of(Alu::rcp(trans_operand(seed, round, lane, 2))));
  put(3, bits_of(Alu::rsq(trans_operand(seed, round, lane, 3))));
  put(4, bits_of(Alu::sqrt(trans_operand(seed, round, lane, 4))));
}

// put(class, word, bits) for the 40 words of a round in order
template <class Alu, class Put>
BGC_VALU_HD void valu_round(uint32_t seed, int round, int lane, Put&& put) {
  valu_int32<Alu>(seed, round, lane, [&](int w, uint32_t v) { put(BGC_VALU_INT32, w, v); });
  valu_fp32<Alu>(seed, round, lane, [&](int w, uint32_t v) { put(BGC_VALU_FP32, w, v); });
  valu_fp16<Alu>(seed, round, lane, [&](int w, uint32_t v) { put(BGC_VALU_FP16, w, v); });
  valu_fp64<Alu>(seed, round, lane, [&](int w, uint32_t v) { put(BGC_VALU_FP64, w, v); });
  valu_cvt<Alu>(seed, round, lane, [&](int w, uint32_t v) { put(BGC_VALU_CVT, w, v); });
  valu_dot<Alu>(seed, round, lane, [&](int w, uint32_t v) { put(BGC_VALU_DOT, w, v); });
  valu_trans<Alu>(seed, round, lane, [&](int w, uint32_t v) { put(BGC_VALU_TRANS, w, v); });
}

// ---------------------------------------------------------------------------------------------
// host arithmetic

// an IEEE half as the double it encodes, and a double rounded once (to nearest even) to a half
inline double f16_to_double(uint32_t h) {
  const int e = static_cast<int>((h >> 10) & 31);
  const double m = static_cast<double>(h & 0x3ff);
  const double mag = e == 0 ? ldexp(m, -24) : e == 31 ? (m == 0 ? INFINITY : NAN) : ldexp(1024.0 + m, e - 25);
  return (h & 0x8000) ? -mag : mag;
}

inline uint32_t f16_from_double(double x) {
  const uint64_t b = bits_of(x);
  const uint32_t sign = static_cast<uint32_t>(b >> 63) << 15;
  const int field = static_cast<int>((b >> 52) & 0x7ff);
  const uint64_t m = b & ((1ULL << 52) - 1);
  if (field == 0x7ff) return sign | 0x7c00 | (m ? 0x200 : 0);
  const int e = field - 1023;
  if (e > 15) return sign | 0x7c00;
  if (e < -14) return sign | static_cast<uint32_t>(nearbyint(fabs(x) * 16777216.0));  // a denormal half (or 0): units of 2^-24
  const uint64_t rest = m & ((1ULL << 42) - 1), half = 1ULL << 41;
  uint32_t h = static_cast<uint32_t>(e + 15) << 10 | static_cast<uint32_t>(m >> 42);
  if (rest > half || (rest == half && (h & 1))) h++;  // a carry out of the significand raises the exponent
  return sign | (h < 0x7c00 ? h : 0x7c00);
}

// op(a, b, c) on both halves of packed fp16 words, in exact double arithmetic with one rounding
template <class Op>
uint32_t f16x2_map(uint32_t a, uint32_t b, uint32_t c, Op&& op) {
  const uint32_t lo = f16_from_double(op(f16_to_double(a & 0xffff), f16_to_double(b & 0xffff), f16_to_double(c & 0xffff)));
  const uint32_t hi = f16_from_double(op(f16_to_double(a >> 16), f16_to_double(b >> 16), f16_to_double(c >> 16)));
  return lo | hi << 16;
}

enum Trans { kExp2, kLog2, kRcp, kRsq, kSqrt };
constexpr double kTransUlps[5] = {BGC_VALU_EXP_ULPS, BGC_VALU_LOG_ULPS, BGC_VALU_RCP_ULPS, BGC_VALU_RSQ_ULPS, BGC_VALU_SQRT_ULPS};

inline double trans_ref(int op, double x) {
  switch (op) {
    case kExp2: return exp2(x);
    case kLog2: return log2(x);
    case kRcp: return 1.0 / x;
    case kRsq: return 1.0 / sqrt(x);
    default: return sqrt(x);
  }
}

// |got - ref| in units of the last place of ref as an fp32 number; infinite for a NaN
inline double ulps_off(float got, double ref) {
  const double err = fabs(static_cast<double>(got) - ref) / ldexp(1.0, ilogb(ref) - 23);
  return err == err ? err : INFINITY;
}

struct HostAlu {
  static uint32_t mul_hi(uint32_t a, uint32_t b) { return static_cast<uint32_t>((static_cast<uint64_t>(a) * b) >> 32); }
  static uint32_t mad24(uint32_t a, uint32_t b, uint32_t c) {
    return static_cast<uint32_t>(static_cast<uint64_t>(a & 0xffffff) * (b & 0xffffff)) + c;
  }
  static uint32_t bfe(uint32_t a, uint32_t offset, uint32_t width) { return (a >> offset) & ((1u << width) - 1); }
  // byte i of the result is byte sel[i] (0..7) of the 64-bit a:b, b being the low half
  static uint32_t perm(uint32_t a, uint32_t b, uint32_t sel) {
    const uint64_t ab = static_cast<uint64_t>(a) << 32 | b;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= static_cast<uint32_t>((ab >> (8 * ((sel >> (8 * i)) & 7))) & 0xff) << (8 * i);
    return r;
  }
  static uint32_t alignbit(uint32_t a, uint32_t b, uint32_t shift) {
    return static_cast<uint32_t>((static_cast<uint64_t>(a) << 32 | b) >> shift);
  }
  static uint32_t popcount(uint32_t a) {
    uint32_t n = 0;
    for (; a; a &= a - 1) n++;
    return n;
  }
  static uint32_t clz(uint32_t a) {
    uint32_t n = 0;
    for (uint32_t bit = 0x80000000U; bit && !(a & bit); bit >>= 1) n++;
    return n;
  }
  static float fma(float a, float b, float c) { return fmaf(a, b, c); }
  static void pk_fma(const float a[2], const float b[2], const float c[2], float r[2]) {
    r[0] = fmaf(a[0], b[0], c[0]);
    r[1] = fmaf(a[1], b[1], c[1]);
  }
  static float mul(float a, float b) { return a * b; }
  static float add(float a, float b) { return a + b; }
  static float sub(float a, float b) { return a - b; }
  static uint32_t pk_fma_f16(uint32_t a, uint32_t b, uint32_t c) {
    return f16x2_map(a, b, c, [](double x, double y, double z) { return x * y + z; });
  }
  static uint32_t pk_add_f16(uint32_t a, uint32_t b) {
    return f16x2_map(a, b, 0, [](double x, double y, double) { return x + y; });
  }
  static uint32_t pk_mul_f16(uint32_t a, uint32_t b) {
    return f16x2_map(a, b, 0, [](double x, double y, double) { return x * y; });
  }
  static double fma(double a, double b, double c) { return ::fma(a, b, c); }
  static double add(double a, double b) { return a + b; }
  static double mul(double a, double b) { return a * b; }
  static int32_t f32_to_i32(float x) { return static_cast<int32_t>(x); }  // truncates; |x| < 2^8
  static float i32_to_f32(int32_t x) { return static_cast<float>(x); }
  static uint32_t f32_to_f16(float x) { return f16_from_double(x); }
  static float f16_to_f32(uint32_t h) { return static_cast<float>(f16_to_double(h)); }
  static uint32_t bf16(float x) {
    const uint32_t b = bits_of(x);
    return (b + 0x7fff + ((b >> 16) & 1)) >> 16;
  }
  static uint32_t pk_bf16(float lo, float hi) { return bf16(lo) | bf16(hi) << 16; }
  static int32_t sdot4(int32_t a, int32_t b, int32_t c) {
    for (int i = 0; i < 4; ++i) c += static_cast<int8_t>(static_cast<uint32_t>(a) >> (8 * i)) * static_cast<int8_t>(static_cast<uint32_t>(b) >> (8 * i));
    return c;
  }
  static uint32_t udot4(uint32_t a, uint32_t b, uint32_t c) {
    for (int i = 0; i < 4; ++i) c += ((a >> (8 * i)) & 0xff) * ((b >> (8 * i)) & 0xff);
    return c;
  }
  static float exp2(float x) { return static_cast<float>(trans_ref(kExp2, x)); }
  static float log2(float x) { return static_cast<float>(trans_ref(kLog2, x)); }
  static float rcp(float x) { return static_cast<float>(trans_ref(kRcp, x)); }
  static float rsq(float x) { return static_cast<float>(trans_ref(kRsq, x)); }
  static float sqrt(float x) { return static_cast<float>(trans_ref(kSqrt, x)); }
};

// The host referee's values for (seed, rounds): raw[(round * 40 + word) * 64 + lane], the classes'
// words in class order, and digests[class * 64 + lane].  Either may be null.
inline void expected(uint32_t seed, int rounds, uint32_t* raw, uint32_t* digests) {
  for (int lane = 0; lane < 64; ++lane) {
    uint32_t d[kClasses];
    for (int c = 0; c < kClasses; ++c) d[c] = digest_start(c);
    for (int r = 0; r < rounds; ++r) {
      valu_round<HostAlu>(seed, r, lane, [&](int cls, int word, uint32_t bits) {
        if (raw) raw[(static_cast<size_t>(r) * kRoundWords + static_cast<size_t>(word_base(cls) + word)) * 64 + static_cast<size_t>(lane)] = bits;
        d[cls] = mix32(d[cls] ^ bits);
      });
    }
    if (digests) {
      for (int c = 0; c < kClasses; ++c) digests[c * 64 + lane] = d[c];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// the rate phase's chains (gpu_diag.h): start values, and the end digest of a lane

constexpr int kRateClasses = BGC_VALU_RATE_CLASSES;
constexpr int kChains = 8;
constexpr uint32_t kLcgA = 0x5bd1e9, kLcgC = 0x9e3779b9U;  // x = (x mod 2^24) * a + c

// component k (0..15 of the packed fp32 and fp16 chains, chain 2 c + j; 0..7 of fp64) of a lane starts at this integer
BGC_VALU_HD int fma_start(int lane, int k) { return 1 + lane + 64 * k; }
constexpr int kFmaB = 2047;  // x -> b - x; every value is an integer below 2^11, exact in fp16
BGC_VALU_HD uint32_t lcg_start(uint32_t seed, int lane, int chain) { return mix32(seed ^ static_cast<uint32_t>(chain << 8 | lane)); }
BGC_VALU_HD float exp_start(int lane, int chain) { return 0.25f + static_cast<float>(lane + 64 * chain) * (1.0f / 1024); }
constexpr float kExpScale = 0.5f;  // x -> 2^x / 2, which settles at 1 from any start in [0.25, 0.75)

BGC_VALU_HD uint32_t rate_digest_start(int cls) { return 0x85ebca6bU + static_cast<uint32_t>(cls); }

// The end digest of `lane` after `iters` iterations, for the four exact rate classes: every word of chain 0, then of
// chain 1, ... folded as in the check (fp32: both components; fp16: one packed word; fp64: low word, high word).
inline uint32_t rate_expected(int cls, uint32_t seed, int iters, int lane) {
  uint32_t d = rate_digest_start(cls);
  for (int c = 0; c < kChains; ++c) {
    auto end = [&](int k) { return (iters & 1) ? kFmaB - fma_start(lane, k) : fma_start(lane, k); };
    if (cls == BGC_VALU_RATE_FP32) {
      d = mix32(d ^ bits_of(static_cast<float>(end(2 * c))));
      d = mix32(d ^ bits_of(static_cast<float>(end(2 * c + 1))));
    } else if (cls == BGC_VALU_RATE_FP16) {
      d = mix32(d ^ (f16_from_double(end(2 * c)) | f16_from_double(end(2 * c + 1)) << 16));
    } else if (cls == BGC_VALU_RATE_FP64) {
      const uint64_t b = bits_of(static_cast<double>(end(c)));
      d = mix32(mix32(d ^ static_cast<uint32_t>(b)) ^ static_cast<uint32_t>(b >> 32));
    } else {
      uint32_t x = lcg_start(seed, lane, c);
      for (int i = 0; i < iters; ++i) x = HostAlu::mad24(x, kLcgA, kLcgC);
      d = mix32(d ^ x);
    }
  }
  return d;
}

}  // namespace bgc_valu
