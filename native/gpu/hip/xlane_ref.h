// The cross-lane check's operands, its instruction sequence and the host's model of every cross-lane
// instruction (gpu_diag.h, "Cross-lane").  No HIP dependency: xlane.hip includes it for both sides,
// and a plain C++17 program can include it alone to run the host referee, under a sanitizer for
// instance.
//
//  * DPP controls, DPP masks and swizzle offsets are instruction immediates, so the sequence is the
//    compile-time tables below (RowSteps .. ScanSteps, kSwizzle, kRate*): the device instantiates an
//    instruction per entry (xlane.hip) and the host model decodes the same entry (dpp_source(),
//    swizzle_source()).  Where the device has to write an instruction as text (the ALU and EXEC
//    classes), the text repeats the entry and says so.
//  * The host model works on whole waves, uint32_t[64]; every function reads all of its sources
//    before it writes, so a destination may be one of the sources.
//  * Hazards on the host are shifts: every lane number is masked to 0..63 and every 64-bit shift
//    count is below 64.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "gpu_diag.h"

#if defined(__HIPCC__)
#define BGC_XLANE_HD __host__ __device__ __forceinline__
#else
#define BGC_XLANE_HD inline
#endif

namespace bgc_xlane {

constexpr int kClasses = BGC_XLANE_CLASSES;
constexpr int kRoundWords = BGC_XLANE_ROUND_WORDS;
// 32-bit result words of a class per round, and where a class starts among the 47 of a round
BGC_XLANE_HD constexpr int class_words(int cls) {
  constexpr int words[kClasses] = {12, 6, 6, 3, 4, 6, 6, 4};
  return words[cls];
}
BGC_XLANE_HD constexpr int word_base(int cls) {
  int base = 0;
  for (int c = 0; c < cls; ++c) base += class_words(c);
  return base;
}
static_assert(word_base(kClasses) == kRoundWords, "the classes' words fill a round");

BGC_XLANE_HD uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// operand word k of (class, round, lane): the vector ALU check's hash
BGC_XLANE_HD uint32_t operand(uint32_t seed, int cls, int round, int k, int lane) {
  return mix32(seed ^ mix32(static_cast<uint32_t>(cls) << 24 | static_cast<uint32_t>(round) << 16 | static_cast<uint32_t>(k) << 8 |
                            static_cast<uint32_t>(lane)));
}
// wave-uniform word k of (class, round): the hash of a lane no wave has
BGC_XLANE_HD uint32_t uniform(uint32_t seed, int cls, int round, int k) { return operand(seed, cls, round, k, 64); }

BGC_XLANE_HD uint32_t digest_start(int cls) { return 0x9e3779b9U + static_cast<uint32_t>(cls); }

// ---------------------------------------------------------------------------------------------
// the sequence: DPP steps as the instruction encodes them

struct Dpp {
  int ctrl;        // the 9-bit dpp_ctrl field
  int row_mask, bank_mask;
  int bound_ctrl;  // 1: an invalid or disabled source lane gives 0; 0: the lane is not written
};

constexpr int quad_perm(int s0, int s1, int s2, int s3) { return s0 | s1 << 2 | s2 << 4 | s3 << 6; }
constexpr int row_shl(int n) { return 0x100 + n; }  // n 1..15
constexpr int row_shr(int n) { return 0x110 + n; }
constexpr int row_ror(int n) { return 0x120 + n; }
constexpr int kWaveShl1 = 0x130, kWaveRol1 = 0x134, kWaveShr1 = 0x138, kWaveRor1 = 0x13c;
constexpr int kRowMirror = 0x140, kRowHalfMirror = 0x141, kRowBcast15 = 0x142, kRowBcast31 = 0x143;

// BGC_XLANE_ROW: v_mov_b32_dpp, src = w_0, old = w_1
struct RowSteps {
  static constexpr int kCount = 12;
  static constexpr Dpp steps[kCount] = {
      {quad_perm(3, 2, 1, 0), 0xf, 0xf, 0}, {quad_perm(1, 0, 3, 2), 0xf, 0xf, 0}, {quad_perm(2, 2, 0, 0), 0xf, 0xf, 0},
      {row_shl(1), 0xf, 0xf, 0},            {row_shl(7), 0xf, 0xf, 0},            {row_shr(1), 0xf, 0xf, 0},
      {row_shr(12), 0xf, 0xf, 0},           {row_ror(1), 0xf, 0xf, 0},            {row_ror(8), 0xf, 0xf, 0},
      {row_ror(15), 0xf, 0xf, 0},           {kRowMirror, 0xf, 0xf, 0},            {kRowHalfMirror, 0xf, 0xf, 0}};
};
// BGC_XLANE_WAVE: alike
struct WaveSteps {
  static constexpr int kCount = 6;
  static constexpr Dpp steps[kCount] = {{kWaveShl1, 0xf, 0xf, 0}, {kWaveRol1, 0xf, 0xf, 0},   {kWaveShr1, 0xf, 0xf, 0},
                                        {kWaveRor1, 0xf, 0xf, 0}, {kRowBcast15, 0xf, 0xf, 0}, {kRowBcast31, 0xf, 0xf, 0}};
};
// BGC_XLANE_MASK: alike
struct MaskSteps {
  static constexpr int kCount = 6;
  static constexpr Dpp steps[kCount] = {{row_shr(1), 0xf, 0xf, 1}, {kWaveShl1, 0xf, 0xf, 1},   {row_ror(3), 0xa, 0xf, 0},
                                        {row_ror(3), 0xf, 0x5, 0}, {kRowBcast15, 0xa, 0xf, 0}, {row_shr(3), 0x6, 0x9, 1}};
};
// BGC_XLANE_ALU words 0 and 1: v_add_u32_dpp and v_min_u32_dpp, vdst = op(dpp(w_0), w_1); a lane that is not written keeps w_2
constexpr Dpp kAluAdd = {row_shr(1), 0xf, 0xf, 1}, kAluMin = {row_ror(8), 0xf, 0xf, 0};
// word 2, the inclusive prefix sum of w_2: acc = v_add_u32_dpp(dpp(x), x), then twice acc = add(dpp(x), acc), then four
// times acc = add(dpp(acc), acc)
struct ScanSteps {
  static constexpr int kCount = 7;
  static constexpr Dpp steps[kCount] = {{row_shr(1), 0xf, 0xf, 1}, {row_shr(2), 0xf, 0xf, 1},  {row_shr(3), 0xf, 0xf, 1}, {row_shr(4), 0xf, 0xe, 0},
                                        {row_shr(8), 0xf, 0xc, 0}, {kRowBcast15, 0xa, 0xf, 0}, {kRowBcast31, 0xc, 0xf, 0}};
};
// BGC_XLANE_LDS words 3..5: ds_swizzle_b32 offsets.  Bit mode: and | or << 5 | xor << 10; quad mode: 0x8000 | quad_perm
constexpr int kSwizzle[3] = {0x1b | 0x04 << 5 | 0x11 << 10, 0x0f | 0x10 << 5 | 0x0a << 10, 0x8000 | quad_perm(1, 3, 0, 2)};
// BGC_XLANE_EXEC words 0 and 1: v_mov_b32_dpp under the mask M
constexpr Dpp kExecKeep = {kWaveRor1, 0xf, 0xf, 0}, kExecZero = {kWaveRor1, 0xf, 0xf, 1};
// the rate phase's steps: each a permutation of the wave
constexpr Dpp kRateDpp = {row_ror(1), 0xf, 0xf, 0};
constexpr int kRateSwizzle = 0x1f | 0x15 << 10;  // lane ^ 0x15 within each half
constexpr int kRateRotate = 1;                   // ds_bpermute: lane l reads lane (l + 1) mod 64

// ---------------------------------------------------------------------------------------------
// the sequence: addresses, lane selects and the EXEC mask, for both sides

// BGC_XLANE_LDS: byte addresses of lane `lane`
BGC_XLANE_HD uint32_t gather_addr(uint32_t w) { return (w & 63) << 2; }  // any lane, duplicates included
BGC_XLANE_HD uint32_t rotate_addr(uint32_t seed, int round, int lane) {  // by a distance 1..63
  return ((static_cast<uint32_t>(lane) + 1 + uniform(seed, BGC_XLANE_LDS, round, 0) % 63) & 63) << 2;
}
BGC_XLANE_HD uint32_t scatter_addr(uint32_t seed, int round, int lane) {  // a bijection: a odd
  const uint32_t a = uniform(seed, BGC_XLANE_LDS, round, 1) | 1, b = uniform(seed, BGC_XLANE_LDS, round, 2);
  return ((a * static_cast<uint32_t>(lane) + b) & 63) << 2;
}
// BGC_XLANE_LANE
BGC_XLANE_HD int readlane_select(uint32_t seed, int round) { return static_cast<int>(uniform(seed, BGC_XLANE_LANE, round, 0) & 63); }
BGC_XLANE_HD uint32_t writelane_value(uint32_t seed, int round) { return uniform(seed, BGC_XLANE_LANE, round, 1); }
BGC_XLANE_HD int writelane_select(uint32_t seed, int round) { return static_cast<int>(uniform(seed, BGC_XLANE_LANE, round, 2) & 63); }
// BGC_XLANE_EXEC: 64 hashed bits, one forced on and another forced off
BGC_XLANE_HD uint64_t exec_mask(uint32_t seed, int round) {
  const uint64_t m = static_cast<uint64_t>(uniform(seed, BGC_XLANE_EXEC, round, 1)) << 32 | uniform(seed, BGC_XLANE_EXEC, round, 0);
  const uint32_t on = uniform(seed, BGC_XLANE_EXEC, round, 2) & 63, off = (on + 1 + uniform(seed, BGC_XLANE_EXEC, round, 3) % 63) & 63;
  return (m | 1ULL << on) & ~(1ULL << off);
}

// ---------------------------------------------------------------------------------------------
// the host's model (gpu_diag.h states it in words)

constexpr uint64_t kAllLanes = ~0ULL;
inline bool lane_on(uint64_t mask, int lane) { return (mask >> (lane & 63)) & 1; }

// the lane that `lane` reads under dpp_ctrl `ctrl`, or -1 if there is none
inline int dpp_source(int ctrl, int lane) {
  const int row = lane & ~15, i = lane & 15, n = ctrl & 15;
  if (ctrl < 0x100) return (lane & ~3) + ((ctrl >> (2 * (lane & 3))) & 3);
  if (ctrl > 0x100 && ctrl <= 0x10f) return i + n <= 15 ? lane + n : -1;
  if (ctrl > 0x110 && ctrl <= 0x11f) return i - n >= 0 ? lane - n : -1;
  if (ctrl > 0x120 && ctrl <= 0x12f) return row + ((i - n) & 15);
  switch (ctrl) {
    case kWaveShl1: return lane < 63 ? lane + 1 : -1;
    case kWaveRol1: return (lane + 1) & 63;
    case kWaveShr1: return lane > 0 ? lane - 1 : -1;
    case kWaveRor1: return (lane + 63) & 63;
    case kRowMirror: return row + 15 - i;
    case kRowHalfMirror: return (lane & ~7) + 7 - (lane & 7);
    case kRowBcast15: return lane >= 16 ? row - 1 : lane;  // row 0 has no previous row: measured, it reads itself
    case kRowBcast31: return lane >= 32 ? 31 : lane;       // alike rows 0 and 1
    default: return -1;
  }
}

// vdst = op(dpp(src0), src1) of a VOP2 with a DPP first operand, under EXEC `exec`; `out` holds vdst before and after
template <class Op>
void dpp_alu(const Dpp& s, uint64_t exec, const uint32_t* src0, const uint32_t* src1, uint32_t* out, Op&& op) {
  uint32_t r[64];
  for (int l = 0; l < 64; ++l) {
    r[l] = out[l];
    if (!lane_on(exec, l) || !((s.row_mask >> (l / 16)) & 1) || !((s.bank_mask >> ((l % 16) / 4)) & 1)) continue;
    const int from = dpp_source(s.ctrl, l);
    if (from >= 0 && lane_on(exec, from)) {
      r[l] = op(src0[from], src1[l]);
    } else if (s.bound_ctrl) {
      r[l] = op(0u, src1[l]);
    }
  }
  memcpy(out, r, sizeof(r));
}
// v_mov_b32_dpp: `out` holds old before
inline void dpp_mov(const Dpp& s, uint64_t exec, const uint32_t* src, uint32_t* out) {
  dpp_alu(s, exec, src, src, out, [](uint32_t moved, uint32_t) { return moved; });
}

// both results of v_permlane32_swap_b32 (16: v_permlane16_swap_b32) vdst, src, in place
inline void permlane_swap(int width, uint32_t* vdst, uint32_t* src) {
  for (int l = 0; l < 64; ++l) {
    if ((l / width) & 1) {  // the upper halves (16: rows 1 and 3) of vdst with the lower of src
      const uint32_t t = vdst[l];
      vdst[l] = src[l - width];
      src[l - width] = t;
    }
  }
}

inline void ds_bpermute(uint64_t exec, const uint32_t* addr, const uint32_t* src, uint32_t* out) {
  uint32_t r[64];
  for (int l = 0; l < 64; ++l) {
    const int from = static_cast<int>((addr[l] >> 2) & 63);
    r[l] = !lane_on(exec, l) ? out[l] : lane_on(exec, from) ? src[from] : 0u;
  }
  memcpy(out, r, sizeof(r));
}

// a lane that nobody writes to gets 0; of several writers the highest lane stays (the sequence's addresses are a bijection)
inline void ds_permute(const uint32_t* addr, const uint32_t* src, uint32_t* out) {
  uint32_t r[64] = {};
  for (int l = 0; l < 64; ++l) r[(addr[l] >> 2) & 63] = src[l];
  memcpy(out, r, sizeof(r));
}

inline int swizzle_source(int offset, int lane) {
  if (offset & 0x8000) return (lane & ~3) + ((offset >> (2 * (lane & 3))) & 3);
  return (lane & 32) | ((((lane & 31) & (offset & 31)) | ((offset >> 5) & 31)) ^ ((offset >> 10) & 31));
}
inline void ds_swizzle(int offset, const uint32_t* src, uint32_t* out) {
  uint32_t r[64];
  for (int l = 0; l < 64; ++l) r[l] = src[swizzle_source(offset, l)];
  memcpy(out, r, sizeof(r));
}

// the lowest lane set in `exec` (which is never 0 here)
inline int first_lane(uint64_t exec) {
  int l = 0;
  while (l < 63 && !lane_on(exec, l)) ++l;
  return l;
}
// v_mbcnt_lo then v_mbcnt_hi: the set bits of `mask` below `lane`
inline uint32_t mbcnt(uint64_t mask, int lane) {
  uint32_t n = 0;
  for (int l = 0; l < lane; ++l) n += lane_on(mask, l);
  return n;
}

// The 47 words of a round for the whole wave: w[word_base(cls) + word][lane].
inline void host_round(uint32_t seed, int round, uint32_t (*w)[64]) {
  uint32_t op[3][64];
  auto operands = [&](int cls) {
    for (int k = 0; k < 3; ++k) {
      for (int l = 0; l < 64; ++l) op[k][l] = operand(seed, cls, round, k, l);
    }
  };
  auto movs = [&](int cls, const Dpp* steps, int n) {
    operands(cls);
    for (int i = 0; i < n; ++i) {
      uint32_t* out = w[word_base(cls) + i];
      memcpy(out, op[1], sizeof(op[1]));
      dpp_mov(steps[i], kAllLanes, op[0], out);
    }
  };
  movs(BGC_XLANE_ROW, RowSteps::steps, RowSteps::kCount);
  movs(BGC_XLANE_WAVE, WaveSteps::steps, WaveSteps::kCount);
  movs(BGC_XLANE_MASK, MaskSteps::steps, MaskSteps::kCount);
  {
    operands(BGC_XLANE_ALU);
    uint32_t(*out)[64] = w + word_base(BGC_XLANE_ALU);
    memcpy(out[0], op[2], sizeof(op[2]));
    dpp_alu(kAluAdd, kAllLanes, op[0], op[1], out[0], [](uint32_t a, uint32_t b) { return a + b; });
    memcpy(out[1], op[2], sizeof(op[2]));
    dpp_alu(kAluMin, kAllLanes, op[0], op[1], out[1], [](uint32_t a, uint32_t b) { return a < b ? a : b; });
    auto add = [](uint32_t a, uint32_t b) { return a + b; };
    uint32_t* acc = out[2];
    memset(acc, 0, sizeof(op[2]));
    dpp_alu(ScanSteps::steps[0], kAllLanes, op[2], op[2], acc, add);
    for (int i = 1; i < 3; ++i) dpp_alu(ScanSteps::steps[i], kAllLanes, op[2], acc, acc, add);
    for (int i = 3; i < ScanSteps::kCount; ++i) dpp_alu(ScanSteps::steps[i], kAllLanes, acc, acc, acc, add);
  }
  {
    operands(BGC_XLANE_SWAP);
    uint32_t(*out)[64] = w + word_base(BGC_XLANE_SWAP);
    for (int i = 0; i < 2; ++i) {
      memcpy(out[2 * i], op[0], sizeof(op[0]));
      memcpy(out[2 * i + 1], op[1], sizeof(op[1]));
      permlane_swap(i == 0 ? 16 : 32, out[2 * i], out[2 * i + 1]);
    }
  }
  {
    operands(BGC_XLANE_LDS);
    uint32_t(*out)[64] = w + word_base(BGC_XLANE_LDS);
    uint32_t addr[64];
    for (int l = 0; l < 64; ++l) addr[l] = gather_addr(op[1][l]);
    ds_bpermute(kAllLanes, addr, op[0], out[0]);
    for (int l = 0; l < 64; ++l) addr[l] = rotate_addr(seed, round, l);
    ds_bpermute(kAllLanes, addr, op[0], out[1]);
    for (int l = 0; l < 64; ++l) addr[l] = scatter_addr(seed, round, l);
    ds_permute(addr, op[0], out[2]);
    for (int i = 0; i < 3; ++i) ds_swizzle(kSwizzle[i], op[0], out[3 + i]);
  }
  {
    operands(BGC_XLANE_LANE);
    uint32_t(*out)[64] = w + word_base(BGC_XLANE_LANE);
    uint64_t ballot = 0;
    for (int l = 0; l < 64; ++l) ballot |= static_cast<uint64_t>(op[0][l] & 1) << l;
    for (int l = 0; l < 64; ++l) {
      out[0][l] = op[0][readlane_select(seed, round)];
      out[1][l] = op[1][first_lane(kAllLanes)];
      out[2][l] = l == writelane_select(seed, round) ? writelane_value(seed, round) : op[2][l];
      out[3][l] = static_cast<uint32_t>(ballot);
      out[4][l] = static_cast<uint32_t>(ballot >> 32);
      out[5][l] = mbcnt(ballot, l);
    }
  }
  {
    operands(BGC_XLANE_EXEC);
    uint32_t(*out)[64] = w + word_base(BGC_XLANE_EXEC);
    const uint64_t m = exec_mask(seed, round);
    for (int i = 0; i < 3; ++i) memcpy(out[i], op[1], sizeof(op[1]));
    dpp_mov(kExecKeep, m, op[0], out[0]);
    dpp_mov(kExecZero, m, op[0], out[1]);
    uint32_t addr[64];
    for (int l = 0; l < 64; ++l) addr[l] = gather_addr(op[2][l]);
    ds_bpermute(m, addr, op[0], out[2]);
    for (int l = 0; l < 64; ++l) out[3][l] = op[0][first_lane(m)];  // a scalar: every lane gets it once EXEC is restored
  }
}

// The host referee's values for (seed, rounds): raw[(round * 47 + word) * 64 + lane], the classes'
// words in class order, and digests[class * 64 + lane].  Either may be null.
inline void expected(uint32_t seed, int rounds, uint32_t* raw, uint32_t* digests) {
  uint32_t d[kClasses][64];
  for (int c = 0; c < kClasses; ++c) {
    for (int l = 0; l < 64; ++l) d[c][l] = digest_start(c);
  }
  for (int r = 0; r < rounds; ++r) {
    uint32_t w[kRoundWords][64];
    host_round(seed, r, w);
    if (raw) memcpy(raw + static_cast<size_t>(r) * kRoundWords * 64, w, sizeof(w));
    for (int c = 0; c < kClasses; ++c) {
      for (int i = 0; i < class_words(c); ++i) {
        for (int l = 0; l < 64; ++l) d[c][l] = mix32(d[c][l] ^ w[word_base(c) + i][l]);
      }
    }
  }
  if (digests) memcpy(digests, d, sizeof(d));
}

// ---------------------------------------------------------------------------------------------
// the rate phase (gpu_diag.h): 8 chains per lane, every step a permutation of the chains' 8 * 64 values

constexpr int kRateClasses = BGC_XLANE_RATE_CLASSES;
constexpr int kChains = 8;
constexpr int kSlots = kChains * 64;  // slot = chain * 64 + lane

BGC_XLANE_HD uint32_t rate_fill(uint32_t seed, int lane, int chain) {
  return mix32(seed ^ (0x10000u | static_cast<uint32_t>(chain) << 8 | static_cast<uint32_t>(lane)));
}
BGC_XLANE_HD uint32_t rate_digest_start(int cls) { return 0x85ebca6bU + static_cast<uint32_t>(cls); }
BGC_XLANE_HD uint32_t rate_rotate_addr(int lane) { return ((static_cast<uint32_t>(lane) + kRateRotate) & 63) << 2; }

// the slot whose value one step of rate class `cls` moves to `slot`
inline int rate_source(int cls, int slot) {
  const int chain = slot / 64, lane = slot % 64;
  switch (cls) {
    case BGC_XLANE_RATE_DPP: return chain * 64 + dpp_source(kRateDpp.ctrl, lane);
    case BGC_XLANE_RATE_SWAP:  // v_permlane32_swap_b32 chain 2 j, chain 2 j + 1
      if (!(chain & 1)) return lane < 32 ? slot : (chain + 1) * 64 + lane - 32;
      return lane < 32 ? (chain - 1) * 64 + lane + 32 : slot;
    case BGC_XLANE_RATE_BPERMUTE: return chain * 64 + static_cast<int>(rate_rotate_addr(lane) >> 2);
    default: return chain * 64 + swizzle_source(kRateSwizzle, lane);
  }
}

// The end digest of every lane after `iters` steps, ends[lane]: the step's source map raised to the power `iters` by
// squaring, applied to the fill; chain 0's word, then chain 1's, ... folded as in the check.
inline void rate_expected(int cls, uint32_t seed, int iters, uint32_t* ends) {
  int power[kSlots], square[kSlots], next[kSlots];
  for (int s = 0; s < kSlots; ++s) {
    power[s] = s;
    square[s] = rate_source(cls, s);
  }
  for (int n = iters; n > 0; n >>= 1) {
    if (n & 1) {
      for (int s = 0; s < kSlots; ++s) next[s] = power[square[s]];
      memcpy(power, next, sizeof(power));
    }
    for (int s = 0; s < kSlots; ++s) next[s] = square[square[s]];
    memcpy(square, next, sizeof(square));
  }
  for (int l = 0; l < 64; ++l) {
    uint32_t d = rate_digest_start(cls);
    for (int c = 0; c < kChains; ++c) {
      const int from = power[c * 64 + l];
      d = mix32(d ^ rate_fill(seed, from % 64, from / 64));
    }
    ends[l] = d;
  }
}

}  // namespace bgc_xlane
