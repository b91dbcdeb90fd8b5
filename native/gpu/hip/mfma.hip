// Matrix cores: the per-CU bf16 MFMA check and throughput (bgc_diag_mfma), the MX fp8/fp4
// block-scaled check and throughput (bgc_diag_mfma_lowp), the fp16 / int8 / fp32 / fp64 checks and
// throughputs (bgc_diag_mfma_classic), the burn-in loop that runs the throughput kernels back to
// back (bgc_diag_burn_dtype), and the one-wave-per-tile GEMMs on caller operands (bgc_diag_gemm,
// bgc_diag_mx_gemm, bgc_diag_gemm_dtype).
//
//  * A tile trait (DenseTile<path, wide>, MxTile<fmt>) says what differs between the matrix-core
//    paths: how a lane's operands are packed, the MFMA, its accumulator type, the row an
//    accumulator element holds, and the exact value of one output element.  One check kernel
//    (mfma_check) and one throughput kernel (mfma_throughput) are instantiated over them.
//  * The dense paths (Bf16Path and the classic F16Path, I8Path, F32Path, F64Path) share one tile
//    layout and one GEMM kernel (dense_gemm).  The classic ones check with operands as wide as their
//    multipliers instead of {-1,0,1}, chosen so that every partial sum stays an exact integer
//    (gpu_diag.h); their throughput phase keeps {-1,0,1}.
//  * The check runs one MFMA tile per wave per round with operands in {-1,0,1} (and, for MX,
//    block scales in {1/2,1,2}) generated from a hash in registers (no memory traffic), so
//    every product sum is an exact fp32 value and is checked element-wise against a
//    VALU recomputation.  Each wave records its physical CU (HW_REG_XCC_ID + HW_ID),
//    so a faulty matrix core is attributed to (XCC, SE, SH, CU).
//  * The throughput phase chains 4 independent accumulators per wave (dependent MFMA
//    latency hidden by 8 waves/SIMD) and verifies acc == iters * tile exactly.
//  * On the host, bgc_diag_mfma, bgc_diag_mfma_lowp and bgc_diag_mfma_classic are each a MatrixRun:
//    the argument checks, the test plants (HostPlants), the per-CU bins (CuBins), the check launches
//    and the warm-up / zero / timed rate launches in one place.  Each run says its limits, lists its
//    launches and fills its own result struct.  with_plants picks between a kernel's production and
//    planted instantiation.
//  * bgc_diag_mfma_tile runs one round of the check in one wave (mfma_tile) and returns what every
//    lane held, for the tests of the generated tiles.
//  * bgc_diag_mfma_delayed and bgc_diag_burn_delayed make chosen waves of a throughput launch wait on
//    the constant clock (delay()), for the tests of the rates and times.
//  * bgc_diag_burn_planted applies value plants in chosen launches of the burn, for the tests of its
//    mismatch count.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include "diag_common.h"

namespace {

using namespace bgc_diag;

// Element (r, c) of operand `which` of a tile, in {-1, 0, 1}.  Every tile trait indexes with
// c < kOperandStride (it asserts kK <= kOperandStride), so no two (r, c) of a tile share a hash.
constexpr int kOperandStride = 128;

__device__ __forceinline__ uint32_t operand_hash(uint32_t seed, uint32_t tile, int r, int c, uint32_t which) {
  return mix32(seed ^ mix32(tile * 0x9e3779b9U + which) ^ static_cast<uint32_t>(r * kOperandStride + c));
}

__device__ __forceinline__ int operand(uint32_t seed, uint32_t tile, int r, int c, uint32_t which) {
  return static_cast<int>(operand_hash(seed, tile, r, c, which) % 3u) - 1;
}

// ---------------------------------------------------------------------------
// Tile traits: a 16x16xkK MFMA on hash-derived operands.  Lane l holds its part of A row
// (l & 15) and of B column (l & 15) from lane group l >> 4; the result lane l holds column
// (l & 15) and, in element i of its accumulator (Acc, of Scalar), row row(l >> 4, i): 4 g + i, the
// C/D map of every 16x16 MFMA but the fp64 one.  Lane is mfma_tile's per-lane record.
// mfma() takes the lane's two scale exponents, scale_exp() of its (row or column, lane group), and
// expect() is the exact value of output element (row, col); a tile without block scales
// ignores `scaled`.

// Low-precision (MX block-scaled) matrix cores: v_mfma_scale_f32_16x16x128_f8f6f4.
// Lane l holds 32 K-elements of A row (l & 15) and of B column (l & 15) from lane group
// g = l >> 4, plus one E8M0 scale byte for (its row or column, block g) of the 4 K-blocks
// of 32.  A and B are laid out alike, so A element (g, j) always meets B element (g, j);
// which block, hence which scale, an element belongs to is lowp_block().  The exact
// result is sum_blk 2^(sa(r, blk) + sb(c, blk)) * sum_{(g, j) in blk} a(r, g, j) b(c, g, j).
// Operands in {-1, 0, 1} and scales in {1/2, 1, 2} keep every product and sum exact.
// kFmt: 0 = fp8 e4m3 (OCP), 4 = fp4 e2m1 (two per byte; 16 of the 32 operand bytes).
template <int kFmt>
__device__ __forceinline__ uint32_t lowp_code(int v) {
  if (kFmt == 0) return v > 0 ? 0x38u : (v < 0 ? 0xB8u : 0u);  // e4m3: +-1.0 = 0 0111 000
  return v > 0 ? 0x2u : (v < 0 ? 0xAu : 0u);                  // e2m1: +-1.0 = 0 01 0
}

// The scale block (= the lane group whose scale byte applies) of element j of lane group g,
// measured on the MI355X with tools/probes/mx_scale_layout.hip (profiles/mx_lowp_r3/):
//  * fp4: a lane group's 32 elements are K 32g..32g+31, one block, its own scale;
//  * fp8: elements 0-15 are K 16g..16g+15 and 16-31 are K 64+16g.., so they fall in
//    blocks g/2 and 2+g/2, scaled by lane groups g/2 and 2+g/2.
template <int kFmt>
__device__ __forceinline__ int lowp_block(int g, int j) {
  return kFmt == 0 ? (g >> 1) + 2 * (j >> 4) : g;
}

// scale exponent in {-1, 0, 1} for (row or column, block); 0 when unscaled
__device__ __forceinline__ int lowp_exp(uint32_t seed, uint32_t tile, int rc, int g, uint32_t which, bool scaled) {
  return scaled ? operand(seed ^ 0x5ca1e, tile, rc, g, which) : 0;
}

// the MX tile: both operands are indexed (row or column, k)
template <int kFmt>
struct MxTile {
  using Frag = i32x8;
  using Acc = f32x4;
  using Scalar = float;
  using Lane = bgc_tile_lane;
  static constexpr int kK = 128;
  static __device__ __forceinline__ int row(int g, int i) { return 4 * g + i; }
  static_assert(kK <= kOperandStride, "operand() must tell every (row or column, k) apart");
  // 32 operands of one lane (row or column `rc`, block `g`) packed for the MFMA
  static __device__ __forceinline__ Frag pack(uint32_t seed, uint32_t tile, int rc, int g, uint32_t which) {
    i32x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const uint32_t c = lowp_code<kFmt>(operand(seed, tile, rc, 32 * g + j, which));
      if (kFmt == 0) {
        v[j >> 2] |= static_cast<int>(c << (8 * (j & 3)));
      } else {
        v[j >> 3] |= static_cast<int>(c << (4 * (j & 7)));
      }
    }
    return v;
  }
  static __device__ __forceinline__ f32x4 mfma(Frag a, Frag b, f32x4 acc, int sa, int sb) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, kFmt, kFmt, 0, 127 + sa, 0, 127 + sb);
  }
  static __device__ __forceinline__ int b_operand(uint32_t seed, uint32_t tile, int k, int col) {
    return operand(seed, tile, col, k, 0xB);
  }
  static __device__ __forceinline__ int scale_exp(uint32_t seed, uint32_t tile, int rc, int g, uint32_t which, bool scaled) {
    return lowp_exp(seed, tile, rc, g, which, scaled);
  }
  static __device__ __forceinline__ float expect(uint32_t seed, uint32_t tile, int row, int col, bool scaled) {
    int dot[4] = {0, 0, 0, 0};  // per scale block
    for (int g = 0; g < 4; ++g) {
      for (int j = 0; j < 32; ++j) {
        dot[lowp_block<kFmt>(g, j)] += operand(seed, tile, row, 32 * g + j, 0xA) * b_operand(seed, tile, 32 * g + j, col);
      }
    }
    float e = 0.f;
    for (int blk = 0; blk < 4; ++blk) {
      e += ldexpf(static_cast<float>(dot[blk]), scale_exp(seed, tile, row, blk, 0xA, scaled) + scale_exp(seed, tile, col, blk, 0xB, scaled));
    }
    return e;
  }
};

// The dense matrix-core paths: bf16 (K 32) and the classic fp16 (K 32), int8 (K 64), fp32 and fp64
// (K 4).  A path says what its MFMA takes and returns and names mfma_tile's lane record; DenseTile
// below makes a tile trait of it.  Lane group g holds k = kPerLane g + j in element j of its
// fragment, of A row rc and of B column rc (the one-hot probes of tests/gpu/test_diag_classic.py
// read this layout and the row maps back through dense_gemm).  A classic path's wide() maps a hash
// to a check-phase operand as wide as the multipliers; the bounds that keep every partial sum an
// exact integer are proved in gpu_diag.h.  bf16 has no wide check.
struct Bf16Path {
  using Elem = __bf16;
  using Frag = bf16x8;
  using Acc = f32x4;
  using Sum = int;
  using Lane = bgc_tile_lane;
  static constexpr int kK = 32, kPerLane = 8;
  static __device__ __forceinline__ int row(int g, int i) { return 4 * g + i; }
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
struct F16Path {
  using Elem = _Float16;
  using Frag = f16x8;
  using Acc = f32x4;
  using Sum = int;
  using Lane = bgc_classic_tile_lane;
  static constexpr int kK = 32, kPerLane = 8;
  static __device__ __forceinline__ int wide(uint32_t h) { return static_cast<int>(h % 1025u) - 512; }
  static __device__ __forceinline__ int row(int g, int i) { return 4 * g + i; }
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
struct I8Path {
  using Elem = int8_t;
  using Frag = i8x16;
  using Acc = i32x4;
  using Sum = int;
  using Lane = bgc_classic_tile_lane;
  static constexpr int kK = 64, kPerLane = 16;
  static __device__ __forceinline__ int wide(uint32_t h) { return static_cast<int8_t>(h & 0xffu); }
  static __device__ __forceinline__ int row(int g, int i) { return 4 * g + i; }
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b), c, 0, 0, 0);
  }
};
struct F32Path {
  using Elem = float;
  using Frag = f32x1;
  using Acc = f32x4;
  using Sum = int;
  using Lane = bgc_classic_tile_lane;
  static constexpr int kK = 4, kPerLane = 1;
  static __device__ __forceinline__ int wide(uint32_t h) { return static_cast<int>(h % 4095u) - 2047; }
  static __device__ __forceinline__ int row(int g, int i) { return 4 * g + i; }
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], c, 0, 0, 0); }
};
// v_mfma_f64_16x16x4_f64 has a C/D map of its own: accumulator element i holds row g + 4 i.
struct F64Path {
  using Elem = double;
  using Frag = f64x1;
  using Acc = f64x4;
  using Sum = long long;
  using Lane = bgc_classic_tile_lane;
  static constexpr int kK = 4, kPerLane = 1;
  static __device__ __forceinline__ int wide(uint32_t h) { return static_cast<int>(h >> 6) - (1 << 25); }
  static __device__ __forceinline__ int row(int g, int i) { return g + 4 * i; }
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[0], c, 0, 0, 0); }
};

// The tile of a dense path: A[row][k] = value(row, k, 0xA) and B[k][col] = value(k, col, 0xB), where
// value is wide() of the operand hash in a classic path's check (kWide) and operand(), in {-1, 0, 1},
// in the bf16 check and in every throughput phase.
template <class Path, bool kWide>
struct DenseTile {
  using Frag = typename Path::Frag;
  using Acc = typename Path::Acc;
  using Scalar = std::remove_reference_t<decltype(Acc{}[0])>;
  using Lane = typename Path::Lane;
  static constexpr int kK = Path::kK;
  static_assert(kK <= kOperandStride, "operand() must tell every (row, k) and (k, column) apart");
  static __device__ __forceinline__ int row(int g, int i) { return Path::row(g, i); }
  static __device__ __forceinline__ int value(uint32_t seed, uint32_t tile, int r, int c, uint32_t which) {
    if constexpr (kWide) {
      return Path::wide(operand_hash(seed, tile, r, c, which));
    } else {
      return operand(seed, tile, r, c, which);
    }
  }
  static __device__ __forceinline__ Frag pack(uint32_t seed, uint32_t tile, int rc, int g, uint32_t which) {
    Frag v;
#pragma unroll
    for (int j = 0; j < Path::kPerLane; ++j) {
      const int k = Path::kPerLane * g + j;
      v[j] = static_cast<typename Path::Elem>(which == 0xA ? value(seed, tile, rc, k, 0xA) : value(seed, tile, k, rc, 0xB));
    }
    return v;
  }
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc acc, int /*sa*/, int /*sb*/) { return Path::mfma(a, b, acc); }
  static __device__ __forceinline__ int scale_exp(uint32_t, uint32_t, int, int, uint32_t, bool) { return 0; }
  // the dot product in integer VALU arithmetic, converted once
  static __device__ __forceinline__ Scalar expect(uint32_t seed, uint32_t tile, int row, int col, bool /*scaled*/) {
    typename Path::Sum dot = 0;
    for (int k = 0; k < kK; ++k) {
      dot += static_cast<typename Path::Sum>(value(seed, tile, row, k, 0xA)) * value(seed, tile, k, col, 0xB);
    }
    return static_cast<Scalar>(dot);
  }
};

using Bf16Tile = DenseTile<Bf16Path, false>;

// Test plants (gpu_diag.h, "planted variants").  The check and throughput kernels end in a pack
// `Plants... plants`: empty in the production instantiations, which so take no further argument and
// call the empty plant() and delay() overloads (they compile to what they would be without), and one
// plant list in the instantiations behind the *_planted entry points (wrong values) and the *_delayed
// ones (DelayPlants: waits on the constant clock).  Everything else, the comparison, the
// wave reduction and the report, is the same source for both; with_plants() below picks between them.
using CheckPlants = PlantList<bgc_mfma_check_plant>;
using RatePlants = PlantList<bgc_mfma_rate_plant>;
using DelayPlants = PlantList<bgc_mfma_delay_plant>;

// acc[i] += delta in the accumulator's type (an int8-path delta is an integer below 2^31, checked on the host)
template <class Acc>
__device__ __forceinline__ void add_at(Acc& acc, int i, float delta) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e == i) acc[e] += static_cast<std::remove_reference_t<decltype(Acc{}[0])>>(delta);
  }
}

// check phase: before round `round`'s comparison
template <class Acc>
__device__ __forceinline__ void plant(Acc&, uint32_t /*wave*/, int /*round*/, int /*lane*/) {}
template <class Acc>
__device__ __forceinline__ void plant(Acc& acc, uint32_t wave, int round, int lane, CheckPlants pl) {
  for (int j = 0; j < pl.n; ++j) {
    const bgc_mfma_check_plant p = pl.p[j];
    if ((p.wave == BGC_PLANT_ALL_WAVES || static_cast<uint32_t>(p.wave) == wave) && p.round == round && p.lane == lane) {
      add_at(acc, p.i, p.delta);
    }
  }
}

// throughput phase: after the loop, before the comparison
template <class Acc>
__device__ __forceinline__ void plant(Acc (&)[4], uint32_t /*wave*/, int /*lane*/) {}
template <class Acc>
__device__ __forceinline__ void plant(Acc (&acc)[4], uint32_t wave, int lane, RatePlants pl) {
  for (int j = 0; j < pl.n; ++j) {
    const bgc_mfma_rate_plant p = pl.p[j];
    if (static_cast<uint32_t>(p.wave) != wave || p.lane != lane) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c == p.chain) add_at(acc[c], p.i, p.delta);
    }
  }
}
template <class Acc>
__device__ __forceinline__ void plant(Acc (&)[4], uint32_t /*wave*/, int /*lane*/, DelayPlants) {}  // no values

// throughput phase, at the same point: the wave waits for the largest `ticks` of the delay plants
// that name it, counted on the constant clock from here (wait_ticks: it ends after `ticks`, at most
// BGC_DIAG_MAX_DELAY_TICKS, checked on the host).
__device__ __forceinline__ void delay(uint32_t /*wave*/) {}
__device__ __forceinline__ void delay(uint32_t /*wave*/, RatePlants) {}
__device__ __forceinline__ void delay(uint32_t wave, DelayPlants pl) {
  uint32_t ticks = 0;
  for (int j = 0; j < pl.n; ++j) {
    const bgc_mfma_delay_plant p = pl.p[j];
    if (p.wave == BGC_PLANT_ALL_WAVES || static_cast<uint32_t>(p.wave) == wave) ticks = max(ticks, p.ticks);
  }
  wait_ticks(__builtin_amdgcn_readfirstlane(ticks));  // the same in every lane of the wave
}

// ---------------------------------------------------------------------------
// Check: wave w checks tiles w * rounds .. w * rounds + rounds - 1 element-wise, with the tile's
// block scales if `scaled`, and bins the outcome by the CU it runs on.
template <class Tile, class... Plants>
__global__ __launch_bounds__(kBlock) void mfma_check(uint32_t seed, int rounds, int scaled, unsigned* __restrict__ cu_tiles,
                                                     unsigned* __restrict__ cu_bad, Plants... plants) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * (kBlock / 64)) + (threadIdx.x >> 6), key = cu_key();
  const int rc = lane & 15, g = lane >> 4;
  unsigned bad = 0;
  for (int r = 0; r < rounds; ++r) {
    const uint32_t tile = wave * static_cast<uint32_t>(rounds) + static_cast<uint32_t>(r);
    const typename Tile::Frag a = Tile::pack(seed, tile, rc, g, 0xA);
    const typename Tile::Frag b = Tile::pack(seed, tile, rc, g, 0xB);
    typename Tile::Acc acc = Tile::mfma(a, b, typename Tile::Acc{}, Tile::scale_exp(seed, tile, rc, g, 0xA, scaled),
                                        Tile::scale_exp(seed, tile, rc, g, 0xB, scaled));
    plant(acc, wave, r, lane, plants...);
#pragma unroll
    for (int i = 0; i < 4; ++i) bad += (acc[i] != Tile::expect(seed, tile, Tile::row(g, i), rc, scaled));
  }
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);  // the wave's sum, in lane 0
  if (lane == 0) {  // one atomic per wave
    atomicAdd(&cu_tiles[key], static_cast<unsigned>(rounds));
    if (bad) atomicAdd(&cu_bad[key], bad);
  }
}

// One round of the check by one wave, for bgc_diag_mfma_tile: every lane writes out what the check
// holds in registers (its fragments, scale exponents, accumulators and expected values).
template <class Tile>
__global__ __launch_bounds__(64) void mfma_tile(uint32_t seed, uint32_t tile, int scaled, typename Tile::Lane* __restrict__ lanes) {
  const int lane = threadIdx.x, rc = lane & 15, g = lane >> 4;
  const typename Tile::Frag a = Tile::pack(seed, tile, rc, g, 0xA);
  const typename Tile::Frag b = Tile::pack(seed, tile, rc, g, 0xB);
  typename Tile::Lane o = {};
  static_assert(sizeof(a) <= sizeof(o.a), "a fragment fits the lane record");
  __builtin_memcpy(o.a, &a, sizeof(a));
  __builtin_memcpy(o.b, &b, sizeof(b));
  const int ea = Tile::scale_exp(seed, tile, rc, g, 0xA, scaled), eb = Tile::scale_exp(seed, tile, rc, g, 0xB, scaled);
  if constexpr (std::is_same_v<typename Tile::Lane, bgc_tile_lane>) {
    o.ea = ea;
    o.eb = eb;
  }
  const typename Tile::Acc acc = Tile::mfma(a, b, typename Tile::Acc{}, ea, eb);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o.acc[i] = acc[i];
    o.expect[i] = Tile::expect(seed, tile, Tile::row(g, i), rc, scaled);
  }
  lanes[lane] = o;
}

// ---------------------------------------------------------------------------
// Throughput: 4 independent accumulator chains per wave, acc == iters * tile + c in the tile's Scalar.  With kTimed
// each wave also times itself on the 100 MHz constant clock and adds its duration to its XCC's
// bin, so a slow (throttled / degraded) XCC shows up as an imbalance even when the whole-chip
// rate still clears its floor.
template <class Tile, bool kTimed, class... Plants>
__global__ __launch_bounds__(kBlock) void mfma_throughput(uint32_t seed, int iters, unsigned* __restrict__ fails,
                                                          unsigned long long* __restrict__ xcc_ticks,
                                                          unsigned* __restrict__ xcc_waves, Plants... plants) {
  uint64_t t_start = 0;
  if constexpr (kTimed) t_start = wall_clock64();
  const int lane = threadIdx.x & 63;
  const uint32_t tile = (blockIdx.x * (kBlock / 64)) + (threadIdx.x >> 6);
  const int rc = lane & 15, g = lane >> 4;
  const typename Tile::Frag a = Tile::pack(seed, tile, rc, g, 0xA);
  const typename Tile::Frag b = Tile::pack(seed, tile, rc, g, 0xB);
  // Distinct initial values keep the compiler from merging the four chains.
  using Scalar = typename Tile::Scalar;
  typename Tile::Acc acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = typename Tile::Acc{Scalar(c), Scalar(c), Scalar(c), Scalar(c)};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = Tile::mfma(a, b, acc[c], 0, 0);
  }
  plant(acc, tile, lane, plants...);
  delay(tile, plants...);
  unsigned bad = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const Scalar e = Tile::expect(seed, tile, Tile::row(g, i), rc, false) * static_cast<Scalar>(iters);
#pragma unroll
    for (int c = 0; c < 4; ++c) bad += (acc[c][i] != e + Scalar(c));
  }
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);  // the wave's sum, in lane 0
  if constexpr (kTimed) {
    const uint64_t t_end = wall_clock64();  // after the accumulators were consumed above
    if (lane == 0) {
      if (bad) atomicAdd(fails, bad);
      const uint32_t xcc = (cu_key() >> 8) & 7;
      atomicAdd(&xcc_ticks[xcc], static_cast<unsigned long long>(t_end - t_start));
      atomicAdd(&xcc_waves[xcc], 1u);
    }
  } else {
    if (lane == 0 && bad) atomicAdd(fails, bad);
  }
}

// MX GEMM on caller operands, for the host cross-check of the block-scaled path against an
// independent decode (PyTorch): C[m, n] = sum_k a(m, k) 2^(sa(m, k/32) - 127) *
// b(n, k) 2^(sb(n, k/32) - 127).  A is M x K codes (fp8: one byte each; fp4: two per byte,
// element 2i in the low nibble), Bt is N x K alike, the E8M0 scales are M x K/32 and
// N x K/32 bytes.  One wave per 16x16 output tile, K consumed 128 at a time; each lane loads
// its operands straight from memory in the MFMA's own layout (lowp_block above): fp8 lane
// group g holds K 16g..16g+15 then 64+16g..64+16g+15, fp4 lane group g holds K 32g..32g+31.
template <int kFmt>
__device__ __forceinline__ i32x8 lowp_load(const uint8_t* __restrict__ X, int row, int K, int k0, int g) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  i32x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (kFmt == 0) {
    const uint8_t* p = X + static_cast<size_t>(row) * K + k0 + 16 * g;
    const i32x4 lo = *reinterpret_cast<const i32x4*>(p);
    const i32x4 hi = *reinterpret_cast<const i32x4*>(p + 64);
    v = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  } else {
    const i32x4 q = *reinterpret_cast<const i32x4*>(X + static_cast<size_t>(row) * (K / 2) + (k0 + 32 * g) / 2);
    v = i32x8{q[0], q[1], q[2], q[3], 0, 0, 0, 0};
  }
  return v;
}

template <int kFmt>
__global__ __launch_bounds__(64) void mx_gemm(const uint8_t* __restrict__ A, const uint8_t* __restrict__ sA,
                                              const uint8_t* __restrict__ Bt, const uint8_t* __restrict__ sB,
                                              float* __restrict__ C, int M, int N, int K) {
  const int lane = threadIdx.x, rc = lane & 15, g = lane >> 4;
  const int tiles_n = N / 16;
  const int m0 = (static_cast<int>(blockIdx.x) / tiles_n) * 16, n0 = (static_cast<int>(blockIdx.x) % tiles_n) * 16;
  const int kb = K / 32;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 128) {
    const i32x8 a = lowp_load<kFmt>(A, m0 + rc, K, k0, g);
    const i32x8 b = lowp_load<kFmt>(Bt, n0 + rc, K, k0, g);
    const int sa = sA[static_cast<size_t>(m0 + rc) * kb + k0 / 32 + g];  // this lane's (row, block g) scale
    const int sb = sB[static_cast<size_t>(n0 + rc) * kb + k0 / 32 + g];
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, kFmt, kFmt, 0, sa, 0, sb);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) C[static_cast<size_t>(m0 + 4 * g + i) * N + n0 + rc] = acc[i];
}

// Plain MFMA GEMM on a dense path for the host cross-check: C[M,N] = A[M,K] * B[K,N] in the path's
// element type, row-major; C is fp32 for bf16 and double, which holds every classic path's results
// exactly, for those.  One wave per 16x16 output tile (grid N/16 x M/16), K consumed Path::kK at a
// time with the same operand layout as the tests above: lane l loads A row (l & 15) / B column
// (l & 15) at k = kPerLane (l >> 4) + j straight from memory and writes rows Path::row(l >> 4, i).
template <class Path, class CElem>
__global__ __launch_bounds__(64) void dense_gemm(const typename Path::Elem* __restrict__ A, const typename Path::Elem* __restrict__ B,
                                                 CElem* __restrict__ C, int /*M*/, int N, int K) {
  const int lane = threadIdx.x;
  const int tm = blockIdx.y * 16, tn = blockIdx.x * 16;
  const int rc = lane & 15, g = lane >> 4, kb = Path::kPerLane * g;
  typename Path::Acc acc = {};
  for (int k0 = 0; k0 < K; k0 += Path::kK) {
    typename Path::Frag a, b;
#pragma unroll
    for (int j = 0; j < Path::kPerLane; ++j) {
      a[j] = A[static_cast<size_t>(tm + rc) * K + k0 + kb + j];
      b[j] = B[static_cast<size_t>(k0 + kb + j) * N + tn + rc];
    }
    acc = Path::mfma(a, b, acc);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) C[static_cast<size_t>(tm + Path::row(g, i)) * N + tn + rc] = static_cast<CElem>(acc[i]);
}

// `f(Path{})` for classic path 0..3 (BGC_CLASSIC_*)
template <class F>
auto with_classic_path(int path, F&& f) {
  switch (path) {
    case BGC_CLASSIC_FP16: return f(F16Path{});
    case BGC_CLASSIC_INT8: return f(I8Path{});
    case BGC_CLASSIC_FP32: return f(F32Path{});
    default: return f(F64Path{});
  }
}

// `f(std::integral_constant<int, kFmt>)` for MX format 0 (fp8 e4m3) or 4 (fp4 e2m1)
template <class F>
auto with_mx_fmt(int fmt, F&& f) {
  if (fmt == 0) return f(std::integral_constant<int, 0>{});
  return f(std::integral_constant<int, 4>{});
}

// `f(Tile{}, kTimed)` for a burn dtype (BGC_BURN_*): the bf16 rate kernel times its waves per XCC,
// the MX ones do not
template <class F>
auto with_burn_dtype(int dtype, F&& f) {
  switch (dtype) {
    case BGC_BURN_BF16: return f(Bf16Tile{}, std::true_type{});
    case BGC_BURN_FP8: return f(MxTile<0>{}, std::false_type{});
    default: return f(MxTile<4>{}, std::false_type{});
  }
}

// `launch(plants...)`: of the production instantiation, or with test plants of the planted one
template <class P, class Launch>
void with_plants(PlantList<P> plants, Launch&& launch) {
  if (plants.n == 0) {
    launch();
  } else {
    launch(plants);
  }
}

template <class Tile>
void launch_check(int blocks, uint32_t seed, int rounds, int scaled, unsigned* cu_tiles, unsigned* cu_bad, CheckPlants plants) {
  with_plants(plants, [&](auto... pl) {
    hipLaunchKernelGGL((mfma_check<Tile, decltype(pl)...>), dim3(blocks), dim3(kBlock), 0, nullptr, seed, rounds, scaled, cu_tiles,
                       cu_bad, pl...);
  });
}

template <class Tile, bool kTimed, class P>
void launch_rate(int blocks, uint32_t seed, int iters, unsigned* fails, unsigned long long* xt, unsigned* xw, PlantList<P> plants) {
  with_plants(plants, [&](auto... pl) {
    hipLaunchKernelGGL((mfma_throughput<Tile, kTimed, decltype(pl)...>), dim3(blocks), dim3(kBlock), 0, nullptr, seed, iters, fails,
                       xt, xw, pl...);
  });
}

// waves of `waves_per_cu` per CU as kBlock-thread blocks
int wave_blocks(int device, int waves_per_cu) { return std::max(1, cu_count(device) * waves_per_cu / (kBlock / 64)); }

// Host checks of test plants, all but `wave` before the device is touched.
bool check_plant_ok(const bgc_mfma_check_plant& p, int rounds) {
  return p.wave >= BGC_PLANT_ALL_WAVES && p.round >= 0 && p.round < rounds && p.lane >= 0 && p.lane < 64 && p.i >= 0 && p.i < 4;
}
bool rate_plant_ok(const bgc_mfma_rate_plant& p) {
  return p.wave >= 0 && p.lane >= 0 && p.lane < 64 && p.chain >= 0 && p.chain < 4 && p.i >= 0 && p.i < 4;
}
bool delay_ticks_ok(uint32_t ticks) { return ticks > 0 && ticks <= BGC_DIAG_MAX_DELAY_TICKS; }
bool delay_plant_ok(const bgc_mfma_delay_plant& p) { return p.wave >= BGC_PLANT_ALL_WAVES && delay_ticks_ok(p.ticks); }

// (launch, place in it) of a test plant: an MX plant names its check variant or rate format, the
// bf16 run has one launch of each kind.
std::pair<int, bgc_mfma_check_plant> split(const bgc_mfma_check_plant& p) { return {0, p}; }
std::pair<int, bgc_mfma_rate_plant> split(const bgc_mfma_rate_plant& p) { return {0, p}; }
std::pair<int, bgc_mfma_delay_plant> split(const bgc_mfma_delay_plant& p) { return {0, p}; }
std::pair<int, bgc_mfma_check_plant> split(const bgc_lowp_check_plant& p) { return {p.variant, p.at}; }
std::pair<int, bgc_mfma_rate_plant> split(const bgc_lowp_rate_plant& p) { return {p.fmt, p.at}; }

// The check-phase, the rate-phase or the delay plants of one run, sorted by the launch they belong to.
template <class At>
struct HostPlants {
  std::vector<At> host[4];
  DeviceBuffer dev[4];
  // Before the device is touched: false unless the list, every plant's launch (< launches) and its place
  // in it (ok(launch, place)) are valid.
  template <class P, class Ok>
  bool take(const P* plants, int n, int launches, Ok&& ok) {
    if (!plant_list_ok(plants, n)) return false;
    for (int j = 0; j < n; ++j) {
      const auto [launch, at] = split(plants[j]);
      if (launch < 0 || launch >= launches || !ok(launch, at)) return false;
      host[launch].push_back(at);
    }
    return true;
  }
  // Once the launch size is known: refuse a plant in a wave beyond it, then copy each launch's plants to
  // the device (a launch without plants allocates nothing).
  int upload(int blocks) {
    for (int l = 0; l < 4; ++l) {
      if (any_beyond(host[l].data(), host[l].size(), &At::wave, blocks * (kBlock / 64))) return refuse(kWaveBeyond);
      if (upload_plants(dev[l], host[l].data(), static_cast<int>(host[l].size())) != 0) return 1;
    }
    return 0;
  }
  PlantList<At> of(int launch) const { return {dev[launch].template as<const At>(), static_cast<int>(host[launch].size())}; }
};

// Per-CU bins of a run's kLaunches check launches: tiles checked and wrong elements by cu_key(),
// one slice of BGC_DIAG_MAX_CU_KEYS per launch.
template <int kLaunches>
struct CuBins {
  static constexpr size_t kWords = static_cast<size_t>(kLaunches) * BGC_DIAG_MAX_CU_KEYS;
  DeviceBuffer tiles, bad;
  int alloc() {
    HIP_TRY(tiles.alloc(kWords * sizeof(unsigned), true));
    HIP_TRY(bad.alloc(kWords * sizeof(unsigned), true));
    return 0;
  }
  unsigned* tiles_of(int launch) const { return tiles.as<unsigned>() + static_cast<size_t>(launch) * BGC_DIAG_MAX_CU_KEYS; }
  unsigned* bad_of(int launch) const { return bad.as<unsigned>() + static_cast<size_t>(launch) * BGC_DIAG_MAX_CU_KEYS; }
  // Download and fold: the result's tiles_checked, cus_seen, bad_cus (a CU that is bad in several launches
  // counts once) and first 64 bad_cu_keys, each launch's wrong elements, the XCCs that ran a check, and
  // the CUs that each launch ran on (launch_cus[kLaunches]).
  template <class Result>
  int fold(Result* out, uint64_t* const (&mismatches)[kLaunches], unsigned* xcc_mask = nullptr, int* launch_cus = nullptr) const {
    std::vector<unsigned> h_tiles(kWords), h_bad(kWords);
    HIP_TRY(hipMemcpy(h_tiles.data(), tiles.p, kWords * sizeof(unsigned), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_bad.data(), bad.p, kWords * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (int k = 0; k < BGC_DIAG_MAX_CU_KEYS; ++k) {
      bool seen = false, bad_here = false;
      for (int l = 0; l < kLaunches; ++l) {
        const size_t i = static_cast<size_t>(l) * BGC_DIAG_MAX_CU_KEYS + static_cast<size_t>(k);
        seen = seen || h_tiles[i];
        if (launch_cus && h_tiles[i]) launch_cus[l]++;
        bad_here = bad_here || h_bad[i];
        out->tiles_checked += h_tiles[i];
        *mismatches[l] += h_bad[i];
      }
      if (!seen) continue;
      out->cus_seen++;
      if (xcc_mask) *xcc_mask |= 1u << ((k >> 8) & 7);
      if (bad_here) note_bad_cu(out, k);
    }
    return 0;
  }
};

// FLOPs of one throughput launch: 4 chains of 16x16xkK MFMAs per wave and iteration
template <class Tile>
double rate_flops(int blocks, int iters) {
  return static_cast<double>(blocks) * (kBlock / 64) * iters * 4.0 * (2.0 * 16 * 16 * Tile::kK);
}

// Per-XCC bins of a timed (kTimed) throughput launch: the waves that ran on each XCC and the sum of their ticks.
struct XccBins {
  DeviceBuffer ticks, waves;
  int alloc() {
    HIP_TRY(ticks.alloc(8 * sizeof(unsigned long long)));
    HIP_TRY(waves.alloc(8 * sizeof(unsigned)));
    return 0;
  }
  int zero() const {
    HIP_TRY(hipMemset(ticks.p, 0, 8 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(waves.p, 0, 8 * sizeof(unsigned)));
    return 0;
  }
  unsigned long long* t() const { return ticks.as<unsigned long long>(); }
  unsigned* w() const { return waves.as<unsigned>(); }
};

bool any_delta(int /*launch*/, float /*delta*/) { return true; }

// What bgc_diag_mfma, bgc_diag_mfma_lowp and bgc_diag_mfma_classic share: kChecks check launches and up to
// four rate launches on the null stream, every launch with its own test plants.
template <int kChecks>
struct MatrixRun {
  const uint32_t seed;
  const int rounds;  // tiles per wave of a check launch
  int blocks = 0;
  HostPlants<bgc_mfma_check_plant> check_plants;  // by check launch
  HostPlants<bgc_mfma_rate_plant> rate_plants;    // by rate launch
  CuBins<kChecks> bins;                           // by check launch
  DeviceBuffer fails;                             // wrong accumulator elements, one word per rate launch
  Events ev;

  MatrixRun(uint32_t seed_, int rounds_) : seed(seed_), rounds(rounds_) {}

  // All that comes before the first launch.  Refuses with "invalid arguments" before the device is touched
  // unless the caller's own limits hold (limits_ok) and every plant names a launch, a place in it and, for
  // delta_ok(launch, delta), a delta that are valid; then clears *out, sizes the launches, uploads the
  // plants (refusing one in a wave beyond the launch) and allocates the bins, the counters and the events.
  template <class Result, class CheckPlant, class RatePlant>
  int begin(Result* out, bool limits_ok, int device, int waves_per_cu, const CheckPlant* check, int n_check, const RatePlant* rate,
            int n_rate, int rate_launches, bool (*delta_ok)(int, float) = any_delta) {
    if (!(out && limits_ok &&
          check_plants.take(check, n_check, kChecks,
                            [&](int l, const auto& at) { return check_plant_ok(at, rounds) && delta_ok(l, at.delta); }) &&
          rate_plants.take(rate, n_rate, rate_launches, [&](int l, const auto& at) { return rate_plant_ok(at) && delta_ok(l, at.delta); }))) {
      g_last_error = "invalid arguments";
      return 1;
    }
    std::memset(out, 0, sizeof(*out));
    HIP_TRY(hipSetDevice(device));
    blocks = wave_blocks(device, waves_per_cu);
    if (check_plants.upload(blocks) != 0 || rate_plants.upload(blocks) != 0 || bins.alloc() != 0) return 1;
    HIP_TRY(fails.alloc(4 * sizeof(unsigned), true));
    HIP_TRY(ev.create());
    return 0;
  }

  // check launch `launch`, into its slice of the bins; the caller puts its check launches in one timed window
  template <class Tile>
  void check(int launch, int scaled) const {
    launch_check<Tile>(blocks, seed, rounds, scaled, bins.tiles_of(launch), bins.bad_of(launch), check_plants.of(launch));
  }

  // Rate launch `launch`: after a warm-up launch of 64 iterations without plants and with the counters it
  // wrote zeroed again (if warm_up), the launch of `iters` iterations with `plants`, alone in a timed
  // window (*ms).  A kTimed launch bins its waves in *xcc.
  template <class Tile, bool kTimed, class P>
  int rate(int launch, int iters, bool warm_up, PlantList<P> plants, float* ms, const XccBins* xcc = nullptr) const {
    unsigned* f = fails.as<unsigned>() + launch;
    unsigned long long* xt = xcc ? xcc->t() : nullptr;
    unsigned* xw = xcc ? xcc->w() : nullptr;
    if (warm_up) {
      launch_rate<Tile, kTimed>(blocks, seed, 64, f, xt, xw, RatePlants{});
      HIP_TRY(hipMemset(f, 0, sizeof(unsigned)));
      if (xcc && xcc->zero() != 0) return 1;
    }
    return timed(ev, ms, [&] { launch_rate<Tile, kTimed>(blocks, seed, iters, f, xt, xw, plants); });
  }

  // after the last launch: whether every rate launch's accumulators matched
  int throughput_ok(int* ok) const {
    unsigned h[4];
    HIP_TRY(hipMemcpy(h, fails.p, sizeof(h), hipMemcpyDeviceToHost));
    *ok = (h[0] | h[1] | h[2] | h[3]) == 0;
    return 0;
  }
};

int mfma_run(int device, int waves_per_cu, int throughput_iters, uint32_t seed, const bgc_mfma_check_plant* check, int n_check,
             const bgc_mfma_rate_plant* rate, int n_rate, const bgc_mfma_delay_plant* delays, int n_delay, bgc_mfma_result* out) {
  MatrixRun<1> run(seed, BGC_MFMA_CHECK_ROUNDS);
  HostPlants<bgc_mfma_delay_plant> delay_plants;  // no entry point takes both these and rate plants
  XccBins xcc;
  const bool limits_ok = waves_per_cu > 0 && throughput_iters > 0 && throughput_iters <= (1 << 18) &&
                         delay_plants.take(delays, n_delay, 1, [](int, const auto& at) { return delay_plant_ok(at); });
  if (run.begin(out, limits_ok, device, waves_per_cu, check, n_check, rate, n_rate, 1) != 0 || delay_plants.upload(run.blocks) != 0 ||
      xcc.alloc() != 0) {
    return 1;
  }
  float ms_check = 0.f, ms_tp = 0.f;
  if (timed(run.ev, &ms_check, [&] { run.check<Bf16Tile>(0, 0); }) != 0) return 1;
  // warm-up, then the timed throughput launch with the delay plants or the value plants
  if ((n_delay > 0 ? run.rate<Bf16Tile, true>(0, throughput_iters, true, delay_plants.of(0), &ms_tp, &xcc)
                   : run.rate<Bf16Tile, true>(0, throughput_iters, true, run.rate_plants.of(0), &ms_tp, &xcc)) != 0) {
    return 1;
  }
  unsigned long long h_ticks[8];
  unsigned h_waves[8];
  HIP_TRY(hipMemcpy(h_ticks, xcc.ticks.p, sizeof(h_ticks), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_waves, xcc.waves.p, sizeof(h_waves), hipMemcpyDeviceToHost));
  const double ticks_per_us = constant_clock_khz(device) * 1e-3;
  TimingFold fold;  // of a wave's mean loop time on an XCC; the result names no slowest XCC
  for (int x = 0; x < 8; ++x) {
    out->xcc_waves[x] = static_cast<int>(h_waves[x]);
    out->xcc_wave_us[x] = fold.add(x, h_ticks[x], h_waves[x], ticks_per_us);
  }
  out->xcc_balance = fold.balance();
  unsigned xcc_mask = 0;
  if (run.bins.fold(out, {&out->mismatches}, &xcc_mask) != 0 || run.throughput_ok(&out->throughput_ok) != 0) return 1;
  out->xccs_seen = __builtin_popcount(xcc_mask);
  out->tflops = rate_flops<Bf16Tile>(run.blocks, throughput_iters) / (ms_tp * 1e-3) / 1e12;
  out->elapsed_ms = ms_check + ms_tp;
  return 0;
}

int lowp_run(int device, int waves_per_cu, int throughput_iters, uint32_t seed, const bgc_lowp_check_plant* check, int n_check,
             const bgc_lowp_rate_plant* rate, int n_rate, bgc_lowp_result* out) {
  // launches: check variant (0 fp8, 1 fp8 scaled, 2 fp4, 3 fp4 scaled), rate format (0 fp8, 1 fp4)
  MatrixRun<4> run(seed, BGC_LOWP_CHECK_ROUNDS);
  const bool limits_ok = waves_per_cu > 0 && waves_per_cu <= 64 && throughput_iters > 0 && throughput_iters <= (1 << 16);
  if (run.begin(out, limits_ok, device, waves_per_cu, check, n_check, rate, n_rate, 2) != 0) return 1;
  float ms_check = 0.f, ms_fmt[2] = {0.f, 0.f};
  if (timed(run.ev, &ms_check, [&] {
        for (int sc = 0; sc < 2; ++sc) {
          run.check<MxTile<0>>(sc, sc);
          run.check<MxTile<4>>(2 + sc, sc);
        }
      }) != 0) {
    return 1;
  }
  // one fp8 warm-up for both formats, then one timed launch per format
  if (run.rate<MxTile<0>, false>(0, throughput_iters, true, run.rate_plants.of(0), &ms_fmt[0]) != 0 ||
      run.rate<MxTile<4>, false>(1, throughput_iters, false, run.rate_plants.of(1), &ms_fmt[1]) != 0) {
    return 1;
  }
  if (run.bins.fold(out, {&out->fp8_mismatches, &out->fp8_scaled_mismatches, &out->fp4_mismatches, &out->fp4_scaled_mismatches}) != 0 ||
      run.throughput_ok(&out->throughput_ok) != 0) {
    return 1;
  }
  const double flops = rate_flops<MxTile<0>>(run.blocks, throughput_iters);  // the same for fp4
  out->fp8_tflops = tera_per_s(flops, ms_fmt[0]);
  out->fp4_tflops = tera_per_s(flops, ms_fmt[1]);
  out->elapsed_ms = ms_check + ms_fmt[0] + ms_fmt[1];
  return 0;
}

// An int8-path plant adds its delta to an i32 accumulator: a finite integer below 2^31 in magnitude.
bool classic_delta_ok(int path, float delta) {
  return path != BGC_CLASSIC_INT8 || (std::isfinite(delta) && delta == std::trunc(delta) && std::fabs(delta) < 2147483648.f);
}

int classic_run(int device, int waves_per_cu, int throughput_iters, uint32_t seed, const bgc_lowp_check_plant* check, int n_check,
                const bgc_lowp_rate_plant* rate, int n_rate, bgc_classic_result* out) {
  // launches: one check and one rate launch per path (BGC_CLASSIC_*)
  MatrixRun<4> run(seed, BGC_CLASSIC_CHECK_ROUNDS);
  const bool limits_ok = waves_per_cu > 0 && waves_per_cu <= 64 && throughput_iters > 0 && throughput_iters <= (1 << 16);
  if (run.begin(out, limits_ok, device, waves_per_cu, check, n_check, rate, n_rate, 4, classic_delta_ok) != 0) return 1;
  float total = 0.f;
  if (timed(run.ev, &total, [&] {
        for (int p = 0; p < 4; ++p) {
          with_classic_path(p, [&](auto path) { run.check<DenseTile<decltype(path), true>>(p, 0); });
        }
      }) != 0) {
    return 1;
  }
  // per path: a warm-up launch, then one timed launch
  for (int p = 0; p < 4; ++p) {
    float ms = 0.f;
    double flops = 0;
    const int rc = with_classic_path(p, [&](auto path) {
      using Tile = DenseTile<decltype(path), false>;
      flops = rate_flops<Tile>(run.blocks, throughput_iters);
      return run.rate<Tile, false>(p, throughput_iters, true, run.rate_plants.of(p), &ms);
    });
    if (rc != 0) return 1;
    out->rate_ms[p] = ms;
    out->rate[p] = tera_per_s(flops, ms);
    total += ms;
  }
  int path_cus[4] = {0, 0, 0, 0};
  if (run.bins.fold(out, {&out->mismatches[0], &out->mismatches[1], &out->mismatches[2], &out->mismatches[3]}, nullptr, path_cus) != 0 ||
      run.throughput_ok(&out->throughput_ok) != 0) {
    return 1;
  }
  // Consecutive launches need not land on the same CUs, so the union over the paths says nothing about
  // one path: report the coverage that every path reached.
  out->cus_seen = *std::min_element(path_cus, path_cus + 4);
  out->elapsed_ms = total;
  return 0;
}

// The value plants of a burn (bgc_diag_burn_planted), sorted by the launch they name: a burn has as many
// launches as its duration allows, so they are one device array and a launch takes its own stretch of it.
struct BurnValuePlants {
  std::vector<int> launch;                // ascending
  std::vector<bgc_mfma_rate_plant> host;  // in the same order
  DeviceBuffer dev;
  // Before the device is touched: false unless the list, every plant's launch (>= 0) and its place are valid.
  bool take(const bgc_burn_plant* plants, int n) {
    if (!plant_list_ok(plants, n)) return false;
    std::vector<bgc_burn_plant> sorted(plants, plants + n);
    std::stable_sort(sorted.begin(), sorted.end(), [](const bgc_burn_plant& a, const bgc_burn_plant& b) { return a.launch < b.launch; });
    for (const bgc_burn_plant& p : sorted) {
      if (p.launch < 0 || !rate_plant_ok(p.at)) return false;
      launch.push_back(p.launch);
      host.push_back(p.at);
    }
    return true;
  }
  // Once the launch size is known: refuse a plant in a wave beyond it, then copy the plants to the device.
  int upload(int blocks) {
    if (any_beyond(host.data(), host.size(), &bgc_mfma_rate_plant::wave, blocks * (kBlock / 64))) return refuse(kWaveBeyond);
    return upload_plants(dev, host.data(), static_cast<int>(host.size()));
  }
  RatePlants of(int l) const {
    const auto [lo, hi] = std::equal_range(launch.begin(), launch.end(), l);
    if (lo == hi) return {};
    return {dev.as<const bgc_mfma_rate_plant>() + (lo - launch.begin()), static_cast<int>(hi - lo)};
  }
};

// bgc_diag_burn_dtype; bgc_diag_burn_delayed with every wave of the launches from `first_delayed_launch`
// on delayed by `ticks` (0: no launch is delayed); and bgc_diag_burn_planted with `plants` applied in the
// launches they name.  No entry point takes both kinds; without either this is the production burn.
int burn_run(int device, int duration_ms, int waves_per_cu, uint32_t seed, int dtype, int first_delayed_launch, uint32_t ticks,
             const bgc_burn_plant* plants, int n, bgc_burn_result* out) {
  BurnValuePlants value_plants;
  if (!out || duration_ms <= 0 || duration_ms > 600000 || waves_per_cu <= 0 || waves_per_cu > 64 ||
      dtype < BGC_BURN_BF16 || dtype > BGC_BURN_FP4 || !value_plants.take(plants, n)) {
    g_last_error = "invalid arguments";
    return 1;
  }
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(device));
  const int blocks = wave_blocks(device, waves_per_cu);
  HostPlants<bgc_mfma_delay_plant> delay_plants;
  if (ticks > 0) {
    delay_plants.host[0].push_back({BGC_PLANT_ALL_WAVES, ticks});
    if (delay_plants.upload(blocks) != 0) return 1;
  }
  if (value_plants.upload(blocks) != 0) return 1;
  DeviceBuffer fails;
  XccBins xcc;  // the bf16 kernel writes them; the burn does not read them
  HIP_TRY(fails.alloc(sizeof(unsigned), true));
  if (xcc.alloc() != 0) return 1;
  Events ev, total;
  HIP_TRY(ev.create());
  HIP_TRY(total.create());
  // size one launch to ~10 ms at MI355X rates (iters * 4 MFMA per wave), measured below
  int iters = 2048;
  const double flops_per_iter = with_burn_dtype(dtype, [&](auto tile, auto) { return rate_flops<decltype(tile)>(blocks, 1); });
  // the longest launch whose accumulators the kernel still compares exactly: kK * iters <= 2^23 (gpu_diag.h)
  const int max_iters = with_burn_dtype(dtype, [](auto tile, auto) { return (1 << 23) / decltype(tile)::kK; });
  float ms = 0.f;
  HIP_TRY(hipEventRecord(total.a, nullptr));
  double sum_flops = 0;
  while (true) {
    const DelayPlants delays = ticks > 0 && out->launches >= first_delayed_launch ? delay_plants.of(0) : DelayPlants{};
    const RatePlants values = value_plants.of(out->launches);
    if (timed(ev, &ms, [&] {
          with_burn_dtype(dtype, [&](auto tile, auto timed_per_xcc) {
            auto launch = [&](auto pl) {
              launch_rate<decltype(tile), decltype(timed_per_xcc)::value>(blocks, seed, iters, fails.as<unsigned>(), xcc.t(), xcc.w(), pl);
            };
            if (values.n > 0) {
              launch(values);
            } else {
              launch(delays);
            }
          });
        }) != 0) {
      return 1;
    }
    const double tf = flops_per_iter * iters / (ms * 1e-3) / 1e12;
    out->tflops_max = std::max(out->tflops_max, tf);
    if (out->launches == 0) {
      out->tflops_first = tf;
      out->tflops_min = tf;
      // retune the launch length to ~10 ms now that the rate is known
      iters = std::max(64, std::min(max_iters, static_cast<int>(iters * (10.0 / std::max(0.01f, ms)))));
    } else {
      out->tflops_min = std::min(out->tflops_min, tf);
    }
    out->tflops_last = tf;
    out->launches++;
    sum_flops += flops_per_iter * (out->launches == 1 ? 2048 : iters);
    HIP_TRY(hipEventRecord(total.b, nullptr));
    HIP_TRY(hipEventSynchronize(total.b));
    float so_far = 0.f;
    HIP_TRY(hipEventElapsedTime(&so_far, total.a, total.b));
    out->elapsed_ms = so_far;
    if (so_far >= static_cast<float>(duration_ms)) break;
  }
  unsigned h_fails = 0;
  HIP_TRY(hipMemcpy(&h_fails, fails.p, sizeof(unsigned), hipMemcpyDeviceToHost));
  out->mismatches = h_fails;
  out->tflops_mean = sum_flops / (out->elapsed_ms * 1e-3) / 1e12;
  return 0;
}

// mfma_tile<Tile> by one wave: what its 64 lanes held, to lanes[0..63]
template <class Tile>
int tile_run(int device, uint32_t seed, uint32_t tile, int scaled, typename Tile::Lane* lanes) {
  using Lane = typename Tile::Lane;
  HIP_TRY(hipSetDevice(device));
  DeviceBuffer d;
  HIP_TRY(d.alloc(64 * sizeof(Lane), true));
  hipLaunchKernelGGL(mfma_tile<Tile>, dim3(1), dim3(64), 0, nullptr, seed, tile, scaled, d.as<Lane>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(lanes, d.p, 64 * sizeof(Lane), hipMemcpyDeviceToHost));
  return 0;
}

// dense_gemm<Path> on host operands, or `refusal` as the last error unless M and N are multiples of 16
// up to 4096 and K a multiple of the path's K up to 8192
template <class Path, class CElem>
int gemm_run(int device, int m, int n, int k, const void* a, const void* b, CElem* c, const char* refusal) {
  using Elem = typename Path::Elem;
  if (!a || !b || !c || m <= 0 || n <= 0 || k <= 0 || m % 16 || n % 16 || k % Path::kK || m > 4096 || n > 4096 || k > 8192) {
    g_last_error = refusal;
    return 1;
  }
  HIP_TRY(hipSetDevice(device));
  const size_t a_bytes = static_cast<size_t>(m) * k * sizeof(Elem), b_bytes = static_cast<size_t>(k) * n * sizeof(Elem);
  return gemm_on_host_operands({{a, a_bytes}, {b, b_bytes}}, c, static_cast<size_t>(m) * n, [&](const void* const* d, CElem* dc) {
    hipLaunchKernelGGL((dense_gemm<Path, CElem>), dim3(n / 16, m / 16), dim3(64), 0, nullptr, static_cast<const Elem*>(d[0]),
                       static_cast<const Elem*>(d[1]), dc, m, n, k);
  });
}

}  // namespace

extern "C" {

int bgc_diag_mfma(int device, int waves_per_cu, int throughput_iters, uint32_t seed, bgc_mfma_result* out) {
  return mfma_run(device, waves_per_cu, throughput_iters, seed, nullptr, 0, nullptr, 0, nullptr, 0, out);
}

int bgc_diag_mfma_planted(int device, int waves_per_cu, int throughput_iters, uint32_t seed, const bgc_mfma_check_plant* check,
                          int n_check, const bgc_mfma_rate_plant* rate, int n_rate, bgc_mfma_result* out) {
  return mfma_run(device, waves_per_cu, throughput_iters, seed, check, n_check, rate, n_rate, nullptr, 0, out);
}

int bgc_diag_mfma_delayed(int device, int waves_per_cu, int throughput_iters, uint32_t seed, const bgc_mfma_delay_plant* delays, int n,
                          bgc_mfma_result* out) {
  return mfma_run(device, waves_per_cu, throughput_iters, seed, nullptr, 0, nullptr, 0, delays, n, out);
}

int bgc_diag_mfma_lowp(int device, int waves_per_cu, int throughput_iters, uint32_t seed, bgc_lowp_result* out) {
  return lowp_run(device, waves_per_cu, throughput_iters, seed, nullptr, 0, nullptr, 0, out);
}

int bgc_diag_mfma_lowp_planted(int device, int waves_per_cu, int throughput_iters, uint32_t seed, const bgc_lowp_check_plant* check,
                               int n_check, const bgc_lowp_rate_plant* rate, int n_rate, bgc_lowp_result* out) {
  return lowp_run(device, waves_per_cu, throughput_iters, seed, check, n_check, rate, n_rate, out);
}

int bgc_diag_mfma_classic(int device, int waves_per_cu, int throughput_iters, uint32_t seed, bgc_classic_result* out) {
  return classic_run(device, waves_per_cu, throughput_iters, seed, nullptr, 0, nullptr, 0, out);
}

int bgc_diag_mfma_classic_planted(int device, int waves_per_cu, int throughput_iters, uint32_t seed, const bgc_lowp_check_plant* check,
                                  int n_check, const bgc_lowp_rate_plant* rate, int n_rate, bgc_classic_result* out) {
  return classic_run(device, waves_per_cu, throughput_iters, seed, check, n_check, rate, n_rate, out);
}

int bgc_diag_mfma_classic_tile(int device, int path, uint32_t seed, uint32_t tile, bgc_classic_tile_lane* lanes) {
  if (!lanes || path < BGC_CLASSIC_FP16 || path > BGC_CLASSIC_FP64) {
    g_last_error = "invalid arguments";
    return 1;
  }
  return with_classic_path(path, [&](auto p) { return tile_run<DenseTile<decltype(p), true>>(device, seed, tile, 0, lanes); });
}

int bgc_diag_gemm_dtype(int device, int path, int m, int n, int k, const void* a, const void* b, double* c) {
  static const char* const kRefusal =
      "invalid arguments (path 0..3; M, N multiples of 16 up to 4096; K a multiple of the path's K up to 8192)";
  if (path < BGC_CLASSIC_FP16 || path > BGC_CLASSIC_FP64) {
    g_last_error = kRefusal;
    return 1;
  }
  return with_classic_path(path, [&](auto p) { return gemm_run<decltype(p)>(device, m, n, k, a, b, c, kRefusal); });
}

int bgc_diag_mfma_tile(int device, int path, int scaled, uint32_t seed, uint32_t tile, bgc_tile_lane* lanes) {
  if (!lanes || path < BGC_TILE_BF16 || path > BGC_TILE_FP4 || (scaled != 0 && scaled != 1) || (scaled && path == BGC_TILE_BF16)) {
    g_last_error = "invalid arguments";
    return 1;
  }
  if (path == BGC_TILE_BF16) return tile_run<Bf16Tile>(device, seed, tile, scaled, lanes);
  return with_mx_fmt(path == BGC_TILE_FP8 ? 0 : 4,
                     [&](auto fmt) { return tile_run<MxTile<decltype(fmt)::value>>(device, seed, tile, scaled, lanes); });
}

int bgc_diag_burn(int device, int duration_ms, int waves_per_cu, uint32_t seed, bgc_burn_result* out) {
  return bgc_diag_burn_dtype(device, duration_ms, waves_per_cu, seed, BGC_BURN_BF16, out);
}

int bgc_diag_burn_dtype(int device, int duration_ms, int waves_per_cu, uint32_t seed, int dtype, bgc_burn_result* out) {
  return burn_run(device, duration_ms, waves_per_cu, seed, dtype, 0, 0, nullptr, 0, out);
}

int bgc_diag_burn_delayed(int device, int duration_ms, int waves_per_cu, uint32_t seed, int dtype, int first_delayed_launch,
                          uint32_t ticks, bgc_burn_result* out) {
  if (first_delayed_launch < 0 || !delay_ticks_ok(ticks)) {
    g_last_error = "invalid arguments";
    return 1;
  }
  return burn_run(device, duration_ms, waves_per_cu, seed, dtype, first_delayed_launch, ticks, nullptr, 0, out);
}

int bgc_diag_burn_planted(int device, int duration_ms, int waves_per_cu, uint32_t seed, int dtype, const bgc_burn_plant* plants, int n,
                          bgc_burn_result* out) {
  return burn_run(device, duration_ms, waves_per_cu, seed, dtype, 0, 0, plants, n, out);
}

int bgc_diag_gemm(int device, int m, int n, int k, const uint16_t* a_bf16, const uint16_t* b_bf16, float* c) {
  return gemm_run<Bf16Path>(device, m, n, k, a_bf16, b_bf16, c,
                            "invalid arguments (M, N multiples of 16 up to 4096; K a multiple of 32 up to 8192)");
}

int bgc_diag_mx_gemm(int device, int fmt, int m, int n, int k, const uint8_t* a, const uint8_t* a_scales,
                     const uint8_t* bt, const uint8_t* bt_scales, float* c) {
  if (!a || !a_scales || !bt || !bt_scales || !c || (fmt != 0 && fmt != 4) || m <= 0 || n <= 0 || k <= 0 ||
      m % 16 || n % 16 || k % 128 || m > 16384 || n > 16384 || k > 65536) {
    g_last_error = "invalid arguments: fmt 0 (fp8 e4m3) or 4 (fp4 e2m1); m, n multiples of 16 (<= 16384), k of 128 (<= 65536)";
    return 1;
  }
  HIP_TRY(hipSetDevice(device));
  const size_t per_byte = fmt == 0 ? 1 : 2;  // codes per byte
  const size_t a_bytes = static_cast<size_t>(m) * k / per_byte, b_bytes = static_cast<size_t>(n) * k / per_byte;
  const size_t sa_bytes = static_cast<size_t>(m) * (k / 32), sb_bytes = static_cast<size_t>(n) * (k / 32);
  return gemm_on_host_operands(
      {{a, a_bytes}, {a_scales, sa_bytes}, {bt, b_bytes}, {bt_scales, sb_bytes}}, c, static_cast<size_t>(m) * n,
      [&](const void* const* d, float* dc) {
        auto p = [&](int i) { return static_cast<const uint8_t*>(d[i]); };
        with_mx_fmt(fmt, [&](auto f) {
          hipLaunchKernelGGL(mx_gemm<decltype(f)::value>, dim3(static_cast<unsigned>((m / 16) * (n / 16))), dim3(64), 0,
                             nullptr, p(0), p(1), p(2), p(3), dc, m, n, k);
        });
      });
}

}  // extern "C"
