// Matrix cores: the per-CU bf16 MFMA check and throughput (bgc_diag_mfma), the MX fp8/fp4
// block-scaled check and throughput (bgc_diag_mfma_lowp), the burn-in loop that runs the
// throughput kernels back to back (bgc_diag_burn_dtype), and the one-wave-per-tile GEMMs on
// caller operands (bgc_diag_gemm, bgc_diag_mx_gemm).
//
//  * The MFMA test runs one v_mfma_f32_16x16x32_bf16 tile per wave per round with
//    operands in {-1,0,1} generated from a hash in registers (no memory traffic), so
//    every product sum is an exact fp32 integer and is checked element-wise against a
//    VALU recomputation.  Each wave records its physical CU (HW_REG_XCC_ID + HW_ID),
//    so a faulty matrix core is attributed to (XCC, SE, SH, CU).
//  * The throughput phase chains 4 independent accumulators per wave (dependent MFMA
//    latency hidden by 8 waves/SIMD) and verifies acc == iters * tile exactly.
#include <algorithm>
#include <cstring>

#include "diag_common.h"

namespace {

using namespace bgc_diag;

__device__ __forceinline__ int operand(uint32_t seed, uint32_t tile, int r, int c, uint32_t which) {
  uint32_t h = mix32(seed ^ mix32(tile * 0x9e3779b9U + which) ^ static_cast<uint32_t>(r * 64 + c));
  return static_cast<int>(h % 3u) - 1;
}

__device__ __forceinline__ uint32_t cu_key() {
  uint32_t xcc, hwid;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  uint32_t cu = (hwid >> 8) & 0xF;
  uint32_t sh = (hwid >> 12) & 0x1;
  uint32_t se = (hwid >> 13) & 0x7;
  return ((xcc & 0x7) << 8) | (se << 5) | (sh << 4) | cu;
}

// ---------------------------------------------------------------------------
// Tile traits: a 16x16xkK MFMA on hash-derived operands.  Lane l holds its part of A row
// (l & 15) and of B column (l & 15) from lane group l >> 4; the result lane l holds column
// (l & 15), rows 4 (l >> 4) + i (the C/D map of every 16x16 MFMA).  A element (row, k) is
// operand(seed, tile, row, k, 0xA); B element (k, col) is b_operand(seed, tile, k, col).

// v_mfma_f32_16x16x32_bf16: A is 16x32, B is 32x16, lane group g holds k = 8 g + j.
struct Bf16Tile {
  using Frag = bf16x8;
  static constexpr int kK = 32;
  static __device__ __forceinline__ Frag pack(uint32_t seed, uint32_t tile, int rc, int g, uint32_t which) {
    Frag v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int o = which == 0xA ? operand(seed, tile, rc, 8 * g + j, 0xA) : b_operand(seed, tile, 8 * g + j, rc);
      v[j] = static_cast<__bf16>(static_cast<float>(o));
    }
    return v;
  }
  static __device__ __forceinline__ f32x4 mfma(Frag a, Frag b, f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }
  static __device__ __forceinline__ int b_operand(uint32_t seed, uint32_t tile, int k, int col) {
    return operand(seed, tile, k, col, 0xB);
  }
};

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

template <int kFmt>
__device__ __forceinline__ f32x4 lowp_mfma(i32x8 a, i32x8 b, f32x4 acc, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, kFmt, kFmt, 0, 127 + sa, 0, 127 + sb);
}

// the MX tile with unit scales: both operands are indexed (row or column, k)
template <int kFmt>
struct MxTile {
  using Frag = i32x8;
  static constexpr int kK = 128;
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
  static __device__ __forceinline__ f32x4 mfma(Frag a, Frag b, f32x4 acc) { return lowp_mfma<kFmt>(a, b, acc, 0, 0); }
  static __device__ __forceinline__ int b_operand(uint32_t seed, uint32_t tile, int k, int col) {
    return operand(seed, tile, col, k, 0xB);
  }
};

// ---------------------------------------------------------------------------
// Check kernels: wave w checks tiles w * rounds .. w * rounds + rounds - 1 element-wise and bins
// the outcome by the CU it runs on.
struct CheckWave {
  int lane;
  uint32_t wave, key;
  __device__ __forceinline__ CheckWave()
      : lane(threadIdx.x & 63), wave((blockIdx.x * (kBlock / 64)) + (threadIdx.x >> 6)), key(cu_key()) {}
  __device__ __forceinline__ uint32_t tile(int rounds, int r) const {
    return wave * static_cast<uint32_t>(rounds) + static_cast<uint32_t>(r);
  }
  // one atomic per wave: `bad` is the wave's sum of wrong elements, in lane 0
  __device__ __forceinline__ void report(int rounds, unsigned bad, unsigned* cu_tiles, unsigned* cu_bad) const {
    if (lane == 0) {
      atomicAdd(&cu_tiles[key], static_cast<unsigned>(rounds));
      if (bad) atomicAdd(&cu_bad[key], bad);
    }
  }
};

// Test plants (gpu_diag.h, "planted variants").  The check and throughput kernels end in a pack
// `Plants... plants`: empty in the production instantiations, which so take no further argument and
// call the empty plant() overloads (they compile to what they would be without), and one plant list
// in the instantiations behind the *_planted entry points.  Everything else, the comparison, the
// wave reduction and the report, is the same source for both.
struct CheckPlants {
  const bgc_mfma_check_plant* p;
  int n;
};
struct RatePlants {
  const bgc_mfma_rate_plant* p = nullptr;
  int n = 0;
};

__device__ __forceinline__ void add_at(f32x4& acc, int i, float delta) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e == i) acc[e] += delta;
  }
}

// check phase: before round `round`'s comparison
__device__ __forceinline__ void plant(f32x4&, uint32_t /*wave*/, int /*round*/, int /*lane*/) {}
__device__ __forceinline__ void plant(f32x4& acc, uint32_t wave, int round, int lane, CheckPlants pl) {
  for (int j = 0; j < pl.n; ++j) {
    const bgc_mfma_check_plant p = pl.p[j];
    if ((p.wave == BGC_PLANT_ALL_WAVES || static_cast<uint32_t>(p.wave) == wave) && p.round == round && p.lane == lane) {
      add_at(acc, p.i, p.delta);
    }
  }
}

// throughput phase: after the loop, before the comparison
__device__ __forceinline__ void plant(f32x4 (&)[4], uint32_t /*wave*/, int /*lane*/) {}
__device__ __forceinline__ void plant(f32x4 (&acc)[4], uint32_t wave, int lane, RatePlants pl) {
  for (int j = 0; j < pl.n; ++j) {
    const bgc_mfma_rate_plant p = pl.p[j];
    if (static_cast<uint32_t>(p.wave) != wave || p.lane != lane) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c == p.chain) add_at(acc[c], p.i, p.delta);
    }
  }
}

template <class... Plants>
__global__ __launch_bounds__(kBlock) void mfma_check(uint32_t seed, int rounds, unsigned* __restrict__ cu_tiles,
                                                     unsigned* __restrict__ cu_bad, Plants... plants) {
  const CheckWave w;
  const int rc = w.lane & 15, g = w.lane >> 4;
  unsigned bad = 0;
  for (int r = 0; r < rounds; ++r) {
    const uint32_t tile = w.tile(rounds, r);
    const bf16x8 a = Bf16Tile::pack(seed, tile, rc, g, 0xA);
    const bf16x8 b = Bf16Tile::pack(seed, tile, rc, g, 0xB);
    f32x4 acc = Bf16Tile::mfma(a, b, f32x4{0.f, 0.f, 0.f, 0.f});
    plant(acc, w.wave, r, w.lane, plants...);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int orow = 4 * g + i;
      int expect = 0;
      for (int k = 0; k < 32; ++k) expect += operand(seed, tile, orow, k, 0xA) * Bf16Tile::b_operand(seed, tile, k, rc);
      bad += (acc[i] != static_cast<float>(expect));
    }
  }
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
  w.report(rounds, bad, cu_tiles, cu_bad);
}

template <int kFmt, class... Plants>
__global__ __launch_bounds__(kBlock) void mfma_lowp_check(uint32_t seed, int rounds, int scaled,
                                                          unsigned* __restrict__ cu_tiles,
                                                          unsigned* __restrict__ cu_bad, Plants... plants) {
  const CheckWave w;
  const int rc = w.lane & 15, g = w.lane >> 4;
  unsigned bad = 0;
  for (int r = 0; r < rounds; ++r) {
    const uint32_t tile = w.tile(rounds, r);
    const i32x8 a = MxTile<kFmt>::pack(seed, tile, rc, g, 0xA);
    const i32x8 b = MxTile<kFmt>::pack(seed, tile, rc, g, 0xB);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = lowp_mfma<kFmt>(a, b, acc, lowp_exp(seed, tile, rc, g, 0xA, scaled), lowp_exp(seed, tile, rc, g, 0xB, scaled));
    plant(acc, w.wave, r, w.lane, plants...);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int orow = 4 * g + i;
      int dot[4] = {0, 0, 0, 0};  // per scale block
      for (int gg = 0; gg < 4; ++gg) {
        for (int j = 0; j < 32; ++j) {
          dot[lowp_block<kFmt>(gg, j)] +=
              operand(seed, tile, orow, 32 * gg + j, 0xA) * operand(seed, tile, rc, 32 * gg + j, 0xB);
        }
      }
      float expect = 0.f;
      for (int blk = 0; blk < 4; ++blk) {
        const int e = lowp_exp(seed, tile, orow, blk, 0xA, scaled) + lowp_exp(seed, tile, rc, blk, 0xB, scaled);
        expect += ldexpf(static_cast<float>(dot[blk]), e);
      }
      bad += (acc[i] != expect);
    }
  }
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
  w.report(rounds, bad, cu_tiles, cu_bad);
}

// ---------------------------------------------------------------------------
// Throughput: 4 independent accumulator chains per wave, acc == iters * tile + c.  With kTimed
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
  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f32x4{float(c), float(c), float(c), float(c)};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = Tile::mfma(a, b, acc[c]);
  }
  plant(acc, tile, lane, plants...);
  unsigned bad = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int orow = 4 * g + i;
    int expect = 0;
    for (int k = 0; k < Tile::kK; ++k) expect += operand(seed, tile, orow, k, 0xA) * Tile::b_operand(seed, tile, k, rc);
    const float e = static_cast<float>(expect) * static_cast<float>(iters);
#pragma unroll
    for (int c = 0; c < 4; ++c) bad += (acc[c][i] != e + float(c));
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

// Plain MFMA GEMM for the host cross-check: C[M,N] (fp32) = A[M,K] * B[K,N] (bf16,
// row-major).  One wave per 16x16 output tile (grid N/16 x M/16), K consumed 32 at a time by
// v_mfma_f32_16x16x32_bf16 with the same operand layout as the tests above: lane l
// holds A row (l & 15) / B column (l & 15), k = 8 * (l >> 4) + j; the result lane l
// holds column (l & 15), rows 4 * (l >> 4) + i.
__global__ __launch_bounds__(64) void mfma_gemm(const __bf16* __restrict__ A, const __bf16* __restrict__ B,
                                                float* __restrict__ C, int /*M*/, int N, int K) {
  const int lane = threadIdx.x;
  const int tm = blockIdx.y * 16, tn = blockIdx.x * 16;
  const int rc = lane & 15, kb = 8 * (lane >> 4);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 32) {
    bf16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = A[static_cast<size_t>(tm + rc) * K + k0 + kb + j];
      b[j] = B[static_cast<size_t>(k0 + kb + j) * N + tn + rc];
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) C[static_cast<size_t>(tm + 4 * (lane >> 4) + i) * N + tn + rc] = acc[i];
}

// `f(std::integral_constant<int, kFmt>)` for MX format 0 (fp8 e4m3) or 4 (fp4 e2m1)
template <class F>
void with_mx_fmt(int fmt, F&& f) {
  if (fmt == 0) {
    f(std::integral_constant<int, 0>{});
  } else {
    f(std::integral_constant<int, 4>{});
  }
}

// the production instantiation, or with test plants the planted one
template <class Tile, bool kTimed>
void launch_rate(int blocks, uint32_t seed, int iters, unsigned* fails, unsigned long long* xt, unsigned* xw, RatePlants plants) {
  if (plants.n == 0) {
    hipLaunchKernelGGL((mfma_throughput<Tile, kTimed>), dim3(blocks), dim3(kBlock), 0, nullptr, seed, iters, fails, xt, xw);
  } else {
    hipLaunchKernelGGL((mfma_throughput<Tile, kTimed, RatePlants>), dim3(blocks), dim3(kBlock), 0, nullptr, seed, iters, fails,
                       xt, xw, plants);
  }
}

// one throughput launch of a burn dtype: bf16 (timed per XCC into xt / xw) or MX fp8 / fp4
void launch_throughput(int dtype, int blocks, uint32_t seed, int iters, unsigned* fails, unsigned long long* xt = nullptr,
                       unsigned* xw = nullptr, RatePlants plants = {}) {
  if (dtype == BGC_BURN_BF16) {
    launch_rate<Bf16Tile, true>(blocks, seed, iters, fails, xt, xw, plants);
  } else {
    with_mx_fmt(dtype == BGC_BURN_FP8 ? 0 : 4,
                [&](auto fmt) { launch_rate<MxTile<decltype(fmt)::value>, false>(blocks, seed, iters, fails, xt, xw, plants); });
  }
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

// plants in device memory; none allocates nothing
template <class P>
int upload_plants(DeviceBuffer& d, const std::vector<P>& plants) {
  if (plants.empty()) return 0;
  HIP_TRY(d.alloc(plants.size() * sizeof(P)));
  HIP_TRY(hipMemcpy(d.p, plants.data(), plants.size() * sizeof(P), hipMemcpyHostToDevice));
  return 0;
}

int mfma_run(int device, int waves_per_cu, int throughput_iters, uint32_t seed, const bgc_mfma_check_plant* check, int n_check,
             const bgc_mfma_rate_plant* rate, int n_rate, bgc_mfma_result* out) {
  const int rounds = BGC_MFMA_CHECK_ROUNDS;
  bool ok = out && waves_per_cu > 0 && throughput_iters > 0 && throughput_iters <= (1 << 18) && plant_list_ok(check, n_check) &&
            plant_list_ok(rate, n_rate);
  for (int j = 0; ok && j < n_check; ++j) ok = check_plant_ok(check[j], rounds);
  for (int j = 0; ok && j < n_rate; ++j) ok = rate_plant_ok(rate[j]);
  if (!ok) {
    g_last_error = "invalid arguments";
    return 1;
  }
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(device));
  const int blocks = wave_blocks(device, waves_per_cu);
  const std::vector<bgc_mfma_check_plant> h_check(check, check + n_check);
  const std::vector<bgc_mfma_rate_plant> h_rate(rate, rate + n_rate);
  for (const auto& p : h_check) ok = ok && p.wave < blocks * (kBlock / 64);
  for (const auto& p : h_rate) ok = ok && p.wave < blocks * (kBlock / 64);
  if (!ok) {
    g_last_error = "invalid arguments: plant in a wave beyond the launch";
    return 1;
  }
  DeviceBuffer d_check, d_rate;
  if (upload_plants(d_check, h_check) != 0 || upload_plants(d_rate, h_rate) != 0) return 1;
  DeviceBuffer tiles, bad, fails, xticks, xwaves;
  HIP_TRY(tiles.alloc(BGC_DIAG_MAX_CU_KEYS * sizeof(unsigned), true));
  HIP_TRY(bad.alloc(BGC_DIAG_MAX_CU_KEYS * sizeof(unsigned), true));
  HIP_TRY(fails.alloc(sizeof(unsigned)));
  HIP_TRY(xticks.alloc(8 * sizeof(unsigned long long)));
  HIP_TRY(xwaves.alloc(8 * sizeof(unsigned)));
  Events ev;
  HIP_TRY(ev.create());
  float ms_check = 0.f, ms_tp = 0.f;
  if (timed(ev, &ms_check, [&] {
        if (n_check == 0) {
          hipLaunchKernelGGL(mfma_check<>, dim3(blocks), dim3(kBlock), 0, nullptr, seed, rounds, tiles.as<unsigned>(),
                             bad.as<unsigned>());
        } else {
          hipLaunchKernelGGL(mfma_check<CheckPlants>, dim3(blocks), dim3(kBlock), 0, nullptr, seed, rounds, tiles.as<unsigned>(),
                             bad.as<unsigned>(), CheckPlants{d_check.as<const bgc_mfma_check_plant>(), n_check});
        }
      }) != 0) {
    return 1;
  }
  // warm-up then timed throughput pass
  auto* xt = xticks.as<unsigned long long>();
  auto* xw = xwaves.as<unsigned>();
  launch_throughput(BGC_BURN_BF16, blocks, seed, 64, fails.as<unsigned>(), xt, xw);
  HIP_TRY(hipMemset(fails.p, 0, sizeof(unsigned)));
  HIP_TRY(hipMemset(xticks.p, 0, 8 * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(xwaves.p, 0, 8 * sizeof(unsigned)));
  const RatePlants rate_plants{d_rate.as<const bgc_mfma_rate_plant>(), n_rate};
  if (timed(ev, &ms_tp, [&] { launch_throughput(BGC_BURN_BF16, blocks, seed, throughput_iters, fails.as<unsigned>(), xt, xw, rate_plants); }) != 0) {
    return 1;
  }
  std::vector<unsigned> h_tiles(BGC_DIAG_MAX_CU_KEYS), h_bad(BGC_DIAG_MAX_CU_KEYS);
  unsigned h_fails = 0;
  HIP_TRY(hipMemcpy(h_tiles.data(), tiles.p, h_tiles.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_bad.data(), bad.p, h_bad.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&h_fails, fails.p, sizeof(unsigned), hipMemcpyDeviceToHost));
  unsigned long long h_ticks[8];
  unsigned h_waves[8];
  HIP_TRY(hipMemcpy(h_ticks, xticks.p, sizeof(h_ticks), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_waves, xwaves.p, sizeof(h_waves), hipMemcpyDeviceToHost));
  int rate_khz = 0;
  if (hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || rate_khz <= 0) {
    rate_khz = 100000;  // CDNA constant clock: 100 MHz
  }
  double lo = 0, hi = 0;
  for (int x = 0; x < 8; ++x) {
    out->xcc_waves[x] = static_cast<int>(h_waves[x]);
    out->xcc_wave_us[x] = h_waves[x] ? static_cast<double>(h_ticks[x]) / h_waves[x] / (rate_khz * 1e-3) : 0.0;
    if (!h_waves[x]) continue;
    lo = lo == 0 ? out->xcc_wave_us[x] : std::min(lo, out->xcc_wave_us[x]);
    hi = std::max(hi, out->xcc_wave_us[x]);
  }
  out->xcc_balance = hi > 0 ? lo / hi : 0.0;
  bool xcc_seen[8] = {false};
  for (int k = 0; k < BGC_DIAG_MAX_CU_KEYS; ++k) {
    if (!h_tiles[static_cast<size_t>(k)]) continue;
    out->cus_seen++;
    out->tiles_checked += h_tiles[static_cast<size_t>(k)];
    xcc_seen[(k >> 8) & 7] = true;
    if (h_bad[static_cast<size_t>(k)]) {
      out->mismatches += h_bad[static_cast<size_t>(k)];
      if (out->bad_cus < 64) out->bad_cu_keys[out->bad_cus] = k;
      out->bad_cus++;
    }
  }
  for (bool s : xcc_seen) out->xccs_seen += s ? 1 : 0;
  const double waves = static_cast<double>(blocks) * (kBlock / 64);
  const double flops = waves * throughput_iters * 4.0 * (2.0 * 16 * 16 * Bf16Tile::kK);
  out->tflops = flops / (ms_tp * 1e-3) / 1e12;
  out->throughput_ok = h_fails == 0;
  out->elapsed_ms = ms_check + ms_tp;
  return 0;
}

int lowp_run(int device, int waves_per_cu, int throughput_iters, uint32_t seed, const bgc_lowp_check_plant* check, int n_check,
             const bgc_lowp_rate_plant* rate, int n_rate, bgc_lowp_result* out) {
  const int rounds = BGC_LOWP_CHECK_ROUNDS;
  bool ok = out && waves_per_cu > 0 && waves_per_cu <= 64 && throughput_iters > 0 && throughput_iters <= (1 << 16) &&
            plant_list_ok(check, n_check) && plant_list_ok(rate, n_rate);
  for (int j = 0; ok && j < n_check; ++j) ok = check[j].variant >= 0 && check[j].variant < 4 && check_plant_ok(check[j].at, rounds);
  for (int j = 0; ok && j < n_rate; ++j) ok = (rate[j].fmt == 0 || rate[j].fmt == 1) && rate_plant_ok(rate[j].at);
  if (!ok) {
    g_last_error = "invalid arguments";
    return 1;
  }
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(device));
  const int blocks = wave_blocks(device, waves_per_cu);
  // test plants, sorted by the launch they belong to: check variant [fmt][scaled], rate format
  std::vector<bgc_mfma_check_plant> h_check[4];
  std::vector<bgc_mfma_rate_plant> h_rate[2];
  for (int j = 0; j < n_check; ++j) {
    ok = ok && check[j].at.wave < blocks * (kBlock / 64);
    h_check[check[j].variant].push_back(check[j].at);
  }
  for (int j = 0; j < n_rate; ++j) {
    ok = ok && rate[j].at.wave < blocks * (kBlock / 64);
    h_rate[rate[j].fmt].push_back(rate[j].at);
  }
  if (!ok) {
    g_last_error = "invalid arguments: plant in a wave beyond the launch";
    return 1;
  }
  DeviceBuffer d_check[4], d_rate[2];
  for (int v = 0; v < 4; ++v) {
    if (upload_plants(d_check[v], h_check[v]) != 0) return 1;
  }
  for (int i = 0; i < 2; ++i) {
    if (upload_plants(d_rate[i], h_rate[i]) != 0) return 1;
  }
  auto launch_check = [&](auto fmt, int sc, unsigned* tiles_v, unsigned* bad_v) {
    constexpr int kFmt = decltype(fmt)::value;
    const int v = (kFmt == 0 ? 0 : 2) + sc;
    if (h_check[v].empty()) {
      hipLaunchKernelGGL(mfma_lowp_check<kFmt>, dim3(blocks), dim3(kBlock), 0, nullptr, seed, rounds, sc, tiles_v, bad_v);
    } else {
      hipLaunchKernelGGL((mfma_lowp_check<kFmt, CheckPlants>), dim3(blocks), dim3(kBlock), 0, nullptr, seed, rounds, sc, tiles_v, bad_v,
                         CheckPlants{d_check[v].as<const bgc_mfma_check_plant>(), static_cast<int>(h_check[v].size())});
    }
  };
  // bins: [fmt][scaled] tiles and mismatches per CU key
  DeviceBuffer tiles, bad, fails;
  const size_t bins = 4 * static_cast<size_t>(BGC_DIAG_MAX_CU_KEYS);
  HIP_TRY(tiles.alloc(bins * sizeof(unsigned), true));
  HIP_TRY(bad.alloc(bins * sizeof(unsigned), true));
  HIP_TRY(fails.alloc(2 * sizeof(unsigned)));
  auto* t = tiles.as<unsigned>();
  auto* b = bad.as<unsigned>();
  auto* f = fails.as<unsigned>();
  Events ev;
  HIP_TRY(ev.create());
  float total = 0.f;
  if (timed(ev, &total, [&] {
        for (int sc = 0; sc < 2; ++sc) {
          const size_t o8 = static_cast<size_t>(sc) * BGC_DIAG_MAX_CU_KEYS, o4 = (2 + static_cast<size_t>(sc)) * BGC_DIAG_MAX_CU_KEYS;
          launch_check(std::integral_constant<int, 0>{}, sc, t + o8, b + o8);
          launch_check(std::integral_constant<int, 4>{}, sc, t + o4, b + o4);
        }
      }) != 0) {
    return 1;
  }
  // warm-up, then one timed launch per format
  launch_throughput(BGC_BURN_FP8, blocks, seed, 64, f);
  HIP_TRY(hipMemset(f, 0, 2 * sizeof(unsigned)));
  float ms_fmt[2] = {0.f, 0.f};
  for (int i = 0; i < 2; ++i) {
    const RatePlants rate_plants{d_rate[i].as<const bgc_mfma_rate_plant>(), static_cast<int>(h_rate[i].size())};
    if (timed(ev, &ms_fmt[i], [&] {
          launch_throughput(i == 0 ? BGC_BURN_FP8 : BGC_BURN_FP4, blocks, seed, throughput_iters, f + i, nullptr, nullptr, rate_plants);
        }) != 0) {
      return 1;
    }
    total += ms_fmt[i];
  }
  std::vector<unsigned> h_t(bins), h_b(bins);
  unsigned h_f[2] = {0, 0};
  HIP_TRY(hipMemcpy(h_t.data(), t, bins * sizeof(unsigned), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_b.data(), b, bins * sizeof(unsigned), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_f, f, sizeof(h_f), hipMemcpyDeviceToHost));
  uint64_t* mism[4] = {&out->fp8_mismatches, &out->fp8_scaled_mismatches, &out->fp4_mismatches,
                       &out->fp4_scaled_mismatches};
  for (int k = 0; k < BGC_DIAG_MAX_CU_KEYS; ++k) {
    unsigned seen = 0, bad_here = 0;
    for (int v = 0; v < 4; ++v) {
      const size_t i = static_cast<size_t>(v) * BGC_DIAG_MAX_CU_KEYS + static_cast<size_t>(k);
      seen += h_t[i];
      bad_here += h_b[i];
      *mism[v] += h_b[i];
      out->tiles_checked += h_t[i];
    }
    if (!seen) continue;
    out->cus_seen++;
    if (bad_here) {
      if (out->bad_cus < 64) out->bad_cu_keys[out->bad_cus] = k;
      out->bad_cus++;
    }
  }
  const double waves = static_cast<double>(blocks) * (kBlock / 64);
  const double flops = waves * throughput_iters * 4.0 * (2.0 * 16 * 16 * MxTile<0>::kK);
  out->fp8_tflops = ms_fmt[0] > 0 ? flops / (ms_fmt[0] * 1e-3) / 1e12 : 0.0;
  out->fp4_tflops = ms_fmt[1] > 0 ? flops / (ms_fmt[1] * 1e-3) / 1e12 : 0.0;
  out->throughput_ok = h_f[0] == 0 && h_f[1] == 0;
  out->elapsed_ms = total;
  return 0;
}

}  // namespace

extern "C" {

int bgc_diag_mfma(int device, int waves_per_cu, int throughput_iters, uint32_t seed, bgc_mfma_result* out) {
  return mfma_run(device, waves_per_cu, throughput_iters, seed, nullptr, 0, nullptr, 0, out);
}

int bgc_diag_mfma_planted(int device, int waves_per_cu, int throughput_iters, uint32_t seed, const bgc_mfma_check_plant* check,
                          int n_check, const bgc_mfma_rate_plant* rate, int n_rate, bgc_mfma_result* out) {
  return mfma_run(device, waves_per_cu, throughput_iters, seed, check, n_check, rate, n_rate, out);
}

int bgc_diag_mfma_lowp(int device, int waves_per_cu, int throughput_iters, uint32_t seed, bgc_lowp_result* out) {
  return lowp_run(device, waves_per_cu, throughput_iters, seed, nullptr, 0, nullptr, 0, out);
}

int bgc_diag_mfma_lowp_planted(int device, int waves_per_cu, int throughput_iters, uint32_t seed, const bgc_lowp_check_plant* check,
                               int n_check, const bgc_lowp_rate_plant* rate, int n_rate, bgc_lowp_result* out) {
  return lowp_run(device, waves_per_cu, throughput_iters, seed, check, n_check, rate, n_rate, out);
}

int bgc_diag_burn(int device, int duration_ms, int waves_per_cu, uint32_t seed, bgc_burn_result* out) {
  return bgc_diag_burn_dtype(device, duration_ms, waves_per_cu, seed, BGC_BURN_BF16, out);
}

int bgc_diag_burn_dtype(int device, int duration_ms, int waves_per_cu, uint32_t seed, int dtype, bgc_burn_result* out) {
  if (!out || duration_ms <= 0 || duration_ms > 600000 || waves_per_cu <= 0 || waves_per_cu > 64 ||
      dtype < BGC_BURN_BF16 || dtype > BGC_BURN_FP4) {
    g_last_error = "invalid arguments";
    return 1;
  }
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(device));
  const int blocks = wave_blocks(device, waves_per_cu);
  DeviceBuffer fails, xticks, xwaves;
  HIP_TRY(fails.alloc(sizeof(unsigned), true));
  HIP_TRY(xticks.alloc(8 * sizeof(unsigned long long)));
  HIP_TRY(xwaves.alloc(8 * sizeof(unsigned)));
  Events ev, total;
  HIP_TRY(ev.create());
  HIP_TRY(total.create());
  // size one launch to ~10 ms at MI355X rates (iters * 4 MFMA per wave), measured below
  int iters = 2048;
  const double mfma_k = dtype == BGC_BURN_BF16 ? Bf16Tile::kK : MxTile<0>::kK;
  const double flops_per_iter = static_cast<double>(blocks) * (kBlock / 64) * 4.0 * (2.0 * 16 * 16 * mfma_k);
  float ms = 0.f;
  HIP_TRY(hipEventRecord(total.a, nullptr));
  double sum_flops = 0;
  while (true) {
    if (timed(ev, &ms, [&] {
          launch_throughput(dtype, blocks, seed, iters, fails.as<unsigned>(), xticks.as<unsigned long long>(), xwaves.as<unsigned>());
        }) != 0) {
      return 1;
    }
    const double tf = flops_per_iter * iters / (ms * 1e-3) / 1e12;
    out->tflops_max = std::max(out->tflops_max, tf);
    if (out->launches == 0) {
      out->tflops_first = tf;
      out->tflops_min = tf;
      // retune the launch length to ~10 ms now that the rate is known
      iters = std::max(64, std::min(1 << 18, static_cast<int>(iters * (10.0 / std::max(0.01f, ms)))));
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

int bgc_diag_gemm(int device, int m, int n, int k, const uint16_t* a_bf16, const uint16_t* b_bf16, float* c) {
  if (!a_bf16 || !b_bf16 || !c || m <= 0 || n <= 0 || k <= 0 || m % 16 || n % 16 || k % 32 || m > 4096 ||
      n > 4096 || k > 8192) {
    g_last_error = "invalid arguments (M, N multiples of 16 up to 4096; K a multiple of 32 up to 8192)";
    return 1;
  }
  HIP_TRY(hipSetDevice(device));
  const size_t a_bytes = static_cast<size_t>(m) * k * 2, b_bytes = static_cast<size_t>(k) * n * 2;
  return gemm_on_host_operands({{a_bf16, a_bytes}, {b_bf16, b_bytes}}, c, static_cast<size_t>(m) * n,
                               [&](const void* const* d, float* dc) {
                                 hipLaunchKernelGGL(mfma_gemm, dim3(n / 16, m / 16), dim3(64), 0, nullptr,
                                                    static_cast<const __bf16*>(d[0]), static_cast<const __bf16*>(d[1]), dc, m, n, k);
                               });
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
