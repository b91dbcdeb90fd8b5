// The vector ALU: the per-SIMD check of its integer, fp32, fp16, fp64, conversion, integer-dot and
// transcendental instructions, and the vector rates (bgc_diag_valu).
//
//  * No wave waits for another, there is no barrier and no LDS, and every address is a function of
//    blockIdx, threadIdx, loop counters and arguments checked on the host: nothing read from memory
//    is used as an index.  The buffers are sized exactly for the launch: waves * 7 * 64 digests,
//    waves (CU key, SIMD) pairs, 4 * rounds * 5 * 64 raw transcendental results of workgroup 0,
//    waves * 64 end digests of a rate launch.
//  * valu_check: cus * waves_per_simd workgroups of 256 threads.  A workgroup's four waves normally
//    land on the four SIMDs of one CU; that is observed (each wave records cu_key() and simd_id(),
//    and the result counts the distinct ones), not promised, and nothing is wrong without it.  Every
//    wave runs the rounds of valu_ref.h's valu_round with DeviceAlu, the gfx950 builtins, on operands
//    hashed per lane (so nothing can move to the scalar unit), folds each result word into the lane's
//    digest of its class and writes the digests with plain vector stores.  It compares nothing: the
//    host (referee(), below) recomputes the six exact classes with valu_ref.h's HostAlu and judges
//    the transcendentals by the waves' consensus and, on the raw results that workgroup 0 also
//    writes, against double-precision libm.  Consensus alone cannot see a fault common to every
//    unit; the accuracy bound can.
//  * Contraction is off in this file: HIP's default would fuse the sequence's separate multiply and
//    add into an FMA, which the host could not reproduce.
//  * valu_rate<class, timed>: the same grid, `iters` iterations of 8 independent chains per lane.
//    The multiplier and the addend arrive as kernel arguments, so the compiler cannot fold the
//    chain.  Each wave times its loop on the 100 MHz constant clock into its CU's bin and writes
//    one end digest per lane, which the host compares with its own (trans: with the consensus).
//    Checked in the gfx950 disassembly: the loop runs four iterations a trip, and its body is 32
//    v_pk_fma_f32 (fp32), 32 v_pk_fma_f16, 32 v_fma_f64, 32 v_mad_u32_u24 (written as an instruction:
//    from __umul24(x, a) + b the compiler made v_mul_lo_u32 and v_add_u32) or 32 v_exp_f32 with the 32
//    multiplies of the chain as v_mul_f32 and v_pk_mul_f32, and the loop control (s_add_i32 twice,
//    s_mov_b32, s_cmp, s_cbranch; the int32 loop also one s_nop 0); a second loop of 8 chain
//    instructions takes the iterations left over.  No scratch, no spills (27 VGPRs in valu_check, at
//    most 22 in a rate kernel).  Measured on the MI355X at the defaults, 2 waves per SIMD and 16384 iterations (profiles/valu_diag/rates.json): 115-121 TF/s fp32 of the 157.3 TF/s
//    vector peak, 126-130 TF/s fp16, 59-61 TF/s fp64, 60-62 TOP/s int32 and 12.3-12.4 T v_exp_f32 per
//    second; 8 waves per SIMD reach 128-130, 138-140, 67-68, 68-69 and 12.8-13.0.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "diag_common.h"
#include "valu_ref.h"

#pragma clang fp contract(off)

namespace {

using namespace bgc_diag;
namespace ref = bgc_valu;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f16x2 halves(uint32_t bits) { return __builtin_bit_cast(f16x2, bits); }
__device__ __forceinline__ uint32_t bits_of(f16x2 x) { return __builtin_bit_cast(uint32_t, x); }

// valu_ref.h's operations as gfx950 instructions (named in gpu_diag.h next to BGC_VALU_*)
struct DeviceAlu {
  __device__ static uint32_t mul_hi(uint32_t a, uint32_t b) { return __umulhi(a, b); }
  __device__ static uint32_t mad24(uint32_t a, uint32_t b, uint32_t c) { return __umul24(a, b) + c; }
  __device__ static uint32_t bfe(uint32_t a, uint32_t offset, uint32_t width) { return __builtin_amdgcn_ubfe(a, offset, width); }
  __device__ static uint32_t perm(uint32_t a, uint32_t b, uint32_t sel) { return __builtin_amdgcn_perm(a, b, sel); }
  __device__ static uint32_t alignbit(uint32_t a, uint32_t b, uint32_t shift) { return __builtin_amdgcn_alignbit(a, b, shift); }
  __device__ static uint32_t popcount(uint32_t a) { return static_cast<uint32_t>(__builtin_popcount(a)); }
  __device__ static uint32_t clz(uint32_t a) { return a ? static_cast<uint32_t>(__builtin_clz(a)) : 32u; }
  __device__ static float fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
  __device__ static void pk_fma(const float a[2], const float b[2], const float c[2], float r[2]) {
    const f32x2 v = __builtin_elementwise_fma(f32x2{a[0], a[1]}, f32x2{b[0], b[1]}, f32x2{c[0], c[1]});
    r[0] = v.x;
    r[1] = v.y;
  }
  __device__ static float mul(float a, float b) { return a * b; }
  __device__ static float add(float a, float b) { return a + b; }
  // as an instruction: from a - b the compiler made a v_pk_add_f32 with a negate modifier
  __device__ static float sub(float a, float b) {
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
  }
  __device__ static uint32_t pk_fma_f16(uint32_t a, uint32_t b, uint32_t c) {
    return bits_of(__builtin_elementwise_fma(halves(a), halves(b), halves(c)));
  }
  __device__ static uint32_t pk_add_f16(uint32_t a, uint32_t b) { return bits_of(halves(a) + halves(b)); }
  __device__ static uint32_t pk_mul_f16(uint32_t a, uint32_t b) { return bits_of(halves(a) * halves(b)); }
  __device__ static double fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
  __device__ static double add(double a, double b) { return a + b; }
  __device__ static double mul(double a, double b) { return a * b; }
  __device__ static int32_t f32_to_i32(float x) { return static_cast<int32_t>(x); }
  __device__ static float i32_to_f32(int32_t x) { return static_cast<float>(x); }
  __device__ static uint32_t f32_to_f16(float x) { return __builtin_bit_cast(uint16_t, static_cast<_Float16>(x)); }
  __device__ static float f16_to_f32(uint32_t h) { return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(h))); }
  __device__ static uint32_t pk_bf16(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, bf16x2{static_cast<__bf16>(lo), static_cast<__bf16>(hi)});
  }
  __device__ static int32_t sdot4(int32_t a, int32_t b, int32_t c) { return __builtin_amdgcn_sdot4(a, b, c, false); }
  __device__ static uint32_t udot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }
  __device__ static float exp2(float x) { return __builtin_amdgcn_exp2f(x); }
  __device__ static float log2(float x) { return __builtin_amdgcn_logf(x); }
  __device__ static float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
  __device__ static float rsq(float x) { return __builtin_amdgcn_rsqf(x); }
  __device__ static float sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
};

// Test plants and the generated-data copy (gpu_diag.h).  Both kernels end in a pack `Extras... extras`:
// empty in the production instantiations, which take the empty tap() below and no after_loop().
struct CheckExtras {  // in device memory
  const bgc_valu_plant* p = nullptr;
  int n = 0;
  int dump_wave = -1;
  uint32_t* raw = nullptr;  // rounds * 40 * 64 words
};
struct RateExtras {
  const bgc_valu_rate_plant* p = nullptr;
  int n = 0;
  const bgc_valu_delay_plant* d = nullptr;
  int nd = 0;
  int dump_wave = -1;
  int* cu_keys = nullptr;  // of dump_wave, one per rate class
};

// a result word on its way into the digest
__device__ __forceinline__ uint32_t tap(uint32_t v, int /*wave*/, int /*cls*/, int /*round*/, int /*lane*/, int /*word*/) { return v; }
__device__ __forceinline__ uint32_t tap(uint32_t v, int wave, int cls, int round, int lane, int word, const CheckExtras& x) {
  for (int j = 0; j < x.n; ++j) {
    const bgc_valu_plant p = x.p[j];
    if ((p.wave == BGC_PLANT_ALL_WAVES || p.wave == wave) && p.cls == cls && p.round == round && p.lane == lane && p.op == word) v ^= p.xor_mask;
  }
  if (wave == x.dump_wave) x.raw[(round * ref::kRoundWords + ref::word_base(cls) + word) * 64 + lane] = v;
  return v;
}

template <class... Extras>
__global__ __launch_bounds__(kBlock) void valu_check(uint32_t seed, int rounds, uint32_t* __restrict__ digests, int2* __restrict__ where,
                                                     uint32_t* __restrict__ trans_raw, Extras... extras) {
  const int lane = threadIdx.x & 63, wave_of_wg = threadIdx.x >> 6, wave = blockIdx.x * (kBlock / 64) + wave_of_wg;
  uint32_t d[ref::kClasses];
#pragma unroll
  for (int c = 0; c < ref::kClasses; ++c) d[c] = ref::digest_start(c);
#pragma unroll 1
  for (int r = 0; r < rounds; ++r) {
    ref::valu_round<DeviceAlu>(seed, r, lane, [&](int cls, int word, uint32_t v) {
      v = tap(v, wave, cls, r, lane, word, extras...);
      if (cls == BGC_VALU_TRANS && blockIdx.x == 0) trans_raw[((wave_of_wg * rounds + r) * 5 + word) * 64 + lane] = v;
      d[cls] = ref::mix32(d[cls] ^ v);
    });
  }
#pragma unroll
  for (int c = 0; c < ref::kClasses; ++c) digests[(wave * ref::kClasses + c) * 64 + lane] = d[c];
  if (lane == 0) where[wave] = int2{static_cast<int>(cu_key()), static_cast<int>(simd_id())};
}

// A rate class's chain: its value type, start, step and result words.  `a` and `b` are the multiplier and the addend as
// the kernel receives them (float bits; fp16: packed halves; int32: the LCG's constants).
template <int kClass>
struct Chain;
template <>
struct Chain<BGC_VALU_RATE_FP32> {
  using T = f32x2;
  static constexpr int kWords = 2;
  __device__ static T start(uint32_t, int lane, int c) {
    return T{static_cast<float>(ref::fma_start(lane, 2 * c)), static_cast<float>(ref::fma_start(lane, 2 * c + 1))};
  }
  __device__ static T constant(uint32_t bits) { return T{ref::f32_of(bits), ref::f32_of(bits)}; }
  __device__ static T step(T x, T a, T b) { return __builtin_elementwise_fma(x, a, b); }
  __device__ static uint32_t word(T x, int i) { return ref::bits_of(i ? x.y : x.x); }
  __device__ static T flip(T x, uint32_t mask) { return T{ref::f32_of(ref::bits_of(x.x) ^ mask), x.y}; }
};
template <>
struct Chain<BGC_VALU_RATE_FP16> {
  using T = f16x2;
  static constexpr int kWords = 1;
  __device__ static T start(uint32_t, int lane, int c) {
    return T{static_cast<_Float16>(ref::fma_start(lane, 2 * c)), static_cast<_Float16>(ref::fma_start(lane, 2 * c + 1))};
  }
  __device__ static T constant(uint32_t bits) { return halves(bits); }
  __device__ static T step(T x, T a, T b) { return __builtin_elementwise_fma(x, a, b); }
  __device__ static uint32_t word(T x, int) { return bits_of(x); }
  __device__ static T flip(T x, uint32_t mask) { return halves(bits_of(x) ^ mask); }
};
template <>
struct Chain<BGC_VALU_RATE_FP64> {
  using T = double;
  static constexpr int kWords = 2;
  __device__ static T start(uint32_t, int lane, int c) { return static_cast<double>(ref::fma_start(lane, c)); }
  __device__ static T constant(uint32_t bits) { return static_cast<double>(ref::f32_of(bits)); }
  __device__ static T step(T x, T a, T b) { return __builtin_fma(x, a, b); }
  __device__ static uint32_t word(T x, int i) { return static_cast<uint32_t>(ref::bits_of(x) >> (32 * i)); }
  __device__ static T flip(T x, uint32_t mask) { return ref::f64_of(ref::bits_of(x) ^ mask); }
};
template <>
struct Chain<BGC_VALU_RATE_INT32> {
  using T = uint32_t;
  static constexpr int kWords = 1;
  __device__ static T start(uint32_t seed, int lane, int c) { return ref::lcg_start(seed, lane, c); }
  __device__ static T constant(uint32_t bits) { return bits; }
  // as an instruction: from __umul24(x, a) + b the compiler made v_mul_lo_u32 and v_add_u32 for three steps of four
  __device__ static T step(T x, T a, T b) {
    T r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(a), "v"(b));
    return r;
  }
  __device__ static uint32_t word(T x, int) { return x; }
  __device__ static T flip(T x, uint32_t mask) { return x ^ mask; }
};
template <>
struct Chain<BGC_VALU_RATE_TRANS> {
  using T = float;
  static constexpr int kWords = 1;
  __device__ static T start(uint32_t, int lane, int c) { return ref::exp_start(lane, c); }
  __device__ static T constant(uint32_t bits) { return ref::f32_of(bits); }
  __device__ static T step(T x, T a, T) { return __builtin_amdgcn_exp2f(x) * a; }
  __device__ static uint32_t word(T x, int) { return ref::bits_of(x); }
  __device__ static T flip(T x, uint32_t mask) { return ref::f32_of(ref::bits_of(x) ^ mask); }
};

// after the loop: the value plants, where the dumped wave runs, then the wait for the largest `ticks` that names this wave
template <class C>
__device__ __forceinline__ void after_loop(typename C::T* x, int cls, int wave, int lane, const RateExtras& e, C) {
  for (int j = 0; j < e.n; ++j) {
    const bgc_valu_rate_plant p = e.p[j];
    if ((p.wave == BGC_PLANT_ALL_WAVES || p.wave == wave) && p.cls == cls && p.lane == lane) {
#pragma unroll
      for (int c = 0; c < ref::kChains; ++c) {
        if (c == p.chain) x[c] = C::flip(x[c], p.xor_mask);
      }
    }
  }
  if (wave == e.dump_wave && lane == 0) e.cu_keys[cls] = static_cast<int>(cu_key());
  uint32_t ticks = 0;
  for (int j = 0; j < e.nd; ++j) {
    const bgc_valu_delay_plant p = e.d[j];
    if ((p.wave == BGC_PLANT_ALL_WAVES || p.wave == wave) && p.cls == cls) ticks = max(ticks, p.ticks);
  }
  wait_ticks(__builtin_amdgcn_readfirstlane(ticks));  // the same in every lane of the wave
}

template <int kClass, bool kTimed, class... Extras>
__global__ __launch_bounds__(kBlock) void valu_rate(uint32_t seed, int iters, uint32_t a_bits, uint32_t b_bits, uint32_t* __restrict__ ends,
                                                    RateBin* __restrict__ bins, Extras... extras) {
  using C = Chain<kClass>;
  using T = typename C::T;
  const int lane = threadIdx.x & 63, wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const T a = C::constant(a_bits), b = C::constant(b_bits);
  T x[ref::kChains];
#pragma unroll
  for (int c = 0; c < ref::kChains; ++c) x[c] = C::start(seed, lane, c);
  uint64_t t0 = 0, t1 = 0;
  if constexpr (kTimed) {
    t0 = wall_clock64();
    asm volatile("" ::"s"(t0));  // wait for the clock here, not inside the loop
  }
  auto step = [&] {
#pragma unroll
    for (int c = 0; c < ref::kChains; ++c) x[c] = C::step(x[c], a, b);
  };
  int it = 0;
#pragma unroll 1
  for (; it + 4 <= iters; it += 4) {  // four iterations per trip: the loop control is a twelfth of the body
    step();
    step();
    step();
    step();
  }
#pragma unroll 1
  for (; it < iters; ++it) step();
#pragma unroll
  for (int c = 0; c < ref::kChains; ++c) asm volatile("" : "+v"(x[c]));  // every chain has ended before the clock is read
  if constexpr (sizeof...(Extras) > 0) after_loop(x, kClass, wave, lane, extras..., C{});
  if constexpr (kTimed) t1 = wall_clock64();
  uint32_t d = ref::rate_digest_start(kClass);
#pragma unroll
  for (int c = 0; c < ref::kChains; ++c) {
#pragma unroll
    for (int i = 0; i < C::kWords; ++i) d = ref::mix32(d ^ C::word(x[c], i));
  }
  ends[wave * 64 + lane] = d;
  if constexpr (kTimed) {
    if (lane == 0) {
      RateBin* bin = &bins[cu_key()];
      atomicAdd(&bin->ticks, static_cast<unsigned long long>(t1 - t0));
      atomicAdd(&bin->n, 1u);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host

struct ValuArgs {
  int waves_per_simd, rounds, rate_iters;
  uint32_t seed;
};

// what the test-only entries add to a run; all empty in bgc_diag_valu
struct ValuExtras {
  const bgc_valu_plant* check = nullptr;
  int n_check = 0;
  const bgc_valu_rate_plant* rate = nullptr;
  int n_rate = 0;
  const bgc_valu_delay_plant* delays = nullptr;
  int n_delay = 0;
  bool want_data = false;
  int wave = 0;
  bgc_valu_wave* data = nullptr;
};

bool rounds_ok(int rounds) { return rounds >= 1 && rounds <= 64; }

bool args_ok(const ValuArgs& a) {
  return a.waves_per_simd >= 1 && a.waves_per_simd <= 8 && rounds_ok(a.rounds) && a.rate_iters >= 1 && a.rate_iters <= (1 << 16);
}

bool extras_ok(const ValuArgs& a, const ValuExtras& x) {
  if (!plant_list_ok(x.check, x.n_check) || !plant_list_ok(x.rate, x.n_rate) || !plant_list_ok(x.delays, x.n_delay)) return false;
  const bool check_ok = std::all_of(x.check, x.check + x.n_check, [&](const bgc_valu_plant& p) {
    return p.wave >= BGC_PLANT_ALL_WAVES && p.cls >= 0 && p.cls < ref::kClasses && p.round >= 0 && p.round < a.rounds && p.lane >= 0 &&
           p.lane < 64 && p.op >= 0 && p.op < ref::class_words(p.cls) && p.xor_mask != 0;
  });
  const bool rate_ok = std::all_of(x.rate, x.rate + x.n_rate, [](const bgc_valu_rate_plant& p) {
    return p.wave >= BGC_PLANT_ALL_WAVES && p.cls >= 0 && p.cls < ref::kRateClasses && p.lane >= 0 && p.lane < 64 && p.chain >= 0 &&
           p.chain < ref::kChains && p.xor_mask != 0;
  });
  const bool delays_ok = std::all_of(x.delays, x.delays + x.n_delay, [](const bgc_valu_delay_plant& p) {
    return p.wave >= BGC_PLANT_ALL_WAVES && p.cls >= 0 && p.cls < ref::kRateClasses && p.ticks > 0 && p.ticks <= BGC_DIAG_MAX_DELAY_TICKS;
  });
  return check_ok && rate_ok && delays_ok && (!x.want_data || (x.data && x.wave >= 0));
}

// The 64-word vector that more than half of `waves` vectors (`stride` words apart) equal: its wave, or -1.
int consensus(const uint32_t* vectors, int waves, size_t stride) {
  auto same = [&](int v, int w) { return std::memcmp(vectors + v * stride, vectors + w * stride, 64 * sizeof(uint32_t)) == 0; };
  int candidate = 0, lead = 0;
  for (int w = 0; w < waves; ++w) {
    if (lead == 0) {
      candidate = w;
      lead = 1;
    } else {
      lead += same(candidate, w) ? 1 : -1;
    }
  }
  int holders = 0;
  for (int w = 0; w < waves; ++w) holders += same(candidate, w);
  return 2 * holders > waves ? candidate : -1;
}

// The host's verdict on the check launch: digests[(wave * 7 + class) * 64 + lane], where[wave] = (CU key, SIMD),
// trans_raw[((wave of workgroup 0 * rounds + round) * 5 + op) * 64 + lane].
void referee(const ValuArgs& a, int waves, const std::vector<uint32_t>& digests, const std::vector<int2>& where,
             const std::vector<uint32_t>& trans_raw, bgc_valu_result* out) {
  std::vector<uint32_t> expect(ref::kClasses * 64);
  ref::expected(a.seed, a.rounds, nullptr, expect.data());
  const size_t stride = ref::kClasses * 64;
  const uint32_t* trans = digests.data() + BGC_VALU_TRANS * 64;  // wave 0's; wave w's is w * stride further
  const int holder = consensus(trans, waves, stride);
  out->consensus_ok = holder >= 0;
  std::vector<int> order(static_cast<size_t>(waves));
  std::iota(order.begin(), order.end(), 0);
  auto place = [&](int w) { return std::make_pair(where[static_cast<size_t>(w)].x, where[static_cast<size_t>(w)].y); };
  std::stable_sort(order.begin(), order.end(), [&](int v, int w) { return place(v) < place(w); });
  std::pair<int, int> last_seen{-1, -1}, last_bad{-1, -1};
  for (int w : order) {
    const auto at = place(w);
    if (at.first != last_seen.first) out->cus_seen++;
    if (at != last_seen) out->simds_seen++;
    last_seen = at;
    for (int c = 0; c < ref::kClasses; ++c) {
      const uint32_t* want = c != BGC_VALU_TRANS ? expect.data() + c * 64 : holder >= 0 ? trans + holder * stride : nullptr;
      const uint32_t* got = digests.data() + w * stride + static_cast<size_t>(c) * 64;
      for (int lane = 0; want && lane < 64; ++lane) {
        if (got[lane] == want[lane]) continue;
        out->mismatches[c]++;
        out->bad_lanes |= 1ULL << lane;
        if (out->first_bad_cu_key < 0) {
          out->first_bad_cu_key = at.first;
          out->first_bad_simd = at.second;
          out->first_bad_lane = lane;
          out->first_bad_class = c;
        }
        if (at.first != last_bad.first) note_bad_cu(out, at.first);
        if (at != last_bad) out->bad_simds++;
        last_bad = at;
      }
    }
  }
  // accuracy: the raw results of the first wave of workgroup 0 that holds the consensus.  If none of the four does,
  // the mismatches above have failed the run already.
  for (int w = 0; holder >= 0 && w < kBlock / 64; ++w) {
    if (std::memcmp(trans + w * stride, trans + holder * stride, 64 * sizeof(uint32_t)) != 0) continue;
    for (int r = 0; r < a.rounds; ++r) {
      for (int op = 0; op < 5; ++op) {
        for (int lane = 0; lane < 64; ++lane) {
          const float got = ref::f32_of(trans_raw[((static_cast<size_t>(w) * a.rounds + r) * 5 + op) * 64 + lane]);
          const double want = ref::trans_ref(op, ref::trans_operand(a.seed, r, lane, op));
          if (!(ref::ulps_off(got, want) <= ref::kTransUlps[op])) out->trans_out_of_bound++;
        }
      }
    }
    break;
  }
}

struct RateRun {
  const ValuArgs& a;
  const ValuExtras& x;
  int grid, waves;
  const Events& ev;
  uint32_t* ends;
  RateBin* bins;
  const bgc_valu_rate_plant* d_plants;
  const bgc_valu_delay_plant* d_delays;
  int* d_cu_keys;
  bgc_valu_result* out;
};

// One rate class: warm-up, the timed launch, its end digests against the host's (trans: against the consensus).
template <int kClass>
int rate_class(const RateRun& r, uint32_t a_bits, uint32_t b_bits, double ops_per_step) {
  const int iters = r.a.rate_iters;
  hipLaunchKernelGGL((valu_rate<kClass, false>), dim3(r.grid), dim3(kBlock), 0, nullptr, r.a.seed, std::min(iters, 64), a_bits, b_bits, r.ends,
                     r.bins);
  float ms = 0.f;
  if (timed(r.ev, &ms, [&] {
        if (r.x.n_rate > 0 || r.x.n_delay > 0 || r.x.want_data) {
          hipLaunchKernelGGL((valu_rate<kClass, true, RateExtras>), dim3(r.grid), dim3(kBlock), 0, nullptr, r.a.seed, iters, a_bits, b_bits,
                             r.ends, r.bins, RateExtras{r.d_plants, r.x.n_rate, r.d_delays, r.x.n_delay, r.x.want_data ? r.x.wave : -1, r.d_cu_keys});
        } else {
          hipLaunchKernelGGL((valu_rate<kClass, true>), dim3(r.grid), dim3(kBlock), 0, nullptr, r.a.seed, iters, a_bits, b_bits, r.ends, r.bins);
        }
      }) != 0) {
    return 1;
  }
  std::vector<uint32_t> ends(static_cast<size_t>(r.waves) * 64);
  HIP_TRY(hipMemcpy(ends.data(), r.ends, ends.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  uint32_t expect[64];
  bool ok = true;
  if (kClass == BGC_VALU_RATE_TRANS) {
    const int holder = consensus(ends.data(), r.waves, 64);
    ok = holder >= 0;
    if (ok) std::memcpy(expect, ends.data() + static_cast<size_t>(holder) * 64, sizeof(expect));
  } else {
    for (int lane = 0; lane < 64; ++lane) expect[lane] = ref::rate_expected(kClass, r.a.seed, iters, lane);
  }
  for (int w = 0; ok && w < r.waves; ++w) ok = std::memcmp(ends.data() + static_cast<size_t>(w) * 64, expect, sizeof(expect)) == 0;
  if (!ok) r.out->rate_ok = 0;
  const double ops = static_cast<double>(r.waves) * 64 * ref::kChains * iters * ops_per_step;
  r.out->rate[kClass] = tera_per_s(ops, ms);
  r.out->rate_ms[kClass] = ms;
  r.out->elapsed_ms += ms;
  return 0;
}

int valu_run(int device, const ValuArgs& a, const ValuExtras& x, bgc_valu_result* out) {
  if (!(out && args_ok(a) && extras_ok(a, x))) {
    g_last_error = "invalid arguments";
    return 1;
  }
  std::memset(out, 0, sizeof(*out));
  out->first_bad_cu_key = out->first_bad_simd = out->first_bad_lane = out->first_bad_class = out->slowest_cu_key = -1;
  out->rate_ok = 1;
  HIP_TRY(hipSetDevice(device));
  const int cus = cu_count(device), grid = cus * a.waves_per_simd, waves = grid * (kBlock / 64);
  out->cus = cus;
  if (any_beyond(x.check, x.n_check, &bgc_valu_plant::wave, waves) || any_beyond(x.rate, x.n_rate, &bgc_valu_rate_plant::wave, waves) ||
      any_beyond(x.delays, x.n_delay, &bgc_valu_delay_plant::wave, waves) || (x.want_data && x.wave >= waves)) {
    return refuse(kWaveBeyond);
  }
  const size_t n_digests = static_cast<size_t>(waves) * ref::kClasses * 64, n_trans = static_cast<size_t>(kBlock / 64) * a.rounds * 5 * 64;
  const size_t n_raw = static_cast<size_t>(a.rounds) * ref::kRoundWords * 64;
  DeviceBuffer digests, where, trans_raw, raw, rate_cu_keys, ends, bins, d_check, d_rate, d_delays;
  HIP_TRY(digests.alloc(n_digests * sizeof(uint32_t), true));
  HIP_TRY(where.alloc(static_cast<size_t>(waves) * sizeof(int2), true));
  HIP_TRY(trans_raw.alloc(n_trans * sizeof(uint32_t), true));
  HIP_TRY(ends.alloc(static_cast<size_t>(waves) * 64 * sizeof(uint32_t), true));
  HIP_TRY(bins.alloc(BGC_DIAG_MAX_CU_KEYS * sizeof(RateBin), true));
  if (x.want_data) {
    HIP_TRY(raw.alloc(n_raw * sizeof(uint32_t), true));
    HIP_TRY(rate_cu_keys.alloc(ref::kRateClasses * sizeof(int), true));
  }
  if (upload_plants(d_check, x.check, x.n_check) != 0 || upload_plants(d_rate, x.rate, x.n_rate) != 0 ||
      upload_plants(d_delays, x.delays, x.n_delay) != 0) {
    return 1;
  }
  Events ev;
  HIP_TRY(ev.create());
  float ms_check = 0.f;
  if (timed(ev, &ms_check, [&] {
        if (x.n_check > 0 || x.want_data) {
          hipLaunchKernelGGL((valu_check<CheckExtras>), dim3(grid), dim3(kBlock), 0, nullptr, a.seed, a.rounds, digests.as<uint32_t>(),
                             where.as<int2>(), trans_raw.as<uint32_t>(),
                             CheckExtras{d_check.as<const bgc_valu_plant>(), x.n_check, x.want_data ? x.wave : -1, raw.as<uint32_t>()});
        } else {
          hipLaunchKernelGGL((valu_check<>), dim3(grid), dim3(kBlock), 0, nullptr, a.seed, a.rounds, digests.as<uint32_t>(), where.as<int2>(),
                             trans_raw.as<uint32_t>());
        }
      }) != 0) {
    return 1;
  }
  std::vector<uint32_t> h_digests(n_digests), h_trans(n_trans);
  std::vector<int2> h_where(static_cast<size_t>(waves));
  HIP_TRY(hipMemcpy(h_digests.data(), digests.p, n_digests * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_where.data(), where.p, h_where.size() * sizeof(int2), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_trans.data(), trans_raw.p, n_trans * sizeof(uint32_t), hipMemcpyDeviceToHost));
  out->values_checked = static_cast<uint64_t>(waves) * 64 * a.rounds * ref::kRoundWords;
  out->elapsed_ms = ms_check;
  referee(a, waves, h_digests, h_where, h_trans, out);
  if (x.want_data) {
    std::memset(x.data, 0, sizeof(*x.data));
    x.data->cu_key = h_where[static_cast<size_t>(x.wave)].x;
    x.data->simd = h_where[static_cast<size_t>(x.wave)].y;
    std::memcpy(x.data->digests, h_digests.data() + static_cast<size_t>(x.wave) * ref::kClasses * 64, sizeof(x.data->digests));
    HIP_TRY(hipMemcpy(x.data->raw, raw.p, n_raw * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  const RateRun r{a, x, grid, waves, ev, ends.as<uint32_t>(), bins.as<RateBin>(), d_rate.as<const bgc_valu_rate_plant>(),
                  d_delays.as<const bgc_valu_delay_plant>(), rate_cu_keys.as<int>(), out};
  const uint32_t minus_one = ref::bits_of(-1.0f), b = ref::bits_of(static_cast<float>(ref::kFmaB));
  const uint32_t minus_one_h = ref::f16_from_double(-1.0) * 0x10001u, b_h = ref::f16_from_double(ref::kFmaB) * 0x10001u;
  if (rate_class<BGC_VALU_RATE_FP32>(r, minus_one, b, 4) != 0 || rate_class<BGC_VALU_RATE_FP16>(r, minus_one_h, b_h, 4) != 0 ||
      rate_class<BGC_VALU_RATE_FP64>(r, minus_one, b, 2) != 0 || rate_class<BGC_VALU_RATE_INT32>(r, ref::kLcgA, ref::kLcgC, 2) != 0 ||
      rate_class<BGC_VALU_RATE_TRANS>(r, ref::bits_of(ref::kExpScale), 0, 1) != 0) {
    return 1;
  }
  if (x.want_data) HIP_TRY(hipMemcpy(x.data->rate_cu_key, rate_cu_keys.p, sizeof(x.data->rate_cu_key), hipMemcpyDeviceToHost));
  std::vector<RateBin> h_bins(BGC_DIAG_MAX_CU_KEYS);
  HIP_TRY(hipMemcpy(h_bins.data(), bins.p, h_bins.size() * sizeof(RateBin), hipMemcpyDeviceToHost));
  TimingFold fold;  // of the mean ticks of a rate wave on a CU, the five timed launches together
  for (int k = 0; k < BGC_DIAG_MAX_CU_KEYS; ++k) fold.add(k, h_bins[static_cast<size_t>(k)].ticks, h_bins[static_cast<size_t>(k)].n, 1.0);
  out->slowest_cu_key = fold.slowest_key;
  out->cu_balance = fold.balance();
  return 0;
}

}  // namespace

extern "C" {

int bgc_diag_valu(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, bgc_valu_result* out) {
  return valu_run(device, {waves_per_simd, rounds, rate_iters, seed}, ValuExtras{}, out);
}

int bgc_diag_valu_planted(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, const bgc_valu_plant* check, int n_check,
                          const bgc_valu_rate_plant* rate, int n_rate, bgc_valu_result* out) {
  ValuExtras x;
  x.check = check;
  x.n_check = n_check;
  x.rate = rate;
  x.n_rate = n_rate;
  return valu_run(device, {waves_per_simd, rounds, rate_iters, seed}, x, out);
}

int bgc_diag_valu_delayed(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, const bgc_valu_delay_plant* delays, int n,
                          bgc_valu_result* out) {
  ValuExtras x;
  x.delays = delays;
  x.n_delay = n;
  return valu_run(device, {waves_per_simd, rounds, rate_iters, seed}, x, out);
}

int bgc_diag_valu_data(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, int wave, const bgc_valu_plant* check,
                       int n_check, const bgc_valu_rate_plant* rate, int n_rate, const bgc_valu_delay_plant* delays, int n_delay,
                       bgc_valu_wave* data, bgc_valu_result* out) {
  ValuExtras x;
  x.check = check;
  x.n_check = n_check;
  x.rate = rate;
  x.n_rate = n_rate;
  x.delays = delays;
  x.n_delay = n_delay;
  x.want_data = true;
  x.wave = wave;
  x.data = data;
  return valu_run(device, {waves_per_simd, rounds, rate_iters, seed}, x, out);
}

int bgc_diag_valu_expected(uint32_t seed, int rounds, bgc_valu_wave* data) {
  if (!data || !rounds_ok(rounds)) {
    g_last_error = "invalid arguments";
    return 1;
  }
  std::memset(data, 0, sizeof(*data));
  data->cu_key = data->simd = -1;
  for (int& key : data->rate_cu_key) key = -1;
  ref::expected(seed, rounds, data->raw, &data->digests[0][0]);
  return 0;
}

}  // extern "C"
