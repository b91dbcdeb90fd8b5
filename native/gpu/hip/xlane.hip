// The cross-lane paths: the per-SIMD check of DPP, the half-wave swaps, the LDS crossbar's permutes and the moves
// between vector lanes and scalar registers, and the cross-lane rates (bgc_diag_xlane).
//
//  * No wave waits for another, there is no barrier and no LDS allocation (the ds_ permutes use the crossbar, not the
//    memory), and every address is a function of blockIdx, threadIdx, loop counters and arguments checked on the
//    host: nothing read from memory is used as an index.  The buffers are sized exactly for the launch: waves * 8 * 64
//    digests, waves (CU key, SIMD) pairs, waves * 64 end digests of a rate launch.
//  * xlane_check: cus * waves_per_simd workgroups of 256 threads, normally one wave per SIMD of a CU; that is
//    observed (each wave records cu_key() and simd_id()), not promised.  Every wave runs the rounds of the sequence
//    that xlane_ref.h's tables hold, folds each result word into the lane's digest of its class and writes the
//    digests with plain vector stores; results that live in scalar registers (readlane, readfirstlane, the ballot)
//    are copied to vector registers first.  It compares nothing: the host (referee(), below) recomputes every digest
//    with xlane_ref.h's model.  All eight classes are exact.
//  * How the instructions are written.  v_mov_b32_dpp of the row, wave and mask classes: __builtin_amdgcn_update_dpp
//    with the table entry as immediates, its result made opaque at once so that the compiler cannot fuse the move
//    into the digest's first v_xor.  The alu class: v_add_u32_dpp and v_min_u32_dpp as text, since the compiler's
//    fusion is not promised.  The swaps, the ds_ permutes, v_readlane, v_readfirstlane, the ballot and v_mbcnt:
//    builtins, so the compiler pads their hazards and counts their waits.  v_writelane_b32 has no builtin and is
//    text, its lane select in m0: two different scalar registers in one VOP3 exceed gfx950's constant-bus limit.  The
//    exec class: one statement each that saves EXEC, sets the mask, issues the instruction, waits for it (s_waitcnt
//    lgkmcnt(0) for the ds_ one) and restores EXEC; a C++ `if` could be if-converted and run under full EXEC.
//  * Hazards inside the text, which the compiler does not see: a VALU write of a register needs 2 wait states before
//    a DPP instruction reads it and 1 before v_readfirstlane; a DPP instruction needs 5 after a VALU write of EXEC
//    (here a scalar write, kept to the same distance); a lane select needs 4 after its write.  Every statement
//    opens with the s_nop that covers its case; the prefix scan pads each step whose DPP operand the step before
//    wrote.
//  * xlane_rate<class, timed>: the same grid, `iters` steps of 8 chains per lane, four steps a trip.  Each wave times
//    its loop on the 100 MHz constant clock into its CU's bin and writes one end digest per lane.  Every step is a
//    permutation of the wave, so the host raises the step's source map to the power `iters` and compares.
//  * Checked in the gfx950 assembly (-save-temps).  xlane_check holds, per round: the 24 v_mov_b32_dpp of the row, wave
//    and mask tables with exactly the tables' controls, masks and bound_ctrl, none fused into another instruction; the
//    v_add_u32_dpp, the v_min_u32_dpp and the scan's seven v_add_u32_dpp as written; one v_permlane16_swap_b32 and one
//    v_permlane32_swap_b32; two ds_bpermute_b32, one ds_permute_b32 and three ds_swizzle_b32 under the compiler's
//    counted lgkmcnt waits, plus the exec class's ds_bpermute_b32 with its own lgkmcnt(0); one v_readlane_b32, two
//    v_readfirstlane_b32 (the builtin's and the exec class's), one v_writelane_b32, the ballot's v_cmp, v_mbcnt_lo and
//    v_mbcnt_hi; the exec class's two v_mov_b32_dpp wave_ror:1, one with bound_ctrl.  A rate loop's trip is 32
//    v_mov_b32_dpp row_ror:1, 16 v_permlane32_swap_b32, 32 ds_bpermute_b32 or 32 ds_swizzle_b32, the ds_ ones with
//    s_waitcnt lgkmcnt(7) between them, so 8 stay in flight; a second loop of one step takes the iterations left over.
//    No scratch and no spills in any kernel: 60 VGPRs in xlane_check (96 with the test plants), at most 12 in a rate
//    kernel (17 with plants).
//  * Measured on the MI355X at the defaults, 2 waves per SIMD and 16384 iterations (profiles/xlane_diag/rates.json),
//    in 10^12 lane-moves per second: 31.6-33.7 v_mov_b32_dpp, 33.1-35.2 v_permlane32_swap_b32, 6.2-6.5
//    ds_bpermute_b32, 16.9-17.5 ds_swizzle_b32; 8 waves per SIMD reach 35.4-36.3, 37.0-37.6, 6.5 and 18.4-18.6.  The
//    first run on the device corrected two statements of the model, both about row_bcast on rows that have no source
//    row (gpu_diag.h, docs/ARCHITECTURE.md).
#include <algorithm>
#include <cstring>
#include <numeric>
#include <utility>
#include <vector>

#include "diag_common.h"
#include "xlane_ref.h"

namespace {

using namespace bgc_diag;
namespace ref = bgc_xlane;

// v_mov_b32_dpp by one entry of xlane_ref.h's tables
template <int kCtrl, int kRowMask, int kBankMask, int kBoundCtrl>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t old, uint32_t src) {
  return static_cast<uint32_t>(
      __builtin_amdgcn_update_dpp(static_cast<int>(old), static_cast<int>(src), kCtrl, kRowMask, kBankMask, kBoundCtrl != 0));
}
template <class Table, int I>
__device__ __forceinline__ uint32_t dpp_step(uint32_t old, uint32_t src) {
  constexpr ref::Dpp s = Table::steps[I];
  uint32_t r = dpp_mov<s.ctrl, s.row_mask, s.bank_mask, s.bound_ctrl>(old, src);
  asm volatile("" : "+v"(r));  // a move of its own: not fused into the instruction that reads it
  return r;
}
template <class Table, class Put, int... I>
__device__ __forceinline__ void dpp_steps(uint32_t old, uint32_t src, Put&& put, std::integer_sequence<int, I...>) {
  (put(I, dpp_step<Table, I>(old, src)), ...);
}

// The eight classes of one round for one lane, the words of a class in order.  The DPP modifiers in text repeat
// xlane_ref.h's entries: kAluAdd, kAluMin, ScanSteps, kExecKeep, kExecZero.
template <class Put>
__device__ __forceinline__ void xlane_round(uint32_t seed, int round, int lane, Put&& put) {
  auto w = [&](int cls, int k) { return ref::operand(seed, cls, round, k, lane); };
  {
    const uint32_t src = w(BGC_XLANE_ROW, 0), old = w(BGC_XLANE_ROW, 1);
    dpp_steps<ref::RowSteps>(old, src, [&](int i, uint32_t v) { put(BGC_XLANE_ROW, i, v); }, std::make_integer_sequence<int, ref::RowSteps::kCount>{});
  }
  {
    const uint32_t src = w(BGC_XLANE_WAVE, 0), old = w(BGC_XLANE_WAVE, 1);
    dpp_steps<ref::WaveSteps>(old, src, [&](int i, uint32_t v) { put(BGC_XLANE_WAVE, i, v); }, std::make_integer_sequence<int, ref::WaveSteps::kCount>{});
  }
  {
    const uint32_t src = w(BGC_XLANE_MASK, 0), old = w(BGC_XLANE_MASK, 1);
    dpp_steps<ref::MaskSteps>(old, src, [&](int i, uint32_t v) { put(BGC_XLANE_MASK, i, v); }, std::make_integer_sequence<int, ref::MaskSteps::kCount>{});
  }
  {
    const uint32_t a = w(BGC_XLANE_ALU, 0), b = w(BGC_XLANE_ALU, 1), c = w(BGC_XLANE_ALU, 2);
    uint32_t sum = c, low = c, acc;
    asm volatile("s_nop 1\n\tv_add_u32_dpp %0, %1, %2 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(sum) : "v"(a), "v"(b));
    asm volatile("s_nop 1\n\tv_min_u32_dpp %0, %1, %2 row_ror:8 row_mask:0xf bank_mask:0xf" : "+v"(low) : "v"(a), "v"(b));
    asm volatile(
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %1, %1 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_u32_dpp %0, %1, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_add_u32_dpp %0, %1, %0 row_shr:3 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xe\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xc\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf"
        : "=&v"(acc)
        : "v"(c));
    put(BGC_XLANE_ALU, 0, sum);
    put(BGC_XLANE_ALU, 1, low);
    put(BGC_XLANE_ALU, 2, acc);
  }
  {
    const uint32_t x = w(BGC_XLANE_SWAP, 0), y = w(BGC_XLANE_SWAP, 1);
    const auto s16 = __builtin_amdgcn_permlane16_swap(x, y, false, false);
    put(BGC_XLANE_SWAP, 0, s16[0]);
    put(BGC_XLANE_SWAP, 1, s16[1]);
    const auto s32 = __builtin_amdgcn_permlane32_swap(x, y, false, false);
    put(BGC_XLANE_SWAP, 2, s32[0]);
    put(BGC_XLANE_SWAP, 3, s32[1]);
  }
  {
    const int src = static_cast<int>(w(BGC_XLANE_LDS, 0));
    put(BGC_XLANE_LDS, 0, __builtin_amdgcn_ds_bpermute(static_cast<int>(ref::gather_addr(w(BGC_XLANE_LDS, 1))), src));
    put(BGC_XLANE_LDS, 1, __builtin_amdgcn_ds_bpermute(static_cast<int>(ref::rotate_addr(seed, round, lane)), src));
    put(BGC_XLANE_LDS, 2, __builtin_amdgcn_ds_permute(static_cast<int>(ref::scatter_addr(seed, round, lane)), src));
    put(BGC_XLANE_LDS, 3, __builtin_amdgcn_ds_swizzle(src, ref::kSwizzle[0]));
    put(BGC_XLANE_LDS, 4, __builtin_amdgcn_ds_swizzle(src, ref::kSwizzle[1]));
    put(BGC_XLANE_LDS, 5, __builtin_amdgcn_ds_swizzle(src, ref::kSwizzle[2]));
  }
  {
    const uint32_t a = w(BGC_XLANE_LANE, 0), b = w(BGC_XLANE_LANE, 1);
    uint32_t c = w(BGC_XLANE_LANE, 2);
    put(BGC_XLANE_LANE, 0, __builtin_amdgcn_readlane(static_cast<int>(a), ref::readlane_select(seed, round)));
    put(BGC_XLANE_LANE, 1, __builtin_amdgcn_readfirstlane(static_cast<int>(b)));
    const uint32_t value = ref::writelane_value(seed, round);
    const int select = ref::writelane_select(seed, round);
    uint32_t m0_saved;  // m0 is reserved: it leaves the statement as it entered
    asm volatile("s_mov_b32 %1, m0\n\ts_mov_b32 m0, %3\n\ts_nop 3\n\tv_writelane_b32 %0, %2, m0\n\ts_mov_b32 m0, %1"
                 : "+v"(c), "=&s"(m0_saved)
                 : "s"(value), "s"(select));
    put(BGC_XLANE_LANE, 2, c);
    const uint64_t ballot = __builtin_amdgcn_ballot_w64((a & 1) != 0);
    const uint32_t lo = static_cast<uint32_t>(ballot), hi = static_cast<uint32_t>(ballot >> 32);
    put(BGC_XLANE_LANE, 3, lo);
    put(BGC_XLANE_LANE, 4, hi);
    put(BGC_XLANE_LANE, 5, __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0)));
  }
  {
    const uint32_t src = w(BGC_XLANE_EXEC, 0), old = w(BGC_XLANE_EXEC, 1), addr = ref::gather_addr(w(BGC_XLANE_EXEC, 2));
    const uint64_t m = ref::exec_mask(seed, round);
    uint64_t saved;
    uint32_t keep = old, zero = old, gather = old, first;
    asm volatile(
        "s_mov_b64 %1, exec\n\ts_mov_b64 exec, %3\n\ts_nop 4\n\t"
        "v_mov_b32_dpp %0, %2 wave_ror:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_mov_b64 exec, %1"
        : "+v"(keep), "=&s"(saved)
        : "v"(src), "s"(m));
    asm volatile(
        "s_mov_b64 %1, exec\n\ts_mov_b64 exec, %3\n\ts_nop 4\n\t"
        "v_mov_b32_dpp %0, %2 wave_ror:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_mov_b64 exec, %1"
        : "+v"(zero), "=&s"(saved)
        : "v"(src), "s"(m));
    asm volatile(
        "s_mov_b64 %1, exec\n\ts_mov_b64 exec, %4\n\ts_nop 4\n\t"
        "ds_bpermute_b32 %0, %2, %3\n\ts_waitcnt lgkmcnt(0)\n\t"
        "s_mov_b64 exec, %1"
        : "+v"(gather), "=&s"(saved)
        : "v"(addr), "v"(src), "s"(m));
    asm volatile(
        "s_mov_b64 %1, exec\n\ts_mov_b64 exec, %3\n\ts_nop 4\n\t"
        "v_readfirstlane_b32 %0, %2\n\t"
        "s_mov_b64 exec, %1"
        : "=&s"(first), "=&s"(saved)
        : "v"(src), "s"(m));
    put(BGC_XLANE_EXEC, 0, keep);
    put(BGC_XLANE_EXEC, 1, zero);
    put(BGC_XLANE_EXEC, 2, gather);
    put(BGC_XLANE_EXEC, 3, first);
  }
}

// Test plants and the generated-data copy (gpu_diag.h).  Both kernels end in a pack `Extras... extras`: empty in the
// production instantiations, which take the empty tap() below and no after_loop().
struct CheckExtras {  // in device memory
  const bgc_xlane_plant* p = nullptr;
  int n = 0;
  int dump_wave = -1;
  uint32_t* raw = nullptr;  // rounds * 47 * 64 words
};
struct RateExtras {
  const bgc_xlane_rate_plant* p = nullptr;
  int n = 0;
  const bgc_xlane_delay_plant* d = nullptr;
  int nd = 0;
  int dump_wave = -1;
  int* cu_keys = nullptr;  // of dump_wave, one per rate class
};

// a result word on its way into the digest
__device__ __forceinline__ uint32_t tap(uint32_t v, int /*wave*/, int /*cls*/, int /*round*/, int /*lane*/, int /*word*/) { return v; }
__device__ __forceinline__ uint32_t tap(uint32_t v, int wave, int cls, int round, int lane, int word, const CheckExtras& x) {
  for (int j = 0; j < x.n; ++j) {
    const bgc_xlane_plant p = x.p[j];
    if ((p.wave == BGC_PLANT_ALL_WAVES || p.wave == wave) && p.cls == cls && p.round == round && p.lane == lane && p.op == word) v ^= p.xor_mask;
  }
  if (wave == x.dump_wave) x.raw[(round * ref::kRoundWords + ref::word_base(cls) + word) * 64 + lane] = v;
  return v;
}

template <class... Extras>
__global__ __launch_bounds__(kBlock) void xlane_check(uint32_t seed, int rounds, uint32_t* __restrict__ digests, int2* __restrict__ where,
                                                      Extras... extras) {
  const int lane = threadIdx.x & 63, wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  uint32_t d[ref::kClasses];
#pragma unroll
  for (int c = 0; c < ref::kClasses; ++c) d[c] = ref::digest_start(c);
#pragma unroll 1
  for (int r = 0; r < rounds; ++r) {
    xlane_round(seed, r, lane, [&](int cls, int word, uint32_t v) {
      v = tap(v, wave, cls, r, lane, word, extras...);
      d[cls] = ref::mix32(d[cls] ^ v);
    });
  }
#pragma unroll
  for (int c = 0; c < ref::kClasses; ++c) digests[(wave * ref::kClasses + c) * 64 + lane] = d[c];
  if (lane == 0) where[wave] = int2{static_cast<int>(cu_key()), static_cast<int>(simd_id())};
}

// one step of a rate class on the lane's 8 chains (xlane_ref.h's rate_source() is the host's)
template <int kClass>
__device__ __forceinline__ void rate_step(uint32_t (&x)[ref::kChains], int rotate_addr) {
  if constexpr (kClass == BGC_XLANE_RATE_DPP) {
    constexpr ref::Dpp s = ref::kRateDpp;
#pragma unroll
    for (int c = 0; c < ref::kChains; ++c) x[c] = dpp_mov<s.ctrl, s.row_mask, s.bank_mask, s.bound_ctrl>(x[c], x[c]);
  } else if constexpr (kClass == BGC_XLANE_RATE_SWAP) {
#pragma unroll
    for (int c = 0; c < ref::kChains; c += 2) {
      const auto s = __builtin_amdgcn_permlane32_swap(x[c], x[c + 1], false, false);
      x[c] = s[0];
      x[c + 1] = s[1];
    }
  } else if constexpr (kClass == BGC_XLANE_RATE_BPERMUTE) {
#pragma unroll
    for (int c = 0; c < ref::kChains; ++c) x[c] = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(rotate_addr, static_cast<int>(x[c])));
  } else {
#pragma unroll
    for (int c = 0; c < ref::kChains; ++c) x[c] = static_cast<uint32_t>(__builtin_amdgcn_ds_swizzle(static_cast<int>(x[c]), ref::kRateSwizzle));
  }
}

// after the loop: the value plants, where the dumped wave runs, then the wait for the largest `ticks` that names this wave
__device__ __forceinline__ void after_loop(uint32_t (&x)[ref::kChains], int cls, int wave, int lane, const RateExtras& e) {
  for (int j = 0; j < e.n; ++j) {
    const bgc_xlane_rate_plant p = e.p[j];
    if ((p.wave == BGC_PLANT_ALL_WAVES || p.wave == wave) && p.cls == cls && p.lane == lane) {
#pragma unroll
      for (int c = 0; c < ref::kChains; ++c) {
        if (c == p.chain) x[c] ^= p.xor_mask;
      }
    }
  }
  if (wave == e.dump_wave && lane == 0) e.cu_keys[cls] = static_cast<int>(cu_key());
  uint32_t ticks = 0;
  for (int j = 0; j < e.nd; ++j) {
    const bgc_xlane_delay_plant p = e.d[j];
    if ((p.wave == BGC_PLANT_ALL_WAVES || p.wave == wave) && p.cls == cls) ticks = max(ticks, p.ticks);
  }
  wait_ticks(__builtin_amdgcn_readfirstlane(ticks));  // the same in every lane of the wave
}

template <int kClass, bool kTimed, class... Extras>
__global__ __launch_bounds__(kBlock) void xlane_rate(uint32_t seed, int iters, uint32_t* __restrict__ ends, RateBin* __restrict__ bins,
                                                     Extras... extras) {
  const int lane = threadIdx.x & 63, wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const int rotate_addr = static_cast<int>(ref::rate_rotate_addr(lane));
  uint32_t x[ref::kChains];
#pragma unroll
  for (int c = 0; c < ref::kChains; ++c) x[c] = ref::rate_fill(seed, lane, c);
  uint64_t t0 = 0, t1 = 0;
  if constexpr (kTimed) {
    t0 = wall_clock64();
    asm volatile("" ::"s"(t0));  // wait for the clock here, not inside the loop, where it would share lgkmcnt with the permutes
  }
  int it = 0;
#pragma unroll 1
  for (; it + 4 <= iters; it += 4) {  // four steps per trip: the loop control is small beside the body
    rate_step<kClass>(x, rotate_addr);
    rate_step<kClass>(x, rotate_addr);
    rate_step<kClass>(x, rotate_addr);
    rate_step<kClass>(x, rotate_addr);
  }
#pragma unroll 1
  for (; it < iters; ++it) rate_step<kClass>(x, rotate_addr);
#pragma unroll
  for (int c = 0; c < ref::kChains; ++c) asm volatile("" : "+v"(x[c]));  // every chain has ended before the clock is read
  if constexpr (sizeof...(Extras) > 0) after_loop(x, kClass, wave, lane, extras...);
  if constexpr (kTimed) t1 = wall_clock64();
  uint32_t d = ref::rate_digest_start(kClass);
#pragma unroll
  for (int c = 0; c < ref::kChains; ++c) d = ref::mix32(d ^ x[c]);
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

struct XlaneArgs {
  int waves_per_simd, rounds, rate_iters;
  uint32_t seed;
};

// what the test-only entries add to a run; all empty in bgc_diag_xlane
struct XlaneExtras {
  const bgc_xlane_plant* check = nullptr;
  int n_check = 0;
  const bgc_xlane_rate_plant* rate = nullptr;
  int n_rate = 0;
  const bgc_xlane_delay_plant* delays = nullptr;
  int n_delay = 0;
  bool want_data = false;
  int wave = 0;
  bgc_xlane_wave* data = nullptr;
};

bool rounds_ok(int rounds) { return rounds >= 1 && rounds <= 64; }

bool args_ok(const XlaneArgs& a) {
  return a.waves_per_simd >= 1 && a.waves_per_simd <= 8 && rounds_ok(a.rounds) && a.rate_iters >= 1 && a.rate_iters <= (1 << 16);
}

bool extras_ok(const XlaneArgs& a, const XlaneExtras& x) {
  if (!plant_list_ok(x.check, x.n_check) || !plant_list_ok(x.rate, x.n_rate) || !plant_list_ok(x.delays, x.n_delay)) return false;
  const bool check_ok = std::all_of(x.check, x.check + x.n_check, [&](const bgc_xlane_plant& p) {
    return p.wave >= BGC_PLANT_ALL_WAVES && p.cls >= 0 && p.cls < ref::kClasses && p.round >= 0 && p.round < a.rounds && p.lane >= 0 &&
           p.lane < 64 && p.op >= 0 && p.op < ref::class_words(p.cls) && p.xor_mask != 0;
  });
  const bool rate_ok = std::all_of(x.rate, x.rate + x.n_rate, [](const bgc_xlane_rate_plant& p) {
    return p.wave >= BGC_PLANT_ALL_WAVES && p.cls >= 0 && p.cls < ref::kRateClasses && p.lane >= 0 && p.lane < 64 && p.chain >= 0 &&
           p.chain < ref::kChains && p.xor_mask != 0;
  });
  const bool delays_ok = std::all_of(x.delays, x.delays + x.n_delay, [](const bgc_xlane_delay_plant& p) {
    return p.wave >= BGC_PLANT_ALL_WAVES && p.cls >= 0 && p.cls < ref::kRateClasses && p.ticks > 0 && p.ticks <= BGC_DIAG_MAX_DELAY_TICKS;
  });
  return check_ok && rate_ok && delays_ok && (!x.want_data || (x.data && x.wave >= 0));
}

// The host's verdict on the check launch: digests[(wave * 8 + class) * 64 + lane], where[wave] = (CU key, SIMD).
void referee(const XlaneArgs& a, int waves, const std::vector<uint32_t>& digests, const std::vector<int2>& where, bgc_xlane_result* out) {
  std::vector<uint32_t> expect(ref::kClasses * 64);
  ref::expected(a.seed, a.rounds, nullptr, expect.data());
  const size_t stride = ref::kClasses * 64;
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
      const uint32_t* want = expect.data() + c * 64;
      const uint32_t* got = digests.data() + w * stride + static_cast<size_t>(c) * 64;
      for (int lane = 0; lane < 64; ++lane) {
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
}

struct RateRun {
  const XlaneArgs& a;
  const XlaneExtras& x;
  int grid, waves;
  const Events& ev;
  uint32_t* ends;
  RateBin* bins;
  const bgc_xlane_rate_plant* d_plants;
  const bgc_xlane_delay_plant* d_delays;
  int* d_cu_keys;
  bgc_xlane_result* out;
};

// One rate class: warm-up, the timed launch, every wave's end digests against the host's.
template <int kClass>
int rate_class(const RateRun& r) {
  const int iters = r.a.rate_iters;
  hipLaunchKernelGGL((xlane_rate<kClass, false>), dim3(r.grid), dim3(kBlock), 0, nullptr, r.a.seed, std::min(iters, 64), r.ends, r.bins);
  float ms = 0.f;
  if (timed(r.ev, &ms, [&] {
        if (r.x.n_rate > 0 || r.x.n_delay > 0 || r.x.want_data) {
          hipLaunchKernelGGL((xlane_rate<kClass, true, RateExtras>), dim3(r.grid), dim3(kBlock), 0, nullptr, r.a.seed, iters, r.ends, r.bins,
                             RateExtras{r.d_plants, r.x.n_rate, r.d_delays, r.x.n_delay, r.x.want_data ? r.x.wave : -1, r.d_cu_keys});
        } else {
          hipLaunchKernelGGL((xlane_rate<kClass, true>), dim3(r.grid), dim3(kBlock), 0, nullptr, r.a.seed, iters, r.ends, r.bins);
        }
      }) != 0) {
    return 1;
  }
  std::vector<uint32_t> ends(static_cast<size_t>(r.waves) * 64);
  HIP_TRY(hipMemcpy(ends.data(), r.ends, ends.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  uint32_t expect[64];
  ref::rate_expected(kClass, r.a.seed, iters, expect);
  bool ok = true;
  for (int w = 0; ok && w < r.waves; ++w) ok = std::memcmp(ends.data() + static_cast<size_t>(w) * 64, expect, sizeof(expect)) == 0;
  if (!ok) r.out->rate_ok = 0;
  r.out->rate[kClass] = tera_per_s(static_cast<double>(r.waves) * 64 * ref::kChains * iters, ms);
  r.out->rate_ms[kClass] = ms;
  r.out->elapsed_ms += ms;
  return 0;
}

int xlane_run(int device, const XlaneArgs& a, const XlaneExtras& x, bgc_xlane_result* out) {
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
  if (any_beyond(x.check, x.n_check, &bgc_xlane_plant::wave, waves) || any_beyond(x.rate, x.n_rate, &bgc_xlane_rate_plant::wave, waves) ||
      any_beyond(x.delays, x.n_delay, &bgc_xlane_delay_plant::wave, waves) || (x.want_data && x.wave >= waves)) {
    return refuse(kWaveBeyond);
  }
  const size_t n_digests = static_cast<size_t>(waves) * ref::kClasses * 64;
  const size_t n_raw = static_cast<size_t>(a.rounds) * ref::kRoundWords * 64;
  DeviceBuffer digests, where, raw, rate_cu_keys, ends, bins, d_check, d_rate, d_delays;
  HIP_TRY(digests.alloc(n_digests * sizeof(uint32_t), true));
  HIP_TRY(where.alloc(static_cast<size_t>(waves) * sizeof(int2), true));
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
          hipLaunchKernelGGL((xlane_check<CheckExtras>), dim3(grid), dim3(kBlock), 0, nullptr, a.seed, a.rounds, digests.as<uint32_t>(),
                             where.as<int2>(), CheckExtras{d_check.as<const bgc_xlane_plant>(), x.n_check, x.want_data ? x.wave : -1, raw.as<uint32_t>()});
        } else {
          hipLaunchKernelGGL((xlane_check<>), dim3(grid), dim3(kBlock), 0, nullptr, a.seed, a.rounds, digests.as<uint32_t>(), where.as<int2>());
        }
      }) != 0) {
    return 1;
  }
  std::vector<uint32_t> h_digests(n_digests);
  std::vector<int2> h_where(static_cast<size_t>(waves));
  HIP_TRY(hipMemcpy(h_digests.data(), digests.p, n_digests * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_where.data(), where.p, h_where.size() * sizeof(int2), hipMemcpyDeviceToHost));
  out->values_checked = static_cast<uint64_t>(waves) * 64 * a.rounds * ref::kRoundWords;
  out->elapsed_ms = ms_check;
  referee(a, waves, h_digests, h_where, out);
  if (x.want_data) {
    std::memset(x.data, 0, sizeof(*x.data));
    x.data->cu_key = h_where[static_cast<size_t>(x.wave)].x;
    x.data->simd = h_where[static_cast<size_t>(x.wave)].y;
    std::memcpy(x.data->digests, h_digests.data() + static_cast<size_t>(x.wave) * ref::kClasses * 64, sizeof(x.data->digests));
    HIP_TRY(hipMemcpy(x.data->raw, raw.p, n_raw * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  const RateRun r{a, x, grid, waves, ev, ends.as<uint32_t>(), bins.as<RateBin>(), d_rate.as<const bgc_xlane_rate_plant>(),
                  d_delays.as<const bgc_xlane_delay_plant>(), rate_cu_keys.as<int>(), out};
  if (rate_class<BGC_XLANE_RATE_DPP>(r) != 0 || rate_class<BGC_XLANE_RATE_SWAP>(r) != 0 || rate_class<BGC_XLANE_RATE_BPERMUTE>(r) != 0 ||
      rate_class<BGC_XLANE_RATE_SWIZZLE>(r) != 0) {
    return 1;
  }
  if (x.want_data) HIP_TRY(hipMemcpy(x.data->rate_cu_key, rate_cu_keys.p, sizeof(x.data->rate_cu_key), hipMemcpyDeviceToHost));
  std::vector<RateBin> h_bins(BGC_DIAG_MAX_CU_KEYS);
  HIP_TRY(hipMemcpy(h_bins.data(), bins.p, h_bins.size() * sizeof(RateBin), hipMemcpyDeviceToHost));
  TimingFold fold;  // of the mean ticks of a rate wave on a CU, the four timed launches together
  for (int k = 0; k < BGC_DIAG_MAX_CU_KEYS; ++k) fold.add(k, h_bins[static_cast<size_t>(k)].ticks, h_bins[static_cast<size_t>(k)].n, 1.0);
  out->slowest_cu_key = fold.slowest_key;
  out->cu_balance = fold.balance();
  return 0;
}

}  // namespace

extern "C" {

int bgc_diag_xlane(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, bgc_xlane_result* out) {
  return xlane_run(device, {waves_per_simd, rounds, rate_iters, seed}, XlaneExtras{}, out);
}

int bgc_diag_xlane_planted(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, const bgc_xlane_plant* check, int n_check,
                           const bgc_xlane_rate_plant* rate, int n_rate, bgc_xlane_result* out) {
  XlaneExtras x;
  x.check = check;
  x.n_check = n_check;
  x.rate = rate;
  x.n_rate = n_rate;
  return xlane_run(device, {waves_per_simd, rounds, rate_iters, seed}, x, out);
}

int bgc_diag_xlane_delayed(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, const bgc_xlane_delay_plant* delays, int n,
                           bgc_xlane_result* out) {
  XlaneExtras x;
  x.delays = delays;
  x.n_delay = n;
  return xlane_run(device, {waves_per_simd, rounds, rate_iters, seed}, x, out);
}

int bgc_diag_xlane_data(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed, int wave, const bgc_xlane_plant* check,
                        int n_check, const bgc_xlane_rate_plant* rate, int n_rate, const bgc_xlane_delay_plant* delays, int n_delay,
                        bgc_xlane_wave* data, bgc_xlane_result* out) {
  XlaneExtras x;
  x.check = check;
  x.n_check = n_check;
  x.rate = rate;
  x.n_rate = n_rate;
  x.delays = delays;
  x.n_delay = n_delay;
  x.want_data = true;
  x.wave = wave;
  x.data = data;
  return xlane_run(device, {waves_per_simd, rounds, rate_iters, seed}, x, out);
}

int bgc_diag_xlane_expected(uint32_t seed, int rounds, bgc_xlane_wave* data) {
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
