// Atomic read-modify-writes: the check of every global and LDS atomic form that jobs rely on, refereed by the host,
// and the atomic rates (bgc_diag_atomic).
//
//  * No wave waits for another and nothing is tried again: there is no spin-wait and no compare-and-swap loop in
//    this file.  Every wave issues a fixed number of atomics, and the kernels end whatever values come back.
//  * Every address is a function of blockIdx, threadIdx, loop counters and arguments checked on the host, with one
//    exception: a ticket that an atomic returned indexes its element's order array, and only after `ticket <
//    capacity`; one at or beyond it is counted and nothing is stored.  The buffers are sized by
//    atomic_ref.h's make_layout() for exactly the launch, and row_of() / word_at() / order_at() stay below those
//    sizes for every (wave, round, lane) of it.
//  * Agent scope and hipMalloc memory only: no system scope, no host-coherent memory.  Every result table, ballot,
//    order slot and CU key is written with vector stores.
//  * atomic_check: cus * wgs_per_cu workgroups of 256 threads.  Each wave runs the rounds of gpu_diag.h's "Atomics"
//    in placement OWN, then SHARED, then on the workgroup's LDS table, which is copied out after a barrier.  The
//    device compares nothing: the host (atomic_ref.h's judge()) recomputes the tables and checks the cas and the
//    tickets by their properties.
//  * atomic_rate<class, timed>: cus * 2 workgroups rounded up to a multiple of 8.  The 8 waves of equal number of 8
//    consecutive workgroups add to the same 64 rows of 256 bytes, row i mod 64 in iteration i, one wave instruction
//    per row (the shape of cdna_hip_programming.md, Guideline 12).  Each wave waits for its atomics, times its loop on
//    the constant clock into its XCC's bin, and the host compares the rows with their closed forms.
//  * Checked in the gfx950 disassembly: one instruction per atomic and no compare-and-swap loop: global_atomic_add,
//    _smin, _umax, _and, _or, _xor, _add_x2, _add_f32, _add_f64, _pk_add_bf16, _pk_add_f16, one global_atomic_cmpswap
//    per cas; ds_add_u32, ds_add_rtn_u32, ds_max_u32, ds_min_i32, ds_and_b32, ds_or_b32, ds_xor_b32, ds_add_f32 and
//    ds_cmpst_rtn_b32.  The float adds are the unsafeAtomicAdd forms: on device memory they are one instruction.
//  * Measured on the MI355X at the defaults, 2 workgroups per CU, 8 rounds and 4095 iterations
//    (profiles/atomic_diag/rates.json): 1.333-1.338 TB/s of added bytes for global_atomic_add_f32, 1.331-1.338 for
//    global_atomic_pk_add_bf16, 1.689-1.703 for global_atomic_add and 0.855-0.856 x 10^9 returning adds per second;
//    0.24-0.25 ms for atomic_check, 14.5 ms of kernels in all, 133-135 ms with the copies and the host referee.
//  * Where the integer atomics execute (in L2 or at the memory side) is not established, and nothing here rests on it.
#include <algorithm>
#include <cstring>
#include <vector>

#include "diag_common.h"  // first: atomic_ref.h uses the HIP runtime's qualifiers when it is compiled for the device

#include "atomic_ref.h"

namespace {

using namespace bgc_diag;
namespace ref = bgc_atomic;

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

#define BGC_RELAXED_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define BGC_RELAXED_WORKGROUP __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

// (a C cast: C++ has no named cast into another address space)
__device__ __forceinline__ void pk_add_bf16(uint32_t* p, uint32_t v) {
  __builtin_amdgcn_global_atomic_fadd_v2bf16((__attribute__((address_space(1))) bf16x2*)p, __builtin_bit_cast(bf16x2, v));
}
__device__ __forceinline__ void pk_add_f16(uint32_t* p, uint32_t v) {
  __builtin_amdgcn_global_atomic_fadd_v2f16((__attribute__((address_space(1))) f16x2*)p, __builtin_bit_cast(f16x2, v));
}

// How often a lane issues one atomic, and what is XORed into its operand word: once and nothing in production; the
// first plant that names the atomic in the planted instantiation (gpu_diag.h, bgc_atomic_plant).
struct Tap {
  int times;
  uint32_t mask;
};
__device__ __forceinline__ Tap tap(int /*placement*/, int /*cls*/, int /*op*/, uint32_t /*wave*/, int /*round*/, int /*lane*/) { return Tap{1, 0}; }
__device__ __forceinline__ Tap tap(int placement, int cls, int op, uint32_t wave, int round, int lane, const PlantList<bgc_atomic_plant>& x) {
  for (int j = 0; j < x.n; ++j) {
    const bgc_atomic_plant p = x.p[j];
    if (p.placement == placement && p.cls == cls && p.op == op && static_cast<uint32_t>(p.wave) == wave && p.round == round && p.lane == lane) {
      return Tap{p.times, p.xor_mask};
    }
  }
  return Tap{1, 0};
}

struct CheckArgs {
  ref::Layout L;
  uint32_t seed;
  uint32_t* table[2];
  unsigned long long* ballots;  // [OWN, SHARED, LDS][pair]
  uint32_t* order[3];
  int* cu_keys;
  unsigned* out_of_range;
};

template <class... Extras>
__global__ __launch_bounds__(kBlock) void atomic_check(CheckArgs a, Extras... extras) {
  __shared__ uint32_t lds[ref::kLdsWords * 128];  // [word][row][lane]
  const int lane = threadIdx.x & 63, rounds = a.L.rounds;
  const uint32_t wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  for (int i = threadIdx.x; i < ref::kLdsWords * 128; i += kBlock) lds[i] = ref::lds_init(i / 128);
  __syncthreads();
#pragma unroll 1
  for (int r = 0; r < rounds; ++r) {
    const uint32_t pair = wave * static_cast<uint32_t>(rounds) + static_cast<uint32_t>(r), id = pair * 64 + static_cast<uint32_t>(lane);
    // f(operand word with the mask in it), as often as the plants say
    auto issue = [&](int pl, int cls, int op, uint32_t raw, auto&& f) {
      const Tap t = tap(pl, cls, op, wave, r, lane, extras...);
      for (int i = 0; i < t.times; ++i) f(raw ^ t.mask);
    };
    // a drawn ticket is an index only below the capacity
    auto keep = [&](int order, uint32_t row, uint32_t drawn, uint32_t value) {
      if (drawn < a.L.order_cap[order]) {
        a.order[order][ref::order_at(a.L, order, row, lane) + drawn] = value + 1;
      } else {
        atomicAdd(a.out_of_range, 1u);
      }
    };
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
      uint32_t* const t = a.table[pl];
      auto at = [&](int cls, int k) { return t + ref::word_at(a.L, pl, cls, k, ref::row_of(a.L, pl, cls, wave, r), lane); };
      auto operand = [&](int cls, int k) { return ref::operand(a.seed, cls, k, wave, r, lane); };
      issue(pl, BGC_ATOMIC_INT32, ref::kAdd, operand(BGC_ATOMIC_INT32, ref::kAdd),
            [&](uint32_t v) { __hip_atomic_fetch_add(at(BGC_ATOMIC_INT32, ref::kAdd), v, BGC_RELAXED_AGENT); });
      issue(pl, BGC_ATOMIC_INT32, ref::kSmin, operand(BGC_ATOMIC_INT32, ref::kSmin), [&](uint32_t v) {
        __hip_atomic_fetch_min(reinterpret_cast<int*>(at(BGC_ATOMIC_INT32, ref::kSmin)), static_cast<int>(v), BGC_RELAXED_AGENT);
      });
      issue(pl, BGC_ATOMIC_INT32, ref::kUmax, operand(BGC_ATOMIC_INT32, ref::kUmax),
            [&](uint32_t v) { __hip_atomic_fetch_max(at(BGC_ATOMIC_INT32, ref::kUmax), v, BGC_RELAXED_AGENT); });
      issue(pl, BGC_ATOMIC_INT32, ref::kAnd, operand(BGC_ATOMIC_INT32, ref::kAnd),
            [&](uint32_t v) { __hip_atomic_fetch_and(at(BGC_ATOMIC_INT32, ref::kAnd), v, BGC_RELAXED_AGENT); });
      issue(pl, BGC_ATOMIC_INT32, ref::kOr, operand(BGC_ATOMIC_INT32, ref::kOr),
            [&](uint32_t v) { __hip_atomic_fetch_or(at(BGC_ATOMIC_INT32, ref::kOr), v, BGC_RELAXED_AGENT); });
      issue(pl, BGC_ATOMIC_INT32, ref::kXor, operand(BGC_ATOMIC_INT32, ref::kXor),
            [&](uint32_t v) { __hip_atomic_fetch_xor(at(BGC_ATOMIC_INT32, ref::kXor), v, BGC_RELAXED_AGENT); });
      issue(pl, BGC_ATOMIC_INT64, 0, operand(BGC_ATOMIC_INT64, 0), [&](uint32_t lo) {
        const unsigned long long v = static_cast<unsigned long long>(operand(BGC_ATOMIC_INT64, 1)) << 32 | lo;
        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(at(BGC_ATOMIC_INT64, 0)), v, BGC_RELAXED_AGENT);
      });
      issue(pl, BGC_ATOMIC_F32, 0, operand(BGC_ATOMIC_F32, 0),
            [&](uint32_t v) { unsafeAtomicAdd(reinterpret_cast<float*>(at(BGC_ATOMIC_F32, 0)), static_cast<float>(ref::f32_value(v))); });
      issue(pl, BGC_ATOMIC_F64, 0, operand(BGC_ATOMIC_F64, 0),
            [&](uint32_t v) { unsafeAtomicAdd(reinterpret_cast<double*>(at(BGC_ATOMIC_F64, 0)), static_cast<double>(ref::f64_value(v))); });
      issue(pl, BGC_ATOMIC_PK16, 0, operand(BGC_ATOMIC_PK16, 0),
            [&](uint32_t v) { pk_add_bf16(at(BGC_ATOMIC_PK16, 0), ref::pk_bf16_trits(ref::trit(v), ref::trit(v >> 16))); });
      issue(pl, BGC_ATOMIC_PK16, 1, operand(BGC_ATOMIC_PK16, 1),
            [&](uint32_t v) { pk_add_f16(at(BGC_ATOMIC_PK16, 1), ref::pk_f16_trits(ref::trit(v), ref::trit(v >> 16))); });
      bool won = false;
      issue(pl, BGC_ATOMIC_CAS, 0, id, [&](uint32_t v) {
        uint32_t seen = ref::kEmpty;
        won |= __hip_atomic_compare_exchange_strong(at(BGC_ATOMIC_CAS, 0), &seen, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      });
      const unsigned long long winners = __ballot(won);
      if (lane == 0) a.ballots[static_cast<size_t>(pl) * a.L.pairs + pair] = winners;
      issue(pl, BGC_ATOMIC_TICKET, 0, id, [&](uint32_t v) {
        const uint32_t drawn = __hip_atomic_fetch_add(at(BGC_ATOMIC_TICKET, 0), 1u, BGC_RELAXED_AGENT);
        keep(pl == BGC_ATOMIC_OWN ? ref::kOrderOwn : ref::kOrderShared, ref::row_of(a.L, pl, BGC_ATOMIC_TICKET, wave, r), drawn, v);
      });
    }
    // the workgroup's LDS table
    const uint32_t lrow = (wave + static_cast<uint32_t>(r)) & 1;
    auto at = [&](int k) { return &lds[(k * 2 + static_cast<int>(lrow)) * 64 + lane]; };
    auto operand = [&](int k) { return ref::operand(a.seed, BGC_ATOMIC_LDS, k, wave, r, lane); };
    constexpr int kOwn = BGC_ATOMIC_OWN, kLds = BGC_ATOMIC_LDS;
    issue(kOwn, kLds, ref::kLdsAdd, operand(ref::kLdsAdd), [&](uint32_t v) { __hip_atomic_fetch_add(at(ref::kLdsAdd), v, BGC_RELAXED_WORKGROUP); });
    issue(kOwn, kLds, ref::kLdsTicket, id, [&](uint32_t v) {
      const uint32_t drawn = __hip_atomic_fetch_add(at(ref::kLdsTicket), 1u, BGC_RELAXED_WORKGROUP);
      keep(ref::kOrderLds, 2 * blockIdx.x + lrow, drawn, v);
    });
    issue(kOwn, kLds, ref::kLdsMax, operand(ref::kLdsMax), [&](uint32_t v) { __hip_atomic_fetch_max(at(ref::kLdsMax), v, BGC_RELAXED_WORKGROUP); });
    issue(kOwn, kLds, ref::kLdsMin, operand(ref::kLdsMin), [&](uint32_t v) {
      __hip_atomic_fetch_min(reinterpret_cast<int*>(at(ref::kLdsMin)), static_cast<int>(v), BGC_RELAXED_WORKGROUP);
    });
    issue(kOwn, kLds, ref::kLdsAnd, operand(ref::kLdsAnd), [&](uint32_t v) { __hip_atomic_fetch_and(at(ref::kLdsAnd), v, BGC_RELAXED_WORKGROUP); });
    issue(kOwn, kLds, ref::kLdsOr, operand(ref::kLdsOr), [&](uint32_t v) { __hip_atomic_fetch_or(at(ref::kLdsOr), v, BGC_RELAXED_WORKGROUP); });
    issue(kOwn, kLds, ref::kLdsXor, operand(ref::kLdsXor), [&](uint32_t v) { __hip_atomic_fetch_xor(at(ref::kLdsXor), v, BGC_RELAXED_WORKGROUP); });
    issue(kOwn, kLds, ref::kLdsAddF32, operand(ref::kLdsAddF32), [&](uint32_t v) {
      __hip_atomic_fetch_add(reinterpret_cast<float*>(at(ref::kLdsAddF32)), static_cast<float>(ref::f32_value(v)), BGC_RELAXED_WORKGROUP);
    });
    bool won = false;
    issue(kOwn, kLds, ref::kLdsCas, id, [&](uint32_t v) {
      uint32_t seen = ref::kEmpty;
      won |= __hip_atomic_compare_exchange_strong(at(ref::kLdsCas), &seen, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    });
    const unsigned long long winners = __ballot(won);
    if (lane == 0) a.ballots[2 * static_cast<size_t>(a.L.pairs) + pair] = winners;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ref::kLdsWords * 128; i += kBlock) {
    a.table[BGC_ATOMIC_OWN][ref::word_at(a.L, BGC_ATOMIC_OWN, BGC_ATOMIC_LDS, i / 128, 2 * blockIdx.x + ((i >> 6) & 1), i & 63)] = lds[i];
  }
  if (threadIdx.x == 0) a.cu_keys[blockIdx.x] = static_cast<int>(cu_key());
}

// Test plants and delays of a rate launch, in device memory (gpu_diag.h).
struct RateExtras {
  const bgc_atomic_rate_plant* p = nullptr;
  int n = 0;
  const bgc_atomic_delay_plant* d = nullptr;
  int nd = 0;
};
__device__ __forceinline__ int rate_times(int /*cls*/, uint32_t /*wave*/, int /*lane*/) { return 1; }
__device__ __forceinline__ int rate_times(int cls, uint32_t wave, int lane, const RateExtras& e) {
  for (int j = 0; j < e.n; ++j) {
    const bgc_atomic_rate_plant p = e.p[j];
    if (p.cls == cls && static_cast<uint32_t>(p.wave) == wave && p.lane == lane) return p.times;
  }
  return 1;
}
__device__ __forceinline__ void rate_wait(int /*cls*/, uint32_t /*wave*/) {}
__device__ __forceinline__ void rate_wait(int cls, uint32_t wave, const RateExtras& e) {
  uint32_t ticks = 0;
  for (int j = 0; j < e.nd; ++j) {
    const bgc_atomic_delay_plant p = e.d[j];
    if ((p.wave == BGC_PLANT_ALL_WAVES || static_cast<uint32_t>(p.wave) == wave) && p.cls == cls) ticks = max(ticks, p.ticks);
  }
  wait_ticks(__builtin_amdgcn_readfirstlane(ticks));  // the same in every lane of the wave
}

// rows: groups * 64 rows of 64 words; heads: one per group; sums: one per wave (rtn); cu_keys: one per workgroup
template <int kClass, bool kTimed, class... Extras>
__global__ __launch_bounds__(kBlock) void atomic_rate(uint32_t seed, int iters, uint32_t* __restrict__ rows, uint32_t* __restrict__ heads,
                                                      unsigned long long* __restrict__ sums, RateBin* __restrict__ bins, int* __restrict__ cu_keys,
                                                      Extras... extras) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), group = ref::rate_group(wave);
  uint32_t* const mine = rows + static_cast<size_t>(group) * ref::kRateRows * 64 + lane;
  const uint32_t h = ref::rate_operand(seed, kClass, wave, lane);
  const int lo = ref::trit(h), hi = ref::trit(h >> 16);
  const float plus = static_cast<float>(lo), minus = static_cast<float>(-lo);  // an integer's negative: no -0
  const uint32_t pk_plus = ref::pk_bf16_trits(lo, hi), pk_minus = ref::pk_bf16_trits(-lo, -hi);
  unsigned long long sum = 0;
  uint64_t t0 = 0, t1 = 0;
  if constexpr (kTimed) {
    t0 = wall_clock64();
    asm volatile("" ::"s"(t0));  // wait for the clock here, not inside the loop
  }
  auto add = [&](int i) {
    uint32_t* const p = mine + (i & (ref::kRateRows - 1)) * 64;
    const bool odd_visit = (i / ref::kRateRows) & 1;
    if constexpr (kClass == BGC_ATOMIC_RATE_F32) {
      unsafeAtomicAdd(reinterpret_cast<float*>(p), odd_visit ? minus : plus);
    } else if constexpr (kClass == BGC_ATOMIC_RATE_PK_BF16) {
      pk_add_bf16(p, odd_visit ? pk_minus : pk_plus);
    } else if constexpr (kClass == BGC_ATOMIC_RATE_U32) {
      __hip_atomic_fetch_add(p, h + static_cast<uint32_t>(i) * ref::kRateStep, BGC_RELAXED_AGENT);
    } else {
      if (lane == 0) sum += __hip_atomic_fetch_add(heads + group, 1u, BGC_RELAXED_AGENT);
    }
  };
  const int plain = sizeof...(Extras) > 0 ? iters - 1 : iters;  // a plant is on the last iteration
#pragma unroll 4
  for (int i = 0; i < plain; ++i) add(i);
  if constexpr (sizeof...(Extras) > 0) {
    const int times = rate_times(kClass, wave, lane, extras...);
    for (int t = 0; t < times; ++t) add(iters - 1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the wave's atomics have left before its clock is read
  rate_wait(kClass, wave, extras...);
  if constexpr (kTimed) t1 = wall_clock64();
  if (kClass == BGC_ATOMIC_RATE_RTN && lane == 0) sums[wave] = sum;
  if constexpr (kTimed) {
    if (lane == 0) {
      RateBin* bin = &bins[xcc_id()];
      atomicAdd(&bin->ticks, static_cast<unsigned long long>(t1 - t0));
      atomicAdd(&bin->n, 1u);
    }
    if (threadIdx.x == 0) cu_keys[blockIdx.x] = static_cast<int>(cu_key());
  }
}

// ---------------------------------------------------------------------------------------------
// host

constexpr int kMaxXccs = 8;

struct AtomicArgs {
  int wgs_per_cu, rounds, rate_iters;
  uint32_t seed;
};

// what the test-only entries add to a run; all empty in bgc_diag_atomic
struct AtomicExtras {
  const bgc_atomic_plant* check = nullptr;
  int n_check = 0;
  const bgc_atomic_rate_plant* rate = nullptr;
  int n_rate = 0;
  const bgc_atomic_delay_plant* delays = nullptr;
  int n_delay = 0;
  bool want_data = false;
  void* data = nullptr;
  uint64_t capacity = 0;
};

bool rounds_ok(int rounds) { return rounds >= 1 && rounds <= 64; }

bool args_ok(const AtomicArgs& a) {
  return a.wgs_per_cu >= 1 && a.wgs_per_cu <= 8 && rounds_ok(a.rounds) && a.rate_iters >= 1 && a.rate_iters <= (1 << 16);
}

bool check_plants_ok(const bgc_atomic_plant* plants, int n, int rounds) {
  return plant_list_ok(plants, n) && std::all_of(plants, plants + n, [&](const bgc_atomic_plant& p) {
           return (p.placement == BGC_ATOMIC_OWN || p.placement == BGC_ATOMIC_SHARED) && p.cls >= 0 && p.cls < ref::kClasses &&
                  !(p.cls == BGC_ATOMIC_LDS && p.placement != BGC_ATOMIC_OWN) && p.op >= 0 && p.op < ref::class_ops(p.cls) && p.wave >= 0 &&
                  p.round >= 0 && p.round < rounds && p.lane >= 0 && p.lane < 64 && p.times >= 0 && p.times <= 2 && !(p.times == 1 && p.xor_mask == 0);
         });
}

bool extras_ok(const AtomicArgs& a, const AtomicExtras& x) {
  if (!check_plants_ok(x.check, x.n_check, a.rounds) || !plant_list_ok(x.rate, x.n_rate) || !plant_list_ok(x.delays, x.n_delay)) return false;
  const bool rate_ok = std::all_of(x.rate, x.rate + x.n_rate, [](const bgc_atomic_rate_plant& p) {
    return p.cls >= 0 && p.cls < ref::kRateClasses && p.wave >= 0 && p.lane >= 0 && p.lane < 64 && !(p.cls == BGC_ATOMIC_RATE_RTN && p.lane != 0) &&
           (p.times == 0 || p.times == 2);
  });
  const bool delays_ok = std::all_of(x.delays, x.delays + x.n_delay, [](const bgc_atomic_delay_plant& p) {
    return p.wave >= BGC_PLANT_ALL_WAVES && p.cls >= 0 && p.cls < ref::kRateClasses && p.ticks > 0 && p.ticks <= BGC_DIAG_MAX_DELAY_TICKS;
  });
  return rate_ok && delays_ok && (!x.want_data || (x.data && x.capacity <= BGC_DIAG_MAX_DATA_BYTES));
}

struct RateRun {
  const AtomicArgs& a;
  const AtomicExtras& x;
  int grid;
  const Events& ev;
  uint32_t* rows;
  uint32_t* heads;
  unsigned long long* sums;
  RateBin* bins;
  int* cu_keys;  // [rate class][workgroup]
  RateExtras extras;
  bgc_atomic_result* out;
};

// One rate class: warm-up, the timed launch, its end values against their closed forms.
template <int kClass>
int rate_class(const RateRun& r) {
  const int iters = r.a.rate_iters, waves = r.grid * (kBlock / 64), groups = r.grid / ref::kRateAdders * 4;
  const size_t row_bytes = static_cast<size_t>(groups) * ref::kRateRows * 64 * sizeof(uint32_t);
  int* const keys = r.cu_keys + kClass * r.grid;
  auto clear = [&]() -> int {
    HIP_TRY(hipMemsetAsync(r.rows, 0, row_bytes, nullptr));
    HIP_TRY(hipMemsetAsync(r.heads, 0, static_cast<size_t>(groups) * sizeof(uint32_t), nullptr));
    HIP_TRY(hipMemsetAsync(r.sums, 0, static_cast<size_t>(waves) * sizeof(unsigned long long), nullptr));
    return 0;
  };
  if (clear() != 0) return 1;
  hipLaunchKernelGGL((atomic_rate<kClass, false>), dim3(r.grid), dim3(kBlock), 0, nullptr, r.a.seed, std::min(iters, 64), r.rows, r.heads, r.sums,
                     r.bins, keys);
  if (clear() != 0) return 1;
  float ms = 0.f;
  if (timed(r.ev, &ms, [&] {
        if (r.extras.n > 0 || r.extras.nd > 0) {
          hipLaunchKernelGGL((atomic_rate<kClass, true, RateExtras>), dim3(r.grid), dim3(kBlock), 0, nullptr, r.a.seed, iters, r.rows, r.heads,
                             r.sums, r.bins, keys, r.extras);
        } else {
          hipLaunchKernelGGL((atomic_rate<kClass, true>), dim3(r.grid), dim3(kBlock), 0, nullptr, r.a.seed, iters, r.rows, r.heads, r.sums, r.bins,
                             keys);
        }
      }) != 0) {
    return 1;
  }
  std::vector<uint32_t> want(ref::rate_words(r.grid, kClass)), got(want.size());
  ref::rate_expected(r.a.seed, r.grid, iters, kClass, want.data());
  HIP_TRY(hipMemcpy(got.data(), kClass == BGC_ATOMIC_RATE_RTN ? r.heads : r.rows, got.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  bool ok = got == want;
  if (kClass == BGC_ATOMIC_RATE_RTN) {  // the tickets of a group are 0 .. n - 1, each drawn once: their sum
    std::vector<unsigned long long> sums(static_cast<size_t>(waves));
    HIP_TRY(hipMemcpy(sums.data(), r.sums, sums.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    const unsigned long long n = static_cast<unsigned long long>(ref::kRateAdders) * static_cast<unsigned long long>(iters);
    for (int g = 0; ok && g < groups; ++g) {
      unsigned long long total = 0;
      for (int adder = 0; adder < ref::kRateAdders; ++adder) total += sums[ref::rate_wave(static_cast<uint32_t>(g), adder)];
      ok = total == n * (n - 1) / 2;
    }
  }
  if (!ok) r.out->rate_ok = 0;
  const double units = static_cast<double>(waves) * iters * (kClass == BGC_ATOMIC_RATE_RTN ? 1e3 : 64.0 * sizeof(uint32_t));  // rtn: 1e9 per second
  r.out->rate[kClass] = tera_per_s(units, ms);
  r.out->rate_ms[kClass] = ms;
  r.out->elapsed_ms += ms;
  return 0;
}

int atomic_run(int device, const AtomicArgs& a, const AtomicExtras& x, bgc_atomic_result* out) {
  if (!(out && args_ok(a) && extras_ok(a, x))) {
    g_last_error = "invalid arguments";
    return 1;
  }
  std::memset(out, 0, sizeof(*out));
  out->first_bad_placement = out->first_bad_class = out->first_bad_op = out->slowest_xcc = -1;
  out->first_bad_element = -1;
  out->rate_ok = 1;
  HIP_TRY(hipSetDevice(device));
  const int cus = cu_count(device), grid = cus * a.wgs_per_cu, rate_grid = (2 * cus + 7) / 8 * 8;
  out->cus = cus;
  if (!ref::layout_args_ok(grid, rate_grid, a.rounds)) return refuse("invalid arguments: a device of that many CUs");
  ref::Layout L;
  ref::make_layout(grid, rate_grid, a.rounds, &L);
  if (any_beyond(x.check, x.n_check, &bgc_atomic_plant::wave, L.waves) || any_beyond(x.rate, x.n_rate, &bgc_atomic_rate_plant::wave, rate_grid * 4) ||
      any_beyond(x.delays, x.n_delay, &bgc_atomic_delay_plant::wave, rate_grid * 4)) {
    return refuse(kWaveBeyond);
  }
  if (x.want_data && L.total_words * sizeof(uint32_t) > x.capacity) return refuse("invalid arguments: the data exceed the capacity");

  // the device's copy of the data block: zero but for the tables' initial values
  std::vector<uint32_t> words(L.total_words);
  DeviceBuffer block, out_of_range, d_check, d_rate, d_delays;
  HIP_TRY(block.alloc(words.size() * sizeof(uint32_t), true));
  HIP_TRY(out_of_range.alloc(sizeof(unsigned), true));
  uint32_t* const d_words = block.as<uint32_t>();
  for (int pl = 0; pl < 2; ++pl) {
    ref::init_table(L, pl, words.data() + L.data_off[pl]);
    HIP_TRY(hipMemcpy(d_words + L.data_off[pl], words.data() + L.data_off[pl], L.data_words[pl] * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  if (upload_plants(d_check, x.check, x.n_check) != 0 || upload_plants(d_rate, x.rate, x.n_rate) != 0 ||
      upload_plants(d_delays, x.delays, x.n_delay) != 0) {
    return 1;
  }
  CheckArgs c{};
  c.L = L;
  c.seed = a.seed;
  c.table[0] = d_words + L.data_off[BGC_ATOMIC_DATA_OWN];
  c.table[1] = d_words + L.data_off[BGC_ATOMIC_DATA_SHARED];
  c.ballots = reinterpret_cast<unsigned long long*>(d_words + L.data_off[BGC_ATOMIC_DATA_BALLOTS]);
  for (int k = 0; k < 3; ++k) c.order[k] = d_words + L.data_off[BGC_ATOMIC_DATA_ORDER_OWN + k];
  c.cu_keys = reinterpret_cast<int*>(d_words + L.data_off[BGC_ATOMIC_DATA_CU_KEYS]);
  c.out_of_range = out_of_range.as<unsigned>();
  Events ev;
  HIP_TRY(ev.create());
  float ms_check = 0.f;
  if (timed(ev, &ms_check, [&] {
        if (x.n_check > 0) {
          hipLaunchKernelGGL((atomic_check<PlantList<bgc_atomic_plant>>), dim3(grid), dim3(kBlock), 0, nullptr, c,
                             PlantList<bgc_atomic_plant>{d_check.as<const bgc_atomic_plant>(), x.n_check});
        } else {
          hipLaunchKernelGGL((atomic_check<>), dim3(grid), dim3(kBlock), 0, nullptr, c);
        }
      }) != 0) {
    return 1;
  }
  out->elapsed_ms = ms_check;
  HIP_TRY(hipMemcpy(words.data(), d_words, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  unsigned beyond = 0;
  HIP_TRY(hipMemcpy(&beyond, out_of_range.p, sizeof(beyond), hipMemcpyDeviceToHost));
  out->tickets_out_of_range = beyond;
  ref::judge(L, a.seed, words.data(), out);

  const int groups = rate_grid / ref::kRateAdders * 4;
  DeviceBuffer rows, heads, sums, bins;
  HIP_TRY(rows.alloc(static_cast<size_t>(groups) * ref::kRateRows * 64 * sizeof(uint32_t)));
  HIP_TRY(heads.alloc(static_cast<size_t>(groups) * sizeof(uint32_t)));
  HIP_TRY(sums.alloc(static_cast<size_t>(rate_grid) * (kBlock / 64) * sizeof(unsigned long long)));
  HIP_TRY(bins.alloc(kMaxXccs * sizeof(RateBin), true));
  int* const d_rate_keys = reinterpret_cast<int*>(d_words + L.data_off[BGC_ATOMIC_DATA_RATE_CU_KEYS]);
  const RateRun r{a, x, rate_grid, ev, rows.as<uint32_t>(), heads.as<uint32_t>(), sums.as<unsigned long long>(), bins.as<RateBin>(), d_rate_keys,
                  RateExtras{d_rate.as<const bgc_atomic_rate_plant>(), x.n_rate, d_delays.as<const bgc_atomic_delay_plant>(), x.n_delay}, out};
  if (rate_class<BGC_ATOMIC_RATE_F32>(r) != 0 || rate_class<BGC_ATOMIC_RATE_PK_BF16>(r) != 0 || rate_class<BGC_ATOMIC_RATE_U32>(r) != 0 ||
      rate_class<BGC_ATOMIC_RATE_RTN>(r) != 0) {
    return 1;
  }
  RateBin h_bins[kMaxXccs];
  HIP_TRY(hipMemcpy(h_bins, bins.p, sizeof(h_bins), hipMemcpyDeviceToHost));
  const double ticks_per_us = constant_clock_khz(device) / 1e3;
  TimingFold fold;  // of the mean loop time of a rate wave on an XCC, the four timed launches together
  for (int k = 0; k < kMaxXccs; ++k) {
    out->xcc_waves[k] = static_cast<int>(h_bins[k].n);
    out->xcc_us[k] = fold.add(k, h_bins[k].ticks, h_bins[k].n, ticks_per_us);
  }
  out->slowest_xcc = fold.slowest_key;
  out->xcc_balance = fold.balance();
  if (x.want_data) {
    HIP_TRY(hipMemcpy(words.data() + L.data_off[BGC_ATOMIC_DATA_RATE_CU_KEYS], d_rate_keys, L.data_words[BGC_ATOMIC_DATA_RATE_CU_KEYS] * sizeof(int),
                      hipMemcpyDeviceToHost));
    std::memcpy(x.data, words.data(), words.size() * sizeof(uint32_t));
  }
  return 0;
}

}  // namespace

extern "C" {

int bgc_diag_atomic(int device, int wgs_per_cu, int rounds, int rate_iters, uint32_t seed, bgc_atomic_result* out) {
  return atomic_run(device, {wgs_per_cu, rounds, rate_iters, seed}, AtomicExtras{}, out);
}

int bgc_diag_atomic_planted(int device, int wgs_per_cu, int rounds, int rate_iters, uint32_t seed, const bgc_atomic_plant* plants, int n,
                            const bgc_atomic_rate_plant* rate, int n_rate, bgc_atomic_result* out) {
  AtomicExtras x;
  x.check = plants;
  x.n_check = n;
  x.rate = rate;
  x.n_rate = n_rate;
  return atomic_run(device, {wgs_per_cu, rounds, rate_iters, seed}, x, out);
}

int bgc_diag_atomic_delayed(int device, int wgs_per_cu, int rounds, int rate_iters, uint32_t seed, const bgc_atomic_delay_plant* delays, int n,
                            bgc_atomic_result* out) {
  AtomicExtras x;
  x.delays = delays;
  x.n_delay = n;
  return atomic_run(device, {wgs_per_cu, rounds, rate_iters, seed}, x, out);
}

int bgc_diag_atomic_data(int device, int wgs_per_cu, int rounds, int rate_iters, uint32_t seed, const bgc_atomic_plant* plants, int n,
                         const bgc_atomic_rate_plant* rate, int n_rate, const bgc_atomic_delay_plant* delays, int n_delay, void* data,
                         uint64_t capacity, bgc_atomic_result* out) {
  AtomicExtras x;
  x.check = plants;
  x.n_check = n;
  x.rate = rate;
  x.n_rate = n_rate;
  x.delays = delays;
  x.n_delay = n_delay;
  x.want_data = true;
  x.data = data;
  x.capacity = capacity;
  return atomic_run(device, {wgs_per_cu, rounds, rate_iters, seed}, x, out);
}

int bgc_diag_atomic_layout(int grid, int rate_grid, int rounds, bgc_atomic_layout* out) {
  if (!out || !ref::layout_args_ok(grid, rate_grid, rounds)) return refuse("invalid arguments");
  ref::make_layout(grid, rate_grid, rounds, out);
  return 0;
}

int bgc_diag_atomic_expected(uint32_t seed, int grid, int rounds, const bgc_atomic_plant* plants, int n, void* data, uint64_t capacity) {
  if (!data || !ref::layout_args_ok(grid, 8, rounds) || capacity > BGC_DIAG_MAX_DATA_BYTES || !check_plants_ok(plants, n, rounds)) {
    return refuse("invalid arguments");
  }
  ref::Layout L;
  ref::make_layout(grid, 8, rounds, &L);
  if (any_beyond(plants, n, &bgc_atomic_plant::wave, L.waves)) return refuse(kWaveBeyond);
  if (L.total_words * sizeof(uint32_t) > capacity) return refuse("invalid arguments: the data exceed the capacity");
  ref::expected(L, seed, plants, n, static_cast<uint32_t*>(data));
  return 0;
}

int bgc_diag_atomic_rate_expected(uint32_t seed, int rate_grid, int rate_iters, int cls, uint32_t* out, uint64_t capacity_words) {
  if (!out || !ref::layout_args_ok(1, rate_grid, 1) || rate_iters < 1 || rate_iters > (1 << 16) || cls < 0 || cls >= ref::kRateClasses ||
      capacity_words < ref::rate_words(rate_grid, cls)) {
    return refuse("invalid arguments");
  }
  ref::rate_expected(seed, rate_grid, rate_iters, cls, out);
  return 0;
}

}  // extern "C"
