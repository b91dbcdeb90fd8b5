// The cache hierarchy between the LDS and HBM: each XCD's 4 MiB L2 (march and read rate, attributed
// to the XCC) and the 256 MiB Infinity Cache (pattern check and read rate) (bgc_diag_cache).
//
//  * No workgroup waits for another, every barrier is reached by every thread of its workgroup, and
//    every address is a function of blockIdx, threadIdx, loop counters and arguments checked on the
//    host: nothing read from memory is used as an index (the test plants' word, checked on the host
//    before the device is touched, is the one exception, and it exists only in the planted
//    instantiation).  The buffers are sized exactly: grid regions of region_words, ic_bytes.
//  * The L2 buffer is one region (1..4 slabs of 32 KiB: 256 threads x 16 B x 8 loads) per CU, and
//    every L2 launch is one 256-thread workgroup per CU.  At the default 96 KiB the 32 workgroups
//    that the dispatcher deals to an XCD hold 3 MiB of its 4 MiB.  That dealing (round-robin over the
//    XCDs) is observed, not promised: nothing here is wrong without it, only slower, because a
//    workgroup reads back what itself wrote through the one L2 it runs on, and bins the outcome under
//    the XCC it reads from HW_REG_XCC_ID.
//  * l2_march, launched once per round: in round r workgroup b takes region (b + r) % grid, so over
//    the rounds an XCD's L2 holds different addresses.  Pass 0 writes the pattern (gpu_diag.h, "the
//    data the diagnostics generate") with plain 16-byte lane-contiguous stores, which leave the line
//    in the XCD's L2, and after a barrier verifies it with nontemporal 16-byte loads
//    (global_load_dwordx4 ... nt in the gfx950 disassembly), which bypass the CU's L1 and are served
//    by L2; each thread checks what the thread 64 further on wrote, so no wave checks only its own
//    stores.  Pass 1 writes the inverse as single dwords in per-thread runs (global_store_dword: the
//    compiler barrier keeps them apart) and verifies with nontemporal 8-byte loads
//    (global_load_dwordx2 ... nt), so the store width and the lane-to-channel routing differ.
//    What this covers: the data that an XCD's L2 held between a fill and its verify read back right,
//    for `rounds` different address sets and for both polarities of every bit.  What it cannot: a
//    cache is not addressable cell by cell as the LDS is, so which set, way or bank held a word is
//    the hardware's choice, a line that the L2 evicted in between was served by the Infinity Cache or
//    HBM instead, and a cell that no line of the buffer was placed in is not tested.
//  * l2_rate: a workgroup fills its region and computes from the hash the 32-bit sum of one sweep,
//    untimed; then it reads the region `sweeps` times with nontemporal 16-byte loads, 8 per lane in
//    flight (a slab at a time), and sums every dword: a sum, since an XOR over an even number of
//    sweeps would cancel a stuck bit (the sum has the same blind spot only for the top bit, which the
//    march covers).  The clock read is consumed before the loop, and the compiler barrier at the end
//    of a sweep keeps the loads in the loop although the region does not change.  Checked in the
//    gfx950 disassembly: the loop body is one slab's eight global_load_dwordx4 ... nt, all issued
//    (the scheduling barrier behind them: without it the compiler consumed the first after two) and
//    then retired by counted s_waitcnt vmcnt(7) .. vmcnt(0) with the adds in between; no scratch, no
//    spills (44 VGPRs).  Each workgroup times its loop on the 100 MHz constant clock into its XCC's
//    bin.  Measured on the MI355X (profiles/cache_diag/cache_rates.json): 31.2-31.6 TB/s at 96 KiB
//    with 99.6 % of the requests hitting L2 (TCC_HIT / TCC_MISS, the misses being the fill's lines).
//  * Infinity Cache: ic_fill writes the pattern and adds its words into S, per wave with one
//    atomicAdd; ic_check compares every word with the hash, once right after the fill (which is also
//    the warm-up that brings the buffer on die) and once after the timed sweeps, so what sat in the
//    cache is checked word by word.  ic_rate sweeps the whole buffer in 32 KiB slabs, grid-stride; in
//    sweep i workgroup b starts at slab (b + i) % gridDim.x, so successive sweeps read the same bytes
//    from another XCD and no L2 can serve them (an XCD's share of a sweep, ic_bytes / 8, exceeds its
//    L2 anyway from 32 MiB on; measured, 4 % of the requests hit L2 at 32 MiB and 0.3 % at 128).  It
//    uses plain loads: nt may change the memory-side allocation policy, and measured 8.4-8.6 TB/s
//    against 9.8-10.7 at 32 MiB and the same from 128 MiB on.  Its 32-bit total must be sweeps * S.
#include <algorithm>
#include <cstring>
#include <vector>

#include "diag_common.h"

namespace {

using namespace bgc_diag;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kSlabElems = BGC_L2_SLAB_BYTES / 16;  // 16-byte elements of a slab
constexpr int kMaxXccs = 8;
constexpr uint64_t kIcMaxBytes = 1ULL << 30;
constexpr int kIcWgsPerCu = 8;  // ic_fill, ic_check, ic_rate: 2048 workgroups on 256 CUs, as the HBM stream uses

// The variants that tools/probes/cache_rate_probe.py measures (profiles/cache_diag/cache_rates.json), 12 runs
// each on the MI355X.  512 rate threads (4 loads per lane and slab) read 29.7-33.4 TB/s over the four region
// sizes and 256 read 28.3-32.0: no difference beyond the spread.  Plain L2 loads read the same from 64 KiB on
// and 34.4-38.5 TB/s at 32 KiB, where the CU's 32 KiB L1 serves a share: nt keeps that out of an L2 rate.
#ifndef BGC_L2_RATE_THREADS
#define BGC_L2_RATE_THREADS 256
#endif
#ifndef BGC_L2_RATE_NT
#define BGC_L2_RATE_NT 1
#endif
#ifndef BGC_IC_RATE_NT
#define BGC_IC_RATE_NT 0
#endif
constexpr int kRateThreads = BGC_L2_RATE_THREADS;
static_assert(kRateThreads == 256 || kRateThreads == 512, "256 or 512 threads");

template <bool kNt>
__device__ __forceinline__ u32x4 load16(const u32x4* p) {
  if constexpr (kNt) {
    return __builtin_nontemporal_load(p);
  } else {
    return *p;
  }
}

__device__ __forceinline__ uint32_t sum4(u32x4 v) { return v.x + v.y + v.z + v.w; }

// workgroup b's seed in round `round` of a launch of `grid` workgroups
__device__ __forceinline__ uint32_t round_seed(uint32_t seed, uint32_t round, uint32_t grid, uint32_t b) {
  return mix32(seed + (round * grid + b + 1) * 0x9e3779b9U);
}

// An XCC's bins.  `first` starts at ~0.
struct MarchBin {
  unsigned long long checked, bad;
  unsigned bits, first;
};
struct IcBin {
  unsigned long long bad;
  unsigned bits, first;
};

// Test plants (gpu_diag.h).  l2_march and l2_rate end in a pack `Extras... extras`: empty in the
// production instantiations, which call the empty overloads below, a plant list behind
// bgc_diag_cache_planted (march) or bgc_diag_cache_delayed (rate).
using L2Plants = PlantList<bgc_l2_plant>;
using DelayPlants = PlantList<bgc_cache_delay_plant>;

// The barrier behind a fill.  A workgroup barrier alone does not wait for the stores of its own wave
// (one CU's vector memory operations stay in order anyway): with the wait, every store of the fill
// has been acknowledged by L2 before any thread of the workgroup reads.
__device__ __forceinline__ void fill_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// after pass `pass`'s fill barrier, before its verify.  The plant's own read bypasses the L1 like the
// verify's, and each store has reached L2 before the next plant reads (two plants may name one word).
__device__ __forceinline__ void after_fill(uint32_t*, uint32_t /*region_words*/, int /*round*/, int /*pass*/) {}
__device__ __forceinline__ void after_fill(uint32_t* region, uint32_t region_words, int round, int pass, L2Plants pl) {
  if (threadIdx.x == 0) {
    for (int j = 0; j < pl.n; ++j) {
      const bgc_l2_plant p = pl.p[j];
      if (p.round == round && (p.wg == BGC_PLANT_ALL_WAVES || p.wg == static_cast<int>(blockIdx.x)) && p.pass == pass &&
          p.word < region_words) {
        region[p.word] = __builtin_nontemporal_load(region + p.word) ^ p.xor_mask;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
  }
  fill_barrier();
}

// after the rate loop, before the end time: the workgroup waits for the largest `ticks` that names it
__device__ __forceinline__ void delay() {}
__device__ __forceinline__ void delay(DelayPlants pl) {
  uint32_t ticks = 0;
  for (int j = 0; j < pl.n; ++j) {
    const bgc_cache_delay_plant p = pl.p[j];
    if (p.wg == BGC_PLANT_ALL_WAVES || p.wg == static_cast<int>(blockIdx.x)) ticks = max(ticks, p.ticks);
  }
  wait_ticks(__builtin_amdgcn_readfirstlane(ticks));  // the same in every thread of the workgroup
}

// `passes` is 2 except behind bgc_diag_cache_data, which ends the last round after pass 0 to see it.
template <class... Extras>
__global__ __launch_bounds__(kBlock) void l2_march(uint32_t* buf, uint32_t region_words, uint32_t seed, int round, int passes,
                                                   MarchBin* __restrict__ bins, Extras... extras) {
  __shared__ unsigned red[kBlock / 64][3];
  const uint32_t t = threadIdx.x, b = blockIdx.x, grid = gridDim.x;
  const uint32_t region = (b + static_cast<uint32_t>(round)) % grid, s = round_seed(seed, static_cast<uint32_t>(round), grid, b);
  const uint32_t base = region * region_words, n_elems = region_words / 4;  // a word's index in the whole buffer: base + j
  uint32_t* words = buf + static_cast<size_t>(region) * region_words;
  u32x4* elems = reinterpret_cast<u32x4*>(words);
  BadWords bad;
  // pass 0: plain 16-byte stores, nontemporal 16-byte loads, lane-contiguous
  for (uint32_t k = 0; k < n_elems / kBlock; ++k) elems[k * kBlock + t] = pattern16(k * kBlock + t, s, 0);
  fill_barrier();
  after_fill(words, region_words, round, 0, extras...);
  for (uint32_t k = 0; k < n_elems / kBlock; ++k) {
    const uint32_t e = k * kBlock + ((t + 64) % kBlock);
    const u32x4 v = __builtin_nontemporal_load(&elems[e]), x = pattern16(e, s, 0);
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) bad.check(base + 4 * e + c, x[c], v[c]);
  }
  if (passes > 1) {
    __syncthreads();
    // pass 1: the inverse as single dwords, thread t a run of consecutive words; verified with
    // nontemporal 8-byte loads, lane-contiguous
    const uint32_t run = region_words / kBlock;
    for (uint32_t i = 0; i < run; ++i) {
      words[t * run + i] = ~mix32((t * run + i) ^ s);
      asm volatile("" ::: "memory");
    }
    fill_barrier();
    after_fill(words, region_words, round, 1, extras...);
    const u32x2* pairs = reinterpret_cast<const u32x2*>(words);
    for (uint32_t k = 0; k < region_words / 2 / kBlock; ++k) {
      const uint32_t q = k * kBlock + t;
      const u32x2 v = __builtin_nontemporal_load(&pairs[q]);
      bad.check(base + 2 * q, ~mix32((2 * q) ^ s), v.x);
      bad.check(base + 2 * q + 1, ~mix32((2 * q + 1) ^ s), v.y);
    }
  }
  // the workgroup's outcome, into the bin of the XCC whose L2 served it
  bad.merge_wave();
  if ((t & 63) == 0) {
    red[t >> 6][0] = bad.count;
    red[t >> 6][1] = bad.bits;
    red[t >> 6][2] = bad.first;
  }
  __syncthreads();
  if (t == 0) {
    BadWords all;
    for (int w = 0; w < kBlock / 64; ++w) all.merge(red[w][0], red[w][1], red[w][2]);
    MarchBin* bin = &bins[xcc_id()];
    atomicAdd(&bin->checked, static_cast<unsigned long long>(passes > 1 ? 2 : 1) * region_words);
    if (all.count) {
      atomicAdd(&bin->bad, static_cast<unsigned long long>(all.count));
      atomicOr(&bin->bits, all.bits);
      atomicMin(&bin->first, all.first);
    }
  }
}

template <int kThreads, bool kNt, class... Extras>
__global__ __launch_bounds__(kThreads) void l2_rate(uint32_t* buf, uint32_t region_words, uint32_t seed, int round, int sweeps,
                                                    RateBin* __restrict__ bins, unsigned* __restrict__ fails, Extras... extras) {
  constexpr uint32_t kReads = kSlabElems / kThreads;  // 16-byte reads of a lane per slab: 8 (4 at 512 threads)
  const uint32_t t = threadIdx.x, b = blockIdx.x, n_elems = region_words / 4;
  const uint32_t s = round_seed(seed, static_cast<uint32_t>(round), gridDim.x, b);
  u32x4* elems = reinterpret_cast<u32x4*>(buf + static_cast<size_t>(b) * region_words);
  // untimed: the pattern, and from the hash the sum of the words this thread reads in one sweep
  uint32_t sweep = 0;
  for (uint32_t e = t; e < n_elems; e += kThreads) {
    const u32x4 v = pattern16(e, s, 0);
    elems[e] = v;
    sweep += sum4(v);
  }
  fill_barrier();  // the fill is in L2 before the clock starts
  const uint64_t t0 = wall_clock64();
  asm volatile("" ::"s"(t0));  // wait for the clock here, not inside the loop
  uint32_t sum = 0;
  for (int it = 0; it < sweeps; ++it) {
    for (uint32_t sl = 0; sl < n_elems; sl += kSlabElems) {
      const u32x4* p = elems + sl + t;
      u32x4 v[kReads];
#pragma unroll
      for (uint32_t k = 0; k < kReads; ++k) v[k] = load16<kNt>(p + k * kThreads);
      __builtin_amdgcn_sched_barrier(0);  // every load of the slab is issued before the first is consumed
#pragma unroll
      for (uint32_t k = 0; k < kReads; ++k) sum += sum4(v[k]);
    }
    asm volatile("" ::: "memory");  // the next sweep loads again
  }
  __syncthreads();  // every wave's loads have returned
  delay(extras...);
  const uint64_t t1 = wall_clock64();
  if (sum != static_cast<uint32_t>(sweeps) * sweep) atomicAdd(fails, 1u);
  if (t == 0) {
    RateBin* bin = &bins[xcc_id()];
    atomicAdd(&bin->ticks, static_cast<unsigned long long>(t1 - t0));
    atomicAdd(&bin->n, 1u);
  }
}

// the sum over the wave, added to *total by its lane 0
__device__ __forceinline__ void add_wave_sum(uint32_t sum, unsigned* total) {
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(total, sum);
}

// s = mix32(~seed); *sum += every word written
__global__ __launch_bounds__(kBlock) void ic_fill(u32x4* __restrict__ buf, uint32_t n_elems, uint32_t s, unsigned* __restrict__ sum) {
  uint32_t mine = 0;
  for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < n_elems; e += gridDim.x * kBlock) {
    const u32x4 v = pattern16(e, s, 0);
    buf[e] = v;
    mine += sum4(v);
  }
  add_wave_sum(mine, sum);
}

__global__ __launch_bounds__(kBlock) void ic_check(const u32x4* __restrict__ buf, uint32_t n_elems, uint32_t s, IcBin* __restrict__ bin) {
  BadWords bad;
  for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < n_elems; e += gridDim.x * kBlock) {
    const u32x4 v = buf[e], x = pattern16(e, s, 0);
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) bad.check(4 * e + c, x[c], v[c]);
  }
  bad.merge_wave();
  if ((threadIdx.x & 63) == 0 && bad.count) {
    atomicAdd(&bin->bad, static_cast<unsigned long long>(bad.count));
    atomicOr(&bin->bits, bad.bits);
    atomicMin(&bin->first, bad.first);
  }
}

template <bool kNt>
__global__ __launch_bounds__(kBlock) void ic_rate(const u32x4* __restrict__ buf, uint32_t slabs, int sweeps, unsigned* __restrict__ total) {
  constexpr uint32_t kReads = kSlabElems / kBlock;
  uint32_t sum = 0;
  for (int i = 0; i < sweeps; ++i) {
    for (uint32_t sl = (blockIdx.x + static_cast<uint32_t>(i)) % gridDim.x; sl < slabs; sl += gridDim.x) {
      const u32x4* p = buf + static_cast<size_t>(sl) * kSlabElems + threadIdx.x;
      u32x4 v[kReads];
#pragma unroll
      for (uint32_t k = 0; k < kReads; ++k) v[k] = load16<kNt>(p + k * kBlock);
      __builtin_amdgcn_sched_barrier(0);  // as in l2_rate
#pragma unroll
      for (uint32_t k = 0; k < kReads; ++k) sum += sum4(v[k]);
      asm volatile("" ::: "memory");  // the next sweep loads again
    }
  }
  add_wave_sum(sum, total);
}

// ---------------------------------------------------------------------------------------------
// host

struct CacheArgs {
  int rounds;
  uint32_t region_bytes;
  int passes;  // of the last round of the march
  int l2_sweeps;
  uint64_t ic_bytes;
  int ic_sweeps;
  uint32_t seed;
};

// what the test-only entries add to a run; all empty in bgc_diag_cache
struct CacheExtras {
  const bgc_l2_plant* l2 = nullptr;
  int n_l2 = 0;
  const bgc_ic_plant* ic = nullptr;
  int n_ic = 0;
  const bgc_cache_delay_plant* delays = nullptr;
  int n_delay = 0;
  bool want_data = false;
  void* l2_data = nullptr;
  uint64_t l2_capacity = 0;
  void* ic_data = nullptr;
};

bool args_ok(const CacheArgs& a) {
  return a.rounds >= 1 && a.rounds <= 16 && a.region_bytes % BGC_L2_SLAB_BYTES == 0 && a.region_bytes >= BGC_L2_SLAB_BYTES &&
         a.region_bytes <= 4 * BGC_L2_SLAB_BYTES && (a.passes == 1 || a.passes == 2) && a.l2_sweeps >= 1 && a.l2_sweeps <= (1 << 16) &&
         a.ic_bytes % (1ULL << 20) == 0 && a.ic_bytes <= kIcMaxBytes && a.ic_sweeps >= 1 && a.ic_sweeps <= 4096;
}

bool extras_ok(const CacheArgs& a, const CacheExtras& x) {
  if (!plant_list_ok(x.l2, x.n_l2) || !plant_list_ok(x.ic, x.n_ic) || !plant_list_ok(x.delays, x.n_delay)) return false;
  const bool l2_ok = std::all_of(x.l2, x.l2 + x.n_l2, [&](const bgc_l2_plant& p) {
    return p.round >= 0 && p.round < a.rounds && p.wg >= BGC_PLANT_ALL_WAVES && (p.pass == 0 || p.pass == 1) &&
           p.word < a.region_bytes / 4 && p.xor_mask != 0;
  });
  const bool ic_ok = std::all_of(x.ic, x.ic + x.n_ic, [&](const bgc_ic_plant& p) {
    return (p.when == 0 || p.when == 1) && p.word < a.ic_bytes / 4 && p.xor_mask != 0;
  });
  const bool delays_ok = std::all_of(x.delays, x.delays + x.n_delay, [](const bgc_cache_delay_plant& p) {
    return p.wg >= BGC_PLANT_ALL_WAVES && p.ticks > 0 && p.ticks <= BGC_DIAG_MAX_DELAY_TICKS;
  });
  const bool data_ok = !x.want_data || (x.l2_data && (x.ic_data || a.ic_bytes == 0) && x.l2_capacity <= BGC_DIAG_MAX_DATA_BYTES &&
                                        x.l2_capacity + a.ic_bytes <= BGC_DIAG_MAX_DATA_BYTES);
  return l2_ok && ic_ok && delays_ok && data_ok;
}

template <class... Extras>
void launch_march(int grid, uint32_t* buf, uint32_t region_words, uint32_t seed, int round, int passes, MarchBin* bins, Extras... extras) {
  hipLaunchKernelGGL((l2_march<Extras...>), dim3(grid), dim3(kBlock), 0, nullptr, buf, region_words, seed, round, passes, bins, extras...);
}

template <class... Extras>
void launch_rate(int grid, uint32_t* buf, uint32_t region_words, uint32_t seed, int round, int sweeps, RateBin* bins, unsigned* fails,
                 Extras... extras) {
  hipLaunchKernelGGL((l2_rate<kRateThreads, BGC_L2_RATE_NT != 0, Extras...>), dim3(grid), dim3(kRateThreads), 0, nullptr, buf,
                     region_words, seed, round, sweeps, bins, fails, extras...);
}

// the Infinity-Cache plants of moment `when`, from the host
int apply_ic_plants(uint32_t* buf, const CacheExtras& x, int when) {
  for (int j = 0; j < x.n_ic; ++j) {
    const bgc_ic_plant& p = x.ic[j];
    if (p.when == when && modify_device_value(buf + p.word, [&](uint32_t v) { return v ^ p.xor_mask; }) != 0) return 1;
  }
  return 0;
}

// the Infinity-Cache phase: fill, check, timed sweeps, check
int ic_run(int cus, const CacheArgs& a, const CacheExtras& x, const Events& ev, bgc_cache_result* out) {
  const uint32_t n_elems = static_cast<uint32_t>(a.ic_bytes / 16), slabs = static_cast<uint32_t>(a.ic_bytes / BGC_L2_SLAB_BYTES);
  const uint32_t s = mix32(~a.seed);
  const int grid = cus * kIcWgsPerCu;
  DeviceBuffer buf, sums, bin;
  HIP_TRY(buf.alloc(a.ic_bytes));
  HIP_TRY(sums.alloc(2 * sizeof(unsigned), true));  // S of the fill, the sweeps' total
  HIP_TRY(bin.alloc_filled(1, IcBin{0, 0, ~0u}));
  auto check = [&] { hipLaunchKernelGGL(ic_check, dim3(grid), dim3(kBlock), 0, nullptr, buf.as<const u32x4>(), n_elems, s, bin.as<IcBin>()); };
  float ms_fill = 0.f, ms_check = 0.f, ms_rate = 0.f, ms_again = 0.f;
  if (timed(ev, &ms_fill, [&] {
        hipLaunchKernelGGL(ic_fill, dim3(grid), dim3(kBlock), 0, nullptr, buf.as<u32x4>(), n_elems, s, sums.as<unsigned>());
      }) != 0 ||
      apply_ic_plants(buf.as<uint32_t>(), x, 0) != 0 || timed(ev, &ms_check, check) != 0 ||
      timed(ev, &ms_rate, [&] {
        hipLaunchKernelGGL(ic_rate<BGC_IC_RATE_NT != 0>, dim3(grid), dim3(kBlock), 0, nullptr, buf.as<const u32x4>(), slabs, a.ic_sweeps,
                           sums.as<unsigned>() + 1);
      }) != 0 ||
      apply_ic_plants(buf.as<uint32_t>(), x, 1) != 0 || timed(ev, &ms_again, check) != 0) {
    return 1;
  }
  unsigned h_sums[2];
  IcBin h_bin;
  HIP_TRY(hipMemcpy(h_sums, sums.p, sizeof(h_sums), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&h_bin, bin.p, sizeof(h_bin), hipMemcpyDeviceToHost));
  if (x.want_data) HIP_TRY(hipMemcpy(x.ic_data, buf.p, a.ic_bytes, hipMemcpyDeviceToHost));
  out->ic_words_checked = 2 * (a.ic_bytes / 4);
  out->ic_mismatches = h_bin.bad;
  if (h_bin.bad) out->ic_first_bad_word = h_bin.first;
  out->ic_bad_bits = h_bin.bits;
  out->ic_read_tbps = tera_per_s(static_cast<double>(a.ic_bytes) * a.ic_sweeps, ms_rate);
  out->ic_rate_ok = h_sums[1] == static_cast<uint32_t>(a.ic_sweeps) * h_sums[0];
  out->elapsed_ms += ms_fill + ms_check + ms_rate + ms_again;
  return 0;
}

int cache_run(int device, const CacheArgs& a, const CacheExtras& x, bgc_cache_result* out) {
  if (!(out && args_ok(a) && extras_ok(a, x))) {
    g_last_error = "invalid arguments";
    return 1;
  }
  std::memset(out, 0, sizeof(*out));
  out->first_bad_xcc = out->slowest_xcc = -1;
  out->ic_first_bad_word = ~0ULL;
  out->ic_rate_ok = 1;
  out->rounds = a.rounds;
  out->region_bytes = a.region_bytes;
  out->ic_bytes = a.ic_bytes;
  HIP_TRY(hipSetDevice(device));
  const int cus = cu_count(device), grid = cus;
  out->cus = cus;
  if (any_beyond(x.l2, x.n_l2, &bgc_l2_plant::wg, grid) || any_beyond(x.delays, x.n_delay, &bgc_cache_delay_plant::wg, grid)) {
    return refuse(kWorkgroupBeyond);
  }
  const uint32_t region_words = a.region_bytes / 4;
  const size_t l2_bytes = static_cast<size_t>(grid) * a.region_bytes;
  if (x.want_data && l2_bytes > x.l2_capacity) {
    g_last_error = "invalid arguments: the L2 buffer of this device exceeds the destination";
    return 1;
  }
  DeviceBuffer l2, d_plants, d_delays, march_bins, rate_bins, fails;
  HIP_TRY(l2.alloc(l2_bytes));
  if (upload_plants(d_plants, x.l2, x.n_l2) != 0 || upload_plants(d_delays, x.delays, x.n_delay) != 0) return 1;
  HIP_TRY(march_bins.alloc_filled(kMaxXccs, MarchBin{0, 0, 0, ~0u}));
  HIP_TRY(rate_bins.alloc(kMaxXccs * sizeof(RateBin), true));
  HIP_TRY(fails.alloc(sizeof(unsigned), true));
  Events ev;
  HIP_TRY(ev.create());
  float ms_march = 0.f, ms_rate = 0.f;
  if (timed(ev, &ms_march, [&] {
        for (int r = 0; r < a.rounds; ++r) {
          const int passes = r == a.rounds - 1 ? a.passes : 2;
          if (x.n_l2 > 0) {
            launch_march(grid, l2.as<uint32_t>(), region_words, a.seed, r, passes, march_bins.as<MarchBin>(),
                         L2Plants{d_plants.as<const bgc_l2_plant>(), x.n_l2});
          } else {
            launch_march(grid, l2.as<uint32_t>(), region_words, a.seed, r, passes, march_bins.as<MarchBin>());
          }
        }
      }) != 0) {
    return 1;
  }
  if (x.want_data) HIP_TRY(hipMemcpy(x.l2_data, l2.p, l2_bytes, hipMemcpyDeviceToHost));
  // warm-up, then the timed rate launch; both with the seed of round `rounds`
  launch_rate(grid, l2.as<uint32_t>(), region_words, a.seed, a.rounds, std::min(a.l2_sweeps, 16), rate_bins.as<RateBin>(), fails.as<unsigned>());
  HIP_TRY(hipMemset(rate_bins.p, 0, kMaxXccs * sizeof(RateBin)));
  HIP_TRY(hipMemset(fails.p, 0, sizeof(unsigned)));
  if (timed(ev, &ms_rate, [&] {
        if (x.n_delay > 0) {
          launch_rate(grid, l2.as<uint32_t>(), region_words, a.seed, a.rounds, a.l2_sweeps, rate_bins.as<RateBin>(), fails.as<unsigned>(),
                      DelayPlants{d_delays.as<const bgc_cache_delay_plant>(), x.n_delay});
        } else {
          launch_rate(grid, l2.as<uint32_t>(), region_words, a.seed, a.rounds, a.l2_sweeps, rate_bins.as<RateBin>(), fails.as<unsigned>());
        }
      }) != 0) {
    return 1;
  }
  MarchBin h_march[kMaxXccs];
  RateBin h_rate[kMaxXccs];
  unsigned h_fails = 0;
  HIP_TRY(hipMemcpy(h_march, march_bins.p, sizeof(h_march), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_rate, rate_bins.p, sizeof(h_rate), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&h_fails, fails.p, sizeof(unsigned), hipMemcpyDeviceToHost));
  const double ticks_per_us = constant_clock_khz(device) * 1e-3;
  TimingFold fold;  // of the mean loop time of a rate workgroup on an XCC
  for (int k = 0; k < kMaxXccs; ++k) {
    const MarchBin& m = h_march[k];
    if (m.checked) {
      out->xccs_seen++;
      out->l2_words_checked += m.checked;
      out->l2_mismatches += m.bad;
      out->xcc_mismatches[k] = m.bad;
      out->l2_bad_bits |= m.bits;
      if (m.bad) {
        if (out->l2_bad_xccs == 0) {
          out->first_bad_xcc = k;
          out->first_bad_word = m.first;
        }
        out->l2_bad_xccs++;
      }
    }
    out->xcc_wgs[k] = static_cast<int>(h_rate[k].n);
    out->xcc_us[k] = fold.add(k, h_rate[k].ticks, h_rate[k].n, ticks_per_us);
  }
  out->slowest_xcc = fold.slowest_key;
  out->xcc_balance = fold.balance();
  out->l2_read_tbps = tera_per_s(static_cast<double>(grid) * a.l2_sweeps * a.region_bytes, ms_rate);
  out->l2_rate_ok = h_fails == 0;
  out->elapsed_ms = ms_march + ms_rate;
  return a.ic_bytes ? ic_run(cus, a, x, ev, out) : 0;
}

}  // namespace

extern "C" {

int bgc_diag_cache(int device, int rounds, uint32_t region_bytes, int l2_sweeps, uint64_t ic_bytes, int ic_sweeps, uint32_t seed,
                   bgc_cache_result* out) {
  return cache_run(device, {rounds, region_bytes, 2, l2_sweeps, ic_bytes, ic_sweeps, seed}, CacheExtras{}, out);
}

int bgc_diag_cache_planted(int device, int rounds, uint32_t region_bytes, int l2_sweeps, uint64_t ic_bytes, int ic_sweeps, uint32_t seed,
                           const bgc_l2_plant* l2_plants, int n_l2, const bgc_ic_plant* ic_plants, int n_ic, bgc_cache_result* out) {
  CacheExtras x;
  x.l2 = l2_plants;
  x.n_l2 = n_l2;
  x.ic = ic_plants;
  x.n_ic = n_ic;
  return cache_run(device, {rounds, region_bytes, 2, l2_sweeps, ic_bytes, ic_sweeps, seed}, x, out);
}

int bgc_diag_cache_delayed(int device, int rounds, uint32_t region_bytes, int l2_sweeps, uint64_t ic_bytes, int ic_sweeps, uint32_t seed,
                           const bgc_cache_delay_plant* delays, int n, bgc_cache_result* out) {
  CacheExtras x;
  x.delays = delays;
  x.n_delay = n;
  return cache_run(device, {rounds, region_bytes, 2, l2_sweeps, ic_bytes, ic_sweeps, seed}, x, out);
}

int bgc_diag_cache_data(int device, int rounds, uint32_t region_bytes, int passes, int l2_sweeps, uint64_t ic_bytes, int ic_sweeps,
                        uint32_t seed, void* l2_data, uint64_t l2_capacity, void* ic_data, bgc_cache_result* out) {
  CacheExtras x;
  x.want_data = true;
  x.l2_data = l2_data;
  x.l2_capacity = l2_capacity;
  x.ic_data = ic_data;
  return cache_run(device, {rounds, region_bytes, passes, l2_sweeps, ic_bytes, ic_sweeps, seed}, x, out);
}

}  // extern "C"
