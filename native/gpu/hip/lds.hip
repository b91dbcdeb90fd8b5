// Local Data Share: the per-CU march test of all 160 KiB and the LDS read rate (bgc_diag_lds).
//
//  * Both kernels declare the whole LDS of a CU as one static array (163840 B, which a single
//    workgroup may hold on CDNA4, where a CU has 160 KiB), so exactly one workgroup is resident
//    per CU, no dynamic-LDS attribute is needed, and a workgroup's array is its CU's physical LDS.
//  * No workgroup waits for another, every barrier is reached by every thread of its workgroup, and
//    every LDS index is a function of threadIdx, a loop counter and constants: nothing read from
//    memory is used as an index (the test plants' word, checked on the host, is the one exception,
//    and it exists only in the planted instantiation).
//  * lds_march: pass 0 writes the pattern (gpu_diag.h, "the data the diagnostics generate") with
//    16-byte lane-contiguous stores and verifies it with 16-byte loads, each thread the elements
//    that the thread 64 further on wrote, so no wave checks only its own stores; pass 1 writes the
//    inverse as single dwords, thread t words 160 t .. 160 t + 159 (another lane-to-bank routing),
//    and verifies with 8-byte lane-contiguous loads.  The array being all of the LDS, the block
//    reduction reuses its first words once the last verify is done.  One thread then adds the
//    workgroup's outcome to the bin of the CU it ran on (cu_key()).
//  * lds_rate: one workgroup per CU fills the pattern, then reads the array `iters` times with
//    conflict-free 16-byte loads (lane l of a wave reads element base + l) and sums every dword: a
//    sum, since an XOR over an even number of sweeps would cancel a stuck bit.  A sweep's loads
//    are all issued before the first is consumed, so the compiler retires them with counted
//    lgkmcnt waits and the LDS stays busy at one or two waves per SIMD.  The compiler barrier at
//    the end of a sweep keeps the loads inside the loop although the LDS does not change: checked
//    in the gfx950 disassembly (one sweep's ds_read_b128, the counted s_waitcnt lgkmcnt and the
//    adds in the loop body, no scratch, LDS size 163840 in both kernels).  Each workgroup times
//    its loop on the 100 MHz constant clock into its CU's bin.
#include <algorithm>
#include <cstring>
#include <vector>

#include "diag_common.h"

namespace {

using namespace bgc_diag;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kWords = BGC_LDS_WORDS;  // of the array, as 32-bit words
constexpr int kElems = kWords / 4;     // as 16-byte elements
constexpr int kMarchRun = kWords / kBlock;  // consecutive words a thread writes in pass 1
static_assert(kElems % kBlock == 0 && (kWords / 2) % kBlock == 0 && kWords % kBlock == 0, "whole sweeps per thread");

// Threads of a rate workgroup: measured on the MI355X, 512 (two waves per SIMD) read 132 TB/s in
// the mean of 12 runs of 8192 sweeps and 256 read 130 (profiles/lds_diag/lds_rate.json).
#ifndef BGC_LDS_RATE_THREADS
#define BGC_LDS_RATE_THREADS 512
#endif
constexpr int kRateThreads = BGC_LDS_RATE_THREADS;
static_assert(kRateThreads == 256 || kRateThreads == 512, "256 or 512 threads");

__device__ __forceinline__ uint32_t wg_seed(uint32_t seed, uint32_t wg) { return mix32(seed + (wg + 1) * 0x9e3779b9U); }

// A CU's bins (index: cu_key()).  `first` starts at ~0.
struct MarchBin {
  unsigned checked, bad, bits, first;
};

// Test plants and the generated-data copy (gpu_diag.h).  lds_march ends in a pack `Extras... extras`:
// empty in the production instantiation, which calls the empty overloads below (neither a plant nor
// the barrier that follows it), a plant list behind bgc_diag_lds_planted, a dump behind
// bgc_diag_lds_data.
using LdsPlants = PlantList<bgc_lds_plant>;
struct LdsDump {
  int wg, pass;
  u32x4* out;  // kElems elements
};

// after pass `pass`'s fill barrier, before its verify
__device__ __forceinline__ void after_fill(u32x4*, int /*pass*/) {}
__device__ __forceinline__ void after_fill(u32x4*, int /*pass*/, LdsDump) {}
__device__ __forceinline__ void after_fill(u32x4* lds, int pass, LdsPlants pl) {
  if (threadIdx.x == 0) {
    uint32_t* w = reinterpret_cast<uint32_t*>(lds);
    for (int j = 0; j < pl.n; ++j) {
      const bgc_lds_plant p = pl.p[j];
      if ((p.wg == BGC_PLANT_ALL_WAVES || p.wg == static_cast<int>(blockIdx.x)) && p.pass == pass && p.word < kWords) {
        w[p.word] ^= p.xor_mask;
      }
    }
  }
  __syncthreads();
}

// after pass `pass`'s verify, before the barrier that frees the array for what comes next
__device__ __forceinline__ void after_verify(const u32x4*, int /*pass*/) {}
__device__ __forceinline__ void after_verify(const u32x4*, int /*pass*/, LdsPlants) {}
__device__ __forceinline__ void after_verify(const u32x4* lds, int pass, LdsDump d) {
  if (d.wg == static_cast<int>(blockIdx.x) && d.pass == pass) {
    for (int k = 0; k < kElems / kBlock; ++k) d.out[k * kBlock + threadIdx.x] = lds[k * kBlock + threadIdx.x];
  }
}

template <class... Extras>
__global__ __launch_bounds__(kBlock) void lds_march(uint32_t seed, MarchBin* __restrict__ bins, Extras... extras) {
  __shared__ __attribute__((aligned(16))) u32x4 lds[kElems];
  const uint32_t t = threadIdx.x, key = cu_key(), s = wg_seed(seed, blockIdx.x);
  BadWords bad;
  // pass 0: 16-byte stores and loads, lane-contiguous
  for (uint32_t k = 0; k < kElems / kBlock; ++k) lds[k * kBlock + t] = pattern16(k * kBlock + t, s, 0);
  __syncthreads();
  after_fill(lds, 0, extras...);
  for (uint32_t k = 0; k < kElems / kBlock; ++k) {
    const uint32_t e = k * kBlock + ((t + 64) % kBlock);
    const u32x4 v = lds[e], x = pattern16(e, s, 0);
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) bad.check(4 * e + c, x[c], v[c]);
  }
  after_verify(lds, 0, extras...);
  __syncthreads();
  // pass 1: the inverse as single dwords, thread t a run of consecutive words (the compiler barrier
  // after each store keeps the compiler from merging them into wider ones: ds_write_b32 in the
  // disassembly); verified with 8-byte loads, lane-contiguous
  uint32_t* words = reinterpret_cast<uint32_t*>(lds);
  for (uint32_t i = 0; i < kMarchRun; ++i) {
    words[t * kMarchRun + i] = ~mix32((t * kMarchRun + i) ^ s);
    asm volatile("" ::: "memory");
  }
  __syncthreads();
  after_fill(lds, 1, extras...);
  const u32x2* pairs = reinterpret_cast<const u32x2*>(lds);
  for (uint32_t k = 0; k < kWords / 2 / kBlock; ++k) {
    const uint32_t q = k * kBlock + t;
    const u32x2 v = pairs[q];
    bad.check(2 * q, ~mix32((2 * q) ^ s), v.x);
    bad.check(2 * q + 1, ~mix32((2 * q + 1) ^ s), v.y);
  }
  after_verify(lds, 1, extras...);
  // the workgroup's outcome: wave sums by shuffle, then through the array, which is free now
  bad.merge_wave();
  __syncthreads();
  if ((t & 63) == 0) {
    words[3 * (t >> 6)] = bad.count;
    words[3 * (t >> 6) + 1] = bad.bits;
    words[3 * (t >> 6) + 2] = bad.first;
  }
  __syncthreads();
  if (t == 0) {
    BadWords all;
    for (int w = 0; w < kBlock / 64; ++w) all.merge(words[3 * w], words[3 * w + 1], words[3 * w + 2]);
    atomicAdd(&bins[key].checked, 2u * kWords);
    if (all.count) {
      atomicAdd(&bins[key].bad, all.count);
      atomicOr(&bins[key].bits, all.bits);
      atomicMin(&bins[key].first, all.first);
    }
  }
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void lds_rate(uint32_t seed, int iters, RateBin* __restrict__ bins, unsigned* __restrict__ fails) {
  __shared__ __attribute__((aligned(16))) u32x4 lds[kElems];
  constexpr int kReads = kElems / kThreads;  // 16-byte reads of a lane per sweep
  const uint32_t t = threadIdx.x, key = cu_key(), s = wg_seed(seed, blockIdx.x);
  // untimed: the pattern, and from the hash the sum of the words this thread reads in one sweep
  uint32_t sweep = 0;
  for (uint32_t k = 0; k < kReads; ++k) {
    const u32x4 v = pattern16(k * kThreads + t, s, 0);
    lds[k * kThreads + t] = v;
    sweep += v.x + v.y + v.z + v.w;
  }
  __syncthreads();
  const uint64_t t0 = wall_clock64();
  // Wait for the clock here: left pending, its scalar read shares the loop's lgkmcnt counter with
  // the LDS loads, and the compiler then drains the counter to 0 in every sweep.
  asm volatile("" ::"s"(t0));
  uint32_t sum = 0;
  for (int it = 0; it < iters; ++it) {
    u32x4 v[kReads];
#pragma unroll
    for (int k = 0; k < kReads; ++k) v[k] = lds[k * kThreads + t];
#pragma unroll
    for (int k = 0; k < kReads; ++k) sum += v[k].x + v[k].y + v[k].z + v[k].w;
    asm volatile("" ::: "memory");  // the next sweep loads again
  }
  __syncthreads();  // every wave's loads have returned
  const uint64_t t1 = wall_clock64();
  if (sum != static_cast<uint32_t>(iters) * sweep) atomicAdd(fails, 1u);
  if (t == 0) {
    atomicAdd(&bins[key].ticks, static_cast<unsigned long long>(t1 - t0));
    atomicAdd(&bins[key].n, 1u);
  }
}

template <class... Extras>
void launch_march(int grid, uint32_t seed, MarchBin* bins, Extras... extras) {
  hipLaunchKernelGGL((lds_march<Extras...>), dim3(grid), dim3(kBlock), 0, nullptr, seed, bins, extras...);
}

void launch_rate(int grid, uint32_t seed, int iters, RateBin* bins, unsigned* fails) {
  hipLaunchKernelGGL(lds_rate<kRateThreads>, dim3(grid), dim3(kRateThreads), 0, nullptr, seed, iters, bins, fails);
}

// the march's bins on the device, every `first` at ~0
hipError_t alloc_march_bins(DeviceBuffer& bins) { return bins.alloc_filled(BGC_DIAG_MAX_CU_KEYS, MarchBin{0, 0, 0, ~0u}); }

bool lds_plant_ok(const bgc_lds_plant& p) {
  return p.wg >= BGC_PLANT_ALL_WAVES && (p.pass == 0 || p.pass == 1) && p.word < BGC_LDS_WORDS && p.xor_mask != 0;
}

int lds_run(int device, int wgs_per_cu, int rate_iters, uint32_t seed, const bgc_lds_plant* plants, int n, bgc_lds_result* out) {
  if (!(out && wgs_per_cu >= 1 && wgs_per_cu <= 64 && rate_iters >= 1 && rate_iters <= (1 << 16) && plant_list_ok(plants, n) &&
        std::all_of(plants, plants + n, lds_plant_ok))) {
    g_last_error = "invalid arguments";
    return 1;
  }
  std::memset(out, 0, sizeof(*out));
  out->first_bad_cu_key = out->slowest_cu_key = -1;
  HIP_TRY(hipSetDevice(device));
  const int cus = cu_count(device), grid = cus * wgs_per_cu;
  out->cus = cus;
  if (any_beyond(plants, n, &bgc_lds_plant::wg, grid)) return refuse(kWorkgroupBeyond);
  DeviceBuffer d_plants, march_bins, rate_bins, fails;
  if (upload_plants(d_plants, plants, n) != 0) return 1;
  HIP_TRY(alloc_march_bins(march_bins));
  HIP_TRY(rate_bins.alloc(BGC_DIAG_MAX_CU_KEYS * sizeof(RateBin), true));
  HIP_TRY(fails.alloc(sizeof(unsigned), true));
  Events ev;
  HIP_TRY(ev.create());
  float ms_march = 0.f, ms_rate = 0.f;
  if (timed(ev, &ms_march, [&] {
        if (n > 0) {
          launch_march(grid, seed, march_bins.as<MarchBin>(), LdsPlants{d_plants.as<const bgc_lds_plant>(), n});
        } else {
          launch_march(grid, seed, march_bins.as<MarchBin>());
        }
      }) != 0) {
    return 1;
  }
  // warm-up, then the timed rate launch
  launch_rate(cus, seed, std::min(rate_iters, 64), rate_bins.as<RateBin>(), fails.as<unsigned>());
  HIP_TRY(hipMemset(rate_bins.p, 0, BGC_DIAG_MAX_CU_KEYS * sizeof(RateBin)));
  HIP_TRY(hipMemset(fails.p, 0, sizeof(unsigned)));
  if (timed(ev, &ms_rate, [&] { launch_rate(cus, seed, rate_iters, rate_bins.as<RateBin>(), fails.as<unsigned>()); }) != 0) return 1;
  std::vector<MarchBin> h_march(BGC_DIAG_MAX_CU_KEYS);
  std::vector<RateBin> h_rate(BGC_DIAG_MAX_CU_KEYS);
  unsigned h_fails = 0;
  HIP_TRY(hipMemcpy(h_march.data(), march_bins.p, h_march.size() * sizeof(MarchBin), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_rate.data(), rate_bins.p, h_rate.size() * sizeof(RateBin), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&h_fails, fails.p, sizeof(unsigned), hipMemcpyDeviceToHost));
  TimingFold fold;  // of the ticks of one rate workgroup on a CU
  for (int k = 0; k < BGC_DIAG_MAX_CU_KEYS; ++k) {
    const MarchBin& m = h_march[static_cast<size_t>(k)];
    if (m.checked) {
      out->cus_seen++;
      out->words_checked += m.checked;
      out->mismatches += m.bad;
      out->bad_bits |= m.bits;
      if (m.bad) {
        if (out->bad_cus == 0) {
          out->first_bad_cu_key = k;
          out->first_bad_word = m.first;
        }
        note_bad_cu(out, k);
      }
    }
    fold.add(k, h_rate[static_cast<size_t>(k)].ticks, h_rate[static_cast<size_t>(k)].n, 1.0);
  }
  out->slowest_cu_key = fold.slowest_key;
  out->cu_balance = fold.balance();
  out->read_tbps = tera_per_s(static_cast<double>(cus) * rate_iters * (4.0 * kWords), ms_rate);
  out->rate_ok = h_fails == 0;
  out->elapsed_ms = ms_march + ms_rate;
  return 0;
}

}  // namespace

extern "C" {

int bgc_diag_lds(int device, int wgs_per_cu, int rate_iters, uint32_t seed, bgc_lds_result* out) {
  return lds_run(device, wgs_per_cu, rate_iters, seed, nullptr, 0, out);
}

int bgc_diag_lds_planted(int device, int wgs_per_cu, int rate_iters, uint32_t seed, const bgc_lds_plant* plants, int n,
                         bgc_lds_result* out) {
  return lds_run(device, wgs_per_cu, rate_iters, seed, plants, n, out);
}

int bgc_diag_lds_data(int device, uint32_t seed, int wg, int pass, int grid, void* data) {
  if (!data || grid < 1 || grid > 4096 || wg < 0 || wg >= grid || (pass != 0 && pass != 1)) {
    g_last_error = "invalid arguments";
    return 1;
  }
  HIP_TRY(hipSetDevice(device));
  DeviceBuffer bins, dump;
  HIP_TRY(alloc_march_bins(bins));
  HIP_TRY(dump.alloc(4 * kWords, true));
  launch_march(grid, seed, bins.as<MarchBin>(), LdsDump{wg, pass, dump.as<u32x4>()});
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(data, dump.p, 4 * kWords, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
