// HBM3E bandwidth (bgc_diag_hbm), the address-in-data walk over free VRAM (bgc_diag_hbm_walk)
// and pinned host<->device copies over PCIe (bgc_diag_pcie).
//
// HBM phases are pure streams: 16 B per lane (global_load/store_dwordx4), 256-thread blocks,
// 8 blocks per CU (2048 WGs >> 256 CUs) each owning one contiguous slab, 4 independent 16 B
// accesses in flight per lane so each CU keeps ~128 KiB outstanding; nontemporal hints since
// every byte is touched exactly once per pass.  The bandwidth phases run on two buffers of
// `bytes` each (the node agent uses 1 GiB, 4x the 256 MiB Infinity Cache, so the rates are
// HBM rates); coverage of the whole HBM is the job of the separate address-pattern walk over
// ~all free VRAM (walk_fill / walk_check).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <utility>

#include "diag_common.h"

namespace {

using namespace bgc_diag;

constexpr int kUnroll = 4;

__device__ __forceinline__ u32x4 pattern16(uint64_t i, uint32_t seed) {
  uint32_t w = static_cast<uint32_t>(i << 2) ^ static_cast<uint32_t>(i >> 30) * 0x9e3779b9U;
  u32x4 v;
  v.x = mix32(w ^ seed);
  v.y = mix32((w + 1) ^ seed);
  v.z = mix32((w + 2) ^ seed);
  v.w = mix32((w + 3) ^ seed);
  return v;
}

// Each block streams one contiguous slab (per-block chunking keeps DRAM pages open and
// measured 5.57 TB/s copy / 6.19 TB/s read on MI355X vs 5.08 / 5.61 for a grid-stride
// interleave — tools/probes/hbm_sweep.hip, profiles/archive/hbm_sweep_r1.jsonl).  Per step a
// lane handles kUnroll 16-byte elements kBlock apart and calls consume(i) on each; with kLoad all
// of them are loaded from src[i] before the first consume(i, value), so a copy keeps kUnroll
// loads in flight.
template <bool kLoad, class Consume>
__device__ __forceinline__ void slab_stream(const u32x4* src, uint64_t n16, Consume consume) {
  const uint64_t per = (n16 + gridDim.x - 1) / gridDim.x;
  const uint64_t beg = static_cast<uint64_t>(blockIdx.x) * per;
  const uint64_t end = beg + per < n16 ? beg + per : n16;
  for (uint64_t b = beg + threadIdx.x; b < end; b += kBlock * kUnroll) {
    u32x4 v[kUnroll];
    if constexpr (kLoad) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint64_t i = b + u * kBlock;
        if (i < end) v[u] = __builtin_nontemporal_load(&src[i]);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint64_t i = b + u * kBlock;
      if (i < end) {
        if constexpr (kLoad) consume(i, v[u]);
        else consume(i);
      }
    }
  }
}

// a lane's wrong words and the lowest of them
struct BadCount {
  unsigned long long count = 0, first = ~0ULL;
  __device__ __forceinline__ void add(unsigned long long n, unsigned long long where) {
    count += n;
    first = std::min(first, where);
  }
  __device__ __forceinline__ void report(unsigned long long* bad, unsigned long long* first_bad) const {
    if (count) {
      atomicAdd(bad, count);
      atomicMin(first_bad, first);
    }
  }
};

__global__ __launch_bounds__(kBlock) void hbm_fill(u32x4* __restrict__ buf, uint64_t n16, uint32_t seed) {
  slab_stream<false>(nullptr, n16, [=](uint64_t i) { __builtin_nontemporal_store(pattern16(i, seed), &buf[i]); });
}

__global__ __launch_bounds__(kBlock) void hbm_copy(const u32x4* __restrict__ src, u32x4* __restrict__ dst, uint64_t n16) {
  slab_stream<true>(src, n16, [=](uint64_t i, const u32x4& v) { __builtin_nontemporal_store(v, &dst[i]); });
}

__global__ __launch_bounds__(kBlock) void hbm_check(const u32x4* __restrict__ buf, uint64_t n16, uint32_t seed,
                                                    unsigned long long* __restrict__ bad,
                                                    unsigned long long* __restrict__ first_bad) {
  BadCount w;
  slab_stream<true>(buf, n16, [=, &w](uint64_t i, const u32x4& v) {
    const u32x4 e = pattern16(i, seed);
    const int nb = (v.x != e.x) + (v.y != e.y) + (v.z != e.z) + (v.w != e.w);
    if (nb) w.add(nb, i * 4 + (v.x != e.x ? 0 : v.y != e.y ? 1 : v.z != e.z ? 2 : 3));
  });
  w.report(bad, first_bad);
}

// ---------------------------------------------------------------------------
// HBM walk (bgc_diag_hbm_walk): every 64-bit word holds its own device address ^ key.
// A stuck bit, a weak cell or a write that decodes to the wrong row/bank/stack shows up
// at verify time as a word whose content is not its address.  The inverse pass is the
// same kernel with ~key, so every bit is checked at 0 and at 1.

__device__ __forceinline__ u32x4 walk_value(const u32x4* p, uint64_t key) {
  const uint64_t a = reinterpret_cast<uint64_t>(p);
  const uint64_t w0 = a ^ key, w1 = (a + 8) ^ key;
  u32x4 v;
  v.x = static_cast<uint32_t>(w0);
  v.y = static_cast<uint32_t>(w0 >> 32);
  v.z = static_cast<uint32_t>(w1);
  v.w = static_cast<uint32_t>(w1 >> 32);
  return v;
}

__global__ __launch_bounds__(kBlock) void walk_fill(u32x4* __restrict__ buf, uint64_t n16, uint64_t key) {
  slab_stream<false>(nullptr, n16, [=](uint64_t i) { __builtin_nontemporal_store(walk_value(&buf[i], key), &buf[i]); });
}

__global__ __launch_bounds__(kBlock) void walk_check(const u32x4* __restrict__ buf, uint64_t n16, uint64_t key,
                                                     unsigned long long* __restrict__ bad,
                                                     unsigned long long* __restrict__ first_bad_addr) {
  BadCount w;
  slab_stream<true>(buf, n16, [=, &w](uint64_t i, const u32x4& v) {
    const u32x4 e = walk_value(&buf[i], key);
    const bool b0 = v.x != e.x || v.y != e.y, b1 = v.z != e.z || v.w != e.w;
    if (b0 || b1) w.add(static_cast<unsigned long long>(b0) + b1, reinterpret_cast<uint64_t>(&buf[i]) + (b0 ? 0 : 8));
  });
  w.report(bad, first_bad_addr);
}

struct HostBuffer {  // pinned: DMA straight from/to it, no staging copy
  void* p = nullptr;
  ~HostBuffer() {
    if (p) (void)hipHostFree(p);
  }
};

struct Streams {
  hipStream_t a = nullptr, b = nullptr;
  hipError_t create() {
    const hipError_t e = hipStreamCreateWithFlags(&a, hipStreamNonBlocking);
    return e == hipSuccess ? hipStreamCreateWithFlags(&b, hipStreamNonBlocking) : e;
  }
  ~Streams() {
    if (a) (void)hipStreamDestroy(a);
    if (b) (void)hipStreamDestroy(b);
  }
};

struct Chunks {  // the HBM walk's allocations, freed on every exit path
  std::vector<std::pair<void*, uint64_t>> v;
  ~Chunks() {
    for (auto& c : v) (void)hipFree(c.first);
  }
};

// {bad words, first bad} counters of the check kernels, as they start
struct Counters {
  unsigned long long bad = 0, first = ~0ULL;
};

uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

// bgc_diag_hbm, bgc_diag_hbm_planted with its test plants XORed into the copy before each check, and
// bgc_diag_hbm_data with the copy downloaded to `dump` at the end
int hbm_run(int device, uint64_t bytes, int iters, uint32_t seed, const bgc_hbm_plant* plants, int n, void* dump,
            bgc_hbm_result* out) {
  bool ok = out && iters > 0 && bytes >= (1u << 20) && plant_list_ok(plants, n);
  bytes &= ~static_cast<uint64_t>(15);
  for (int j = 0; ok && j < n; ++j) ok = plants[j].word32_index < bytes / 4;
  if (!ok) {
    g_last_error = "invalid arguments";
    return 1;
  }
  std::memset(out, 0, sizeof(*out));
  const uint64_t n16 = bytes / 16;
  HIP_TRY(hipSetDevice(device));
  DeviceBuffer a, b, counters;
  HIP_TRY(a.alloc(bytes));
  HIP_TRY(b.alloc(bytes));
  HIP_TRY(counters.alloc_filled(1, Counters{}));
  auto* bad = counters.as<unsigned long long>();
  const dim3 grid(cu_count(device) * 8), block(kBlock);
  Events ev;
  HIP_TRY(ev.create());
  float best_fill = 1e30f, best_copy = 1e30f, best_check = 1e30f, total = 0.f;
  // Every fill gets a pattern seed of its own (gpu_diag.h: the warm-up is iteration -1), and both
  // buffers start out poisoned: a fill or a copy that wrote nothing leaves data that differs from
  // what the check expects in every word, whatever the pages or an earlier iteration held.
  auto pattern_seed = [=](int it) { return mix32(seed + static_cast<uint32_t>(it + 1) * 0x9e3779b9U); };
  uint32_t pseed = pattern_seed(-1);
  HIP_TRY(hipMemset(a.p, 0xFF, bytes));
  HIP_TRY(hipMemset(b.p, 0xFF, bytes));
  auto fill = [&] { hipLaunchKernelGGL(hbm_fill, grid, block, 0, nullptr, a.as<u32x4>(), n16, pseed); };
  auto copy = [&] { hipLaunchKernelGGL(hbm_copy, grid, block, 0, nullptr, a.as<const u32x4>(), b.as<u32x4>(), n16); };
  auto check = [&] { hipLaunchKernelGGL(hbm_check, grid, block, 0, nullptr, b.as<const u32x4>(), n16, pseed, bad, bad + 1); };
  auto phase = [&](auto& launch, float* best) {
    float ms = 0.f;
    if (timed(ev, &ms, launch) != 0) return 1;
    *best = std::min(*best, ms);
    total += ms;
    return 0;
  };
  fill();  // warm-up (also first-touch of the pages)
  HIP_TRY(hipGetLastError());
  for (int it = 0; it < iters; ++it) {
    pseed = pattern_seed(it);
    if (phase(fill, &best_fill) != 0 || phase(copy, &best_copy) != 0) return 1;
    for (int j = 0; j < n; ++j) {
      const uint32_t mask = plants[j].xor_mask;
      if (modify_device_value(b.as<uint32_t>() + plants[j].word32_index, [=](uint32_t w) { return w ^ mask; }) != 0) return 1;
    }
    if (phase(check, &best_check) != 0) return 1;
  }
  unsigned long long res[2];
  HIP_TRY(hipMemcpy(res, bad, sizeof(res), hipMemcpyDeviceToHost));
  if (dump) HIP_TRY(hipMemcpy(dump, b.p, bytes, hipMemcpyDeviceToHost));
  out->bytes = bytes;
  out->iters = iters;
  out->write_gbps = static_cast<double>(bytes) / (best_fill * 1e-3) / 1e9;
  out->copy_gbps = 2.0 * static_cast<double>(bytes) / (best_copy * 1e-3) / 1e9;
  out->read_gbps = static_cast<double>(bytes) / (best_check * 1e-3) / 1e9;
  out->mismatches = res[0];
  out->first_bad_word = res[1];
  out->elapsed_ms = total;
  return 0;
}

constexpr uint64_t kMinChunk = 64ULL << 20;
constexpr uint64_t kWalkAlign = 2ULL << 20;

// The walk over `target_bytes`, or over `fraction` of the free VRAM when that is 0 (arguments
// checked by the callers).  Test plants are XORed in after their pass's fill; with any, the
// allocations must come out as `target_bytes` and `chunk_bytes` imply, since the plants were
// checked against that layout.  The walk ends after `passes` passes; with `dump` every chunk's
// contents are then downloaded to it back to back, and the allocations must come out as implied too.
int walk_run(int device, double fraction, uint64_t target_bytes, uint64_t chunk_bytes, int budget_ms, uint32_t seed,
             const bgc_walk_plant* plants, int n, bgc_walk_chunk* chunks_out, int max_chunks, int passes, void* dump,
             bgc_hbm_walk_result* out) {
  std::memset(out, 0, sizeof(*out));
  const auto t0 = std::chrono::steady_clock::now();
  auto elapsed_ms = [&] {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  HIP_TRY(hipSetDevice(device));
  DeviceBuffer counters;  // before the walk takes the memory
  HIP_TRY(counters.alloc(2 * sizeof(unsigned long long)));
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  out->free_bytes = free_b;
  out->total_bytes = total_b;
  const uint64_t align = kWalkAlign;
  const uint64_t target = (target_bytes ? target_bytes : static_cast<uint64_t>(fraction * static_cast<double>(free_b))) & ~(align - 1);
  out->target_bytes = target;
  Chunks chunks;
  uint64_t got = 0, cb = chunk_bytes & ~(align - 1);
  while (got < target) {
    const uint64_t want = std::min(cb, target - got);
    void* p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess || !p) {
      (void)hipGetLastError();  // clear the sticky allocation error
      if (cb <= kMinChunk) break;
      cb = std::max(kMinChunk, (cb / 2) & ~(align - 1));
      continue;
    }
    chunks.v.emplace_back(p, want);
    got += want;
  }
  if (chunks.v.empty()) {
    g_last_error = "hbm walk: no device memory could be allocated";
    return 1;
  }
  out->chunks = static_cast<int>(chunks.v.size());
  out->alloc_ms = elapsed_ms();
  for (int c = 0; c < out->chunks && c < max_chunks; ++c) {
    chunks_out[c] = {reinterpret_cast<uint64_t>(chunks.v[static_cast<size_t>(c)].first), chunks.v[static_cast<size_t>(c)].second};
  }
  if ((n > 0 || dump) && (got != target || cb != (chunk_bytes & ~(align - 1)))) {
    g_last_error = "hbm walk: the chunks could not be allocated as the plants assume";
    return 1;
  }
  auto* bad = counters.as<unsigned long long>();
  const dim3 grid(cu_count(device) * 8), block(kBlock);
  Events ev;
  HIP_TRY(ev.create());
  const uint64_t key0 = mix64(0x9e3779b97f4a7c15ULL ^ seed);
  double fill_ms = 0, check_ms = 0;
  for (int pass = 0; pass < passes; ++pass) {
    if (pass > 0 && elapsed_ms() > budget_ms) {
      out->budget_hit = 1;
      break;
    }
    const uint64_t key = pass == 0 ? key0 : ~key0;
    const Counters none;
    HIP_TRY(hipMemcpy(bad, &none, sizeof(none), hipMemcpyHostToDevice));
    float ms = 0.f;
    if (timed(ev, &ms, [&] {
          for (const auto& c : chunks.v) {
            hipLaunchKernelGGL(walk_fill, grid, block, 0, nullptr, static_cast<u32x4*>(c.first), c.second / 16, key);
          }
        }) != 0) {
      return 1;
    }
    fill_ms += ms;
    for (int j = 0; j < n; ++j) {
      if (plants[j].pass != pass) continue;
      const uint64_t mask = plants[j].xor_mask;
      auto* word = static_cast<uint64_t*>(chunks.v[static_cast<size_t>(plants[j].chunk)].first) + plants[j].word64_offset;
      if (modify_device_value(word, [=](uint64_t w) { return w ^ mask; }) != 0) return 1;
    }
    if (timed(ev, &ms, [&] {
          for (const auto& c : chunks.v) {
            hipLaunchKernelGGL(walk_check, grid, block, 0, nullptr, static_cast<const u32x4*>(c.first), c.second / 16, key,
                               bad, bad + 1);
          }
        }) != 0) {
      return 1;
    }
    check_ms += ms;
    unsigned long long res[2];
    HIP_TRY(hipMemcpy(res, bad, sizeof(res), hipMemcpyDeviceToHost));
    if (res[0] && !out->mismatches) {  // the first failing pass names the first bad word
      out->first_bad_addr = res[1];
      uint64_t found = 0;
      HIP_TRY(hipMemcpy(&found, reinterpret_cast<void*>(static_cast<uintptr_t>(res[1])), 8, hipMemcpyDeviceToHost));
      out->first_bad_xor = found ^ (static_cast<uint64_t>(res[1]) ^ key);
    }
    out->mismatches += res[0];
    out->passes = pass + 1;
  }
  if (dump) {
    char* to = static_cast<char*>(dump);
    for (const auto& c : chunks.v) {
      HIP_TRY(hipMemcpy(to, c.first, c.second, hipMemcpyDeviceToHost));
      to += c.second;
    }
  }
  out->bytes_covered = got;
  const double moved = static_cast<double>(got) * out->passes;
  out->write_gbps = fill_ms > 0 ? moved / (fill_ms * 1e-3) / 1e9 : 0.0;
  out->read_gbps = check_ms > 0 ? moved / (check_ms * 1e-3) / 1e9 : 0.0;
  out->elapsed_ms = elapsed_ms();
  return 0;
}

// bgc_diag_pcie, bgc_diag_pcie_planted with its test plants XORed into the uploaded buffer, and
// bgc_diag_pcie_data with the buffer that came back copied to `dump` after the round-trip check
int pcie_run(int device, uint64_t bytes, int iters, uint32_t seed, const bgc_pcie_plant* plants, int n, void* dump,
             bgc_pcie_result* out) {
  bool ok = out && iters > 0 && bytes >= (1u << 20) && bytes <= (uint64_t{16} << 30) && plant_list_ok(plants, n);
  bytes &= ~static_cast<uint64_t>(7);
  const uint64_t words = bytes / 8;
  for (int j = 0; ok && j < n; ++j) ok = plants[j].word64_index < words;
  if (!ok) {
    g_last_error = "invalid arguments";
    return 1;
  }
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(device));
  HostBuffer src, dst, src2;
  DeviceBuffer d1, d2;
  HIP_TRY(hipHostMalloc(&src.p, bytes, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc(&dst.p, bytes, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc(&src2.p, bytes, hipHostMallocDefault));
  HIP_TRY(d1.alloc(bytes));
  HIP_TRY(d2.alloc(bytes));
  auto* s64 = static_cast<uint64_t*>(src.p);
  // words <= 2^31 (16 GiB), so the low 32 bits of i are all of it: both halves differ from word to word
  for (uint64_t i = 0; i < words; ++i) {
    const uint32_t x = static_cast<uint32_t>(i);
    s64[i] = (static_cast<uint64_t>(mix32(x ^ seed)) << 32) | mix32(x ^ ~seed);
  }
  std::memset(dst.p, 0, bytes);
  std::memset(src2.p, 0x5a, bytes);
  Streams st;
  HIP_TRY(st.create());
  Events ev, ev2;
  HIP_TRY(ev.create());
  HIP_TRY(ev2.create());
  // warm-up both directions (page tables, DMA engine clocks)
  HIP_TRY(hipMemcpyAsync(d1.p, src.p, bytes, hipMemcpyHostToDevice, st.a));
  if (n > 0) HIP_TRY(hipStreamSynchronize(st.a));  // the upload has landed; the copies below are issued after the plants
  for (int j = 0; j < n; ++j) {
    const uint64_t mask = plants[j].xor_mask;
    if (modify_device_value(d1.as<uint64_t>() + plants[j].word64_index, [=](uint64_t w) { return w ^ mask; }) != 0) return 1;
  }
  HIP_TRY(hipMemcpyAsync(d2.p, d1.p, bytes, hipMemcpyDeviceToDevice, st.a));
  HIP_TRY(hipMemcpyAsync(dst.p, d2.p, bytes, hipMemcpyDeviceToHost, st.a));
  HIP_TRY(hipStreamSynchronize(st.a));
  // round trip check: the pattern went host -> device -> device -> host
  const auto* d64 = static_cast<const uint64_t*>(dst.p);
  uint64_t bad = 0;
  for (uint64_t i = 0; i < words; ++i) bad += d64[i] != s64[i];
  if (dump) std::memcpy(dump, dst.p, bytes);
  float best_h2d = 1e30f, best_d2h = 1e30f, ms = 0.f, total = 0.f;
  double best_bidir = 0;
  for (int it = 0; it < iters; ++it) {
    if (timed(ev, &ms, [&] { return hipMemcpyAsync(d1.p, src.p, bytes, hipMemcpyHostToDevice, st.a); }, st.a) != 0) return 1;
    best_h2d = std::min(best_h2d, ms);
    total += ms;
    if (timed(ev, &ms, [&] { return hipMemcpyAsync(dst.p, d1.p, bytes, hipMemcpyDeviceToHost, st.a); }, st.a) != 0) return 1;
    best_d2h = std::min(best_d2h, ms);
    total += ms;
    // both directions at once: H2D on one stream, D2H on the other
    HIP_TRY(hipEventRecord(ev.a, st.a));
    HIP_TRY(hipEventRecord(ev2.a, st.b));
    HIP_TRY(hipMemcpyAsync(d2.p, src2.p, bytes, hipMemcpyHostToDevice, st.a));
    HIP_TRY(hipMemcpyAsync(dst.p, d1.p, bytes, hipMemcpyDeviceToHost, st.b));
    HIP_TRY(hipEventRecord(ev.b, st.a));
    HIP_TRY(hipEventRecord(ev2.b, st.b));
    HIP_TRY(hipEventSynchronize(ev.b));
    HIP_TRY(hipEventSynchronize(ev2.b));
    float ms_a = 0.f, ms_b = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms_a, ev.a, ev.b));
    HIP_TRY(hipEventElapsedTime(&ms_b, ev2.a, ev2.b));
    const double span = std::max(ms_a, ms_b);
    best_bidir = std::max(best_bidir, 2.0 * static_cast<double>(bytes) / (span * 1e-3) / 1e9);
    total += static_cast<float>(span);
  }
  HIP_TRY(hipGetLastError());
  out->bytes = bytes;
  out->iters = iters;
  out->h2d_gbps = static_cast<double>(bytes) / (best_h2d * 1e-3) / 1e9;
  out->d2h_gbps = static_cast<double>(bytes) / (best_d2h * 1e-3) / 1e9;
  out->bidir_gbps = best_bidir;
  out->mismatches = bad;
  out->elapsed_ms = total;
  return 0;
}

}  // namespace

extern "C" {

int bgc_diag_hbm(int device, uint64_t bytes, int iters, uint32_t seed, bgc_hbm_result* out) {
  return hbm_run(device, bytes, iters, seed, nullptr, 0, nullptr, out);
}

int bgc_diag_hbm_planted(int device, uint64_t bytes, uint32_t seed, const bgc_hbm_plant* plants, int n, bgc_hbm_result* out) {
  return hbm_run(device, bytes, 1, seed, plants, n, nullptr, out);
}

int bgc_diag_hbm_walk(int device, double fraction, uint64_t chunk_bytes, int budget_ms, uint32_t seed,
                      bgc_hbm_walk_result* out) {
  if (!out || !(fraction > 0.0 && fraction <= 0.99) || chunk_bytes < kMinChunk || budget_ms <= 0) {
    g_last_error = "invalid arguments: 0 < fraction <= 0.99, chunk_bytes >= 64 MiB, budget_ms > 0";
    return 1;
  }
  return walk_run(device, fraction, 0, chunk_bytes, budget_ms, seed, nullptr, 0, nullptr, 0, 2, nullptr, out);
}

int bgc_diag_hbm_walk_planted(int device, uint64_t bytes, uint64_t chunk_bytes, uint32_t seed, const bgc_walk_plant* plants,
                              int n, bgc_walk_chunk* chunks, int max_chunks, bgc_hbm_walk_result* out) {
  const uint64_t target = bytes & ~(kWalkAlign - 1), cb = chunk_bytes & ~(kWalkAlign - 1);
  bool ok = out && target > 0 && target <= (1ULL << 40) && chunk_bytes >= kMinChunk && plant_list_ok(plants, n) &&
            max_chunks >= 0 && (max_chunks == 0 || chunks);
  const uint64_t n_chunks = ok ? (target + cb - 1) / cb : 0;  // as the allocation loop splits the target
  for (int j = 0; ok && j < n; ++j) {
    const bgc_walk_plant& p = plants[j];
    ok = (p.pass == 0 || p.pass == 1) && p.chunk >= 0 && static_cast<uint64_t>(p.chunk) < n_chunks &&
         p.word64_offset < std::min(cb, target - static_cast<uint64_t>(p.chunk) * cb) / 8;
  }
  if (!ok) {
    g_last_error = "invalid arguments: bytes >= 2 MiB, chunk_bytes >= 64 MiB, plants inside their chunk, pass 0 or 1";
    return 1;
  }
  return walk_run(device, 0.0, target, chunk_bytes, INT32_MAX, seed, plants, n, chunks, max_chunks, 2, nullptr, out);
}

int bgc_diag_pcie(int device, uint64_t bytes, int iters, uint32_t seed, bgc_pcie_result* out) {
  return pcie_run(device, bytes, iters, seed, nullptr, 0, nullptr, out);
}

int bgc_diag_pcie_planted(int device, uint64_t bytes, uint32_t seed, const bgc_pcie_plant* plants, int n, bgc_pcie_result* out) {
  return pcie_run(device, bytes, 1, seed, plants, n, nullptr, out);
}

int bgc_diag_hbm_data(int device, uint64_t bytes, int iters, uint32_t seed, void* data, bgc_hbm_result* out) {
  if (!data || bytes > BGC_DIAG_MAX_DATA_BYTES) {
    g_last_error = "invalid arguments";
    return 1;
  }
  return hbm_run(device, bytes, iters, seed, nullptr, 0, data, out);
}

int bgc_diag_hbm_walk_data(int device, uint64_t bytes, uint64_t chunk_bytes, int passes, uint32_t seed, bgc_walk_chunk* chunks,
                           int max_chunks, void* data, bgc_hbm_walk_result* out) {
  const uint64_t target = bytes & ~(kWalkAlign - 1), cb = chunk_bytes & ~(kWalkAlign - 1);
  if (!out || !data || !chunks || target == 0 || target > BGC_DIAG_MAX_DATA_BYTES || chunk_bytes < kMinChunk ||
      (passes != 1 && passes != 2) || max_chunks < 0 || static_cast<uint64_t>(max_chunks) < (target + cb - 1) / cb) {
    g_last_error = "invalid arguments: 2 MiB <= bytes <= 128 MiB, chunk_bytes >= 64 MiB, 1 or 2 passes, room for every chunk";
    return 1;
  }
  return walk_run(device, 0.0, target, chunk_bytes, INT32_MAX, seed, nullptr, 0, chunks, max_chunks, passes, data, out);
}

int bgc_diag_pcie_data(int device, uint64_t bytes, uint32_t seed, void* data, bgc_pcie_result* out) {
  if (!data || bytes > BGC_DIAG_MAX_DATA_BYTES) {
    g_last_error = "invalid arguments";
    return 1;
  }
  return pcie_run(device, bytes, 1, seed, nullptr, 0, data, out);
}

}  // extern "C"
