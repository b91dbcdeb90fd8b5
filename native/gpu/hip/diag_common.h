// Shared by the diagnostics' sources (gpu_diag.hip, hbm.hip, mfma.hip, lds.hip, cache.hip, valu.hip, atomic.hip, regfile.hip, xlane.hip, gemm_soak.hip): vector
// types, the hash, the CU a wave runs on, the marches' pattern and wrong-word record, the delay plants' wait, a rate
// launch's timing bin, the last-error string and the host helpers every entry point uses: device buffers and events,
// the test plants' list, upload and beyond-the-launch refusal, the constant clock's rate, the rate formula and
// (diag_fold.h) the fold of the timing bins.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "diag_fold.h"
#include "gpu_diag.h"

// The two types that kernels of several sources take as arguments.  They are in the unnamed namespace, where every
// source has its kernels: a kernel's symbol names its argument types, and so stays what it is whichever file
// declares them.
namespace {

// A rate launch's timing bin of one key (a CU: cu_key(), or an XCC: xcc_id()): the ticks of the constant clock that
// the `n` workgroups or waves that ran there took in all.  TimingFold (diag_fold.h) folds the bins.
struct RateBin {
  unsigned long long ticks;
  unsigned n, pad;
};

// Test plants (gpu_diag.h, "planted variants") in device memory.  The planted instantiation of a kernel takes one.
template <class P>
struct PlantList {
  const P* p = nullptr;
  int n = 0;
};

}  // namespace

namespace bgc_diag __attribute__((visibility("hidden"))) {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int8_t i8x16 __attribute__((ext_vector_type(16)));
typedef float f32x1 __attribute__((ext_vector_type(1)));
typedef double f64x1 __attribute__((ext_vector_type(1)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;

extern thread_local std::string g_last_error;  // gpu_diag.hip; read by bgc_diag_last_error()

__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// The physical CU a wave runs on: xcc << 8 | se << 5 | sh << 4 | cu, below BGC_DIAG_MAX_CU_KEYS.
__device__ __forceinline__ uint32_t cu_key() {
  uint32_t xcc, hwid;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  uint32_t cu = (hwid >> 8) & 0xF;
  uint32_t sh = (hwid >> 12) & 0x1;
  uint32_t se = (hwid >> 13) & 0x7;
  return ((xcc & 0x7) << 8) | (se << 5) | (sh << 4) | cu;
}

// The SIMD (0..3) of its CU that a wave runs on: HW_REG_HW_ID bits 5:4, in the GFX9 layout whose CU, SH and SE fields
// cu_key() uses.
__device__ __forceinline__ uint32_t simd_id() {
  uint32_t hwid;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  return (hwid >> 4) & 0x3;
}

// The XCC (0..7) a wave runs on: the owner of the L2 it reads and writes through.
__device__ __forceinline__ uint32_t xcc_id() { return cu_key() >> 8; }

// A delay plant's wait (gpu_diag.h): until `ticks` of the constant clock have passed since this
// point.  The clock difference is the loop's only exit condition, so it ends after `ticks` (checked
// on the host) whatever else happens.
__device__ __forceinline__ void wait_ticks(uint32_t ticks) {
  const uint64_t t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// words 4 e .. 4 e + 3 of a hash pattern with seed s (mix32(word ^ s)), XOR `inv` (0, or ~0 for the inverse)
__device__ __forceinline__ u32x4 pattern16(uint32_t e, uint32_t s, uint32_t inv) {
  const uint32_t w = 4 * e;
  return u32x4{mix32(w ^ s) ^ inv, mix32((w + 1) ^ s) ^ inv, mix32((w + 2) ^ s) ^ inv, mix32((w + 3) ^ s) ^ inv};
}

// a thread's (then a wave's, then a workgroup's) wrong words of a march
struct BadWords {
  unsigned count = 0, bits = 0, first = ~0u;
  __device__ __forceinline__ void check(uint32_t word, uint32_t expected, uint32_t found) {
    if (expected != found) {
      count++;
      bits |= expected ^ found;
      first = min(first, word);
    }
  }
  __device__ __forceinline__ void merge(unsigned c, unsigned b, unsigned f) {
    count += c;
    bits |= b;
    first = min(first, f);
  }
  // the sum over the wave, in its lane 0
  __device__ __forceinline__ void merge_wave() {
    for (int off = 32; off > 0; off >>= 1) merge(__shfl_down(count, off, 64), __shfl_down(bits, off, 64), __shfl_down(first, off, 64));
  }
};

#define HIP_TRY(expr)                                                                  \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      bgc_diag::g_last_error = std::string(#expr) + ": " + hipGetErrorString(_e);       \
      return 1;                                                                         \
    }                                                                                   \
  } while (0)

inline int cu_count(int device) {
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
  return n;
}

struct DeviceBuffer {
  void* p = nullptr;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  hipError_t alloc(size_t bytes, bool zero = false) {
    const hipError_t e = hipMalloc(&p, bytes);
    return e == hipSuccess && zero ? hipMemset(p, 0, bytes) : e;
  }
  // `n` copies of `init`: bins whose `first` starts at ~0
  template <class T>
  hipError_t alloc_filled(size_t n, const T& init) {
    const std::vector<T> host(n, init);
    const hipError_t e = alloc(n * sizeof(T));
    return e == hipSuccess ? hipMemcpy(p, host.data(), n * sizeof(T), hipMemcpyHostToDevice) : e;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
};

struct Events {
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t create() {
    const hipError_t e = hipEventCreate(&a);
    return e == hipSuccess ? hipEventCreate(&b) : e;
  }
  ~Events() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

// Device time of `launch` (kernel launches, or one async copy whose hipError_t it returns) on
// stream `s`.  Non-zero with the last error set on any HIP failure, the launch's included.
template <class Launch>
int timed(const Events& ev, float* ms, Launch&& launch, hipStream_t s = nullptr) {
  HIP_TRY(hipEventRecord(ev.a, s));
  if constexpr (std::is_void_v<decltype(launch())>) {
    launch();
  } else {
    HIP_TRY(launch());
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ev.b, s));
  HIP_TRY(hipEventSynchronize(ev.b));
  HIP_TRY(hipEventElapsedTime(ms, ev.a, ev.b));
  return 0;
}

// One more bad CU of a result: counted, and its key kept while bad_cu_keys has room.
template <class Result>
void note_bad_cu(Result* out, int key) {
  if (out->bad_cus < 64) out->bad_cu_keys[out->bad_cus] = key;
  out->bad_cus++;
}

// Test plants (gpu_diag.h, "planted variants").  A plant list is `n` entries at `plants`.
inline bool plant_list_ok(const void* plants, int n) {
  return n >= 0 && n <= BGC_DIAG_MAX_PLANTS && (n == 0 || plants);
}

// A plant list in device memory (nothing for an empty one).
template <class P>
int upload_plants(DeviceBuffer& d, const P* plants, int n) {
  if (n == 0) return 0;
  HIP_TRY(d.alloc(static_cast<size_t>(n) * sizeof(P)));
  HIP_TRY(hipMemcpy(d.p, plants, static_cast<size_t>(n) * sizeof(P), hipMemcpyHostToDevice));
  return 0;
}

// Whether a plant names a wave or a workgroup (its member `place`) that a launch of `limit` of them does not have;
// the caller then refuses, once the launch size is known, with one of the two texts.
constexpr const char* kWaveBeyond = "invalid arguments: plant in a wave beyond the launch";
constexpr const char* kWorkgroupBeyond = "invalid arguments: plant in a workgroup beyond the launch";
template <class P>
bool any_beyond(const P* plants, size_t n, int P::*place, int limit) {
  return std::any_of(plants, plants + n, [&](const P& p) { return p.*place >= limit; });
}
inline int refuse(const char* why) {
  g_last_error = why;
  return 1;
}

// kHz of the constant clock that wall_clock64() reads
inline int constant_clock_khz(int device) {
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) khz = 100000;  // CDNA: 100 MHz
  return khz;
}

// 1e12 operations or bytes per second: `x` of them in `ms`
inline double tera_per_s(double x, float ms) { return ms > 0 ? x / (ms * 1e-3) / 1e12 : 0.0; }

// *p = f(*p) on one value in device memory: a host read-modify-write on the null stream, so it is
// ordered after the null-stream kernels that produced the data and before those that check it.
template <class T, class F>
int modify_device_value(T* p, F&& f) {
  T v;
  HIP_TRY(hipMemcpy(&v, p, sizeof(v), hipMemcpyDeviceToHost));
  v = f(v);
  HIP_TRY(hipMemcpy(p, &v, sizeof(v), hipMemcpyHostToDevice));
  return 0;
}

// A GEMM on caller operands: upload `in`, poison C (float or double) with 0xFF (NaN: an element the kernel never
// writes cannot pass), launch(device operands in order, device C), download C.
struct HostOperand {
  const void* p;
  size_t bytes;
};

template <class C, class Launch>
int gemm_on_host_operands(std::initializer_list<HostOperand> in, C* c, size_t c_elems, Launch&& launch) {
  std::vector<DeviceBuffer> d(in.size());
  std::vector<const void*> dp;
  for (const HostOperand& h : in) {
    DeviceBuffer& buf = d[dp.size()];
    HIP_TRY(buf.alloc(h.bytes));
    HIP_TRY(hipMemcpy(buf.p, h.p, h.bytes, hipMemcpyHostToDevice));
    dp.push_back(buf.p);
  }
  DeviceBuffer dc;
  HIP_TRY(dc.alloc(c_elems * sizeof(C)));
  HIP_TRY(hipMemset(dc.p, 0xFF, c_elems * sizeof(C)));
  launch(dp.data(), dc.as<C>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(c, dc.p, c_elems * sizeof(C), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace bgc_diag
