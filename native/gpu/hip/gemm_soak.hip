// GEMM soak (bgc_diag_gemm_soak) and the same kernels on caller operands (bgc_diag_gemm_tiled):
// the LDS-tiled 2-buffer gemm_soak, the 8-phase gemm_pingpong, and the ABFT checksum kernels.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "diag_common.h"

namespace {

using namespace bgc_diag;

// ---------------------------------------------------------------------------
// GEMM soak: an LDS-tiled bf16 MFMA GEMM run back to back, verified by checksums.
//
// Unlike mfma_throughput (operands in registers), this exercises the whole matrix path a
// training step uses: HBM -> LDS by global_load_lds (16 B per lane, no VGPR round trip),
// LDS -> VGPR fragment reads, MFMA, and C written back to HBM.
//  * Tile 128x128x64, 4 waves (2x2, 64x64 per wave = 4x4 accumulators of 16x16), two LDS
//    buffers (2 x 32 KiB): tile k+1 streams in while tile k is multiplied; one
//    vmcnt(0) + barrier per K-step.  64 KiB per block -> 2 blocks per CU.
//  * LDS image [128 rows][8 chunks of 16 B] with chunk p of row r holding source chunk
//    p ^ (r & 7): the 16 rows a fragment read touches land on distinct 16-B slots of the
//    bank row (linear rows 128 B apart would stack 8 deep).  glds writes lane-linear LDS,
//    so the swizzle is applied to the GLOBAL source address.
//  * B is given transposed (Bt[N][K]) so both operands are K-contiguous.
//  * Blocks are remapped XCD-aware (bijective for any grid) and grouped 8 tile-rows at a
//    time so the tiles sharing A rows / B columns run on one XCD's L2.
// Verification (ABFT): operands in {-1, 0, 1} make every C element an exact integer, so
// C's row sums must equal A * (B 1) and its column sums (1^T A) * B, both computed with
// integer kernels on a separate path; any wrong element shows in its row and its column.
constexpr int kSoakBK = 64;

__device__ __forceinline__ bf16x8 soak_frag(const char* base, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(base + row * 128 + ((chunk ^ (row & 7)) << 4));
}

// This block's output tile (tm, tn) of tiles_m x tiles_n: an XCD-aware bijective remap
// (consecutive ids of one XCD get consecutive tiles, for any grid), then a grouped ordering in
// which 8 tile-rows share each B column tile in L2.
__device__ __forceinline__ void soak_tile_of(int tiles_m, int tiles_n, int& tm, int& tn) {
  const int nwg = static_cast<int>(gridDim.x), orig = static_cast<int>(blockIdx.x);
  const int xcd = orig % 8, q = nwg / 8, r = nwg % 8;
  const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
  const int group = 8;
  const int per_group = group * tiles_n;
  const int first_m = (wgid / per_group) * group;
  const int gsize = min(tiles_m - first_m, group);
  tm = first_m + (wgid % per_group) % gsize;
  tn = (wgid % per_group) / gsize;
}

// kInstr global_load_lds wave-instructions of 8 rows x 128 B each: instruction i brings rows
// 8 (first8 + i * kStep8) .. +7 of the K-tile at src[row_base + row][k0 ..] into dst + row * 128.
// glds writes lane-linear LDS, so LDS slot (lane & 7) of a row takes source chunk slot ^ (row & 7).
template <int kInstr, int kStep8>
__device__ __forceinline__ void glds_rows(char* dst, const __bf16* src, int K, int row_base, int k0, int first8, int lane) {
#pragma unroll
  for (int i = 0; i < kInstr; ++i) {
    const int row0 = (first8 + i * kStep8) * 8;
    const int row = row0 + (lane >> 3);
    const int chunk = (lane & 7) ^ (row & 7);
    const __bf16* g = src + static_cast<size_t>(row_base + row) * K + k0 + chunk * 8;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)(dst + row0 * 128), 16, 0, 0);
  }
}

// BM x BN tile, WM x WN waves (each wave (BM/WM) x (BN/WN) outputs as 16x16 MFMA tiles).
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN, (BM * BN >= 256 * 256) ? 1 : 2) void gemm_soak(
    const __bf16* __restrict__ A, const __bf16* __restrict__ Bt, float* __restrict__ C, int M, int N, int K) {
  constexpr int kWaves = WM * WN;
  constexpr int kMI = BM / WM / 16, kNI = BN / WN / 16;
  constexpr int kA = BM * kSoakBK * 2, kB = BN * kSoakBK * 2;  // bytes per stage
  constexpr int kAInstr = BM / 8 / kWaves, kBInstr = BN / 8 / kWaves;  // 8 rows of 128 B per wave-instruction
  static_assert(BM % (8 * kWaves) == 0 && BN % (8 * kWaves) == 0, "tile rows must split over the waves");
  __shared__ __attribute__((aligned(16))) char lds[2 * (kA + kB)];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid / WN, wc = wid % WN;
  int tm, tn;
  soak_tile_of(M / BM, N / BN, tm, tn);

  // stage `buf` <- the K-tile at k0: A rows then Bt rows, split over the waves
  auto stage = [&](int buf, int k0) {
    char* a_l = lds + buf * (kA + kB);
    char* b_l = a_l + kA;
    glds_rows<kAInstr, 1>(a_l, A, K, tm * BM, k0, wid * kAInstr, lane);
    glds_rows<kBInstr, 1>(b_l, Bt, K, tn * BN, k0, wid * kBInstr, lane);
  };

  f32x4 acc[kMI][kNI];
#pragma unroll
  for (int mi = 0; mi < kMI; ++mi)
#pragma unroll
    for (int ni = 0; ni < kNI; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int kt_n = K / kSoakBK;
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < kt_n; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < kt_n) stage(buf ^ 1, (kt + 1) * kSoakBK);  // streams in under this tile's MFMAs
    const char* a_l = lds + buf * (kA + kB);
    const char* b_l = a_l + kA;
#pragma unroll
    for (int s = 0; s < 2; ++s) {  // two K=32 MFMA steps per 64-deep tile
      bf16x8 af[kMI], bfr[kNI];
#pragma unroll
      for (int mi = 0; mi < kMI; ++mi) af[mi] = soak_frag(a_l, wr * (BM / WM) + mi * 16 + (lane & 15), s * 4 + (lane >> 4));
#pragma unroll
      for (int ni = 0; ni < kNI; ++ni) bfr[ni] = soak_frag(b_l, wc * (BN / WN) + ni * 16 + (lane & 15), s * 4 + (lane >> 4));
#pragma unroll
      for (int mi = 0; mi < kMI; ++mi)
#pragma unroll
        for (int ni = 0; ni < kNI; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next tile has landed ...
    __syncthreads();                                   // ... and nobody still reads this one
  }
#pragma unroll
  for (int mi = 0; mi < kMI; ++mi)
#pragma unroll
    for (int ni = 0; ni < kNI; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const size_t row = static_cast<size_t>(tm * BM + wr * (BM / WM) + mi * 16 + (lane >> 4) * 4 + j);
        C[row * N + tn * BN + wc * (BN / WN) + ni * 16 + (lane & 15)] = acc[mi][ni][j];
      }
}

// ---------------------------------------------------------------------------
// 256x256 ping-pong GEMM: the soak's kernel whenever K is a multiple of 128.
//
// The 2-buffer kernel above drains every K-tile's loads (vmcnt(0) + barrier) one tile
// after issuing them; with one 512-thread block per CU a tile's 64 MFMAs per wave
// (~0.9 us per SIMD) do not cover an HBM/L2 fetch under full load, and the matrix pipe
// sat idle 42 % of the time (profiles/archive/gemm_soak_r2/pmc_soak_8192.json).  This kernel
// keeps the same LDS budget (two K-tiles, 128 KiB) but manages it in eight 16 KiB
// half-tiles (A rows 0-127 / 128-255, Bt rows 0-127 / 128-255 of each K-tile):
//
//  * Two wave groups, waves 0-3 (output rows 0-127) and 4-7 (rows 128-255): each SIMD
//    hosts one wave of each.  Group 1 runs one s_barrier behind group 0, so between any
//    two barriers one wave of a SIMD issues its 16 MFMAs while its partner issues LDS
//    fragment reads and global->LDS loads — matrix beside memory, never matrix beside
//    matrix.
//  * A phase is one C quadrant of the wave's 128x64 output (4x2 tiles of 16x16, K=64):
//    16 v_mfma_f32_16x16x32_bf16.  Eight phases = two K-tiles per loop iteration.
//    Fragments: all of the wave's B (64 columns) and half its A at phase 0, the other A
//    half at phase 2 (192 VGPRs: 128 accumulator, 32 A, 32 B).
//  * Two half-tile loads in every odd phase (the even phases carry all the fragment
//    reads), each into a half last read at least two barriers earlier (B halves are read
//    only in the first phase of a K-tile, A halves in the first and third).  Waits are
//    counted, vmcnt(4) at phases 3 and 7 (each half-tile is 2 glds per thread), and a
//    half is first read one phase after the wait that retires it; loads stay in flight
//    across the barriers.  All fragment reads happen in the even phases (16 at 0/4, 8 at
//    2/6; at four reading waves per CU, 16 take the partner's whole MFMA interval), which is
//    why the loads go to the odd ones (profiles/gemm_soak_r3/: +3-7 % at 4096^3, +0.5 % at
//    8192^3 over the first schedule, one half-tile in every phase).
//  * Staging past the last K-tile re-reads the last tile into a buffer nobody reads
//    again, so the vmcnt counts never change; the block drains (vmcnt(0)) before its
//    epilogue.
constexpr int kPPHalf = 128 * 128;  // one half-tile image: 128 rows x 64 k x 2 B

__device__ __forceinline__ void pp_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

__global__ __launch_bounds__(512, 1) void gemm_pingpong(const __bf16* __restrict__ A, const __bf16* __restrict__ Bt,
                                                        float* __restrict__ C, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) char lds[8 * kPPHalf];  // [buf][A_top, A_bot, B_left, B_right]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 2, wc = wid & 3;  // wave group = output row half
  int tm, tn;
  soak_tile_of(M / 256, N / 256, tm, tn);
  const int kt_n = K / kSoakBK;
  const int a_row = tm * 256, b_row = tn * 256;
  auto kofs = [&](int t) { return min(t, kt_n - 1) * kSoakBK; };
  // half-tile images of buffer b: A_top 4b, A_bot 4b+1, B_left 4b+2, B_right 4b+3; each is
  // 16 wave-instructions of 8 rows, two per wave
  auto stage = [&](int half, int t) {
    const int h = half & 3;
    char* dst = lds + half * kPPHalf;
    if (h < 2) glds_rows<2, 8>(dst, A, K, a_row + h * 128, kofs(t), wid, lane);
    else glds_rows<2, 8>(dst, Bt, K, b_row + (h - 2) * 128, kofs(t), wid, lane);
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int mi = 0; mi < 8; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 af[4][2], bfr[4][2];

  // prologue: K-tile 0 into buffer 0, K-tile 1's B halves into buffer 1
  stage(0, 0);
  stage(1, 0);
  stage(2, 0);
  stage(3, 0);
  stage(6, 1);
  stage(7, 1);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  pp_barrier();
  if (wr == 1) pp_barrier();  // the stagger: group 1 runs one barrier behind

  const int a_half = wr;            // A image this wave reads (per buffer)
  const int b_half = 2 + (wc >> 1);  // Bt image
  const int b_row0 = (wc & 1) * 64;  // first of the wave's 64 Bt rows inside that image

  for (int it = 0; it < kt_n / 2; ++it) {
    const int t_odd = 2 * it + 1, t_next = 2 * it + 2, t_next_odd = 2 * it + 3;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const char* buf = lds + (p >> 2) * 4 * kPPHalf;
      if ((p & 3) == 0) {  // all of B, rows 0-63 of A
        const char* bi = buf + b_half * kPPHalf;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) bfr[ni][ks] = soak_frag(bi, b_row0 + ni * 16 + (lane & 15), ks * 4 + (lane >> 4));
      }
      if ((p & 1) == 0) {  // phases 0/2 (4/6): the A half this quadrant pair needs
        const char* ai = buf + a_half * kPPHalf;
        const int m0 = (p & 2) ? 64 : 0;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) af[mi][ks] = soak_frag(ai, m0 + mi * 16 + (lane & 15), ks * 4 + (lane >> 4));
      }
      switch (p) {  // two half-tiles in every odd phase, each reloaded >= 2 barriers after its last read
        case 1: stage(4, t_odd); stage(5, t_odd); break;           // buffer 1 A (read at phase 4)
        case 3: stage(2, t_next); stage(3, t_next); break;         // buffer 0 B (last read at phase 0)
        case 5: stage(0, t_next); stage(1, t_next); break;         // buffer 0 A (last read at phase 2)
        case 7: stage(6, t_next_odd); stage(7, t_next_odd); break; // buffer 1 B (last read at phase 4)
        default: break;
      }
      if ((p & 3) == 3) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // retires everything through phase p-2
      pp_barrier();
      __builtin_amdgcn_s_setprio(1);
      const int mh = (p >> 1) & 1, nh = p & 1;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            acc[mh * 4 + mi][nh * 2 + ni] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mi][ks], bfr[nh * 2 + ni][ks], acc[mh * 4 + mi][nh * 2 + ni], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      pp_barrier();
    }
  }
  if (wr == 0) pp_barrier();  // matches group 1's extra barrier
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA may outlive the block
#pragma unroll
  for (int mi = 0; mi < 8; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const size_t row = static_cast<size_t>(a_row + wr * 128 + mi * 16 + (lane >> 4) * 4 + j);
        C[row * N + b_row + wc * 64 + ni * 16 + (lane & 15)] = acc[mi][ni][j];
      }
}

// X[rows][cols] = hash-derived values in {-1, 0, 1} (exact in bf16)
__global__ __launch_bounds__(kBlock) void soak_fill(__bf16* __restrict__ X, uint64_t n, uint32_t seed) {
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const uint32_t h = mix32(static_cast<uint32_t>(i) ^ mix32(static_cast<uint32_t>(i >> 32) + seed));
    X[i] = static_cast<__bf16>(static_cast<float>(static_cast<int>(h % 3u) - 1));
  }
}

// ABFT checksums, on integer paths: elements are exact integers held as bf16 (operands) or
// fp32 (C).
__device__ __forceinline__ long long as_int(__bf16 x) { return static_cast<int>(static_cast<float>(x)); }
__device__ __forceinline__ long long as_int(float x) { return llrintf(x); }
// An fp32 C element that is no exact integer (NaN and Inf included) is wrong whatever the sums
// say: as_int would round an error below 0.5, such as a flipped low mantissa bit, away.
__device__ __forceinline__ bool inexact(__bf16) { return false; }
__device__ __forceinline__ bool inexact(float x) { return x != rintf(x) || isinf(x); }

// out[c] += sum over a 64-row slab of X[r][c]  (column sums; atomics over the slabs.  Sum is int
// or unsigned long long: in two's complement signed sums add correctly).  flag[c], when given, is
// set if the column holds an inexact element.
template <class T, class Sum>
__global__ __launch_bounds__(kBlock) void soak_colsum(const T* __restrict__ X, int rows, int cols, Sum* __restrict__ out,
                                                      unsigned* __restrict__ flag = nullptr) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= cols) return;
  const int r0 = blockIdx.y * 64, r1 = min(rows, r0 + 64);
  Sum s = 0;
  bool odd = false;
  for (int r = r0; r < r1; ++r) {
    const T x = X[static_cast<size_t>(r) * cols + c];
    s += static_cast<Sum>(as_int(x));
    odd |= inexact(x);
  }
  atomicAdd(&out[c], s);
  if (flag && odd) atomicOr(&flag[c], 1u);
}

// out[r] = sum_k X[r][k] * w[k], or the plain row sum without w  (one block per row).  flag[r],
// when given, is set if the row holds an inexact element.
template <class T>
__global__ __launch_bounds__(kBlock) void soak_rowsum(const T* __restrict__ X, int cols, const int* __restrict__ w,
                                                      long long* __restrict__ out, unsigned* __restrict__ flag = nullptr) {
  __shared__ long long part[kBlock];
  const size_t base = static_cast<size_t>(blockIdx.x) * cols;
  long long s = 0;
  bool odd = false;
  for (int k = threadIdx.x; k < cols; k += kBlock) {
    const T x = X[base + k];
    s += as_int(x) * (w ? w[k] : 1);
    odd |= inexact(x);
  }
  if (flag && odd) atomicOr(&flag[blockIdx.x], 1u);
  part[threadIdx.x] = s;
  __syncthreads();
  for (int i = kBlock / 2; i > 0; i >>= 1) {
    if (static_cast<int>(threadIdx.x) < i) part[threadIdx.x] += part[threadIdx.x + i];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = part[0];
}

// Which GEMM the soak launches.  256x256 tiles (8 waves, 128 KiB LDS, 1 block/CU) when the
// shape divides, else 128x128; the ping-pong kernel whenever it can (256 tiles, K a multiple of
// two K-tiles).  BGC_SOAK_TILE=128 and BGC_SOAK_KERNEL=2buf keep the smaller tile / the
// double-buffered kernel for A/B runs.
enum class SoakKernel { k2Buf128, k2Buf256, kPingPong };

SoakKernel soak_kernel(int m, int n, int k) {
  const char* tile_env = std::getenv("BGC_SOAK_TILE");
  const char* kern_env = std::getenv("BGC_SOAK_KERNEL");
  if (m % 256 || n % 256 || (tile_env && std::string(tile_env) == "128")) return SoakKernel::k2Buf128;
  if (k % (2 * kSoakBK) || (kern_env && std::string(kern_env) == "2buf")) return SoakKernel::k2Buf256;
  return SoakKernel::kPingPong;
}

void launch_soak_gemm(SoakKernel kern, const void* a, const void* bt, void* c, int m, int n, int k) {
  const auto* pa = static_cast<const __bf16*>(a);
  const auto* pb = static_cast<const __bf16*>(bt);
  auto* pc = static_cast<float*>(c);
  const dim3 big_grid((m / 256) * (n / 256));
  switch (kern) {
    case SoakKernel::kPingPong:
      hipLaunchKernelGGL(gemm_pingpong, big_grid, dim3(512), 0, nullptr, pa, pb, pc, m, n, k);
      break;
    case SoakKernel::k2Buf256:
      hipLaunchKernelGGL((gemm_soak<256, 256, 2, 4>), big_grid, dim3(512), 0, nullptr, pa, pb, pc, m, n, k);
      break;
    case SoakKernel::k2Buf128:
      hipLaunchKernelGGL((gemm_soak<128, 128, 2, 2>), dim3((m / 128) * (n / 128)), dim3(256), 0, nullptr, pa, pb, pc, m, n, k);
      break;
  }
}

bool soak_shape_ok(int m, int n, int k) {
  return m >= 128 && n >= 128 && k >= kSoakBK && m % 128 == 0 && n % 128 == 0 && k % kSoakBK == 0 && m <= 32768 &&
         n <= 32768 && k <= 32768;
}

// bgc_diag_gemm_soak, bgc_diag_gemm_soak_planted with its test plants added to C after their launch, and
// bgc_diag_gemm_soak_data with the operands, the reference checksums and C downloaded to `dump` at the end
int soak_run(int device, int m, int n, int k, int launches, uint32_t seed, const bgc_soak_plant* plants, int n_plants,
             const bgc_soak_data* dump, bgc_soak_result* out) {
  bool ok = out && launches > 0 && soak_shape_ok(m, n, k) && plant_list_ok(plants, n_plants);
  for (int j = 0; ok && j < n_plants; ++j) {
    const bgc_soak_plant& p = plants[j];
    // only the first and the last launch are verified
    ok = (p.launch == 0 || p.launch == launches - 1) && p.row >= 0 && p.row < m && p.col >= 0 && p.col < n;
  }
  if (!ok) {
    g_last_error = n_plants ? "invalid arguments: m, n multiples of 128 and k of 64 (each <= 32768); plants inside C, on the first or the last launch"
                            : "invalid arguments: m, n multiples of 128 and k of 64 (each <= 32768)";
    return 1;
  }
  const SoakKernel kern = soak_kernel(m, n, k);
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(device));
  const size_t na = static_cast<size_t>(m) * k, nb = static_cast<size_t>(n) * k, nc = static_cast<size_t>(m) * n;
  DeviceBuffer a, bt, c, sa, sb, rref, cref, rgot, cgot, flags;
  HIP_TRY(flags.alloc((static_cast<size_t>(m) + n) * 4));  // inexact rows, then columns
  HIP_TRY(a.alloc(na * 2));
  HIP_TRY(bt.alloc(nb * 2));
  HIP_TRY(c.alloc(nc * 4));
  HIP_TRY(sa.alloc(static_cast<size_t>(k) * 4, true));
  HIP_TRY(sb.alloc(static_cast<size_t>(k) * 4, true));
  HIP_TRY(rref.alloc(static_cast<size_t>(m) * 8));
  HIP_TRY(cref.alloc(static_cast<size_t>(n) * 8));
  HIP_TRY(rgot.alloc(static_cast<size_t>(m) * 8));
  HIP_TRY(cgot.alloc(static_cast<size_t>(n) * 8));
  const dim3 block(kBlock), fill_grid(cu_count(device) * 8);
  auto slabs = [](int rows, int cols) { return dim3((cols + kBlock - 1) / kBlock, (rows + 63) / 64); };
  hipLaunchKernelGGL(soak_fill, fill_grid, block, 0, nullptr, a.as<__bf16>(), na, seed);
  hipLaunchKernelGGL(soak_fill, fill_grid, block, 0, nullptr, bt.as<__bf16>(), nb, seed ^ 0xB7B7B7B7u);
  // reference checksums: sA = 1^T A (per k), sB = B 1 = per-k sums of Bt's rows
  hipLaunchKernelGGL((soak_colsum<__bf16, int>), slabs(m, k), block, 0, nullptr, a.as<const __bf16>(), m, k, sa.as<int>());
  hipLaunchKernelGGL((soak_colsum<__bf16, int>), slabs(n, k), block, 0, nullptr, bt.as<const __bf16>(), n, k, sb.as<int>());
  hipLaunchKernelGGL(soak_rowsum<__bf16>, dim3(m), block, 0, nullptr, a.as<const __bf16>(), k, sb.as<const int>(),
                     rref.as<long long>());  // rows of C = A (B 1)
  hipLaunchKernelGGL(soak_rowsum<__bf16>, dim3(n), block, 0, nullptr, bt.as<const __bf16>(), k, sa.as<const int>(),
                     cref.as<long long>());  // cols of C = (1^T A) B
  HIP_TRY(hipGetLastError());
  std::vector<long long> rr(static_cast<size_t>(m)), cr(static_cast<size_t>(n)), rg(static_cast<size_t>(m)),
      cg(static_cast<size_t>(n));
  HIP_TRY(hipMemcpy(rr.data(), rref.p, rr.size() * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cr.data(), cref.p, cr.size() * 8, hipMemcpyDeviceToHost));
  std::vector<unsigned> fl(static_cast<size_t>(m) + n);
  auto verify = [&](uint64_t* row_bad, uint64_t* col_bad) -> int {
    HIP_TRY(hipMemset(cgot.p, 0, static_cast<size_t>(n) * 8));
    HIP_TRY(hipMemset(flags.p, 0, fl.size() * 4));
    hipLaunchKernelGGL(soak_rowsum<float>, dim3(m), block, 0, nullptr, c.as<const float>(), n, static_cast<const int*>(nullptr),
                       rgot.as<long long>(), flags.as<unsigned>());
    hipLaunchKernelGGL((soak_colsum<float, unsigned long long>), slabs(m, n), block, 0, nullptr, c.as<const float>(), m, n,
                       cgot.as<unsigned long long>(), flags.as<unsigned>() + m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(rg.data(), rgot.p, rg.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cg.data(), cgot.p, cg.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(fl.data(), flags.p, fl.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < m; ++i) *row_bad += rg[static_cast<size_t>(i)] != rr[static_cast<size_t>(i)] || fl[static_cast<size_t>(i)];
    for (int j = 0; j < n; ++j) *col_bad += cg[static_cast<size_t>(j)] != cr[static_cast<size_t>(j)] || fl[static_cast<size_t>(m) + j];
    return 0;
  };
  // test plants of launch `it`, applied once it has finished (timed() waits for it)
  auto plant = [&](int it) -> int {
    for (int j = 0; j < n_plants; ++j) {
      if (plants[j].launch != it) continue;
      const float delta = plants[j].delta;
      float* at = c.as<float>() + static_cast<size_t>(plants[j].row) * n + plants[j].col;
      if (modify_device_value(at, [=](float x) { return x + delta; }) != 0) return 1;
    }
    return 0;
  };
  Events ev;
  HIP_TRY(ev.create());
  const double flop = 2.0 * m * n * static_cast<double>(k);
  float ms = 0.f, best = 1e30f, total = 0.f;
  for (int it = 0; it < launches; ++it) {
    // poison C before the last checked launch, so its checksums cover that launch's writes
    if (it > 0 && it == launches - 1) HIP_TRY(hipMemsetAsync(c.p, 0xFF, nc * 4, nullptr));
    if (timed(ev, &ms, [&] { launch_soak_gemm(kern, a.p, bt.p, c.p, m, n, k); }) != 0) return 1;
    best = std::min(best, ms);
    total += ms;
    if ((it == 0 || it == launches - 1) && plant(it) != 0) return 1;
    if (it == 0 && verify(&out->row_mismatches, &out->col_mismatches) != 0) return 1;
  }
  if (launches > 1 && verify(&out->row_mismatches, &out->col_mismatches) != 0) return 1;
  if (dump) {
    HIP_TRY(hipMemcpy(dump->a, a.p, na * 2, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dump->bt, bt.p, nb * 2, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dump->c, c.p, nc * 4, hipMemcpyDeviceToHost));
    std::memcpy(dump->rref, rr.data(), rr.size() * 8);
    std::memcpy(dump->cref, cr.data(), cr.size() * 8);
  }
  out->m = m;
  out->n = n;
  out->k = k;
  out->tile = kern == SoakKernel::k2Buf128 ? 128 : 256;
  out->kernel = kern == SoakKernel::kPingPong ? 2 : 1;
  out->launches = launches;
  out->elapsed_ms = total;
  out->tflops_best = flop / (best * 1e-3) / 1e12;
  out->tflops_mean = flop * launches / (total * 1e-3) / 1e12;
  return 0;
}

}  // namespace

extern "C" {

int bgc_diag_gemm_soak(int device, int m, int n, int k, int launches, uint32_t seed, bgc_soak_result* out) {
  return soak_run(device, m, n, k, launches, seed, nullptr, 0, nullptr, out);
}

int bgc_diag_gemm_soak_planted(int device, int m, int n, int k, int launches, uint32_t seed, const bgc_soak_plant* plants,
                               int n_plants, bgc_soak_result* out) {
  return soak_run(device, m, n, k, launches, seed, plants, n_plants, nullptr, out);
}

int bgc_diag_gemm_soak_data(int device, int m, int n, int k, uint32_t seed, const bgc_soak_data* data, bgc_soak_result* out) {
  // of a valid shape (each side <= 32768, so no product overflows): operands, C and the checksums
  const auto bytes = [&] { return 2ULL * m * k + 2ULL * n * k + 4ULL * m * n + 8ULL * m + 8ULL * n; };
  if (!data || !data->a || !data->bt || !data->rref || !data->cref || !data->c ||
      (soak_shape_ok(m, n, k) && bytes() > BGC_DIAG_MAX_DATA_BYTES)) {
    g_last_error = "invalid arguments: five destinations, and at most 128 MiB to return";
    return 1;
  }
  return soak_run(device, m, n, k, 1, seed, nullptr, 0, data, out);
}

int bgc_diag_gemm_tiled(int device, int m, int n, int k, const uint16_t* a_bf16, const uint16_t* bt_bf16, float* c) {
  if (!a_bf16 || !bt_bf16 || !c || !soak_shape_ok(m, n, k)) {
    g_last_error = "invalid arguments: m, n multiples of 128 and k of 64 (each <= 32768)";
    return 1;
  }
  HIP_TRY(hipSetDevice(device));
  const size_t na = static_cast<size_t>(m) * k, nb = static_cast<size_t>(n) * k;
  return gemm_on_host_operands(
      {{a_bf16, na * 2}, {bt_bf16, nb * 2}}, c, static_cast<size_t>(m) * n,
      [&](const void* const* d, float* dc) { launch_soak_gemm(soak_kernel(m, n, k), d[0], d[1], dc, m, n, k); });
}

}  // extern "C"
