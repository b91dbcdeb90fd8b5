// MI355X (gfx950 / CDNA4) GPU health diagnostics (libbgc_gpu_diag.so).  See gpu_diag.h for the
// C ABI.  This file: ABI version, the last error, device count, arch and PCI bus id.  The
// kernels and their entry points, one file per family:
//  * hbm.hip: HBM3E bandwidth (fill/copy/check), the address-in-data walk over free VRAM and
//    the pinned host<->device copies for PCIe;
//  * mfma.hip: the per-CU bf16, MX fp8/fp4 and fp16/int8/fp32/fp64 matrix-core checks and throughput kernels, the
//    burn-in loop that runs them back to back, and the one-wave GEMMs on caller operands;
//  * lds.hip: the per-CU march test of the whole Local Data Share and its read rate;
//  * cache.hip: the per-XCC march through every XCD's L2 with its read rate, and the Infinity Cache's
//    pattern check and read rate;
//  * valu.hip: the per-SIMD vector-ALU check (integer, fp32, fp16, fp64, conversions, integer dots and
//    transcendentals, refereed by the host through valu_ref.h) and the vector rates;
//  * atomic.hip: the check of every global and LDS atomic form in a table per workgroup and in one shared by the
//    launch, refereed by the host through atomic_ref.h, and the atomic rates;
//  * regfile.hip: the per-SIMD march of the whole vector register file (v0..v255, a0..a255) in two layouts and the
//    rotate of 504 registers with its move rate, both held to regfile_ref.h;
//  * xlane.hip: the per-SIMD check of the cross-lane paths (DPP, the half-wave swaps, the LDS crossbar's permutes, the
//    moves between lanes and scalar registers), refereed by the host through xlane_ref.h, and the cross-lane rates;
//  * gemm_soak.hip: the ABFT-checked LDS-tiled GEMMs (gemm_soak and the 8-phase gemm_pingpong).
// The design notes in those files follow the CDNA4 guides (cdna_hip_programming.md,
// MI355X_MICROARCH.md).
#include <cctype>
#include <cstdio>

#include "diag_common.h"

namespace bgc_diag {
thread_local std::string g_last_error;
}

extern "C" {

int bgc_diag_abi_version(void) { return BGC_DIAG_ABI_VERSION; }

const char* bgc_diag_last_error(void) { return bgc_diag::g_last_error.c_str(); }

int bgc_diag_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int bgc_diag_device_arch(int device, char* buf, size_t len) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  std::snprintf(buf, len, "%s", prop.gcnArchName);
  return 0;
}

int bgc_diag_device_bdf(int device, char* buf, size_t len) {
  if (!buf || len < 13) {
    bgc_diag::g_last_error = "invalid arguments";
    return 1;
  }
  char tmp[64] = {0};
  HIP_TRY(hipDeviceGetPCIBusId(tmp, static_cast<int>(sizeof(tmp)), device));
  for (char* p = tmp; *p; ++p) *p = static_cast<char>(std::tolower(static_cast<unsigned char>(*p)));
  std::snprintf(buf, len, "%s", tmp);
  return 0;
}

}  // extern "C"
