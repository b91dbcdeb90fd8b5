// Loader for libbgc_gpu_diag.so (HIP/CDNA4 health kernels, native/gpu/hip/).
#pragma once

#include <cstdint>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <variant>
#include <vector>

#include "core/json.h"
#include "gpu/hip/gpu_diag.h"

namespace bgc::gpu {

// read(name, field&) for every (name, member pointer) of `fields`: a struct read or written by its fields' names.
template <class T, class Fields, class Read>
void apply_fields(T& object, const Fields& fields, Read&& read) {
  for (const auto& f : fields) std::visit([&](auto member) { read(f.first, object.*member); }, f.second);
}

// Performance floors that turn the diagnostics into a health gate: a GPU whose HBM or matrix cores run well below what
// an MI355X delivers is not advertised, even when every pattern and tile checks out.  Each member starts at its MI355X
// default, ~25 % under the rate measured at the node agent's default sizes; 0 (false) disables a floor.
struct DiagFloors {
  // `hbm` and `mfma` sections.  MI355X, ROCm 7.2, 1 GiB buffers / 16 waves per CU x 2048 MFMA iterations
  // (profiles/archive/diag_floors_r2.json): read 6.33-6.57 TB/s, copy 5.36-5.42, write 5.11-5.25, MFMA bf16 1.92-2.06 PF/s,
  // XCC balance 0.96.  At 256 MiB (Infinity-Cache-sized, the smallest sensible buffer) read is still 5.56 TB/s, so these
  // floors hold down to it.
  double min_read_gbps = 4750, min_copy_gbps = 4000, min_write_gbps = 3800;
  double min_mfma_tflops = 1500;
  double min_xcc_balance = 0.85;  // slowest XCC mean wave time / fastest, inverted (0..1]
  // MX block-scaled low-precision matrix cores (`lowp` section): any wrong tile fails; rate floors for the dense fp8 and
  // fp4 phases.  v_mfma_scale_f32_16x16x128_f8f6f4, 32 waves per CU x 4096 iterations (profiles/mx_lowp_r3/): 4.1-4.7 PF/s
  // fp8 and 7.3-8.1 PF/s fp4 depending on how warm the clocks are, against ~5 and ~10 PF/s dense peaks
  double min_fp8_tflops = 3000, min_fp4_tflops = 5000;
  int min_xccs = 8;  // XCCs that must have run MFMA work
  // fp16 / int8 / fp32 / fp64 matrix-core paths (`classic` section): any wrong tile element fails; rate floors on each
  // path's dense MFMA rate (int8 in TOP/s).  32 waves per CU x 8192 iterations, right after the MX check
  // (profiles/mfma_classic/rates.json): over 12 runs back to back fp16 2177-2288 TF/s, int8 4204-4424 TOP/s, fp32
  // 155.8-157.5 and fp64 78.0-78.3 TF/s; in whole passes in a fresh process 2074-2090, 3902-3979, 146.4-148.2 and
  // 77.2-77.7.  Each floor is 25 % under the lowest run of its path.
  double min_fp16_tflops = 1550, min_int8_tops = 2900, min_fp32_tflops = 109, min_fp64_tflops = 57;
  // Local Data Share (`lds` section): any word of the per-CU march that reads back wrong fails; rate floor on the aggregate
  // LDS read rate, and the share of the device's CUs (cus_seen / cus) that a march workgroup must have run on.  4 march
  // workgroups per CU, then 8192 sweeps of 512-thread 16-byte reads, right after the MFMA check
  // (profiles/lds_diag/lds_rate.json): 121-138 TB/s over 12 runs back to back, rising as the clocks warm, and 116-120 TB/s
  // in whole passes in a fresh worker process, against ~150 TB/s at 2.4 GHz; the march reached 256 of 256 CUs in every run
  double min_lds_read_tbps = 85;
  double min_lds_cu_coverage = 1.0;
  // Burn-in (sustained MFMA load, `burn` section): rate floor, the rate may not sag below this fraction of its best launch,
  // and the thermal limits under load.  Measured on MI355X in profiles/archive/diag_burn_r2.json (sustained bf16 MFMA at
  // 97 % of the 2.5 PF/s dense peak once clocks settle)
  double min_burn_tflops = 1800;  // measured 2409-2421 PF/s mean over 10 s at 1.17-1.22 kW, 2.34-2.39 GHz
  double min_burn_sustain = 0.80;  // tflops_last / tflops_max
  double max_burn_hotspot_c = 100;
  double max_burn_thermal_violation_pct = 20;
  // PCIe (`pcie` section): host<->device DMA rates, and the link must run at its full width (and at least this fraction of
  // its top speed) while the copies run.  Gen5 x16 host link (profiles/archive/pcie_r2/probe.json): 57.1 GB/s
  // host-to-device and 56.7 GB/s device-to-host with 64 MiB - 1 GiB pinned copies, 97 GB/s both ways at once; a
  // Gen4-trained or x8 link delivers half of that.
  double min_pcie_h2d_gbps = 45, min_pcie_d2h_gbps = 45;
  bool require_full_pcie_width = true;
  double min_pcie_speed_fraction = 0.5;
  // GEMM soak (`soak` section): every checksum must match; rate floor on the mean.  8-phase ping-pong bf16 MFMA, 256x256
  // tiles: 1463-1587 TF/s at 8192^3 and 1348-1444 at 4096^3 on MI355X (profiles/gemm_soak_r3/); the floor stays where
  // round 2's double-buffered kernel (1253-1361 TF/s) also passes, for BGC_SOAK_KERNEL=2buf
  double min_soak_tflops = 950;
  // HBM walk (`hbm_walk` section): any mismatch fails; the walk must cover at least this share of the free VRAM (a failed
  // allocation on an idle, fenced GPU means something else holds its memory).  0.9 of free VRAM is requested; 0.8 leaves
  // room for allocator granularity
  double min_hbm_walk_coverage = 0.8;
  // Node-level burn (judge_node_burn, diag_runner.h): under the shared load every GPU must reach this fraction of the
  // node's fastest GPU, and the summed draw must stay under the limit.  One GPU 15 % behind the node's fastest is a cooling
  // or power-delivery outlier (healthy MI355X burns agree within ~1 %, profiles/archive/diag_burn_r2.json); the node power
  // limit is site-specific (0 = off)
  double min_node_burn_balance = 0.85;
  double max_node_power_w = 0;
  static DiagFloors mi355x_defaults() { return DiagFloors(); }
  // Every member by its name (a static_assert in diag.cc holds the list to that): what the node agent reads as
  // CONF_DIAG_<FIELD> and judge_diag as its floors JSON.
  using Field = std::variant<double DiagFloors::*, bool DiagFloors::*, int DiagFloors::*>;
  static const std::vector<std::pair<std::string, Field>>& fields();
  template <class Read>
  void apply(Read&& read) { apply_fields(*this, fields(), read); }  // the field as double&, bool& or int&
};

// Burn dtype names ("bf16", "fp8", "fp4") <-> BGC_BURN_*; the name throws on anything else.
int burn_dtype_code(const std::string& name);
const char* burn_dtype_name(int code);
// Dense-rate ratio of a burn dtype to bf16 on MI355X, as the burn kernels measure it (fp8
// 2.0x, fp4 3.5x; profiles/mx_lowp_r3/): the bf16 burn floor scales by it.
double burn_dtype_rate_ratio(int code);

// The result structs as JSON: one shape for a diagnostic and its planted variant.
json::Value to_json(int device, const bgc_hbm_result& r);
json::Value to_json(int device, const bgc_mfma_result& r);
json::Value to_json(int device, const bgc_lowp_result& r);
json::Value to_json(int device, const bgc_classic_result& r);
json::Value to_json(int device, const bgc_lds_result& r);
json::Value to_json(int device, const bgc_cache_result& r);
json::Value to_json(int device, const bgc_valu_result& r);
json::Value to_json(int device, const bgc_atomic_result& r);
json::Value to_json(int device, const bgc_regfile_result& r);
json::Value to_json(int device, const bgc_xlane_result& r);
json::Value to_json(int device, const bgc_pcie_result& r);
json::Value to_json(int device, const bgc_soak_result& r);
json::Value to_json(int device, const bgc_hbm_walk_result& r);
// The burn's JSON names its dtype (BGC_BURN_*) instead of a device.
json::Value to_json(const bgc_burn_result& r, int dtype);

class Diag {
 public:
  // Searches $BGC_GPU_DIAG_LIB, then <exe dir>/../bacchus_gpu_controller_amd/, then the
  // dynamic linker path. Throws std::runtime_error if not found.
  static Diag& instance(const std::string& explicit_path = "");
  int device_count();
  std::string device_arch(int device);
  json::Value hbm(int device, uint64_t bytes, int iters, uint32_t seed);
  json::Value mfma(int device, int waves_per_cu, int throughput_iters, uint32_t seed);
  // MX block-scaled fp8 / fp4 matrix-core tiles and rates (see bgc_diag_mfma_lowp).
  json::Value mfma_lowp(int device, int waves_per_cu, int throughput_iters, uint32_t seed);
  // fp16 / int8 / fp32 / fp64 matrix-core tiles and rates (see bgc_diag_mfma_classic).
  json::Value mfma_classic(int device, int waves_per_cu, int throughput_iters, uint32_t seed);
  // March test of every CU's whole LDS and the LDS read rate (see bgc_diag_lds).
  json::Value lds(int device, int wgs_per_cu, int rate_iters, uint32_t seed);
  // March and read rate of every XCD's L2, pattern check and read rate of the Infinity Cache (see bgc_diag_cache).
  json::Value cache(int device, int rounds, uint32_t region_bytes, int l2_sweeps, uint64_t ic_bytes, int ic_sweeps, uint32_t seed);
  // Per-SIMD check of the vector ALU's instruction classes, refereed by the host, and the vector rates (see bgc_diag_valu).
  json::Value valu(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed);
  // Check of every global and LDS atomic form, refereed by the host, and the atomic rates (see bgc_diag_atomic).
  json::Value atomic(int device, int wgs_per_cu, int rounds, int rate_iters, uint32_t seed);
  // Per-SIMD march of the whole vector register file and the rotate's move rate (see bgc_diag_regfile).
  json::Value regfile(int device, int wgs_per_cu, int sweeps, uint32_t seed);
  // Per-SIMD check of the cross-lane paths (DPP, half-wave swaps, LDS crossbar, lane <-> scalar), refereed by the host,
  // and the cross-lane rates (see bgc_diag_xlane).
  json::Value xlane(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed);
  // MFMA GEMM on the device vs a host fp32 product of the same bf16 operands
  // (deterministic pseudo-random values in [-1, 1]).  Returns max error and the bound.
  json::Value gemm_check(int device, int m, int n, int k, uint32_t seed);
  // Sustained MFMA load for duration_ms (see bgc_diag_burn_dtype; dtype BGC_BURN_*).
  json::Value burn(int device, int duration_ms, int waves_per_cu, uint32_t seed, int dtype = BGC_BURN_BF16);
  // Pinned host <-> device copies (see bgc_diag_pcie).
  json::Value pcie(int device, uint64_t bytes, int iters, uint32_t seed);
  // LDS-tiled MFMA GEMM run back to back, checked by exact checksums (bgc_diag_gemm_soak).
  json::Value gemm_soak(int device, int m, int n, int k, int launches, uint32_t seed);
  // Raw GEMM: A/B as bf16 bit patterns, C fp32 (row-major).
  void gemm(int device, int m, int n, int k, const uint16_t* a, const uint16_t* b, float* c);
  // The soak's LDS-tiled GEMM on caller operands (Bt = B transposed, [n][k]).
  void gemm_tiled(int device, int m, int n, int k, const uint16_t* a, const uint16_t* bt, float* c);
  // MX fp8 (fmt 0) / fp4 (fmt 4) block-scaled GEMM on caller codes and E8M0 scales
  void mx_gemm(int device, int fmt, int m, int n, int k, const uint8_t* a, const uint8_t* a_scales, const uint8_t* bt,
               const uint8_t* bt_scales, float* c);
  // GEMM on classic path `path` (BGC_CLASSIC_*): A/B in the path's element type, C double (row-major).
  void gemm_dtype(int device, int path, int m, int n, int k, const void* a, const void* b, double* c);
  // Address-pattern walk of `fraction` of the free VRAM (see bgc_diag_hbm_walk).
  json::Value hbm_walk(int device, double fraction, uint64_t chunk_bytes, int budget_ms, uint32_t seed);
  // PCI bus id of a HIP device, lower-case ("0000:05:00.0").
  std::string device_bdf(int device);
  const std::string& path() const { return path_; }

  // An entry point by name, as the type gpu_diag.h declares it with:
  // entry<decltype(&bgc_diag_hbm)>("bgc_diag_hbm").  Throws if the library lacks it.  The methods
  // above cover what the node agent and the diag worker run; this is how a test reaches an entry
  // they do not load.
  template <class Fn>
  Fn entry(const char* name) const {
    return reinterpret_cast<Fn>(symbol(name));
  }
  // Throws "<what>: <the library's last error>" unless an entry returned 0.
  void check(const char* what, int rc) const;
  // One run of an entry that takes (device, args..., result struct*): the result as JSON.
  template <class... P, class... A>
  json::Value call(const char* what, int (*fn)(P...), int device, A... args) const {
    std::remove_pointer_t<std::tuple_element_t<sizeof...(P) - 1, std::tuple<P...>>> r{};
    check(what, fn(device, args..., &r));
    return to_json(device, r);
  }

 private:
  explicit Diag(const std::string& path);
  void* symbol(const char* name) const;
  std::string path_;
  void* lib_ = nullptr;
  // each entry is loaded as the type gpu_diag.h declares it with, in this order, after lib_
#define BGC_DIAG_ENTRY(member, name) decltype(&name) member = entry<decltype(&name)>(#name)
  BGC_DIAG_ENTRY(last_error_, bgc_diag_last_error);
  BGC_DIAG_ENTRY(device_count_, bgc_diag_device_count);
  BGC_DIAG_ENTRY(arch_, bgc_diag_device_arch);
  BGC_DIAG_ENTRY(bdf_, bgc_diag_device_bdf);
  BGC_DIAG_ENTRY(hbm_, bgc_diag_hbm);
  BGC_DIAG_ENTRY(walk_, bgc_diag_hbm_walk);
  BGC_DIAG_ENTRY(pcie_, bgc_diag_pcie);
  BGC_DIAG_ENTRY(mfma_, bgc_diag_mfma);
  BGC_DIAG_ENTRY(lowp_, bgc_diag_mfma_lowp);
  BGC_DIAG_ENTRY(classic_, bgc_diag_mfma_classic);
  BGC_DIAG_ENTRY(lds_, bgc_diag_lds);
  BGC_DIAG_ENTRY(cache_, bgc_diag_cache);
  BGC_DIAG_ENTRY(valu_, bgc_diag_valu);
  BGC_DIAG_ENTRY(atomic_, bgc_diag_atomic);
  BGC_DIAG_ENTRY(regfile_, bgc_diag_regfile);
  BGC_DIAG_ENTRY(xlane_, bgc_diag_xlane);
  BGC_DIAG_ENTRY(burn_, bgc_diag_burn_dtype);
  BGC_DIAG_ENTRY(soak_, bgc_diag_gemm_soak);
  BGC_DIAG_ENTRY(gemm_, bgc_diag_gemm);
  BGC_DIAG_ENTRY(tiled_, bgc_diag_gemm_tiled);
  BGC_DIAG_ENTRY(mx_gemm_, bgc_diag_mx_gemm);
  BGC_DIAG_ENTRY(gemm_dtype_, bgc_diag_gemm_dtype);
#undef BGC_DIAG_ENTRY
};

}  // namespace bgc::gpu
