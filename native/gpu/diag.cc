#include "gpu/diag.h"

#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <mutex>
#include <stdexcept>

namespace bgc::gpu {

namespace {

std::string exe_dir() {
  char buf[4096];
  ssize_t n = readlink("/proc/self/exe", buf, sizeof(buf) - 1);
  if (n <= 0) return ".";
  buf[n] = 0;
  std::string p(buf);
  return p.substr(0, p.rfind('/'));
}

std::string so_dir() {
  Dl_info info;
  if (dladdr(reinterpret_cast<void*>(&exe_dir), &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    size_t s = p.rfind('/');
    if (s != std::string::npos) return p.substr(0, s);
  }
  return ".";
}

void* open_library(const std::string& path) {
  void* lib = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
  if (!lib) throw std::runtime_error("cannot load " + path + ": " + dlerror());
  return lib;
}

// How many members an aggregate has: the most initialisers that T{...} takes.
struct AnyMember {
  template <class T>
  operator T() const;
};
template <class T, class... A>
constexpr size_t member_count(...) { return sizeof...(A) - 1; }
template <class T, class... A>
constexpr auto member_count(int) -> decltype(T{A{}...}, size_t()) { return member_count<T, A..., AnyMember>(0); }

}  // namespace

// the entry members load themselves (diag.h), each throwing if the library lacks it
Diag::Diag(const std::string& path) : path_(path), lib_(open_library(path)) {
  if (entry<decltype(&bgc_diag_abi_version)>("bgc_diag_abi_version")() != BGC_DIAG_ABI_VERSION) {
    throw std::runtime_error(path + " is not a compatible bgc diag library");
  }
}

void* Diag::symbol(const char* name) const {
  void* sym = dlsym(lib_, name);
  if (!sym) throw std::runtime_error(path_ + " is not a compatible bgc diag library: no " + name);
  return sym;
}

void Diag::check(const char* what, int rc) const {
  if (rc != 0) throw std::runtime_error(std::string(what) + ": " + last_error_());
}

Diag& Diag::instance(const std::string& explicit_path) {
  static std::mutex mu;
  static Diag* d = nullptr;
  std::lock_guard<std::mutex> lk(mu);
  if (d) return *d;
  std::vector<std::string> candidates;
  if (!explicit_path.empty()) candidates.push_back(explicit_path);
  if (const char* e = std::getenv("BGC_GPU_DIAG_LIB")) candidates.emplace_back(e);
  candidates.push_back(so_dir() + "/libbgc_gpu_diag.so");
  candidates.push_back(exe_dir() + "/../bacchus_gpu_controller_amd/libbgc_gpu_diag.so");
  candidates.push_back("libbgc_gpu_diag.so");
  std::string errors;
  for (const auto& c : candidates) {
    if (c.find('/') != std::string::npos && access(c.c_str(), R_OK) != 0) continue;
    try {
      d = new Diag(c);
      return *d;
    } catch (const std::exception& e) {
      errors += std::string(e.what()) + "; ";
    }
  }
  throw std::runtime_error("libbgc_gpu_diag.so not found: " + errors);
}

int Diag::device_count() { return device_count_(); }

std::string Diag::device_arch(int device) {
  char buf[128] = {0};
  if (arch_(device, buf, sizeof(buf)) != 0) throw std::runtime_error(last_error_());
  return buf;
}

// the bad CU keys that a result holds (its first 64), as an array
template <class Result>
json::Value bad_cu_keys(const Result& r) {
  json::Value keys = json::Value::array();
  for (int i = 0; i < r.bad_cus && i < 64; ++i) keys.push_back(r.bad_cu_keys[i]);
  return keys;
}

json::Value to_json(int device, const bgc_hbm_result& r) {
  json::Value v = json::Value::object();
  v["device"] = device;
  v["bytes"] = static_cast<unsigned long long>(r.bytes);
  v["iters"] = r.iters;
  v["write_gbps"] = r.write_gbps;
  v["read_gbps"] = r.read_gbps;
  v["copy_gbps"] = r.copy_gbps;
  v["mismatches"] = static_cast<unsigned long long>(r.mismatches);
  v["first_bad_word"] = r.first_bad_word == ~0ULL ? json::Value() : json::Value(static_cast<unsigned long long>(r.first_bad_word));
  v["elapsed_ms"] = r.elapsed_ms;
  v["passed"] = r.mismatches == 0;
  return v;
}

json::Value to_json(int device, const bgc_mfma_result& r) {
  json::Value v = json::Value::object();
  v["device"] = device;
  v["tiles_checked"] = static_cast<unsigned long long>(r.tiles_checked);
  v["mismatches"] = static_cast<unsigned long long>(r.mismatches);
  v["cus_seen"] = r.cus_seen;
  v["xccs_seen"] = r.xccs_seen;
  v["bad_cus"] = r.bad_cus;
  v["bad_cu_keys"] = bad_cu_keys(r);
  v["tflops"] = r.tflops;
  v["throughput_ok"] = r.throughput_ok != 0;
  json::Value xw = json::Value::array(), xus = json::Value::array();
  for (int x = 0; x < 8; ++x) {
    xw.push_back(r.xcc_waves[x]);
    xus.push_back(r.xcc_wave_us[x]);
  }
  v["xcc_waves"] = xw;
  v["xcc_wave_us"] = xus;
  v["xcc_balance"] = r.xcc_balance;
  v["elapsed_ms"] = r.elapsed_ms;
  v["passed"] = r.mismatches == 0 && r.throughput_ok != 0;
  return v;
}

json::Value to_json(int device, const bgc_lowp_result& r) {
  const uint64_t mism = r.fp8_mismatches + r.fp8_scaled_mismatches + r.fp4_mismatches + r.fp4_scaled_mismatches;
  return json::Value::object({{"device", device},
                              {"tiles_checked", static_cast<unsigned long long>(r.tiles_checked)},
                              {"fp8_mismatches", static_cast<unsigned long long>(r.fp8_mismatches)},
                              {"fp8_scaled_mismatches", static_cast<unsigned long long>(r.fp8_scaled_mismatches)},
                              {"fp4_mismatches", static_cast<unsigned long long>(r.fp4_mismatches)},
                              {"fp4_scaled_mismatches", static_cast<unsigned long long>(r.fp4_scaled_mismatches)},
                              {"mismatches", static_cast<unsigned long long>(mism)},
                              {"cus_seen", r.cus_seen},
                              {"bad_cus", r.bad_cus},
                              {"bad_cu_keys", bad_cu_keys(r)},
                              {"fp8_tflops", r.fp8_tflops},
                              {"fp4_tflops", r.fp4_tflops},
                              {"throughput_ok", r.throughput_ok != 0},
                              {"elapsed_ms", r.elapsed_ms},
                              {"passed", mism == 0 && r.throughput_ok != 0}});
}

json::Value to_json(int device, const bgc_classic_result& r) {
  json::Value ms = json::Value::array();
  for (int p = 0; p < 4; ++p) ms.push_back(r.rate_ms[p]);
  const uint64_t mism = r.mismatches[0] + r.mismatches[1] + r.mismatches[2] + r.mismatches[3];
  return json::Value::object({{"device", device},
                              {"tiles_checked", static_cast<unsigned long long>(r.tiles_checked)},
                              {"fp16_mismatches", static_cast<unsigned long long>(r.mismatches[BGC_CLASSIC_FP16])},
                              {"int8_mismatches", static_cast<unsigned long long>(r.mismatches[BGC_CLASSIC_INT8])},
                              {"fp32_mismatches", static_cast<unsigned long long>(r.mismatches[BGC_CLASSIC_FP32])},
                              {"fp64_mismatches", static_cast<unsigned long long>(r.mismatches[BGC_CLASSIC_FP64])},
                              {"mismatches", static_cast<unsigned long long>(mism)},
                              {"cus_seen", r.cus_seen},
                              {"bad_cus", r.bad_cus},
                              {"bad_cu_keys", bad_cu_keys(r)},
                              {"fp16_tflops", r.rate[BGC_CLASSIC_FP16]},
                              {"int8_tops", r.rate[BGC_CLASSIC_INT8]},
                              {"fp32_tflops", r.rate[BGC_CLASSIC_FP32]},
                              {"fp64_tflops", r.rate[BGC_CLASSIC_FP64]},
                              {"rate_ms", ms},
                              {"throughput_ok", r.throughput_ok != 0},
                              {"elapsed_ms", r.elapsed_ms},
                              {"passed", mism == 0 && r.throughput_ok != 0}});
}

json::Value to_json(int device, const bgc_lds_result& r) {
  char bits[16];
  std::snprintf(bits, sizeof(bits), "0x%08x", r.bad_bits);
  const bool clean = r.mismatches == 0;
  return json::Value::object({{"device", device},
                              {"cus", r.cus},
                              {"cus_seen", r.cus_seen},
                              {"bad_cus", r.bad_cus},
                              {"bad_cu_keys", bad_cu_keys(r)},
                              {"words_checked", static_cast<unsigned long long>(r.words_checked)},
                              {"mismatches", static_cast<unsigned long long>(r.mismatches)},
                              {"first_bad_cu_key", clean ? json::Value() : json::Value(r.first_bad_cu_key)},
                              {"first_bad_word", clean ? json::Value() : json::Value(static_cast<unsigned long long>(r.first_bad_word))},
                              {"bad_bits", clean ? json::Value() : json::Value(std::string(bits))},
                              {"read_tbps", r.read_tbps},
                              {"rate_ok", r.rate_ok != 0},
                              {"slowest_cu_key", r.slowest_cu_key},
                              {"cu_balance", r.cu_balance},
                              {"elapsed_ms", r.elapsed_ms},
                              {"passed", clean && r.rate_ok != 0}});
}

json::Value to_json(int device, const bgc_cache_result& r) {
  char l2_bits[16], ic_bits[16];
  std::snprintf(l2_bits, sizeof(l2_bits), "0x%08x", r.l2_bad_bits);
  std::snprintf(ic_bits, sizeof(ic_bits), "0x%08x", r.ic_bad_bits);
  const bool l2_clean = r.l2_mismatches == 0, ic_clean = r.ic_mismatches == 0, ic_ran = r.ic_bytes != 0;
  // the per-XCC arrays end at the highest XCC that ran a workgroup: a partitioned device has fewer than 8
  int xccs = 0;
  for (int x = 0; x < 8; ++x) {
    if (r.xcc_wgs[x] > 0 || r.xcc_mismatches[x] > 0) xccs = x + 1;
  }
  json::Value mism = json::Value::array(), wgs = json::Value::array(), us = json::Value::array();
  for (int x = 0; x < xccs; ++x) {
    mism.push_back(static_cast<unsigned long long>(r.xcc_mismatches[x]));
    wgs.push_back(r.xcc_wgs[x]);
    us.push_back(r.xcc_us[x]);
  }
  return json::Value::object({{"device", device},
                              {"cus", r.cus},
                              {"xccs_seen", r.xccs_seen},
                              {"rounds", r.rounds},
                              {"region_bytes", static_cast<unsigned long long>(r.region_bytes)},
                              {"l2_words_checked", static_cast<unsigned long long>(r.l2_words_checked)},
                              {"l2_mismatches", static_cast<unsigned long long>(r.l2_mismatches)},
                              {"l2_bad_xccs", r.l2_bad_xccs},
                              {"xcc_mismatches", mism},
                              {"first_bad_xcc", l2_clean ? json::Value() : json::Value(r.first_bad_xcc)},
                              {"first_bad_word", l2_clean ? json::Value() : json::Value(static_cast<unsigned long long>(r.first_bad_word))},
                              {"l2_bad_bits", l2_clean ? json::Value() : json::Value(std::string(l2_bits))},
                              {"l2_read_tbps", r.l2_read_tbps},
                              {"l2_rate_ok", r.l2_rate_ok != 0},
                              {"xcc_wgs", wgs},
                              {"xcc_us", us},
                              {"slowest_xcc", r.slowest_xcc},
                              {"xcc_balance", r.xcc_balance},
                              {"ic_bytes", static_cast<unsigned long long>(r.ic_bytes)},
                              {"ic_words_checked", static_cast<unsigned long long>(r.ic_words_checked)},
                              {"ic_mismatches", static_cast<unsigned long long>(r.ic_mismatches)},
                              {"ic_first_bad_word", ic_clean ? json::Value() : json::Value(static_cast<unsigned long long>(r.ic_first_bad_word))},
                              {"ic_bad_bits", ic_clean ? json::Value() : json::Value(std::string(ic_bits))},
                              {"ic_read_tbps", ic_ran ? json::Value(r.ic_read_tbps) : json::Value()},
                              {"ic_rate_ok", r.ic_rate_ok != 0},
                              {"elapsed_ms", r.elapsed_ms},
                              {"passed", l2_clean && ic_clean && r.l2_rate_ok != 0 && r.ic_rate_ok != 0}});
}

json::Value to_json(int device, const bgc_valu_result& r) {
  static const char* const kClasses[BGC_VALU_CLASSES] = {"int32", "fp32", "fp16", "fp64", "cvt", "dot", "trans"};
  json::Value by_class = json::Value::array(), rate_ms = json::Value::array();
  uint64_t mism = 0;
  for (int c = 0; c < BGC_VALU_CLASSES; ++c) {
    by_class.push_back(static_cast<unsigned long long>(r.mismatches[c]));
    mism += r.mismatches[c];
  }
  for (int c = 0; c < BGC_VALU_RATE_CLASSES; ++c) rate_ms.push_back(r.rate_ms[c]);
  char lanes[24];
  std::snprintf(lanes, sizeof(lanes), "0x%016llx", static_cast<unsigned long long>(r.bad_lanes));
  const bool clean = mism == 0;
  return json::Value::object({{"device", device},
                              {"cus", r.cus},
                              {"cus_seen", r.cus_seen},
                              {"simds_seen", r.simds_seen},
                              {"values_checked", static_cast<unsigned long long>(r.values_checked)},
                              {"class_mismatches", by_class},  // int32, fp32, fp16, fp64, cvt, dot, trans
                              {"mismatches", static_cast<unsigned long long>(mism)},
                              {"consensus_ok", r.consensus_ok != 0},
                              {"trans_out_of_bound", static_cast<unsigned long long>(r.trans_out_of_bound)},
                              {"bad_cus", r.bad_cus},
                              {"bad_simds", r.bad_simds},
                              {"bad_cu_keys", bad_cu_keys(r)},
                              {"first_bad_cu_key", clean ? json::Value() : json::Value(r.first_bad_cu_key)},
                              {"first_bad_simd", clean ? json::Value() : json::Value(r.first_bad_simd)},
                              {"first_bad_lane", clean ? json::Value() : json::Value(r.first_bad_lane)},
                              {"first_bad_class", clean ? json::Value() : json::Value(std::string(kClasses[r.first_bad_class]))},
                              {"bad_lanes", clean ? json::Value() : json::Value(std::string(lanes))},
                              {"fp32_tflops", r.rate[BGC_VALU_RATE_FP32]},
                              {"fp16_tflops", r.rate[BGC_VALU_RATE_FP16]},
                              {"fp64_tflops", r.rate[BGC_VALU_RATE_FP64]},
                              {"int32_tops", r.rate[BGC_VALU_RATE_INT32]},
                              {"trans_tips", r.rate[BGC_VALU_RATE_TRANS]},
                              {"rate_ms", rate_ms},  // fp32, fp16, fp64, int32, trans
                              {"rate_ok", r.rate_ok != 0},
                              {"slowest_cu_key", r.slowest_cu_key},
                              {"cu_balance", r.cu_balance},
                              {"elapsed_ms", r.elapsed_ms},
                              {"passed", clean && r.consensus_ok != 0 && r.trans_out_of_bound == 0 && r.rate_ok != 0}});
}

json::Value to_json(int device, const bgc_atomic_result& r) {
  static const char* const kClasses[BGC_ATOMIC_CLASSES] = {"int32", "int64", "f32", "f64", "pk16", "cas", "ticket", "lds"};
  json::Value own = json::Value::array(), shared = json::Value::array(), rate_ms = json::Value::array();
  json::Value xw = json::Value::array(), xus = json::Value::array();
  uint64_t mism = 0;
  for (int c = 0; c < BGC_ATOMIC_CLASSES; ++c) {
    own.push_back(static_cast<unsigned long long>(r.mismatches[BGC_ATOMIC_OWN][c]));
    shared.push_back(static_cast<unsigned long long>(r.mismatches[BGC_ATOMIC_SHARED][c]));
    mism += r.mismatches[BGC_ATOMIC_OWN][c] + r.mismatches[BGC_ATOMIC_SHARED][c];
  }
  for (int c = 0; c < BGC_ATOMIC_RATE_CLASSES; ++c) rate_ms.push_back(r.rate_ms[c]);
  for (int x = 0; x < 8; ++x) {
    xw.push_back(r.xcc_waves[x]);
    xus.push_back(r.xcc_us[x]);
  }
  char bits[24];
  std::snprintf(bits, sizeof(bits), "0x%016llx", static_cast<unsigned long long>(r.first_bad_xor));
  const bool clean = mism == 0;
  return json::Value::object({{"device", device},
                              {"cus", r.cus},
                              {"cus_seen", r.cus_seen},
                              {"values_checked", static_cast<unsigned long long>(r.values_checked)},
                              {"own_mismatches", own},  // int32, int64, f32, f64, pk16, cas, ticket, lds
                              {"shared_mismatches", shared},
                              {"mismatches", static_cast<unsigned long long>(mism)},
                              {"bad_cus", r.bad_cus},
                              {"bad_cu_keys", bad_cu_keys(r)},
                              {"first_bad_placement", clean ? json::Value() : json::Value(std::string(r.first_bad_placement == BGC_ATOMIC_OWN ? "own" : "shared"))},
                              {"first_bad_class", clean ? json::Value() : json::Value(std::string(kClasses[r.first_bad_class]))},
                              {"first_bad_op", clean ? json::Value() : json::Value(r.first_bad_op)},
                              {"first_bad_element", clean ? json::Value() : json::Value(static_cast<long long>(r.first_bad_element))},
                              {"first_bad_xor", clean ? json::Value() : json::Value(std::string(bits))},
                              {"first_bad_delta", clean ? json::Value() : json::Value(static_cast<long long>(r.first_bad_delta))},
                              {"tickets_out_of_range", static_cast<unsigned long long>(r.tickets_out_of_range)},
                              {"f32_add_tbps", r.rate[BGC_ATOMIC_RATE_F32]},
                              {"pk_bf16_add_tbps", r.rate[BGC_ATOMIC_RATE_PK_BF16]},
                              {"u32_add_tbps", r.rate[BGC_ATOMIC_RATE_U32]},
                              {"rtn_gops", r.rate[BGC_ATOMIC_RATE_RTN]},
                              {"rate_ms", rate_ms},  // f32, pk bf16, u32, rtn
                              {"rate_ok", r.rate_ok != 0},
                              {"xcc_waves", xw},
                              {"xcc_us", xus},
                              {"slowest_xcc", r.slowest_xcc},
                              {"xcc_balance", r.xcc_balance},
                              {"elapsed_ms", r.elapsed_ms},
                              {"passed", clean && r.tickets_out_of_range == 0 && r.rate_ok != 0}});
}

json::Value to_json(int device, const bgc_regfile_result& r) {
  static const char* const kPhases[BGC_REGFILE_PHASES] = {"layout0_pass0", "layout0_pass1", "layout1_pass0", "layout1_pass1", "rotate"};
  char bits[16], lanes[24], reg[8] = "";
  std::snprintf(bits, sizeof(bits), "0x%08x", r.bad_bits);
  std::snprintf(lanes, sizeof(lanes), "0x%016llx", static_cast<unsigned long long>(r.bad_lane_mask));
  const bool clean = r.mismatches == 0;
  if (!clean) std::snprintf(reg, sizeof(reg), "%c%d", r.first_bad_reg < 256 ? 'v' : 'a', r.first_bad_reg % 256);
  return json::Value::object({{"device", device},
                              {"cus", r.cus},
                              {"cus_seen", r.cus_seen},
                              {"simds", r.simds},
                              {"simds_seen", r.simds_seen},
                              {"regs_marched", r.regs_marched},
                              {"ring_regs", r.ring_regs},
                              {"words_checked", static_cast<unsigned long long>(r.words_checked)},
                              {"mismatches", static_cast<unsigned long long>(r.mismatches)},
                              {"vgpr_mismatches", static_cast<unsigned long long>(r.vgpr_mismatches)},
                              {"agpr_mismatches", static_cast<unsigned long long>(r.agpr_mismatches)},
                              {"rotate_mismatches", static_cast<unsigned long long>(r.rotate_mismatches)},
                              {"bad_simds", r.bad_simds},
                              {"bad_bits", clean ? json::Value() : json::Value(std::string(bits))},
                              {"bad_lane_mask", clean ? json::Value() : json::Value(std::string(lanes))},
                              {"first_bad_cu_key", clean ? json::Value() : json::Value(r.first_bad_cu_key)},
                              {"first_bad_simd", clean ? json::Value() : json::Value(r.first_bad_simd)},
                              {"first_bad_reg", clean ? json::Value() : json::Value(r.first_bad_reg)},  // 0..511: v0..v255, a0..a255
                              {"first_bad_reg_name", clean ? json::Value() : json::Value(std::string(reg))},
                              {"first_bad_lane", clean ? json::Value() : json::Value(r.first_bad_lane)},
                              {"first_bad_phase", clean ? json::Value() : json::Value(r.first_bad_phase)},
                              {"first_bad_phase_name", clean ? json::Value() : json::Value(std::string(kPhases[r.first_bad_phase]))},
                              {"mov_tops", r.mov_tops},
                              {"rate_ok", r.rate_ok != 0},
                              {"simd_balance", r.simd_balance},
                              {"slowest_cu_key", r.slowest_cu_key},
                              {"slowest_simd", r.slowest_simd},
                              {"march_ms", r.march_ms},
                              {"rotate_ms", r.rotate_ms},
                              {"elapsed_ms", r.elapsed_ms},
                              {"passed", clean && r.rate_ok != 0 && r.simds_seen == r.simds}});
}

json::Value to_json(int device, const bgc_xlane_result& r) {
  static const char* const kClasses[BGC_XLANE_CLASSES] = {"row", "wave", "mask", "alu", "swap", "lds", "lane", "exec"};
  json::Value by_class = json::Value::array(), rate_ms = json::Value::array();
  uint64_t mism = 0;
  for (int c = 0; c < BGC_XLANE_CLASSES; ++c) {
    by_class.push_back(static_cast<unsigned long long>(r.mismatches[c]));
    mism += r.mismatches[c];
  }
  for (int c = 0; c < BGC_XLANE_RATE_CLASSES; ++c) rate_ms.push_back(r.rate_ms[c]);
  char lanes[24];
  std::snprintf(lanes, sizeof(lanes), "0x%016llx", static_cast<unsigned long long>(r.bad_lanes));
  const bool clean = mism == 0;
  return json::Value::object({{"device", device},
                              {"cus", r.cus},
                              {"cus_seen", r.cus_seen},
                              {"simds_seen", r.simds_seen},
                              {"values_checked", static_cast<unsigned long long>(r.values_checked)},
                              {"class_mismatches", by_class},  // row, wave, mask, alu, swap, lds, lane, exec
                              {"mismatches", static_cast<unsigned long long>(mism)},
                              {"bad_cus", r.bad_cus},
                              {"bad_simds", r.bad_simds},
                              {"bad_cu_keys", bad_cu_keys(r)},
                              {"first_bad_cu_key", clean ? json::Value() : json::Value(r.first_bad_cu_key)},
                              {"first_bad_simd", clean ? json::Value() : json::Value(r.first_bad_simd)},
                              {"first_bad_lane", clean ? json::Value() : json::Value(r.first_bad_lane)},
                              {"first_bad_class", clean ? json::Value() : json::Value(std::string(kClasses[r.first_bad_class]))},
                              {"bad_lanes", clean ? json::Value() : json::Value(std::string(lanes))},
                              {"dpp_tops", r.rate[BGC_XLANE_RATE_DPP]},  // all four in 1e12 lane-moves per second
                              {"swap_tops", r.rate[BGC_XLANE_RATE_SWAP]},
                              {"bpermute_tops", r.rate[BGC_XLANE_RATE_BPERMUTE]},
                              {"swizzle_tops", r.rate[BGC_XLANE_RATE_SWIZZLE]},
                              {"rate_ms", rate_ms},  // dpp, swap, bpermute, swizzle
                              {"rate_ok", r.rate_ok != 0},
                              {"slowest_cu_key", r.slowest_cu_key},
                              {"cu_balance", r.cu_balance},
                              {"elapsed_ms", r.elapsed_ms},
                              {"passed", clean && r.rate_ok != 0}});
}

json::Value to_json(int device, const bgc_pcie_result& r) {
  return json::Value::object({{"device", device}, {"bytes", static_cast<unsigned long long>(r.bytes)},
                              {"iters", r.iters}, {"h2d_gbps", r.h2d_gbps}, {"d2h_gbps", r.d2h_gbps},
                              {"bidir_gbps", r.bidir_gbps}, {"mismatches", static_cast<unsigned long long>(r.mismatches)},
                              {"elapsed_ms", r.elapsed_ms}, {"passed", r.mismatches == 0}});
}

json::Value to_json(int device, const bgc_soak_result& r) {
  return json::Value::object({{"device", device}, {"m", r.m}, {"n", r.n}, {"k", r.k}, {"launches", r.launches},
                              {"tile", r.tile}, {"kernel", r.kernel == 2 ? "pingpong" : "2buf"},
                              {"elapsed_ms", r.elapsed_ms}, {"tflops_mean", r.tflops_mean},
                              {"tflops_best", r.tflops_best},
                              {"row_mismatches", static_cast<unsigned long long>(r.row_mismatches)},
                              {"col_mismatches", static_cast<unsigned long long>(r.col_mismatches)},
                              {"passed", r.row_mismatches == 0 && r.col_mismatches == 0}});
}

json::Value to_json(int device, const bgc_hbm_walk_result& r) {
  char addr[32], flips[32];
  std::snprintf(addr, sizeof(addr), "0x%llx", static_cast<unsigned long long>(r.first_bad_addr));
  std::snprintf(flips, sizeof(flips), "0x%016llx", static_cast<unsigned long long>(r.first_bad_xor));
  const double cov = r.free_bytes ? static_cast<double>(r.bytes_covered) / static_cast<double>(r.free_bytes) : 0.0;
  return json::Value::object({{"device", device},
                              {"free_bytes", static_cast<unsigned long long>(r.free_bytes)},
                              {"total_bytes", static_cast<unsigned long long>(r.total_bytes)},
                              {"target_bytes", static_cast<unsigned long long>(r.target_bytes)},
                              {"bytes_covered", static_cast<unsigned long long>(r.bytes_covered)},
                              {"coverage_of_free", cov},
                              {"chunks", r.chunks},
                              {"passes", r.passes},
                              {"mismatches", static_cast<unsigned long long>(r.mismatches)},
                              {"first_bad_addr", r.mismatches ? json::Value(std::string(addr)) : json::Value()},
                              {"first_bad_bits", r.mismatches ? json::Value(std::string(flips)) : json::Value()},
                              {"write_gbps", r.write_gbps},
                              {"read_gbps", r.read_gbps},
                              {"alloc_ms", r.alloc_ms},
                              {"elapsed_ms", r.elapsed_ms},
                              {"budget_hit", r.budget_hit != 0},
                              {"passed", r.mismatches == 0 && r.passes == 2}});
}

json::Value Diag::hbm(int device, uint64_t bytes, int iters, uint32_t seed) {
  return call("hbm diag", hbm_, device, bytes, iters, seed);
}

json::Value Diag::mfma(int device, int waves_per_cu, int throughput_iters, uint32_t seed) {
  return call("mfma diag", mfma_, device, waves_per_cu, throughput_iters, seed);
}

json::Value Diag::mfma_lowp(int device, int waves_per_cu, int throughput_iters, uint32_t seed) {
  return call("low-precision mfma diag", lowp_, device, waves_per_cu, throughput_iters, seed);
}

json::Value Diag::mfma_classic(int device, int waves_per_cu, int throughput_iters, uint32_t seed) {
  return call("classic mfma diag", classic_, device, waves_per_cu, throughput_iters, seed);
}

json::Value Diag::lds(int device, int wgs_per_cu, int rate_iters, uint32_t seed) {
  return call("lds diag", lds_, device, wgs_per_cu, rate_iters, seed);
}

json::Value Diag::cache(int device, int rounds, uint32_t region_bytes, int l2_sweeps, uint64_t ic_bytes, int ic_sweeps, uint32_t seed) {
  return call("cache diag", cache_, device, rounds, region_bytes, l2_sweeps, ic_bytes, ic_sweeps, seed);
}

json::Value Diag::valu(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed) {
  return call("valu diag", valu_, device, waves_per_simd, rounds, rate_iters, seed);
}

json::Value Diag::atomic(int device, int wgs_per_cu, int rounds, int rate_iters, uint32_t seed) {
  return call("atomic diag", atomic_, device, wgs_per_cu, rounds, rate_iters, seed);
}

json::Value Diag::regfile(int device, int wgs_per_cu, int sweeps, uint32_t seed) {
  return call("regfile diag", regfile_, device, wgs_per_cu, sweeps, seed);
}

json::Value Diag::xlane(int device, int waves_per_simd, int rounds, int rate_iters, uint32_t seed) {
  return call("xlane diag", xlane_, device, waves_per_simd, rounds, rate_iters, seed);
}

json::Value Diag::pcie(int device, uint64_t bytes, int iters, uint32_t seed) {
  return call("pcie diag", pcie_, device, bytes, iters, seed);
}

json::Value Diag::gemm_soak(int device, int m, int n, int k, int launches, uint32_t seed) {
  return call("gemm soak", soak_, device, m, n, k, launches, seed);
}

json::Value Diag::hbm_walk(int device, double fraction, uint64_t chunk_bytes, int budget_ms, uint32_t seed) {
  return call("hbm walk", walk_, device, fraction, chunk_bytes, budget_ms, seed);
}

// The burn's JSON carries an argument (the dtype) and no device.
json::Value to_json(const bgc_burn_result& r, int dtype) {
  return json::Value::object({{"dtype", burn_dtype_name(dtype)}, {"launches", r.launches},
                              {"elapsed_ms", r.elapsed_ms}, {"tflops_mean", r.tflops_mean},
                              {"tflops_min", r.tflops_min}, {"tflops_first", r.tflops_first},
                              {"tflops_last", r.tflops_last}, {"tflops_max", r.tflops_max},
                              // the last launch against the best: < 1 when the GPU throttled
                              {"sustain", r.tflops_max > 0 ? r.tflops_last / r.tflops_max : 0.0},
                              {"mismatches", static_cast<unsigned long long>(r.mismatches)}});
}

json::Value Diag::burn(int device, int duration_ms, int waves_per_cu, uint32_t seed, int dtype) {
  bgc_burn_result r{};
  check("burn", burn_(device, duration_ms, waves_per_cu, seed, dtype, &r));
  return to_json(r, dtype);
}

void Diag::gemm(int device, int m, int n, int k, const uint16_t* a, const uint16_t* b, float* c) {
  check("gemm diag", gemm_(device, m, n, k, a, b, c));
}

void Diag::gemm_tiled(int device, int m, int n, int k, const uint16_t* a, const uint16_t* bt, float* c) {
  check("tiled gemm", tiled_(device, m, n, k, a, bt, c));
}

void Diag::gemm_dtype(int device, int path, int m, int n, int k, const void* a, const void* b, double* c) {
  check("dtype gemm", gemm_dtype_(device, path, m, n, k, a, b, c));
}

void Diag::mx_gemm(int device, int fmt, int m, int n, int k, const uint8_t* a, const uint8_t* a_scales,
                   const uint8_t* bt, const uint8_t* bt_scales, float* c) {
  check("mx gemm", mx_gemm_(device, fmt, m, n, k, a, a_scales, bt, bt_scales, c));
}

std::string Diag::device_bdf(int device) {
  char buf[64] = {0};
  check("device bdf", bdf_(device, buf, sizeof(buf)));
  return buf;
}

namespace {

uint32_t mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// bf16 bit pattern of a pseudo-random value in [-1, 1] (round-to-nearest-even), and the
// exact float it encodes.
uint16_t rand_bf16(uint32_t seed, uint32_t i, float* exact) {
  float f = static_cast<float>(mix(seed ^ mix(i * 0x9e3779b9U))) / 4294967295.0f * 2.0f - 1.0f;
  uint32_t bits;
  std::memcpy(&bits, &f, 4);
  bits += 0x7fff + ((bits >> 16) & 1);
  uint16_t h = static_cast<uint16_t>(bits >> 16);
  uint32_t back = static_cast<uint32_t>(h) << 16;
  std::memcpy(exact, &back, 4);
  return h;
}

}  // namespace

json::Value Diag::gemm_check(int device, int m, int n, int k, uint32_t seed) {
  std::vector<uint16_t> a(static_cast<size_t>(m) * k), b(static_cast<size_t>(k) * n);
  std::vector<float> af(a.size()), bf(b.size()), c(static_cast<size_t>(m) * n);
  for (size_t i = 0; i < a.size(); ++i) a[i] = rand_bf16(seed, static_cast<uint32_t>(i), &af[i]);
  for (size_t i = 0; i < b.size(); ++i) b[i] = rand_bf16(seed ^ 0xB0B0B0B0U, static_cast<uint32_t>(i), &bf[i]);
  gemm(device, m, n, k, a.data(), b.data(), c.data());
  // fp32 MFMA accumulation of exact bf16 products: |err| <= K * 2^-24 * sum|a||b| (plus
  // slack); measured against a double-precision host product.
  double max_err = 0, max_ratio = 0;
  uint64_t bad = 0;
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j < n; ++j) {
      double ref = 0, mag = 0;
      for (int kk = 0; kk < k; ++kk) {
        const double p = static_cast<double>(af[static_cast<size_t>(i) * k + kk]) * bf[static_cast<size_t>(kk) * n + j];
        ref += p;
        mag += std::fabs(p);
      }
      const double err = std::fabs(static_cast<double>(c[static_cast<size_t>(i) * n + j]) - ref);
      const double bound = 4.0 * k * 5.96e-8 * mag + 1e-6;
      max_err = std::max(max_err, err);
      max_ratio = std::max(max_ratio, err / bound);
      if (err > bound || !std::isfinite(c[static_cast<size_t>(i) * n + j])) ++bad;
    }
  }
  return json::Value::object({{"m", m}, {"n", n}, {"k", k}, {"max_abs_err", max_err},
                              {"max_err_over_bound", max_ratio}, {"bad_elements", static_cast<unsigned long long>(bad)},
                              {"passed", bad == 0}});
}

int burn_dtype_code(const std::string& name) {
  if (name == "bf16") return BGC_BURN_BF16;
  if (name == "fp8") return BGC_BURN_FP8;
  if (name == "fp4") return BGC_BURN_FP4;
  throw std::runtime_error("burn dtype must be bf16, fp8 or fp4, not '" + name + "'");
}

const char* burn_dtype_name(int code) {
  return code == BGC_BURN_FP8 ? "fp8" : code == BGC_BURN_FP4 ? "fp4" : "bf16";
}

double burn_dtype_rate_ratio(int code) {
  // sustained on MI355X: bf16 2.40, MX fp8 4.79, MX fp4 8.47 PF/s (profiles/mx_lowp_r3/)
  return code == BGC_BURN_FP8 ? 2.0 : code == BGC_BURN_FP4 ? 3.5 : 1.0;
}

const std::vector<std::pair<std::string, DiagFloors::Field>>& DiagFloors::fields() {
#define BGC_FLOOR(field) {#field, &DiagFloors::field}
  static const std::pair<const char*, Field> rows[] = {
      BGC_FLOOR(min_read_gbps), BGC_FLOOR(min_copy_gbps), BGC_FLOOR(min_write_gbps), BGC_FLOOR(min_mfma_tflops),
      BGC_FLOOR(min_xcc_balance), BGC_FLOOR(min_fp8_tflops), BGC_FLOOR(min_fp4_tflops), BGC_FLOOR(min_xccs),
      BGC_FLOOR(min_fp16_tflops), BGC_FLOOR(min_int8_tops), BGC_FLOOR(min_fp32_tflops), BGC_FLOOR(min_fp64_tflops),
      BGC_FLOOR(min_lds_read_tbps), BGC_FLOOR(min_lds_cu_coverage), BGC_FLOOR(min_burn_tflops),
      BGC_FLOOR(min_burn_sustain), BGC_FLOOR(max_burn_hotspot_c), BGC_FLOOR(max_burn_thermal_violation_pct),
      BGC_FLOOR(min_pcie_h2d_gbps), BGC_FLOOR(min_pcie_d2h_gbps), BGC_FLOOR(require_full_pcie_width),
      BGC_FLOOR(min_pcie_speed_fraction), BGC_FLOOR(min_soak_tflops), BGC_FLOOR(min_hbm_walk_coverage),
      BGC_FLOOR(min_node_burn_balance), BGC_FLOOR(max_node_power_w)};
#undef BGC_FLOOR
  static_assert(std::size(rows) == member_count<DiagFloors>(0), "DiagFloors::fields() must name every member of DiagFloors");
  static const std::vector<std::pair<std::string, Field>> table(std::begin(rows), std::end(rows));
  return table;
}

}  // namespace bgc::gpu
