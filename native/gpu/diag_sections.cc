#include "gpu/diag_sections.h"

#include <cstdio>
#include <mutex>

#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>

#include "gpu/diag_runner.h"

namespace bgc::gpu {

using json::Value;

const std::vector<std::pair<std::string, DiagPlan::Field>>& DiagPlan::fields() {
#define BGC_PLAN(field) {#field, &DiagPlan::field}
  static const std::vector<std::pair<std::string, Field>> table = {
      BGC_PLAN(hbm_bytes), BGC_PLAN(hbm_walk_fraction), BGC_PLAN(hbm_walk_chunk_bytes), BGC_PLAN(hbm_walk_budget_ms),
      BGC_PLAN(pcie_bytes), BGC_PLAN(soak_size), BGC_PLAN(soak_launches), BGC_PLAN(lowp), BGC_PLAN(classic),
      BGC_PLAN(lds), BGC_PLAN(burn_ms)};
#undef BGC_PLAN
  return table;
}

Value to_json(const DiagPlan& p) {
  Value v = Value::object();
  apply_fields(p, DiagPlan::fields(), [&](const std::string& name, const auto& field) {
    if constexpr (std::is_same_v<decltype(field), const uint64_t&>) v[name] = static_cast<unsigned long long>(field);
    else v[name] = field;
  });
  v["burn_dtype"] = burn_dtype_name(p.burn_dtype);
  return v;
}

// a plan's field from its JSON value; a value of another type than the field leaves it as it is
static void read_json(const Value& j, bool& field) { if (j.is_bool()) field = j.as_bool(); }
static void read_json(const Value& j, double& field) { if (j.is_number()) field = j.as_double(); }
static void read_json(const Value& j, uint64_t& field) { if (j.is_int()) field = j.as_uint(); }
static void read_json(const Value& j, int& field) { if (j.is_int()) field = static_cast<int>(j.as_int()); }

DiagPlan diag_plan_from_json(const Value& v) {
  DiagPlan p;
  apply_fields(p, DiagPlan::fields(), [&](const std::string& name, auto& field) { read_json(v.get(name), field); });
  if (v.get("burn_dtype").is_string()) p.burn_dtype = burn_dtype_code(v.get_string("burn_dtype"));
  return p;
}

namespace {

// flock(2) on a file: PCIe sections of concurrent worker processes take turns.
class FileLock {
 public:
  explicit FileLock(const std::string& path) {
    if (path.empty()) return;
    fd_ = ::open(path.c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0600);
    if (fd_ >= 0) {
      while (::flock(fd_, LOCK_EX) != 0 && errno == EINTR) {
      }
    }
  }
  ~FileLock() {
    if (fd_ >= 0) ::close(fd_);  // releases the lock
  }
  FileLock(const FileLock&) = delete;
  FileLock& operator=(const FileLock&) = delete;
  bool held() const { return fd_ >= 0; }

 private:
  int fd_ = -1;
};

// Iterations of each classic path's rate launch: 1.9-2.1 ms fp16, 2.0-2.3 ms int8, 3.5-3.8 ms fp32 and
// 7.0-7.1 ms fp64 on the MI355X (profiles/mfma_classic/rates.json)
constexpr int kClassicIters = 8192;
// Sweeps of the LDS rate phase: 2.4-2.9 ms on the MI355X (profiles/lds_diag/lds_rate.json)
constexpr int kLdsRateIters = 8192;

double num(const Value& v, const char* k) { return v.get(k).is_number() ? v.get(k).as_double() : 0.0; }
uint64_t count(const Value& v, const char* k) { return static_cast<uint64_t>(num(v, k)); }
int whole(const Value& v, const char* k) { return static_cast<int>(num(v, k)); }
bool is_false(const Value& v, const char* k) { return v.get(k).is_bool() && !v.get(k).as_bool(); }

// ---- how the HIP engine runs it
Value run_hbm(Diag& d, Backend&, const DiagRun& r) { return d.hbm(r.dev, r.plan.hbm_bytes, 2, r.seed); }
Value run_hbm_walk(Diag& d, Backend&, const DiagRun& r) {
  return d.hbm_walk(r.dev, r.plan.hbm_walk_fraction, r.plan.hbm_walk_chunk_bytes, r.plan.hbm_walk_budget_ms, r.seed);
}
Value run_mfma(Diag& d, Backend&, const DiagRun& r) { return d.mfma(r.dev, 16, 2048, r.seed); }
Value run_lowp(Diag& d, Backend&, const DiagRun& r) { return d.mfma_lowp(r.dev, 32, 4096, r.seed); }  // ~5 ms
Value run_classic(Diag& d, Backend&, const DiagRun& r) { return d.mfma_classic(r.dev, 32, kClassicIters, r.seed); }
Value run_lds(Diag& d, Backend&, const DiagRun& r) { return d.lds(r.dev, 4, kLdsRateIters, r.seed); }
Value run_gemm(Diag& d, Backend&, const DiagRun& r) { return d.gemm_check(r.dev, 64, 64, 512, r.seed); }
Value run_pcie(Diag&, Backend& backend, const DiagRun& r) {
  // One GPU at a time: eight concurrent pinned-copy streams share the host's memory
  // bandwidth and root complexes, so concurrent rates would measure the host, not
  // the GPU's link.  ~50 ms per GPU.
  static std::mutex pcie_mu;
  std::lock_guard<std::mutex> lk(pcie_mu);
  FileLock across_processes(r.pcie_lock_path);
  Value out = pcie_check(backend, r.gpu, r.dev, r.plan.pcie_bytes, r.seed);
  // false: the lock file could not be opened, so other GPUs' copies may have overlapped
  if (!r.pcie_lock_path.empty()) out["serialized"] = across_processes.held();
  return out;
}
Value run_soak(Diag& d, Backend&, const DiagRun& r) {
  return d.gemm_soak(r.dev, r.plan.soak_size, r.plan.soak_size, r.plan.soak_size, r.plan.soak_launches, r.seed);
}

// ---- what the scripted engine reports for it: a healthy MI355X
Value scripted_hbm(const DiagRun& r) {
  return Value::object({{"device", r.dev}, {"bytes", static_cast<unsigned long long>(r.plan.hbm_bytes)}, {"read_gbps", 6400.0},
                        {"write_gbps", 5200.0}, {"copy_gbps", 5400.0}, {"mismatches", 0}, {"passed", true}});
}
Value scripted_hbm_walk(const DiagRun& r) {
  const uint64_t free_b = r.gpu.vram_total_mb * (1ULL << 20);
  const uint64_t covered = static_cast<uint64_t>(static_cast<double>(free_b) * r.plan.hbm_walk_fraction);
  const uint64_t bad = count(*r.script, "walk_mismatches");  // the one wrong value a script can plant
  return Value::object({{"device", r.dev}, {"free_bytes", static_cast<unsigned long long>(free_b)},
                        {"bytes_covered", static_cast<unsigned long long>(covered)},
                        {"coverage_of_free", r.plan.hbm_walk_fraction}, {"passes", 2},
                        {"mismatches", static_cast<unsigned long long>(bad)}, {"passed", bad == 0}});
}
Value scripted_mfma(const DiagRun& r) {
  return Value::object({{"device", r.dev}, {"tflops", 2000.0}, {"xcc_balance", 0.96}, {"xccs_seen", 8},
                        {"mismatches", 0}, {"bad_cus", 0}, {"throughput_ok", true}, {"passed", true}});
}
Value scripted_lowp(const DiagRun& r) {
  return Value::object({{"device", r.dev}, {"fp8_tflops", 4000.0}, {"fp4_tflops", 7000.0}, {"mismatches", 0},
                        {"bad_cus", 0}, {"throughput_ok", true}, {"passed", true}});
}
Value scripted_classic(const DiagRun& r) {
  return Value::object({{"device", r.dev}, {"fp16_tflops", 2000.0}, {"int8_tops", 4000.0}, {"fp32_tflops", 150.0},
                        {"fp64_tflops", 75.0}, {"mismatches", 0}, {"bad_cus", 0}, {"throughput_ok", true}, {"passed", true}});
}
Value scripted_lds(const DiagRun& r) {
  return Value::object({{"device", r.dev}, {"cus", 256}, {"cus_seen", 256}, {"bad_cus", 0}, {"mismatches", 0},
                        {"read_tbps", 100.0}, {"rate_ok", true}, {"cu_balance", 0.97}, {"passed", true}});
}
Value scripted_gemm(const DiagRun&) { return Value::object({{"passed", true}}); }
Value scripted_soak(const DiagRun&) {
  return Value::object({{"tflops_mean", 1300.0}, {"row_mismatches", 0}, {"col_mismatches", 0}, {"passed", true}});
}

// ---- its verdict beyond the floors of its numbers
template <class... A>
void fail(Value& failures, const char* format, A... args) {
  char buf[200];
  std::snprintf(buf, sizeof(buf), format, args...);
  failures.push_back(std::string(buf));
}

// "<what> <value> below floor <floor>": the line of every floor in a section's numbers
void judge_floor(const Value& v, const char* key, double floor, const char* what, int decimals, Value& failures) {
  if (floor > 0 && num(v, key) < floor) fail(failures, "%s %.*f below floor %.*f", what, decimals, num(v, key), decimals, floor);
}

void judge_hbm(const Value& v, const DiagFloors&, Value& failures) {
  if (num(v, "mismatches") > 0) failures.push_back("HBM pattern mismatches: " + std::to_string(count(v, "mismatches")));
}
void judge_hbm_walk(const Value& v, const DiagFloors& fl, Value& failures) {
  if (num(v, "mismatches") > 0) {
    std::string msg = "HBM walk mismatches: " + std::to_string(count(v, "mismatches"));
    if (v.get("first_bad_addr").is_string()) {
      msg += " (first at " + v.get_string("first_bad_addr") + ", bits " + v.get_string("first_bad_bits") + ")";
    }
    failures.push_back(msg);
  }
  if (fl.min_hbm_walk_coverage > 0 && num(v, "coverage_of_free") < fl.min_hbm_walk_coverage) {
    fail(failures, "HBM walk covered %.2f of free VRAM (floor %.2f)", num(v, "coverage_of_free"), fl.min_hbm_walk_coverage);
  }
}
void judge_mfma(const Value& v, const DiagFloors&, Value& failures) {
  if (num(v, "mismatches") > 0) failures.push_back("MFMA tile mismatches on " + std::to_string(whole(v, "bad_cus")) + " CU(s)");
  if (is_false(v, "throughput_ok")) failures.push_back("MFMA throughput accumulators wrong");
}
void judge_mfma_xccs(const Value& v, const DiagFloors& fl, Value& failures) {
  if (fl.min_xccs > 0 && num(v, "xccs_seen") < fl.min_xccs) {
    failures.push_back("only " + std::to_string(whole(v, "xccs_seen")) + " XCCs ran MFMA work");
  }
}
void judge_lowp(const Value& v, const DiagFloors&, Value& failures) {
  if (num(v, "mismatches") > 0) {
    fail(failures, "MX fp8/fp4 MFMA tile mismatches on %d CU(s): fp8 %.0f, fp8 scaled %.0f, fp4 %.0f, fp4 scaled %.0f",
         whole(v, "bad_cus"), num(v, "fp8_mismatches"), num(v, "fp8_scaled_mismatches"), num(v, "fp4_mismatches"),
         num(v, "fp4_scaled_mismatches"));
  }
  if (is_false(v, "throughput_ok")) failures.push_back("MX fp8/fp4 MFMA throughput accumulators wrong");
}
void judge_classic(const Value& v, const DiagFloors&, Value& failures) {
  for (const char* path : {"fp16", "int8", "fp32", "fp64"}) {
    const double bad = num(v, (std::string(path) + "_mismatches").c_str());
    if (bad > 0) {
      const Value& keys = v.get("bad_cu_keys");
      const int first = keys.is_array() && !keys.items().empty() && keys.items()[0].is_number() ? static_cast<int>(keys.items()[0].as_double()) : -1;
      fail(failures, "%s MFMA tile mismatches: %.0f elements, %d bad CU(s), first CU key %d", path, bad, whole(v, "bad_cus"), first);
    }
  }
  if (is_false(v, "throughput_ok")) failures.push_back("fp16/int8/fp32/fp64 MFMA throughput accumulators wrong");
}
void judge_lds(const Value& v, const DiagFloors&, Value& failures) {
  if (num(v, "mismatches") > 0) {
    fail(failures, "LDS march mismatches on %d CU(s): %.0f words (first on CU key %d at word %d, bits %s)", whole(v, "bad_cus"),
         num(v, "mismatches"), whole(v, "first_bad_cu_key"), whole(v, "first_bad_word"), v.get_string("bad_bits", "?").c_str());
  }
  if (is_false(v, "rate_ok")) failures.push_back("LDS rate phase read wrong data");
}
void judge_lds_coverage(const Value& v, const DiagFloors& fl, Value& failures) {
  if (fl.min_lds_cu_coverage > 0 && num(v, "cus") > 0 && num(v, "cus_seen") < fl.min_lds_cu_coverage * num(v, "cus")) {
    fail(failures, "LDS march reached %d of %d CUs", whole(v, "cus_seen"), whole(v, "cus"));
  }
}
void judge_burn(const Value& v, const DiagFloors& fl, Value& failures) {
  if (num(v, "mismatches") > 0) failures.push_back("burn-in MFMA accumulators wrong");
  // the floor is for bf16; an fp8 / fp4 burn is held to it scaled by that path's rate
  const std::string dt = v.get_string("dtype", "bf16");
  int code = BGC_BURN_BF16;  // also what a dtype the burn does not know is judged as
  try {
    code = burn_dtype_code(dt);
  } catch (const std::runtime_error&) {
  }
  const std::string what = "burn-in MFMA " + (code == BGC_BURN_BF16 ? std::string() : "MX " + dt + " ") + "TFLOP/s";
  judge_floor(v, "tflops_mean", fl.min_burn_tflops * burn_dtype_rate_ratio(code), what.c_str(), 0, failures);
  if (fl.min_burn_sustain > 0 && num(v, "sustain") < fl.min_burn_sustain) {
    fail(failures, "MFMA rate sagged to %.2f of its start under sustained load (floor %.2f)", num(v, "sustain"), fl.min_burn_sustain);
  }
  if (fl.max_burn_hotspot_c > 0 && num(v, "max_hotspot_c") > fl.max_burn_hotspot_c) {
    fail(failures, "hotspot %.0f C under sustained load (limit %.0f)", num(v, "max_hotspot_c"), fl.max_burn_hotspot_c);
  }
  if (fl.max_burn_thermal_violation_pct > 0 && num(v, "thermal_violation_pct") > fl.max_burn_thermal_violation_pct) {
    fail(failures, "thermal throttling %.0f%% of the burn (limit %.0f%%)", num(v, "thermal_violation_pct"),
         fl.max_burn_thermal_violation_pct);
  }
}
void judge_pcie(const Value& v, const DiagFloors&, Value& failures) {
  if (num(v, "mismatches") > 0) failures.push_back("PCIe round-trip mismatches: " + std::to_string(count(v, "mismatches")));
}
// link state read right after the copies (amdsmi; absent when unknown)
void judge_pcie_link(const Value& v, const DiagFloors& fl, Value& failures) {
  const double w = num(v, "link_width"), mw = num(v, "max_width");
  if (fl.require_full_pcie_width && w > 0 && mw > 0 && w < mw) {
    failures.push_back("PCIe link x" + std::to_string(static_cast<int>(w)) + " of x" + std::to_string(static_cast<int>(mw)));
  }
  const double sp = num(v, "link_speed_mts"), msp = num(v, "max_speed_mts");
  if (fl.min_pcie_speed_fraction > 0 && sp > 0 && msp > 0 && sp < fl.min_pcie_speed_fraction * msp) {
    fail(failures, "PCIe link at %.0f of %.0f MT/s under load", sp, msp);
  }
}
void judge_soak(const Value& v, const DiagFloors&, Value& failures) {
  if (num(v, "row_mismatches") + num(v, "col_mismatches") > 0) {
    failures.push_back("GEMM soak checksums wrong: " + std::to_string(count(v, "row_mismatches")) + " rows, " +
                       std::to_string(count(v, "col_mismatches")) + " columns");
  }
}
void judge_gemm(const Value& v, const DiagFloors&, Value& failures) {
  if (is_false(v, "passed")) failures.push_back("MFMA GEMM differs from the host fp32 product");
}

}  // namespace

// Written in the order checks() runs the sections, which is the key order of a GPU's published result; the
// burn, a node-level phase, is added to the result last.  The verdict's order differs (the burn before the
// PCIe section, the GEMM last) and is each entry's second field.  A number is {key, floor, what, decimals,
// gauge, help}; a floor that a section's judge_* reads itself (scaled, or not a "below floor" line) has no row.
const std::vector<DiagSection>& diag_sections() {
  using F = DiagFloors;
  using P = const DiagPlan&;
  static const std::vector<DiagSection> table = {
      {"hbm", 0, [](P) { return true; }, run_hbm, scripted_hbm, judge_hbm, nullptr,
       {{"read_gbps", &F::min_read_gbps, "HBM read GB/s", 0, "amd_gpu_diag_hbm_read_gbps", "Diagnostics: HBM read GB/s"},
        {"copy_gbps", &F::min_copy_gbps, "HBM copy GB/s", 0, "amd_gpu_diag_hbm_copy_gbps", "Diagnostics: HBM copy GB/s"},
        {"write_gbps", &F::min_write_gbps, "HBM write GB/s", 0, "amd_gpu_diag_hbm_write_gbps", "Diagnostics: HBM write GB/s"}}},
      {"hbm_walk", 1, [](P p) { return p.hbm_walk_fraction > 0; }, run_hbm_walk, scripted_hbm_walk, judge_hbm_walk, nullptr,
       {{"bytes_covered", nullptr, nullptr, 0, "amd_gpu_diag_hbm_walk_covered_bytes", "Diagnostics: HBM bytes pattern-walked"},
        {"mismatches", nullptr, nullptr, 0, "amd_gpu_diag_hbm_walk_mismatches", "Diagnostics: HBM walk words read back wrong"}}},
      {"mfma", 2, [](P) { return true; }, run_mfma, scripted_mfma, judge_mfma, judge_mfma_xccs,
       {{"tflops", &F::min_mfma_tflops, "MFMA bf16 TFLOP/s", 0, "amd_gpu_diag_mfma_tflops", "Diagnostics: bf16 MFMA TFLOP/s (register operands)"},
        {"xcc_balance", &F::min_xcc_balance, "XCC balance", 2, "amd_gpu_diag_xcc_balance", "Diagnostics: fastest/slowest XCC wave time"}}},
      {"lowp", 3, [](P p) { return p.lowp; }, run_lowp, scripted_lowp, judge_lowp, nullptr,
       {{"fp8_tflops", &F::min_fp8_tflops, "MX fp8 MFMA TFLOP/s", 0, "amd_gpu_diag_fp8_tflops", "Diagnostics: MX fp8 MFMA TFLOP/s (register operands)"},
        {"fp4_tflops", &F::min_fp4_tflops, "MX fp4 MFMA TFLOP/s", 0, "amd_gpu_diag_fp4_tflops", "Diagnostics: MX fp4 MFMA TFLOP/s (register operands)"}}},
      {"classic", 4, [](P p) { return p.classic; }, run_classic, scripted_classic, judge_classic, nullptr,
       {{"fp16_tflops", &F::min_fp16_tflops, "fp16 MFMA TFLOP/s", 0, "amd_gpu_diag_fp16_tflops", "Diagnostics: fp16 MFMA TFLOP/s (register operands)"},
        {"int8_tops", &F::min_int8_tops, "int8 MFMA TOP/s", 0, "amd_gpu_diag_int8_tops", "Diagnostics: int8 MFMA TOP/s (register operands)"},
        {"fp32_tflops", &F::min_fp32_tflops, "fp32 MFMA TFLOP/s", 0, "amd_gpu_diag_fp32_tflops", "Diagnostics: fp32-input MFMA TFLOP/s (register operands)"},
        {"fp64_tflops", &F::min_fp64_tflops, "fp64 MFMA TFLOP/s", 0, "amd_gpu_diag_fp64_tflops", "Diagnostics: fp64 MFMA TFLOP/s (register operands)"},
        {"bad_cus", nullptr, nullptr, 0, "amd_gpu_diag_classic_bad_cus", "Diagnostics: CUs with a wrong fp16 / int8 / fp32 / fp64 MFMA tile element"}}},
      {"lds", 5, [](P p) { return p.lds; }, run_lds, scripted_lds, judge_lds, judge_lds_coverage,
       {{"read_tbps", &F::min_lds_read_tbps, "LDS read TB/s", 1, "amd_gpu_diag_lds_read_tbps", "Diagnostics: LDS read TB/s, all CUs"},
        {"bad_cus", nullptr, nullptr, 0, "amd_gpu_diag_lds_bad_cus", "Diagnostics: CUs whose LDS march read back a wrong word"}}},
      {"gemm", 9, [](P) { return true; }, run_gemm, scripted_gemm, judge_gemm, nullptr, {}},
      {"pcie", 7, [](P p) { return p.pcie_bytes > 0; }, run_pcie, nullptr, judge_pcie, judge_pcie_link,
       {{"h2d_gbps", &F::min_pcie_h2d_gbps, "PCIe host-to-device GB/s", 0, "amd_gpu_diag_pcie_h2d_gbps", "Diagnostics: PCIe host-to-device GB/s"},
        {"d2h_gbps", &F::min_pcie_d2h_gbps, "PCIe device-to-host GB/s", 0, "amd_gpu_diag_pcie_d2h_gbps", "Diagnostics: PCIe device-to-host GB/s"}}},
      {"soak", 8, [](P p) { return p.soak_launches > 0; }, run_soak, scripted_soak, judge_soak, nullptr,
       {{"tflops_mean", &F::min_soak_tflops, "GEMM soak TFLOP/s", 0, "amd_gpu_diag_soak_tflops", "Diagnostics: LDS-tiled MFMA GEMM soak TFLOP/s"}}},
      {"burn", 6, nullptr, nullptr, nullptr, judge_burn, nullptr,
       {{"tflops_mean", nullptr, nullptr, 0, "amd_gpu_diag_burn_tflops", "Diagnostics: burn-in mean MFMA TFLOP/s"},
        {"max_hotspot_c", nullptr, nullptr, 0, "amd_gpu_diag_burn_max_hotspot_celsius", "Diagnostics: burn-in peak hotspot temperature"}}},
  };
  return table;
}

json::Value judge_diag(const json::Value& result, const DiagFloors& fl) {
  std::vector<const DiagSection*> in_verdict_order(diag_sections().size());
  for (const DiagSection& s : diag_sections()) in_verdict_order.at(s.verdict_place) = &s;
  json::Value out = result;
  json::Value failures = json::Value::array();
  for (const DiagSection* s : in_verdict_order) {
    const json::Value& v = result.get(s->name);
    if (!v.is_object()) continue;
    if (s->judge) s->judge(v, fl, failures);
    for (const DiagNumber& n : s->numbers) {
      if (n.floor) judge_floor(v, n.key, fl.*n.floor, n.what, n.decimals, failures);
    }
    if (s->judge_reach) s->judge_reach(v, fl, failures);
  }
  if (result.get("error").is_string()) failures.push_back(result.get_string("error"));
  // a section that failed to run (a HIP fault, a worker that timed out) carries the cause
  // as {"error": ...}: that is a failure in its own right, whatever the floors say
  for (const DiagSection* s : in_verdict_order) {
    const json::Value& v = result.get(s->name);
    if (v.is_object() && v.get("error").is_string()) failures.push_back(std::string(s->name) + ": " + v.get_string("error"));
  }
  out["failures"] = failures;
  out["passed"] = failures.items().empty();
  return out;
}

}  // namespace bgc::gpu
