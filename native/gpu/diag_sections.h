// The sections of the GPU diagnostics, each described once (diag_sections()): when the plan runs it, how the
// HIP engine runs it, what the scripted engine reports for it, its verdict and its named numbers with their
// floors and gauges.  The engines (diag_runner.cc), judge_diag and the node agent's gauges loop over that
// table.  With it: the floors of the verdicts (DiagFloors) and the plan of a pass (DiagPlan).
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "core/json.h"
#include "gpu/diag.h"

namespace bgc::gpu {

class Backend;
struct GpuInfo;

// What one pass runs, and how large.
struct DiagPlan {
  uint64_t hbm_bytes = 1ULL << 30;       // bandwidth phases (two buffers of this size)
  double hbm_walk_fraction = 0.9;        // address-pattern walk of this share of free VRAM (0 = off)
  uint64_t hbm_walk_chunk_bytes = 4ULL << 30;
  int hbm_walk_budget_ms = 20000;
  uint64_t pcie_bytes = 256ULL << 20;    // 0 = off
  int soak_size = 8192;
  int soak_launches = 20;                // 0 = off
  bool lowp = true;                      // MX fp8 / fp4 matrix-core tiles and rates
  bool classic = true;                   // fp16 / int8 / fp32 / fp64 matrix-core tiles and rates
  bool lds = true;                       // per-CU LDS march and LDS read rate
  int burn_ms = 0;                       // node-level burn phase (0 = off)
  int burn_dtype = BGC_BURN_BF16;         // its matrix-core path (bf16, MX fp8, MX fp4)
  // Every field but burn_dtype by its name, in the order of the plan's JSON, which gives burn_dtype as "fp4" last.
  using Field = std::variant<uint64_t DiagPlan::*, double DiagPlan::*, int DiagPlan::*, bool DiagPlan::*>;
  static const std::vector<std::pair<std::string, Field>>& fields();
};
// A key that is absent or of another JSON type than its field keeps the default.
json::Value to_json(const DiagPlan& p);
DiagPlan diag_plan_from_json(const json::Value& v);

// What a section's run is given.
struct DiagRun {
  const GpuInfo& gpu;
  int dev;                            // its HIP device
  const DiagPlan& plan;
  uint32_t seed;
  std::string pcie_lock_path;          // HIP engine: the file PCIe sections of concurrent workers take turns on
  const json::Value* script = nullptr;  // scripted engine: this GPU's entry of the diag script
};

// One named number of a section's result.  With `floor`, the verdict fails "<what> <value> below floor <floor>" (both
// with `decimals`) when the number is below a floor that is not 0; with `gauge`, the node agent publishes it per GPU.
struct DiagNumber {
  const char* key;
  double DiagFloors::*floor;
  const char* what;
  int decimals;
  const char* gauge;
  const char* help;
};

using DiagJudge = void (*)(const json::Value& section, const DiagFloors& floors, json::Value& failures);
struct DiagSection {
  const char* name;   // the key in a GPU's result
  int verdict_place;  // judge_diag gives the sections' failures, and then their run errors, in this order
  bool (*planned)(const DiagPlan&);  // whether checks() runs it; null for the burn, which is a phase of its own
  json::Value (*run)(Diag&, Backend&, const DiagRun&);  // HIP engine
  json::Value (*scripted)(const DiagRun&);              // scripted engine: a healthy result; null = reports nothing
  // The verdict beyond the floors of `numbers`, as code: wrong values before the floors' lines (judge), and
  // what the section must have reached after them (judge_reach).  Either may be null.
  DiagJudge judge, judge_reach;
  std::vector<DiagNumber> numbers;
};

// The table, in the order checks() runs the sections and inserts them into a GPU's result.
const std::vector<DiagSection>& diag_sections();

// Pure verdict over one GPU's results ({"hbm":…, "mfma":…, "gemm":…}): adds "passed" and
// "failures" (one string per violated check) to a copy of `result`.
json::Value judge_diag(const json::Value& result, const DiagFloors& floors);

}  // namespace bgc::gpu
