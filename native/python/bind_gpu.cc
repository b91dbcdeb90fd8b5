// GPU bindings: amdsmi/mock discovery, the telemetry side thread, and the HIP
// diagnostic kernels (dlopen of libbgc_gpu_diag.so).
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <chrono>
#include <memory>

#include "core/json.h"
#include "core/roctx.h"
#include "gpu/device.h"
#include "gpu/diag.h"
#include "gpu/node_agent.h"
#include "gpu/telemetry.h"

namespace py = pybind11;
using bgc::json::Value;

namespace bgc_py {

namespace {

struct PyBackend {
  std::unique_ptr<bgc::gpu::Backend> b;
};

struct PyPoller {
  std::shared_ptr<PyBackend> backend;  // keeps the backend alive
  std::unique_ptr<bgc::gpu::TelemetryPoller> poller;
};

std::string snapshot_json(const bgc::gpu::Snapshot& s) {
  Value v = Value::object();
  v["poll_seq"] = static_cast<unsigned long long>(s.poll_seq);
  v["poll_us"] = s.poll_us;
  Value devs = Value::array();
  for (auto& d : s.devices) devs.push_back(bgc::gpu::to_json(d));
  v["devices"] = devs;
  Value hs = Value::array();
  for (auto& h : s.health) {
    hs.push_back(Value::object({{"index", h.index}, {"healthy", h.healthy}, {"reason", h.reason}}));
  }
  v["health"] = hs;
  v["stalled"] = s.stalled;
  return v.dump();
}

bgc::gpu::HealthPolicy policy_from_json(const std::string& js) {
  bgc::gpu::HealthPolicy p;
  Value v = bgc::json::parse(js.empty() ? "{}" : js);
  auto d = [&](const char* k, double& dst) {
    if (v.get(k).is_number()) dst = v.get(k).as_double();
  };
  auto u = [&](const char* k, uint64_t& dst) {
    if (v.get(k).is_int()) dst = v.get(k).as_uint();
  };
  auto i = [&](const char* k, int& dst) {
    if (v.get(k).is_int()) dst = static_cast<int>(v.get(k).as_int());
  };
  d("max_hotspot_c", p.max_hotspot_c);
  d("max_mem_c", p.max_mem_c);
  u("max_new_uncorrectable", p.max_new_uncorrectable);
  u("max_uncorrectable_at_start", p.max_uncorrectable_at_start);
  if (v.get("require_all_xgmi_links").is_bool()) p.require_all_xgmi_links = v.get("require_all_xgmi_links").as_bool();
  u("max_retired_pages", p.max_retired_pages);
  d("max_thermal_violation_pct", p.max_thermal_violation_pct);
  d("max_ppt_violation_pct", p.max_ppt_violation_pct);
  i("violation_sustain_polls", p.violation_sustain_polls);
  i("fail_threshold", p.fail_threshold);
  i("recover_threshold", p.recover_threshold);
  if (v.get("require_full_pcie_width").is_bool()) p.require_full_pcie_width = v.get("require_full_pcie_width").as_bool();
  if (v.get("max_pcie_replays_per_poll").is_int()) p.max_pcie_replays_per_poll = v.get("max_pcie_replays_per_poll").as_int();
  return p;
}

// Runs a diagnostic (a callable that returns its JSON) with the GIL released; the JSON as text.
template <class Run>
std::string dump_nogil(Run&& run) {
  Value v;
  {
    py::gil_scoped_release nogil;
    v = run();
  }
  return v.dump();
}

// Runs a GEMM that fills an m x n fp32 C with the GIL released; C as bytes.
template <class Run>
py::bytes gemm_nogil(int m, int n, Run&& run) {
  std::string c(static_cast<size_t>(m) * n * 4, '\0');
  {
    py::gil_scoped_release nogil;
    run(reinterpret_cast<float*>(c.data()));
  }
  return py::bytes(c);
}

const uint16_t* u16(const std::string& x) { return reinterpret_cast<const uint16_t*>(x.data()); }
const uint8_t* u8(const std::string& x) { return reinterpret_cast<const uint8_t*>(x.data()); }
template <class T>
int count(const std::vector<T>& v) { return static_cast<int>(v.size()); }

// A planted entry run like Diag's own: "<what>: <last error>" when it fails, the result struct as JSON.
template <class Fn, class... A>
std::string planted(const char* what, Fn entry, A... args) {
  return dump_nogil([&] { return bgc::gpu::Diag::instance().call(what, entry, args...); });
}

using AtomicPlant = std::tuple<int, int, int, int, int, int, int, unsigned>;  // placement, class, word, wave, round, lane, times, mask
std::vector<bgc_atomic_plant> atomic_plants(const std::vector<AtomicPlant>& plants) {
  std::vector<bgc_atomic_plant> c;
  for (const auto& [placement, cls, op, wave, round, lane, times, mask] : plants) c.push_back({placement, cls, op, wave, round, lane, times, mask});
  return c;
}

using AccPlant = std::tuple<int, int, int, int, float>;       // check: wave, round, lane, i, delta; rate: wave, lane, chain, i, delta
using RegfilePlant = std::tuple<int, int, int, int, unsigned>;  // wave or -1, phase, slot, lane, mask
std::vector<bgc_regfile_plant> regfile_plants(const std::vector<RegfilePlant>& plants) {
  std::vector<bgc_regfile_plant> p;
  for (const auto& [wave, phase, slot, lane, mask] : plants) p.push_back({wave, phase, slot, lane, mask});
  return p;
}

using LowpPlant = std::tuple<int, int, int, int, int, float>;  // the variant or path (check), the format or path (rate) or the burn's launch in front

// The MX or the classic planted entry on its plant tuples as the C structs.
template <class Fn>
std::string lowp_planted(const char* what, Fn entry, int device, int waves_per_cu, int iters, unsigned seed,
                         const std::vector<LowpPlant>& check, const std::vector<LowpPlant>& rate) {
  std::vector<bgc_lowp_check_plant> c;
  std::vector<bgc_lowp_rate_plant> r;
  for (const auto& [variant, wave, round, lane, i, delta] : check) c.push_back({variant, {wave, round, lane, i, delta}});
  for (const auto& [fmt, wave, lane, chain, i, delta] : rate) r.push_back({fmt, {wave, lane, chain, i, delta}});
  return planted(what, entry, device, waves_per_cu, iters, seed, c.data(), count(c), r.data(), count(r));
}

// A walk's result plus "chunk_list": [[device address, bytes], ...]
Value with_chunk_list(Value v, const std::vector<bgc_walk_chunk>& chunks) {
  Value list = Value::array();
  for (int c = 0; c < v.get("chunks").as_int() && c < count(chunks); ++c) {
    const bgc_walk_chunk& one = chunks[static_cast<size_t>(c)];
    list.push_back(Value::array({static_cast<unsigned long long>(one.base), static_cast<unsigned long long>(one.bytes)}));
  }
  v["chunk_list"] = list;
  return v;
}

// The host buffer a generated-data entry fills.  A size beyond the library's cap gets an empty one:
// the library refuses that call before it writes.
std::string data_buffer(unsigned long long bytes) { return std::string(bytes <= BGC_DIAG_MAX_DATA_BYTES ? bytes : 0, '\0'); }

}  // namespace

void register_gpu(py::module_& m) {
  py::class_<PyBackend, std::shared_ptr<PyBackend>>(m, "GpuBackend")
      .def_property_readonly("name", [](PyBackend& b) { return b.b->name(); })
      .def("discover", [](PyBackend& b) {
        Value arr = Value::array();
        {
          py::gil_scoped_release nogil;
          for (auto& g : b.b->discover()) arr.push_back(bgc::gpu::to_json(g));
        }
        return arr.dump();
      })
      .def("sample", [](PyBackend& b, int idx, int level) {
        bgc::gpu::Telemetry t;
        {
          py::gil_scoped_release nogil;
          t = b.b->sample(idx, static_cast<bgc::gpu::SampleLevel>(std::clamp(level, 0, 2)));
        }
        return bgc::gpu::to_json(t).dump();
      }, py::arg("index"), py::arg("level") = 2)
      .def("busy_processes", [](PyBackend& b, int idx) { return b.b->busy_processes(idx); });

  m.def("gpu_backend", [](const std::string& kind, const std::string& fixture_json) {
    auto pb = std::make_shared<PyBackend>();
    if (kind == "mock") {
      pb->b = bgc::gpu::make_mock_backend(fixture_json.empty() ? bgc::gpu::default_mi355x_fixture()
                                                               : bgc::json::parse(fixture_json));
    } else {
      pb->b = bgc::gpu::make_backend(kind, "");
    }
    return pb;
  }, py::arg("kind") = "auto", py::arg("fixture_json") = "");

  m.def("default_mi355x_fixture",
        [](int n, uint64_t hive_id) { return bgc::gpu::default_mi355x_fixture(n, hive_id).dump(); }, py::arg("n") = 8,
        py::arg("hive_id") = 0x1a2b3c4d5e6f7788ULL);

  py::class_<PyPoller>(m, "TelemetryPoller")
      .def(py::init([](std::shared_ptr<PyBackend> b, std::vector<int> idx, int interval_ms, const std::string& policy,
                       int slow_every, int ras_every, std::vector<uint64_t> page_limits, int stall_ms) {
             auto p = std::make_unique<PyPoller>();
             p->backend = b;
             p->poller = std::make_unique<bgc::gpu::TelemetryPoller>(
                 *b->b, idx, std::chrono::milliseconds(interval_ms), policy_from_json(policy), slow_every, ras_every,
                 std::move(page_limits));
             p->poller->set_stall_timeout(std::chrono::milliseconds(stall_ms));
             return p;
           }),
           py::arg("backend"), py::arg("indices"), py::arg("interval_ms") = 1000, py::arg("policy") = "{}",
           py::arg("slow_every") = 10, py::arg("ras_every") = 60, py::arg("page_limits") = std::vector<uint64_t>{},
           py::arg("stall_ms") = 0)
      .def("stalled", [](PyPoller& p) { return p.poller->stalled(); })
      .def("start", [](PyPoller& p) { p.poller->start(); })
      .def("stop", [](PyPoller& p) {
        py::gil_scoped_release nogil;
        p.poller->stop();
      })
      .def("poll_once", [](PyPoller& p) {
        py::gil_scoped_release nogil;
        p.poller->poll_once();
      })
      .def("polls", [](PyPoller& p) { return p.poller->polls(); })
      .def("snapshot", [](PyPoller& p) { return snapshot_json(*p.poller->snapshot()); });

  m.def("health_step", [](const std::string& telemetry_json, int fail_threshold, int recover_threshold,
                          const std::string& policy, uint64_t page_limit) {
    // Runs the health state machine over a sequence of telemetry samples (violation
    // percentages are derived from accumulators when a sample carries acc_counter);
    // returns (healthy, reason) after each step.
    bgc::gpu::HealthPolicy pol = policy_from_json(policy);
    pol.fail_threshold = fail_threshold;
    pol.recover_threshold = recover_threshold;
    bgc::gpu::DeviceHealth h;
    h.page_limit = page_limit ? std::min<uint64_t>(page_limit, pol.max_retired_pages) : pol.max_retired_pages;
    const Value pol_json = bgc::json::parse(policy.empty() ? "{}" : policy);
    if (pol_json.get("pcie_max_width").is_int()) {
      h.pcie_max_width = static_cast<int>(pol_json.get("pcie_max_width").as_int());  // capability (discovery)
    }
    bgc::gpu::Telemetry prev;
    std::vector<py::tuple> out;
    Value seq = bgc::json::parse(telemetry_json);
    for (const auto& tv : seq.items()) {
      bgc::gpu::Telemetry t = bgc::gpu::telemetry_from_json(tv);
      if (t.acc_counter != bgc::gpu::Telemetry::kNoAcc) {
        bgc::gpu::TelemetryPoller::violation_deltas(prev, t);
        prev = t;
      }
      bgc::gpu::TelemetryPoller::evaluate(t, pol, h);
      out.push_back(py::make_tuple(h.healthy, h.reason));
    }
    return out;
  }, py::arg("telemetry_json"), py::arg("fail_threshold") = 3, py::arg("recover_threshold") = 3,
     py::arg("policy") = "{}", py::arg("page_limit") = 0);

  // --- HIP diagnostics ---
  using bgc::gpu::Diag;
  m.def("diag_library_path", [](const std::string& p) { return Diag::instance(p).path(); }, py::arg("explicit_path") = "");
  m.def("diag_device_count", [] { return Diag::instance().device_count(); });
  m.def("diag_device_arch", [](int d) { return Diag::instance().device_arch(d); });
  m.def("diag_device_bdf", [](int d) { return Diag::instance().device_bdf(d); });
  m.def("diag_hbm", [](int device, unsigned long long bytes, int iters, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().hbm(device, bytes, iters, seed); });
  }, py::arg("device"), py::arg("bytes") = 2ULL << 30, py::arg("iters") = 3, py::arg("seed") = 0x5eed);
  m.def("diag_mfma", [](int device, int waves_per_cu, int iters, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().mfma(device, waves_per_cu, iters, seed); });
  }, py::arg("device"), py::arg("waves_per_cu") = 32, py::arg("iters") = 4096, py::arg("seed") = 0x5eed);
  m.def("diag_mfma_lowp", [](int device, int waves_per_cu, int iters, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().mfma_lowp(device, waves_per_cu, iters, seed); });
  }, py::arg("device"), py::arg("waves_per_cu") = 32, py::arg("iters") = 4096, py::arg("seed") = 0x5eed);
  m.def("diag_mfma_classic", [](int device, int waves_per_cu, int iters, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().mfma_classic(device, waves_per_cu, iters, seed); });
  }, py::arg("device"), py::arg("waves_per_cu") = 32, py::arg("iters") = 8192, py::arg("seed") = 0x5eed);
  m.def("diag_lds", [](int device, int wgs_per_cu, int rate_iters, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().lds(device, wgs_per_cu, rate_iters, seed); });
  }, py::arg("device"), py::arg("wgs_per_cu") = 4, py::arg("rate_iters") = 8192, py::arg("seed") = 0x5eed);
  m.def("diag_cache", [](int device, int rounds, unsigned region_bytes, int l2_sweeps, unsigned long long ic_bytes, int ic_sweeps,
                         unsigned seed) {
    return dump_nogil([&] { return Diag::instance().cache(device, rounds, region_bytes, l2_sweeps, ic_bytes, ic_sweeps, seed); });
  }, py::arg("device"), py::arg("rounds") = 4, py::arg("region_bytes") = BGC_L2_REGION_BYTES, py::arg("l2_sweeps") = 4096,
     py::arg("ic_bytes") = 128ULL << 20, py::arg("ic_sweeps") = 128, py::arg("seed") = 0x5eed);
  m.def("diag_valu", [](int device, int waves_per_simd, int rounds, int rate_iters, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().valu(device, waves_per_simd, rounds, rate_iters, seed); });
  }, py::arg("device"), py::arg("waves_per_simd") = 2, py::arg("rounds") = 16, py::arg("rate_iters") = 16384, py::arg("seed") = 0x5eed);
  m.def("diag_xlane", [](int device, int waves_per_simd, int rounds, int rate_iters, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().xlane(device, waves_per_simd, rounds, rate_iters, seed); });
  }, py::arg("device"), py::arg("waves_per_simd") = 2, py::arg("rounds") = 16, py::arg("rate_iters") = 16384, py::arg("seed") = 0x5eed);
  m.def("diag_atomic", [](int device, int wgs_per_cu, int rounds, int rate_iters, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().atomic(device, wgs_per_cu, rounds, rate_iters, seed); });
  }, py::arg("device"), py::arg("wgs_per_cu") = 2, py::arg("rounds") = 8, py::arg("rate_iters") = 4095, py::arg("seed") = 0x5eed);
  m.def("diag_regfile", [](int device, int wgs_per_cu, int sweeps, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().regfile(device, wgs_per_cu, sweeps, seed); });
  }, py::arg("device"), py::arg("wgs_per_cu") = 2, py::arg("sweeps") = 4096, py::arg("seed") = 0x5eed);
  m.def("diag_gemm", [](int device, int mm, int nn, int kk, const std::string& a, const std::string& b) {
    if (a.size() != static_cast<size_t>(mm) * kk * 2 || b.size() != static_cast<size_t>(kk) * nn * 2) {
      throw std::invalid_argument("A must be M*K and B K*N bf16 values");
    }
    return gemm_nogil(mm, nn, [&](float* c) { Diag::instance().gemm(device, mm, nn, kk, u16(a), u16(b), c); });
  }, py::arg("device"), py::arg("m"), py::arg("n"), py::arg("k"), py::arg("a_bf16"), py::arg("b_bf16"));
  m.def("diag_gemm_tiled", [](int device, int mm, int nn, int kk, const std::string& a, const std::string& bt) {
    if (a.size() != static_cast<size_t>(mm) * kk * 2 || bt.size() != static_cast<size_t>(nn) * kk * 2) {
      throw std::invalid_argument("A must be M*K and Bt N*K bf16 values");
    }
    return gemm_nogil(mm, nn, [&](float* c) { Diag::instance().gemm_tiled(device, mm, nn, kk, u16(a), u16(bt), c); });
  }, py::arg("device"), py::arg("m"), py::arg("n"), py::arg("k"), py::arg("a_bf16"), py::arg("bt_bf16"));
  m.def("diag_mx_gemm", [](int device, int fmt, int mm, int nn, int kk, const std::string& a, const std::string& sa,
                           const std::string& bt, const std::string& sb) {
    const size_t per = fmt == 0 ? static_cast<size_t>(kk) : static_cast<size_t>(kk) / 2;
    if ((fmt != 0 && fmt != 4) || kk % 128 || a.size() != static_cast<size_t>(mm) * per ||
        bt.size() != static_cast<size_t>(nn) * per || sa.size() != static_cast<size_t>(mm) * (kk / 32) ||
        sb.size() != static_cast<size_t>(nn) * (kk / 32)) {
      throw std::invalid_argument("fmt 0: A M*K, Bt N*K bytes; fmt 4: M*K/2, N*K/2; scales M*K/32 and N*K/32 bytes");
    }
    return gemm_nogil(mm, nn, [&](float* c) {
      Diag::instance().mx_gemm(device, fmt, mm, nn, kk, u8(a), u8(sa), u8(bt), u8(sb), c);
    });
  }, py::arg("device"), py::arg("fmt"), py::arg("m"), py::arg("n"), py::arg("k"), py::arg("a"), py::arg("a_scales"),
     py::arg("bt"), py::arg("bt_scales"));
  // A and B as bytes in classic path `path`'s element type (2, 1, 4, 8 bytes); C as bytes of doubles
  m.def("diag_gemm_dtype", [](int device, int path, int mm, int nn, int kk, const std::string& a, const std::string& b) {
    static const size_t kElemBytes[4] = {2, 1, 4, 8};
    // a shape the library may accept gets its operand sizes checked and a C; any other is refused there
    const bool sized = path >= 0 && path < 4 && mm > 0 && nn > 0 && kk > 0 && mm <= 4096 && nn <= 4096 && kk <= 8192;
    if (sized && (a.size() != static_cast<size_t>(mm) * kk * kElemBytes[path] || b.size() != static_cast<size_t>(kk) * nn * kElemBytes[path])) {
      throw std::invalid_argument("A must be M*K and B K*N elements of the path's type");
    }
    std::string c(sized ? static_cast<size_t>(mm) * nn * sizeof(double) : 0, '\0');
    {
      py::gil_scoped_release nogil;
      Diag::instance().gemm_dtype(device, path, mm, nn, kk, a.data(), b.data(), reinterpret_cast<double*>(c.data()));
    }
    return py::bytes(c);
  }, py::arg("device"), py::arg("path"), py::arg("m"), py::arg("n"), py::arg("k"), py::arg("a"), py::arg("b"));
  m.def("diag_hbm_walk", [](int device, double fraction, unsigned long long chunk_bytes, int budget_ms, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().hbm_walk(device, fraction, chunk_bytes, budget_ms, seed); });
  }, py::arg("device"), py::arg("fraction") = 0.9, py::arg("chunk_bytes") = 4ULL << 30, py::arg("budget_ms") = 20000,
     py::arg("seed") = 0x5eed);
  m.def("diag_gemm_check", [](int device, int mm, int nn, int kk, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().gemm_check(device, mm, nn, kk, seed); });
  }, py::arg("device"), py::arg("m") = 64, py::arg("n") = 64, py::arg("k") = 512, py::arg("seed") = 0x5eed);
  m.def("diag_burn", [](std::shared_ptr<PyBackend> b, int index, int hip_device, int duration_ms, unsigned seed,
                        const std::string& dtype) {
    const int code = bgc::gpu::burn_dtype_code(dtype);
    return dump_nogil([&] { return bgc::gpu::burn_in(*b->b, index, hip_device, duration_ms, seed, nullptr, code); });
  }, py::arg("backend"), py::arg("index"), py::arg("hip_device"), py::arg("duration_ms"), py::arg("seed") = 0x5eed,
     py::arg("dtype") = "bf16");
  m.def("diag_pcie", [](int device, unsigned long long bytes, int iters, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().pcie(device, bytes, iters, seed); });
  }, py::arg("device"), py::arg("bytes") = 256ULL << 20, py::arg("iters") = 5, py::arg("seed") = 0x5eed);
  m.def("diag_gemm_soak", [](int device, int mm, int nn, int kk, int launches, unsigned seed) {
    return dump_nogil([&] { return Diag::instance().gemm_soak(device, mm, nn, kk, launches, seed); });
  }, py::arg("device"), py::arg("m") = 8192, py::arg("n") = 8192, py::arg("k") = 8192, py::arg("launches") = 10,
     py::arg("seed") = 0x5eed);
  // Planted variants (gpu_diag.h): for tests only, so only these bindings resolve their entries, at the
  // call.  Plants are lists of tuples in the order of the C structs' fields; the library checks them
  // ("invalid arguments") before it touches the GPU.
#define BGC_DIAG_ENTRY(name) Diag::instance().entry<decltype(&name)>(#name)
  using u64 = unsigned long long;
  m.def("diag_hbm_planted", [](int device, u64 bytes, unsigned seed, const std::vector<std::tuple<u64, unsigned>>& plants) {
    std::vector<bgc_hbm_plant> p;
    for (const auto& [word, mask] : plants) p.push_back({word, mask});
    return planted("hbm diag", BGC_DIAG_ENTRY(bgc_diag_hbm_planted), device, bytes, seed, p.data(), count(p));
  }, py::arg("device"), py::arg("bytes"), py::arg("seed"), py::arg("plants"));
  m.def("diag_hbm_walk_planted", [](int device, u64 bytes, u64 chunk_bytes, unsigned seed,
                                    const std::vector<std::tuple<int, int, u64, u64>>& plants) {
    std::vector<bgc_walk_plant> p;
    for (const auto& [pass, chunk, offset, mask] : plants) p.push_back({pass, chunk, offset, mask});
    std::vector<bgc_walk_chunk> chunks(1024);
    return dump_nogil([&] {
      return with_chunk_list(Diag::instance().call("hbm walk", BGC_DIAG_ENTRY(bgc_diag_hbm_walk_planted), device, bytes,
                                                   chunk_bytes, seed, p.data(), count(p), chunks.data(), count(chunks)),
                             chunks);
    });
  }, py::arg("device"), py::arg("bytes"), py::arg("chunk_bytes"), py::arg("seed"), py::arg("plants"));
  m.def("diag_pcie_planted", [](int device, u64 bytes, unsigned seed, const std::vector<std::tuple<u64, u64>>& plants) {
    std::vector<bgc_pcie_plant> p;
    for (const auto& [word, mask] : plants) p.push_back({word, mask});
    return planted("pcie diag", BGC_DIAG_ENTRY(bgc_diag_pcie_planted), device, bytes, seed, p.data(), count(p));
  }, py::arg("device"), py::arg("bytes"), py::arg("seed"), py::arg("plants"));
  m.def("diag_mfma_planted", [](int device, int waves_per_cu, int iters, unsigned seed, const std::vector<AccPlant>& check,
                                const std::vector<AccPlant>& rate) {
    std::vector<bgc_mfma_check_plant> c;
    std::vector<bgc_mfma_rate_plant> r;
    for (const auto& [wave, round, lane, i, delta] : check) c.push_back({wave, round, lane, i, delta});
    for (const auto& [wave, lane, chain, i, delta] : rate) r.push_back({wave, lane, chain, i, delta});
    return planted("mfma diag", BGC_DIAG_ENTRY(bgc_diag_mfma_planted), device, waves_per_cu, iters, seed, c.data(), count(c),
                   r.data(), count(r));
  }, py::arg("device"), py::arg("waves_per_cu"), py::arg("iters"), py::arg("seed"), py::arg("check_plants"),
     py::arg("rate_plants"));
  m.def("diag_mfma_lowp_planted", [](int device, int waves_per_cu, int iters, unsigned seed, const std::vector<LowpPlant>& check,
                                     const std::vector<LowpPlant>& rate) {
    return lowp_planted("low-precision mfma diag", BGC_DIAG_ENTRY(bgc_diag_mfma_lowp_planted), device, waves_per_cu, iters, seed, check, rate);
  }, py::arg("device"), py::arg("waves_per_cu"), py::arg("iters"), py::arg("seed"), py::arg("check_plants"),
     py::arg("rate_plants"));
  m.def("diag_mfma_classic_planted", [](int device, int waves_per_cu, int iters, unsigned seed, const std::vector<LowpPlant>& check,
                                        const std::vector<LowpPlant>& rate) {
    return lowp_planted("classic mfma diag", BGC_DIAG_ENTRY(bgc_diag_mfma_classic_planted), device, waves_per_cu, iters, seed, check, rate);
  }, py::arg("device"), py::arg("waves_per_cu"), py::arg("iters"), py::arg("seed"), py::arg("check_plants"),
     py::arg("rate_plants"));
  m.def("diag_lds_planted", [](int device, int wgs_per_cu, int rate_iters, unsigned seed,
                               const std::vector<std::tuple<int, int, unsigned, unsigned>>& plants) {
    std::vector<bgc_lds_plant> p;
    for (const auto& [wg, pass, word, mask] : plants) p.push_back({wg, pass, word, mask});
    return planted("lds diag", BGC_DIAG_ENTRY(bgc_diag_lds_planted), device, wgs_per_cu, rate_iters, seed, p.data(), count(p));
  }, py::arg("device"), py::arg("wgs_per_cu"), py::arg("rate_iters"), py::arg("seed"), py::arg("plants"));
  // L2 plants (round, wg or -1, pass, word of the region, mask) and Infinity-Cache plants (when, word of the buffer, mask)
  m.def("diag_cache_planted", [](int device, int rounds, unsigned region_bytes, int l2_sweeps, u64 ic_bytes, int ic_sweeps, unsigned seed,
                                 const std::vector<std::tuple<int, int, int, unsigned, unsigned>>& l2_plants,
                                 const std::vector<std::tuple<int, u64, unsigned>>& ic_plants) {
    std::vector<bgc_l2_plant> l2;
    std::vector<bgc_ic_plant> ic;
    for (const auto& [round, wg, pass, word, mask] : l2_plants) l2.push_back({round, wg, pass, word, mask});
    for (const auto& [when, word, mask] : ic_plants) ic.push_back({when, word, mask});
    return planted("cache diag", BGC_DIAG_ENTRY(bgc_diag_cache_planted), device, rounds, region_bytes, l2_sweeps, ic_bytes, ic_sweeps,
                   seed, l2.data(), count(l2), ic.data(), count(ic));
  }, py::arg("device"), py::arg("rounds"), py::arg("region_bytes"), py::arg("l2_sweeps"), py::arg("ic_bytes"), py::arg("ic_sweeps"),
     py::arg("seed"), py::arg("l2_plants"), py::arg("ic_plants"));
  // (workgroup or -1, ticks of the constant clock) in the timed L2 rate launch
  m.def("diag_cache_delayed", [](int device, int rounds, unsigned region_bytes, int l2_sweeps, u64 ic_bytes, int ic_sweeps, unsigned seed,
                                 const std::vector<std::tuple<int, unsigned>>& delays) {
    std::vector<bgc_cache_delay_plant> d;
    for (const auto& [wg, ticks] : delays) d.push_back({wg, ticks});
    return planted("cache diag", BGC_DIAG_ENTRY(bgc_diag_cache_delayed), device, rounds, region_bytes, l2_sweeps, ic_bytes, ic_sweeps,
                   seed, d.data(), count(d));
  }, py::arg("device"), py::arg("rounds"), py::arg("region_bytes"), py::arg("l2_sweeps"), py::arg("ic_bytes"), py::arg("ic_sweeps"),
     py::arg("seed"), py::arg("delays"));
  // check plants (wave or -1, class, round, lane, result word, mask) and rate plants (wave or -1, rate class, lane, chain, mask)
  m.def("diag_valu_planted", [](int device, int waves_per_simd, int rounds, int rate_iters, unsigned seed,
                                const std::vector<std::tuple<int, int, int, int, int, unsigned>>& check_plants,
                                const std::vector<std::tuple<int, int, int, int, unsigned>>& rate_plants) {
    std::vector<bgc_valu_plant> c;
    std::vector<bgc_valu_rate_plant> r;
    for (const auto& [wave, cls, round, lane, op, mask] : check_plants) c.push_back({wave, cls, round, lane, op, mask});
    for (const auto& [wave, cls, lane, chain, mask] : rate_plants) r.push_back({wave, cls, lane, chain, mask});
    return planted("valu diag", BGC_DIAG_ENTRY(bgc_diag_valu_planted), device, waves_per_simd, rounds, rate_iters, seed, c.data(), count(c),
                   r.data(), count(r));
  }, py::arg("device"), py::arg("waves_per_simd"), py::arg("rounds"), py::arg("rate_iters"), py::arg("seed"), py::arg("check_plants"),
     py::arg("rate_plants"));
  // (wave or -1, rate class, ticks of the constant clock) in that class's timed rate launch
  m.def("diag_valu_delayed", [](int device, int waves_per_simd, int rounds, int rate_iters, unsigned seed,
                                const std::vector<std::tuple<int, int, unsigned>>& delays) {
    std::vector<bgc_valu_delay_plant> d;
    for (const auto& [wave, cls, ticks] : delays) d.push_back({wave, cls, ticks});
    return planted("valu diag", BGC_DIAG_ENTRY(bgc_diag_valu_delayed), device, waves_per_simd, rounds, rate_iters, seed, d.data(), count(d));
  }, py::arg("device"), py::arg("waves_per_simd"), py::arg("rounds"), py::arg("rate_iters"), py::arg("seed"), py::arg("delays"));
  // the cross-lane check's plants, shaped as the vector ALU's
  m.def("diag_xlane_planted", [](int device, int waves_per_simd, int rounds, int rate_iters, unsigned seed,
                                 const std::vector<std::tuple<int, int, int, int, int, unsigned>>& check_plants,
                                 const std::vector<std::tuple<int, int, int, int, unsigned>>& rate_plants) {
    std::vector<bgc_xlane_plant> c;
    std::vector<bgc_xlane_rate_plant> r;
    for (const auto& [wave, cls, round, lane, op, mask] : check_plants) c.push_back({wave, cls, round, lane, op, mask});
    for (const auto& [wave, cls, lane, chain, mask] : rate_plants) r.push_back({wave, cls, lane, chain, mask});
    return planted("xlane diag", BGC_DIAG_ENTRY(bgc_diag_xlane_planted), device, waves_per_simd, rounds, rate_iters, seed, c.data(), count(c),
                   r.data(), count(r));
  }, py::arg("device"), py::arg("waves_per_simd"), py::arg("rounds"), py::arg("rate_iters"), py::arg("seed"), py::arg("check_plants"),
     py::arg("rate_plants"));
  m.def("diag_xlane_delayed", [](int device, int waves_per_simd, int rounds, int rate_iters, unsigned seed,
                                 const std::vector<std::tuple<int, int, unsigned>>& delays) {
    std::vector<bgc_xlane_delay_plant> d;
    for (const auto& [wave, cls, ticks] : delays) d.push_back({wave, cls, ticks});
    return planted("xlane diag", BGC_DIAG_ENTRY(bgc_diag_xlane_delayed), device, waves_per_simd, rounds, rate_iters, seed, d.data(), count(d));
  }, py::arg("device"), py::arg("waves_per_simd"), py::arg("rounds"), py::arg("rate_iters"), py::arg("seed"), py::arg("delays"));
  // plants (placement, class, word, wave, round, lane, times, mask) and rate plants (rate class, wave, lane, times)
  m.def("diag_atomic_planted", [](int device, int wgs_per_cu, int rounds, int rate_iters, unsigned seed, const std::vector<AtomicPlant>& plants,
                                  const std::vector<std::tuple<int, int, int, int>>& rate_plants) {
    const std::vector<bgc_atomic_plant> c = atomic_plants(plants);
    std::vector<bgc_atomic_rate_plant> r;
    for (const auto& [cls, wave, lane, times] : rate_plants) r.push_back({cls, wave, lane, times});
    return planted("atomic diag", BGC_DIAG_ENTRY(bgc_diag_atomic_planted), device, wgs_per_cu, rounds, rate_iters, seed, c.data(), count(c),
                   r.data(), count(r));
  }, py::arg("device"), py::arg("wgs_per_cu"), py::arg("rounds"), py::arg("rate_iters"), py::arg("seed"), py::arg("plants"), py::arg("rate_plants"));
  // (rate class, wave or -1, ticks of the constant clock) in that class's timed rate launch
  m.def("diag_atomic_delayed", [](int device, int wgs_per_cu, int rounds, int rate_iters, unsigned seed,
                                  const std::vector<std::tuple<int, int, unsigned>>& delays) {
    std::vector<bgc_atomic_delay_plant> d;
    for (const auto& [cls, wave, ticks] : delays) d.push_back({cls, wave, ticks});
    return planted("atomic diag", BGC_DIAG_ENTRY(bgc_diag_atomic_delayed), device, wgs_per_cu, rounds, rate_iters, seed, d.data(), count(d));
  }, py::arg("device"), py::arg("wgs_per_cu"), py::arg("rounds"), py::arg("rate_iters"), py::arg("seed"), py::arg("delays"));
  // Delay plants: (wave or -1, ticks of the constant clock) in the timed throughput launch; and a burn
  // whose launches from `first_delayed_launch` on have every wave delayed by `ticks`.
  m.def("diag_mfma_delayed", [](int device, int waves_per_cu, int iters, unsigned seed,
                                const std::vector<std::tuple<int, unsigned>>& delays) {
    std::vector<bgc_mfma_delay_plant> d;
    for (const auto& [wave, ticks] : delays) d.push_back({wave, ticks});
    return planted("mfma diag", BGC_DIAG_ENTRY(bgc_diag_mfma_delayed), device, waves_per_cu, iters, seed, d.data(), count(d));
  }, py::arg("device"), py::arg("waves_per_cu"), py::arg("iters"), py::arg("seed"), py::arg("delays"));
  m.def("diag_burn_delayed", [](int device, int duration_ms, int waves_per_cu, unsigned seed, const std::string& dtype,
                                int first_delayed_launch, unsigned ticks) {
    const int code = bgc::gpu::burn_dtype_code(dtype);
    return dump_nogil([&] {
      bgc_burn_result r{};
      Diag::instance().check("burn", BGC_DIAG_ENTRY(bgc_diag_burn_delayed)(device, duration_ms, waves_per_cu, seed, code,
                                                                           first_delayed_launch, ticks, &r));
      return bgc::gpu::to_json(r, code);
    });
  }, py::arg("device"), py::arg("duration_ms"), py::arg("waves_per_cu"), py::arg("seed"), py::arg("dtype"),
     py::arg("first_delayed_launch"), py::arg("ticks"));
  // The burn with value plants: (launch, wave, lane, chain, i, delta), applied in that launch of the burn.
  m.def("diag_burn_planted", [](int device, int duration_ms, int waves_per_cu, unsigned seed, const std::string& dtype,
                                const std::vector<LowpPlant>& plants) {
    const int code = bgc::gpu::burn_dtype_code(dtype);
    std::vector<bgc_burn_plant> p;
    for (const auto& [launch, wave, lane, chain, i, delta] : plants) p.push_back({launch, {wave, lane, chain, i, delta}});
    return dump_nogil([&] {
      bgc_burn_result r{};
      Diag::instance().check("burn", BGC_DIAG_ENTRY(bgc_diag_burn_planted)(device, duration_ms, waves_per_cu, seed, code, p.data(),
                                                                           count(p), &r));
      return bgc::gpu::to_json(r, code);
    });
  }, py::arg("device"), py::arg("duration_ms"), py::arg("waves_per_cu"), py::arg("seed"), py::arg("dtype"), py::arg("plants"));
  m.def("diag_gemm_soak_planted", [](int device, int mm, int nn, int kk, int launches, unsigned seed,
                                     const std::vector<std::tuple<int, int, int, float>>& plants) {
    std::vector<bgc_soak_plant> p;
    for (const auto& [launch, row, col, delta] : plants) p.push_back({launch, row, col, delta});
    return planted("gemm soak", BGC_DIAG_ENTRY(bgc_diag_gemm_soak_planted), device, mm, nn, kk, launches, seed, p.data(),
                   count(p));
  }, py::arg("device"), py::arg("m"), py::arg("n"), py::arg("k"), py::arg("launches"), py::arg("seed"), py::arg("plants"));
  // Generated data (gpu_diag.h): for tests only and resolved here alike.  Each returns the result JSON
  // followed by the data as bytes.
  m.def("diag_hbm_data", [](int device, u64 bytes, int iters, unsigned seed) {
    std::string data = data_buffer(bytes & ~15ULL);
    const std::string r = planted("hbm diag", BGC_DIAG_ENTRY(bgc_diag_hbm_data), device, bytes, iters, seed,
                                  static_cast<void*>(data.data()));
    return py::make_tuple(r, py::bytes(data));
  }, py::arg("device"), py::arg("bytes"), py::arg("iters"), py::arg("seed"));
  m.def("diag_hbm_walk_data", [](int device, u64 bytes, u64 chunk_bytes, int passes, unsigned seed) {
    std::string data = data_buffer(bytes & ~((2ULL << 20) - 1));
    std::vector<bgc_walk_chunk> chunks(64);  // 128 MiB at most, in chunks of at least 64 MiB
    const std::string r = dump_nogil([&] {
      return with_chunk_list(Diag::instance().call("hbm walk", BGC_DIAG_ENTRY(bgc_diag_hbm_walk_data), device, bytes, chunk_bytes,
                                                   passes, seed, chunks.data(), count(chunks), static_cast<void*>(data.data())),
                             chunks);
    });
    return py::make_tuple(r, py::bytes(data));
  }, py::arg("device"), py::arg("bytes"), py::arg("chunk_bytes"), py::arg("passes"), py::arg("seed"));
  m.def("diag_pcie_data", [](int device, u64 bytes, unsigned seed) {
    std::string data = data_buffer(bytes & ~7ULL);
    const std::string r = planted("pcie diag", BGC_DIAG_ENTRY(bgc_diag_pcie_data), device, bytes, seed, static_cast<void*>(data.data()));
    return py::make_tuple(r, py::bytes(data));
  }, py::arg("device"), py::arg("bytes"), py::arg("seed"));
  m.def("diag_gemm_soak_data", [](int device, int mm, int nn, int kk, unsigned seed) {
    // the sizes of a shape the library may accept; any other gets empty buffers and is refused there
    const bool sized = mm > 0 && nn > 0 && kk > 0 && mm <= 32768 && nn <= 32768 && kk <= 32768;
    const u64 um = sized ? mm : 0, un = sized ? nn : 0, uk = sized ? kk : 0;
    const bool fits = 2 * um * uk + 2 * un * uk + 4 * um * un + 8 * (um + un) <= BGC_DIAG_MAX_DATA_BYTES;
    auto buffer = [&](u64 bytes) { return std::string(fits ? bytes : 0, '\0'); };
    std::string a = buffer(2 * um * uk), bt = buffer(2 * un * uk), rref = buffer(8 * um), cref = buffer(8 * un), c = buffer(4 * um * un);
    const bgc_soak_data data = {reinterpret_cast<uint16_t*>(a.data()), reinterpret_cast<uint16_t*>(bt.data()),
                                reinterpret_cast<int64_t*>(rref.data()), reinterpret_cast<int64_t*>(cref.data()),
                                reinterpret_cast<float*>(c.data())};
    const std::string r = planted("gemm soak", BGC_DIAG_ENTRY(bgc_diag_gemm_soak_data), device, mm, nn, kk, seed, &data);
    return py::make_tuple(r, py::bytes(a), py::bytes(bt), py::bytes(rref), py::bytes(cref), py::bytes(c));
  }, py::arg("device"), py::arg("m"), py::arg("n"), py::arg("k"), py::arg("seed"));
  // the 64 bgc_tile_lane of one tile, as bytes
  m.def("diag_mfma_tile", [](int device, int path, int scaled, unsigned seed, unsigned tile) {
    std::string lanes(64 * sizeof(bgc_tile_lane), '\0');
    {
      py::gil_scoped_release nogil;
      Diag::instance().check("mfma tile", BGC_DIAG_ENTRY(bgc_diag_mfma_tile)(device, path, scaled, seed, tile,
                                                                             reinterpret_cast<bgc_tile_lane*>(lanes.data())));
    }
    return py::bytes(lanes);
  }, py::arg("device"), py::arg("path"), py::arg("scaled"), py::arg("seed"), py::arg("tile"));
  // the 64 bgc_classic_tile_lane of one classic-path tile, as bytes
  m.def("diag_mfma_classic_tile", [](int device, int path, unsigned seed, unsigned tile) {
    std::string lanes(64 * sizeof(bgc_classic_tile_lane), '\0');
    {
      py::gil_scoped_release nogil;
      Diag::instance().check("classic mfma tile", BGC_DIAG_ENTRY(bgc_diag_mfma_classic_tile)(
                                                      device, path, seed, tile, reinterpret_cast<bgc_classic_tile_lane*>(lanes.data())));
    }
    return py::bytes(lanes);
  }, py::arg("device"), py::arg("path"), py::arg("seed"), py::arg("tile"));
  // the BGC_LDS_WORDS words of one march workgroup, as bytes
  m.def("diag_lds_data", [](int device, unsigned seed, int wg, int pass, int grid) {
    std::string data(4 * BGC_LDS_WORDS, '\0');
    {
      py::gil_scoped_release nogil;
      Diag::instance().check("lds diag", BGC_DIAG_ENTRY(bgc_diag_lds_data)(device, seed, wg, pass, grid, static_cast<void*>(data.data())));
    }
    return py::bytes(data);
  }, py::arg("device"), py::arg("seed"), py::arg("wg"), py::arg("pass"), py::arg("grid"));
  // the result, the L2 buffer (cus regions) and the Infinity-Cache buffer, as bytes.  The destination holds the L2
  // buffer of up to 512 CUs; a request that exceeds the library's cap with it gets empty buffers and is refused there.
  m.def("diag_cache_data", [](int device, int rounds, unsigned region_bytes, int passes, int l2_sweeps, u64 ic_bytes, int ic_sweeps,
                              unsigned seed) {
    const u64 capacity = region_bytes <= 4 * BGC_L2_SLAB_BYTES ? 512ULL * region_bytes : 0;
    const bool fits = ic_bytes <= BGC_DIAG_MAX_DATA_BYTES && capacity + ic_bytes <= BGC_DIAG_MAX_DATA_BYTES;
    std::string l2(fits ? capacity : 0, '\0'), ic(fits ? ic_bytes : 0, '\0');
    Value v;
    {
      py::gil_scoped_release nogil;
      v = Diag::instance().call("cache diag", BGC_DIAG_ENTRY(bgc_diag_cache_data), device, rounds, region_bytes, passes, l2_sweeps,
                                ic_bytes, ic_sweeps, seed, static_cast<void*>(l2.data()), capacity, static_cast<void*>(ic.data()));
    }
    l2.resize(static_cast<size_t>(v.get("cus").as_int()) * region_bytes);
    return py::make_tuple(v.dump(), py::bytes(l2), py::bytes(ic));
  }, py::arg("device"), py::arg("rounds"), py::arg("region_bytes"), py::arg("passes"), py::arg("l2_sweeps"), py::arg("ic_bytes"),
     py::arg("ic_sweeps"), py::arg("seed"));
  // the result and one check wave as bytes of bgc_valu_wave; and the host referee's expectation alike, without a device
  m.def("diag_valu_data", [](int device, int waves_per_simd, int rounds, int rate_iters, unsigned seed, int wave,
                             const std::vector<std::tuple<int, int, int, int, int, unsigned>>& check_plants,
                             const std::vector<std::tuple<int, int, int, int, unsigned>>& rate_plants,
                             const std::vector<std::tuple<int, int, unsigned>>& delays) {
    std::vector<bgc_valu_plant> c;
    std::vector<bgc_valu_rate_plant> r;
    std::vector<bgc_valu_delay_plant> d;
    for (const auto& [w, cls, round, lane, op, mask] : check_plants) c.push_back({w, cls, round, lane, op, mask});
    for (const auto& [w, cls, lane, chain, mask] : rate_plants) r.push_back({w, cls, lane, chain, mask});
    for (const auto& [w, cls, ticks] : delays) d.push_back({w, cls, ticks});
    std::string data(sizeof(bgc_valu_wave), '\0');
    const std::string result = planted("valu diag", BGC_DIAG_ENTRY(bgc_diag_valu_data), device, waves_per_simd, rounds, rate_iters, seed, wave,
                                       c.data(), count(c), r.data(), count(r), d.data(), count(d), reinterpret_cast<bgc_valu_wave*>(data.data()));
    return py::make_tuple(result, py::bytes(data));
  }, py::arg("device"), py::arg("waves_per_simd"), py::arg("rounds"), py::arg("rate_iters"), py::arg("seed"), py::arg("wave"),
     py::arg("check_plants"), py::arg("rate_plants"), py::arg("delays"));
  m.def("diag_valu_expected", [](unsigned seed, int rounds) {
    std::string data(sizeof(bgc_valu_wave), '\0');
    Diag::instance().check("valu diag", BGC_DIAG_ENTRY(bgc_diag_valu_expected)(seed, rounds, reinterpret_cast<bgc_valu_wave*>(data.data())));
    return py::bytes(data);
  }, py::arg("seed"), py::arg("rounds"));
  // the same for the cross-lane check, as bytes of bgc_xlane_wave
  m.def("diag_xlane_data", [](int device, int waves_per_simd, int rounds, int rate_iters, unsigned seed, int wave,
                              const std::vector<std::tuple<int, int, int, int, int, unsigned>>& check_plants,
                              const std::vector<std::tuple<int, int, int, int, unsigned>>& rate_plants,
                              const std::vector<std::tuple<int, int, unsigned>>& delays) {
    std::vector<bgc_xlane_plant> c;
    std::vector<bgc_xlane_rate_plant> r;
    std::vector<bgc_xlane_delay_plant> d;
    for (const auto& [w, cls, round, lane, op, mask] : check_plants) c.push_back({w, cls, round, lane, op, mask});
    for (const auto& [w, cls, lane, chain, mask] : rate_plants) r.push_back({w, cls, lane, chain, mask});
    for (const auto& [w, cls, ticks] : delays) d.push_back({w, cls, ticks});
    std::string data(sizeof(bgc_xlane_wave), '\0');
    const std::string result = planted("xlane diag", BGC_DIAG_ENTRY(bgc_diag_xlane_data), device, waves_per_simd, rounds, rate_iters, seed, wave,
                                       c.data(), count(c), r.data(), count(r), d.data(), count(d), reinterpret_cast<bgc_xlane_wave*>(data.data()));
    return py::make_tuple(result, py::bytes(data));
  }, py::arg("device"), py::arg("waves_per_simd"), py::arg("rounds"), py::arg("rate_iters"), py::arg("seed"), py::arg("wave"),
     py::arg("check_plants"), py::arg("rate_plants"), py::arg("delays"));
  m.def("diag_xlane_expected", [](unsigned seed, int rounds) {
    std::string data(sizeof(bgc_xlane_wave), '\0');
    Diag::instance().check("xlane diag", BGC_DIAG_ENTRY(bgc_diag_xlane_expected)(seed, rounds, reinterpret_cast<bgc_xlane_wave*>(data.data())));
    return py::bytes(data);
  }, py::arg("seed"), py::arg("rounds"));
  // bgc_atomic_layout as bytes; the result and the run's data block (sized for a device of up to 512 CUs, and at most the
  // library's cap, where a larger run is refused) as bytes; the referee's block; a rate class's end values
  m.def("diag_atomic_layout", [](int grid, int rate_grid, int rounds) {
    std::string layout(sizeof(bgc_atomic_layout), '\0');
    Diag::instance().check("atomic diag", BGC_DIAG_ENTRY(bgc_diag_atomic_layout)(grid, rate_grid, rounds, reinterpret_cast<bgc_atomic_layout*>(layout.data())));
    return py::bytes(layout);
  }, py::arg("grid"), py::arg("rate_grid"), py::arg("rounds"));
  m.def("diag_atomic_data", [](int device, int wgs_per_cu, int rounds, int rate_iters, unsigned seed, const std::vector<AtomicPlant>& plants,
                               const std::vector<std::tuple<int, int, int, int>>& rate_plants, const std::vector<std::tuple<int, int, unsigned>>& delays) {
    const std::vector<bgc_atomic_plant> c = atomic_plants(plants);
    std::vector<bgc_atomic_rate_plant> r;
    std::vector<bgc_atomic_delay_plant> d;
    for (const auto& [cls, wave, lane, times] : rate_plants) r.push_back({cls, wave, lane, times});
    for (const auto& [cls, wave, ticks] : delays) d.push_back({cls, wave, ticks});
    bgc_atomic_layout layout{};
    u64 capacity = 0;
    if (wgs_per_cu >= 1 && wgs_per_cu <= 8 && BGC_DIAG_ENTRY(bgc_diag_atomic_layout)(512 * wgs_per_cu, 1024, rounds, &layout) == 0) {
      capacity = std::min<u64>(layout.total_words * 4, BGC_DIAG_MAX_DATA_BYTES);
    }
    std::string data(capacity, '\0');
    Value v;
    {
      py::gil_scoped_release nogil;
      v = Diag::instance().call("atomic diag", BGC_DIAG_ENTRY(bgc_diag_atomic_data), device, wgs_per_cu, rounds, rate_iters, seed, c.data(), count(c),
                                r.data(), count(r), d.data(), count(d), static_cast<void*>(data.data()), capacity);
    }
    const int cus = static_cast<int>(v.get("cus").as_int());
    Diag::instance().check("atomic diag", BGC_DIAG_ENTRY(bgc_diag_atomic_layout)(cus * wgs_per_cu, (2 * cus + 7) / 8 * 8, rounds, &layout));
    data.resize(layout.total_words * 4);
    return py::make_tuple(v.dump(), py::bytes(data));
  }, py::arg("device"), py::arg("wgs_per_cu"), py::arg("rounds"), py::arg("rate_iters"), py::arg("seed"), py::arg("plants"), py::arg("rate_plants"),
     py::arg("delays"));
  m.def("diag_atomic_expected", [](unsigned seed, int grid, int rounds, const std::vector<AtomicPlant>& plants) {
    const std::vector<bgc_atomic_plant> c = atomic_plants(plants);
    bgc_atomic_layout layout{};
    const bool sized = BGC_DIAG_ENTRY(bgc_diag_atomic_layout)(grid, 8, rounds, &layout) == 0 && layout.total_words * 4 <= BGC_DIAG_MAX_DATA_BYTES;
    std::string data(sized ? layout.total_words * 4 : 0, '\0');
    {
      py::gil_scoped_release nogil;
      Diag::instance().check("atomic diag", BGC_DIAG_ENTRY(bgc_diag_atomic_expected)(seed, grid, rounds, c.data(), count(c), static_cast<void*>(data.data()),
                                                                                     data.size()));
    }
    return py::bytes(data);
  }, py::arg("seed"), py::arg("grid"), py::arg("rounds"), py::arg("plants"));
  m.def("diag_atomic_rate_expected", [](unsigned seed, int rate_grid, int rate_iters, int cls) {
    const bool sized = rate_grid >= 8 && rate_grid <= 4096;
    std::string data(sized ? static_cast<size_t>(rate_grid) / 8 * 4 * (cls == BGC_ATOMIC_RATE_RTN ? 1 : 4096) * 4 : 0, '\0');
    Diag::instance().check("atomic diag", BGC_DIAG_ENTRY(bgc_diag_atomic_rate_expected)(seed, rate_grid, rate_iters, cls,
                                                                                          reinterpret_cast<uint32_t*>(data.data()), data.size() / 4));
    return py::bytes(data);
  }, py::arg("seed"), py::arg("rate_grid"), py::arg("rate_iters"), py::arg("cls"));
  // register-file plants (wave or -1, phase, slot, lane, mask) and delays (wave or -1, ticks of the constant clock)
  m.def("diag_regfile_planted", [](int device, int wgs_per_cu, int sweeps, unsigned seed, const std::vector<RegfilePlant>& plants) {
    const std::vector<bgc_regfile_plant> p = regfile_plants(plants);
    return planted("regfile diag", BGC_DIAG_ENTRY(bgc_diag_regfile_planted), device, wgs_per_cu, sweeps, seed, p.data(), count(p));
  }, py::arg("device"), py::arg("wgs_per_cu"), py::arg("sweeps"), py::arg("seed"), py::arg("plants"));
  m.def("diag_regfile_delayed", [](int device, int wgs_per_cu, int sweeps, unsigned seed, const std::vector<std::tuple<int, unsigned>>& delays) {
    std::vector<bgc_regfile_delay_plant> d;
    for (const auto& [wave, ticks] : delays) d.push_back({wave, ticks});
    return planted("regfile diag", BGC_DIAG_ENTRY(bgc_diag_regfile_delayed), device, wgs_per_cu, sweeps, seed, d.data(), count(d));
  }, py::arg("device"), py::arg("wgs_per_cu"), py::arg("sweeps"), py::arg("seed"), py::arg("delays"));
  // the result, the wave's 512 x 64 words, and every wave's (CU key, SIMD) of the march and of the timed rotate launch
  // (room for a device of 512 CUs), as bytes
  m.def("diag_regfile_data", [](int device, int wgs_per_cu, int sweeps, unsigned seed, int wave, int phase, const std::vector<RegfilePlant>& plants,
                                const std::vector<std::tuple<int, unsigned>>& delays) {
    const std::vector<bgc_regfile_plant> p = regfile_plants(plants);
    std::vector<bgc_regfile_delay_plant> d;
    for (const auto& [w, ticks] : delays) d.push_back({w, ticks});
    const int max_waves = 512 * 8 * 4;
    std::string words(BGC_REGFILE_REGS * 64 * 4, '\0'), march(max_waves * sizeof(bgc_regfile_place), '\0'), rotate(march.size(), '\0');
    Value v;
    {
      py::gil_scoped_release nogil;
      v = Diag::instance().call("regfile diag", BGC_DIAG_ENTRY(bgc_diag_regfile_data), device, wgs_per_cu, sweeps, seed, wave, phase, p.data(), count(p),
                                d.data(), count(d), reinterpret_cast<uint32_t*>(words.data()), reinterpret_cast<bgc_regfile_place*>(march.data()),
                                reinterpret_cast<bgc_regfile_place*>(rotate.data()), max_waves);
    }
    const size_t waves = static_cast<size_t>(v.get("cus").as_int()) * wgs_per_cu * 4;
    march.resize(waves * sizeof(bgc_regfile_place));
    rotate.resize(waves * sizeof(bgc_regfile_place));
    return py::make_tuple(v.dump(), py::bytes(words), py::bytes(march), py::bytes(rotate));
  }, py::arg("device"), py::arg("wgs_per_cu"), py::arg("sweeps"), py::arg("seed"), py::arg("wave"), py::arg("phase"), py::arg("plants"),
     py::arg("delays"));
  m.def("diag_regfile_layout", [] {
    std::string layout(sizeof(bgc_regfile_layout), '\0');
    Diag::instance().check("regfile diag", BGC_DIAG_ENTRY(bgc_diag_regfile_layout)(reinterpret_cast<bgc_regfile_layout*>(layout.data())));
    return py::bytes(layout);
  });
  m.def("diag_regfile_expected", [](unsigned seed, int wave, int phase, int sweeps, const std::vector<RegfilePlant>& plants) {
    const std::vector<bgc_regfile_plant> p = regfile_plants(plants);
    std::string words(BGC_REGFILE_REGS * 64 * 4, '\0');
    Diag::instance().check("regfile diag", BGC_DIAG_ENTRY(bgc_diag_regfile_expected)(seed, wave, phase, sweeps, p.data(), count(p),
                                                                                     reinterpret_cast<uint32_t*>(words.data())));
    return py::bytes(words);
  }, py::arg("seed"), py::arg("wave"), py::arg("phase"), py::arg("sweeps"), py::arg("plants"));
  m.def("diag_valu_trans_ulps", [] {
    return py::make_tuple(BGC_VALU_EXP_ULPS, BGC_VALU_LOG_ULPS, BGC_VALU_RCP_ULPS, BGC_VALU_RSQ_ULPS, BGC_VALU_SQRT_ULPS);
  });
#undef BGC_DIAG_ENTRY
  m.def("pcie_check", [](std::shared_ptr<PyBackend> b, int index, int hip_device, unsigned long long bytes, unsigned seed) {
    return dump_nogil([&] {
      auto gpus = b->b->discover();
      if (index < 0 || static_cast<size_t>(index) >= gpus.size()) throw std::out_of_range("no such GPU");
      return bgc::gpu::pcie_check(*b->b, gpus[static_cast<size_t>(index)], hip_device, bytes, seed);
    });
  }, py::arg("backend"), py::arg("index"), py::arg("hip_device"), py::arg("bytes") = 256ULL << 20, py::arg("seed") = 0x5eed);
  m.def("judge_diag", [](const std::string& result, const std::string& floors_json) {
    bgc::gpu::DiagFloors f = bgc::gpu::DiagFloors::mi355x_defaults();
    const Value fj = bgc::json::parse(floors_json);
    f.apply([&](const std::string& name, auto& v) {  // a floor of another JSON type than its field is ignored
      const Value& j = fj.get(name);
      if constexpr (std::is_same_v<decltype(v), double&>) {
        if (j.is_number()) v = j.as_double();
      } else if constexpr (std::is_same_v<decltype(v), bool&>) {
        if (j.is_bool()) v = j.as_bool();
      } else if (j.is_int()) {
        v = static_cast<int>(j.as_int());
      }
    });
    return bgc::gpu::judge_diag(bgc::json::parse(result), f).dump();
  }, py::arg("result"), py::arg("floors") = "{}");
  m.def("roctx_available", &bgc::roctx::available);

  // Node agent rendering (pure functions).
  m.def("node_patches", [](const std::string& gpus_json, int healthy, const std::string& node, bool diag_ran,
                           bool diag_passed, const std::string& reason) {
    bgc::gpu::NodeAgentConfig cfg;
    cfg.node_name = node;
    std::vector<bgc::gpu::GpuInfo> gpus;
    bgc::json::Value parsed = bgc::json::parse(gpus_json);
    for (const auto& g : parsed.items()) gpus.push_back(bgc::gpu::gpu_info_from_json(g));
    bgc::gpu::DiagOutcome d;
    d.ran = diag_ran;
    d.passed = diag_passed;
    return py::make_tuple(bgc::gpu::node_labels_patch(cfg, gpus, healthy, d).dump(),
                          bgc::gpu::node_status_patch(cfg, gpus, healthy, reason).dump());
  }, py::arg("gpus_json"), py::arg("healthy"), py::arg("node") = "node-0", py::arg("diag_ran") = false,
     py::arg("diag_passed") = true, py::arg("reason") = "");
  m.def("sanitize_label_value", &bgc::gpu::sanitize_label_value);
}

}  // namespace bgc_py
