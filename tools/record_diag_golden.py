"""Record what the diagnostics' verdict and the node agent's diagnostics gauges give today:

    python3 tools/record_diag_golden.py        # rewrites both files under tests/golden/

* diag_verdicts.json: [{name, result, floors, judged_text}], one case per line of judge_diag
  that can append a failure, named after the line it reaches, plus a
  clean result, every floor at 0, floors of the wrong JSON type and every failure at once.
  `judged_text` is the text judge_diag returns for (result, floors).
* diag_gauges.txt: every line of a node agent's /metrics that contains "amd_gpu_diag_", then the
  "diag" array of its /gpus without the timing fields, one GPU per line.  The agent runs the
  scripted engine on a mock backend (scripted_pass below).

tests/unit/test_judge_golden.py and tests/integration/test_diag_gauges_golden.py compare a build
with these files; record them again only when a change to the verdict or the gauges is meant.
"""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

CLEAN = {
    "hbm": {"device": 0, "bytes": 1 << 30, "iters": 2, "write_gbps": 5200.5, "read_gbps": 6400.25, "copy_gbps": 5400.0,
            "mismatches": 0, "first_bad_word": None, "elapsed_ms": 1.75, "passed": True},
    "hbm_walk": {"device": 0, "free_bytes": 300 << 30, "total_bytes": 309 << 30, "target_bytes": 270 << 30,
                 "bytes_covered": 270 << 30, "coverage_of_free": 0.9, "chunks": 68, "passes": 2, "mismatches": 0,
                 "first_bad_addr": None, "first_bad_bits": None, "write_gbps": 4100.0, "read_gbps": 4900.0, "alloc_ms": 12.5,
                 "elapsed_ms": 310.0, "budget_hit": False, "passed": True},
    "mfma": {"device": 0, "tiles_checked": 32768, "mismatches": 0, "cus_seen": 256, "xccs_seen": 8, "bad_cus": 0,
             "bad_cu_keys": [], "tflops": 2000.0, "throughput_ok": True, "xcc_waves": [512] * 8, "xcc_wave_us": [410.5] * 8,
             "xcc_balance": 0.96, "elapsed_ms": 1.5, "passed": True},
    "lowp": {"device": 0, "tiles_checked": 65536, "fp8_mismatches": 0, "fp8_scaled_mismatches": 0, "fp4_mismatches": 0,
             "fp4_scaled_mismatches": 0, "mismatches": 0, "cus_seen": 256, "bad_cus": 0, "bad_cu_keys": [], "fp8_tflops": 4400.0,
             "fp4_tflops": 7700.0, "throughput_ok": True, "elapsed_ms": 5.25, "passed": True},
    "classic": {"device": 0, "tiles_checked": 4 * 8192 * 4, "fp16_mismatches": 0, "int8_mismatches": 0, "fp32_mismatches": 0,
                "fp64_mismatches": 0, "mismatches": 0, "cus_seen": 256, "bad_cus": 0, "bad_cu_keys": [], "fp16_tflops": 2100.0,
                "int8_tops": 4000.0, "fp32_tflops": 150.0, "fp64_tflops": 77.5, "rate_ms": [2.2, 2.2, 3.6, 7.2],
                "throughput_ok": True, "elapsed_ms": 16.0, "passed": True},
    "lds": {"device": 0, "cus": 256, "cus_seen": 256, "bad_cus": 0, "bad_cu_keys": [], "words_checked": 2 * 40960 * 4 * 256,
            "mismatches": 0, "first_bad_cu_key": None, "first_bad_word": None, "bad_bits": None, "read_tbps": 118.5,
            "rate_ok": True, "slowest_cu_key": 17, "cu_balance": 0.97, "elapsed_ms": 3.5, "passed": True},
    "gemm": {"m": 64, "n": 64, "k": 512, "max_abs_err": 1.5e-6, "max_err_over_bound": 0.01, "bad_elements": 0, "passed": True},
    "pcie": {"device": 0, "bytes": 256 << 20, "iters": 5, "h2d_gbps": 57.1, "d2h_gbps": 56.7, "bidir_gbps": 97.0,
             "mismatches": 0, "elapsed_ms": 48.0, "passed": True, "link_width": 16, "link_speed_mts": 32000, "max_width": 16,
             "max_speed_mts": 32000, "max_gen": 5, "replays": 0, "recoveries": 0, "serialized": True},
    "soak": {"device": 0, "m": 8192, "n": 8192, "k": 8192, "launches": 20, "tile": 256, "kernel": "pingpong",
             "elapsed_ms": 15.0, "tflops_mean": 1500.0, "tflops_best": 1580.0, "row_mismatches": 0, "col_mismatches": 0,
             "passed": True},
    "timing_ms": {"hbm": 2.0, "soak": 15.5},
    "index": 0,
    "hip_device": 0,
    "burn": {"dtype": "bf16", "launches": 950, "elapsed_ms": 2000.5, "tflops_mean": 2410.0, "tflops_min": 2380.0,
             "tflops_first": 2440.0, "tflops_last": 2405.0, "tflops_max": 2440.0, "sustain": 0.9856, "mismatches": 0,
             "samples": 19, "max_hotspot_c": 81.0, "max_mem_c": 70.0, "power_mean_w": 1150.0, "power_max_w": 1210.0,
             "gfxclk_mean_mhz": 2350.0, "gfxclk_min_mhz": 2300.0, "thermal_violation_pct": 0.0, "ppt_violation_pct": 12.5},
}
# the order in which judge_diag gives its failures
JUDGE_ORDER = ["hbm", "hbm_walk", "mfma", "lowp", "classic", "lds", "burn", "pcie", "soak", "gemm"]
# every field of DiagFloors; all at 0 (false) turns every floor off
FLOORS_OFF = {name: 0 for name in (
    "min_read_gbps", "min_copy_gbps", "min_write_gbps", "min_mfma_tflops", "min_xcc_balance", "min_fp8_tflops",
    "min_fp4_tflops", "min_xccs", "min_fp16_tflops", "min_int8_tops", "min_fp32_tflops", "min_fp64_tflops",
    "min_lds_read_tbps", "min_lds_cu_coverage", "min_burn_tflops", "min_burn_sustain", "max_burn_hotspot_c",
    "max_burn_thermal_violation_pct", "min_pcie_h2d_gbps", "min_pcie_d2h_gbps", "min_pcie_speed_fraction",
    "min_soak_tflops", "min_hbm_walk_coverage", "min_node_burn_balance", "max_node_power_w")}
FLOORS_OFF["require_full_pcie_width"] = False

# section -> [(case, changes to the clean section)]: one per failure line, under the default floors
BAD = {
    "hbm": [("mismatches", {"mismatches": 3, "first_bad_word": 4096, "passed": False}),
            ("read_floor", {"read_gbps": 4100.4}), ("copy_floor", {"copy_gbps": 3999.5}), ("write_floor", {"write_gbps": 100.0})],
    "hbm_walk": [("mismatches_with_address", {"mismatches": 2, "first_bad_addr": "0x7f1200004000",
                                              "first_bad_bits": "0x0000000000010000", "passed": False}),
                 ("mismatches_without_address", {"mismatches": 5, "passed": False}),
                 ("coverage", {"coverage_of_free": 0.4567, "bytes_covered": 137 << 30})],
    "mfma": [("mismatches", {"mismatches": 17, "bad_cus": 2, "bad_cu_keys": [3, 200], "passed": False}),
             ("accumulators", {"throughput_ok": False, "passed": False}), ("rate_floor", {"tflops": 1499.4}),
             ("balance_floor", {"xcc_balance": 0.8449}), ("xccs_seen", {"xccs_seen": 7})],
    "lowp": [("mismatches", {"mismatches": 10, "fp8_mismatches": 1, "fp8_scaled_mismatches": 2, "fp4_mismatches": 3,
                             "fp4_scaled_mismatches": 4, "bad_cus": 3, "bad_cu_keys": [1, 2, 3], "passed": False}),
             ("accumulators", {"throughput_ok": False, "passed": False}), ("fp8_floor", {"fp8_tflops": 2999.5}),
             ("fp4_floor", {"fp4_tflops": 12.0})],
    "classic": [(f"{path}_mismatches_{which}", {path + "_mismatches": 3, "mismatches": 3, "bad_cus": len(keys),
                                                "bad_cu_keys": keys, "passed": False})
                for path in ("fp16", "int8", "fp32", "fp64") for which, keys in (("no_keys", []), ("keys", [0x123, 0x2a5]))] +
               [("accumulators", {"throughput_ok": False, "passed": False}), ("fp16_floor", {"fp16_tflops": 1549.5}),
                ("int8_floor", {"int8_tops": 40.25}), ("fp32_floor", {"fp32_tflops": 108.4}), ("fp64_floor", {"fp64_tflops": 0.0})],
    "lds": [("mismatches_with_bits", {"mismatches": 3, "bad_cus": 2, "bad_cu_keys": [0x123, 0x2a5], "first_bad_cu_key": 0x123,
                                      "first_bad_word": 16384, "bad_bits": "0x80000001", "passed": False}),
            ("mismatches_without_bits", {"mismatches": 1, "bad_cus": 1, "passed": False}),
            ("rate_ok", {"rate_ok": False, "passed": False}), ("rate_floor", {"read_tbps": 40.25}),
            ("coverage", {"cus_seen": 255}), ("coverage_no_cus", {"cus": 0, "cus_seen": 0})],
    "burn": [("mismatches", {"mismatches": 4}), ("rate_floor_bf16", {"tflops_mean": 1799.4}),
             ("rate_floor_fp8", {"dtype": "fp8", "tflops_mean": 3599.4}), ("rate_floor_fp4", {"dtype": "fp4", "tflops_mean": 6299.4}),
             ("rate_floor_unknown_dtype", {"dtype": "fp6", "tflops_mean": 1799.4}), ("sustain", {"sustain": 0.7949}),
             ("hotspot", {"max_hotspot_c": 100.6}), ("thermal", {"thermal_violation_pct": 20.6})],
    "pcie": [("mismatches", {"mismatches": 9, "passed": False}), ("h2d_floor", {"h2d_gbps": 44.4}), ("d2h_floor", {"d2h_gbps": 27.5}),
             ("width", {"link_width": 8}), ("speed", {"link_speed_mts": 8000})],
    "soak": [("checksums", {"row_mismatches": 1, "col_mismatches": 2, "passed": False}), ("rate_floor", {"tflops_mean": 949.4})],
    "gemm": [("differs", {"bad_elements": 5, "passed": False})],
}


def verdict_cases():
    """[(name, result, floors)] in the order of the file."""
    def with_section(sect, changes):
        return {sect: dict(CLEAN[sect], **changes)}  # the whole results are in the cases at the end

    cases = [("clean_default_floors", CLEAN, {})]
    everything = copy.deepcopy(CLEAN)
    for sect in JUDGE_ORDER:
        for name, changes in BAD[sect]:
            cases.append((f"{sect}_{name}", with_section(sect, changes), {}))
            # but for the variants of a line that another case of the same section reaches
            if not any(x in name for x in ("coverage_no_cus", "no_keys", "without_", "_fp8", "_fp4", "unknown_dtype")):
                everything[sect].update(changes)
    cases.append(("top_level_error", dict(copy.deepcopy(CLEAN), error="diagnostics worker timed out"), {}))
    for sect in JUDGE_ORDER:
        cases.append((f"{sect}_error", {sect: {"error": f"{sect} diag: hipErrorLaunchFailure"}}, {}))
    everything["error"] = "scripted failure"
    cases.append(("every_failure_at_once", everything, {}))
    crashed = {sect: {"error": f"{sect}: worker died"} for sect in reversed(JUDGE_ORDER)}
    cases.append(("every_section_error_at_once", dict(crashed, error="pass failed"), {}))
    # floors off: the rates and limits of `everything` without its wrong values
    slow = copy.deepcopy(CLEAN)
    for sect in JUDGE_ORDER:
        for name, changes in BAD[sect]:
            if ("floor" in name and "rate_floor_" not in name) or name in ("coverage", "sustain", "hotspot", "thermal", "width",
                                                                            "speed", "xccs_seen", "rate_floor_bf16"):
                slow[sect].update(changes)
    cases.append(("every_floor_missed_all_floors_zero", slow, FLOORS_OFF))
    # a floor of another JSON type than its field keeps its default: every floor is missed
    cases.append(("floors_of_the_wrong_type", slow, {"min_read_gbps": "0", "min_xccs": 6.5, "require_full_pcie_width": 0,
                                                       "min_fp64_tflops": None, "min_soak_tflops": [0], "min_copy_gbps": False}))
    cases.append(("floors_raised", CLEAN, {"min_read_gbps": 1e9, "min_xcc_balance": 0.99, "min_lds_read_tbps": 200.55,
                                           "min_xccs": 9, "min_hbm_walk_coverage": 0.95, "min_burn_sustain": 0.99}))
    return cases


def record_verdicts(nat):
    out = []
    for name, result, floors in verdict_cases():
        out.append({"name": name, "result": result, "floors": floors,
                    "judged_text": nat.judge_diag(json.dumps(result), json.dumps(floors))})
    return out


# what a pass measures with a clock, or counts while it waits: different in every run
TIMING_FIELDS = {"checks_ms", "checks_started_ms", "worker_ms", "worker_ready_ms", "ready_at_ns", "late_ms", "timing_ms",
                 "samples"}


def without_timing(v):
    if isinstance(v, dict):
        return {k: without_timing(x) for k, x in v.items() if k not in TIMING_FIELDS}
    return [without_timing(x) for x in v] if isinstance(v, list) else v


def scripted_pass():
    """The start-up pass of a node agent on a mock backend with two GPUs and a scripted engine: the text
    that diag_gauges.txt holds."""
    import requests

    from bacchus_gpu_controller_amd import native
    from bacchus_gpu_controller_amd.testing.cluster import Cluster

    fx = json.loads(native().default_mi355x_fixture(2))
    fx["diag_script"] = {"checks_ms": 10}
    with Cluster(admission=False, controller=False) as c:
        c.start_node_agent(node_name="mi355x-golden", backend="mock", poll_interval_ms=200, fixture_obj=fx,
                           extra_env={"CONF_RUN_DIAG": "true", "CONF_DIAG_BURN_MS": "100"})
        url = f"http://127.0.0.1:{c.node_agent_ports['mi355x-golden']}"
        metrics = requests.get(url + "/metrics", timeout=10).text
        # the order of the keys is part of the document
        diag = json.loads(requests.get(url + "/gpus", timeout=10).text)["diag"]
    lines = [l for l in metrics.splitlines() if "amd_gpu_diag_" in l]
    lines += ["diag " + json.dumps(without_timing(g)) for g in diag]
    return "\n".join(lines) + "\n"


def main():
    sys.path.insert(0, ROOT)
    from bacchus_gpu_controller_amd import native
    from bacchus_gpu_controller_amd.utils.build import ensure_built

    ensure_built(hip=False)
    with open(os.path.join(GOLDEN, "diag_verdicts.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(case) for case in record_verdicts(native())) + "\n]\n")
    with open(os.path.join(GOLDEN, "diag_gauges.txt"), "w") as f:
        f.write(scripted_pass())


if __name__ == "__main__":
    main()
