"""The JSON of every diagnostic: its exact key set and the JSON type of every value, for one clean
run at the smallest valid size.  The node agent's verdict, its gauges and the tests read these keys
by name, and a result struct reaches JSON through one conversion per struct, shared by a
diagnostic and its planted variant, so a key that is lost, renamed or changes type there shows
here.  Values that vary from run to run are not compared."""
import json

import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
NONE = type(None)

HBM = {"device": int, "bytes": int, "iters": int, "write_gbps": float, "read_gbps": float, "copy_gbps": float,
       "mismatches": int, "first_bad_word": NONE, "elapsed_ms": float, "passed": bool}
PCIE = {"device": int, "bytes": int, "iters": int, "h2d_gbps": float, "d2h_gbps": float, "bidir_gbps": float,
        "mismatches": int, "elapsed_ms": float, "passed": bool}
MFMA = {"device": int, "tiles_checked": int, "mismatches": int, "cus_seen": int, "xccs_seen": int, "bad_cus": int,
        "bad_cu_keys": [], "tflops": float, "throughput_ok": bool, "xcc_waves": [int] * 8, "xcc_wave_us": [float] * 8,
        "xcc_balance": float, "elapsed_ms": float, "passed": bool}
LOWP = {"device": int, "tiles_checked": int, "fp8_mismatches": int, "fp8_scaled_mismatches": int, "fp4_mismatches": int,
        "fp4_scaled_mismatches": int, "mismatches": int, "cus_seen": int, "bad_cus": int, "bad_cu_keys": [],
        "fp8_tflops": float, "fp4_tflops": float, "throughput_ok": bool, "elapsed_ms": float, "passed": bool}
SOAK = {"device": int, "m": int, "n": int, "k": int, "launches": int, "tile": int, "kernel": str, "elapsed_ms": float,
        "tflops_mean": float, "tflops_best": float, "row_mismatches": int, "col_mismatches": int, "passed": bool}
GEMM_CHECK = {"m": int, "n": int, "k": int, "max_abs_err": float, "max_err_over_bound": float, "bad_elements": int,
              "passed": bool}
WALK = {"device": int, "free_bytes": int, "total_bytes": int, "target_bytes": int, "bytes_covered": int,
        "coverage_of_free": float, "chunks": int, "passes": int, "mismatches": int, "first_bad_addr": NONE,
        "first_bad_bits": NONE, "write_gbps": float, "read_gbps": float, "alloc_ms": float, "elapsed_ms": float,
        "budget_hit": bool, "passed": bool}
WALK_PLANTED = dict(WALK, chunk_list=[[int, int]] * 2)  # 128 MiB in chunks of 64 MiB
# Diag::burn, then what the engine and the telemetry sampler add (diag_runner.cc); the two throttle
# residencies are null when the backend's samples carry no accumulators
BURN = {"dtype": str, "launches": int, "elapsed_ms": float, "tflops_mean": float, "tflops_min": float,
        "tflops_first": float, "tflops_last": float, "tflops_max": float, "sustain": float, "mismatches": int,
        "ready_at_ns": int, "late_ms": float, "samples": int, "max_hotspot_c": float, "max_mem_c": float,
        "power_mean_w": float, "power_max_w": float, "gfxclk_mean_mhz": float, "gfxclk_min_mhz": float,
        "thermal_violation_pct": (float, NONE), "ppt_violation_pct": (float, NONE)}


def _burn(ops):
    from bacchus_gpu_controller_amd import native

    n = native()
    return json.loads(n.diag_burn(n.gpu_backend("mock"), 0, 0, 200))


CALLS = {
    "hbm": (lambda ops: ops.hbm(nbytes=MIB, iters=1), HBM),
    "pcie": (lambda ops: ops.pcie(nbytes=MIB, iters=1), PCIE),
    "mfma": (lambda ops: ops.mfma(waves_per_cu=1, iters=64), MFMA),
    "mfma_lowp": (lambda ops: ops.mfma_lowp(waves_per_cu=1, iters=64), LOWP),
    "gemm_soak": (lambda ops: ops.gemm_soak(m=256, n=256, k=128, launches=1), SOAK),
    "gemm_check": (lambda ops: ops.gemm_check(m=16, n=16, k=32), GEMM_CHECK),
    "hbm_walk": (lambda ops: ops.hbm_walk(fraction=0.001, chunk_bytes=64 * MIB), WALK),
    "burn": (_burn, BURN),
    "hbm_planted": (lambda ops: ops.hbm_planted(MIB, []), HBM),
    "pcie_planted": (lambda ops: ops.pcie_planted(MIB, []), PCIE),
    "mfma_planted": (lambda ops: ops.mfma_planted([], []), MFMA),
    "mfma_lowp_planted": (lambda ops: ops.mfma_lowp_planted([], []), LOWP),
    "gemm_soak_planted": (lambda ops: ops.gemm_soak_planted(256, 256, 128, 1, []), SOAK),
    "hbm_walk_planted": (lambda ops: ops.hbm_walk_planted(128 * MIB, 64 * MIB, []), WALK_PLANTED),
    "mfma_delayed": (lambda ops: ops.mfma_delayed([]), MFMA),
    # the burn's own keys, without the engine's and the sampler's
    "burn_delayed": (lambda ops: ops.burn_delayed(200, 1 << 30, 1000), {k: BURN[k] for k in list(BURN)[:10]}),
    "burn_planted": (lambda ops: ops.burn_planted(200, []), {k: BURN[k] for k in list(BURN)[:10]}),
}


def _matches(value, shape):
    """A type, a tuple of allowed types, or a list with one shape per element.  bool is not an int here."""
    if isinstance(shape, list):
        return type(value) is list and len(value) == len(shape) and all(_matches(v, s) for v, s in zip(value, shape))
    return type(value) in (shape if isinstance(shape, tuple) else (shape,))


@pytest.mark.parametrize("name", list(CALLS))
def test_result_keys_and_types(name):
    from bacchus_gpu_controller_amd import ops

    call, shape = CALLS[name]
    r = call(ops)
    assert list(r) == list(shape), r  # the keys, in the order the conversion writes them
    wrong = {k: v for k, v in r.items() if not _matches(v, shape[k])}
    assert not wrong, (wrong, r)
    if "passed" in shape:
        assert r["passed"] is True, r
