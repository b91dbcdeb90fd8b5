"""Exception type and full message of one refused call of every HIP-diagnostics binding, as
literals.  Each diagnostic's error is "<prefix>: <the library's last error>", and the prefix is
added on the way from the C ABI to Python, so these pin that every binding still goes through
its own prefix ("hbm diag: ", "low-precision mfma diag: ", "tiled gemm: ", ...) and that the
bindings' own size checks keep their messages.  Every call here is refused before the first HIP
call, which is why these run without a GPU.  The shapes and plants differ from the ones in
test_diag_gemm_args.py and test_diag_planted_args.py, which pin that the refusal happens."""
import json
import subprocess

import pytest

MIB = 1 << 20
SEED = 0x5EED
SOAK_SHAPE = "m, n multiples of 128 and k of 64 (each <= 32768)"
MX_SIZES = "fmt 0: A M*K, Bt N*K bytes; fmt 4: M*K/2, N*K/2; scales M*K/32 and N*K/32 bytes"


def _bf16(rows, cols):
    return b"\0" * (rows * cols * 2)


REFUSED = {
    "hbm": (lambda n: n.diag_hbm(0, 0, 1, 0), RuntimeError, "hbm diag: invalid arguments"),
    "pcie": (lambda n: n.diag_pcie(0, 0, 1, 0), RuntimeError, "pcie diag: invalid arguments"),
    "mfma": (lambda n: n.diag_mfma(0, 0, 64, 0), RuntimeError, "mfma diag: invalid arguments"),
    "mfma_lowp": (lambda n: n.diag_mfma_lowp(0, 0, 64, 0), RuntimeError, "low-precision mfma diag: invalid arguments"),
    "gemm_soak": (lambda n: n.diag_gemm_soak(0, 100, 128, 64, 1, 0), RuntimeError,
                  "gemm soak: invalid arguments: " + SOAK_SHAPE),
    "hbm_walk": (lambda n: n.diag_hbm_walk(0, 0.0, 64 << 20, 1, 0), RuntimeError,
                 "hbm walk: invalid arguments: 0 < fraction <= 0.99, chunk_bytes >= 64 MiB, budget_ms > 0"),
    "burn_dtype": (lambda n: n.diag_burn(n.gpu_backend("mock"), 0, 0, 200, SEED, "fp16"), RuntimeError,
                   "burn dtype must be bf16, fp8 or fp4, not 'fp16'"),
    "pcie_check_no_such_gpu": (lambda n: n.pcie_check(n.gpu_backend("mock"), 99, 0, MIB, SEED), IndexError, "no such GPU"),
    "gemm_length": (lambda n: n.diag_gemm(0, 16, 16, 32, b"\0" * 10, _bf16(32, 16)), ValueError,
                    "A must be M*K and B K*N bf16 values"),
    "gemm_shape": (lambda n: n.diag_gemm(0, 16, 16, 16, _bf16(16, 16), _bf16(16, 16)), RuntimeError,
                   "gemm diag: invalid arguments (M, N multiples of 16 up to 4096; K a multiple of 32 up to 8192)"),
    "gemm_tiled_length": (lambda n: n.diag_gemm_tiled(0, 128, 128, 64, _bf16(128, 64), b"\0" * 10), ValueError,
                          "A must be M*K and Bt N*K bf16 values"),
    "gemm_tiled_shape": (lambda n: n.diag_gemm_tiled(0, 128, 64, 64, _bf16(128, 64), _bf16(64, 64)), RuntimeError,
                         "tiled gemm: invalid arguments: " + SOAK_SHAPE),
    "mx_gemm_length": (lambda n: n.diag_mx_gemm(0, 0, 16, 16, 128, b"\0" * 10, b"\x7f" * 64, b"\0" * 2048, b"\x7f" * 64),
                       ValueError, MX_SIZES),
    "mx_gemm_format": (lambda n: n.diag_mx_gemm(0, 2, 16, 16, 128, b"\0" * 2048, b"\x7f" * 64, b"\0" * 2048, b"\x7f" * 64),
                       ValueError, MX_SIZES),
    "mx_gemm_shape": (lambda n: n.diag_mx_gemm(0, 4, 16, 8, 128, b"\0" * 1024, b"\x7f" * 64, b"\0" * 512, b"\x7f" * 32),
                      RuntimeError, "mx gemm: invalid arguments: fmt 0 (fp8 e4m3) or 4 (fp4 e2m1); m, n multiples of 16 "
                                    "(<= 16384), k of 128 (<= 65536)"),
    "hbm_planted": (lambda n: n.diag_hbm_planted(0, MIB, SEED, [(MIB // 4 + 5, 1)]), RuntimeError, "hbm diag: invalid arguments"),
    "pcie_planted": (lambda n: n.diag_pcie_planted(0, MIB, SEED, [(MIB // 8 + 5, 1)]), RuntimeError,
                     "pcie diag: invalid arguments"),
    "hbm_walk_planted": (lambda n: n.diag_hbm_walk_planted(0, 128 * MIB, 64 * MIB, SEED, [(0, 2, 0, 1)]), RuntimeError,
                         "hbm walk: invalid arguments: bytes >= 2 MiB, chunk_bytes >= 64 MiB, plants inside their chunk, "
                         "pass 0 or 1"),
    "mfma_planted": (lambda n: n.diag_mfma_planted(0, 1, 64, SEED, [(0, 0, 65, 0, 1.0)], []), RuntimeError,
                     "mfma diag: invalid arguments"),
    "mfma_lowp_planted": (lambda n: n.diag_mfma_lowp_planted(0, 1, 64, SEED, [], [(5, 0, 0, 0, 0, 1.0)]), RuntimeError,
                          "low-precision mfma diag: invalid arguments"),
    "mfma_delayed": (lambda n: n.diag_mfma_delayed(0, 1, 64, SEED, [(3, 10_000_001)]), RuntimeError, "mfma diag: invalid arguments"),
    "burn_delayed": (lambda n: n.diag_burn_delayed(0, 300, 32, SEED, "bf16", -3, 500), RuntimeError, "burn: invalid arguments"),
    "burn_delayed_dtype": (lambda n: n.diag_burn_delayed(0, 300, 32, SEED, "int8", 2, 500), RuntimeError,
                           "burn dtype must be bf16, fp8 or fp4, not 'int8'"),
    "burn_planted": (lambda n: n.diag_burn_planted(0, 300, 32, SEED, "fp8", [(1, 0, 0, 5, 0, 1.0)]), RuntimeError,
                     "burn: invalid arguments"),
    "burn_planted_dtype": (lambda n: n.diag_burn_planted(0, 300, 32, SEED, "fp16", [(1, 0, 0, 0, 0, 1.0)]), RuntimeError,
                           "burn dtype must be bf16, fp8 or fp4, not 'fp16'"),
    "gemm_soak_planted": (lambda n: n.diag_gemm_soak_planted(0, 256, 256, 128, 1, SEED, [(0, 300, 0, 1.0)]), RuntimeError,
                          "gemm soak: invalid arguments: " + SOAK_SHAPE + "; plants inside C, on the first or the last launch"),
    "hbm_data": (lambda n: n.diag_hbm_data(0, 129 * MIB, 1, SEED), RuntimeError, "hbm diag: invalid arguments"),
    "pcie_data": (lambda n: n.diag_pcie_data(0, 129 * MIB, SEED), RuntimeError, "pcie diag: invalid arguments"),
    "hbm_walk_data": (lambda n: n.diag_hbm_walk_data(0, 130 * MIB, 64 * MIB, 2, SEED), RuntimeError,
                      "hbm walk: invalid arguments: 2 MiB <= bytes <= 128 MiB, chunk_bytes >= 64 MiB, 1 or 2 passes, room for "
                      "every chunk"),
    "gemm_soak_data": (lambda n: n.diag_gemm_soak_data(0, 8192, 8192, 128, SEED), RuntimeError,
                       "gemm soak: invalid arguments: five destinations, and at most 128 MiB to return"),
    "gemm_soak_data_shape": (lambda n: n.diag_gemm_soak_data(0, 100, 128, 64, SEED), RuntimeError,
                             "gemm soak: invalid arguments: " + SOAK_SHAPE),
    "mfma_tile": (lambda n: n.diag_mfma_tile(0, 4, 0, SEED, 0), RuntimeError, "mfma tile: invalid arguments"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_call_raises_the_same_error(nat, name):
    call, exc, message = REFUSED[name]
    with pytest.raises(exc) as e:
        call(nat)
    assert type(e.value) is exc and str(e.value) == message


# One section that violates one floor given in judge_diag's floors JSON, and the failure it must give:
# every floor the per-GPU verdict reads, under the name it has in the floors JSON.
FLOORED = [
    ("hbm", {"read_gbps": 100.0}, {"min_read_gbps": 200}, "HBM read GB/s 100 below floor 200"),
    ("hbm", {"copy_gbps": 100.0}, {"min_copy_gbps": 200}, "HBM copy GB/s 100 below floor 200"),
    ("hbm", {"write_gbps": 100.0}, {"min_write_gbps": 200}, "HBM write GB/s 100 below floor 200"),
    ("hbm_walk", {"coverage_of_free": 0.5}, {"min_hbm_walk_coverage": 0.75}, "HBM walk covered 0.50 of free VRAM (floor 0.75)"),
    ("mfma", {"tflops": 100.0}, {"min_mfma_tflops": 200}, "MFMA bf16 TFLOP/s 100 below floor 200"),
    ("mfma", {"xcc_balance": 0.5}, {"min_xcc_balance": 0.75}, "XCC balance 0.50 below floor 0.75"),
    ("mfma", {"xccs_seen": 7}, {"min_xccs": 8}, "only 7 XCCs ran MFMA work"),
    ("lowp", {"fp8_tflops": 100.0}, {"min_fp8_tflops": 200}, "MX fp8 MFMA TFLOP/s 100 below floor 200"),
    ("lowp", {"fp4_tflops": 100.0}, {"min_fp4_tflops": 200}, "MX fp4 MFMA TFLOP/s 100 below floor 200"),
    ("burn", {"tflops_mean": 100.0}, {"min_burn_tflops": 200}, "burn-in MFMA TFLOP/s 100 below floor 200"),
    ("burn", {"dtype": "fp8", "tflops_mean": 100.0}, {"min_burn_tflops": 200}, "burn-in MFMA MX fp8 TFLOP/s 100 below floor 400"),
    ("burn", {"dtype": "fp4", "tflops_mean": 100.0}, {"min_burn_tflops": 200}, "burn-in MFMA MX fp4 TFLOP/s 100 below floor 700"),
    # a dtype the burn does not know is judged as bf16
    ("burn", {"dtype": "fp16", "tflops_mean": 100.0}, {"min_burn_tflops": 200}, "burn-in MFMA TFLOP/s 100 below floor 200"),
    ("burn", {"sustain": 0.5}, {"min_burn_sustain": 0.75}, "MFMA rate sagged to 0.50 of its start under sustained load (floor 0.75)"),
    ("burn", {"max_hotspot_c": 90.0}, {"max_burn_hotspot_c": 80}, "hotspot 90 C under sustained load (limit 80)"),
    ("burn", {"thermal_violation_pct": 30.0}, {"max_burn_thermal_violation_pct": 10}, "thermal throttling 30% of the burn (limit 10%)"),
    ("pcie", {"h2d_gbps": 10.0}, {"min_pcie_h2d_gbps": 20}, "PCIe host-to-device GB/s 10 below floor 20"),
    ("pcie", {"d2h_gbps": 10.0}, {"min_pcie_d2h_gbps": 20}, "PCIe device-to-host GB/s 10 below floor 20"),
    ("pcie", {"link_width": 8, "max_width": 16}, {"require_full_pcie_width": True}, "PCIe link x8 of x16"),
    ("pcie", {"link_speed_mts": 8000, "max_speed_mts": 32000}, {"min_pcie_speed_fraction": 0.5},
     "PCIe link at 8000 of 32000 MT/s under load"),
    ("soak", {"tflops_mean": 100.0}, {"min_soak_tflops": 200}, "GEMM soak TFLOP/s 100 below floor 200"),
    ("lowp", {"mismatches": 6, "bad_cus": 2, "fp8_mismatches": 1, "fp8_scaled_mismatches": 2, "fp4_mismatches": 3},
     {}, "MX fp8/fp4 MFMA tile mismatches on 2 CU(s): fp8 1, fp8 scaled 2, fp4 3, fp4 scaled 0"),
]
ALL_OFF = {"min_read_gbps": 0, "min_copy_gbps": 0, "min_write_gbps": 0, "min_hbm_walk_coverage": 0, "min_mfma_tflops": 0,
           "min_xcc_balance": 0, "min_xccs": 0, "min_fp8_tflops": 0, "min_fp4_tflops": 0, "min_burn_tflops": 0,
           "min_burn_sustain": 0, "max_burn_hotspot_c": 0, "max_burn_thermal_violation_pct": 0, "min_pcie_h2d_gbps": 0,
           "min_pcie_d2h_gbps": 0, "require_full_pcie_width": False, "min_pcie_speed_fraction": 0, "min_soak_tflops": 0}


FLOOR_FIELDS = list(ALL_OFF) + ["min_node_burn_balance", "max_node_power_w"]


@pytest.mark.parametrize("field", FLOOR_FIELDS)
def test_node_agent_reads_each_floor_from_its_env_key(field):
    """CONF_DIAG_<FIELD> reaches the floor: a value that cannot be one stops the agent, naming the field."""
    from bacchus_gpu_controller_amd import binary

    env = {"CONF_LISTEN_ADDR": "127.0.0.1", "CONF_LISTEN_PORT": "0", "CONF_NODE_NAME": "n", "CONF_DIAG_" + field.upper(): "x"}
    p = subprocess.run([binary("node-agent")], env=env, capture_output=True, text=True, timeout=30)
    assert p.returncode == 1 and p.stderr == f'Error: invalid value for field diag_{field}: "x"\n', (p.returncode, p.stderr)


@pytest.mark.parametrize("section,values,floor,failure", FLOORED, ids=[f"{s}-{next(iter(f), 'tiles')}-{i}" for i, (s, _, f, _) in enumerate(FLOORED)])
def test_judge_diag_reads_each_floor_and_words_its_failure(nat, section, values, floor, failure):
    off = json.loads(nat.judge_diag(json.dumps({section: values}), json.dumps(ALL_OFF)))
    expected_off = [failure] if not floor else []
    assert off["failures"] == expected_off and off["passed"] == (not expected_off)
    on = json.loads(nat.judge_diag(json.dumps({section: values}), json.dumps(dict(ALL_OFF, **floor))))
    assert on["failures"] == [failure] and on["passed"] is False
