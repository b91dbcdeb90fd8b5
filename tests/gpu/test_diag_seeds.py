"""Every diagnostic under the seeds the node agent really passes.  The agent seeds device `dev` with
0x5eed + dev, and every other GPU test passes 0x5EED, device 0's seed: on an 8-GPU node seven GPUs
run tiles, scales, HBM patterns, walk keys and soak operands that no other test generates, and a
false mismatch under one of them cordons a healthy GPU.  So for the seeds of devices 1-7, for 0 and
2^32 - 1, and for 0x5CA1E (the XOR constant of the MX scale hash, which makes the scale seed 0),
every section runs clean at its smallest honest size and the verdict passes.

The rates of runs this small say nothing, so the verdict gets every rate floor as 0; so are the two
coverage floors, which are about the size of a run (the walk here covers 256 MiB, not most of the
free memory) and not about its seed.  The floors on values stay.  torch stays on the CPU in this
process."""
import json

import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SEEDS = list(range(0x5EEE, 0x5EF5)) + [0, 0xFFFFFFFF, 0x5CA1E]
RATE_FLOORS_OFF = json.dumps({k: 0 for k in (
    "min_read_gbps", "min_copy_gbps", "min_write_gbps", "min_mfma_tflops", "min_xcc_balance", "min_fp8_tflops", "min_fp4_tflops",
    "min_fp16_tflops", "min_int8_tops", "min_fp32_tflops", "min_fp64_tflops", "min_lds_read_tbps", "min_burn_tflops",
    "min_burn_sustain", "min_pcie_h2d_gbps", "min_pcie_d2h_gbps", "min_pcie_speed_fraction", "min_soak_tflops",
    "min_lds_cu_coverage", "min_hbm_walk_coverage")})
# tests/gpu/test_diag_detection.py: (m, n, k), BGC_SOAK_TILE, the (tile, kernel) that shape runs on
SOAK_SHAPES = [((256, 256, 128), None, (256, "pingpong")), ((256, 512, 192), None, (256, "2buf")),
               ((256, 256, 128), "128", (128, "2buf"))]
WALK_BYTES, WALK_CHUNK = 256 * MIB, 64 * MIB  # test_hbm_walk_clean's


def _judge(result):
    from bacchus_gpu_controller_amd import native

    return json.loads(native().judge_diag(json.dumps(result), RATE_FLOORS_OFF))


@pytest.mark.parametrize("seed", SEEDS, ids=[f"{s:#x}" for s in SEEDS])
def test_every_section_runs_clean_under_this_seed(monkeypatch, seed):
    from bacchus_gpu_controller_amd import ops

    r = {
        "mfma": ops.mfma(waves_per_cu=1, iters=64, seed=seed),
        "lowp": ops.mfma_lowp(waves_per_cu=1, iters=64, seed=seed),
        "classic": ops.mfma_classic(waves_per_cu=1, iters=64, seed=seed),
        "lds": ops.lds(wgs_per_cu=1, rate_iters=64, seed=seed),
        "hbm": ops.hbm(nbytes=MIB + 16 * 37, iters=1, seed=seed),
        "hbm_walk": ops.hbm_walk_planted(WALK_BYTES, WALK_CHUNK, [], seed=seed),
        "pcie": ops.pcie(nbytes=MIB, iters=1, seed=seed),
        "gemm": ops.gemm_check(m=64, n=64, k=512, seed=seed),  # the agent's own shape
        "burn": ops.burn_planted(100, [], dtype="bf16", seed=seed),
    }
    soaks = []
    for (m, n, k), tile_env, kernel in SOAK_SHAPES:
        if tile_env:
            monkeypatch.setenv("BGC_SOAK_TILE", tile_env)
        soak = ops.gemm_soak(m=m, n=n, k=k, launches=2, seed=seed)
        assert (soak["tile"], soak["kernel"]) == kernel, soak
        soaks.append(soak)
    # each section's own word first, for a failure that names the section
    for name in ("mfma", "lowp", "classic"):
        assert r[name]["mismatches"] == 0 and r[name]["bad_cus"] == 0 and r[name]["throughput_ok"] is True, (name, r[name])
    assert r["lds"]["mismatches"] == 0 and r["lds"]["rate_ok"] is True, r["lds"]
    assert r["hbm"]["mismatches"] == 0 and r["hbm"]["first_bad_word"] is None, r["hbm"]
    assert r["hbm_walk"]["mismatches"] == 0 and r["hbm_walk"]["passes"] == 2 and r["hbm_walk"]["bytes_covered"] == WALK_BYTES, r["hbm_walk"]
    assert r["pcie"]["mismatches"] == 0, r["pcie"]
    assert r["gemm"]["bad_elements"] == 0, r["gemm"]
    assert r["burn"]["mismatches"] == 0 and r["burn"]["launches"] >= 2, r["burn"]
    for soak in soaks:
        assert (soak["row_mismatches"], soak["col_mismatches"]) == (0, 0), soak
    for name, section in r.items():
        if "passed" in section:
            assert section["passed"] is True, (name, section)
    # and the verdict the node agent acts on, one soak at a time
    for soak in soaks:
        judged = _judge(dict(r, soak=soak))
        assert judged["failures"] == [] and judged["passed"] is True, judged["failures"]
