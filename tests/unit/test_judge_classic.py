"""The per-GPU verdict over a `classic` section (the fp16, int8, fp32 and fp64 matrix-core tiles and
rates): each of its failures with its exact wording, each of its four floors under its own name in
the floors JSON and in the node agent's environment, a clean section, a section that failed to run,
and the `classic` switch of the diagnostics plan on its way to a worker process.  All on hand-written
results: no GPU."""
import json
import os
import subprocess

import pytest

CLEAN = {"device": 0, "tiles_checked": 4 * 8192 * 4, "fp16_mismatches": 0, "int8_mismatches": 0, "fp32_mismatches": 0,
         "fp64_mismatches": 0, "mismatches": 0, "cus_seen": 256, "bad_cus": 0, "bad_cu_keys": [], "fp16_tflops": 2000.0,
         "int8_tops": 4000.0, "fp32_tflops": 150.0, "fp64_tflops": 75.0, "rate_ms": [2.2, 2.2, 3.6, 7.2],
         "throughput_ok": True, "elapsed_ms": 16.0, "passed": True}
OFF = {"min_fp16_tflops": 0, "min_int8_tops": 0, "min_fp32_tflops": 0, "min_fp64_tflops": 0}
RATE_KEY = {"min_fp16_tflops": "fp16_tflops", "min_int8_tops": "int8_tops", "min_fp32_tflops": "fp32_tflops",
            "min_fp64_tflops": "fp64_tflops"}
WHAT = {"min_fp16_tflops": "fp16 MFMA TFLOP/s", "min_int8_tops": "int8 MFMA TOP/s", "min_fp32_tflops": "fp32 MFMA TFLOP/s",
        "min_fp64_tflops": "fp64 MFMA TFLOP/s"}


def _judge(nat, section, floors):
    return json.loads(nat.judge_diag(json.dumps({"classic": section}), json.dumps(floors)))


def test_clean_section_passes(nat):
    at_the_rates = {"min_fp16_tflops": 2000.0, "min_int8_tops": 4000.0, "min_fp32_tflops": 150.0, "min_fp64_tflops": 75.0}
    for floors in (OFF, at_the_rates, {}):
        r = _judge(nat, CLEAN, floors)
        assert r["failures"] == [] and r["passed"] is True, (floors, r["failures"])
        assert r["classic"] == CLEAN  # the section itself is passed on unchanged


@pytest.mark.parametrize("path", ["fp16", "int8", "fp32", "fp64"])
def test_mismatches_name_the_path_the_cu_count_and_the_first_cu(nat, path):
    bad = dict(CLEAN, **{path + "_mismatches": 3}, mismatches=3, bad_cus=2, bad_cu_keys=[0x123, 0x2a5], passed=False)
    r = _judge(nat, bad, OFF)
    assert r["failures"] == [f"{path} MFMA tile mismatches: 3 elements, 2 bad CU(s), first CU key 291"]
    assert r["passed"] is False


def test_two_bad_paths_fail_separately(nat):
    bad = dict(CLEAN, fp16_mismatches=1, fp64_mismatches=64, mismatches=65, bad_cus=1, bad_cu_keys=[7], passed=False)
    assert _judge(nat, bad, OFF)["failures"] == ["fp16 MFMA tile mismatches: 1 elements, 1 bad CU(s), first CU key 7",
                                                 "fp64 MFMA tile mismatches: 64 elements, 1 bad CU(s), first CU key 7"]


def test_rate_phase_wrong_accumulators(nat):
    r = _judge(nat, dict(CLEAN, throughput_ok=False, passed=False), OFF)
    assert r["failures"] == ["fp16/int8/fp32/fp64 MFMA throughput accumulators wrong"] and r["passed"] is False


@pytest.mark.parametrize("field", list(OFF))
def test_each_floor_is_read_under_its_name_and_no_other(nat, field):
    section = dict(CLEAN, **{RATE_KEY[field]: 40.25})
    off = _judge(nat, section, OFF)
    assert off["failures"] == [] and off["passed"] is True
    on = _judge(nat, section, dict(OFF, **{field: 60.5}))
    assert on["failures"] == [f"{WHAT[field]} 40 below floor 60"] and on["passed"] is False
    # the three other floors, set just above this rate, fail for their own rates or not at all, never for this one
    others = {k: 60.5 for k in OFF if k != field}
    r = _judge(nat, section, dict(OFF, **others))
    assert all(not f.startswith(WHAT[field]) for f in r["failures"]), r["failures"]
    # and each floor sees only its own rate: with every other rate at zero it still passes at its floor
    alone = dict(CLEAN, **{RATE_KEY[k]: 0.0 for k in OFF if k != field})
    assert _judge(nat, alone, dict(OFF, **{field: CLEAN[RATE_KEY[field]]}))["failures"] == []


def test_all_failures_together(nat):
    bad = dict(CLEAN, int8_mismatches=2, mismatches=2, bad_cus=1, bad_cu_keys=[5], throughput_ok=False, fp16_tflops=10.0,
               int8_tops=20.0, fp32_tflops=3.0, fp64_tflops=2.0)
    r = _judge(nat, bad, {"min_fp16_tflops": 1000, "min_int8_tops": 2000, "min_fp32_tflops": 100, "min_fp64_tflops": 50})
    assert r["failures"] == ["int8 MFMA tile mismatches: 2 elements, 1 bad CU(s), first CU key 5",
                             "fp16/int8/fp32/fp64 MFMA throughput accumulators wrong", "fp16 MFMA TFLOP/s 10 below floor 1000",
                             "int8 MFMA TOP/s 20 below floor 2000", "fp32 MFMA TFLOP/s 3 below floor 100",
                             "fp64 MFMA TFLOP/s 2 below floor 50"]


def test_a_section_that_failed_to_run_fails_under_its_name(nat):
    r = _judge(nat, {"error": "classic mfma diag: hipErrorLaunchFailure"}, OFF)
    assert r["failures"] == ["classic: classic mfma diag: hipErrorLaunchFailure"] and r["passed"] is False


def test_default_floors_are_set(nat):
    """Every path has a default floor: a section with zero rates fails under all four names."""
    r = _judge(nat, dict(CLEAN, fp16_tflops=0.0, int8_tops=0.0, fp32_tflops=0.0, fp64_tflops=0.0), {})
    assert [f.split(" 0 below")[0] for f in r["failures"]] == list(WHAT.values())


@pytest.mark.parametrize("field", list(OFF))
def test_node_agent_reads_each_floor_from_its_env_key(field):
    from bacchus_gpu_controller_amd import binary

    env = {"CONF_LISTEN_ADDR": "127.0.0.1", "CONF_LISTEN_PORT": "0", "CONF_NODE_NAME": "n", "CONF_DIAG_" + field.upper(): "x"}
    p = subprocess.run([binary("node-agent")], env=env, capture_output=True, text=True, timeout=30)
    assert p.returncode == 1 and p.stderr == f'Error: invalid value for field diag_{field}: "x"\n', (p.returncode, p.stderr)


def test_node_agent_reads_the_classic_switch_from_its_env_key():
    from bacchus_gpu_controller_amd import binary

    env = {"CONF_LISTEN_ADDR": "127.0.0.1", "CONF_LISTEN_PORT": "0", "CONF_NODE_NAME": "n", "CONF_DIAG_CLASSIC": "x"}
    p = subprocess.run([binary("node-agent")], env=env, capture_output=True, text=True, timeout=30)
    assert p.returncode == 1 and p.stderr == 'Error: invalid value for field diag_classic: "x"\n', (p.returncode, p.stderr)


def test_plan_switch_reaches_a_worker(nat, tmp_path):
    """No binding exposes the plan's JSON, so the round trip is the one the agent makes: the plan as
    JSON in a worker's request, parsed there, and the scripted engine running what it says."""
    from bacchus_gpu_controller_amd import binary

    fx = json.loads(nat.default_mi355x_fixture(1))
    fx["diag_script"] = {"checks_ms": 0}
    path = tmp_path / "fixture.json"
    path.write_text(json.dumps(fx))
    plan = {"hbm_walk_fraction": 0.0, "pcie_bytes": 0, "soak_launches": 0}

    def checks(plan):
        req = {"op": "checks", "backend": "mock", "fixture": str(path), "gpu": fx["gpus"][0], "plan": plan, "seed": 1}
        p = subprocess.run([binary("node-agent"), "--diag-worker"], env=dict(os.environ, BGC_DIAG_REQUEST=json.dumps(req)),
                           capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        return json.loads(p.stdout.strip().splitlines()[-1])

    on, off, default = checks(dict(plan, classic=True)), checks(dict(plan, classic=False)), checks(plan)
    assert "error" not in on and "error" not in off, (on, off)
    assert "classic" in on and "classic" in default and "classic" not in off
    assert set(on) - {"classic"} == set(off)
    # what the scripted engine reports for a healthy GPU clears the default floors
    judged = json.loads(nat.judge_diag(json.dumps({"classic": on["classic"]}), "{}"))
    assert judged["failures"] == [] and on["classic"]["passed"] is True
