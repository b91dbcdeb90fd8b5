"""The per-GPU verdict over an `lds` section (the per-CU LDS march and the LDS read rate): each of
its four failures with its exact wording, each of its two floors under its own name in the floors
JSON and in the node agent's environment, a clean section, a section that failed to run, and the
`lds` switch of the diagnostics plan on its way to a worker process.  All on hand-written results:
no GPU."""
import json
import os
import subprocess

import pytest

CLEAN = {"device": 0, "cus": 256, "cus_seen": 256, "bad_cus": 0, "bad_cu_keys": [], "words_checked": 2 * 40960 * 4 * 256,
         "mismatches": 0, "first_bad_cu_key": None, "first_bad_word": None, "bad_bits": None, "read_tbps": 90.0,
         "rate_ok": True, "slowest_cu_key": 17, "cu_balance": 0.97, "elapsed_ms": 3.5, "passed": True}
OFF = {"min_lds_read_tbps": 0, "min_lds_cu_coverage": 0}


def _judge(nat, section, floors):
    return json.loads(nat.judge_diag(json.dumps({"lds": section}), json.dumps(floors)))


def test_clean_section_passes(nat):
    for floors in (OFF, {"min_lds_read_tbps": 89.9, "min_lds_cu_coverage": 1.0}, {}):
        r = _judge(nat, CLEAN, floors)
        assert r["failures"] == [] and r["passed"] is True, (floors, r["failures"])
        assert r["lds"] == CLEAN  # the section itself is passed on unchanged


def test_march_mismatches_name_the_cu_the_word_and_the_bits(nat):
    bad = dict(CLEAN, mismatches=3, bad_cus=2, bad_cu_keys=[0x123, 0x2a5], first_bad_cu_key=0x123, first_bad_word=16384,
               bad_bits="0x80000001", passed=False)
    r = _judge(nat, bad, OFF)
    assert r["failures"] == ["LDS march mismatches on 2 CU(s): 3 words (first on CU key 291 at word 16384, bits 0x80000001)"]
    assert r["passed"] is False


def test_rate_phase_wrong_data(nat):
    r = _judge(nat, dict(CLEAN, rate_ok=False, passed=False), OFF)
    assert r["failures"] == ["LDS rate phase read wrong data"] and r["passed"] is False


@pytest.mark.parametrize("section,floor,failure", [
    ({"read_tbps": 40.25}, {"min_lds_read_tbps": 60.5}, "LDS read TB/s 40.2 below floor 60.5"),
    ({"cus": 256, "cus_seen": 255}, {"min_lds_cu_coverage": 1.0}, "LDS march reached 255 of 256 CUs"),
    ({"cus": 256, "cus_seen": 100}, {"min_lds_cu_coverage": 0.5}, "LDS march reached 100 of 256 CUs"),
], ids=["read_tbps", "cu_coverage_all", "cu_coverage_half"])
def test_each_floor_is_read_under_its_name(nat, section, floor, failure):
    off = _judge(nat, section, OFF)
    assert off["failures"] == [] and off["passed"] is True
    on = _judge(nat, section, dict(OFF, **floor))
    assert on["failures"] == [failure] and on["passed"] is False
    # the other floor does not make this failure
    other = {k: (1000.0 if k == "min_lds_read_tbps" else 1.0) for k in OFF if k not in floor}
    assert failure not in _judge(nat, dict(CLEAN, **section), dict(OFF, **other))["failures"]


def test_coverage_at_the_floor_passes(nat):
    assert _judge(nat, dict(CLEAN, cus_seen=128), dict(OFF, min_lds_cu_coverage=0.5))["failures"] == []


def test_all_four_failures_together(nat):
    bad = dict(CLEAN, mismatches=1, bad_cus=1, first_bad_cu_key=5, first_bad_word=0, bad_bits="0x00000001", rate_ok=False,
               read_tbps=10.0, cus_seen=200)
    r = _judge(nat, bad, {"min_lds_read_tbps": 50, "min_lds_cu_coverage": 1.0})
    assert r["failures"] == ["LDS march mismatches on 1 CU(s): 1 words (first on CU key 5 at word 0, bits 0x00000001)",
                             "LDS rate phase read wrong data", "LDS read TB/s 10.0 below floor 50.0",
                             "LDS march reached 200 of 256 CUs"]


def test_a_section_that_failed_to_run_fails_under_its_name(nat):
    r = _judge(nat, {"error": "lds diag: hipErrorLaunchFailure"}, OFF)
    assert r["failures"] == ["lds: lds diag: hipErrorLaunchFailure"] and r["passed"] is False


@pytest.mark.parametrize("field", list(OFF))
def test_node_agent_reads_each_floor_from_its_env_key(field):
    from bacchus_gpu_controller_amd import binary

    env = {"CONF_LISTEN_ADDR": "127.0.0.1", "CONF_LISTEN_PORT": "0", "CONF_NODE_NAME": "n", "CONF_DIAG_" + field.upper(): "x"}
    p = subprocess.run([binary("node-agent")], env=env, capture_output=True, text=True, timeout=30)
    assert p.returncode == 1 and p.stderr == f'Error: invalid value for field diag_{field}: "x"\n', (p.returncode, p.stderr)


def test_node_agent_reads_the_lds_switch_from_its_env_key():
    from bacchus_gpu_controller_amd import binary

    env = {"CONF_LISTEN_ADDR": "127.0.0.1", "CONF_LISTEN_PORT": "0", "CONF_NODE_NAME": "n", "CONF_DIAG_LDS": "x"}
    p = subprocess.run([binary("node-agent")], env=env, capture_output=True, text=True, timeout=30)
    assert p.returncode == 1 and p.stderr == 'Error: invalid value for field diag_lds: "x"\n', (p.returncode, p.stderr)


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

    on, off, default = checks(dict(plan, lds=True)), checks(dict(plan, lds=False)), checks(plan)
    assert "error" not in on and "error" not in off, (on, off)
    assert "lds" in on and "lds" in default and "lds" not in off
    assert set(on) - {"lds"} == set(off)
    # what the scripted engine reports for a healthy GPU clears the default floors
    judged = json.loads(nat.judge_diag(json.dumps({"lds": on["lds"]}), "{}"))
    assert judged["failures"] == [] and on["lds"]["passed"] is True
