"""A scripted diagnostics pass of the node agent against its recording (tests/golden/diag_gauges.txt,
written by tools/record_diag_golden.py): every amd_gpu_diag_ line of /metrics, with name, help, labels
and value, and the judged per-GPU results of /gpus with their keys in order, but for the timings."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.slow

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_scripted_pass_gives_the_recorded_gauges_and_results():
    spec = importlib.util.spec_from_file_location("record_diag_golden", os.path.join(REPO, "tools", "record_diag_golden.py"))
    recorder = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(recorder)
    with open(os.path.join(REPO, "tests", "golden", "diag_gauges.txt")) as f:
        want = f.read().splitlines()
    got = recorder.scripted_pass().splitlines()
    assert got == want
    assert len([l for l in want if l.startswith("# HELP")]) == 22 and len([l for l in want if l.startswith("diag ")]) == 2
