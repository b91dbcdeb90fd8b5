"""judge_diag against its recorded verdicts (tests/golden/diag_verdicts.json, written by
tools/record_diag_golden.py): one case per line of the verdict that can add a failure, each section's
run error, a clean result, every failure at once, every floor at 0 and floors of the wrong JSON type.
The whole text is compared: the failures' wording and order, and the order of the result's keys."""
import json
import os

import pytest

with open(os.path.join(os.path.dirname(__file__), "..", "golden", "diag_verdicts.json")) as f:
    CASES = json.load(f)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_judge_diag_gives_the_recorded_text(nat, case):
    assert nat.judge_diag(json.dumps(case["result"]), json.dumps(case["floors"])) == case["judged_text"]


def test_the_cases_reach_every_failure_line():
    """The fixture still holds what it was recorded for: the sections' failures are each reached alone, and
    the case with all of them has them in the verdict's order."""
    alone = {c["name"]: json.loads(c["judged_text"])["failures"] for c in CASES}
    single = [n for n, f in alone.items() if len(f) == 1]
    assert len(single) >= 50, single
    everything = alone["every_failure_at_once"]
    assert len(everything) == 42 and everything[0].startswith("HBM pattern") and everything[-1] == "scripted failure"
    assert alone["clean_default_floors"] == [] and alone["every_floor_missed_all_floors_zero"] == []
