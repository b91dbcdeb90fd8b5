"""What ties the diagnostics' one table of sections (native/gpu/diag_sections.cc) to the list of floors
(DiagFloors::fields() in native/gpu/diag.cc): every floor is read in exactly one place of the verdicts, and every section
of the table is one whose run error the verdict reports."""
import json
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _read(name):
    with open(os.path.join(REPO, "native", "gpu", name)) as f:
        return f.read()


def _functions(src, prefix):
    """name -> body of every function `prefix...(` defined at the start of a line, up to the closing brace there."""
    return {m.group(1): m.group(2) for m in re.finditer(r"^[\w:<>& ]*\b(%s\w*)\([^)]*\) \{\n(.*?)^\}" % prefix, src, re.M | re.S)}


FLOORS = re.findall(r"BGC_FLOOR\((\w+)\)[,}]", _read("diag.cc").split("DiagFloors::fields() {")[1].split("return table;")[0])
SECTIONS_CC = _read("diag_sections.cc")
TABLE = SECTIONS_CC.split("const std::vector<DiagSection>& diag_sections() {")[1].split("return table;")[0]


def test_every_floor_is_read_by_one_table_row_or_one_named_judge():
    judges = _functions(SECTIONS_CC, "judge_")
    judges.update(_functions(_read("diag_runner.cc"), "judge_node_burn"))
    assert len(FLOORS) == 26 and len(judges) >= 15
    for floor in FLOORS:
        rows = len(re.findall(r"&F::%s\b" % floor, TABLE))
        # judge_diag itself reads a row's floor through the table, never by name
        named = sorted(name for name, body in judges.items() if name != "judge_diag" and re.search(r"\bfl\.%s\b" % floor, body))
        if floor == "max_burn_hotspot_c":  # one limit for a GPU's own burn and for the node's peak
            assert rows == 0 and named == ["judge_burn", "judge_node_burn"]
        else:
            assert rows + len(named) == 1, (floor, rows, named)
    # and nothing reads a floor that the list does not have
    read = set(re.findall(r"&F::(\w+)", TABLE)) | {f for body in judges.values() for f in re.findall(r"\bfl\.(\w+)", body)}
    assert read == set(FLOORS)


def test_every_section_of_the_table_is_covered_by_the_error_sweep(nat):
    sections = re.findall(r'^      \{"(\w+)", \d+, ', TABLE, re.M)
    assert len(sections) == len(set(sections)) == 10 and {"hbm", "burn", "gemm"} <= set(sections)
    off = json.dumps({name: (False if name.startswith("require") else 0) for name in FLOORS})
    for name in sections:
        judged = json.loads(nat.judge_diag(json.dumps({name: {"error": "did not run"}}), off))
        assert judged["failures"] == [f"{name}: did not run"] and judged["passed"] is False
    # the places in the verdict are each taken once
    places = [int(p) for p in re.findall(r'^      \{"\w+", (\d+), ', TABLE, re.M)]
    assert sorted(places) == list(range(10))
