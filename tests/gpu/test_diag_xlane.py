"""The cross-lane diagnostic (bgc_diag_xlane): the per-SIMD check of DPP, the half-wave swaps, the LDS crossbar's
permutes and the moves between lanes and scalar registers in eight classes, refereed by the host, and the four
cross-lane rates.

* A clean run finds nothing in any class, folds waves * 64 * rounds * 47 result words, and reports the CUs and
  SIMDs it reached (printed: coverage is observed, not promised); its JSON has exactly these keys and types.
* The device equals the host referee bit for bit in all eight classes, in the first and in the last wave; the
  numpy model of tests/unit/test_xlane_reference.py, written from gpu_diag.h's text alone, is held to the same
  words.
* One flipped bit, the top bit or all bits of one result word of each class reach every counter: one mismatch in
  that class, one bad CU, one bad SIMD, that lane.  There is no consensus, so a plant on every wave is caught too.
* A plant on a rate chain clears rate_ok and nothing else; a wave made to wait 2 ms shows in its class's time.

Where a wave runs is the dispatcher's choice and differs from run to run and from launch to launch, so the truth
about a planted or delayed wave comes from the same run: xlane_data takes the plants and the delays and returns
the CU key and SIMD that the wave itself recorded.  Every plant is an XOR of a value in a register or a wait; no
kernel reads or writes out of bounds and every one runs to completion.  No assertion compares with a measured
rate."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED
SMALL = dict(waves_per_simd=1, rounds=2, rate_iters=16)
LARGE = dict(waves_per_simd=2, rounds=8, rate_iters=64)
SHAPES = [("small", SMALL), ("large", LARGE)]
NONE = type(None)
XLANE = {"device": int, "cus": int, "cus_seen": int, "simds_seen": int, "values_checked": int, "class_mismatches": int, "mismatches": int,
         "bad_cus": int, "bad_simds": int, "bad_cu_keys": int, "first_bad_cu_key": NONE, "first_bad_simd": NONE, "first_bad_lane": NONE,
         "first_bad_class": NONE, "bad_lanes": NONE, "dpp_tops": float, "swap_tops": float, "bpermute_tops": float, "swizzle_tops": float,
         "rate_ms": float, "rate_ok": bool, "slowest_cu_key": int, "cu_balance": float, "elapsed_ms": float, "passed": bool}
LISTS = {"class_mismatches": 8, "bad_cu_keys": 0, "rate_ms": 4}
RATES = ("dpp_tops", "swap_tops", "bpermute_tops", "swizzle_tops")
TIMES = RATES + ("rate_ms", "slowest_cu_key", "cu_balance", "elapsed_ms")  # what a clock decides
CLASSES = ("row", "wave", "mask", "alu", "swap", "lds", "lane", "exec")
WORDS = (12, 6, 6, 3, 4, 6, 6, 4)
BASE = (0, 12, 18, 24, 27, 31, 37, 43)
RATE_CLASSES = ("dpp", "swap", "bpermute", "swizzle")
MASKS = [0x1, 0x80000000, 0xFFFFFFFF]


@pytest.fixture(scope="module")
def ops():
    from bacchus_gpu_controller_amd import ops

    return ops


@pytest.fixture(scope="module")
def model():
    """the numpy model of the unit test, loaded from its file"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unit", "test_xlane_reference.py")
    spec = importlib.util.spec_from_file_location("xlane_numpy_model", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def clean(ops):
    """computed once, shared and left unchanged"""
    return {name: ops.xlane(seed=SEED, **args) for name, args in SHAPES}


def _untimed(r):
    return {k: v for k, v in r.items() if k not in TIMES}


def _waves(r, args):
    return r["cus"] * args["waves_per_simd"] * 4


# ---------------------------------------------------------------------------------------------
# the clean run

@pytest.mark.parametrize("name,args", SHAPES)
def test_clean_run(clean, name, args):
    r = clean[name]
    print("xlane clean", name, {k: r[k] for k in ("cus", "cus_seen", "simds_seen") + TIMES})
    assert r["class_mismatches"] == [0] * 8 and r["mismatches"] == 0 and r["bad_cus"] == 0 and r["bad_simds"] == 0 and r["bad_cu_keys"] == []
    assert r["rate_ok"] is True and r["passed"] is True
    assert r["values_checked"] == _waves(r, args) * 64 * args["rounds"] * 47
    assert 0 < r["cus_seen"] <= r["cus"] and r["cus_seen"] <= r["simds_seen"] <= 4 * r["cus_seen"]
    assert all(r[k] > 0 for k in RATES) and all(ms > 0 for ms in r["rate_ms"])
    assert 0 < r["cu_balance"] <= 1 and r["slowest_cu_key"] >= 0
    assert r["elapsed_ms"] >= sum(r["rate_ms"])


def test_result_shape(clean):
    r = clean["large"]
    assert list(r) == list(XLANE)
    wrong = {k: type(r[k]).__name__ for k in XLANE if k not in LISTS and type(r[k]) is not XLANE[k]}
    assert not wrong, wrong
    for k, n in LISTS.items():
        assert type(r[k]) is list and len(r[k]) == n and all(type(v) is XLANE[k] for v in r[k]), k


@pytest.mark.parametrize("name,args", SHAPES)
def test_planted_and_delayed_variants_without_plants_are_the_same_run(ops, clean, name, args):
    for r in (ops.xlane_planted([], [], seed=SEED, **args), ops.xlane_delayed([], seed=SEED, **args)):
        assert list(r) == list(XLANE)
        assert _untimed(r) == _untimed(clean[name])


# ---------------------------------------------------------------------------------------------
# the device against the referee and against the numpy model

@pytest.fixture(scope="module")
def expected(ops):
    return {name: ops.xlane_expected(args["rounds"], seed=SEED) for name, args in SHAPES}


@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("name,args", SHAPES)
def test_device_equals_the_referee_and_the_numpy_model(ops, clean, expected, model, name, args, which):
    index = 0 if which == "first" else _waves(clean[name], args) - 1
    r, wave = ops.xlane_data(index, seed=SEED, **args)
    exp = expected[name]
    print("xlane wave", name, which, "ran on CU key", wave["cu_key"], "SIMD", wave["simd"])
    assert _untimed(r) == _untimed(clean[name])
    assert 0 <= wave["cu_key"] < 2048 and 0 <= wave["simd"] < 4 and all(0 <= key < 2048 for key in wave["rate_cu_key"])
    assert wave["raw"].shape == exp["raw"].shape == (args["rounds"], 47, 64)
    for c in range(8):
        got, want = wave["raw"][:, BASE[c]:BASE[c] + WORDS[c]], exp["raw"][:, BASE[c]:BASE[c] + WORDS[c]]
        assert np.array_equal(got, want), (CLASSES[c], np.argwhere(got != want)[:4])
    assert np.array_equal(wave["digests"], exp["digests"])
    numpy_words = np.array([model.model_round(SEED, rnd) for rnd in range(args["rounds"])])
    assert np.array_equal(wave["raw"], numpy_words), np.argwhere(wave["raw"] != numpy_words)[:4]
    assert np.array_equal(wave["digests"], model.model_digests(wave["raw"]))  # every digest is the fold of the words returned


# ---------------------------------------------------------------------------------------------
# plants reach the counters

# one word of each class: (round, destination lane, word), at the ends of the rounds, the lanes and the words
PLANTS = {"row": (0, 0, 0), "wave": (1, 63, 5), "mask": (0, 16, 2), "alu": (1, 63, 2), "swap": (0, 32, 3), "lds": (1, 31, 1),
          "lane": (0, 5, 2), "exec": (1, 47, 3)}


@pytest.mark.parametrize("mask", MASKS, ids=[f"{m:#x}" for m in MASKS])
@pytest.mark.parametrize("where", ["first_wave", "last_wave"])
@pytest.mark.parametrize("cls", range(8), ids=CLASSES)
def test_one_planted_word_is_detected_and_names_its_wave(ops, clean, expected, cls, where, mask):
    c = clean["small"]
    wave = 0 if where == "first_wave" else _waves(c, SMALL) - 1
    rnd, lane, word = PLANTS[CLASSES[cls]]
    r, planted = ops.xlane_data(wave, check_plants=[(wave, CLASSES[cls], rnd, lane, word, mask)], seed=SEED, **SMALL)
    assert r["class_mismatches"] == [int(k == cls) for k in range(8)] and r["mismatches"] == 1
    # the wave's own record of where it ran, in this run
    assert 0 <= planted["cu_key"] < 2048 and planted["simd"] in range(4)
    assert r["first_bad_cu_key"] == planted["cu_key"] and r["first_bad_simd"] == planted["simd"]
    assert r["bad_cus"] == 1 and r["bad_simds"] == 1 and r["bad_cu_keys"] == [planted["cu_key"]]
    assert r["first_bad_lane"] == lane and r["first_bad_class"] == CLASSES[cls] and r["bad_lanes"] == f"0x{1 << lane:016x}"
    want = expected["small"]["raw"].copy()  # the word it folded is the referee's with the mask in it, and nothing else moved
    want[rnd, BASE[cls] + word, lane] ^= np.uint32(mask)
    assert np.array_equal(planted["raw"], want)
    assert r["values_checked"] == c["values_checked"] and r["cus_seen"] == c["cus_seen"] and r["simds_seen"] == c["simds_seen"]
    assert r["rate_ok"] is True  # a check plant never touches the rate phase
    assert r["passed"] is False


PLACE = ("first_bad_cu_key", "first_bad_simd", "bad_cu_keys")  # what the dispatcher decides anew in every run


def test_the_planted_entry_and_the_data_entry_count_a_plant_alike(ops, clean):
    wave = _waves(clean["small"], SMALL) - 1
    plant = [(wave, "swap", 1, 63, 3, 0x8000)]
    p = ops.xlane_planted(plant, [], seed=SEED, **SMALL)
    d, data = ops.xlane_data(wave, check_plants=plant, seed=SEED, **SMALL)
    print("xlane plant on wave", wave, "named CU key", p["first_bad_cu_key"], "SIMD", p["first_bad_simd"], "; in the data run",
          d["first_bad_cu_key"], d["first_bad_simd"])
    assert p["mismatches"] == 1 and p["bad_cu_keys"] == [p["first_bad_cu_key"]] and p["first_bad_simd"] in range(4)
    assert {k: v for k, v in _untimed(p).items() if k not in PLACE} == {k: v for k, v in _untimed(d).items() if k not in PLACE}


def test_two_plants_on_one_word_whose_masks_cancel(ops, clean):
    r = ops.xlane_planted([(7, "lds", 1, 5, 3, 0xDEADBEEF), (7, "lds", 1, 5, 3, 0xDEADBEEF)], [], seed=SEED, **SMALL)
    assert _untimed(r) == _untimed(clean["small"])


@pytest.mark.parametrize("cls", range(8), ids=CLASSES)
def test_a_plant_on_every_wave_is_caught(ops, clean, cls):
    """the host recomputes every digest: there is no consensus that a common fault could move"""
    c = clean["small"]
    r = ops.xlane_planted([(ops.ALL_WAVES, CLASSES[cls], 1, 40, WORDS[cls] - 1, 0x100)], [], seed=SEED, **SMALL)
    assert r["class_mismatches"] == [_waves(c, SMALL) * int(k == cls) for k in range(8)]
    assert r["bad_cus"] == r["cus_seen"] == c["cus_seen"] and r["bad_simds"] == r["simds_seen"] == c["simds_seen"]
    assert len(r["bad_cu_keys"]) == min(64, r["bad_cus"]) and r["bad_cu_keys"] == sorted(set(r["bad_cu_keys"]))
    assert r["first_bad_cu_key"] == r["bad_cu_keys"][0] and r["first_bad_lane"] == 40 and r["bad_lanes"] == f"0x{1 << 40:016x}"
    assert r["rate_ok"] is True and r["passed"] is False


def test_a_plant_beyond_the_launch_is_refused(ops, clean):
    waves = _waves(clean["small"], SMALL)
    beyond = "xlane diag: invalid arguments: plant in a wave beyond the launch"
    with pytest.raises(RuntimeError, match=beyond):
        ops.xlane_planted([(waves, "row", 0, 0, 0, 1)], [], seed=SEED, **SMALL)
    with pytest.raises(RuntimeError, match=beyond):
        ops.xlane_planted([], [(0, "dpp", 0, 0, 1), (waves + 3, "dpp", 0, 0, 1)], seed=SEED, **SMALL)
    with pytest.raises(RuntimeError, match=beyond):
        ops.xlane_delayed([(waves, "swizzle", 1)], seed=SEED, **SMALL)
    with pytest.raises(RuntimeError, match=beyond):
        ops.xlane_data(waves, seed=SEED, **SMALL)


# ---------------------------------------------------------------------------------------------
# the rate phase

@pytest.mark.parametrize("name,args", SHAPES)
@pytest.mark.parametrize("cls", RATE_CLASSES)
def test_a_rate_plant_clears_rate_ok_and_nothing_else(ops, clean, cls, name, args):
    c = clean[name]
    for wave, lane, chain, mask in ((0, 0, 0, 0x1), (_waves(c, args) - 1, 63, 7, 0x80000000)):
        r = ops.xlane_planted([], [(wave, cls, lane, chain, mask)], seed=SEED, **args)
        assert r["rate_ok"] is False and r["passed"] is False
        assert _untimed(dict(r, rate_ok=True, passed=True)) == _untimed(c)


@pytest.mark.parametrize("iters", [1, 2, 3, 5, 17, 4096])
def test_rate_end_values_match_the_closed_form_at_other_iteration_counts(ops, iters):
    """odd and even counts, counts below and above the four steps of a loop trip, and many trips"""
    r = ops.xlane(waves_per_simd=1, rounds=1, rate_iters=iters, seed=SEED)
    assert r["rate_ok"] is True and r["passed"] is True


T = 200_000  # ticks of the 100 MHz constant clock: 2 ms


@pytest.mark.parametrize("where", ["first_wave", "last_wave"])
@pytest.mark.parametrize("cls", range(4), ids=RATE_CLASSES)
def test_a_delayed_wave_shows_in_its_class_and_names_its_cu(ops, clean, cls, where):
    c = clean["small"]
    wave = 0 if where == "first_wave" else _waves(c, SMALL) - 1
    r, delayed = ops.xlane_data(wave, delays=[(wave, RATE_CLASSES[cls], T)], seed=SEED, **SMALL)
    print("xlane delayed", RATE_CLASSES[cls], where, {k: r[k] for k in TIMES}, "ran on", delayed["rate_cu_key"], "clean", {k: c[k] for k in TIMES})
    assert r["rate_ms"][cls] >= 2.0  # the launch cannot end before its wave's 2 ms
    assert r[RATES[cls]] <= c["cus"] * 4 * 64 * 8 * SMALL["rate_iters"] / 2e-3 / 1e12
    # the CU that the wave recorded in that class's timed launch of this run has waited 2 ms more than any other
    assert all(0 <= key < 2048 for key in delayed["rate_cu_key"])
    assert r["slowest_cu_key"] == delayed["rate_cu_key"][cls]
    assert r["cu_balance"] < min(c["cu_balance"], 0.5)
    assert _untimed(r) == _untimed(c)  # nothing else moves: no value is touched


def test_the_delayed_entry_shows_the_delay_alike(ops, clean):
    r = ops.xlane_delayed([(3, "bpermute", T)], seed=SEED, **SMALL)
    assert r["rate_ms"][2] >= 2.0 and 0 <= r["slowest_cu_key"] < 2048 and r["cu_balance"] < 0.5
    assert _untimed(r) == _untimed(clean["small"])
