"""The vector-ALU diagnostic (bgc_diag_valu): the per-SIMD check of seven instruction classes, refereed by the
host, and the five vector rates.

* A clean run finds nothing in any class, folds waves * 64 * rounds * 40 result words, and reports the CUs and
  SIMDs it reached (printed: coverage is observed, not promised); its JSON has exactly these keys and types.
* The device equals the host referee bit for bit in the six exact classes, in the first and in the last wave;
  the referee is checked on its own against an independent reference in tests/unit/test_valu_reference.py.
* The raw transcendental results lie within the recorded bounds (gpu_diag.h, BGC_VALU_*_ULPS) of numpy float64.
* One flipped bit, the top bit or all bits of one result word reach every counter: one mismatch in that class,
  one bad CU, one bad SIMD, that lane.  A plant on every wave is caught in an exact class; in the transcendental
  class it moves the consensus, which is the documented limit of consensus, and the accuracy bound catches it.
* A plant on a rate chain clears rate_ok and nothing else; a wave made to wait 2 ms shows in its class's time.

Where a wave runs is the dispatcher's choice and differs from run to run and from launch to launch, so the
truth about a planted or delayed wave comes from the same run: valu_data takes the plants and the delays and
returns the CU key and SIMD that the wave itself recorded in the check launch and the CU key it recorded in each
timed rate launch.  The place that the result names must equal it.  Every plant is an XOR of a value in a
register; no kernel reads or writes out of bounds and every one runs to completion.  No assertion compares with
a measured rate."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED
SMALL = dict(waves_per_simd=1, rounds=2, rate_iters=16)
LARGE = dict(waves_per_simd=2, rounds=8, rate_iters=64)
NONE = type(None)
VALU = {"device": int, "cus": int, "cus_seen": int, "simds_seen": int, "values_checked": int, "class_mismatches": int, "mismatches": int,
        "consensus_ok": bool, "trans_out_of_bound": int, "bad_cus": int, "bad_simds": int, "bad_cu_keys": int, "first_bad_cu_key": NONE,
        "first_bad_simd": NONE, "first_bad_lane": NONE, "first_bad_class": NONE, "bad_lanes": NONE, "fp32_tflops": float,
        "fp16_tflops": float, "fp64_tflops": float, "int32_tops": float, "trans_tips": float, "rate_ms": float, "rate_ok": bool,
        "slowest_cu_key": int, "cu_balance": float, "elapsed_ms": float, "passed": bool}
LISTS = {"class_mismatches": 7, "bad_cu_keys": 0, "rate_ms": 5}
RATES = ("fp32_tflops", "fp16_tflops", "fp64_tflops", "int32_tops", "trans_tips")
TIMES = RATES + ("rate_ms", "slowest_cu_key", "cu_balance", "elapsed_ms")  # what a clock decides
CLASSES = ("int32", "fp32", "fp16", "fp64", "cvt", "dot", "trans")
WORDS = (13, 6, 3, 6, 5, 2, 5)
BASE = (0, 13, 19, 22, 28, 33, 35)
RATE_CLASSES = ("fp32", "fp16", "fp64", "int32", "trans")
MASKS = [0x1, 0x80000000, 0xFFFFFFFF]


@pytest.fixture(scope="module")
def ops():
    from bacchus_gpu_controller_amd import ops

    return ops


@pytest.fixture(scope="module")
def clean(ops):
    """computed once, shared and left unchanged"""
    return {name: ops.valu(seed=SEED, **args) for name, args in (("small", SMALL), ("large", LARGE))}


def _untimed(r):
    return {k: v for k, v in r.items() if k not in TIMES}


def _waves(r, args):
    return r["cus"] * args["waves_per_simd"] * 4


# ---------------------------------------------------------------------------------------------
# the clean run

@pytest.mark.parametrize("name,args", [("small", SMALL), ("large", LARGE)])
def test_clean_run(clean, name, args):
    r = clean[name]
    print("valu clean", name, {k: r[k] for k in ("cus", "cus_seen", "simds_seen") + TIMES})
    assert r["class_mismatches"] == [0] * 7 and r["mismatches"] == 0 and r["bad_cus"] == 0 and r["bad_simds"] == 0 and r["bad_cu_keys"] == []
    assert r["consensus_ok"] is True and r["trans_out_of_bound"] == 0 and r["rate_ok"] is True and r["passed"] is True
    assert r["values_checked"] == _waves(r, args) * 64 * args["rounds"] * 40
    assert 0 < r["cus_seen"] <= r["cus"] and r["cus_seen"] <= r["simds_seen"] <= 4 * r["cus_seen"]
    assert all(r[k] > 0 for k in RATES) and all(ms > 0 for ms in r["rate_ms"])
    assert 0 < r["cu_balance"] <= 1 and r["slowest_cu_key"] >= 0
    assert r["elapsed_ms"] >= sum(r["rate_ms"])


def test_result_shape(clean):
    r = clean["large"]
    assert list(r) == list(VALU)
    wrong = {k: type(r[k]).__name__ for k in VALU if k not in LISTS and type(r[k]) is not VALU[k]}
    assert not wrong, wrong
    for k, n in LISTS.items():
        assert type(r[k]) is list and len(r[k]) == n and all(type(v) is VALU[k] for v in r[k]), k


@pytest.mark.parametrize("name,args", [("small", SMALL), ("large", LARGE)])
def test_planted_and_delayed_variants_without_plants_are_the_same_run(ops, clean, name, args):
    for r in (ops.valu_planted([], [], seed=SEED, **args), ops.valu_delayed([], seed=SEED, **args)):
        assert list(r) == list(VALU)
        assert _untimed(r) == _untimed(clean[name])


# ---------------------------------------------------------------------------------------------
# the device against the referee

@pytest.fixture(scope="module")
def waves(ops, clean):
    """(result, wave) of the first and the last wave of the large run, and the referee's expectation"""
    last = _waves(clean["large"], LARGE) - 1
    return {"first": ops.valu_data(0, seed=SEED, **LARGE), "last": ops.valu_data(last, seed=SEED, **LARGE),
            "expected": ops.valu_expected(LARGE["rounds"], seed=SEED)}


def _mix32(x):
    x = np.array(x, dtype=np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


@pytest.mark.parametrize("which", ["first", "last"])
def test_device_equals_the_referee_in_the_exact_classes(clean, waves, which):
    r, wave = waves[which]
    exp = waves["expected"]
    print("valu wave", which, "ran on CU key", wave["cu_key"], "SIMD", wave["simd"])
    assert _untimed(r) == _untimed(clean["large"])
    assert 0 <= wave["cu_key"] < 2048 and 0 <= wave["simd"] < 4
    assert wave["raw"].shape == exp["raw"].shape == (LARGE["rounds"], 40, 64)
    for c in range(6):
        got, want = wave["raw"][:, BASE[c]:BASE[c] + WORDS[c]], exp["raw"][:, BASE[c]:BASE[c] + WORDS[c]]
        assert np.array_equal(got, want), (CLASSES[c], np.argwhere(got != want)[:4])
        assert np.array_equal(wave["digests"][c], exp["digests"][c]), CLASSES[c]
    # every digest, the transcendentals' included, is the fold of the words the wave returned
    for c in range(7):
        d = np.full(64, 0x9E3779B9 + c, dtype=np.uint32)
        for rnd in range(LARGE["rounds"]):
            for word in range(WORDS[c]):
                d = _mix32(d ^ wave["raw"][rnd, BASE[c] + word])
        assert np.array_equal(wave["digests"][c], d), CLASSES[c]
    assert np.array_equal(waves["first"][1]["digests"], waves["last"][1]["digests"])  # the consensus, seen from both ends


def _trans_operands(seed, r):
    """gpu_diag.h, "Vector ALU": the operands of the five transcendental words of round r"""
    def f32(h, emin=-8, mask=15):
        return (h & np.uint32(0x807FFFFF)) | ((np.uint32(127 + emin) + ((h >> np.uint32(23)) & np.uint32(mask))) << np.uint32(23))

    w = [_mix32(np.uint32(seed) ^ _mix32(np.uint32(6 << 24 | r << 16 | k << 8) | np.arange(64, dtype=np.uint32))) for k in range(5)]
    t = ((w[1] >> np.uint32(23)) & np.uint32(7)).astype(np.int64)
    log_in = (w[1] & np.uint32(0x007FFFFF)) | ((127 + np.where(t < 4, t - 5, t - 3)).astype(np.uint32) << np.uint32(23))
    pos = np.uint32(0x7FFFFFFF)
    return [v.view(np.float32).astype(np.float64) for v in (f32(w[0], -2, 7), log_in, f32(w[2]), f32(w[3]) & pos, f32(w[4]) & pos)]


@pytest.mark.parametrize("which", ["first", "last"])
def test_transcendentals_are_within_the_recorded_bound_of_float64(ops, waves, which):
    _, wave = waves[which]
    bounds = ops.valu_trans_ulps()
    worst = [0.0] * 5
    for rnd in range(LARGE["rounds"]):
        x = _trans_operands(SEED, rnd)
        for op, want in enumerate((np.exp2(x[0]), np.log2(x[1]), 1.0 / x[2], 1.0 / np.sqrt(x[3]), np.sqrt(x[4]))):
            got = wave["raw"][rnd, BASE[6] + op].view(np.float32).astype(np.float64)
            worst[op] = max(worst[op], float((np.abs(got - want) / np.exp2(np.floor(np.log2(np.abs(want))) - 23)).max()))
    print("valu trans ulps", which, [round(u, 4) for u in worst], "bounds", bounds)
    assert all(u <= b for u, b in zip(worst, bounds)), (worst, bounds)


# ---------------------------------------------------------------------------------------------
# plants reach the counters

@pytest.fixture(scope="module")
def expected_small(ops):
    return ops.valu_expected(SMALL["rounds"], seed=SEED)


@pytest.mark.parametrize("mask", MASKS, ids=[f"{m:#x}" for m in MASKS])
@pytest.mark.parametrize("where", ["first_wave", "last_wave"])
@pytest.mark.parametrize("round_", ["round0", "last_round"])
@pytest.mark.parametrize("lane", [0, 31, 32, 63])
@pytest.mark.parametrize("cls", range(7), ids=CLASSES)
def test_one_planted_word_is_detected_and_names_its_wave(ops, clean, expected_small, cls, lane, round_, where, mask):
    c = clean["small"]
    wave = 0 if where == "first_wave" else _waves(c, SMALL) - 1
    rnd, word = (0, 0) if round_ == "round0" else (SMALL["rounds"] - 1, WORDS[cls] - 1)
    r, planted = ops.valu_data(wave, check_plants=[(wave, CLASSES[cls], rnd, lane, word, mask)], seed=SEED, **SMALL)
    assert r["class_mismatches"] == [int(k == cls) for k in range(7)] and r["mismatches"] == 1
    # the wave's own record of where it ran, in this run
    assert 0 <= planted["cu_key"] < 2048 and planted["simd"] in range(4)
    assert r["first_bad_cu_key"] == planted["cu_key"] and r["first_bad_simd"] == planted["simd"]
    assert r["bad_cus"] == 1 and r["bad_simds"] == 1 and r["bad_cu_keys"] == [planted["cu_key"]]
    assert r["first_bad_lane"] == lane and r["first_bad_class"] == CLASSES[cls] and r["bad_lanes"] == f"0x{1 << lane:016x}"
    if cls < 6:  # the word it folded is the referee's with the mask in it, and nothing else moved
        want = expected_small["raw"].copy()
        want[rnd, BASE[cls] + word, lane] ^= np.uint32(mask)
        assert np.array_equal(planted["raw"][:, :BASE[6]], want[:, :BASE[6]])
    # one wave of 1024 cannot move the consensus, and the accuracy step judges a wave that holds it
    assert r["consensus_ok"] is True and r["trans_out_of_bound"] == 0
    assert r["values_checked"] == c["values_checked"] and r["cus_seen"] == c["cus_seen"] and r["simds_seen"] == c["simds_seen"]
    assert r["rate_ok"] is True  # a check plant never touches the rate phase
    assert r["passed"] is False


PLACE = ("first_bad_cu_key", "first_bad_simd", "bad_cu_keys")  # what the dispatcher decides anew in every run


def test_the_planted_entry_and_the_data_entry_count_a_plant_alike(ops, clean):
    wave = _waves(clean["small"], SMALL) - 1
    plant = [(wave, "cvt", 1, 63, 4, 0x8000)]
    p = ops.valu_planted(plant, [], seed=SEED, **SMALL)
    d, data = ops.valu_data(wave, check_plants=plant, seed=SEED, **SMALL)
    print("valu plant on wave", wave, "named CU key", p["first_bad_cu_key"], "SIMD", p["first_bad_simd"], "; in the data run",
          d["first_bad_cu_key"], d["first_bad_simd"])
    assert p["mismatches"] == 1 and p["bad_cu_keys"] == [p["first_bad_cu_key"]] and p["first_bad_simd"] in range(4)
    assert {k: v for k, v in _untimed(p).items() if k not in PLACE} == {k: v for k, v in _untimed(d).items() if k not in PLACE}


def test_plants_on_two_waves_name_the_lower_place_first(ops, clean):
    """first_bad_* is the mismatch with the lowest (CU key, SIMD): the run is asked for each wave's place in turn"""
    last = _waves(clean["small"], SMALL) - 1
    plants = [(0, "dot", 0, 5, 1, 0x10), (last, "fp16", 1, 9, 2, 0x4)]
    for wave in (0, last):
        r, data = ops.valu_data(wave, check_plants=plants, seed=SEED, **SMALL)
        assert r["mismatches"] == 2 and r["bad_simds"] in (1, 2) and 1 <= r["bad_cus"] <= r["bad_simds"] and len(r["bad_cu_keys"]) == r["bad_cus"]
        assert data["cu_key"] in r["bad_cu_keys"] and r["bad_cu_keys"] == sorted(r["bad_cu_keys"])
        assert (r["first_bad_cu_key"], r["first_bad_simd"]) <= (data["cu_key"], data["simd"])
        assert r["bad_lanes"] == f"0x{1 << 5 | 1 << 9:016x}"


def test_the_four_waves_of_a_workgroup_are_one_cu(ops, clean):
    """a workgroup runs on one CU whatever the dispatcher does, so four plants in one workgroup name one CU"""
    first = _waves(clean["small"], SMALL) - 4
    r = ops.valu_planted([(first + k, "int32", 0, 8 * k, k, 1 << k) for k in range(4)], [], seed=SEED, **SMALL)
    print("valu workgroup plant", r["bad_cus"], r["bad_simds"], r["bad_cu_keys"])
    assert r["class_mismatches"] == [4, 0, 0, 0, 0, 0, 0] and r["bad_cus"] == 1 and 1 <= r["bad_simds"] <= 4
    assert r["bad_lanes"] == f"0x{1 | 1 << 8 | 1 << 16 | 1 << 24:016x}" and r["first_bad_lane"] in (0, 8, 16, 24)


def test_two_plants_on_one_word_whose_masks_cancel(ops, clean):
    r = ops.valu_planted([(7, "fp64", 1, 5, 3, 0xDEADBEEF), (7, "fp64", 1, 5, 3, 0xDEADBEEF)], [], seed=SEED, **SMALL)
    assert _untimed(r) == _untimed(clean["small"])


@pytest.mark.parametrize("cls", range(6), ids=CLASSES[:6])
def test_a_plant_on_every_wave_of_an_exact_class(ops, clean, cls):
    c = clean["small"]
    r = ops.valu_planted([(ops.ALL_WAVES, CLASSES[cls], 1, 40, WORDS[cls] - 1, 0x100)], [], seed=SEED, **SMALL)
    assert r["class_mismatches"] == [_waves(c, SMALL) * int(k == cls) for k in range(7)]
    assert r["bad_cus"] == r["cus_seen"] == c["cus_seen"] and r["bad_simds"] == r["simds_seen"] == c["simds_seen"]
    assert len(r["bad_cu_keys"]) == min(64, r["bad_cus"]) and r["bad_cu_keys"] == sorted(set(r["bad_cu_keys"]))
    assert r["first_bad_cu_key"] == r["bad_cu_keys"][0] and r["first_bad_lane"] == 40 and r["bad_lanes"] == f"0x{1 << 40:016x}"
    assert r["consensus_ok"] is True and r["trans_out_of_bound"] == 0 and r["rate_ok"] is True and r["passed"] is False


@pytest.mark.parametrize("mask", [0x80000000, 0x40000000, 0x00400000], ids=["sign", "exponent", "significand"])
@pytest.mark.parametrize("word", range(5), ids=["exp", "log", "rcp", "rsq", "sqrt"])
def test_a_plant_on_every_wave_of_the_transcendentals_moves_the_consensus_and_breaks_the_bound(ops, clean, word, mask):
    """Every wave holds the same wrong value, so the consensus is that value and no wave mismatches: the limit of
    consensus.  A flipped sign, exponent bit or top significand bit is far beyond 2 units in the last place."""
    r = ops.valu_planted([(ops.ALL_WAVES, "trans", 0, 17, word, mask)], [], seed=SEED, **SMALL)
    assert r["class_mismatches"] == [0] * 7 and r["mismatches"] == 0 and r["consensus_ok"] is True and r["bad_cus"] == 0
    assert r["trans_out_of_bound"] == 1
    assert r["rate_ok"] is True and r["passed"] is False


def test_a_plant_beyond_the_launch_is_refused(ops, clean):
    waves = _waves(clean["small"], SMALL)
    beyond = "valu diag: invalid arguments: plant in a wave beyond the launch"
    with pytest.raises(RuntimeError, match=beyond):
        ops.valu_planted([(waves, "int32", 0, 0, 0, 1)], [], seed=SEED, **SMALL)
    with pytest.raises(RuntimeError, match=beyond):
        ops.valu_planted([], [(0, "fp32", 0, 0, 1), (waves + 3, "fp32", 0, 0, 1)], seed=SEED, **SMALL)
    with pytest.raises(RuntimeError, match=beyond):
        ops.valu_delayed([(waves, "trans", 1)], seed=SEED, **SMALL)
    with pytest.raises(RuntimeError, match=beyond):
        ops.valu_data(waves, seed=SEED, **SMALL)


# ---------------------------------------------------------------------------------------------
# the rate phase

@pytest.mark.parametrize("name,args", [("small", SMALL), ("large", LARGE)])
@pytest.mark.parametrize("cls", RATE_CLASSES)
def test_a_rate_plant_clears_rate_ok_and_nothing_else(ops, clean, cls, name, args):
    c = clean[name]
    for wave, lane, chain, mask in ((0, 0, 0, 0x1), (_waves(c, args) - 1, 63, 7, 0x80000000)):
        r = ops.valu_planted([], [(wave, cls, lane, chain, mask)], seed=SEED, **args)
        assert r["rate_ok"] is False and r["passed"] is False
        assert _untimed(dict(r, rate_ok=True, passed=True)) == _untimed(c)


T = 200_000  # ticks of the 100 MHz constant clock: 2 ms


@pytest.mark.parametrize("where", ["first_wave", "last_wave"])
@pytest.mark.parametrize("cls", range(5), ids=RATE_CLASSES)
def test_a_delayed_wave_shows_in_its_class_and_names_its_cu(ops, clean, cls, where):
    c = clean["small"]
    wave = 0 if where == "first_wave" else _waves(c, SMALL) - 1
    r, delayed = ops.valu_data(wave, delays=[(wave, RATE_CLASSES[cls], T)], seed=SEED, **SMALL)
    print("valu delayed", RATE_CLASSES[cls], where, {k: r[k] for k in TIMES}, "ran on", delayed["rate_cu_key"], "clean", {k: c[k] for k in TIMES})
    assert r["rate_ms"][cls] >= 2.0  # the launch cannot end before its wave's 2 ms
    assert r[RATES[cls]] <= c["cus"] * 4 * 64 * 8 * SMALL["rate_iters"] * 4 / 2e-3 / 1e12  # at most 4 operations a step
    # the CU that the wave recorded in that class's timed launch of this run has waited 2 ms more than any other
    assert all(0 <= key < 2048 for key in delayed["rate_cu_key"])
    assert r["slowest_cu_key"] == delayed["rate_cu_key"][cls]
    assert r["cu_balance"] < min(c["cu_balance"], 0.5)
    assert _untimed(r) == _untimed(c)  # nothing else moves: no value is touched


def test_the_delayed_entry_shows_the_delay_alike(ops, clean):
    r = ops.valu_delayed([(3, "fp64", T)], seed=SEED, **SMALL)
    assert r["rate_ms"][2] >= 2.0 and 0 <= r["slowest_cu_key"] < 2048 and r["cu_balance"] < 0.5
    assert _untimed(r) == _untimed(clean["small"])
