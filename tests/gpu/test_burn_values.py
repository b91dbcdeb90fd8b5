"""The burn's value check: `mismatches` of bgc_diag_burn_dtype, the count that judge_diag turns into
"burn-in MFMA accumulators wrong".

* Plants (ops.burn_planted): one accumulator element of one lane of one wave of one launch is changed
  after the launch's loop and before its comparison.  Each must add exactly one to the count, whichever
  launch it is in: the first (2048 iterations), a retuned one, the far end of the grid and of the wave
  reduction, a NaN, two chains of one lane.  The count must survive the launches after it, and nothing
  else of the result may move.
* The verdict fails on a planted burn with that one message and passes the clean one.
* The launch length: the throughput kernel compares acc == iters * tile + c in fp32, which is exact only
  while K * iters <= 2^23 (gpu_diag.h).  The burn reports no iteration count, but its FLOP count is
  tflops_mean * elapsed_ms and every launch but the first has the same length, so the count follows
  from the result.

Every plant adds to an accumulator register of a named lane: no kernel reads or writes out of bounds
and every one runs to completion.  torch stays on the CPU in this process."""
import json

import pytest

from test_diag_rates import _check_burn_summary

pytestmark = pytest.mark.gpu

BURN_MS = 200
DTYPES = ["bf16", "fp8", "fp4"]
K = {"bf16": 32, "fp8": 128, "fp4": 128}
FIRST_ITERS = 2048  # of launch 0, before the retune
NAN = float("nan")
KEYS = ["dtype", "launches", "elapsed_ms", "tflops_mean", "tflops_min", "tflops_first", "tflops_last", "tflops_max", "sustain",
        "mismatches"]
# tests/unit/test_gpu_health_rules.py: the burn's floors off, so that only the values are judged
BURN_FLOORS_OFF = json.dumps({k: 0 for k in ("min_burn_tflops", "min_burn_sustain", "max_burn_hotspot_c",
                                             "max_burn_thermal_violation_pct")})


@pytest.fixture(scope="module")
def ops():
    from bacchus_gpu_controller_amd import ops

    return ops


@pytest.fixture(scope="module")
def cus(ops):
    return ops.lds(wgs_per_cu=1, rate_iters=64)["cus"]


def _waves(cus, waves_per_cu):
    return max(1, cus * waves_per_cu // 4) * 4  # 256-thread blocks of 4 waves, as the header documents


@pytest.fixture(scope="module")
def clean(ops):
    """one burn without plants per dtype, shared by the tests that only read it"""
    return {dtype: ops.burn_planted(BURN_MS, [], dtype=dtype) for dtype in DTYPES}


# ---------------------------------------------------------------------------------------------
# a. plant counts.  plants: (launch, wave, lane, chain, i, delta); `last` is the launch's last wave

def _cases(last):
    return {
        "first_launch": ([(0, 0, 0, 0, 0, 1.0)], 1),
        "retuned_launch_far_end": ([(2, last, 63, 3, 3, 1.0)], 1),
        # the count must survive the launches after it
        "launches_0_1_2": ([(0, 5, 17, 1, 2, 1.0), (1, last, 63, 3, 3, 1.0), (2, 0, 0, 0, 0, 1.0)], 3),
        "nan": ([(1, last // 2, 31, 2, 0, NAN)], 1),
        "two_chains_of_one_lane": ([(1, 7, 40, 0, 1, 1.0), (1, 7, 40, 3, 1, 1.0)], 2),
        "launch_never_reached": ([(1 << 30, 0, 0, 0, 0, 1.0)], 0),
    }


@pytest.mark.parametrize("case", list(_cases(0)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_burn_counts_planted_accumulators(ops, cus, dtype, case):
    plants, count = _cases(_waves(cus, 32) - 1)[case]
    r = ops.burn_planted(BURN_MS, plants, dtype=dtype)
    print("burn planted", dtype, case, r)
    assert r["mismatches"] == count, r
    # what must not move
    assert list(r) == KEYS and r["dtype"] == dtype, r
    _check_burn_summary(r, BURN_MS)
    assert r["launches"] > 2, r  # the burn did reach the launches the cases name


@pytest.mark.parametrize("dtype", DTYPES)
def test_burn_without_plants_is_clean(ops, clean, dtype):
    r = clean[dtype]
    assert r["mismatches"] == 0 and r["dtype"] == dtype, r
    _check_burn_summary(r, BURN_MS)
    assert list(r) == KEYS == list(ops.burn_delayed(BURN_MS, 1 << 30, 1000, dtype=dtype)), r


def test_burn_plant_in_a_wave_beyond_the_launch_is_refused(ops, cus):
    waves = _waves(cus, 1)
    with pytest.raises(RuntimeError, match="burn: invalid arguments: plant in a wave beyond the launch"):
        ops.burn_planted(BURN_MS, [(0, 0, 0, 0, 0, 1.0), (1 << 30, waves, 0, 0, 0, 1.0)], waves_per_cu=1)


# ---------------------------------------------------------------------------------------------
# b. the verdict

@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_burn_fails_the_verdict_and_the_clean_one_passes(ops, clean, dtype):
    from bacchus_gpu_controller_amd import native

    planted = ops.burn_planted(BURN_MS, [(1, 3, 9, 2, 1, 1.0)], dtype=dtype)
    assert planted["mismatches"] == 1, planted
    judged = json.loads(native().judge_diag(json.dumps({"burn": planted}), BURN_FLOORS_OFF))
    assert judged["failures"] == ["burn-in MFMA accumulators wrong"] and judged["passed"] is False, judged
    judged = json.loads(native().judge_diag(json.dumps({"burn": clean[dtype]}), BURN_FLOORS_OFF))
    assert judged["failures"] == [] and judged["passed"] is True, judged


# ---------------------------------------------------------------------------------------------
# c. the launch length

# The JSON prints a double with the fewest digits that read back as the same double (std::to_chars), so it
# adds no error of its own: json.loads(dump(x)) == x.  What is left are the roundings of the arithmetic
# between the burn's exact FLOP count (an integer below 2^53) and the product formed here: four in the
# library (elapsed_ms * 1e-3, whose constant is itself rounded, the two divisions), two here (the two
# multiplications), each at most 2^-53 relative.  Sixteen of them is more than twice that; the
# deviations measured on the MI355X are in profiles/burn_value_check/README.md.
REL = 16 * 2.0 ** -53


def recovered_iters(r, cus, waves_per_cu, dtype):
    """(the retuned launches' iteration count, the relative deviation of the result's FLOP count from
    the count of FIRST_ITERS + (launches - 1) * iters iterations)"""
    flops_per_iter = _waves(cus, waves_per_cu) * 4 * 2 * 16 * 16 * K[dtype]  # 4 chains of 16x16xK MFMAs per wave
    flops = r["tflops_mean"] * r["elapsed_ms"] * 1e9
    iters = round((flops / flops_per_iter - FIRST_ITERS) / (r["launches"] - 1))
    exact = flops_per_iter * (FIRST_ITERS + (r["launches"] - 1) * iters)
    return iters, abs(flops - exact) / exact


@pytest.mark.parametrize("waves_per_cu", [1, 8, 32])
@pytest.mark.parametrize("dtype", DTYPES)
def test_burn_launch_length_stays_within_the_exactness_bound(ops, cus, dtype, waves_per_cu):
    r = ops.burn_planted(BURN_MS, [], dtype=dtype, waves_per_cu=waves_per_cu)
    assert r["launches"] >= 2, r
    iters, deviation = recovered_iters(r, cus, waves_per_cu, dtype)
    print(f"burn launch length: {dtype} waves_per_cu={waves_per_cu} iters={iters} K*iters/2^23={K[dtype] * iters / (1 << 23):.4f} "
          f"launches={r['launches']} deviation={deviation:.3e} tflops_mean={r['tflops_mean']:.1f}")
    assert deviation <= REL, (iters, deviation, r)  # an integer number of iterations
    assert 64 <= iters, (iters, r)
    assert K[dtype] * iters <= 1 << 23, (iters, r)
    assert r["mismatches"] == 0, r
