"""The LDS diagnostic (bgc_diag_lds): the per-CU march over all 160 KiB of every CU's Local Data
Share and the LDS read rate.

* A clean run checks every word twice and finds nothing; its JSON has exactly these keys and types.
* The data a march workgroup holds is the documented pattern (gpu_diag.h), compared word for word
  with a numpy reference written here.
* One wrong bit planted in one word, in either pass, in the first or the last workgroup, at either
  end of the array and on both sides of the 64 KiB line, reaches every counter: one mismatch, one
  bad CU, that word, that mask, and a verdict that names the CU.

Every plant is an XOR of a value inside the array, applied between a fill and its verify: no kernel
reads or writes out of bounds and every one runs to completion.  Every expected value is computed
here from the plant list alone."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED
WORDS = 40960
ITERS = 64
NONE = type(None)
LDS = {"device": int, "cus": int, "cus_seen": int, "bad_cus": int, "bad_cu_keys": [], "words_checked": int, "mismatches": int,
       "first_bad_cu_key": NONE, "first_bad_word": NONE, "bad_bits": NONE, "read_tbps": float, "rate_ok": bool,
       "slowest_cu_key": int, "cu_balance": float, "elapsed_ms": float, "passed": bool}


@pytest.fixture(scope="module")
def ops():
    from bacchus_gpu_controller_amd import ops

    return ops


@pytest.fixture(scope="module")
def clean(ops):
    return ops.lds(wgs_per_cu=2, rate_iters=ITERS, seed=SEED)


def _judge(r):
    from bacchus_gpu_controller_amd import native

    return json.loads(native().judge_diag(json.dumps({"lds": r}), json.dumps({"min_lds_read_tbps": 0, "min_lds_cu_coverage": 0})))


def _shape(value, spec):
    if isinstance(spec, list):
        return isinstance(value, list) and len(value) == len(spec) and all(_shape(v, s) for v, s in zip(value, spec))
    return type(value) is spec


def test_clean_run(clean):
    r = clean
    print("lds clean", {k: r[k] for k in ("cus", "cus_seen", "read_tbps", "cu_balance", "elapsed_ms")})
    assert r["mismatches"] == 0 and r["bad_cus"] == 0 and r["bad_cu_keys"] == []
    assert r["cus"] > 0 and r["words_checked"] == 2 * WORDS * 2 * r["cus"]
    assert 0 < r["cus_seen"] <= r["cus"]
    assert r["rate_ok"] is True and r["passed"] is True
    assert r["read_tbps"] > 0 and 0 < r["cu_balance"] <= 1 and r["slowest_cu_key"] >= 0
    assert _judge(r)["failures"] == []


def test_result_shape(clean):
    assert list(clean) == list(LDS)
    wrong = {k: type(clean[k]).__name__ for k in LDS if not _shape(clean[k], LDS[k])}
    assert not wrong, wrong


def test_planted_variant_without_plants_is_the_same_run(ops, clean):
    r = ops.lds_planted([], wgs_per_cu=2, rate_iters=ITERS, seed=SEED)
    assert list(r) == list(LDS)
    same = ("device", "cus", "bad_cus", "bad_cu_keys", "words_checked", "mismatches", "first_bad_cu_key", "first_bad_word",
            "bad_bits", "rate_ok", "passed")
    assert {k: r[k] for k in same} == {k: clean[k] for k in same}


# ---------------------------------------------------------------------------------------------
# generated data

def _mix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def _pattern(wg, pass_, seed=SEED):
    s = _mix32(np.array([(seed + (wg + 1) * 0x9E3779B9) & 0xFFFFFFFF], dtype=np.uint32))[0]
    p = _mix32(np.arange(WORDS, dtype=np.uint32) ^ s)
    return ~p if pass_ else p


GRID = 3


@pytest.fixture(scope="module")
def images(ops):
    return {(wg, p): ops.lds_data(wg, p, GRID, seed=SEED) for wg, p in ((0, 0), (0, 1), (GRID - 1, 0))}


@pytest.mark.parametrize("wg,pass_", [(0, 0), (0, 1), (GRID - 1, 0)], ids=["wg0_pass0", "wg0_pass1", "last_wg_pass0"])
def test_generated_data_is_the_documented_pattern(images, wg, pass_):
    got = images[(wg, pass_)]
    assert got.dtype == np.dtype("<u4") and got.shape == (WORDS,)
    assert np.array_equal(got, _pattern(wg, pass_)), np.flatnonzero(got != _pattern(wg, pass_))[:8]


def test_pass_1_is_the_inverse_and_workgroups_differ_in_every_word(images):
    assert np.array_equal(images[(0, 1)], ~images[(0, 0)])
    assert np.all(images[(0, 0)] != images[(GRID - 1, 0)])
    assert len(np.unique(images[(0, 0)])) == WORDS  # mix32 is a bijection: no two words of a workgroup are equal


# ---------------------------------------------------------------------------------------------
# detection

PLANT_WORDS = [0, 16383, 16384, 32768, WORDS - 1]  # both ends, both sides of the 64 KiB line, the 128 KiB line
MASKS = [0x1, 0x80000000, 0xFFFFFFFF]


def _last_wg(clean, wgs_per_cu=1):
    return clean["cus"] * wgs_per_cu - 1


@pytest.mark.parametrize("mask", MASKS, ids=[f"{m:#x}" for m in MASKS])
@pytest.mark.parametrize("where", ["wg0", "last_wg"])
@pytest.mark.parametrize("pass_", [0, 1])
@pytest.mark.parametrize("word", PLANT_WORDS)
def test_one_planted_word_is_detected(ops, clean, word, pass_, where, mask):
    wg = 0 if where == "wg0" else _last_wg(clean)
    r = ops.lds_planted([(wg, pass_, word, mask)], rate_iters=ITERS, seed=SEED)
    assert r["mismatches"] == 1 and r["bad_cus"] == 1 and len(r["bad_cu_keys"]) == 1
    assert r["first_bad_word"] == word and r["first_bad_cu_key"] == r["bad_cu_keys"][0]
    assert r["bad_bits"] == f"0x{mask:08x}"
    assert r["words_checked"] == 2 * WORDS * clean["cus"]
    assert r["rate_ok"] is True  # a plant never touches the rate phase
    assert r["passed"] is False
    j = _judge(r)
    assert j["passed"] is False and j["failures"] == [
        f"LDS march mismatches on 1 CU(s): 1 words (first on CU key {r['bad_cu_keys'][0]} at word {word}, bits 0x{mask:08x})"]


def test_two_plants_on_one_word_whose_masks_cancel(ops):
    r = ops.lds_planted([(0, 0, 12345, 0xDEADBEEF), (0, 0, 12345, 0xDEADBEEF)], rate_iters=ITERS, seed=SEED)
    assert r["mismatches"] == 0 and r["bad_cus"] == 0 and r["bad_bits"] is None and r["first_bad_word"] is None
    assert r["first_bad_cu_key"] is None and r["rate_ok"] is True and r["passed"] is True


@pytest.mark.parametrize("pass_", [0, 1])
def test_two_plants_on_different_words_of_one_workgroup(ops, clean, pass_):
    wg = _last_wg(clean) // 2
    r = ops.lds_planted([(wg, pass_, 30001, 0x00F00000), (wg, pass_, 255, 0x0000000F)], rate_iters=ITERS, seed=SEED)
    assert r["mismatches"] == 2 and r["bad_cus"] == 1
    assert r["first_bad_word"] == 255 and r["bad_bits"] == "0x00f0000f"
    assert r["rate_ok"] is True and r["passed"] is False


def test_one_word_planted_in_both_passes_counts_twice(ops):
    r = ops.lds_planted([(0, 0, 777, 0x10), (0, 1, 777, 0x20)], rate_iters=ITERS, seed=SEED)
    assert r["mismatches"] == 2 and r["bad_cus"] == 1 and r["first_bad_word"] == 777 and r["bad_bits"] == "0x00000030"


@pytest.mark.parametrize("wgs_per_cu", [1, 2])
def test_a_plant_in_every_workgroup(ops, clean, wgs_per_cu):
    r = ops.lds_planted([(ops.ALL_WAVES, 1, 20000, 0x100)], wgs_per_cu=wgs_per_cu, rate_iters=ITERS, seed=SEED)
    assert r["mismatches"] == clean["cus"] * wgs_per_cu
    assert r["bad_cus"] == r["cus_seen"] and r["cus_seen"] > 0
    assert r["bad_cu_keys"] == sorted(set(r["bad_cu_keys"])) and len(r["bad_cu_keys"]) == min(64, r["bad_cus"])
    assert r["first_bad_cu_key"] == r["bad_cu_keys"][0] and r["first_bad_word"] == 20000 and r["bad_bits"] == "0x00000100"
    assert r["rate_ok"] is True and r["passed"] is False


def test_a_plant_beyond_the_launch_is_refused(ops, clean):
    with pytest.raises(RuntimeError, match="lds diag: invalid arguments: plant in a workgroup beyond the launch"):
        ops.lds_planted([(_last_wg(clean) + 1, 0, 0, 1)], rate_iters=ITERS, seed=SEED)
    with pytest.raises(RuntimeError, match="lds diag: invalid arguments: plant in a workgroup beyond the launch"):
        ops.lds_planted([(0, 0, 0, 1), (_last_wg(clean, 2) + 1, 0, 0, 1)], wgs_per_cu=2, rate_iters=ITERS, seed=SEED)
