"""The cache diagnostic (bgc_diag_cache): the march through every XCD's L2 with its read rate, and the
Infinity Cache's pattern check with its read rate.

* A clean run checks every word of every region twice per round and every word of the
  Infinity-Cache buffer twice, and finds nothing; its JSON has exactly these keys and types.
* The data the march leaves in the L2 buffer and the Infinity-Cache buffer are the documented
  patterns (gpu_diag.h), compared word for word with a numpy reference written here, the rotation
  of the regions over the workgroups included.
* One wrong bit, the top bit or all bits planted in one word of an L2 region, in either pass, in the
  first or the last workgroup and round, at either end of the region, reaches every counter: one
  mismatch, one bad XCC, that word of the buffer, that mask.  A word planted in the Infinity-Cache
  buffer is counted by every check that runs after it and by the sweeps' sum if they read it.
* A workgroup of the timed L2 rate launch that is made to wait 2 ms shows in the rate and in its
  XCC's time, and nowhere else.

Every plant is an XOR of a value inside a buffer, applied between a fill and its check: no kernel
reads or writes out of bounds and every one runs to completion.  Every expected value is computed
here from the arguments and the plant list alone; no assertion compares with a measured rate."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED
KIB, MIB = 1 << 10, 1 << 20
REGIONS = [32 * KIB, 96 * KIB]  # one slab (the slab loops run once) and three
ROUNDS = 2
L2_SWEEPS = 16
IC = 2 * MIB
IC_WORDS = IC // 4
IC_SWEEPS = 2
GOLDEN = 0x9E3779B9
NONE = type(None)
CACHE = {"device": int, "cus": int, "xccs_seen": int, "rounds": int, "region_bytes": int, "l2_words_checked": int,
         "l2_mismatches": int, "l2_bad_xccs": int, "xcc_mismatches": int, "first_bad_xcc": NONE, "first_bad_word": NONE,
         "l2_bad_bits": NONE, "l2_read_tbps": float, "l2_rate_ok": bool, "xcc_wgs": int, "xcc_us": float, "slowest_xcc": int,
         "xcc_balance": float, "ic_bytes": int, "ic_words_checked": int, "ic_mismatches": int, "ic_first_bad_word": NONE,
         "ic_bad_bits": NONE, "ic_read_tbps": float, "ic_rate_ok": bool, "elapsed_ms": float, "passed": bool}
PER_XCC = ("xcc_mismatches", "xcc_wgs", "xcc_us")
TIMES = ("l2_read_tbps", "xcc_us", "slowest_xcc", "xcc_balance", "ic_read_tbps", "elapsed_ms")  # what a clock decides


@pytest.fixture(scope="module")
def ops():
    from bacchus_gpu_controller_amd import ops

    return ops


@pytest.fixture(scope="module")
def clean(ops):
    return {region: ops.cache(rounds=ROUNDS, region_bytes=region, l2_sweeps=L2_SWEEPS, ic_bytes=IC, ic_sweeps=IC_SWEEPS, seed=SEED)
            for region in REGIONS}


def _untimed(r):
    return {k: v for k, v in r.items() if k not in TIMES}


# ---------------------------------------------------------------------------------------------
# the clean run

@pytest.mark.parametrize("region", REGIONS)
def test_clean_run(clean, region):
    r = clean[region]
    print("cache clean", region, {k: r[k] for k in ("cus", "xccs_seen", "xcc_wgs", "xcc_us") + TIMES})
    assert r["l2_mismatches"] == 0 and r["l2_bad_xccs"] == 0 and not any(r["xcc_mismatches"])
    assert r["ic_mismatches"] == 0 and r["l2_rate_ok"] is True and r["ic_rate_ok"] is True and r["passed"] is True
    assert r["cus"] > 0 and r["rounds"] == ROUNDS and r["region_bytes"] == region and r["ic_bytes"] == IC
    assert r["l2_words_checked"] == 2 * ROUNDS * r["cus"] * (region // 4)
    assert r["ic_words_checked"] == 2 * IC // 4
    assert sum(r["xcc_wgs"]) == r["cus"]
    assert 1 <= r["xccs_seen"] <= 8 and r["xccs_seen"] == sum(1 for w in r["xcc_wgs"] if w)
    assert 0 < r["xcc_balance"] <= 1 and r["xcc_wgs"][r["slowest_xcc"]] > 0
    assert r["l2_read_tbps"] > 0 and r["ic_read_tbps"] > 0
    assert all((us > 0) == (wgs > 0) for us, wgs in zip(r["xcc_us"], r["xcc_wgs"]))


def test_result_shape(clean):
    r = clean[REGIONS[1]]
    assert list(r) == list(CACHE)
    wrong = {k: type(r[k]).__name__ for k in CACHE if k not in PER_XCC and type(r[k]) is not CACHE[k]}
    assert not wrong, wrong
    for k in PER_XCC:  # one entry per XCC of the device, up to the highest that ran a workgroup
        assert type(r[k]) is list and 1 <= len(r[k]) <= 8 and len(r[k]) == len(r["xcc_wgs"]), k
        assert all(type(v) is CACHE[k] for v in r[k]), k
    assert r["xcc_wgs"][-1] > 0


def test_infinity_cache_phase_off(ops, clean):
    r = ops.cache(rounds=1, region_bytes=REGIONS[0], l2_sweeps=L2_SWEEPS, ic_bytes=0, ic_sweeps=IC_SWEEPS, seed=SEED)
    assert list(r) == list(CACHE)
    assert r["ic_bytes"] == 0 and r["ic_words_checked"] == 0 and r["ic_mismatches"] == 0 and r["ic_read_tbps"] is None
    assert r["ic_rate_ok"] is True and r["l2_mismatches"] == 0 and r["passed"] is True
    assert r["l2_words_checked"] == 2 * r["cus"] * (REGIONS[0] // 4)


@pytest.mark.parametrize("region", REGIONS)
def test_planted_and_delayed_variants_without_plants_are_the_same_run(ops, clean, region):
    args = dict(rounds=ROUNDS, region_bytes=region, l2_sweeps=L2_SWEEPS, ic_bytes=IC, ic_sweeps=IC_SWEEPS, seed=SEED)
    for r in (ops.cache_planted([], [], **args), ops.cache_delayed([], **args)):
        assert list(r) == list(CACHE)
        assert _untimed(r) == _untimed(clean[region])


# ---------------------------------------------------------------------------------------------
# generated data

def _mix32(x):
    x = np.array(x, dtype=np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def _l2_reference(cus, region, rounds, passes, seed=SEED):
    """The buffer after the last round, r = rounds - 1: region g was written by workgroup b = (g - r) mod cus
    with s = mix32(seed + (r * cus + b + 1) * GOLDEN); word j holds mix32(j ^ s), inverted after pass 1."""
    r = rounds - 1
    b = (np.arange(cus, dtype=np.int64) - r) % cus
    s = _mix32((seed + (r * cus + b + 1) * GOLDEN) & 0xFFFFFFFF)
    ref = _mix32(np.arange(region // 4, dtype=np.uint32)[None, :] ^ s[:, None])
    return ~ref if passes == 2 else ref


def _ic_reference(seed=SEED):
    return _mix32(np.arange(IC_WORDS, dtype=np.uint32) ^ _mix32([~seed & 0xFFFFFFFF])[0])


@pytest.fixture(scope="module")
def images(ops):
    return {(region, rounds, passes): ops.cache_data(passes, rounds=rounds, region_bytes=region, l2_sweeps=L2_SWEEPS, ic_bytes=IC,
                                                     ic_sweeps=IC_SWEEPS, seed=SEED)
            for region, rounds, passes in ((REGIONS[0], 1, 1), (REGIONS[0], 2, 2), (REGIONS[1], 2, 1), (REGIONS[1], 2, 2))}


@pytest.mark.parametrize("region,rounds,passes", [(REGIONS[0], 1, 1), (REGIONS[0], 2, 2), (REGIONS[1], 2, 1), (REGIONS[1], 2, 2)])
def test_l2_buffer_is_the_documented_pattern(images, region, rounds, passes):
    r, l2, _ = images[(region, rounds, passes)]
    assert l2.dtype == np.dtype("<u4") and l2.shape == (r["cus"], region // 4)
    ref = _l2_reference(r["cus"], region, rounds, passes)
    assert np.array_equal(l2, ref), np.argwhere(l2 != ref)[:8]
    # the last round ends after `passes` passes, every earlier one after two
    assert r["l2_words_checked"] == (2 * (rounds - 1) + passes) * r["cus"] * (region // 4)
    assert r["l2_mismatches"] == 0 and r["passed"] is True


def test_regions_rotate_and_no_two_hold_the_same_word(images):
    _, one_round, _ = images[(REGIONS[0], 1, 1)]
    _, two_rounds, _ = images[(REGIONS[0], 2, 2)]
    cus = one_round.shape[0]
    # round 0 puts workgroup b on region b, round 1 on region b + 1 with another seed: nothing of round 0 is left
    assert np.array_equal(one_round, _l2_reference(cus, REGIONS[0], 1, 1))
    assert np.all(~two_rounds != one_round)
    assert np.all(one_round[0] != one_round[cus - 1]) and len(np.unique(one_round[0])) == REGIONS[0] // 4


def test_infinity_cache_buffer_is_the_documented_pattern_and_its_sum_is_S(images):
    """ic_rate_ok compares the sweeps' 32-bit total with ic_sweeps * S, S being what ic_fill summed from the
    hash in registers.  The buffer the sweeps read is the reference word for word, so its sum is S as numpy
    computes it, and a True ic_rate_ok says the sweeps read ic_sweeps * that sum
    (test_infinity_cache_plant_before_the_sweeps shows that any other total turns it False)."""
    ref = _ic_reference()
    s_ref = int(ref.sum(dtype=np.uint64)) & 0xFFFFFFFF
    for (region, rounds, passes), (r, _, ic) in images.items():
        assert ic.dtype == np.dtype("<u4") and ic.shape == (IC_WORDS,)
        assert np.array_equal(ic, ref), np.flatnonzero(ic != ref)[:8]
        assert int(ic.sum(dtype=np.uint64)) & 0xFFFFFFFF == s_ref
        assert r["ic_rate_ok"] is True and r["ic_mismatches"] == 0 and r["ic_words_checked"] == 2 * IC_WORDS
    assert len(np.unique(ref)) == IC_WORDS  # mix32 is a bijection


# ---------------------------------------------------------------------------------------------
# L2 detection

MASKS = [0x1, 0x80000000, 0xFFFFFFFF]


def _planted(ops, region, l2_plants, ic_plants=(), rounds=ROUNDS, ic_sweeps=IC_SWEEPS):
    return ops.cache_planted(l2_plants, ic_plants, rounds=rounds, region_bytes=region, l2_sweeps=L2_SWEEPS, ic_bytes=IC,
                             ic_sweeps=ic_sweeps, seed=SEED)


@pytest.mark.parametrize("mask", MASKS, ids=[f"{m:#x}" for m in MASKS])
@pytest.mark.parametrize("round_", ["round0", "last_round"])
@pytest.mark.parametrize("where", ["wg0", "last_wg"])
@pytest.mark.parametrize("pass_", [0, 1])
@pytest.mark.parametrize("end", ["first_word", "last_word"])
@pytest.mark.parametrize("region", REGIONS)
def test_one_planted_l2_word_is_detected(ops, clean, region, end, pass_, where, round_, mask):
    cus, words = clean[region]["cus"], region // 4
    wg = 0 if where == "wg0" else cus - 1
    rnd = 0 if round_ == "round0" else ROUNDS - 1
    word = 0 if end == "first_word" else words - 1
    r = _planted(ops, region, [(rnd, wg, pass_, word, mask)])
    assert r["l2_mismatches"] == 1 and r["l2_bad_xccs"] == 1
    assert r["first_bad_word"] == ((wg + rnd) % cus) * words + word  # in round r workgroup b works on region (b + r) % cus
    assert r["l2_bad_bits"] == f"0x{mask:08x}"
    assert r["xcc_wgs"][r["first_bad_xcc"]] > 0
    assert r["xcc_mismatches"] == [int(x == r["first_bad_xcc"]) for x in range(len(r["xcc_mismatches"]))]
    assert r["l2_words_checked"] == clean[region]["l2_words_checked"]
    assert r["l2_rate_ok"] is True  # a plant never touches the rate phase
    assert r["ic_mismatches"] == 0 and r["ic_rate_ok"] is True and r["ic_bad_bits"] is None
    assert r["passed"] is False


@pytest.mark.parametrize("pass_", [0, 1])
def test_two_plants_on_one_word_whose_masks_cancel(ops, pass_):
    r = _planted(ops, REGIONS[1], [(1, 3, pass_, 12345, 0xDEADBEEF), (1, 3, pass_, 12345, 0xDEADBEEF)])
    assert r["l2_mismatches"] == 0 and r["l2_bad_xccs"] == 0 and r["l2_bad_bits"] is None and r["first_bad_word"] is None
    assert r["first_bad_xcc"] is None and r["l2_rate_ok"] is True and r["passed"] is True


def test_two_plants_on_different_words_of_one_workgroup(ops, clean):
    region = REGIONS[1]
    cus, words = clean[region]["cus"], region // 4
    wg = cus // 2
    r = _planted(ops, region, [(1, wg, 1, 20001, 0x00F00000), (1, wg, 0, 255, 0x0000000F)])
    assert r["l2_mismatches"] == 2 and r["l2_bad_xccs"] == 1
    assert r["first_bad_word"] == ((wg + 1) % cus) * words + 255 and r["l2_bad_bits"] == "0x00f0000f"
    assert r["passed"] is False


@pytest.mark.parametrize("rounds", [1, 2])
def test_a_plant_in_every_workgroup(ops, clean, rounds):
    """ALL_WAVES names every workgroup of one round, so the count does not depend on `rounds`; the march and
    the rate launch are dealt to the XCCs alike, so the wrong words spread as xcc_wgs."""
    region = REGIONS[0]
    cus = clean[region]["cus"]
    r = _planted(ops, region, [(rounds - 1, ops.ALL_WAVES, 1, 4000, 0x100)], rounds=rounds)
    assert r["l2_mismatches"] == cus
    assert r["xcc_mismatches"] == r["xcc_wgs"] and r["l2_bad_xccs"] == r["xccs_seen"] > 0
    assert r["first_bad_xcc"] == min(x for x, w in enumerate(r["xcc_wgs"]) if w)
    assert r["first_bad_word"] % (region // 4) == 4000 and r["l2_bad_bits"] == "0x00000100"
    assert r["l2_rate_ok"] is True and r["passed"] is False


def test_a_plant_beyond_the_launch_is_refused(ops, clean):
    cus = clean[REGIONS[0]]["cus"]
    beyond = "cache diag: invalid arguments: plant in a workgroup beyond the launch"
    with pytest.raises(RuntimeError, match=beyond):
        _planted(ops, REGIONS[0], [(0, cus, 0, 0, 1)])
    with pytest.raises(RuntimeError, match=beyond):
        _planted(ops, REGIONS[0], [(0, 0, 0, 0, 1), (1, cus + 7, 1, 0, 1)])
    with pytest.raises(RuntimeError, match=beyond):
        ops.cache_delayed([(cus, 1)], rounds=1, region_bytes=REGIONS[0], l2_sweeps=L2_SWEEPS, ic_bytes=IC, ic_sweeps=IC_SWEEPS, seed=SEED)


# ---------------------------------------------------------------------------------------------
# Infinity-Cache detection.  Three sweeps: a plant changes the buffer's sum by d = (v ^ mask) - v, non-zero
# modulo 2^32, and the sweeps' total by ic_sweeps * d; the top bit's d is 2^31, which an even count cancels.

IC_DETECT_SWEEPS = 3


@pytest.mark.parametrize("mask", MASKS, ids=[f"{m:#x}" for m in MASKS])
@pytest.mark.parametrize("word", [0, IC_WORDS - 1], ids=["first_word", "last_word"])
def test_infinity_cache_plant_before_the_sweeps(ops, clean, word, mask):
    r = _planted(ops, REGIONS[0], [], [(0, word, mask)], rounds=1, ic_sweeps=IC_DETECT_SWEEPS)
    assert r["ic_mismatches"] == 2  # the check after the fill and the one after the sweeps
    assert r["ic_first_bad_word"] == word and r["ic_bad_bits"] == f"0x{mask:08x}"
    assert r["ic_rate_ok"] is False  # the sweeps read it three times
    assert r["ic_words_checked"] == 2 * IC_WORDS
    assert r["l2_mismatches"] == 0 and r["l2_rate_ok"] is True and r["first_bad_word"] is None
    assert r["passed"] is False


@pytest.mark.parametrize("mask", MASKS, ids=[f"{m:#x}" for m in MASKS])
@pytest.mark.parametrize("word", [0, IC_WORDS - 1], ids=["first_word", "last_word"])
def test_infinity_cache_plant_after_the_sweeps(ops, clean, word, mask):
    r = _planted(ops, REGIONS[0], [], [(1, word, mask)], rounds=1, ic_sweeps=IC_DETECT_SWEEPS)
    assert r["ic_mismatches"] == 1 and r["ic_first_bad_word"] == word and r["ic_bad_bits"] == f"0x{mask:08x}"
    assert r["ic_rate_ok"] is True  # the sweeps came first
    assert r["l2_mismatches"] == 0 and r["l2_rate_ok"] is True
    assert r["passed"] is False


def test_infinity_cache_plants_at_both_moments_and_in_l2(ops, clean):
    region = REGIONS[1]
    words = region // 4
    r = _planted(ops, region, [(0, 1, 0, 77, 0x4)], [(0, 1000, 0x10), (1, 500, 0x20), (1, 1000, 0x10)], ic_sweeps=IC_DETECT_SWEEPS)
    # word 1000 is wrong in the first check and put right before the last; word 500 is wrong in the last
    assert r["ic_mismatches"] == 2 and r["ic_first_bad_word"] == 500 and r["ic_bad_bits"] == "0x00000030"
    assert r["ic_rate_ok"] is False
    assert r["l2_mismatches"] == 1 and r["first_bad_word"] == words + 77 and r["l2_bad_bits"] == "0x00000004"


# ---------------------------------------------------------------------------------------------
# delays

T = 200_000  # ticks of the 100 MHz constant clock: 2 ms
T_US = 2000


def _delayed(ops, region, delays):
    return ops.cache_delayed(delays, rounds=ROUNDS, region_bytes=region, l2_sweeps=L2_SWEEPS, ic_bytes=IC, ic_sweeps=IC_SWEEPS, seed=SEED)


@pytest.mark.parametrize("region", REGIONS)
def test_a_delay_on_every_workgroup_reaches_the_rate_and_every_xcc(ops, clean, region):
    c = clean[region]
    r = _delayed(ops, region, [(ops.ALL_WAVES, T)])
    print("cache delayed all", region, {k: r[k] for k in TIMES}, "clean", {k: c[k] for k in TIMES})
    nbytes = c["cus"] * L2_SWEEPS * region
    assert 0 < r["l2_read_tbps"] <= nbytes / 2e-3 / 1e12  # the launch cannot end before its workgroups' 2 ms
    assert all(us >= T_US for us, wgs in zip(r["xcc_us"], r["xcc_wgs"]) if wgs)
    assert _untimed(r) == _untimed(c)  # nothing else moves: no value is touched


def test_a_delay_on_one_workgroup_names_its_xcc(ops, clean):
    region = REGIONS[1]
    c = clean[region]
    r = _delayed(ops, region, [(0, T)])
    print("cache delayed wg0", {k: r[k] for k in TIMES}, "clean", {k: c[k] for k in TIMES})
    x = r["slowest_xcc"]
    fastest_clean = min(us for us, wgs in zip(c["xcc_us"], c["xcc_wgs"]) if wgs)
    assert r["xcc_wgs"][x] > 0 and r["xcc_us"][x] >= fastest_clean + T_US / r["xcc_wgs"][x]  # the mean of its workgroups
    assert r["xcc_balance"] < c["xcc_balance"]
    assert _untimed(r) == _untimed(c)
