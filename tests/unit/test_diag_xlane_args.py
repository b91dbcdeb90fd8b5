"""The cross-lane diagnostic's entries (bgc_diag_xlane, its planted, delayed and generated-data variants and the
host referee's bgc_diag_xlane_expected) refuse every out-of-range argument with "invalid arguments" on the host,
before the first HIP call: the sizes decide what the kernels address, and a plant names a wave, a lane and a
result word that a kernel thread compares its own with.  Because the refusal comes first, these run without a
GPU (with one, a valid call would succeed; without, it would fail with a HIP error instead)."""
import ctypes

import pytest

SEED = 0x5EED
MAX_PLANTS = 4096  # BGC_DIAG_MAX_PLANTS
MAX_DELAY_TICKS = 10_000_000  # BGC_DIAG_MAX_DELAY_TICKS
CLASS_WORDS = (12, 6, 6, 3, 4, 6, 6, 4)
OK_CHECK = (0, 0, 0, 0, 0, 1)  # wave, class, round, lane, result word, mask
OK_RATE = (0, 0, 0, 0, 1)  # wave, rate class, lane, chain, mask
OK_DELAY = (0, 0, 1)  # wave, rate class, ticks
WPS, ROUNDS, ITERS = 1, 2, 16


def _refused(call, *args):
    with pytest.raises(RuntimeError) as e:
        call(*args)
    assert str(e.value) == "xlane diag: invalid arguments"


SIZES = {
    "waves_per_simd_0": (0, 2, 16), "waves_per_simd_9": (9, 2, 16), "waves_per_simd_-1": (-1, 2, 16),
    "rounds_0": (1, 0, 16), "rounds_65": (1, 65, 16), "rounds_-1": (1, -1, 16),
    "rate_iters_0": (1, 2, 0), "rate_iters_-1": (1, 2, -1), "rate_iters_over_2^16": (1, 2, (1 << 16) + 1),
}


@pytest.mark.parametrize("sizes", SIZES.values(), ids=SIZES.keys())
def test_xlane_sizes_out_of_range(nat, sizes):
    wps, rounds, iters = sizes
    _refused(nat.diag_xlane, 0, wps, rounds, iters, SEED)
    _refused(nat.diag_xlane_planted, 0, wps, rounds, iters, SEED, [], [])
    _refused(nat.diag_xlane_delayed, 0, wps, rounds, iters, SEED, [])
    _refused(nat.diag_xlane_delayed, 0, wps, rounds, iters, SEED, [OK_DELAY])
    _refused(nat.diag_xlane_data, 0, wps, rounds, iters, SEED, 0, [], [], [])


CHECK_PLANTS = {
    "wave_-2": (-2, 0, 0, 0, 0, 1), "class_8": (0, 8, 0, 0, 0, 1), "class_-1": (0, -1, 0, 0, 0, 1),
    "round_at_rounds": (0, 0, ROUNDS, 0, 0, 1), "round_-1": (0, 0, -1, 0, 0, 1),
    "lane_64": (0, 0, 0, 64, 0, 1), "lane_-1": (0, 0, 0, -1, 0, 1), "word_-1": (0, 0, 0, 0, -1, 1),
    "mask_0": (0, 0, 0, 0, 0, 0), "all_waves_mask_0": (-1, 7, 1, 63, 3, 0),
    **{f"word_past_class_{c}": (0, c, 0, 0, n, 1) for c, n in enumerate(CLASS_WORDS)},
}


@pytest.mark.parametrize("plant", CHECK_PLANTS.values(), ids=CHECK_PLANTS.keys())
def test_check_plant_out_of_range(nat, plant):
    _refused(nat.diag_xlane_planted, 0, WPS, ROUNDS, ITERS, SEED, [plant], [])
    _refused(nat.diag_xlane_planted, 0, WPS, ROUNDS, ITERS, SEED, [OK_CHECK, plant], [])  # not only the first one is checked
    _refused(nat.diag_xlane_planted, 0, WPS, ROUNDS, ITERS, SEED, [plant], [OK_RATE])
    _refused(nat.diag_xlane_data, 0, WPS, ROUNDS, ITERS, SEED, 0, [OK_CHECK, plant], [], [])


RATE_PLANTS = {
    "wave_-2": (-2, 0, 0, 0, 1), "class_4": (0, 4, 0, 0, 1), "class_-1": (0, -1, 0, 0, 1), "lane_64": (0, 0, 64, 0, 1),
    "lane_-1": (0, 0, -1, 0, 1), "chain_8": (0, 0, 0, 8, 1), "chain_-1": (0, 0, 0, -1, 1), "mask_0": (0, 3, 63, 7, 0),
}


@pytest.mark.parametrize("plant", RATE_PLANTS.values(), ids=RATE_PLANTS.keys())
def test_rate_plant_out_of_range(nat, plant):
    _refused(nat.diag_xlane_planted, 0, WPS, ROUNDS, ITERS, SEED, [], [plant])
    _refused(nat.diag_xlane_planted, 0, WPS, ROUNDS, ITERS, SEED, [], [OK_RATE, plant])
    _refused(nat.diag_xlane_planted, 0, WPS, ROUNDS, ITERS, SEED, [OK_CHECK], [plant])
    _refused(nat.diag_xlane_data, 0, WPS, ROUNDS, ITERS, SEED, 0, [], [OK_RATE, plant], [])


DELAYS = {
    "ticks_0": (0, 0, 0), "ticks_over_max": (0, 0, MAX_DELAY_TICKS + 1), "all_ticks_0": (-1, 0, 0), "wave_-2": (-2, 0, 1),
    "class_4": (0, 4, 1), "class_-1": (0, -1, 1),
}


@pytest.mark.parametrize("delay", DELAYS.values(), ids=DELAYS.keys())
def test_delay_out_of_range(nat, delay):
    _refused(nat.diag_xlane_delayed, 0, WPS, ROUNDS, ITERS, SEED, [delay])
    _refused(nat.diag_xlane_delayed, 0, WPS, ROUNDS, ITERS, SEED, [OK_DELAY, delay])
    _refused(nat.diag_xlane_data, 0, WPS, ROUNDS, ITERS, SEED, 0, [], [], [OK_DELAY, delay])


def test_plant_lists_too_long(nat):
    _refused(nat.diag_xlane_planted, 0, WPS, ROUNDS, ITERS, SEED, [OK_CHECK] * (MAX_PLANTS + 1), [])
    _refused(nat.diag_xlane_planted, 0, WPS, ROUNDS, ITERS, SEED, [], [OK_RATE] * (MAX_PLANTS + 1))
    _refused(nat.diag_xlane_delayed, 0, WPS, ROUNDS, ITERS, SEED, [OK_DELAY] * (MAX_PLANTS + 1))
    _refused(nat.diag_xlane_data, 0, WPS, ROUNDS, ITERS, SEED, 0, [OK_CHECK] * (MAX_PLANTS + 1), [], [])
    _refused(nat.diag_xlane_data, 0, WPS, ROUNDS, ITERS, SEED, 0, [], [OK_RATE] * (MAX_PLANTS + 1), [])
    _refused(nat.diag_xlane_data, 0, WPS, ROUNDS, ITERS, SEED, 0, [], [], [OK_DELAY] * (MAX_PLANTS + 1))


def test_data_wave_negative(nat):
    _refused(nat.diag_xlane_data, 0, WPS, ROUNDS, ITERS, SEED, -1, [], [], [])


@pytest.mark.parametrize("rounds", [0, 65, -1])
def test_expected_rounds_out_of_range(nat, rounds):
    _refused(nat.diag_xlane_expected, SEED, rounds)


def test_xlane_null_pointers_and_negative_counts():
    """The bindings always pass buffers and a list's own length, so these go to the C ABI directly."""
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    lib.bgc_diag_last_error.restype = ctypes.c_char_p
    out = ctypes.create_string_buffer(4096)  # larger than the result struct
    zeros = ctypes.create_string_buffer(4096)  # plants with mask 0 or ticks 0, were they ever looked at
    u32, i32 = ctypes.c_uint32, ctypes.c_int
    run = [i32(0), i32(WPS), i32(ROUNDS), i32(ITERS), u32(SEED)]
    no_lists = [None, i32(0), None, i32(0), None, i32(0)]
    wave = ctypes.create_string_buffer(8 + 4 * 4 + 4 * 8 * 64 + 4 * 64 * 47 * 64)  # bgc_xlane_wave; never written: every call is refused
    calls = [
        (lib.bgc_diag_xlane, run + [None]),
        (lib.bgc_diag_xlane_planted, run + [None, i32(0), None, i32(0), None]),
        (lib.bgc_diag_xlane_planted, run + [zeros, i32(-1), None, i32(0), out]),
        (lib.bgc_diag_xlane_planted, run + [None, i32(0), zeros, i32(-1), out]),
        (lib.bgc_diag_xlane_planted, run + [None, i32(1), None, i32(0), out]),  # a count without a list
        (lib.bgc_diag_xlane_planted, run + [None, i32(0), None, i32(1), out]),
        (lib.bgc_diag_xlane_delayed, run + [None, i32(0), None]),
        (lib.bgc_diag_xlane_delayed, run + [zeros, i32(-1), out]),
        (lib.bgc_diag_xlane_delayed, run + [None, i32(1), out]),
        (lib.bgc_diag_xlane_data, run + [i32(0)] + no_lists + [None, out]),  # no destination
        (lib.bgc_diag_xlane_data, run + [i32(0)] + no_lists + [zeros, None]),
        (lib.bgc_diag_xlane_data, run + [i32(0), zeros, i32(-1), None, i32(0), None, i32(0), wave, out]),
        (lib.bgc_diag_xlane_data, run + [i32(0), None, i32(0), None, i32(1), None, i32(0), wave, out]),  # a count without a list
        (lib.bgc_diag_xlane_data, run + [i32(0), None, i32(0), None, i32(0), zeros, i32(-1), wave, out]),
        (lib.bgc_diag_xlane_expected, [u32(SEED), i32(2), None]),
    ]
    for fn, args in calls:
        fn.restype = ctypes.c_int
        assert fn(*args) != 0, fn.__name__
        assert lib.bgc_diag_last_error().decode() == "invalid arguments", (fn.__name__, lib.bgc_diag_last_error())


def test_abi_version_and_class_tables():
    import os
    import re

    from bacchus_gpu_controller_amd import REPO_ROOT, ops
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    assert lib.bgc_diag_abi_version() == 15
    with open(os.path.join(REPO_ROOT, "native", "gpu", "hip", "gpu_diag.h")) as f:
        defines = dict(re.findall(r"^#define BGC_XLANE_(\w+) (\d+)", f.read(), re.M))
    assert int(defines.pop("CLASSES")) == len(ops.XLANE_CLASSES) == len(ops.XLANE_CLASS_WORDS) == 8
    assert int(defines.pop("ROUND_WORDS")) == ops.XLANE_ROUND_WORDS == sum(ops.XLANE_CLASS_WORDS) == 47
    assert int(defines.pop("RATE_CLASSES")) == len(ops.XLANE_RATE_CLASSES) == 4
    assert ops.XLANE_CLASS_WORDS == CLASS_WORDS
    rate = {k[5:]: int(v) for k, v in defines.items() if k.startswith("RATE_")}
    check = {k: int(v) for k, v in defines.items() if not k.startswith("RATE_")}
    assert [name.upper() for name in ops.XLANE_CLASSES] == sorted(check, key=check.get) and sorted(check.values()) == list(range(8))
    assert [name.upper() for name in ops.XLANE_RATE_CLASSES] == sorted(rate, key=rate.get) and sorted(rate.values()) == list(range(4))
    assert ops.XLANE_WAVE.itemsize == 8 + 4 * 4 + 4 * 8 * 64 + 4 * 64 * 47 * 64  # bgc_xlane_wave
