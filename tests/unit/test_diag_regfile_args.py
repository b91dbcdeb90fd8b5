"""The register-file diagnostic's entries (bgc_diag_regfile, its planted, delayed and generated-data variants, and the host
reference's bgc_diag_regfile_layout and _expected) refuse every out-of-range argument with "invalid arguments" on the host,
before the first HIP call: the sizes decide what the kernels address and how long they loop, and a plant names a wave, a
phase, a register and a lane that the kernel compares its own with.  Because the refusal comes first, these run without a
GPU (with one, a valid call would succeed; without, it would fail with a HIP error instead)."""
import ctypes

import pytest

SEED = 0x5EED
MAX_PLANTS = 4096  # BGC_DIAG_MAX_PLANTS
MAX_DELAY_TICKS = 10_000_000  # BGC_DIAG_MAX_DELAY_TICKS
MAX_DATA_BYTES = 128 << 20  # BGC_DIAG_MAX_DATA_BYTES
OK_PLANT = (0, 0, 2, 0, 1)  # wave, phase, slot, lane, mask: v128 in layout 0, pass 0
OK_DELAY = (0, 1)  # wave, ticks
WGS, SWEEPS = 1, 3


def _refused(call, *args):
    with pytest.raises(RuntimeError) as e:
        call(*args)
    assert str(e.value) == "regfile diag: invalid arguments"


SIZES = {"wgs_per_cu_0": (0, 3), "wgs_per_cu_9": (9, 3), "wgs_per_cu_-1": (-1, 3), "sweeps_0": (1, 0), "sweeps_-1": (1, -1),
         "sweeps_over_2^16": (1, (1 << 16) + 1)}


@pytest.mark.parametrize("sizes", SIZES.values(), ids=SIZES.keys())
def test_regfile_sizes_out_of_range(nat, sizes):
    wgs, sweeps = sizes
    _refused(nat.diag_regfile, 0, wgs, sweeps, SEED)
    _refused(nat.diag_regfile_planted, 0, wgs, sweeps, SEED, [])
    _refused(nat.diag_regfile_planted, 0, wgs, sweeps, SEED, [OK_PLANT])
    _refused(nat.diag_regfile_delayed, 0, wgs, sweeps, SEED, [OK_DELAY])
    _refused(nat.diag_regfile_data, 0, wgs, sweeps, SEED, 0, 0, [], [])


PLANTS = {
    "wave_-2": (-2, 0, 2, 0, 1), "phase_5": (0, 5, 2, 0, 1), "phase_-1": (0, -1, 2, 0, 1), "slot_8": (0, 0, 8, 0, 1), "slot_-1": (0, 0, -1, 0, 1),
    "lane_64": (0, 0, 2, 64, 1), "lane_-1": (0, 0, 2, -1, 1), "mask_0": (0, 0, 2, 0, 0),
    # a register that the phase keeps for itself holds no pattern: v0 and v5 in layout 0 and in the rotate, v250 and v255 in layout 1
    "v0_in_layout_0": (0, 0, 0, 0, 1), "v5_in_layout_0_pass_1": (0, 1, 1, 0, 1), "v0_in_rotate": (0, 4, 0, 0, 1), "v5_in_rotate": (0, 4, 1, 0, 1),
    "v250_in_layout_1": (0, 2, 3, 0, 1), "v255_in_layout_1_pass_1": (0, 3, 4, 0, 1),
}


@pytest.mark.parametrize("plant", PLANTS.values(), ids=PLANTS.keys())
def test_plant_out_of_range(nat, plant):
    _refused(nat.diag_regfile_planted, 0, WGS, SWEEPS, SEED, [plant])
    _refused(nat.diag_regfile_planted, 0, WGS, SWEEPS, SEED, [OK_PLANT, plant])  # not only the first one is checked
    _refused(nat.diag_regfile_data, 0, WGS, SWEEPS, SEED, 0, 0, [OK_PLANT, plant], [])
    _refused(nat.diag_regfile_expected, SEED, 0, 0, SWEEPS, [OK_PLANT, plant])


DELAYS = {"ticks_0": (0, 0), "ticks_over_max": (0, MAX_DELAY_TICKS + 1), "all_ticks_0": (-1, 0), "wave_-2": (-2, 1)}


@pytest.mark.parametrize("delay", DELAYS.values(), ids=DELAYS.keys())
def test_delay_out_of_range(nat, delay):
    _refused(nat.diag_regfile_delayed, 0, WGS, SWEEPS, SEED, [delay])
    _refused(nat.diag_regfile_delayed, 0, WGS, SWEEPS, SEED, [OK_DELAY, delay])
    _refused(nat.diag_regfile_data, 0, WGS, SWEEPS, SEED, 0, 0, [], [OK_DELAY, delay])


def test_lists_too_long(nat):
    _refused(nat.diag_regfile_planted, 0, WGS, SWEEPS, SEED, [OK_PLANT] * (MAX_PLANTS + 1))
    _refused(nat.diag_regfile_delayed, 0, WGS, SWEEPS, SEED, [OK_DELAY] * (MAX_PLANTS + 1))
    _refused(nat.diag_regfile_data, 0, WGS, SWEEPS, SEED, 0, 0, [OK_PLANT] * (MAX_PLANTS + 1), [])
    _refused(nat.diag_regfile_data, 0, WGS, SWEEPS, SEED, 0, 0, [], [OK_DELAY] * (MAX_PLANTS + 1))
    _refused(nat.diag_regfile_expected, SEED, 0, 0, SWEEPS, [OK_PLANT] * (MAX_PLANTS + 1))


DUMPS = {"wave_-1": (-1, 0), "phase_5": (0, 5), "phase_-1": (0, -1)}


@pytest.mark.parametrize("dump", DUMPS.values(), ids=DUMPS.keys())
def test_dump_and_expected_out_of_range(nat, dump):
    wave, phase = dump
    _refused(nat.diag_regfile_data, 0, WGS, SWEEPS, SEED, wave, phase, [], [])
    _refused(nat.diag_regfile_expected, SEED, wave, phase, SWEEPS, [])


def test_expected_sweeps_out_of_range(nat):
    _refused(nat.diag_regfile_expected, SEED, 0, 4, 0, [])
    _refused(nat.diag_regfile_expected, SEED, 0, 4, (1 << 16) + 1, [])


def test_regfile_null_pointers_negative_counts_and_capacity():
    """The bindings always pass buffers and a list's own length, so these go to the C ABI directly."""
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    lib.bgc_diag_last_error.restype = ctypes.c_char_p
    out = ctypes.create_string_buffer(4096)  # larger than the result struct
    zeros = ctypes.create_string_buffer(4096)  # plants with mask 0, or ticks 0, were they ever looked at
    words = ctypes.create_string_buffer(512 * 64 * 4)
    places = ctypes.create_string_buffer(8 * 64)
    u32, i32 = ctypes.c_uint32, ctypes.c_int
    run = [i32(0), i32(WGS), i32(SWEEPS), u32(SEED)]
    dump = [i32(0), i32(0)]  # wave, phase
    no_lists = [None, i32(0), None, i32(0)]
    over_cap = (MAX_DATA_BYTES - 512 * 64 * 4) // 16 + 1  # waves whose two places no longer fit beside the words
    calls = [
        (lib.bgc_diag_regfile, run + [None]),
        (lib.bgc_diag_regfile_planted, run + [None, i32(0), None]),
        (lib.bgc_diag_regfile_planted, run + [zeros, i32(-1), out]),
        (lib.bgc_diag_regfile_planted, run + [None, i32(1), out]),  # a count without a list
        (lib.bgc_diag_regfile_delayed, run + [None, i32(0), None]),
        (lib.bgc_diag_regfile_delayed, run + [zeros, i32(-1), out]),
        (lib.bgc_diag_regfile_delayed, run + [None, i32(1), out]),
        (lib.bgc_diag_regfile_data, run + dump + no_lists + [None, places, places, i32(64), out]),  # no destination
        (lib.bgc_diag_regfile_data, run + dump + no_lists + [words, None, places, i32(64), out]),
        (lib.bgc_diag_regfile_data, run + dump + no_lists + [words, places, None, i32(64), out]),
        (lib.bgc_diag_regfile_data, run + dump + no_lists + [words, places, places, i32(64), None]),
        (lib.bgc_diag_regfile_data, run + dump + no_lists + [words, places, places, i32(0), out]),  # room for no wave
        (lib.bgc_diag_regfile_data, run + dump + no_lists + [words, places, places, i32(over_cap), out]),  # more than the cap
        (lib.bgc_diag_regfile_data, run + dump + [None, i32(1), None, i32(0), words, places, places, i32(64), out]),  # a count without a list
        (lib.bgc_diag_regfile_data, run + dump + [None, i32(0), None, i32(1), words, places, places, i32(64), out]),
        (lib.bgc_diag_regfile_data, run + dump + [zeros, i32(-1), None, i32(0), words, places, places, i32(64), out]),
        (lib.bgc_diag_regfile_layout, [None]),
        (lib.bgc_diag_regfile_expected, [u32(SEED), i32(0), i32(0), i32(SWEEPS), None, i32(0), None]),
        (lib.bgc_diag_regfile_expected, [u32(SEED), i32(0), i32(0), i32(SWEEPS), None, i32(1), words]),
        (lib.bgc_diag_regfile_expected, [u32(SEED), i32(0), i32(0), i32(SWEEPS), zeros, i32(-1), words]),
    ]
    for fn, args in calls:
        fn.restype = ctypes.c_int
        assert fn(*args) != 0, fn.__name__
        assert lib.bgc_diag_last_error().decode() == "invalid arguments", (fn.__name__, lib.bgc_diag_last_error())
    assert words.raw == bytes(512 * 64 * 4)  # nothing was written


def test_abi_version_and_constants():
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    assert lib.bgc_diag_abi_version() == 15
    from bacchus_gpu_controller_amd import ops

    assert (ops.REGFILE_WGS_PER_CU, ops.REGFILE_SWEEPS) == (2, 4096)
    assert ops.REGFILE_PLANT_REGS == (0, 5, 128, 250, 255, 256, 384, 511) and len(ops.REGFILE_PHASES) == 5
    assert ops.REGFILE_LAYOUT.itemsize == 20 + 1024 + 64 + 2048 + 32 + 40  # bgc_regfile_layout
