"""The atomic diagnostic's entries (bgc_diag_atomic, its planted, delayed and generated-data variants, and the host
referee's bgc_diag_atomic_layout, _expected and _rate_expected) refuse every out-of-range argument with "invalid
arguments" on the host, before the first HIP call: the sizes decide what the kernels address, and a plant names a
wave, a round, a lane and a word that a kernel thread compares its own with.  Because the refusal comes first, these
run without a GPU (with one, a valid call would succeed; without, it would fail with a HIP error instead)."""
import ctypes

import pytest

SEED = 0x5EED
MAX_PLANTS = 4096  # BGC_DIAG_MAX_PLANTS
MAX_DELAY_TICKS = 10_000_000  # BGC_DIAG_MAX_DELAY_TICKS
MAX_DATA_BYTES = 128 << 20  # BGC_DIAG_MAX_DATA_BYTES
CLASS_OPS = (6, 1, 1, 1, 2, 1, 1, 9)
OK_PLANT = (0, 0, 0, 0, 0, 0, 0, 0)  # placement, class, word, wave, round, lane, times, mask: a lost update
OK_RATE = (0, 0, 0, 0)  # rate class, wave, lane, times
OK_DELAY = (0, 0, 1)  # rate class, wave, ticks
WGS, ROUNDS, ITERS = 1, 2, 15


def _refused(call, *args):
    with pytest.raises(RuntimeError) as e:
        call(*args)
    assert str(e.value) == "atomic diag: invalid arguments"


SIZES = {
    "wgs_per_cu_0": (0, 2, 15), "wgs_per_cu_9": (9, 2, 15), "wgs_per_cu_-1": (-1, 2, 15),
    "rounds_0": (1, 0, 15), "rounds_65": (1, 65, 15), "rounds_-1": (1, -1, 15),
    "rate_iters_0": (1, 2, 0), "rate_iters_-1": (1, 2, -1), "rate_iters_over_2^16": (1, 2, (1 << 16) + 1),
}


@pytest.mark.parametrize("sizes", SIZES.values(), ids=SIZES.keys())
def test_atomic_sizes_out_of_range(nat, sizes):
    wgs, rounds, iters = sizes
    _refused(nat.diag_atomic, 0, wgs, rounds, iters, SEED)
    _refused(nat.diag_atomic_planted, 0, wgs, rounds, iters, SEED, [], [])
    _refused(nat.diag_atomic_delayed, 0, wgs, rounds, iters, SEED, [])
    _refused(nat.diag_atomic_delayed, 0, wgs, rounds, iters, SEED, [OK_DELAY])
    _refused(nat.diag_atomic_data, 0, wgs, rounds, iters, SEED, [], [], [])


PLANTS = {
    "placement_2": (2, 0, 0, 0, 0, 0, 0, 0), "placement_-1": (-1, 0, 0, 0, 0, 0, 0, 0),
    "class_8": (0, 8, 0, 0, 0, 0, 0, 0), "class_-1": (0, -1, 0, 0, 0, 0, 0, 0), "lds_in_shared": (1, 7, 0, 0, 0, 0, 0, 0),
    "word_-1": (0, 0, -1, 0, 0, 0, 0, 0), "wave_-1": (0, 0, 0, -1, 0, 0, 0, 0), "wave_-2": (0, 0, 0, -2, 0, 0, 0, 0),
    "round_at_rounds": (0, 0, 0, 0, ROUNDS, 0, 0, 0), "round_-1": (0, 0, 0, 0, -1, 0, 0, 0),
    "lane_64": (0, 0, 0, 0, 0, 64, 0, 0), "lane_-1": (0, 0, 0, 0, 0, -1, 0, 0),
    "times_3": (0, 0, 0, 0, 0, 0, 3, 1), "times_-1": (0, 0, 0, 0, 0, 0, -1, 1), "times_1_mask_0": (1, 6, 0, 0, 1, 63, 1, 0),
    **{f"word_past_class_{c}": (0, c, n, 0, 0, 0, 0, 0) for c, n in enumerate(CLASS_OPS)},
}


@pytest.mark.parametrize("plant", PLANTS.values(), ids=PLANTS.keys())
def test_plant_out_of_range(nat, plant):
    _refused(nat.diag_atomic_planted, 0, WGS, ROUNDS, ITERS, SEED, [plant], [])
    _refused(nat.diag_atomic_planted, 0, WGS, ROUNDS, ITERS, SEED, [OK_PLANT, plant], [])  # not only the first one is checked
    _refused(nat.diag_atomic_planted, 0, WGS, ROUNDS, ITERS, SEED, [plant], [OK_RATE])
    _refused(nat.diag_atomic_data, 0, WGS, ROUNDS, ITERS, SEED, [OK_PLANT, plant], [], [])
    _refused(nat.diag_atomic_expected, SEED, 4, ROUNDS, [OK_PLANT, plant])


RATE_PLANTS = {
    "class_4": (4, 0, 0, 0), "class_-1": (-1, 0, 0, 0), "wave_-1": (0, -1, 0, 0), "lane_64": (0, 0, 64, 0), "lane_-1": (0, 0, -1, 0),
    "rtn_lane_1": (3, 0, 1, 0), "times_1": (0, 0, 0, 1), "times_3": (0, 0, 0, 3), "times_-1": (2, 0, 63, -1),
}


@pytest.mark.parametrize("plant", RATE_PLANTS.values(), ids=RATE_PLANTS.keys())
def test_rate_plant_out_of_range(nat, plant):
    _refused(nat.diag_atomic_planted, 0, WGS, ROUNDS, ITERS, SEED, [], [plant])
    _refused(nat.diag_atomic_planted, 0, WGS, ROUNDS, ITERS, SEED, [], [OK_RATE, plant])
    _refused(nat.diag_atomic_planted, 0, WGS, ROUNDS, ITERS, SEED, [OK_PLANT], [plant])
    _refused(nat.diag_atomic_data, 0, WGS, ROUNDS, ITERS, SEED, [], [OK_RATE, plant], [])


DELAYS = {
    "ticks_0": (0, 0, 0), "ticks_over_max": (0, 0, MAX_DELAY_TICKS + 1), "all_ticks_0": (0, -1, 0), "wave_-2": (0, -2, 1),
    "class_4": (4, 0, 1), "class_-1": (-1, 0, 1),
}


@pytest.mark.parametrize("delay", DELAYS.values(), ids=DELAYS.keys())
def test_delay_out_of_range(nat, delay):
    _refused(nat.diag_atomic_delayed, 0, WGS, ROUNDS, ITERS, SEED, [delay])
    _refused(nat.diag_atomic_delayed, 0, WGS, ROUNDS, ITERS, SEED, [OK_DELAY, delay])
    _refused(nat.diag_atomic_data, 0, WGS, ROUNDS, ITERS, SEED, [], [], [OK_DELAY, delay])


def test_plant_lists_too_long(nat):
    _refused(nat.diag_atomic_planted, 0, WGS, ROUNDS, ITERS, SEED, [OK_PLANT] * (MAX_PLANTS + 1), [])
    _refused(nat.diag_atomic_planted, 0, WGS, ROUNDS, ITERS, SEED, [], [OK_RATE] * (MAX_PLANTS + 1))
    _refused(nat.diag_atomic_delayed, 0, WGS, ROUNDS, ITERS, SEED, [OK_DELAY] * (MAX_PLANTS + 1))
    _refused(nat.diag_atomic_data, 0, WGS, ROUNDS, ITERS, SEED, [OK_PLANT] * (MAX_PLANTS + 1), [], [])
    _refused(nat.diag_atomic_data, 0, WGS, ROUNDS, ITERS, SEED, [], [OK_RATE] * (MAX_PLANTS + 1), [])
    _refused(nat.diag_atomic_data, 0, WGS, ROUNDS, ITERS, SEED, [], [], [OK_DELAY] * (MAX_PLANTS + 1))
    _refused(nat.diag_atomic_expected, SEED, 4, ROUNDS, [OK_PLANT] * (MAX_PLANTS + 1))


LAYOUTS = {"grid_0": (0, 8, 2), "grid_-1": (-1, 8, 2), "grid_over_16384": (16385, 8, 2), "rate_grid_0": (4, 0, 2), "rate_grid_12": (4, 12, 2),
           "rate_grid_over_4096": (4, 4104, 2), "rounds_0": (4, 8, 0), "rounds_65": (4, 8, 65)}


@pytest.mark.parametrize("layout", LAYOUTS.values(), ids=LAYOUTS.keys())
def test_layout_and_expected_sizes_out_of_range(nat, layout):
    grid, rate_grid, rounds = layout
    _refused(nat.diag_atomic_layout, grid, rate_grid, rounds)
    if rate_grid == 8:
        _refused(nat.diag_atomic_expected, SEED, grid, rounds, [])


def test_expected_refuses_a_plant_beyond_the_grid_and_data_beyond_the_cap(nat):
    with pytest.raises(RuntimeError) as e:
        nat.diag_atomic_expected(SEED, 4, ROUNDS, [(0, 0, 0, 16, 0, 0, 0, 0)])  # 4 workgroups have waves 0..15
    assert str(e.value) == "atomic diag: invalid arguments: plant in a wave beyond the launch"
    with pytest.raises(RuntimeError) as e:
        nat.diag_atomic_expected(SEED, 2048, 64, [])  # 400 MB of tables and order arrays
    assert str(e.value) == "atomic diag: invalid arguments: the data exceed the capacity"


RATE_EXPECTED = {"rate_grid_0": (0, 15, 0), "rate_grid_12": (12, 15, 0), "rate_grid_over_4096": (4104, 15, 0), "iters_0": (8, 0, 0),
                 "iters_over_2^16": (8, (1 << 16) + 1, 0), "class_4": (8, 15, 4), "class_-1": (8, 15, -1)}


@pytest.mark.parametrize("args", RATE_EXPECTED.values(), ids=RATE_EXPECTED.keys())
def test_rate_expected_out_of_range(nat, args):
    _refused(nat.diag_atomic_rate_expected, SEED, *args)


def test_atomic_null_pointers_negative_counts_and_capacity():
    """The bindings always pass buffers and a list's own length, so these go to the C ABI directly."""
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    lib.bgc_diag_last_error.restype = ctypes.c_char_p
    out = ctypes.create_string_buffer(4096)  # larger than the result struct and the layout
    zeros = ctypes.create_string_buffer(4096)  # plants with times 1 and mask 0, or ticks 0, were they ever looked at
    u32, i32, u64 = ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64
    run = [i32(0), i32(WGS), i32(ROUNDS), i32(ITERS), u32(SEED)]
    no_lists = [None, i32(0), None, i32(0), None, i32(0)]
    calls = [
        (lib.bgc_diag_atomic, run + [None]),
        (lib.bgc_diag_atomic_planted, run + [None, i32(0), None, i32(0), None]),
        (lib.bgc_diag_atomic_planted, run + [zeros, i32(-1), None, i32(0), out]),
        (lib.bgc_diag_atomic_planted, run + [None, i32(0), zeros, i32(-1), out]),
        (lib.bgc_diag_atomic_planted, run + [None, i32(1), None, i32(0), out]),  # a count without a list
        (lib.bgc_diag_atomic_planted, run + [None, i32(0), None, i32(1), out]),
        (lib.bgc_diag_atomic_delayed, run + [None, i32(0), None]),
        (lib.bgc_diag_atomic_delayed, run + [zeros, i32(-1), out]),
        (lib.bgc_diag_atomic_delayed, run + [None, i32(1), out]),
        (lib.bgc_diag_atomic_data, run + no_lists + [None, u64(4096), out]),  # no destination
        (lib.bgc_diag_atomic_data, run + no_lists + [zeros, u64(4096), None]),
        (lib.bgc_diag_atomic_data, run + no_lists + [zeros, u64(MAX_DATA_BYTES + 1), out]),  # more than the cap
        (lib.bgc_diag_atomic_data, run + [zeros, i32(-1), None, i32(0), None, i32(0), zeros, u64(4096), out]),
        (lib.bgc_diag_atomic_data, run + [None, i32(0), None, i32(1), None, i32(0), zeros, u64(4096), out]),  # a count without a list
        (lib.bgc_diag_atomic_data, run + [None, i32(0), None, i32(0), zeros, i32(-1), zeros, u64(4096), out]),
        (lib.bgc_diag_atomic_layout, [i32(4), i32(8), i32(2), None]),
        (lib.bgc_diag_atomic_expected, [u32(SEED), i32(4), i32(2), None, i32(0), None, u64(1 << 20)]),
        (lib.bgc_diag_atomic_expected, [u32(SEED), i32(4), i32(2), None, i32(1), zeros, u64(1 << 20)]),
        (lib.bgc_diag_atomic_expected, [u32(SEED), i32(4), i32(2), None, i32(0), zeros, u64(MAX_DATA_BYTES + 1)]),
        (lib.bgc_diag_atomic_rate_expected, [u32(SEED), i32(8), i32(15), i32(0), None, u64(1 << 20)]),
        (lib.bgc_diag_atomic_rate_expected, [u32(SEED), i32(8), i32(15), i32(0), zeros, u64(4 * 4096 - 1)]),  # one word short
    ]
    for fn, args in calls:
        fn.restype = ctypes.c_int
        assert fn(*args) != 0, fn.__name__
        assert lib.bgc_diag_last_error().decode() == "invalid arguments", (fn.__name__, lib.bgc_diag_last_error())
    # a destination smaller than the referee's tables is refused with its own text, and nothing is written
    assert lib.bgc_diag_atomic_expected(u32(SEED), i32(4), i32(2), None, i32(0), zeros, u64(4096)) != 0
    assert lib.bgc_diag_last_error().decode() == "invalid arguments: the data exceed the capacity"
    assert zeros.raw == bytes(4096)


def test_abi_version_and_class_tables():
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    assert lib.bgc_diag_abi_version() == 15
    from bacchus_gpu_controller_amd import ops

    assert len(ops.ATOMIC_CLASSES) == 8 and ops.ATOMIC_CLASS_OPS == CLASS_OPS and len(ops.ATOMIC_RATE_CLASSES) == 4
    assert len(ops.ATOMIC_INT_WORDS) == 6 and len(ops.ATOMIC_LDS_WORDS) == 9
    assert ops.ATOMIC_LAYOUT.itemsize == 16 + 4 + 64 + 12 + 128 + 64 + 64 + 8  # bgc_atomic_layout
    assert (ops.ATOMIC_WGS_PER_CU, ops.ATOMIC_ROUNDS, ops.ATOMIC_RATE_ITERS) == (2, 8, 4095)
