"""The cache diagnostic's four entries (bgc_diag_cache, its planted, delayed and generated-data
variants) refuse every out-of-range argument with "invalid arguments" on the host, before the first
HIP call: a plant names a word of a buffer that a kernel thread or a host copy then writes, and the
sizes decide what the kernels address, so none of them may reach the device out of range.  Because
the refusal comes first, these run without a GPU (with one, a valid call would succeed; without, it
would fail with a HIP error instead)."""
import ctypes

import pytest

SEED = 0x5EED
KIB, MIB = 1 << 10, 1 << 20
REGION = 96 * KIB
REGION_WORDS = REGION // 4
IC = 2 * MIB
MAX_PLANTS = 4096  # BGC_DIAG_MAX_PLANTS
MAX_DELAY_TICKS = 10_000_000  # BGC_DIAG_MAX_DELAY_TICKS
MAX_DATA_BYTES = 128 * MIB  # BGC_DIAG_MAX_DATA_BYTES
OK_L2 = (0, 0, 0, 0, 1)  # round, wg, pass, word, mask
OK_IC = (0, 0, 1)  # when, word, mask
OK_DELAY = (0, 1)  # wg, ticks


def _refused(call, *args):
    with pytest.raises(RuntimeError) as e:
        call(*args)
    assert str(e.value) == "cache diag: invalid arguments"


SIZES = {
    "rounds_0": (0, REGION, 16, IC, 2), "rounds_17": (17, REGION, 16, IC, 2), "rounds_-1": (-1, REGION, 16, IC, 2),
    "region_0": (1, 0, 16, IC, 2), "region_48K": (1, 48 * KIB, 16, IC, 2), "region_160K": (1, 160 * KIB, 16, IC, 2),
    "region_32K+16": (1, 32 * KIB + 16, 16, IC, 2),
    "l2_sweeps_0": (1, REGION, 0, IC, 2), "l2_sweeps_-1": (1, REGION, -1, IC, 2), "l2_sweeps_over_2^16": (1, REGION, (1 << 16) + 1, IC, 2),
    "ic_sweeps_0": (1, REGION, 16, IC, 0), "ic_sweeps_-1": (1, REGION, 16, IC, -1), "ic_sweeps_4097": (1, REGION, 16, IC, 4097),
    "ic_sweeps_0_phase_off": (1, REGION, 16, 0, 0),
    "ic_bytes_1MiB+16": (1, REGION, 16, MIB + 16, 2), "ic_bytes_512KiB": (1, REGION, 16, MIB // 2, 2),
    "ic_bytes_1GiB+1MiB": (1, REGION, 16, (1 << 30) + MIB, 2), "ic_bytes_2^40": (1, REGION, 16, 1 << 40, 2),
}


@pytest.mark.parametrize("sizes", SIZES.values(), ids=SIZES.keys())
def test_cache_sizes_out_of_range(nat, sizes):
    rounds, region, l2_sweeps, ic_bytes, ic_sweeps = sizes
    _refused(nat.diag_cache, 0, rounds, region, l2_sweeps, ic_bytes, ic_sweeps, SEED)
    _refused(nat.diag_cache_planted, 0, rounds, region, l2_sweeps, ic_bytes, ic_sweeps, SEED, [], [])
    _refused(nat.diag_cache_delayed, 0, rounds, region, l2_sweeps, ic_bytes, ic_sweeps, SEED, [])
    _refused(nat.diag_cache_delayed, 0, rounds, region, l2_sweeps, ic_bytes, ic_sweeps, SEED, [OK_DELAY])
    _refused(nat.diag_cache_data, 0, rounds, region, 2, l2_sweeps, ic_bytes, ic_sweeps, SEED)


L2_PLANTS = {
    "pass_2": (0, 0, 2, 0, 1), "pass_-1": (0, 0, -1, 0, 1), "word_at_region_words": (0, 0, 0, REGION_WORDS, 1),
    "word_u32_max": (0, 0, 0, (1 << 32) - 1, 1), "mask_0": (0, 0, 0, 0, 0), "all_wgs_mask_0": (0, -1, 1, REGION_WORDS - 1, 0),
    "wg_-2": (0, -2, 0, 0, 1), "round_at_rounds": (2, 0, 0, 0, 1), "round_-1": (-1, 0, 0, 0, 1),
}


@pytest.mark.parametrize("plant", L2_PLANTS.values(), ids=L2_PLANTS.keys())
def test_l2_plant_out_of_range(nat, plant):
    _refused(nat.diag_cache_planted, 0, 2, REGION, 16, IC, 2, SEED, [plant], [])
    _refused(nat.diag_cache_planted, 0, 2, REGION, 16, IC, 2, SEED, [OK_L2, plant], [])  # not only the first one is checked
    _refused(nat.diag_cache_planted, 0, 2, REGION, 16, IC, 2, SEED, [plant], [OK_IC])


def test_l2_plant_word_is_checked_against_the_region_of_the_call(nat):
    """word 8192 is the first outside a 32 KiB region and well inside a 96 KiB one"""
    _refused(nat.diag_cache_planted, 0, 1, 32 * KIB, 16, IC, 2, SEED, [(0, 0, 0, 8192, 1)], [])


IC_PLANTS = {
    "when_2": (2, 0, 1), "when_-1": (-1, 0, 1), "word_at_ic_words": (0, IC // 4, 1), "word_2^40": (1, 1 << 40, 1), "mask_0": (0, 0, 0),
}


@pytest.mark.parametrize("plant", IC_PLANTS.values(), ids=IC_PLANTS.keys())
def test_ic_plant_out_of_range(nat, plant):
    _refused(nat.diag_cache_planted, 0, 1, REGION, 16, IC, 2, SEED, [], [plant])
    _refused(nat.diag_cache_planted, 0, 1, REGION, 16, IC, 2, SEED, [], [OK_IC, plant])
    _refused(nat.diag_cache_planted, 0, 1, REGION, 16, IC, 2, SEED, [OK_L2], [plant])


def test_ic_plant_without_an_ic_phase(nat):
    _refused(nat.diag_cache_planted, 0, 1, REGION, 16, 0, 2, SEED, [], [OK_IC])


def test_plant_lists_too_long(nat):
    _refused(nat.diag_cache_planted, 0, 1, REGION, 16, IC, 2, SEED, [OK_L2] * (MAX_PLANTS + 1), [])
    _refused(nat.diag_cache_planted, 0, 1, REGION, 16, IC, 2, SEED, [], [OK_IC] * (MAX_PLANTS + 1))
    _refused(nat.diag_cache_delayed, 0, 1, REGION, 16, IC, 2, SEED, [OK_DELAY] * (MAX_PLANTS + 1))


@pytest.mark.parametrize("delay", [(0, 0), (0, MAX_DELAY_TICKS + 1), (-1, 0), (-2, 1)], ids=["ticks_0", "ticks_over_max", "all_ticks_0", "wg_-2"])
def test_delay_out_of_range(nat, delay):
    _refused(nat.diag_cache_delayed, 0, 1, REGION, 16, IC, 2, SEED, [delay])
    _refused(nat.diag_cache_delayed, 0, 1, REGION, 16, IC, 2, SEED, [OK_DELAY, delay])


@pytest.mark.parametrize("passes", [0, 3, -1])
def test_data_passes_out_of_range(nat, passes):
    _refused(nat.diag_cache_data, 0, 1, REGION, passes, 16, IC, 2, SEED)


@pytest.mark.parametrize("region,ic_bytes", [(REGION, MAX_DATA_BYTES), (128 * KIB, MAX_DATA_BYTES - 63 * MIB), (32 * KIB, 1 << 30)],
                         ids=["ic_alone_at_the_cap", "both_1MiB_over", "ic_1GiB"])
def test_data_request_over_the_cap(nat, region, ic_bytes):
    """the destination of the L2 buffer (that of 512 CUs) and the Infinity-Cache buffer together exceed 128 MiB"""
    _refused(nat.diag_cache_data, 0, 1, region, 2, 16, ic_bytes, 2, SEED)


def test_cache_null_pointers_and_negative_counts():
    """The bindings always pass buffers and a list's own length, so these go to the C ABI directly."""
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    lib.bgc_diag_last_error.restype = ctypes.c_char_p
    out = ctypes.create_string_buffer(4096)  # larger than the result struct
    zeros = ctypes.create_string_buffer(4096)  # plants with mask 0 or ticks 0, were they ever looked at
    data = ctypes.create_string_buffer(64)  # never written: every call below is refused
    u32, u64, i32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    run = [i32(0), i32(1), u32(REGION), i32(16), u64(IC), i32(2), u32(SEED)]
    data_run = [i32(0), i32(1), u32(REGION), i32(2), i32(16), u64(IC), i32(2), u32(SEED)]
    calls = [
        (lib.bgc_diag_cache, run + [None]),
        (lib.bgc_diag_cache_planted, run + [None, i32(0), None, i32(0), None]),
        (lib.bgc_diag_cache_planted, run + [zeros, i32(-1), None, i32(0), out]),
        (lib.bgc_diag_cache_planted, run + [None, i32(0), zeros, i32(-1), out]),
        (lib.bgc_diag_cache_planted, run + [None, i32(1), None, i32(0), out]),  # a count without a list
        (lib.bgc_diag_cache_planted, run + [None, i32(0), None, i32(1), out]),
        (lib.bgc_diag_cache_delayed, run + [None, i32(0), None]),
        (lib.bgc_diag_cache_delayed, run + [zeros, i32(-1), out]),
        (lib.bgc_diag_cache_delayed, run + [None, i32(1), out]),
        (lib.bgc_diag_cache_data, data_run + [None, u64(64 * MIB), data, out]),
        (lib.bgc_diag_cache_data, data_run + [data, u64(64 * MIB), None, out]),  # an Infinity-Cache phase without a destination
        (lib.bgc_diag_cache_data, data_run + [data, u64(64 * MIB), data, None]),
        (lib.bgc_diag_cache_data, data_run + [data, u64(MAX_DATA_BYTES), data, out]),  # with ic_bytes, over the cap
        (lib.bgc_diag_cache_data, data_run + [data, u64((1 << 64) - IC), data, out]),  # a capacity that wraps the sum
    ]
    for fn, args in calls:
        fn.restype = ctypes.c_int
        assert fn(*args) != 0, fn.__name__
        assert lib.bgc_diag_last_error().decode() == "invalid arguments", (fn.__name__, lib.bgc_diag_last_error())


def test_abi_version_and_region_size():
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    assert lib.bgc_diag_abi_version() == 15
    from bacchus_gpu_controller_amd import ops

    assert ops.L2_REGION_BYTES == 96 << 10 and ops.L2_REGION_BYTES % ops.L2_SLAB_BYTES == 0
