"""The LDS diagnostic's three entries (bgc_diag_lds, its planted variant and its generated-data
variant) refuse every out-of-range argument with "invalid arguments" on the host, before the first
HIP call: a plant names a word of the LDS array that a kernel thread then writes, so a word outside
the array must never reach the device.  Because the refusal comes first, these run without a GPU
(with one, a valid call would succeed; without, it would fail with a HIP error instead)."""
import ctypes

import pytest

SEED = 0x5EED
LDS_WORDS = 40960
OK_PLANT = (0, 0, 0, 1)
MAX_PLANTS = 4096  # BGC_DIAG_MAX_PLANTS


def _refused(call, *args):
    with pytest.raises(RuntimeError) as e:
        call(*args)
    assert str(e.value) == "lds diag: invalid arguments"


@pytest.mark.parametrize("wgs_per_cu,rate_iters", [(0, 64), (65, 64), (-1, 64), (1, 0), (1, -1), (1, (1 << 16) + 1)],
                         ids=["wgs_0", "wgs_65", "wgs_-1", "iters_0", "iters_-1", "iters_over_2^16"])
def test_lds_sizes_out_of_range(nat, wgs_per_cu, rate_iters):
    _refused(nat.diag_lds, 0, wgs_per_cu, rate_iters, SEED)
    _refused(nat.diag_lds_planted, 0, wgs_per_cu, rate_iters, SEED, [])
    _refused(nat.diag_lds_planted, 0, wgs_per_cu, rate_iters, SEED, [OK_PLANT])


@pytest.mark.parametrize("plant", [(-2, 0, 0, 1), (0, 2, 0, 1), (0, -1, 0, 1), (0, 0, LDS_WORDS, 1), (0, 0, (1 << 32) - 1, 1),
                                   (0, 0, 0, 0), (-1, 1, LDS_WORDS - 1, 0)],
                         ids=["wg_-2", "pass_2", "pass_-1", "word_40960", "word_u32_max", "mask_0", "all_wgs_mask_0"])
def test_lds_plant_out_of_range(nat, plant):
    _refused(nat.diag_lds_planted, 0, 1, 64, SEED, [plant])
    _refused(nat.diag_lds_planted, 0, 1, 64, SEED, [OK_PLANT, plant])  # not only the first one is checked


def test_lds_plant_list_too_long(nat):
    _refused(nat.diag_lds_planted, 0, 1, 64, SEED, [OK_PLANT] * (MAX_PLANTS + 1))


@pytest.mark.parametrize("wg,pass_,grid", [(-1, 0, 3), (3, 0, 3), (0, 2, 3), (0, -1, 3), (0, 0, 0), (0, 0, 4097), (0, 0, -1)],
                         ids=["wg_-1", "wg_at_grid", "pass_2", "pass_-1", "grid_0", "grid_4097", "grid_-1"])
def test_lds_data_out_of_range(nat, wg, pass_, grid):
    _refused(nat.diag_lds_data, 0, SEED, wg, pass_, grid)


def test_lds_null_pointers_and_negative_count():
    """The bindings always pass buffers and a list's own length, so these go to the C ABI directly."""
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    lib.bgc_diag_last_error.restype = ctypes.c_char_p
    out = ctypes.create_string_buffer(4096)  # larger than the result struct
    plants = ctypes.create_string_buffer(4096)  # zeroes: a plant with mask 0, were it ever looked at
    u32, i32 = ctypes.c_uint32, ctypes.c_int
    calls = [
        (lib.bgc_diag_lds, [i32(0), i32(1), i32(64), u32(SEED), None]),
        (lib.bgc_diag_lds_planted, [i32(0), i32(1), i32(64), u32(SEED), None, i32(0), None]),
        (lib.bgc_diag_lds_planted, [i32(0), i32(1), i32(64), u32(SEED), plants, i32(-1), out]),
        (lib.bgc_diag_lds_planted, [i32(0), i32(1), i32(64), u32(SEED), None, i32(1), out]),  # a count without a list
        (lib.bgc_diag_lds_data, [i32(0), u32(SEED), i32(0), i32(0), i32(3), None]),
    ]
    for fn, args in calls:
        fn.restype = ctypes.c_int
        assert fn(*args) != 0, fn.__name__
        assert lib.bgc_diag_last_error().decode() == "invalid arguments", (fn.__name__, lib.bgc_diag_last_error())


def test_abi_version_and_array_size():
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    assert lib.bgc_diag_abi_version() == 15
    from bacchus_gpu_controller_amd import ops

    assert ops.LDS_WORDS == LDS_WORDS and ops.LDS_WORDS * 4 == 160 * 1024
