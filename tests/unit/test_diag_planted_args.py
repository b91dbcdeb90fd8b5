"""The planted variants of the GPU diagnostics (tests/gpu/test_diag_detection.py) write into device
memory and accumulators at positions a test names, so a position outside the buffer, or a wave,
lane, round, chain or element index out of range, must be refused on the host before the GPU is
touched: an out-of-range plant can never become an out-of-bounds write.  The refusal comes before
the first HIP call, which is why these run without a GPU (with one, a valid call would succeed;
without, it would fail with a HIP error, not with "invalid arguments")."""
import ctypes

import pytest

MIB = 1 << 20
SEED = 0x5EED
OK_ACC = (0, 0, 0, 0, 1.0)


def _refused(call, *args):
    with pytest.raises((RuntimeError, ValueError), match="invalid arguments"):
        call(*args)


def test_hbm_plant_outside_the_buffer(nat):
    words = MIB // 4
    _refused(nat.diag_hbm_planted, 0, MIB, SEED, [(words, 1)])
    _refused(nat.diag_hbm_planted, 0, MIB, SEED, [(0, 1), (1 << 40, 1)])
    # the buffer is rounded down to 16 bytes: the last three words of MIB + 12 do not exist
    _refused(nat.diag_hbm_planted, 0, MIB + 12, SEED, [(words, 1)])


def test_pcie_plant_outside_the_buffer(nat):
    _refused(nat.diag_pcie_planted, 0, MIB, SEED, [(MIB // 8, 1)])
    _refused(nat.diag_pcie_planted, 0, MIB, SEED, [(0, 1), ((1 << 64) - 1, 1)])


def test_walk_plant_outside_its_chunk(nat):
    chunk = 64 * MIB
    target = 3 * chunk + 2 * MIB  # four chunks, the last of 2 MiB
    _refused(nat.diag_hbm_walk_planted, 0, target, chunk, SEED, [(0, 4, 0, 1)])  # a fifth chunk
    _refused(nat.diag_hbm_walk_planted, 0, target, chunk, SEED, [(0, -1, 0, 1)])
    _refused(nat.diag_hbm_walk_planted, 0, target, chunk, SEED, [(0, 0, chunk // 8, 1)])
    _refused(nat.diag_hbm_walk_planted, 0, target, chunk, SEED, [(0, 3, 2 * MIB // 8, 1)])  # past the short last chunk
    _refused(nat.diag_hbm_walk_planted, 0, target, chunk, SEED, [(2, 0, 0, 1)])  # there are two passes
    _refused(nat.diag_hbm_walk_planted, 0, target, chunk - 1, SEED, [])  # chunks of at least 64 MiB
    _refused(nat.diag_hbm_walk_planted, 0, MIB, chunk, SEED, [])  # nothing left after rounding to 2 MiB


@pytest.mark.parametrize("plant", [(0, 0, 64, 0, 1.0), (0, 0, -1, 0, 1.0), (0, 0, 0, 4, 1.0), (0, 0, 0, -1, 1.0),
                                   (0, 8, 0, 0, 1.0), (0, -1, 0, 0, 1.0), (-2, 0, 0, 0, 1.0)],
                         ids=["lane_64", "lane_-1", "i_4", "i_-1", "round_8", "round_-1", "wave_-2"])
def test_mfma_check_plant_out_of_range(nat, plant):
    _refused(nat.diag_mfma_planted, 0, 1, 64, SEED, [OK_ACC, plant], [])


@pytest.mark.parametrize("plant", [(0, 64, 0, 0, 1.0), (0, 0, 4, 0, 1.0), (0, 0, -1, 0, 1.0), (0, 0, 0, 4, 1.0),
                                   (-1, 0, 0, 0, 1.0)],
                         ids=["lane_64", "chain_4", "chain_-1", "i_4", "wave_-1"])
def test_mfma_rate_plant_out_of_range(nat, plant):
    _refused(nat.diag_mfma_planted, 0, 1, 64, SEED, [], [OK_ACC, plant])


@pytest.mark.parametrize("plant", [(0, 0, 0, 64, 0, 1.0), (0, 0, 0, 0, 4, 1.0), (0, 0, 2, 0, 0, 1.0), (4, 0, 0, 0, 0, 1.0),
                                   (-1, 0, 0, 0, 0, 1.0)],
                         ids=["lane_64", "i_4", "round_2", "variant_4", "variant_-1"])
def test_lowp_check_plant_out_of_range(nat, plant):
    _refused(nat.diag_mfma_lowp_planted, 0, 1, 64, SEED, [(3,) + OK_ACC, plant], [])


@pytest.mark.parametrize("plant", [(0, 0, 64, 0, 0, 1.0), (0, 0, 0, 4, 0, 1.0), (0, 0, 0, 0, 4, 1.0), (2, 0, 0, 0, 0, 1.0)],
                         ids=["lane_64", "chain_4", "i_4", "format_2"])
def test_lowp_rate_plant_out_of_range(nat, plant):
    _refused(nat.diag_mfma_lowp_planted, 0, 1, 64, SEED, [], [(1,) + OK_ACC, plant])


@pytest.mark.parametrize("launches,plant", [(1, (0, 256, 0, 1.0)), (1, (0, -1, 0, 1.0)), (1, (0, 0, 512, 1.0)), (1, (0, 0, -1, 1.0)),
                                            (3, (1, 0, 0, 1.0)), (2, (2, 0, 0, 1.0)), (2, (-1, 0, 0, 1.0))],
                         ids=["row_m", "row_-1", "col_n", "col_-1", "launch_1_of_3", "launch_2_of_2", "launch_-1"])
def test_soak_plant_outside_the_matrix_or_on_an_unverified_launch(nat, launches, plant):
    _refused(nat.diag_gemm_soak_planted, 0, 256, 512, 128, launches, SEED, [(0, 0, 0, 1.0), plant])


MAX_DELAY_TICKS = 10_000_000  # BGC_DIAG_MAX_DELAY_TICKS: 100 ms of the 100 MHz constant clock


@pytest.mark.parametrize("delay", [(-2, 1000), (0, 0), (-1, 0), (0, MAX_DELAY_TICKS + 1), (-1, (1 << 32) - 1)],
                         ids=["wave_-2", "ticks_0", "all_waves_ticks_0", "ticks_over_the_cap", "ticks_u32_max"])
def test_mfma_delay_plant_out_of_range(nat, delay):
    """A delay plant makes a wave wait in a loop on the clock, so the wait's length is bounded on the
    host: 100 ms at most, and never 0 (a plant that does nothing is a mistake in the test)."""
    _refused(nat.diag_mfma_delayed, 0, 1, 64, SEED, [(0, MAX_DELAY_TICKS), delay])


def test_mfma_delay_plant_list_too_long(nat):
    _refused(nat.diag_mfma_delayed, 0, 1, 64, SEED, [(0, 1000)] * 4097)  # BGC_DIAG_MAX_PLANTS is 4096


@pytest.mark.parametrize("first,ticks,dtype", [(-1, 1000, "bf16"), (0, 0, "bf16"), (0, MAX_DELAY_TICKS + 1, "fp8"),
                                               (1 << 30, (1 << 32) - 1, "fp4")],
                         ids=["first_launch_-1", "ticks_0", "ticks_over_the_cap", "ticks_u32_max"])
def test_burn_delay_out_of_range(nat, first, ticks, dtype):
    _refused(nat.diag_burn_delayed, 0, 300, 32, SEED, dtype, first, ticks)


@pytest.mark.parametrize("duration_ms,waves_per_cu", [(0, 32), (600001, 32), (300, 0), (300, 65)],
                         ids=["duration_0", "duration_over_10_min", "waves_0", "waves_65"])
def test_burn_delayed_refuses_what_the_burn_refuses(nat, duration_ms, waves_per_cu):
    _refused(nat.diag_burn_delayed, 0, duration_ms, waves_per_cu, SEED, "bf16", 2, 1000)


OK_BURN = (0,) + OK_ACC  # (launch, wave, lane, chain, i, delta)


@pytest.mark.parametrize("plant", [(-1, 0, 0, 0, 0, 1.0), (0, -1, 0, 0, 0, 1.0), (0, 0, 64, 0, 0, 1.0), (0, 0, -1, 0, 0, 1.0),
                                   (2, 0, 0, 4, 0, 1.0), (2, 0, 0, -1, 0, 1.0), (1 << 30, 0, 0, 0, 4, 1.0), (0, 0, 0, 0, -1, 1.0)],
                         ids=["launch_-1", "wave_-1", "lane_64", "lane_-1", "chain_4", "chain_-1", "i_4", "i_-1"])
@pytest.mark.parametrize("dtype", ["bf16", "fp8", "fp4"])
def test_burn_plant_out_of_range(nat, dtype, plant):
    """A burn plant adds to an accumulator register of a named lane of a named launch: its place is
    checked like a rate plant's, and its launch may be any the burn could reach, but not negative."""
    _refused(nat.diag_burn_planted, 0, 300, 32, SEED, dtype, [OK_BURN, plant])


def test_burn_plant_list_too_long(nat):
    _refused(nat.diag_burn_planted, 0, 300, 32, SEED, "bf16", [OK_BURN] * 4097)  # BGC_DIAG_MAX_PLANTS is 4096


@pytest.mark.parametrize("duration_ms,waves_per_cu", [(0, 32), (600001, 32), (300, 0), (300, 65)],
                         ids=["duration_0", "duration_over_10_min", "waves_0", "waves_65"])
@pytest.mark.parametrize("plants", [[], [OK_BURN]], ids=["no_plants", "one_plant"])
def test_burn_planted_refuses_what_the_burn_refuses(nat, plants, duration_ms, waves_per_cu):
    _refused(nat.diag_burn_planted, 0, duration_ms, waves_per_cu, SEED, "bf16", plants)


def test_generated_data_beyond_the_download_cap(nat):
    """The generated-data variants (tests/gpu/test_diag_generated_data.py) copy what a diagnostic
    generated back to the host: at most 128 MiB per call."""
    cap = 128 * MIB
    _refused(nat.diag_hbm_data, 0, cap + 16, 1, SEED)
    _refused(nat.diag_hbm_data, 0, 1 << 40, 1, SEED)
    _refused(nat.diag_hbm_data, 0, MIB, 0, SEED)  # and what bgc_diag_hbm refuses
    _refused(nat.diag_pcie_data, 0, cap + 8, SEED)
    _refused(nat.diag_pcie_data, 0, MIB - 8, SEED)
    _refused(nat.diag_hbm_walk_data, 0, cap + 2 * MIB, 64 * MIB, 1, SEED)
    _refused(nat.diag_hbm_walk_data, 0, MIB, 64 * MIB, 1, SEED)  # nothing left after rounding to 2 MiB
    _refused(nat.diag_hbm_walk_data, 0, 66 * MIB, 64 * MIB - 1, 1, SEED)
    _refused(nat.diag_hbm_walk_data, 0, 66 * MIB, 64 * MIB, 0, SEED)  # one or two passes
    _refused(nat.diag_hbm_walk_data, 0, 66 * MIB, 64 * MIB, 3, SEED)
    _refused(nat.diag_gemm_soak_data, 0, 4096, 4096, 4096, SEED)  # 128 MiB of operands and C, and the checksums
    _refused(nat.diag_gemm_soak_data, 0, 32768, 32768, 32768, SEED)
    _refused(nat.diag_gemm_soak_data, 0, 256, 200, 128, SEED)  # and what bgc_diag_gemm_soak refuses
    _refused(nat.diag_gemm_soak_data, 0, -256, 256, 128, SEED)


@pytest.mark.parametrize("path,scaled", [(3, 0), (-1, 0), (0, 1), (1, 2), (2, -1)],
                         ids=["path_3", "path_-1", "bf16_scaled", "scaled_2", "scaled_-1"])
def test_mfma_tile_path_or_scaling_out_of_range(nat, path, scaled):
    _refused(nat.diag_mfma_tile, 0, path, scaled, SEED, 0)


def test_generated_data_without_a_destination():
    """The bindings always pass buffers, so the null destinations go to the C ABI directly."""
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    lib.bgc_diag_last_error.restype = ctypes.c_char_p
    out = ctypes.create_string_buffer(4096)  # larger than any result struct
    room = ctypes.create_string_buffer(4096)
    u64, u32, i32, ptr = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p

    def soak_data(missing):
        return (ptr * 5)(*[None if i == missing else ctypes.addressof(room) for i in range(5)])

    calls = [
        (lib.bgc_diag_hbm_data, [i32(0), u64(MIB), i32(1), u32(SEED), None, out]),
        (lib.bgc_diag_hbm_data, [i32(0), u64(MIB), i32(1), u32(SEED), room, None]),
        (lib.bgc_diag_pcie_data, [i32(0), u64(MIB), u32(SEED), None, out]),
        (lib.bgc_diag_pcie_data, [i32(0), u64(MIB), u32(SEED), room, None]),
        (lib.bgc_diag_hbm_walk_data, [i32(0), u64(66 * MIB), u64(64 * MIB), i32(1), u32(SEED), room, i32(2), None, out]),
        (lib.bgc_diag_hbm_walk_data, [i32(0), u64(66 * MIB), u64(64 * MIB), i32(1), u32(SEED), None, i32(2), room, out]),
        (lib.bgc_diag_hbm_walk_data, [i32(0), u64(66 * MIB), u64(64 * MIB), i32(1), u32(SEED), room, i32(2), room, None]),
        # two chunks, room for one
        (lib.bgc_diag_hbm_walk_data, [i32(0), u64(66 * MIB), u64(64 * MIB), i32(1), u32(SEED), room, i32(1), room, out]),
        (lib.bgc_diag_gemm_soak_data, [i32(0), i32(256), i32(256), i32(128), u32(SEED), None, out]),
        (lib.bgc_diag_gemm_soak_data, [i32(0), i32(256), i32(256), i32(128), u32(SEED), soak_data(None), None]),
        *[(lib.bgc_diag_gemm_soak_data, [i32(0), i32(256), i32(256), i32(128), u32(SEED), soak_data(i), out]) for i in range(5)],
        (lib.bgc_diag_mfma_tile, [i32(0), i32(0), i32(0), u32(SEED), u32(0), None]),
    ]
    for fn, args in calls:
        fn.restype = ctypes.c_int
        assert fn(*args) != 0, fn.__name__
        assert lib.bgc_diag_last_error().decode().startswith("invalid arguments"), (fn.__name__, lib.bgc_diag_last_error())


def test_negative_plant_count():
    """A Python list cannot have a negative length, so this one goes to the C ABI directly."""
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    lib.bgc_diag_last_error.restype = ctypes.c_char_p
    out = ctypes.create_string_buffer(4096)  # larger than any result struct
    plants = ctypes.create_string_buffer(4096)
    u64, u32, i32 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    calls = [
        (lib.bgc_diag_hbm_planted, [i32(0), u64(MIB), u32(SEED), plants, i32(-1), out]),
        (lib.bgc_diag_hbm_planted, [i32(0), u64(MIB), u32(SEED), None, i32(1), out]),  # a count without a list
        (lib.bgc_diag_pcie_planted, [i32(0), u64(MIB), u32(SEED), plants, i32(-1), out]),
        (lib.bgc_diag_hbm_walk_planted, [i32(0), u64(128 * MIB), u64(64 * MIB), u32(SEED), plants, i32(-1), None, i32(0), out]),
        (lib.bgc_diag_mfma_planted, [i32(0), i32(1), i32(64), u32(SEED), plants, i32(-1), None, i32(0), out]),
        (lib.bgc_diag_mfma_planted, [i32(0), i32(1), i32(64), u32(SEED), None, i32(0), plants, i32(-1), out]),
        (lib.bgc_diag_mfma_lowp_planted, [i32(0), i32(1), i32(64), u32(SEED), plants, i32(-1), None, i32(0), out]),
        (lib.bgc_diag_mfma_lowp_planted, [i32(0), i32(1), i32(64), u32(SEED), None, i32(0), plants, i32(-1), out]),
        (lib.bgc_diag_gemm_soak_planted, [i32(0), i32(256), i32(256), i32(128), i32(1), u32(SEED), plants, i32(-1), out]),
        (lib.bgc_diag_mfma_delayed, [i32(0), i32(1), i32(64), u32(SEED), plants, i32(-1), out]),
        (lib.bgc_diag_mfma_delayed, [i32(0), i32(1), i32(64), u32(SEED), None, i32(1), out]),  # a count without a list
        (lib.bgc_diag_mfma_delayed, [i32(0), i32(1), i32(64), u32(SEED), plants, i32(4097), out]),
        (lib.bgc_diag_mfma_delayed, [i32(0), i32(1), i32(64), u32(SEED), None, i32(0), None]),  # no result struct
        (lib.bgc_diag_burn_delayed, [i32(0), i32(300), i32(32), u32(SEED), i32(0), i32(2), u32(1000), None]),
        (lib.bgc_diag_burn_delayed, [i32(0), i32(300), i32(32), u32(SEED), i32(3), i32(2), u32(1000), out]),  # no such dtype
        (lib.bgc_diag_burn_planted, [i32(0), i32(300), i32(32), u32(SEED), i32(0), plants, i32(-1), out]),
        (lib.bgc_diag_burn_planted, [i32(0), i32(300), i32(32), u32(SEED), i32(0), None, i32(1), out]),  # a count without a list
        (lib.bgc_diag_burn_planted, [i32(0), i32(300), i32(32), u32(SEED), i32(0), plants, i32(4097), out]),
        (lib.bgc_diag_burn_planted, [i32(0), i32(300), i32(32), u32(SEED), i32(0), None, i32(0), None]),  # no result struct
        (lib.bgc_diag_burn_planted, [i32(0), i32(300), i32(32), u32(SEED), i32(3), None, i32(0), out]),  # no such dtype
        (lib.bgc_diag_burn_planted, [i32(0), i32(300), i32(32), u32(SEED), i32(-1), plants, i32(1), out]),
    ]
    for fn, args in calls:
        fn.restype = ctypes.c_int
        assert fn(*args) != 0, fn.__name__
        assert lib.bgc_diag_last_error().decode().startswith("invalid arguments"), (fn.__name__, lib.bgc_diag_last_error())
