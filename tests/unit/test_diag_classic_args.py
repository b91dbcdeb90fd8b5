"""The classic matrix-core entries (bgc_diag_mfma_classic, its planted variant, bgc_diag_mfma_classic_tile
and bgc_diag_gemm_dtype) refuse every out-of-range argument with "invalid arguments" on the host,
before the first HIP call: a plant names a wave, round, lane and accumulator element of a kernel, and
a GEMM shape sizes the buffers its kernel indexes, so neither may reach the device unchecked.
Because the refusal comes first, these run without a GPU (with one, a valid call would succeed;
without, it would fail with a HIP error instead)."""
import ctypes
import math

import pytest

SEED = 0x5EED
ROUNDS = 4  # BGC_CLASSIC_CHECK_ROUNDS
MAX_PLANTS = 4096  # BGC_DIAG_MAX_PLANTS
OK_CHECK = (0, 0, 0, 0, 0, 1.0)  # path, wave, round, lane, i, delta
OK_RATE = (0, 0, 0, 0, 0, 1.0)  # path, wave, lane, chain, i, delta
GEMM_K = {0: 32, 1: 64, 2: 4, 3: 4}
ELEM_BYTES = {0: 2, 1: 1, 2: 4, 3: 8}


def _refused(call, *args, what="classic mfma diag", detail=""):
    with pytest.raises(RuntimeError) as e:
        call(*args)
    assert str(e.value) == f"{what}: invalid arguments{detail}"


@pytest.mark.parametrize("waves_per_cu,iters", [(0, 64), (-1, 64), (65, 64), (1, 0), (1, (1 << 16) + 1)],
                         ids=["waves_0", "waves_-1", "waves_65", "iters_0", "iters_over_2^16"])
def test_classic_sizes_out_of_range(nat, waves_per_cu, iters):
    _refused(nat.diag_mfma_classic, 0, waves_per_cu, iters, SEED)
    _refused(nat.diag_mfma_classic_planted, 0, waves_per_cu, iters, SEED, [], [])
    _refused(nat.diag_mfma_classic_planted, 0, waves_per_cu, iters, SEED, [OK_CHECK], [OK_RATE])


@pytest.mark.parametrize("plant", [(-1, 0, 0, 0, 0, 1.0), (4, 0, 0, 0, 0, 1.0), (0, -2, 0, 0, 0, 1.0), (0, 0, -1, 0, 0, 1.0),
                                   (0, 0, ROUNDS, 0, 0, 1.0), (0, 0, 0, -1, 0, 1.0), (0, 0, 0, 64, 0, 1.0),
                                   (0, 0, 0, 0, -1, 1.0), (0, 0, 0, 0, 4, 1.0)],
                         ids=["path_-1", "path_4", "wave_-2", "round_-1", "round_at_rounds", "lane_-1", "lane_64", "i_-1", "i_4"])
def test_classic_check_plant_out_of_range(nat, plant):
    _refused(nat.diag_mfma_classic_planted, 0, 1, 64, SEED, [plant], [])
    _refused(nat.diag_mfma_classic_planted, 0, 1, 64, SEED, [OK_CHECK, plant], [])  # not only the first one is checked


@pytest.mark.parametrize("plant", [(-1, 0, 0, 0, 0, 1.0), (4, 0, 0, 0, 0, 1.0), (0, -1, 0, 0, 0, 1.0), (0, 0, -1, 0, 0, 1.0),
                                   (0, 0, 64, 0, 0, 1.0), (0, 0, 0, -1, 0, 1.0), (0, 0, 0, 4, 0, 1.0), (0, 0, 0, 0, -1, 1.0),
                                   (0, 0, 0, 0, 4, 1.0)],
                         ids=["path_-1", "path_4", "wave_-1", "lane_-1", "lane_64", "chain_-1", "chain_4", "i_-1", "i_4"])
def test_classic_rate_plant_out_of_range(nat, plant):
    _refused(nat.diag_mfma_classic_planted, 0, 1, 64, SEED, [], [plant])
    _refused(nat.diag_mfma_classic_planted, 0, 1, 64, SEED, [], [OK_RATE, plant])


@pytest.mark.parametrize("delta", [math.nan, math.inf, -math.inf, 2.0 ** 31, -(2.0 ** 31), 0.5],
                         ids=["nan", "inf", "-inf", "2^31", "-2^31", "half"])
def test_int8_delta_must_be_an_integer_below_2_31(nat, delta):
    _refused(nat.diag_mfma_classic_planted, 0, 1, 64, SEED, [(1, 0, 0, 0, 0, delta)], [])
    _refused(nat.diag_mfma_classic_planted, 0, 1, 64, SEED, [], [(1, 0, 0, 0, 0, delta)])
    _refused(nat.diag_mfma_classic_planted, 0, 1, 64, SEED, [OK_CHECK, (1, 0, 0, 0, 0, delta)], [])


def test_classic_plant_list_too_long(nat):
    _refused(nat.diag_mfma_classic_planted, 0, 1, 64, SEED, [OK_CHECK] * (MAX_PLANTS + 1), [])
    _refused(nat.diag_mfma_classic_planted, 0, 1, 64, SEED, [], [OK_RATE] * (MAX_PLANTS + 1))


@pytest.mark.parametrize("path", [-1, 4])
def test_classic_tile_path_out_of_range(nat, path):
    _refused(nat.diag_mfma_classic_tile, 0, path, SEED, 0, what="classic mfma tile")


GEMM_DETAIL = " (path 0..3; M, N multiples of 16 up to 4096; K a multiple of the path's K up to 8192)"


@pytest.mark.parametrize("path", [0, 1, 2, 3])
def test_gemm_dtype_shapes_out_of_range(nat, path):
    kk = GEMM_K[path]
    shapes = [(8, 16, kk), (16, 24, kk), (16, 16, kk // 2), (16, 16, kk + kk // 2), (0, 16, kk), (16, 0, kk), (16, 16, 0),
              (-16, 16, kk), (4096 + 16, 16, kk), (16, 4096 + 16, kk), (16, 16, 8192 + kk)]
    for m, n, k in shapes:
        size = ELEM_BYTES[path] * max(m, 0) * max(k, 0), ELEM_BYTES[path] * max(k, 0) * max(n, 0)
        _refused(nat.diag_gemm_dtype, 0, path, m, n, k, bytes(size[0]), bytes(size[1]), what="dtype gemm", detail=GEMM_DETAIL)


@pytest.mark.parametrize("path", [-1, 4])
def test_gemm_dtype_path_out_of_range(nat, path):
    _refused(nat.diag_gemm_dtype, 0, path, 16, 16, 64, bytes(16 * 64 * 8), bytes(16 * 64 * 8), what="dtype gemm", detail=GEMM_DETAIL)


def test_classic_null_pointers_and_negative_counts():
    """The bindings always pass buffers and a list's own length, so these go to the C ABI directly."""
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    lib.bgc_diag_last_error.restype = ctypes.c_char_p
    out = ctypes.create_string_buffer(4096)  # larger than the result struct
    plants = ctypes.create_string_buffer(4096)  # zeroes: valid plants, were they ever looked at
    ab = ctypes.create_string_buffer(16 * 64 * 8)
    u32, i32 = ctypes.c_uint32, ctypes.c_int
    run = [i32(0), i32(1), i32(64), u32(SEED)]
    calls = [
        (lib.bgc_diag_mfma_classic, run + [None]),
        (lib.bgc_diag_mfma_classic_planted, run + [None, i32(0), None, i32(0), None]),
        (lib.bgc_diag_mfma_classic_planted, run + [plants, i32(-1), None, i32(0), out]),
        (lib.bgc_diag_mfma_classic_planted, run + [None, i32(0), plants, i32(-1), out]),
        (lib.bgc_diag_mfma_classic_planted, run + [None, i32(1), None, i32(0), out]),  # a count without a list
        (lib.bgc_diag_mfma_classic_planted, run + [None, i32(0), None, i32(1), out]),
        (lib.bgc_diag_mfma_classic_tile, [i32(0), i32(0), u32(SEED), u32(0), None]),
        (lib.bgc_diag_gemm_dtype, [i32(0), i32(0), i32(16), i32(16), i32(32), None, ab, out]),
        (lib.bgc_diag_gemm_dtype, [i32(0), i32(0), i32(16), i32(16), i32(32), ab, None, out]),
        (lib.bgc_diag_gemm_dtype, [i32(0), i32(0), i32(16), i32(16), i32(32), ab, ab, None]),
    ]
    for fn, args in calls:
        fn.restype = ctypes.c_int
        assert fn(*args) != 0, fn.__name__
        assert lib.bgc_diag_last_error().decode().startswith("invalid arguments"), (fn.__name__, lib.bgc_diag_last_error())


def test_constants_match_the_header():
    import os
    import re

    from bacchus_gpu_controller_amd import ops

    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    header = open(os.path.join(root, "native", "gpu", "hip", "gpu_diag.h")).read()
    assert int(re.search(r"#define BGC_CLASSIC_CHECK_ROUNDS (\d+)", header).group(1)) == ops.CLASSIC_CHECK_ROUNDS == ROUNDS
    for name, code in ops.CLASSIC_PATHS.items():
        assert int(re.search(rf"#define BGC_CLASSIC_{name.upper()} (\d)", header).group(1)) == code
    assert ops.CLASSIC_TILE_LANE.itemsize == 2 * 16 + 2 * 32
    assert re.search(r"#define BGC_DIAG_ABI_VERSION 15\b", header)  # the change adds symbols only
