"""The GEMMs on caller operands (bgc_diag_gemm, bgc_diag_gemm_tiled, bgc_diag_mx_gemm) launch one
wave or one block per output tile with no bounds checks in the kernels, so a shape that is no
multiple of the tile, or larger than the entry point allows, must be refused on the host before the
GPU is touched.  The operand buffers here have the size the shape asks for, so the binding's own
size check passes and the library's check is the one reached.  The refusal comes before the first
HIP call, which is why these run without a GPU (with one, a valid call would succeed; without, it
would fail with a HIP error, not with "invalid arguments")."""
import ctypes

import pytest


def _refused(call, *args):
    with pytest.raises((RuntimeError, ValueError), match="invalid arguments"):
        call(*args)


@pytest.mark.parametrize("m,n,k", [(0, 16, 32), (16, 24, 32), (16, 16, 48), (4112, 16, 32)],
                         ids=["m_0", "n_24", "k_48", "m_4112"])
def test_gemm_shape_refused(nat, m, n, k):
    _refused(nat.diag_gemm, 0, m, n, k, b"\0" * (m * k * 2), b"\0" * (k * n * 2))


@pytest.mark.parametrize("m,n,k", [(64, 128, 64), (128, 192, 64), (128, 128, 96), (128, 128, 32), (32768 + 128, 128, 64)],
                         ids=["m_64", "n_192", "k_96", "k_32", "m_32896"])
def test_gemm_tiled_shape_refused(nat, m, n, k):
    _refused(nat.diag_gemm_tiled, 0, m, n, k, b"\0" * (m * k * 2), b"\0" * (n * k * 2))


@pytest.mark.parametrize("fmt", [0, 4], ids=["fp8", "fp4"])
@pytest.mark.parametrize("m,n,k", [(8, 16, 128), (16, 24, 128), (16384 + 16, 16, 128)], ids=["m_8", "n_24", "m_16400"])
def test_mx_gemm_shape_refused(nat, fmt, m, n, k):
    per = k if fmt == 0 else k // 2
    _refused(nat.diag_mx_gemm, 0, fmt, m, n, k, b"\0" * (m * per), b"\x7f" * (m * (k // 32)), b"\0" * (n * per),
             b"\x7f" * (n * (k // 32)))


def test_null_operands():
    """The binding always passes buffers, so the null pointers go to the C ABI directly."""
    from bacchus_gpu_controller_amd.utils.build import gpu_diag_path

    lib = ctypes.CDLL(gpu_diag_path())
    lib.bgc_diag_last_error.restype = ctypes.c_char_p
    i32 = ctypes.c_int
    buf = ctypes.create_string_buffer(128 * 128 * 4)  # holds any operand or C of the shapes below
    calls = []
    for fn, shape in [(lib.bgc_diag_gemm, [i32(16), i32(16), i32(32)]), (lib.bgc_diag_gemm_tiled, [i32(128), i32(128), i32(64)])]:
        for null in range(3):  # A, B or Bt, C
            calls.append((fn, [i32(0)] + shape + [None if i == null else buf for i in range(3)]))
    for null in range(5):  # A, its scales, Bt, its scales, C
        calls.append((lib.bgc_diag_mx_gemm, [i32(0), i32(0), i32(16), i32(16), i32(128)] + [None if i == null else buf for i in range(5)]))
    for fn, args in calls:
        fn.restype = ctypes.c_int
        assert fn(*args) != 0, (fn.__name__, args)
        assert lib.bgc_diag_last_error().decode().startswith("invalid arguments"), (fn.__name__, lib.bgc_diag_last_error())
