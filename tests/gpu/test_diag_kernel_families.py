"""The diagnostics' shared helpers at the smallest shapes at which they can still go wrong, on a
real MI355X: ragged slabs in the HBM streams, every soak-GEMM kernel the selection can pick
(checksums and an independent fp32 product), its two environment knobs, and the burn's dtype
dispatch.  torch stays on the CPU in this process."""
import json

import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nbytes", [(1 << 20) + 16 * 37, (32 << 20) + 16 * (2048 * 3 + 5)],
                         ids=["slab_shorter_than_a_block", "ragged_slab_ends"])
def test_hbm_ragged_streams(nbytes):
    from bacchus_gpu_controller_amd import ops

    r = ops.hbm(0, nbytes=nbytes, iters=1)
    assert r["passed"] and r["mismatches"] == 0, r
    assert r["bytes"] == nbytes, r


# (m, n, k) -> (tile, kernel): the 256-tile double-buffered kernel; 15 workgroups (the remap's
# nwg % 8 != 0 branch, a partial row group) with a single 8-phase iteration (the last-tile
# clamp); the single-workgroup minimum
SOAK_SHAPES = [((256, 512, 192), (256, "2buf")), ((768, 1280, 128), (256, "pingpong")),
               ((256, 256, 128), (256, "pingpong"))]


@pytest.mark.parametrize("shape,expect", SOAK_SHAPES, ids=["x".join(map(str, s)) for s, _ in SOAK_SHAPES])
def test_soak_kernel_selection(shape, expect):
    import torch

    from bacchus_gpu_controller_amd import native, ops

    m, n, k = shape
    r = json.loads(native().diag_gemm_soak(0, m, n, k, 1, 0x5EED))
    assert (r["tile"], r["kernel"]) == expect, r
    assert r["passed"], r
    torch.manual_seed(m * 7 + n * 3 + k)
    a = torch.randn(m, k).to(torch.bfloat16)
    bt = torch.randn(n, k).to(torch.bfloat16)
    c = torch.from_numpy(ops.gemm_tiled(a, bt).copy())
    af, bf = a.float(), bt.float()
    ref = af @ bf.T
    mag = af.abs() @ bf.abs().T
    bound = 4.0 * k * 5.96e-8 * mag + 1e-6  # the gemm_check bound: fp32 accumulation of exact bf16 products
    ratio = ((c - ref).abs() / bound).max().item()
    assert torch.isfinite(c).all()
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("var,value,expect", [("BGC_SOAK_KERNEL", "2buf", (256, "2buf")),
                                              ("BGC_SOAK_TILE", "128", (128, "2buf"))])
def test_soak_environment_knobs(monkeypatch, var, value, expect):
    from bacchus_gpu_controller_amd import native

    monkeypatch.setenv(var, value)
    r = json.loads(native().diag_gemm_soak(0, 256, 256, 128, 1, 0x5EED))
    assert (r["tile"], r["kernel"]) == expect, r
    assert r["passed"], r


@pytest.mark.parametrize("dtype", ["bf16", "fp8", "fp4"])
def test_burn_dtype_dispatch(dtype):
    from bacchus_gpu_controller_amd import native

    n = native()
    r = json.loads(n.diag_burn(n.gpu_backend("amdsmi", ""), 0, 0, 200, 0x5EED, dtype))
    assert r["dtype"] == dtype, r
    assert r["mismatches"] == 0 and r["launches"] >= 1, r
