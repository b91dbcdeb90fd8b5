"""The diagnostics' five GEMM kernels on caller operands, held to exact equality at the smallest
shapes at which each of their code paths exists, on a real MI355X: mfma_gemm (ops.gemm),
gemm_soak<128,128,2,2>, gemm_soak<256,256,2,4> and gemm_pingpong (ops.gemm_tiled, the kernel forced
and checked case by case), and mx_gemm<fp8> / mx_gemm<fp4> (ops.mx_gemm).  They are the independent
evidence that the operand layouts, the LDS swizzle, the ping-pong staging schedule and the MX
scale-block layout are what the exact-integer tile checks and the ABFT soak assume.  Every assertion
covers every element of C; nothing is sampled or masked, and a failure names the kernel, the shape,
the number of wrong elements and the first wrong one.  torch stays on the CPU in this process.

What each section rests on:

1. Bit-exact integer products.  Derived from the code and the formats: integers in [-7, 7] are exact
   in bf16, and with K <= 1152 every partial sum in any order is below 2^16 in magnitude, so exact in
   fp32; the reference is an int64 product.  For MX with unit scales the exact domains (fp4: all 16
   codes; fp8: exponent field 7 or 8, 1 <= |a| < 4, and zeros) rest on an earlier measurement,
   profiles/mx_lowp_r3/mx_numerics.json (both 100 % exact on the MI355X); on paper products are
   multiples of 1/64 of at most 36, so sums over K <= 512 are exact in fp32.
2. Position probes.  Derived: one operand is one-hot per row, so each output is a single product
   and involves no accumulation; the other operand carries a code that is injective in k (bf16: for
   K <= 256; fp8: 253 finite codes of distinct value; fp4: the 14 non-zero values cycling), so a
   wrong output says which k, and for MX which scale block, was read.
3. MX scaling is a shift.  Derived: scales are powers of two, |C_unit| < 2^15 with granularity 2^-6
   and shifts within +-60 cannot overflow or underflow fp32, so C == ldexp(C_unit, sa + sb - 254).
   With scales that differ from block to block and several products per output the hardware's
   accumulation is not exact; those cases keep the project's fp32-accumulation bound and the
   fp8-narrow / fp4 domains of test_mx_gemm_matches_torch_decode.
4. The four bf16 kernels agree bit for bit.  Derived from the code, not measured before: all feed
   v_mfma_f32_16x16x32_bf16 the same 32 K-elements in the same lane positions (mfma_gemm:
   k = 8 (lane >> 4) + j; soak_frag: chunk 4 s + (lane >> 4)) and chain the accumulator through
   ascending K.
5. NaN and Inf stay in their row or column.  Derived: one non-finite operand, no zero operands, so
   IEEE arithmetic gives exactly one NaN row or one column of signed Inf; everything else equals the
   int64 reference.  Which non-finite value appears is compared with a torch fp64 product.

On the MI355X every one of these holds: sections 3 to 5 found no deviation of the matrix cores from
IEEE arithmetic, so no assertion here is relaxed for the hardware."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED

# ---------------------------------------------------------------------------------------------
# bf16 kernels

KERNEL_NAMES = {"mfma": "dense_gemm<Bf16Path, float>", "soak128": "gemm_soak<128,128,2,2>", "soak256": "gemm_soak<256,256,2,4>",
                "pingpong": "gemm_pingpong"}
# environment that forces the kernel for any shape it can run, and what diag_gemm_soak then reports
_FORCE = {"soak128": ({"BGC_SOAK_TILE": "128"}, (128, "2buf")), "soak256": ({"BGC_SOAK_KERNEL": "2buf"}, (256, "2buf")),
          "pingpong": ({}, (256, "pingpong"))}
PROBE_SHAPES = {"soak128": (128, 128, 192), "soak256": (256, 256, 192), "pingpong": (256, 256, 256), "mfma": (32, 32, 64)}


def _what(kernel, shape):
    return f"{KERNEL_NAMES.get(kernel, kernel)} at {'x'.join(map(str, shape))}"


def _select(monkeypatch, nat, kernel, shape):
    """Make bgc_diag_gemm_tiled run `kernel` at `shape`, and check that it will: it shares
    soak_kernel() with the soak, which reports what it ran."""
    for var in ("BGC_SOAK_TILE", "BGC_SOAK_KERNEL"):
        monkeypatch.delenv(var, raising=False)
    if kernel == "mfma":
        return
    env, expect = _FORCE[kernel]
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    r = json.loads(nat.diag_gemm_soak(0, *shape, 1, SEED))
    assert (r["tile"], r["kernel"]) == expect, f"{_what(kernel, shape)}: the selection runs {(r['tile'], r['kernel'])}"


def _bf16(x):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    assert np.array_equal(t.float().numpy(), np.asarray(x, dtype=np.float32), equal_nan=True), "operand not exact in bf16"
    return t


def _run(monkeypatch, nat, kernel, a, bt):
    """C = A Bt^T (A: M x K, Bt: N x K, bf16 tensors) on `kernel`."""
    from bacchus_gpu_controller_amd import ops

    shape = (a.shape[0], bt.shape[0], a.shape[1])
    _select(monkeypatch, nat, kernel, shape)
    return ops.gemm(a, bt.T.contiguous()) if kernel == "mfma" else ops.gemm_tiled(a, bt)


def _assert_equal(c, ref, what, describe=None, equal_nan=False):
    """Every element of c equals ref (NaN equals NaN only with equal_nan); the failure names the
    extent of the damage and the first wrong element, `describe(row, col, got)` adding what it knows."""
    c = np.asarray(c)
    ref = np.asarray(ref, dtype=c.dtype)
    assert c.shape == ref.shape, (what, c.shape, ref.shape)
    if np.array_equal(c, ref, equal_nan=equal_nan):
        return
    same = c == ref
    if equal_nan:
        same |= np.isnan(c) & np.isnan(ref)
    bad = np.argwhere(~same)
    r, col = (int(x) for x in bad[0])
    msg = (f"{what}: {len(bad)} of {c.size} elements wrong, in rows {bad[:, 0].min()}..{bad[:, 0].max()} and columns "
           f"{bad[:, 1].min()}..{bad[:, 1].max()}; first at (row {r}, col {col}): got {float(c[r, col])!r}, expected {float(ref[r, col])!r}")
    if describe:
        msg += "; " + describe(r, col, c[r, col])
    pytest.fail(msg)


def _int_operands(m, n, k, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi + 1, (m, k)), rng.integers(lo, hi + 1, (n, k))


def _int_ref(a, bt):
    ref = a.astype(np.int64) @ bt.astype(np.int64).T
    assert np.abs(ref).max() < 1 << 24
    return ref.astype(np.float32)


# --- 1. bit-exact integer products ---------------------------------------------------------------
# soak128: one block with one K-tile (the loop never stages); two K-tiles; 3 blocks (fewer than 8
# XCDs) with an odd number of K-tiles; 27 blocks, 9 tile-rows = a full group of 8 and a partial one.
# soak256: the same minima; 2buf forced where ping-pong would run; 18 blocks in 9 tile-rows.
# pingpong: one 8-phase iteration (every later stage hits the last-tile clamp), two, three; two
# blocks; 9 blocks in a group and a partial group; 3 blocks side by side.
# mfma: one tile with one K step; tiles side by side; tiles above each other with two K steps; the
# shape of test_mfma_gemm_matches_torch_fp32.
INT_CASES = [("soak128", (128, 128, 64)), ("soak128", (128, 128, 128)), ("soak128", (128, 384, 192)), ("soak128", (1152, 384, 64)),
             ("soak256", (256, 256, 64)), ("soak256", (256, 256, 192)), ("soak256", (256, 256, 128)), ("soak256", (2304, 512, 64)),
             ("pingpong", (256, 256, 128)), ("pingpong", (256, 256, 256)), ("pingpong", (256, 256, 384)),
             ("pingpong", (512, 256, 128)), ("pingpong", (2304, 256, 128)), ("pingpong", (256, 768, 256)),
             ("mfma", (16, 16, 32)), ("mfma", (16, 48, 32)), ("mfma", (48, 16, 64)), ("mfma", (128, 96, 512))]


def _case_id(case):
    return f"{case[0]}-{'x'.join(map(str, case[1]))}"


@pytest.mark.parametrize("kernel,shape", INT_CASES, ids=[_case_id(c) for c in INT_CASES])
def test_integer_product_is_exact(monkeypatch, nat, kernel, shape):
    m, n, k = shape
    a, bt = _int_operands(m, n, k, -7, 7, m * 7 + n * 3 + k)
    c = _run(monkeypatch, nat, kernel, _bf16(a), _bf16(bt))
    _assert_equal(c, _int_ref(a, bt), _what(kernel, shape))


# --- 2. position probes --------------------------------------------------------------------------
def _probe_pos(i, k):
    return (7 * i + 3) % k


def _one_hot(rows, k):
    x = np.zeros((rows, k), dtype=np.int64)
    x[np.arange(rows), _probe_pos(np.arange(rows), k)] = 1
    return x


def _k_code(rows, k):
    """[i][k] -> ((k + 17 i) mod 256) - 128: exact in bf16, injective in k for K <= 256"""
    assert k <= 256
    return (np.arange(k)[None, :] + 17 * np.arange(rows)[:, None]) % 256 - 128


def _k_name(k):
    return f"k = {k} (K-tile {k // 64}, chunk {k % 64 // 8}, element {k % 8})"


@pytest.mark.parametrize("one_hot", ["A", "Bt"])
@pytest.mark.parametrize("kernel", list(PROBE_SHAPES))
def test_one_hot_probe_reads_the_right_k(monkeypatch, nat, kernel, one_hot):
    """A one-hot in k = (7 row + 3) mod K and Bt[c][k] a code of k (and the mirror): C[r][c] is the
    code at the one position A selects, so a wrong element says which k was read instead.  Over
    both probes every (row mod 8, 16-byte chunk) pair of the LDS swizzle occurs on both operands."""
    m, n, k = shape = PROBE_SHAPES[kernel]
    if one_hot == "A":
        a, bt = _one_hot(m, k), _k_code(n, k)
        ref = bt[:, _probe_pos(np.arange(m), k)].T
    else:
        a, bt = _k_code(m, k), _one_hot(n, k)
        ref = a[:, _probe_pos(np.arange(n), k)]
    hit = {(int(i) % 8, int(_probe_pos(i, k)) % 64 // 8) for i in range(m if one_hot == "A" else n)}
    assert len(hit) == 64 or kernel == "mfma", "the probe misses a (row mod 8, chunk) pair"

    def describe(r, col, got):
        hot, coded, name = (r, col, "Bt") if one_hot == "A" else (col, r, "A")
        want = int(_probe_pos(hot, k))
        if not (np.isfinite(got) and got == int(got) and -128 <= got <= 127):
            return f"row {r}, col {col} should have read {name}[{coded}] at {_k_name(want)}; {got!r} is no single element of it"
        read = (int(got) + 128 - 17 * coded) % 256
        # 17 row mod 256 shifts the code in k, so another row may hold the same value at the right k
        code_rows = n if one_hot == "A" else m
        others = [j for j in range(code_rows) if j != coded and (want + 17 * j) % 256 - 128 == got]
        also = f" (or the right k of {name}[{others[0]}])" if others else ""
        if got == 0:
            also += " (or nothing at all: 0 is also the empty sum)"
        if read >= k:
            return f"row {r}, col {col} should have read {name}[{coded}] at {_k_name(want)}; {got!r} is at no k of that row{also}"
        return f"row {r}, col {col} read {_k_name(read)} instead of {_k_name(want)} of {name}[{coded}]{also}"

    c = _run(monkeypatch, nat, kernel, _bf16(a), _bf16(bt))
    _assert_equal(c, ref.astype(np.float32), f"{_what(kernel, shape)}, one-hot {one_hot}", describe)


# --- 4. the bf16 kernels agree bit for bit -------------------------------------------------------
AGREE_CASES = [((256, 256, 128), ["mfma", "soak128", "soak256", "pingpong"]), ((256, 512, 192), ["mfma", "soak128", "soak256"]),
               ((512, 256, 384), ["mfma", "pingpong"])]


@pytest.mark.parametrize("shape,kernels", AGREE_CASES, ids=["x".join(map(str, s)) for s, _ in AGREE_CASES])
def test_bf16_kernels_agree_bit_for_bit(monkeypatch, nat, shape, kernels):
    import torch

    m, n, k = shape
    torch.manual_seed(m * 7 + n * 3 + k)
    a = torch.randn(m, k).to(torch.bfloat16)
    bt = torch.randn(n, k).to(torch.bfloat16)
    first = _run(monkeypatch, nat, kernels[0], a, bt)
    assert np.isfinite(first).all(), _what(kernels[0], shape)
    for kernel in kernels[1:]:
        c = _run(monkeypatch, nat, kernel, a, bt)
        if c.tobytes() == first.tobytes():
            continue
        bad = np.argwhere(c.view(np.uint32) != first.view(np.uint32))
        r, col = (int(x) for x in bad[0])
        pytest.fail(f"{_what(kernel, shape)} differs from {KERNEL_NAMES[kernels[0]]} in {len(bad)} of {c.size} elements, in rows "
                    f"{bad[:, 0].min()}..{bad[:, 0].max()} and columns {bad[:, 1].min()}..{bad[:, 1].max()}; first at (row {r}, "
                    f"col {col}): {float(c[r, col])!r} against {float(first[r, col])!r}")


# --- 5. NaN and Inf stay where they belong -------------------------------------------------------
def _nonfinite_positions(kernel):
    """(r0, c0, k0): off every border; then on the borders of a 128-row half-tile (16-row tile for
    mfma_gemm), first and last row, with k0 in the last K-tile (its last and its first element)."""
    m, n, k = PROBE_SHAPES[kernel]
    edge = 16 if kernel == "mfma" else 128
    step = 32 if kernel == "mfma" else 64
    return [(m // 4 + 5, n // 2 + 5, 21), (edge - 1, n - edge, k - 1), (m - edge, edge - 1, k - step)]


NONFINITE_CASES = [(kernel, i) for kernel in PROBE_SHAPES for i in range(3)]


def _nonfinite_operands(kernel, which):
    import torch

    m, n, k = PROBE_SHAPES[kernel]
    rng = np.random.default_rng(m + n + k + which)
    a = (rng.integers(1, 4, (m, k)) * rng.choice([-1, 1], (m, k))).astype(np.float32)
    bt = (rng.integers(1, 4, (n, k)) * rng.choice([-1, 1], (n, k))).astype(np.float32)
    return a, bt, lambda x, y: (torch.from_numpy(x).double() @ torch.from_numpy(y).double().T).numpy()


@pytest.mark.parametrize("kernel,which", NONFINITE_CASES, ids=[f"{k}-{('inside', 'last_k', 'last_tile')[i]}" for k, i in NONFINITE_CASES])
def test_nan_stays_in_its_row(monkeypatch, nat, kernel, which):
    shape = PROBE_SHAPES[kernel]
    r0, _, k0 = _nonfinite_positions(kernel)[which]
    a, bt, product = _nonfinite_operands(kernel, which)
    ref = _int_ref(a, bt)
    a[r0, k0] = np.nan
    c = _run(monkeypatch, nat, kernel, _bf16(a), _bf16(bt))
    what = f"{_what(kernel, shape)}, A[{r0}][{k0}] = NaN"
    # confinement: every other row is exact, and row r0 is not finite
    others = np.arange(shape[0]) != r0
    confined = ref.copy()
    confined[r0] = c[r0]
    _assert_equal(c, confined, what + " (outside row r0)", equal_nan=True)
    assert not np.isfinite(c[r0]).any(), f"{what}: row {r0} has finite elements at columns {np.flatnonzero(np.isfinite(c[r0]))[:8]}"
    # the value: NaN throughout, as IEEE arithmetic and the torch product have it
    tref = product(a, bt)
    assert np.isnan(tref[r0]).all() and np.array_equal(tref[others], ref[others])
    _assert_equal(c, tref.astype(np.float32), what, equal_nan=True)


@pytest.mark.parametrize("kernel,which", NONFINITE_CASES, ids=[f"{k}-{('inside', 'last_k', 'last_tile')[i]}" for k, i in NONFINITE_CASES])
def test_inf_stays_in_its_column(monkeypatch, nat, kernel, which):
    shape = PROBE_SHAPES[kernel]
    _, c0, k0 = _nonfinite_positions(kernel)[which]
    a, bt, product = _nonfinite_operands(kernel, which)
    ref = _int_ref(a, bt)
    bt[c0, k0] = np.inf
    c = _run(monkeypatch, nat, kernel, _bf16(a), _bf16(bt))
    what = f"{_what(kernel, shape)}, Bt[{c0}][{k0}] = +Inf"
    others = np.arange(shape[1]) != c0
    confined = ref.copy()
    confined[:, c0] = c[:, c0]
    _assert_equal(c, confined, what + " (outside column c0)", equal_nan=True)
    assert not np.isfinite(c[:, c0]).any(), f"{what}: column {c0} has finite elements at rows {np.flatnonzero(np.isfinite(c[:, c0]))[:8]}"
    # the value: sign(A[r][k0]) Inf, as IEEE arithmetic and the torch product have it
    tref = product(a, bt)
    assert np.array_equal(tref[:, c0], np.sign(a[:, k0]) * np.inf) and np.array_equal(tref[:, others], ref[:, others])
    _assert_equal(c, tref.astype(np.float32), what, equal_nan=True)


# ---------------------------------------------------------------------------------------------
# MX block-scaled kernels (mx_gemm<0> fp8 e4m3, mx_gemm<4> fp4 e2m1)

_FP4_E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])
_FP4_NONZERO = np.array([1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15], dtype=np.uint8)
# every finite e4m3 code but -0: 253 distinct values (0x7F and 0xFF are NaN)
_FP8_DISTINCT = np.array([c for c in range(256) if c & 0x7F != 0x7F and c != 0x80], dtype=np.uint8)


def _decode(fmt, codes):
    """fp64 values of an array of codes (fp8: e4m3 bytes; fp4: one e2m1 code per element), by a
    decode that shares nothing with the kernels: torch.float8_e4m3fn and the e2m1 table."""
    import torch

    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if fmt == "fp8":
        return torch.from_numpy(codes.copy()).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    return _FP4_E2M1[codes]


def _pack(fmt, codes):
    """the bytes ops.mx_gemm takes: fp4 two per byte, element 2i in the low nibble"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    return codes if fmt == "fp8" else (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def _exact_domain_codes(fmt, rows, k, rng):
    """codes of the domain measured exact under unit scales: fp4 all 16 codes; fp8 exponent field
    7 or 8 (1 <= |a| < 4) of both signs, and one in eight a zero of either sign"""
    if fmt == "fp4":
        return rng.integers(0, 16, (rows, k)).astype(np.uint8)
    sign = rng.integers(0, 2, (rows, k)) << 7
    c = sign | (rng.integers(7, 9, (rows, k)) << 3) | rng.integers(0, 8, (rows, k))
    return np.where(rng.integers(0, 8, (rows, k)) == 0, sign, c).astype(np.uint8)


def _mx(fmt, a_codes, sa, bt_codes, sb):
    from bacchus_gpu_controller_amd import ops

    return ops.mx_gemm(_pack(fmt, a_codes), sa, _pack(fmt, bt_codes), sb, fmt=fmt).astype(np.float64)


def _unit(rows, k):
    return np.full((rows, k // 32), 127, dtype=np.uint8)


def _is_fp32(x):
    return np.array_equal(x.astype(np.float32).astype(np.float64), x)


MX_EXACT_SHAPES = [(16, 16, 128), (16, 48, 128), (48, 16, 256), (32, 32, 512)]


@pytest.mark.parametrize("shape", MX_EXACT_SHAPES, ids=["x".join(map(str, s)) for s in MX_EXACT_SHAPES])
@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_mx_unit_scale_product_is_exact(fmt, shape):
    m, n, k = shape
    rng = np.random.default_rng(m * 7 + n * 3 + k + (fmt == "fp4"))
    a, bt = _exact_domain_codes(fmt, m, k, rng), _exact_domain_codes(fmt, n, k, rng)
    ref = _decode(fmt, a) @ _decode(fmt, bt).T
    assert _is_fp32(ref)
    _assert_equal(_mx(fmt, a, _unit(m, k), bt, _unit(n, k)), ref, _what(f"mx_gemm<{fmt}> (unit scales)", shape))


def _mx_probe_pos(i, k):
    return (37 * i + 5) % k


@pytest.mark.parametrize("one_hot", ["A", "Bt"])
@pytest.mark.parametrize("shape", [(16, 16, 128), (32, 48, 256)], ids=["16x16x128", "32x48x256"])
@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_mx_one_hot_probe_reads_the_right_k_and_scales(fmt, shape, one_hot):
    """One operand is 1.0 at k = p(row) = (37 row + 5) mod K and zero elsewhere, the other a code of
    k; scale bytes are drawn per (row or column, block of 32).  Each output is the one product
    decode(code at p) 2^(sa[r][p/32] + sb[c][p/32] - 254), exact whatever the accumulation does.
    p takes every scale block and, for fp8, both 16-element halves of every lane group (K 16g.. and
    64+16g..), so this pins the lane layout and which lane group's scale byte reaches which block."""
    m, n, k = shape
    rng = np.random.default_rng(m * 7 + n * 3 + k + (fmt == "fp4") + 2 * (one_hot == "A"))
    hot_rows, code_rows = (m, n) if one_hot == "A" else (n, m)
    p = _mx_probe_pos(np.arange(hot_rows), k)
    assert {int(x) % 128 // 16 for x in p} == set(range(8)), "the probe misses a lane group half or a scale block"
    hot = np.zeros((hot_rows, k), dtype=np.uint8)
    hot[np.arange(hot_rows), p] = 0x38 if fmt == "fp8" else 2  # 1.0
    kk, ii = np.arange(k)[None, :], np.arange(code_rows)[:, None]
    coded = _FP8_DISTINCT[(kk + 17 * ii) % len(_FP8_DISTINCT)] if fmt == "fp8" else _FP4_NONZERO[(kk + 3 * ii) % 14]
    s_hot = rng.integers(127 - 8, 127 + 9, (hot_rows, k // 32)).astype(np.uint8)
    s_code = rng.integers(127 - 8, 127 + 9, (code_rows, k // 32)).astype(np.uint8)
    values = _decode(fmt, coded)  # [code row][k]
    # ref[h][j] = values[j][p(h)] 2^(s_hot[h][p(h)/32] + s_code[j][p(h)/32] - 254)
    exps = s_hot[np.arange(hot_rows), p // 32].astype(np.int64)[:, None] + s_code[:, p // 32].T.astype(np.int64) - 254
    ref = np.ldexp(values[:, p].T, exps)
    assert _is_fp32(ref)
    names = ("A", "Bt") if one_hot == "A" else ("Bt", "A")

    def describe(r, col, got):
        h, j = (r, col) if one_hot == "A" else (col, r)
        want = int(p[h])
        said = (f"row {r}, col {col} should be {names[1]}[{j}] at k = {want} (lane-group K step {want // 128}, offset {want % 128}) "
                f"with the scales of block {want // 32}")
        fits = [(kr, bh, bj) for kr in range(k) for bh in range(k // 32) for bj in range(k // 32)
                if np.ldexp(values[j, kr], int(s_hot[h, bh]) + int(s_code[j, bj]) - 254) == got]
        fits.sort(key=lambda f: (f[0] != want, f[1] != want // 32, f[2] != want // 32))
        if not fits:
            return said + "; the value is no single scaled element of that row"
        return said + "; the value is " + " or ".join(
            f"k = {kr} (offset {kr % 128}) with the {names[0]} scale of block {bh} and the {names[1]} scale of block {bj}"
            for kr, bh, bj in fits[:4]) + (f" or {len(fits) - 4} more" if len(fits) > 4 else "")

    if one_hot == "A":
        c = _mx(fmt, hot, s_hot, coded, s_code)
    else:
        c, ref = _mx(fmt, coded, s_code, hot, s_hot), ref.T
    _assert_equal(c, ref, f"{_what(f'mx_gemm<{fmt}>', shape)}, one-hot {one_hot}", describe)


# --- 3. scaling is a shift -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 16, 128), (32, 32, 512)], ids=["16x16x128", "32x32x512"])
@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_mx_uniform_scales_shift_the_unit_product(fmt, shape):
    """Every block of row r carries the scale byte sa[r], every block of column c sb[c], drawn from
    [127 - 30, 127 + 30]: C == ldexp(C_unit, sa[r] + sb[c] - 254) exactly."""
    m, n, k = shape
    rng = np.random.default_rng(m * 7 + n * 3 + k + (fmt == "fp4") + 0x5ca1e)
    a, bt = _exact_domain_codes(fmt, m, k, rng), _exact_domain_codes(fmt, n, k, rng)
    sa = rng.integers(127 - 30, 127 + 31, (m, 1)).astype(np.uint8)
    sb = rng.integers(127 - 30, 127 + 31, (n, 1)).astype(np.uint8)
    unit = _decode(fmt, a) @ _decode(fmt, bt).T
    ref = np.ldexp(unit, sa.astype(np.int64) + sb.astype(np.int64).T - 254)
    assert _is_fp32(unit) and _is_fp32(ref)
    c = _mx(fmt, a, np.repeat(sa, k // 32, axis=1), bt, np.repeat(sb, k // 32, axis=1))

    def describe(r, col, got):
        return (f"scales 2^{int(sa[r, 0]) - 127} and 2^{int(sb[col, 0]) - 127}, unit-scale product {unit[r, col]!r}: "
                f"got / expected = {got / ref[r, col]!r}")

    _assert_equal(c, ref, _what(f"mx_gemm<{fmt}> (one scale per row and column)", shape), describe)


@pytest.mark.parametrize("shape", [(16, 16, 128), (16, 48, 256)], ids=["16x16x128", "16x48x256"])
@pytest.mark.parametrize("case", ["fp8-narrow", "fp4"])
def test_mx_block_scales_match_decode_at_the_smallest_shapes(case, shape):
    """test_mx_gemm_matches_torch_decode (128x96x512) at one K step on a single tile and at two K
    steps on three: random codes of the fp8-narrow (0.5 <= |a| < 4) and fp4 (all codes) domains,
    scales 2^-8..2^8 per block, within the fp32-accumulation bound."""
    fmt = "fp4" if case == "fp4" else "fp8"
    m, n, k = shape
    rng = np.random.default_rng(m * 7 + n * 3 + k + (fmt == "fp4") + 0xb10c)
    sa = rng.integers(127 - 8, 127 + 9, (m, k // 32)).astype(np.uint8)
    sb = rng.integers(127 - 8, 127 + 9, (n, k // 32)).astype(np.uint8)

    def codes(rows):
        if fmt == "fp4":
            return rng.integers(0, 16, (rows, k)).astype(np.uint8)
        return ((rng.integers(0, 2, (rows, k)) << 7) | (rng.integers(6, 9, (rows, k)) << 3) | rng.integers(0, 8, (rows, k))).astype(np.uint8)

    a, bt = codes(m), codes(n)
    af = _decode(fmt, a) * np.repeat(np.exp2(sa.astype(np.float64) - 127), 32, axis=1)
    bf = _decode(fmt, bt) * np.repeat(np.exp2(sb.astype(np.float64) - 127), 32, axis=1)
    ref, mag = af @ bf.T, np.abs(af) @ np.abs(bf).T
    c = _mx(fmt, a, sa, bt, sb)
    bound = 4.0 * k * 5.96e-8 * mag + 1e-30  # fp32 accumulation of exact scaled products
    ratio = np.abs(c - ref) / bound
    assert np.isfinite(c).all()
    r, col = (int(x) for x in np.unravel_index(np.argmax(ratio), ratio.shape))
    assert ratio.max() <= 1.0, (f"{_what(f'mx_gemm<{fmt}>', shape)}: {(ratio > 1).sum()} of {c.size} elements beyond the bound; worst at "
                                f"(row {r}, col {col}): got {c[r, col]!r}, expected {ref[r, col]!r}, {ratio[r, col]:.3g} bounds off")
