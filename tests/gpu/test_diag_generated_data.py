"""The data the GPU diagnostics generate for themselves, against references that share no code with
the library.  Every diagnostic checks its generator against itself (the function that fills a buffer
also says what the buffer must hold), so a generator that is degenerate, repeats itself or leaves
stale data in place makes the diagnostic weaker without making it fail.  The *_data entry points and
mfma_tile (gpu_diag.h, "generated data") run the production implementation and hand back what it
generated; every reference here is written from the documentation in gpu_diag.h, in numpy and plain
Python.  All comparisons are exact and cover every word or element; nothing is sampled.  Every kernel
runs to completion and every access stays inside its allocation.  torch is not used.

The share bounds (45 % to 55 % of the words per bit, 30 % to 37 % per operand value) are wide around
what the reference patterns give on the CPU: 49.7 % to 50.2 % per bit at the small HBM size, 33.0 % to
33.6 % per value for a 256 x 128 soak operand and 33.1 % to 33.6 % over 64 matrix-core tiles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED
MIB = 1 << 20
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
GOLDEN = 0x9E3779B9


# ---------------------------------------------------------------------------------------------
# the documented hashes

def mix32(x):
    """on a uint32 array (products wrap)"""
    x = np.array(x, dtype=np.uint32, copy=True)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def mix32_int(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def mix64_int(x):
    x &= M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    return x ^ (x >> 33)


def test_the_two_mix32_agree():
    xs = [0, 1, SEED, GOLDEN, M32, 0x80000000, 123456789]
    assert [int(v) for v in mix32(xs)] == [mix32_int(x) for x in xs]


def trit(h):
    return (h % np.uint32(3)).astype(np.int64) - 1


def _all_distinct(x):
    return len(np.unique(x)) == x.size


def _first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return f"{len(bad)} of {got.size} differ; first at {int(bad[0])}: got {int(got[bad[0]]):#x}, expected {int(want[bad[0]]):#x}"


def _shares(values):
    """the share of -1, 0 and 1 in an array that holds nothing else"""
    return [float(np.mean(values == v)) for v in (-1, 0, 1)]


# ---------------------------------------------------------------------------------------------
# HBM stream

HBM_SIZES = {"slab_shorter_than_a_block": (1 << 20) + 16 * 37, "ragged_slab_ends": (32 << 20) + 16 * (2048 * 3 + 5)}


def hbm_pattern_seed(seed, it):
    """of timed iteration `it`; the warm-up fill is it = -1"""
    return mix32_int(seed + (it + 1) * GOLDEN)


def hbm_pattern(n16, s):
    i = np.arange(n16, dtype=np.uint64)
    w = (i << np.uint64(2)).astype(np.uint32) ^ ((i >> np.uint64(30)).astype(np.uint32) * np.uint32(GOLDEN))
    words = w[:, None] + np.arange(4, dtype=np.uint32)[None, :]
    return mix32(words ^ np.uint32(s)).reshape(-1)


@pytest.fixture(scope="module", params=list(HBM_SIZES))
def hbm_copies(request):
    """{iters: the copy buffer after a run of `iters` iterations} at one size"""
    from bacchus_gpu_controller_amd import ops

    nbytes = HBM_SIZES[request.param]
    out = {}
    for iters in (1, 2):
        r, words = ops.hbm_data(nbytes, iters, seed=SEED)
        assert r["bytes"] == nbytes and r["iters"] == iters and r["mismatches"] == 0 and r["passed"] is True, r
        assert words.size == nbytes // 4
        out[iters] = words
    return out


@pytest.mark.parametrize("iters", [1, 2])
def test_hbm_copy_holds_the_last_iterations_pattern(hbm_copies, iters):
    got = hbm_copies[iters]
    want = hbm_pattern(got.size // 4, hbm_pattern_seed(SEED, iters - 1))
    assert np.array_equal(got, want), _first_difference(got, want)


def test_hbm_iterations_differ_in_every_word(hbm_copies):
    same = np.flatnonzero(hbm_copies[1] == hbm_copies[2])
    assert same.size == 0, f"{same.size} of {hbm_copies[1].size} words are the same after one and after two iterations; first {int(same[0])}"


def test_hbm_warm_up_differs_from_the_first_iteration_in_every_word(hbm_copies):
    """By the documented seeds: what the warm-up fill leaves in `a` cannot pass for iteration 0."""
    n16 = hbm_copies[1].size // 4
    assert not np.any(hbm_pattern(n16, hbm_pattern_seed(SEED, -1)) == hbm_copies[1])


@pytest.mark.parametrize("iters", [1, 2])
def test_hbm_words_are_pairwise_distinct(hbm_copies, iters):
    assert _all_distinct(hbm_copies[iters])


@pytest.mark.parametrize("iters", [1, 2])
def test_hbm_every_bit_is_set_in_about_half_of_the_words(hbm_copies, iters):
    words = hbm_copies[iters]
    share = [float(np.mean((words >> np.uint32(b)) & np.uint32(1))) for b in range(32)]
    print("share of words with each bit set:", [round(s, 4) for s in share])
    assert all(0.45 <= s <= 0.55 for s in share), share


# ---------------------------------------------------------------------------------------------
# HBM walk: 66 MiB in chunks of 64 MiB, one chunk of exactly two unroll steps per block (64 MiB / 16 /
# 2048 blocks = 2048 elements = 2 x 256 lanes x 4) and one of 2 MiB whose slabs are shorter than a block

WALK_BYTES, WALK_CHUNK = 66 * MIB, 64 * MIB


def walk_key(seed):
    return mix64_int(0x9E3779B97F4A7C15 ^ seed)


def _walk(passes):
    from bacchus_gpu_controller_amd import ops

    r, words = ops.hbm_walk_data(WALK_BYTES, WALK_CHUNK, passes, seed=SEED)
    chunks = r["chunk_list"]
    assert [size for _, size in chunks] == [64 * MIB, 2 * MIB] and r["chunks"] == 2, r
    assert r["passes"] == passes and r["mismatches"] == 0 and r["bytes_covered"] == WALK_BYTES, r
    assert words.size == WALK_BYTES // 8
    addresses = np.concatenate([np.uint64(base) + np.uint64(8) * np.arange(size // 8, dtype=np.uint64) for base, size in chunks])
    return words, addresses


def test_walk_first_pass_holds_address_xor_key():
    words, addresses = _walk(1)
    want = addresses ^ np.uint64(walk_key(SEED))
    assert np.array_equal(words, want), _first_difference(words, want)


def test_walk_second_pass_holds_the_complement():
    words, addresses = _walk(2)
    want = ~(addresses ^ np.uint64(walk_key(SEED)))
    assert np.array_equal(words, want), _first_difference(words, want)


# ---------------------------------------------------------------------------------------------
# PCIe

PCIE_BYTES = MIB


def test_pcie_pattern():
    from bacchus_gpu_controller_amd import ops

    r, words = ops.pcie_data(PCIE_BYTES, seed=SEED)
    assert r["bytes"] == PCIE_BYTES and r["iters"] == 1 and r["mismatches"] == 0, r
    assert words.size == PCIE_BYTES // 8
    i = np.arange(words.size, dtype=np.uint32)
    want = (mix32(i ^ np.uint32(SEED)).astype(np.uint64) << np.uint64(32)) | mix32(i ^ np.uint32(~SEED & M32)).astype(np.uint64)
    assert np.array_equal(words, want), _first_difference(words, want)


def test_pcie_both_halves_vary_from_word_to_word():
    from bacchus_gpu_controller_amd import ops

    _, words = ops.pcie_data(PCIE_BYTES, seed=SEED)
    high, low = (words >> np.uint64(32)).astype(np.uint32), words.astype(np.uint32)
    assert _all_distinct(high), f"{len(np.unique(high))} distinct high halves in {words.size} words"
    assert _all_distinct(low), f"{len(np.unique(low))} distinct low halves in {words.size} words"


# ---------------------------------------------------------------------------------------------
# GEMM soak

BF16_CODES = {0xBF80: -1, 0x0000: 0, 0x3F80: 1}
# (256, 256, 128): ping-pong.  (256, 512, 192): k is no multiple of 128, the 256-tile 2buf kernel.
# (384, 640, 320): the 128 tile; k exceeds one 256-thread pass of the row sums and leaves a partial
# column block of the column sums, m is six 64-row slabs.
SOAK_CASES = {(256, 256, 128): (256, "pingpong"), (256, 512, 192): (256, "2buf"), (384, 640, 320): (128, "2buf")}


def soak_operand(rows, cols, s):
    i = np.arange(rows * cols, dtype=np.uint32)  # below 2^32: the high half of the index is 0
    return trit(mix32(i ^ np.uint32(mix32_int(s)))).reshape(rows, cols)


def _from_bf16_codes(x, name):
    strange = sorted(set(np.unique(x).tolist()) - set(BF16_CODES))
    assert not strange, f"{name} holds bf16 codes other than those of -1, 0 and 1: {[hex(c) for c in strange[:8]]}"
    out = np.zeros(x.shape, dtype=np.int64)
    for code, value in BF16_CODES.items():
        out[x == code] = value
    return out


@pytest.mark.parametrize("shape", list(SOAK_CASES), ids=["x".join(map(str, s)) for s in SOAK_CASES])
def test_soak_operands_checksums_and_product(monkeypatch, shape):
    from bacchus_gpu_controller_amd import ops

    for var in ("BGC_SOAK_TILE", "BGC_SOAK_KERNEL"):
        monkeypatch.delenv(var, raising=False)
    m, n, k = shape
    r, a_codes, bt_codes, rref, cref, c = ops.gemm_soak_data(m, n, k, seed=SEED)
    assert (r["tile"], r["kernel"]) == SOAK_CASES[shape], r
    assert (r["m"], r["n"], r["k"], r["launches"]) == (m, n, k, 1) and r["passed"] is True, r
    a, bt = _from_bf16_codes(a_codes, "A"), _from_bf16_codes(bt_codes, "Bt")
    assert np.array_equal(a, soak_operand(m, k, SEED)), "A is not the documented hash"
    assert np.array_equal(bt, soak_operand(n, k, SEED ^ 0xB7B7B7B7)), "Bt is not the documented hash"
    rows = min(m, n)
    assert not np.array_equal(a[:rows], bt[:rows]), "A and Bt hold the same values"
    for name, x in (("A", a), ("Bt", bt)):
        shares = _shares(x)
        print(f"{name} {shape}: shares of -1, 0, 1 = {[round(s, 4) for s in shares]}")
        assert all(0.30 <= s <= 0.37 for s in shares), (name, shares)
    ones_m, ones_n = np.ones(m, dtype=np.int64), np.ones(n, dtype=np.int64)
    assert np.array_equal(rref, a @ (bt.T @ ones_n)), "rref is not A (B 1)"
    assert np.array_equal(cref, (ones_m @ a) @ bt.T), "cref is not (1^T A) B"
    product = a @ bt.T
    assert np.abs(product).max() < 1 << 24
    assert np.array_equal(c, product.astype(np.float32)), _first_difference(c.reshape(-1), product.astype(np.float32).reshape(-1))


# ---------------------------------------------------------------------------------------------
# matrix-core tiles

K_OF = {"bf16": 32, "fp8": 128, "fp4": 128}
FP4_E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])


def _fp8_e4m3(codes):
    """OCP e4m3: 1 sign, 4 exponent (bias 7), 3 mantissa bits; 0x7F and 0xFF are NaN"""
    codes = codes.astype(np.int64)
    e, mant = (codes >> 3) & 0xF, codes & 7
    value = np.where(e == 0, mant / 8.0 * 2.0 ** -6, (1 + mant / 8.0) * np.exp2(e - 7.0))
    value = np.where((e == 15) & (mant == 7), np.nan, value)
    return np.where(codes & 0x80, -value, value)


def _bf16_values(halfwords):
    return (halfwords.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def _lane_operands(path, dwords):
    """(hardware k, value) of the elements one lane group holds, from its 64 x 8 fragment dwords:
    value[lane][e] is the operand at k[lane >> 4][e] of the lane's row (A) or column (B)"""
    g = np.arange(4)[:, None]
    raw = np.ascontiguousarray(dwords, dtype="<u4")
    if path == "bf16":  # k = 8 g + j
        assert not raw[:, 4:].any(), "a bf16 fragment is 4 dwords"
        return 8 * g + np.arange(8)[None, :], _bf16_values(raw[:, :4].copy().view("<u2"))
    if path == "fp8":  # K 16 g .. then 64 + 16 g ..
        e = np.arange(32)[None, :]
        return np.where(e < 16, 16 * g + e, 64 + 16 * g + (e - 16)), _fp8_e4m3(raw.view(np.uint8))
    assert not raw[:, 4:].any(), "an fp4 fragment is 4 dwords"
    packed = raw[:, :4].copy().view(np.uint8)  # K 32 g .., the even k in the low nibble
    nibbles = np.stack([packed & 0xF, packed >> 4], axis=2).reshape(64, 32)
    return 32 * g + np.arange(32)[None, :], FP4_E2M1[nibbles]


def decode_tile(path, lanes):
    """A[16][K], B[K][16], EA[16][4], EB[16][4], ACC[16][16], EXPECT[16][16] of one tile's 64 lanes"""
    kk = K_OF[path]
    lane = np.arange(64)
    rc, g = lane & 15, lane >> 4
    a, b = np.full((16, kk), np.nan), np.full((kk, 16), np.nan)
    k, va = _lane_operands(path, lanes["a"])
    _, vb = _lane_operands(path, lanes["b"])
    a[rc[:, None], k[g]] = va
    b[k[g], rc[:, None]] = vb
    ea, eb = np.zeros((16, 4), dtype=np.int64), np.zeros((16, 4), dtype=np.int64)
    ea[rc, g], eb[rc, g] = lanes["ea"], lanes["eb"]  # lane group g carries block g
    acc, expect = np.zeros((16, 16)), np.zeros((16, 16))
    rows = 4 * g[:, None] + np.arange(4)[None, :]
    acc[rows, rc[:, None]] = lanes["acc"]
    expect[rows, rc[:, None]] = lanes["expect"]
    return a, b, ea, eb, acc, expect


TILE_VARIANTS = [("bf16", False), ("fp8", False), ("fp8", True), ("fp4", False), ("fp4", True)]
TILES = [0, 1, 12345, 2**32 - 1]


# device 0's seed, the node agent's seed for device 7, and 0; a case under SEED keeps the name it had
# before the others were added
TILE_SEEDS = (SEED, 0x5EF4, 0)


def _seed_id(name, tile, seed):
    return f"{name}-{tile}" + ("" if seed == SEED else f"-seed_{seed:#x}")


PRODUCT_CASES = [pytest.param(path, scaled, tile, seed, id=_seed_id(path + ("_scaled" if scaled else ""), tile, seed))
                 for seed in TILE_SEEDS for tile in TILES for path, scaled in TILE_VARIANTS]


@pytest.mark.parametrize("path,scaled,tile,seed", PRODUCT_CASES)
def test_tile_operands_scales_and_product(path, scaled, tile, seed):
    from bacchus_gpu_controller_amd import ops

    a, b, ea, eb, acc, expect = decode_tile(path, ops.mfma_tile(path, tile, scaled=scaled, seed=seed))
    for name, x in (("A", a), ("B", b)):
        assert np.isin(x, (-1.0, 0.0, 1.0)).all(), f"{name} holds {np.unique(x)[:8]}"
    assert np.isin(ea, (-1, 0, 1)).all() and np.isin(eb, (-1, 0, 1)).all(), (ea, eb)
    if not scaled:
        assert not ea.any() and not eb.any(), (ea, eb)
    blocks = K_OF[path] // 32
    product = np.zeros((16, 16))
    for blk in range(blocks):
        ks = slice(32 * blk, 32 * blk + 32)
        product += np.exp2((ea[:, blk][:, None] + eb[:, blk][None, :]).astype(np.float64)) * (a[:, ks] @ b[ks, :])
    assert np.array_equal(acc, product), f"matrix core: {int((acc != product).sum())} of 256 elements differ from the fp64 product"
    assert np.array_equal(expect, product), f"expect(): {int((expect != product).sum())} of 256 elements differ from the fp64 product"


def operand_hash(seed, tile, r, c, which):
    """op() of gpu_diag.h on index arrays r, c"""
    inner = mix32_int(tile * GOLDEN + which)
    return trit(mix32(np.uint32(seed ^ inner) ^ (np.uint32(128) * r.astype(np.uint32) + c.astype(np.uint32))))


def _generator_index(path, k):
    """the index c that op() takes for hardware k: lane group g's element j is c = 32 g + j"""
    if path != "fp8":
        return k
    g, half, t = (k % 64) // 16, k // 64, k % 16
    return 32 * g + 16 * half + t


HASH_CASES = [pytest.param(path, tile, seed, id=_seed_id(path, tile, seed)) for seed in TILE_SEEDS for tile in TILES for path in K_OF]


@pytest.mark.parametrize("path,tile,seed", HASH_CASES)
def test_tile_operands_are_the_documented_hash(path, tile, seed):
    from bacchus_gpu_controller_amd import ops

    scaled = path != "bf16"
    a, b, ea, eb, _, _ = decode_tile(path, ops.mfma_tile(path, tile, scaled=scaled, seed=seed))
    kk = K_OF[path]
    rc, k = np.meshgrid(np.arange(16), np.arange(kk), indexing="ij")  # [rc][k]
    c = _generator_index(path, k)
    assert np.array_equal(a, operand_hash(seed, tile, rc, c, 0xA)), "A"
    want_b = operand_hash(seed, tile, k, rc, 0xB) if path == "bf16" else operand_hash(seed, tile, rc, c, 0xB)
    assert np.array_equal(b.T, want_b), "B"
    if scaled:
        rc4, blk = np.meshgrid(np.arange(16), np.arange(4), indexing="ij")
        assert np.array_equal(ea, operand_hash(seed ^ 0x5CA1E, tile, rc4, blk, 0xA)), "A scale exponents"
        assert np.array_equal(eb, operand_hash(seed ^ 0x5CA1E, tile, rc4, blk, 0xB)), "B scale exponents"


@pytest.fixture(scope="module", params=list(K_OF))
def tiles_0_to_63(request):
    """(path, A[64][16 K], B[64][16 K], EA[64][64], EB[64][64]): every operand and scale position as the
    column of its values over tiles 0..63 (the MX paths with block scales)"""
    from bacchus_gpu_controller_amd import ops

    path = request.param
    rows = [decode_tile(path, ops.mfma_tile(path, tile, scaled=path != "bf16", seed=SEED))[:4] for tile in range(64)]
    a, b, ea, eb = (np.stack([x[i].reshape(-1) for x in rows]) for i in range(4))
    return path, a, b, ea, eb


def _distinct_columns(x):
    return np.unique(x, axis=1).shape[1]


def test_tile_positions_take_distinct_value_sequences(tiles_0_to_63):
    path, a, b, _, _ = tiles_0_to_63
    positions = 16 * K_OF[path]
    assert a.shape == b.shape == (64, positions)
    assert _distinct_columns(a) == positions, f"{path}: the {positions} positions of A take {_distinct_columns(a)} distinct sequences"
    assert _distinct_columns(b) == positions, f"{path}: the {positions} positions of B take {_distinct_columns(b)} distinct sequences"
    both = _distinct_columns(np.concatenate([a, b], axis=1))
    assert both == 2 * positions, f"{path}: {2 * positions - both} sequences of A are also sequences of B"


def test_tile_operand_values_are_balanced(tiles_0_to_63):
    path, a, b, _, _ = tiles_0_to_63
    for name, x in (("A", a), ("B", b)):
        shares = _shares(x)
        print(f"{path} {name}: shares of -1, 0, 1 over 64 tiles = {[round(s, 4) for s in shares]}")
        assert all(0.30 <= s <= 0.37 for s in shares), (path, name, shares)


def test_tile_scale_positions_take_distinct_sequences(tiles_0_to_63):
    path, _, _, ea, eb = tiles_0_to_63
    if path == "bf16":
        assert not ea.any() and not eb.any()
        return
    assert _distinct_columns(ea) == 64, f"{path}: the 64 (row, block) scales of A take {_distinct_columns(ea)} distinct sequences"
    assert _distinct_columns(eb) == 64, f"{path}: the 64 (column, block) scales of B take {_distinct_columns(eb)} distinct sequences"
