"""The classic matrix-core diagnostic (bgc_diag_mfma_classic): exact fp16, int8, fp32-input and fp64
MFMA tiles with full-width operands on every CU, and each path's dense rate.

* A clean run finds nothing; its JSON has exactly these keys and types, and its rates and times are
  consistent with each other and with the documented FLOP count.
* One wrong accumulator element planted in one lane of one wave reaches that path's counter and no
  other; a planted rate-phase accumulator turns `throughput_ok` false and moves nothing else.
* The tiles the check generates are the documented ones (gpu_diag.h), fragment bits, results and the
  lane that holds each result, against a numpy reference written here from the header alone.
* The operand and result layouts the traits assume are the hardware's, independently of the
  self-check: GEMMs on caller operands (ops.gemm_dtype) against int64 numpy products, one-hot probes
  that name the K position actually read, and N(0, 1) operands within the accumulation bound.
* The verdict passes a real section with the default floors and fails under an unreachable one.

Every plant adds to an accumulator register of a named lane: no kernel reads or writes out of
bounds and every one runs to completion."""
import json
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED
ITERS = 64
ROUNDS = 4  # BGC_CLASSIC_CHECK_ROUNDS
PATHS = ["fp16", "int8", "fp32", "fp64"]
K = {"fp16": 32, "int8": 64, "fp32": 4, "fp64": 4}
FLOAT_PATHS = ["fp16", "fp32", "fp64"]
MISMATCH_KEYS = [p + "_mismatches" for p in PATHS]
RATE_KEYS = ["fp16_tflops", "int8_tops", "fp32_tflops", "fp64_tflops"]
SHAPE = {"device": int, "tiles_checked": int, "fp16_mismatches": int, "int8_mismatches": int, "fp32_mismatches": int,
         "fp64_mismatches": int, "mismatches": int, "cus_seen": int, "bad_cus": int, "bad_cu_keys": [], "fp16_tflops": float,
         "int8_tops": float, "fp32_tflops": float, "fp64_tflops": float, "rate_ms": [float] * 4, "throughput_ok": bool,
         "elapsed_ms": float, "passed": bool}
TIMES = ("fp16_tflops", "int8_tops", "fp32_tflops", "fp64_tflops", "rate_ms", "elapsed_ms")


@pytest.fixture(scope="module")
def ops():
    from bacchus_gpu_controller_amd import ops

    return ops


@pytest.fixture(scope="module")
def clean(ops):
    t0 = time.perf_counter()
    r = ops.mfma_classic(waves_per_cu=1, iters=ITERS, seed=SEED)
    r["_wall_ms"] = (time.perf_counter() - t0) * 1e3
    return r


@pytest.fixture(scope="module")
def blocks(ops):
    """256-thread blocks of a launch at one wave per CU: max(1, CUs / 4), as the header documents"""
    return max(1, ops.lds(wgs_per_cu=1, rate_iters=ITERS)["cus"] // 4)


def _shape(value, spec):
    if isinstance(spec, list):
        return isinstance(value, list) and len(value) == len(spec) and all(_shape(v, s) for v, s in zip(value, spec))
    return type(value) is spec


# ---------------------------------------------------------------------------------------------
# a. clean run

def test_clean_run(ops, clean, blocks):
    r = {k: v for k, v in clean.items() if k != "_wall_ms"}
    print("classic clean", r)
    assert r["passed"] is True and r["throughput_ok"] is True
    assert [r[k] for k in MISMATCH_KEYS] == [0, 0, 0, 0] and r["mismatches"] == 0 and r["bad_cus"] == 0 and r["bad_cu_keys"] == []
    assert list(r) == list(SHAPE)
    wrong = {k: type(r[k]).__name__ for k in SHAPE if not _shape(r[k], SHAPE[k])}
    assert not wrong, wrong
    waves = blocks * 4
    assert r["tiles_checked"] == 4 * waves * ROUNDS
    assert r["cus_seen"] == ops.mfma(waves_per_cu=1, iters=ITERS)["cus_seen"]


def test_rates_times_and_flops_agree(clean, blocks):
    r = clean
    for p, path in enumerate(PATHS):
        flops = blocks * 4 * ITERS * 4 * 2 * 16 * 16 * K[path]
        got = r[RATE_KEYS[p]] * 1e12 * r["rate_ms"][p] * 1e-3
        print(path, "rate", r[RATE_KEYS[p]], "ms", r["rate_ms"][p], "flops", got, "documented", flops)
        assert r["rate_ms"][p] > 0 and abs(got - flops) <= 1e-6 * flops
    assert sum(r["rate_ms"]) <= r["elapsed_ms"] <= r["_wall_ms"]


# ---------------------------------------------------------------------------------------------
# b. plants

def _same_but_times(a, b):
    return {k: v for k, v in a.items() if k not in TIMES and k != "_wall_ms"} == {k: v for k, v in b.items() if k not in TIMES and k != "_wall_ms"}


def test_planted_variant_without_plants_is_the_same_run(ops, clean):
    r = ops.mfma_classic_planted([], [], waves_per_cu=1, iters=ITERS, seed=SEED)
    assert list(r) == list(SHAPE) and _same_but_times(r, clean)


@pytest.mark.parametrize("delta", [1.0, float("nan")], ids=["plus_1", "nan"])
@pytest.mark.parametrize("path", PATHS)
def test_one_check_plant_reaches_its_path_only(ops, clean, blocks, path, delta):
    if path == "int8" and delta != delta:
        with pytest.raises(RuntimeError, match="classic mfma diag: invalid arguments"):  # refused on the host
            ops.mfma_classic_planted([(path, 0, 0, 0, 0, delta)], iters=ITERS, seed=SEED)
        return
    p = PATHS.index(path)
    wave, rnd, lane, i = [(0, 0, 0, 0), (blocks * 4 - 1, ROUNDS - 1, 63, 3), (5, 1, 17, 2), (2, 2, 46, 1)][p]
    r = ops.mfma_classic_planted([(path, wave, rnd, lane, i, delta)], iters=ITERS, seed=SEED)
    assert [r[k] for k in MISMATCH_KEYS] == [1 if q == p else 0 for q in range(4)], r
    assert r["mismatches"] == 1 and r["bad_cus"] == 1 and len(r["bad_cu_keys"]) == 1
    assert r["throughput_ok"] is True and r["passed"] is False
    assert r["tiles_checked"] == clean["tiles_checked"] and r["cus_seen"] == clean["cus_seen"]


@pytest.mark.parametrize("path", PATHS)
def test_one_rate_plant_turns_throughput_ok_false_and_nothing_else(ops, clean, blocks, path):
    p = PATHS.index(path)
    wave, lane, chain, i = [(0, 0, 0, 0), (blocks * 4 - 1, 63, 3, 3), (3, 21, 1, 2), (1, 40, 2, 1)][p]
    r = ops.mfma_classic_planted([], [(path, wave, lane, chain, i, 1.0)], iters=ITERS, seed=SEED)
    assert r["throughput_ok"] is False and r["passed"] is False
    assert _same_but_times(dict(r, throughput_ok=True, passed=True), clean)


def test_a_plant_beyond_the_launch_is_refused(ops, blocks):
    with pytest.raises(RuntimeError, match="classic mfma diag: invalid arguments: plant in a wave beyond the launch"):
        ops.mfma_classic_planted([("fp64", blocks * 4, 0, 0, 0, 1.0)], iters=ITERS, seed=SEED)


# ---------------------------------------------------------------------------------------------
# c. generated tiles, against gpu_diag.h

TILES = [0, 1, 12345]
RANGE = {"fp16": 512, "int8": 128, "fp32": 2047, "fp64": 1 << 25}  # |operand| <= RANGE


def _mix32(x):
    x = np.asarray(x).astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def _hashes(tile, which, rows, cols, seed=SEED):
    """h(seed, tile, r, c, which) for r < rows, c < cols"""
    r, c = np.meshgrid(np.arange(rows, dtype=np.uint32), np.arange(cols, dtype=np.uint32), indexing="ij")
    t = _mix32(np.array([(tile * 0x9E3779B9 + which) & 0xFFFFFFFF], dtype=np.uint32))[0]
    return _mix32(np.uint32(seed) ^ t ^ (np.uint32(128) * r + c))


def _wide(path, h):
    h = h.astype(np.int64)
    if path == "fp16":
        return h % 1025 - 512
    if path == "int8":
        return (h & 0xFF).astype(np.uint8).view(np.int8).astype(np.int64)
    if path == "fp32":
        return h % 4095 - 2047
    return (h >> 6) - (1 << 25)


def _reference(path, tile, seed=SEED):
    """A (16 x K), B (K x 16) and C = A B as int64, and the hashes both came from"""
    ha, hb = _hashes(tile, 0xA, 16, K[path], seed), _hashes(tile, 0xB, K[path], 16, seed)
    a, b = _wide(path, ha), _wide(path, hb)
    return a, b, a @ b, ha, hb


@pytest.mark.parametrize("path", PATHS)
def test_reference_tiles_are_not_degenerate(path):
    """Conditions on the reference alone: the operands of these tiles use their range, and no two
    operand positions of a tile share a hash.  The largest dot product stays an exact integer."""
    lo, hi = [], []
    for tile in TILES:
        a, b, c, ha, hb = _reference(path, tile)
        lo.append(min(a.min(), b.min()))
        hi.append(max(a.max(), b.max()))
        both = np.concatenate([ha.ravel(), hb.ravel()])
        assert len(np.unique(both)) == both.size, (path, tile)
        assert np.abs(a).max() <= RANGE[path] and np.abs(b).max() <= RANGE[path]
        limit = {"fp16": 1 << 24, "int8": 1 << 31, "fp32": 1 << 24, "fp64": 1 << 53}[path]
        assert (np.abs(a) @ np.abs(b)).max() < limit
    assert min(lo) < -RANGE[path] / 2 and max(hi) > RANGE[path] / 2, (path, lo, hi)


def _fragment_bits(path, values):
    """the 4 dwords of a lane's fragment holding `values` (its 8, 16 or 1 operands in order)"""
    if path == "fp16":
        raw = values.astype(np.float16).view(np.uint16)
    elif path == "int8":
        raw = values.astype(np.int8).view(np.uint8)
    elif path == "fp32":
        raw = values.astype(np.float32).view(np.uint32)
    else:
        raw = values.astype(np.float64).view(np.uint64)
    out = np.zeros(16, dtype=np.uint8)
    out[:raw.nbytes] = np.frombuffer(raw.astype(raw.dtype.newbyteorder("<")).tobytes(), dtype=np.uint8)
    return out.view("<u4")


# device 0's seed, the node agent's seed for device 7, and 0; a case under SEED keeps the name it had
# before the others were added
TILE_SEEDS = (SEED, 0x5EF4, 0)
TILE_CASES = [pytest.param(path, tile, seed, id=f"{path}-{tile}" + ("" if seed == SEED else f"-seed_{seed:#x}"))
              for seed in TILE_SEEDS for tile in TILES for path in PATHS]


@pytest.mark.parametrize("path,tile,seed", TILE_CASES)
def test_generated_tile_is_the_documented_one(ops, path, tile, seed):
    lanes = ops.mfma_classic_tile(path, tile, seed=seed)
    assert lanes.shape == (64,)
    a, b, c, _, _ = _reference(path, tile, seed)
    per = {"fp16": 8, "int8": 16, "fp32": 1, "fp64": 1}[path]
    for lane in range(64):
        g, rc = lane >> 4, lane & 15
        ks = per * g + np.arange(per)
        assert np.array_equal(lanes["a"][lane], _fragment_bits(path, a[rc, ks])), ("A", path, tile, lane)
        assert np.array_equal(lanes["b"][lane], _fragment_bits(path, b[ks, rc])), ("B", path, tile, lane)
        rows = [g + 4 * i if path == "fp64" else 4 * g + i for i in range(4)]
        want = c[rows, rc].astype(np.float64)  # exact: |c| < 2^53
        assert np.array_equal(lanes["expect"][lane], want), ("expect", path, tile, lane, lanes["expect"][lane], want)
        assert np.array_equal(lanes["acc"][lane], want), ("acc", path, tile, lane, lanes["acc"][lane], want)


# ---------------------------------------------------------------------------------------------
# d. layout, independently of the self-check

def _shapes(path):
    return [(16, 16, K[path]), (32, 48, 2 * K[path])]


@pytest.mark.parametrize("big", [False, True], ids=["one_tile", "32x48x2K"])
@pytest.mark.parametrize("path", PATHS)
def test_gemm_small_integers_match_int64(ops, path, big):
    m, n, k = _shapes(path)[big]
    rng = np.random.default_rng(1234 + PATHS.index(path))
    a, b = rng.integers(-8, 9, size=(m, k)), rng.integers(-8, 9, size=(k, n))  # asymmetric, exact in every path
    c = ops.gemm_dtype(a, b, path)
    want = a.astype(np.int64) @ b.astype(np.int64)
    bad = np.argwhere(c != want)
    assert bad.size == 0, (path, (m, n, k), len(bad), "first wrong (row, col):", bad[:8].tolist())


@pytest.mark.parametrize("big", [False, True], ids=["one_tile", "32x48x2K"])
@pytest.mark.parametrize("path", PATHS)
def test_gemm_one_hot_probes(ops, path, big):
    """A holds one 1 per row, at k = ka(r); B one 1 per column, at k = kb(c): C[r][c] = 1 exactly where
    ka(r) == kb(c).  The offsets sweep every pair (k of A, k of B); a 1 anywhere else names the K
    position of B that the hardware paired with that K position of A."""
    m, n, k = _shapes(path)[big]
    for a_off in range(0, k, m):
        for b_off in range(0, k, n):
            ka, kb = (a_off + np.arange(m)) % k, (b_off + np.arange(n)) % k
            a, b = np.zeros((m, k), dtype=np.int64), np.zeros((k, n), dtype=np.int64)
            a[np.arange(m), ka] = 1
            b[kb, np.arange(n)] = 1
            c = ops.gemm_dtype(a, b, path)
            want = (ka[:, None] == kb[None, :]).astype(np.float64)
            wrong = [f"A[{r}][k={ka[r]}] x B[k={kb[col]}][{col}] gave {c[r, col]}, expected {want[r, col]}"
                     for r, col in np.argwhere(c != want)[:8]]
            assert not wrong, (path, (m, n, k), (a_off, b_off), wrong)


@pytest.mark.parametrize("path,eps,tiny", [("fp32", 2.0 ** -24, 1e-6), ("fp64", 2.0 ** -53, 1e-6 * 2.0 ** -29)], ids=["fp32", "fp64"])
def test_gemm_normal_operands_within_the_accumulation_bound(ops, path, eps, tiny):
    """The bound of gemm_check: |C - ref| <= 4 k eps sum|a||b| + tiny, against a wider reference."""
    m, n, k = 32, 48, 64
    rng = np.random.default_rng(99)
    dt = np.float32 if path == "fp32" else np.float64
    a, b = rng.standard_normal((m, k)).astype(dt), rng.standard_normal((k, n)).astype(dt)
    c = ops.gemm_dtype(a, b, path)
    wide = np.float64 if path == "fp32" else np.longdouble
    assert np.finfo(wide).eps < eps / 4
    ref = a.astype(wide) @ b.astype(wide)
    mag = np.abs(a).astype(wide) @ np.abs(b).astype(wide)
    err, bound = np.abs(c.astype(wide) - ref), 4 * k * eps * mag + tiny
    print(path, "max err / bound", float((err / bound).max()))
    assert np.all(np.isfinite(c)) and np.all(err <= bound), (path, float((err / bound).max()))


# ---------------------------------------------------------------------------------------------
# e. verdict

def test_verdict_end_to_end(ops):
    from bacchus_gpu_controller_amd import native

    r = ops.mfma_classic(seed=SEED)  # the runner's settings
    print("classic", {k: r[k] for k in RATE_KEYS + ["rate_ms", "elapsed_ms"]})
    ok = json.loads(native().judge_diag(json.dumps({"classic": r}), "{}"))
    assert ok["failures"] == [] and ok["passed"] is True
    bad = json.loads(native().judge_diag(json.dumps({"classic": r}), json.dumps({"min_fp64_tflops": 1e9})))
    assert bad["passed"] is False and len(bad["failures"]) == 1
    assert bad["failures"][0].startswith("fp64 MFMA TFLOP/s ") and bad["failures"][0].endswith(" below floor 1000000000")
