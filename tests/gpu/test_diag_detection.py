"""The diagnostics must say "bad" when the data is bad.  Every test here plants wrong values
(one word XORed with a mask in a buffer the diagnostic allocated, or one accumulator changed by a
delta) between the phase that produces the data and the phase that checks it, and asserts that
exactly those values reach the counters: the comparison, the wave reduction, the per-CU bins, the
first-bad bookkeeping and the checksums.  Every expected value is computed here from the plant
list alone; all comparisons are exact integers.  Every kernel runs to completion and every access
stays inside its allocation.  torch stays on the CPU in this process."""
import json
import random

import pytest

pytestmark = pytest.mark.gpu

CUS = 256                 # an MI355X
GRID = CUS * 8            # blocks of the HBM stream kernels
K_BLOCK, K_UNROLL = 256, 4
NAN = float("nan")


# ---------------------------------------------------------------------------------------------
# HBM stream

HBM_SIZES = {"slab_shorter_than_a_block": (1 << 20) + 16 * 37, "ragged_slab_ends": (32 << 20) + 16 * (2048 * 3 + 5)}


def _hbm_plants(case, nbytes):
    n16 = nbytes // 16
    words = 4 * n16
    e = n16 // 2 + 7  # an element in the middle
    if case == "nothing":
        return []
    if case == "word_0":
        return [(0, 0x1)]
    if case == "last_word":
        return [(words - 1, 0x80000000)]
    if case in ("component_y", "component_z", "component_w"):
        return [(4 * e + "xyzw".index(case[-1]), 0x00010000)]
    if case == "all_four_words_of_an_element":
        return [(4 * e + c, 1 << (8 * c)) for c in range(4)]
    if case == "last_element_then_first_element":
        return [(4 * (n16 - 1) + 2, 0x4), (1, 0x4)]
    if case == "unroll_step_boundary":
        per = -(-n16 // GRID)
        assert per > K_BLOCK * K_UNROLL, "the slab must reach a second unroll step"
        beg = 1000 * per
        return [(4 * (beg + K_BLOCK * K_UNROLL - 1) + 3, 0x2), (4 * (beg + K_BLOCK * K_UNROLL), 0x2)]
    if case == "last_element":
        return [(4 * (n16 - 1) + 1, 0xFFFFFFFF)]
    if case == "random_64":
        rng = random.Random(0x5EED)
        return [(w, rng.randrange(1, 1 << 32)) for w in rng.sample(range(words), 64)]
    if case == "same_word_twice_cancels":
        return [(4 * e + 2, 0xDEADBEEF), (4 * e + 2, 0xDEADBEEF)]
    if case == "same_word_twice_different_masks":
        return [(4 * e + 2, 0xDEADBEEF), (4 * e + 2, 0xDEADBEEE)]
    raise AssertionError(case)


HBM_CASES = ["nothing", "word_0", "last_word", "component_y", "component_z", "component_w",
             "all_four_words_of_an_element", "last_element_then_first_element", "unroll_step_boundary", "last_element",
             "random_64", "same_word_twice_cancels", "same_word_twice_different_masks"]


# a slab of the smaller size ends before the first unroll step does
HBM_PARAMS = [(c, s) for s in HBM_SIZES for c in HBM_CASES
              if not (c == "unroll_step_boundary" and s == "slab_shorter_than_a_block")]


@pytest.mark.parametrize("case,size", HBM_PARAMS, ids=[f"{s}-{c}" for c, s in HBM_PARAMS])
def test_hbm_stream_counts_planted_words(case, size):
    from bacchus_gpu_controller_amd import ops

    nbytes = HBM_SIZES[size]
    plants = _hbm_plants(case, nbytes)
    net = {}
    for w, mask in plants:
        net[w] = net.get(w, 0) ^ mask
    bad = sorted(w for w, mask in net.items() if mask)
    r = ops.hbm_planted(nbytes, plants)
    assert r["bytes"] == nbytes, r
    assert r["mismatches"] == len(bad), (r, bad[:8])
    assert r["first_bad_word"] == (bad[0] if bad else None), (r, bad[:8])
    assert r["passed"] is (not bad), r


# ---------------------------------------------------------------------------------------------
# HBM walk

WALK_BYTES, WALK_CHUNK = 256 << 20, 64 << 20
WALK_CHUNKS = WALK_BYTES // WALK_CHUNK
WALK_WORDS = WALK_CHUNK // 8  # 64-bit words per chunk
_E = 2 * 123457               # the even 8-byte half of a 16-byte element
_X, _Y = 1001, 77778          # two words inside a chunk's first 2 MiB

# plants: (pass, chunk, word64 offset in the chunk, xor mask)
WALK_CASES = {
    "even_half": [(0, 1, _E, 0x1)],
    "odd_half": [(0, 1, _E + 1, 0x8000000000000000)],
    "both_halves": [(0, 1, _E, 0x10), (0, 1, _E + 1, 0x20)],
    "first_word_and_last_word": [(0, 0, 0, 0xFF), (0, WALK_CHUNKS - 1, WALK_WORDS - 1, 0xFF00)],
    "a_word_in_each_of_two_chunks": [(0, 2, 5, 0x3), (0, 0, WALK_WORDS - 3, 0x5)],
    "inverse_pass_only": [(1, 3, 4242, 0x0123456789ABCDEF)],
    "both_passes": [(0, 2, 10, 0x1), (1, 1, 3, 0x2), (1, 2, 11, 0x4)],
    # word Y holds word X's content (its address ^ key): a write that landed on the wrong word.
    # A chunk is 2 MiB aligned (asserted below), so inside its first 2 MiB addrX ^ addrY = 8X ^ 8Y.
    "misdirected_write": [(0, 1, _Y, (8 * _X) ^ (8 * _Y))],
}


@pytest.mark.parametrize("case", list(WALK_CASES))
def test_hbm_walk_reports_planted_words(case):
    from bacchus_gpu_controller_amd import ops

    plants = WALK_CASES[case]
    r = ops.hbm_walk_planted(WALK_BYTES, WALK_CHUNK, plants)
    chunks = r["chunk_list"]
    assert len(chunks) == WALK_CHUNKS == r["chunks"] and all(size == WALK_CHUNK for _, size in chunks), r
    assert r["bytes_covered"] == WALK_BYTES and r["passes"] == 2, r
    per_pass = [{}, {}]
    for p, chunk, off, mask in plants:
        addr = chunks[chunk][0] + 8 * off
        per_pass[p][addr] = per_pass[p].get(addr, 0) ^ mask
    bad = [{a: m for a, m in d.items() if m} for d in per_pass]
    first_pass = bad[0] or bad[1]  # the first failing pass names the first bad word
    first_addr = min(first_pass)
    assert r["mismatches"] == len(bad[0]) + len(bad[1]), r
    assert int(r["first_bad_addr"], 16) == first_addr, (r, hex(first_addr))
    assert int(r["first_bad_bits"], 16) == first_pass[first_addr], r
    assert r["passed"] is False, r
    if case == "misdirected_write":
        base = chunks[1][0]
        assert base % (2 << 20) == 0, hex(base)
        assert int(r["first_bad_bits"], 16) == (base + 8 * _X) ^ (base + 8 * _Y), r


def test_hbm_walk_clean():
    from bacchus_gpu_controller_amd import ops

    r = ops.hbm_walk_planted(WALK_BYTES, WALK_CHUNK, [])
    assert r["mismatches"] == 0 and r["first_bad_addr"] is None and r["first_bad_bits"] is None, r
    assert r["passes"] == 2 and r["passed"] is True, r


# ---------------------------------------------------------------------------------------------
# PCIe

PCIE_BYTES = 1 << 20


def _pcie_random():
    rng = random.Random(0x5EED)
    return [(w, rng.randrange(1, 1 << 64)) for w in rng.sample(range(PCIE_BYTES // 8), 16)]


PCIE_CASES = {
    "nothing": [],
    "word_0": [(0, 0x1)],
    "last_word": [(PCIE_BYTES // 8 - 1, 0x8000000000000000)],
    "random_16": _pcie_random(),
    "word_0_and_last_and_random": [(0, 0x1), (PCIE_BYTES // 8 - 1, 0x2)] + _pcie_random(),
}


@pytest.mark.parametrize("case", list(PCIE_CASES))
def test_pcie_round_trip_counts_planted_words(case):
    from bacchus_gpu_controller_amd import ops

    plants = PCIE_CASES[case]
    net = {}
    for w, mask in plants:
        net[w] = net.get(w, 0) ^ mask
    bad = [w for w, mask in net.items() if mask]
    r = ops.pcie_planted(PCIE_BYTES, plants)
    assert r["mismatches"] == len(bad), r
    assert r["passed"] is (not bad), r


# ---------------------------------------------------------------------------------------------
# bf16 MFMA

WPC, RATE_ITERS = 1, 64
MFMA_ROUNDS, LOWP_ROUNDS = 8, 2


def _waves(waves_per_cu):
    return max(1, CUS * waves_per_cu // 4) * 4  # 256-thread blocks of 4 waves


WAVES = _waves(WPC)

# check-phase plants: (wave, round, lane, i, delta)
MFMA_CASES = {
    "no_plant": [],
    "wave_0_lane_0": [(0, 0, 0, 0, 1.0)],
    "wave_0_lane_63": [(0, 0, 63, 3, 1.0)],  # the far end of the 64-lane reduction
    "last_wave_last_round": [(WAVES - 1, MFMA_ROUNDS - 1, 63, 3, -1.0)],
    "two_plants_in_one_wave": [(5, 1, 17, 2, 1.0), (5, 6, 40, 1, 2.0)],
    "nan_delta": [(WAVES // 2, 3, 31, 0, NAN)],
}


def _check_cu_keys(r):
    # Which CU a wave lands on changes from launch to launch and the result lists bad CUs only, so
    # the keys cannot be compared with another run's; that every bad CU is one that ran the check
    # is asserted where every wave is planted (bad_cus == cus_seen).
    assert len(r["bad_cu_keys"]) == min(r["bad_cus"], 64), r
    assert len(set(r["bad_cu_keys"])) == len(r["bad_cu_keys"]), r
    for key in r["bad_cu_keys"]:
        assert 0 <= key < 2048, r
        xcc, se, sh, cu = key >> 8, (key >> 5) & 7, (key >> 4) & 1, key & 15
        assert xcc < 8 and se < 8 and sh < 2 and cu < 16, (key, r)


@pytest.mark.parametrize("case", list(MFMA_CASES))
def test_mfma_check_counts_planted_accumulators(case):
    from bacchus_gpu_controller_amd import ops

    plants = MFMA_CASES[case]
    r = ops.mfma_planted(plants, waves_per_cu=WPC, iters=RATE_ITERS)
    assert r["mismatches"] == len(plants), r
    assert r["tiles_checked"] == WAVES * MFMA_ROUNDS, r
    assert r["bad_cus"] == len({p[0] for p in plants}), r  # a wave runs on one CU
    assert r["throughput_ok"] is True, r
    assert sum(r["xcc_waves"]) == WAVES, r
    assert r["passed"] is (not plants), r
    _check_cu_keys(r)


@pytest.mark.parametrize("waves_per_cu", [1, 4], ids=["64_blocks", "more_than_64_bad_cus"])
def test_mfma_check_plant_in_every_wave(waves_per_cu):
    """Every wave reports one mismatch, so every CU that ran the check is bad: the per-CU bins and
    the 64-entry key array at and beyond their capacity."""
    from bacchus_gpu_controller_amd import ops

    waves = _waves(waves_per_cu)
    r = ops.mfma_planted([(ops.ALL_WAVES, 2, 33, 1, 4.0)], waves_per_cu=waves_per_cu, iters=RATE_ITERS)
    assert r["mismatches"] == waves, r
    assert r["tiles_checked"] == waves * MFMA_ROUNDS, r
    assert r["bad_cus"] == r["cus_seen"], r
    assert len(r["bad_cu_keys"]) == 64, r
    assert sum(r["xcc_waves"]) == waves, r  # the key array did not overrun into its neighbours
    assert r["throughput_ok"] is True, r
    _check_cu_keys(r)


@pytest.mark.parametrize("chain", range(4))
def test_mfma_rate_phase_plant_clears_throughput_ok(chain):
    from bacchus_gpu_controller_amd import ops

    # rate-phase plants: (wave, lane, chain, i, delta)
    wave, lane = [(0, 0), (WAVES - 1, 63), (7, 16), (WAVES // 2, 47)][chain]
    r = ops.mfma_planted([], [(wave, lane, chain, chain, 1.0)], waves_per_cu=WPC, iters=RATE_ITERS)
    assert r["throughput_ok"] is False, r
    assert r["mismatches"] == 0 and r["bad_cus"] == 0 and r["bad_cu_keys"] == [], r
    assert r["tiles_checked"] == WAVES * MFMA_ROUNDS, r
    assert r["passed"] is False, r


# ---------------------------------------------------------------------------------------------
# MX low precision

LOWP_VARIANTS = ["fp8", "fp8_scaled", "fp4", "fp4_scaled"]
# (wave, round, lane, i, delta)
LOWP_EDGES = {
    "wave_0_lane_0": [(0, 0, 0, 0, 1.0)],
    "wave_0_lane_63": [(0, 0, 63, 3, 1.0)],
    "last_wave_last_round": [(WAVES - 1, LOWP_ROUNDS - 1, 63, 3, -1.0)],
    "two_plants_in_one_wave": [(5, 0, 17, 2, 1.0), (5, 1, 40, 1, 2.0)],
    "nan_delta": [(WAVES // 2, 1, 31, 0, NAN)],
}


def test_mfma_lowp_clean():
    from bacchus_gpu_controller_amd import ops

    r = ops.mfma_lowp_planted([], waves_per_cu=WPC, iters=RATE_ITERS)
    assert r["mismatches"] == 0 and r["bad_cus"] == 0 and r["throughput_ok"] is True and r["passed"] is True, r
    assert r["tiles_checked"] == 4 * WAVES * LOWP_ROUNDS, r


@pytest.mark.parametrize("variant", LOWP_VARIANTS)
@pytest.mark.parametrize("edge", list(LOWP_EDGES))
def test_mfma_lowp_check_counts_planted_accumulators(edge, variant):
    from bacchus_gpu_controller_amd import ops

    plants = [(variant,) + p for p in LOWP_EDGES[edge]]
    r = ops.mfma_lowp_planted(plants, waves_per_cu=WPC, iters=RATE_ITERS)
    for v in LOWP_VARIANTS:  # only that variant's counter moves: the four bin offsets
        assert r[v + "_mismatches"] == (len(plants) if v == variant else 0), (v, r)
    assert r["mismatches"] == len(plants), r
    assert r["bad_cus"] == 1, r
    assert r["tiles_checked"] == 4 * WAVES * LOWP_ROUNDS, r
    assert r["throughput_ok"] is True and r["passed"] is False, r
    _check_cu_keys(r)


def test_mfma_lowp_plant_in_every_wave_of_two_variants():
    """Every wave reports one mismatch in the first and in the last variant's bins, so every CU is
    bad in both and is still counted once; the 64-entry key array beyond its capacity."""
    from bacchus_gpu_controller_amd import ops

    waves = _waves(4)
    plants = [("fp8", ops.ALL_WAVES, 1, 33, 1, 4.0), ("fp4_scaled", ops.ALL_WAVES, 0, 2, 3, -2.0)]
    r = ops.mfma_lowp_planted(plants, waves_per_cu=4, iters=RATE_ITERS)
    assert r["fp8_mismatches"] == r["fp4_scaled_mismatches"] == waves, r
    assert r["fp8_scaled_mismatches"] == r["fp4_mismatches"] == 0, r
    assert r["mismatches"] == 2 * waves, r
    assert r["tiles_checked"] == 4 * waves * LOWP_ROUNDS, r
    assert r["bad_cus"] == r["cus_seen"], r
    assert len(r["bad_cu_keys"]) == 64, r
    assert r["throughput_ok"] is True, r
    _check_cu_keys(r)


def test_mfma_lowp_one_plant_in_each_variant_lands_in_its_own_bin():
    """All four check launches of one run at once: each variant's plant, at a place of its own, reaches
    that variant's counter and no other."""
    from bacchus_gpu_controller_amd import ops

    places = [(0, 0, 0, 0), (WAVES - 1, LOWP_ROUNDS - 1, 63, 3), (5, 1, 17, 2), (WAVES // 2, 0, 46, 1)]
    plants = [(v,) + at + (1.0,) for v, at in zip(LOWP_VARIANTS, places)]
    r = ops.mfma_lowp_planted(plants, waves_per_cu=WPC, iters=RATE_ITERS)
    for v in LOWP_VARIANTS:
        assert r[v + "_mismatches"] == 1, (v, r)
    assert r["mismatches"] == 4, r
    assert r["tiles_checked"] == 4 * (WAVES // 4) * 4 * LOWP_ROUNDS, r  # variants x blocks x waves of a block x rounds
    assert r["throughput_ok"] is True and r["passed"] is False, r
    _check_cu_keys(r)


# what a run reports besides its rates and times
_MFMA_COUNTS = ["tiles_checked", "cus_seen", "bad_cus", "xccs_seen", "mismatches", "throughput_ok"]
_LOWP_COUNTS = ["tiles_checked", "cus_seen", "bad_cus", "mismatches", "throughput_ok"] + [v + "_mismatches" for v in LOWP_VARIANTS]


def test_mfma_planted_without_plants_is_the_production_run():
    from bacchus_gpu_controller_amd import ops

    clean = ops.mfma(waves_per_cu=WPC, iters=RATE_ITERS)
    r = ops.mfma_planted([], [], waves_per_cu=WPC, iters=RATE_ITERS)
    assert list(r) == list(clean), (r, clean)
    assert {k: r[k] for k in _MFMA_COUNTS} == {k: clean[k] for k in _MFMA_COUNTS}, (r, clean)
    assert sum(r["xcc_waves"]) == sum(clean["xcc_waves"]) == WAVES, (r, clean)
    assert r["bad_cu_keys"] == clean["bad_cu_keys"] == [] and r["passed"] is clean["passed"] is True, (r, clean)


def test_mfma_lowp_planted_without_plants_is_the_production_run():
    from bacchus_gpu_controller_amd import ops

    clean = ops.mfma_lowp(waves_per_cu=WPC, iters=RATE_ITERS)
    r = ops.mfma_lowp_planted([], [], waves_per_cu=WPC, iters=RATE_ITERS)
    assert list(r) == list(clean), (r, clean)
    assert {k: r[k] for k in _LOWP_COUNTS} == {k: clean[k] for k in _LOWP_COUNTS}, (r, clean)
    assert r["bad_cu_keys"] == clean["bad_cu_keys"] == [] and r["passed"] is clean["passed"] is True, (r, clean)


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_mfma_lowp_rate_phase_plant_clears_throughput_ok(fmt):
    from bacchus_gpu_controller_amd import ops

    # rate-phase plants: (format, wave, lane, chain, i, delta)
    r = ops.mfma_lowp_planted([], [(fmt, WAVES - 1, 63, 3, 3, 1.0)], waves_per_cu=WPC, iters=RATE_ITERS)
    assert r["throughput_ok"] is False and r["passed"] is False, r
    assert r["mismatches"] == 0 and r["bad_cus"] == 0, r


# ---------------------------------------------------------------------------------------------
# The rate phases at the most iterations their entry points take: 2^18 for bf16 (K = 32) and 2^16 for
# the MX and the classic paths (K up to 128), where K * iters reaches 2^23.  The accumulators then
# hold integers up to 2^23 + 3, the largest at which the fp32 comparison acc == iters * tile + c is
# still exact and at which a delta of 1 is still representable, so a clean run must pass and one
# wrong accumulator must still be seen.  One wave per CU keeps every launch at a few milliseconds.

LIMIT_ITERS = {"mfma": 1 << 18, "lowp": 1 << 16, "classic": 1 << 16}
CLASSIC_PATHS = ["fp16", "int8", "fp32", "fp64"]
_FAR_END = (WAVES - 1, 63, 3, 3, 1.0)  # rate plant: the last wave, lane 63, chain 3, element 3


def _limit_run(ops, family, planted=None):
    """the family's run at its limit, with the far-end plant in the rate launch of format or path `planted`"""
    if family == "mfma":
        r = ops.mfma_planted([], [_FAR_END] if planted else [], waves_per_cu=WPC, iters=LIMIT_ITERS[family])
        flops = WAVES * LIMIT_ITERS[family] * 4 * 2 * 16 * 16 * 32
        rate_ms, counters = [flops / (r["tflops"] * 1e12) * 1e3], ["mismatches"]
    elif family == "lowp":
        r = ops.mfma_lowp_planted([], [(planted,) + _FAR_END] if planted else [], waves_per_cu=WPC, iters=LIMIT_ITERS[family])
        flops = WAVES * LIMIT_ITERS[family] * 4 * 2 * 16 * 16 * 128
        rate_ms = [flops / (r[f + "_tflops"] * 1e12) * 1e3 for f in ("fp8", "fp4")]
        counters = ["mismatches"] + [v + "_mismatches" for v in LOWP_VARIANTS]
    else:
        r = ops.mfma_classic_planted([], [(planted,) + _FAR_END] if planted else [], waves_per_cu=WPC, iters=LIMIT_ITERS[family])
        rate_ms, counters = r["rate_ms"], ["mismatches"] + [p + "_mismatches" for p in CLASSIC_PATHS]
    print("rate phase at its limit:", family, planted or "clean", "iters", LIMIT_ITERS[family], "rate_ms", rate_ms, "elapsed_ms",
          r["elapsed_ms"])
    return r, counters


@pytest.mark.parametrize("family", list(LIMIT_ITERS))
def test_rate_phase_at_its_iteration_limit_is_clean(family):
    from bacchus_gpu_controller_amd import ops

    r, counters = _limit_run(ops, family)
    assert r["throughput_ok"] is True and r["passed"] is True, r
    assert [r[k] for k in counters] == [0] * len(counters) and r["bad_cus"] == 0, r


LIMIT_PLANTS = [("mfma", "bf16"), ("lowp", "fp8"), ("lowp", "fp4")] + [("classic", p) for p in CLASSIC_PATHS]


@pytest.mark.parametrize("family,planted", LIMIT_PLANTS, ids=[f"{f}-{p}" for f, p in LIMIT_PLANTS])
def test_rate_phase_at_its_iteration_limit_sees_a_delta_of_one(family, planted):
    from bacchus_gpu_controller_amd import ops

    r, counters = _limit_run(ops, family, planted)
    assert r["throughput_ok"] is False and r["passed"] is False, r
    assert [r[k] for k in counters] == [0] * len(counters) and r["bad_cus"] == 0, r


# ---------------------------------------------------------------------------------------------
# GEMM soak

# (m, n, k), BGC_SOAK_TILE, (tile, kernel)
SOAK_SHAPES = {
    "pingpong": ((256, 256, 128), None, (256, "pingpong")),
    "2buf_256": ((256, 512, 192), None, (256, "2buf")),
    "2buf_128": ((256, 256, 128), "128", (128, "2buf")),
}


def _soak_cases(m, n):
    # launches, plants (launch, row, col, delta), expected (row mismatches, column mismatches)
    return {
        "first_element": (1, [(0, 0, 0, 1.0)], (1, 1)),
        "last_element": (1, [(0, m - 1, n - 1, 1.0)], (1, 1)),
        # the row checksum cannot see it: why both checksums exist
        "plus_and_minus_in_one_row": (1, [(0, 100, 3, 1.0), (0, 100, n - 70, -1.0)], (0, 2)),
        # far below the 0.5 that rounding to an integer hides; exact in fp32 next to any |C| <= k
        "sub_half_delta": (1, [(0, 131, 65, 2.0 ** -10)], (1, 1)),
        "nan": (1, [(0, m - 17, 129, NAN)], (1, 1)),
        "first_launch_of_two": (2, [(0, 7, 200, 1.0)], (1, 1)),
        "last_launch_of_two": (2, [(1, 200, 7, 1.0)], (1, 1)),
    }


@pytest.mark.parametrize("shape", list(SOAK_SHAPES))
@pytest.mark.parametrize("case", list(_soak_cases(256, 256)))
def test_soak_checksums_see_planted_elements(monkeypatch, case, shape):
    from bacchus_gpu_controller_amd import ops

    (m, n, k), tile_env, kernel = SOAK_SHAPES[shape]
    if tile_env:
        monkeypatch.setenv("BGC_SOAK_TILE", tile_env)
    launches, plants, (rows, cols) = _soak_cases(m, n)[case]
    r = ops.gemm_soak_planted(m, n, k, launches, plants)
    assert (r["tile"], r["kernel"]) == kernel, r
    assert (r["row_mismatches"], r["col_mismatches"]) == (rows, cols), r
    assert r["passed"] is False, r


@pytest.mark.parametrize("shape", list(SOAK_SHAPES))
def test_soak_clean_and_unverified_launch(monkeypatch, shape):
    from bacchus_gpu_controller_amd import ops

    (m, n, k), tile_env, kernel = SOAK_SHAPES[shape]
    if tile_env:
        monkeypatch.setenv("BGC_SOAK_TILE", tile_env)
    r = ops.gemm_soak_planted(m, n, k, 2, [])
    assert (r["tile"], r["kernel"]) == kernel, r
    assert (r["row_mismatches"], r["col_mismatches"]) == (0, 0) and r["passed"] is True, r
    # only the first and the last launch are verified: a plant on another one is refused, not ignored
    with pytest.raises((RuntimeError, ValueError), match="invalid arguments"):
        ops.gemm_soak_planted(m, n, k, 3, [(1, 0, 0, 1.0)])


# ---------------------------------------------------------------------------------------------
# end to end: planted results through the verdict the node agent acts on

def test_planted_results_fail_the_verdict():
    from bacchus_gpu_controller_amd import native, ops

    nbytes = HBM_SIZES["slab_shorter_than_a_block"]
    hbm = ops.hbm_planted(nbytes, [(5, 0x1), (6, 0x1), (nbytes // 4 - 1, 0x1)])
    mfma = ops.mfma_planted([(3, 0, 9, 0, 1.0)], waves_per_cu=WPC, iters=RATE_ITERS)
    judged = json.loads(native().judge_diag(json.dumps({"hbm": hbm, "mfma": mfma})))
    assert judged["passed"] is False, judged
    assert "HBM pattern mismatches: 3" in judged["failures"], judged["failures"]
    assert "MFMA tile mismatches on 1 CU(s)" in judged["failures"], judged["failures"]
