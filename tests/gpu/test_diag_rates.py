"""The measurement side of the GPU diagnostics: the rates and times a verdict is judged on.

* Work counts: every reported rate, multiplied back by the time it was measured over, must give the
  FLOPs or bytes that gpu_diag.h documents for that diagnostic.  The counts are written out here.
* A second clock: no diagnostic's device time may exceed the host's wall time around the call; the
  matrix-core rate must grow with the work as the host's wall time does; and the waves' own time on
  the constant clock must sit just under the event time of their launch.
* Delay plants (ops.mfma_delayed, ops.burn_delayed): chosen waves or launches are made slow by a
  known time, and that time must reach xcc_wave_us, xcc_balance, tflops, sustain and the verdict.
* The walk's time budget must end a walk.

The identities hold up to the rounding of a few fp32 millisecond values (event times have a 24-bit
mantissa, 6e-8 relative each), hence REL = 1e-5.  The measured margins are in
profiles/diag_rates/README.md with the runs behind them.  torch stays on the CPU in this process."""
import json
import time

import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
CUS = 256  # an MI355X
REL = 1e-5
SEED = 0x5EED

# profiles/diag_rates/README.md: twice the worst deviation of 36 clean runs (two processes) on the MI355X
SCALING_MARGIN = 0.0145     # growth of the host's wall time against growth of flops / tflops, relative (worst 0.00725)
WAVE_CLOSE_MARGIN = 0.083   # (flops / tflops - xcc_wave_us) / (flops / tflops), every XCC (worst 0.0412)
DELAY_EXCESS_US = 20.4      # xcc_wave_us - 5000 with every wave delayed by 5 ms (worst 10.19)
# The event clock and the constant clock are two crystal-derived clocks: they may differ by parts per
# million, so a bound of one by the other gets 1e-4 of room, far below anything a wrong factor gives.
SKEW = 1e-4


def _waves(waves_per_cu):
    return max(1, CUS * waves_per_cu // 4) * 4  # 256-thread blocks of 4 waves


def _mfma_flops(waves_per_cu, iters, k):
    """Throughput phase (gpu_diag.h): every wave runs `iters` iterations of 4 chained 16x16xk MFMAs,
    2 FLOPs per multiply-add."""
    return _waves(waves_per_cu) * iters * 4 * 2 * 16 * 16 * k


def _timed(call):
    """(result, the host's wall time around the call in ms); the device time inside cannot exceed it."""
    t0 = time.perf_counter()
    r = call()
    wall_ms = (time.perf_counter() - t0) * 1e3
    assert r["elapsed_ms"] <= wall_ms, (r["elapsed_ms"], wall_ms, r)
    return r, wall_ms


def _burn(dtype, duration_ms):
    from bacchus_gpu_controller_amd import native

    n = native()
    return json.loads(n.diag_burn(n.gpu_backend("mock"), 0, 0, duration_ms, SEED, dtype))


# ---------------------------------------------------------------------------------------------
# a. work counts against the header, and b. the host's wall clock around every call

@pytest.mark.parametrize("m,n,k", [(128, 384, 64), (512, 768, 1024)])
def test_soak_rate_times_time_is_the_gemms_flops(m, n, k):
    from bacchus_gpu_controller_amd import ops

    launches = 3
    r, _ = _timed(lambda: ops.gemm_soak(m=m, n=n, k=k, launches=launches))
    print("soak", (m, n, k), r["tflops_mean"], r["tflops_best"], r["elapsed_ms"])
    assert r["tflops_mean"] * r["elapsed_ms"] * 1e9 == pytest.approx(2 * m * n * k * launches, rel=REL), r
    assert r["tflops_best"] >= r["tflops_mean"] * (1 - REL), r
    assert r["passed"] is True, r


@pytest.mark.parametrize("nbytes", [64 * MIB + 16, MIB], ids=["64MiB+16", "1MiB"])
def test_hbm_rates_account_for_the_elapsed_time(nbytes):
    """A fill writes `bytes`, a copy reads and writes them (2 * bytes), a check reads them."""
    from bacchus_gpu_controller_amd import ops

    def phases_s(r):
        b = r["bytes"]
        return b / (r["write_gbps"] * 1e9) + 2 * b / (r["copy_gbps"] * 1e9) + b / (r["read_gbps"] * 1e9)

    r, _ = _timed(lambda: ops.hbm(nbytes=nbytes, iters=1))
    print("hbm", nbytes, r["write_gbps"], r["copy_gbps"], r["read_gbps"], r["elapsed_ms"])
    assert r["bytes"] == nbytes and r["mismatches"] == 0, r
    assert phases_s(r) == pytest.approx(r["elapsed_ms"] * 1e-3, rel=REL), r
    # over several iterations the rates are the best ones: their times are at most the mean iteration's
    r3, _ = _timed(lambda: ops.hbm(nbytes=nbytes, iters=3))
    assert r3["iters"] == 3 and r3["mismatches"] == 0, r3
    assert phases_s(r3) <= r3["elapsed_ms"] * 1e-3 / 3 * (1 + REL), r3


def test_pcie_rates_account_for_the_elapsed_time():
    """One upload, one download, and both at once on two streams (2 * bytes over the longer of the two)."""
    from bacchus_gpu_controller_amd import ops

    nbytes = 16 * MIB
    r, _ = _timed(lambda: ops.pcie(nbytes=nbytes, iters=1))
    print("pcie", r["h2d_gbps"], r["d2h_gbps"], r["bidir_gbps"], r["elapsed_ms"])
    assert r["bytes"] == nbytes and r["mismatches"] == 0, r
    phases_s = nbytes / (r["h2d_gbps"] * 1e9) + nbytes / (r["d2h_gbps"] * 1e9) + 2 * nbytes / (r["bidir_gbps"] * 1e9)
    assert phases_s == pytest.approx(r["elapsed_ms"] * 1e-3, rel=REL), r


def test_mfma_rate_window_lies_inside_the_elapsed_time():
    from bacchus_gpu_controller_amd import ops

    r, _ = _timed(lambda: ops.mfma(waves_per_cu=4, iters=4096))
    assert sum(r["xcc_waves"]) == _waves(4) and r["passed"] is True, r
    rate_ms = _mfma_flops(4, 4096, 32) / (r["tflops"] * 1e12) * 1e3
    print("mfma", r["tflops"], rate_ms, r["elapsed_ms"])
    assert 0 < rate_ms < r["elapsed_ms"], (rate_ms, r)


def test_lowp_rate_windows_lie_inside_the_elapsed_time():
    from bacchus_gpu_controller_amd import ops

    r, _ = _timed(lambda: ops.mfma_lowp(waves_per_cu=4, iters=4096))
    assert r["passed"] is True, r
    flops = _mfma_flops(4, 4096, 128)
    fp8_ms, fp4_ms = flops / (r["fp8_tflops"] * 1e12) * 1e3, flops / (r["fp4_tflops"] * 1e12) * 1e3
    print("lowp", r["fp8_tflops"], r["fp4_tflops"], fp8_ms, fp4_ms, r["elapsed_ms"])
    assert fp8_ms > 0 and fp4_ms > 0 and fp8_ms + fp4_ms < r["elapsed_ms"], (fp8_ms, fp4_ms, r)


def _check_burn_summary(r, duration_ms):
    assert r["elapsed_ms"] >= duration_ms, r
    assert r["tflops_min"] <= r["tflops_first"] <= r["tflops_max"], r
    assert r["tflops_min"] <= r["tflops_last"] <= r["tflops_max"], r
    assert r["tflops_mean"] <= r["tflops_max"], r
    assert r["launches"] >= 2, r
    assert r["sustain"] == pytest.approx(r["tflops_last"] / r["tflops_max"], rel=1e-12), r


@pytest.mark.parametrize("dtype", ["bf16", "fp8", "fp4"])
def test_burn_summary_is_consistent(dtype):
    duration_ms = 300
    r, _ = _timed(lambda: _burn(dtype, duration_ms))
    print("burn", dtype, {k: r[k] for k in ("launches", "elapsed_ms", "tflops_mean", "tflops_min", "tflops_first", "tflops_last",
                                            "tflops_max", "sustain")})
    assert r["dtype"] == dtype and r["mismatches"] == 0, r
    _check_burn_summary(r, duration_ms)


# ---------------------------------------------------------------------------------------------
# b. a second clock for the matrix-core rate

SCALE_ITERS = 16384  # and 16 times that, the most bgc_diag_mfma takes
SCALE_REPEATS = 3


def _fastest(ops, iters):
    """(host wall ms, rate window ms, result) of the fastest of SCALE_REPEATS runs by each clock"""
    walls, windows = [], []
    for _ in range(SCALE_REPEATS):
        r, wall_ms = _timed(lambda: ops.mfma(waves_per_cu=4, iters=iters))
        assert r["passed"] is True, r
        walls.append(wall_ms)
        windows.append(_mfma_flops(4, iters, 32) / (r["tflops"] * 1e12) * 1e3)
    return min(walls), min(windows), r


def scaling_deviation(ops):
    """Sixteen times the iterations: the host's wall time and the rate window (flops / tflops) must grow
    by the same time, whatever the call costs around the launch.  Relative difference of the two growths."""
    wall_1, window_1, _ = _fastest(ops, SCALE_ITERS)
    wall_16, window_16, _ = _fastest(ops, 16 * SCALE_ITERS)
    grow_wall, grow_window = wall_16 - wall_1, window_16 - window_1
    return abs(grow_wall - grow_window) / grow_window, (wall_1, wall_16, window_1, window_16)


def test_mfma_rate_window_grows_as_the_host_wall_time_does():
    from bacchus_gpu_controller_amd import ops

    deviation, times = scaling_deviation(ops)
    print("scaling", deviation, times)
    assert times[3] > 8 * times[2], times  # the window did grow: 16 times the work
    assert deviation < SCALING_MARGIN, (deviation, times)


def wave_clock_gaps(ops, iters=16 * SCALE_ITERS // 4):
    """At 4 waves per CU every wave is resident from the start of the launch to its end, so the mean wave
    time of every XCC on the constant clock is at most the launch's event time, and close to it.
    ((window - xcc_wave_us) / window per XCC that ran waves, the result)"""
    r = ops.mfma(waves_per_cu=4, iters=iters)
    window_us = _mfma_flops(4, iters, 32) / (r["tflops"] * 1e12) * 1e6
    return [(window_us - us) / window_us for us, w in zip(r["xcc_wave_us"], r["xcc_waves"]) if w], r


def test_wave_times_on_the_constant_clock_sit_just_under_the_event_time():
    from bacchus_gpu_controller_amd import ops

    gaps, r = wave_clock_gaps(ops)
    print("wave clock gaps", gaps, r["tflops"], r["xcc_wave_us"])
    assert len(gaps) == 8 and sum(r["xcc_waves"]) == _waves(4), r
    assert min(gaps) >= -SKEW, (gaps, r)                # no wave ran longer than its launch
    assert max(gaps) < WAVE_CLOSE_MARGIN, (gaps, r)     # and the launch was the waves and little else


# ---------------------------------------------------------------------------------------------
# c. delays reach the numbers

WPC, ITERS = 1, 64
WAVES = _waves(WPC)
TICKS, DELAY_US = 500000, 5000.0  # of the documented 100 MHz


def _balance(r):
    ran = [us for us, w in zip(r["xcc_wave_us"], r["xcc_waves"]) if w]
    return min(ran) / max(ran)


def delayed_everywhere(ops):
    return ops.mfma_delayed([(ops.ALL_WAVES, TICKS)], waves_per_cu=WPC, iters=ITERS)


def test_clean_launch_is_far_shorter_than_the_delay():
    from bacchus_gpu_controller_amd import ops

    r = ops.mfma_delayed([], waves_per_cu=WPC, iters=ITERS)  # an empty list: the production run
    assert r["passed"] is True and sum(r["xcc_waves"]) == WAVES, r
    assert 0 < max(r["xcc_wave_us"]) < DELAY_US / 10, r
    assert _mfma_flops(WPC, ITERS, 32) / (r["tflops"] * 1e12) * 1e6 < DELAY_US / 10, r
    assert r["xcc_balance"] == pytest.approx(_balance(r), rel=1e-12), r


def test_delay_of_every_wave_reaches_wave_times_and_rate():
    from bacchus_gpu_controller_amd import ops

    r = delayed_everywhere(ops)
    ran = [us for us, w in zip(r["xcc_wave_us"], r["xcc_waves"]) if w]
    window_us = _mfma_flops(WPC, ITERS, 32) / (r["tflops"] * 1e12) * 1e6
    print("delayed everywhere", r["xcc_wave_us"], window_us, r["tflops"])
    assert sum(r["xcc_waves"]) == WAVES and len(ran) == 8, r
    # every wave waited 500000 ticks inside its own timing: exact, and it pins ticks -> microseconds
    assert all(us >= DELAY_US for us in ran), r
    assert all(us == 0 for us, w in zip(r["xcc_wave_us"], r["xcc_waves"]) if not w), r
    assert window_us >= 0.98 * DELAY_US, (window_us, r)
    assert r["throughput_ok"] is True and r["mismatches"] == 0 and r["passed"] is True, r  # the values are untouched
    assert r["xcc_balance"] == pytest.approx(_balance(r), rel=1e-12), r
    assert max(ran) - DELAY_US < DELAY_EXCESS_US, r


@pytest.mark.parametrize("residue", [0, 7])
def test_delay_of_one_xcc_reaches_its_bin_and_the_verdict(residue):
    """Blocks are dealt round-robin over the 8 XCDs, so the blocks b with b % 8 == residue run on one XCC:
    delaying their waves must slow exactly one bin."""
    from bacchus_gpu_controller_amd import native, ops

    blocks = [b for b in range(WAVES // 4) if b % 8 == residue]
    delays = [(4 * b + w, TICKS) for b in blocks for w in range(4)]
    assert len(delays) == 32
    r = ops.mfma_delayed(delays, waves_per_cu=WPC, iters=ITERS)
    print("delayed blocks", residue, r["xcc_waves"], r["xcc_wave_us"], r["xcc_balance"])
    assert sum(r["xcc_waves"]) == WAVES, r
    assert sum(w * us for w, us in zip(r["xcc_waves"], r["xcc_wave_us"])) >= 32 * DELAY_US, r
    assert r["throughput_ok"] is True and r["mismatches"] == 0, r
    slow = [x for x in range(8) if r["xcc_wave_us"][x] >= DELAY_US]
    assert len(slow) == 1 and r["xcc_waves"][slow[0]] == 32, r
    assert all(r["xcc_wave_us"][x] < DELAY_US / 10 for x in range(8) if x != slow[0]), r
    assert r["xcc_balance"] == pytest.approx(_balance(r), rel=1e-12) and r["xcc_balance"] < 0.85, r
    judged = json.loads(native().judge_diag(json.dumps({"mfma": r})))
    assert judged["passed"] is False and any("XCC balance" in f for f in judged["failures"]), judged["failures"]


def test_delay_in_a_wave_beyond_the_launch_is_refused():
    from bacchus_gpu_controller_amd import ops

    with pytest.raises(RuntimeError, match="invalid arguments: plant in a wave beyond the launch"):
        ops.mfma_delayed([(0, TICKS), (WAVES, TICKS)], waves_per_cu=WPC, iters=ITERS)
    r = ops.mfma_delayed([(WAVES - 1, 1000)], waves_per_cu=WPC, iters=ITERS)  # the last wave is inside
    assert r["passed"] is True, r


BURN_MS, BURN_TICKS = 300, 4000000  # 40 ms, against launches retuned to about 10 ms


@pytest.mark.parametrize("dtype", ["bf16", "fp8", "fp4"])
def test_delayed_launches_sag_the_burn(dtype):
    from bacchus_gpu_controller_amd import native, ops

    clean = ops.burn_delayed(BURN_MS, 1 << 30, BURN_TICKS, dtype=dtype)  # a launch the burn never reaches
    slow = ops.burn_delayed(BURN_MS, 2, BURN_TICKS, dtype=dtype)
    keys = ("launches", "elapsed_ms", "tflops_mean", "tflops_min", "tflops_first", "tflops_last", "tflops_max", "sustain")
    print("burn clean", dtype, {k: clean[k] for k in keys})
    print("burn slow", dtype, {k: slow[k] for k in keys})
    assert clean["dtype"] == slow["dtype"] == dtype, (clean, slow)
    assert clean["mismatches"] == 0 and clean["sustain"] >= 0.8, clean
    _check_burn_summary(clean, BURN_MS)
    _check_burn_summary(slow, BURN_MS)
    assert slow["launches"] > 2 and slow["mismatches"] == 0, slow
    assert slow["sustain"] < 0.5, slow
    assert clean["tflops_min"] <= slow["tflops_first"] <= clean["tflops_max"], (clean, slow)
    judged = json.loads(native().judge_diag(json.dumps({"burn": slow})))
    assert judged["passed"] is False and any("MFMA rate sagged" in f for f in judged["failures"]), judged["failures"]
    judged = json.loads(native().judge_diag(json.dumps({"burn": clean})))
    assert not any("MFMA rate sagged" in f for f in judged["failures"]), judged["failures"]


# ---------------------------------------------------------------------------------------------
# d. the walk's time budget

# At 0.001 of the free 308 GB a whole walk of two passes takes 0.55 ms on the MI355X and never meets a
# budget of 1 ms.  A pass writes and reads what it covers; at 0.03 that moves 18 GB, which takes 2.3 ms
# at HBM3E's peak of 8 TB/s, more than twice the budget at a rate the fill and the check cannot reach.
WALK_FRACTION = 0.03


def test_walk_budget_ends_the_walk_after_the_first_pass():
    from bacchus_gpu_controller_amd import ops

    r, _ = _timed(lambda: ops.hbm_walk(fraction=WALK_FRACTION, chunk_bytes=64 * MIB, budget_ms=1))
    print("walk, 1 ms", r["elapsed_ms"], r["alloc_ms"], r["bytes_covered"])
    assert r["budget_hit"] is True and r["passes"] == 1 and r["passed"] is False, r
    assert r["mismatches"] == 0 and r["bytes_covered"] > 0, r
    r, _ = _timed(lambda: ops.hbm_walk(fraction=WALK_FRACTION, chunk_bytes=64 * MIB, budget_ms=20000))
    assert r["budget_hit"] is False and r["passes"] == 2 and r["passed"] is True, r
    assert r["mismatches"] == 0 and r["bytes_covered"] > 0, r
