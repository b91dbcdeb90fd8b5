"""The register-file diagnostic (bgc_diag_regfile): the per-SIMD march of all 512 registers of a lane in two layouts, and
the rotate of a 504-register ring, which is a moving-data check and the move rate.

* A clean run at the smallest shape and at the defaults finds nothing, marches all 512 registers, reaches every SIMD of
  every CU (the allocation of the whole file guarantees one wave per SIMD) and checks the closed-form number of words.
* The generated data: the whole file of wave 0 and of the last wave, dumped after each march fill and after the rotate's
  sweeps, equals an independent numpy recomputation word for word in every register the phase holds; the eight registers
  that the phase keeps for itself, and only those, are excluded.  A kernel that merely agreed with itself would not pass.
* One flipped bit, the top bit or all bits in every plant register, in a phase that holds it, reach every counter and name
  the register, the lane, the phase, and the CU and SIMD that the planted wave recorded for itself in the same run.
* A word planted before the sweeps travels with the ring and is reported where the host reference says it went.
* A wave made to wait 20 ms is named as the slowest (CU, SIMD), and no value changes.

Where a wave runs is the dispatcher's choice, so the truth about a planted or delayed wave comes from the same run:
regfile_data takes the plants and the delays and returns every wave's own record of its place in both launches.  Every
plant is an XOR of a value in a register; no kernel reads or writes out of bounds and every one runs to completion.  No
assertion compares with a measured rate."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED
SMALL = dict(wgs_per_cu=1, sweeps=3)
M32 = 0xFFFFFFFF
RING = 504
ROTATE = 4


@pytest.fixture(scope="module")
def ops():
    from bacchus_gpu_controller_amd import ops

    return ops


@pytest.fixture(scope="module")
def layout(ops):
    return ops.regfile_layout()


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def fill(seed, wave, inverse=False):
    """[register, lane]: what a fill writes where it writes, recomputed here"""
    wseed = mix32((seed + (wave + 1) * 0x9E3779B9) & M32)
    lane_hash = mix32((wseed + np.arange(64, dtype=np.uint64)) & M32)
    words = (lane_hash[None, :] + np.arange(512, dtype=np.uint64)[:, None] * 0x61C88647) & M32
    return ((words ^ M32) if inverse else words).astype(np.uint32)


def _held(layout, phase):
    """the registers that a phase holds a pattern in: all but its own eight"""
    held = np.ones(512, dtype=bool)
    held[layout["temp_regs"][0 if phase == ROTATE else phase >> 1]] = False
    return held


def _clean(r, waves_per_cu):
    assert r["passed"] and r["mismatches"] == 0 and r["rate_ok"], r
    assert (r["vgpr_mismatches"], r["agpr_mismatches"], r["rotate_mismatches"], r["bad_simds"]) == (0, 0, 0, 0), r
    assert r["regs_marched"] == 512 and r["ring_regs"] >= 496, r
    assert r["cus_seen"] == r["cus"] and r["simds_seen"] == 4 * r["cus"] == r["simds"], r
    waves = r["cus"] * waves_per_cu * 4
    assert r["words_checked"] == waves * 64 * (2 * 2 * (512 - 8) + r["ring_regs"]), r
    assert math.isfinite(r["mov_tops"]) and r["mov_tops"] > 0, r
    assert r["first_bad_reg"] is None and r["first_bad_cu_key"] is None and r["bad_bits"] is None, r
    assert 0 < r["simd_balance"] <= 1 and r["slowest_cu_key"] >= 0 and 0 <= r["slowest_simd"] <= 3, r


def test_clean_run_smallest(ops):
    r = ops.regfile(seed=SEED, **SMALL)
    print("regfile small:", r)
    _clean(r, 1)


def test_clean_run_defaults(ops):
    r = ops.regfile()
    print("regfile defaults:", r)
    _clean(r, ops.REGFILE_WGS_PER_CU)


@pytest.mark.parametrize("which", ["first_wave", "last_wave"])
def test_generated_data_equals_the_recomputation(ops, layout, which):
    cus = ops.regfile(seed=SEED, **SMALL)["cus"] if which == "last_wave" else 0
    wave = 4 * cus - 1 if which == "last_wave" else 0
    p0, p1 = fill(SEED, wave), fill(SEED, wave, inverse=True)
    for phase in range(4):
        r, words, march, rotate = ops.regfile_data(wave, phase, seed=SEED, **SMALL)
        assert r["mismatches"] == 0 and len(march) == len(rotate) == r["cus"] * 4, r
        held = _held(layout, phase)
        want = p1 if phase & 1 else p0
        assert (words[held] == want[held]).all(), (phase, np.argwhere(words[held] != want[held])[:4])
        assert (words[~held] == 0).all()  # never stored
    ring = layout["ring"][:RING]
    for sweeps in (1, RING + 1):
        r, words, _, _ = ops.regfile_data(wave, ROTATE, seed=SEED, wgs_per_cu=1, sweeps=sweeps)
        assert r["mismatches"] == 0 and r["rate_ok"], r
        assert (words[ring] == p0[np.roll(ring, -(sweeps % RING))]).all(), sweeps  # ring index i holds the fill of index i + sweeps
        assert (words == ops.regfile_expected(wave, ROTATE, sweeps=sweeps, seed=SEED)).all()


# every slot of REGFILE_PLANT_REGS in a phase that holds it (each layout's own registers in the other layout), both passes and
# both layouts used; lanes 0, 31, 63 and the three masks spread over the cases
PLANT_CASES = [  # slot, phase, lane, mask
    (0, 2, 0, 0x1), (1, 3, 31, 0x80000000), (2, 0, 63, 0xFFFFFFFF), (3, 1, 0, 0x80000000), (4, 0, 31, 0xFFFFFFFF), (5, 2, 63, 0x1),
    (6, 1, 31, 0x1), (7, 3, 0, 0xFFFFFFFF), (2, 2, 63, 0x80000000), (7, 0, 31, 0x80000000),
]


@pytest.mark.parametrize("slot,phase,lane,mask", PLANT_CASES, ids=[f"slot{s}_phase{p}_lane{l}_{m:#x}" for s, p, l, m in PLANT_CASES])
def test_plant_is_seen_and_named(ops, slot, phase, lane, mask):
    reg = ops.REGFILE_PLANT_REGS[slot]
    wave = 5 + 4 * slot + phase  # some wave, another in every case
    r, words, march, _ = ops.regfile_data(wave, phase, plants=[(wave, phase, slot, lane, mask)], seed=SEED, **SMALL)
    assert r["mismatches"] == 1 and not r["passed"], r
    assert (r["vgpr_mismatches"], r["agpr_mismatches"], r["rotate_mismatches"]) == ((1, 0, 0) if reg < 256 else (0, 1, 0)), r
    assert (r["first_bad_reg"], r["first_bad_lane"], r["first_bad_phase"]) == (reg, lane, phase), r
    assert int(r["bad_bits"], 16) == mask and int(r["bad_lane_mask"], 16) == 1 << lane, r
    assert (r["first_bad_cu_key"], r["first_bad_simd"]) == (march[wave]["cu_key"], march[wave]["simd"]), r
    assert r["bad_simds"] == 1 and r["rate_ok"], r
    want = fill(SEED, wave, inverse=bool(phase & 1))
    assert words[reg, lane] == want[reg, lane] ^ mask and np.count_nonzero(words[reg] != want[reg]) == 1


def test_plant_in_every_wave(ops):
    r = ops.regfile_planted([(ops.ALL_WAVES, 1, 6, 17, 0x10)], seed=SEED, **SMALL)
    assert r["bad_simds"] == r["simds_seen"] == 4 * r["cus"], r
    assert r["mismatches"] == r["agpr_mismatches"] == 4 * r["cus"] and int(r["bad_lane_mask"], 16) == 1 << 17, r


@pytest.mark.parametrize("sweeps", [1, RING - 1, RING, RING + 1])
def test_rotation_carries_a_plant(ops, sweeps):
    slot, lane, mask, wave = 4, 63, 0x00010000, 9  # v255, the last VGPR of the ring: its next place is over the v / a boundary
    plant = (wave, ROTATE, slot, lane, mask)
    r, words, _, rotate = ops.regfile_data(wave, ROTATE, plants=[plant], seed=SEED, wgs_per_cu=1, sweeps=sweeps)
    want = ops.regfile_expected(wave, ROTATE, sweeps=sweeps, plants=[plant], seed=SEED)
    clean = ops.regfile_expected(wave, ROTATE, sweeps=sweeps, seed=SEED)
    (where,), (at_lane,) = np.nonzero(want != clean)
    assert at_lane == lane and (want ^ clean)[where, lane] == mask
    assert (words == want).all()
    assert r["mismatches"] == r["rotate_mismatches"] == 1 and not r["rate_ok"] and not r["passed"], r
    assert (r["first_bad_reg"], r["first_bad_lane"], r["first_bad_phase"]) == (where, lane, ROTATE), r
    assert (r["first_bad_cu_key"], r["first_bad_simd"]) == (rotate[wave]["cu_key"], rotate[wave]["simd"]), r
    assert int(r["bad_bits"], 16) == mask and r["bad_simds"] == 1, r


def test_delayed_wave_is_the_slowest(ops):
    ticks, wave = 2_000_000, 6  # 20 ms of the 100 MHz constant clock
    base = ops.regfile(seed=SEED, wgs_per_cu=1, sweeps=64)
    r, _, _, rotate = ops.regfile_data(wave, 0, delays=[(wave, ticks)], seed=SEED, wgs_per_cu=1, sweeps=64)
    print("undelayed:", base["rotate_ms"], base["simd_balance"], "delayed:", r["rotate_ms"], r["simd_balance"])
    assert (r["slowest_cu_key"], r["slowest_simd"]) == (rotate[wave]["cu_key"], rotate[wave]["simd"]), r
    assert r["rotate_ms"] >= 20, r
    assert r["simd_balance"] < base["simd_balance"], (r, base)
    assert r["mismatches"] == 0 and r["rate_ok"] and base["mismatches"] == 0, r


def test_seeds_differ_and_run_clean(ops):
    a = ops.regfile_data(0, 0, seed=1, **SMALL)
    b = ops.regfile_data(0, 0, seed=2, **SMALL)
    assert a[0]["mismatches"] == 0 and b[0]["mismatches"] == 0 and a[0]["passed"] and b[0]["passed"]
    assert (a[1] != b[1]).any() and (a[1][8:] == fill(1, 0)[8:]).all() and (b[1][8:] == fill(2, 0)[8:]).all()


def test_plant_beyond_the_launch_is_refused(ops):
    waves = ops.regfile(seed=SEED, **SMALL)["cus"] * 4
    for call in (lambda: ops.regfile_planted([(waves, 0, 2, 0, 1)], **SMALL), lambda: ops.regfile_delayed([(waves, 1)], wgs_per_cu=1, sweeps=3),
                 lambda: ops.regfile_data(waves, 0, **SMALL)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == "regfile diag: invalid arguments: plant in a wave beyond the launch"
