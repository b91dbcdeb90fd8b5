"""The register-file check's host reference (native/gpu/hip/regfile_ref.h) through ops.regfile_layout and
ops.regfile_expected, without a GPU: the layouts' conditions (both march layouts leave out only their own eight registers
and together cover all 512; the ring holds at least 496 registers, each once; every plant slot is held by the phases it
may name) and the pattern, the rotation and a plant's journey against a numpy recomputation written here."""
import numpy as np
import pytest

from bacchus_gpu_controller_amd import ops

SEEDS = (0x5EED, 0, 0xFFFFFFFF)
M32 = 0xFFFFFFFF


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def fill(seed, wave, inverse=False):
    """[register, lane]: what a fill writes where it writes"""
    wseed = mix32((seed + (wave + 1) * 0x9E3779B9) & M32)
    lane_hash = mix32((wseed + np.arange(64, dtype=np.uint64)) & M32)
    words = (lane_hash[None, :] + np.arange(512, dtype=np.uint64)[:, None] * 0x61C88647) & M32
    return ((words ^ M32) if inverse else words).astype(np.uint32)


@pytest.fixture(scope="module")
def layout():
    return ops.regfile_layout()


def test_layouts_cover_every_register(layout):
    assert (layout["regs"], layout["lanes"], layout["temps"], layout["plant_slots"]) == (512, 64, 8, 8)
    marched = layout["marched"].astype(bool)
    for lay in range(2):
        temps = set(int(t) for t in layout["temp_regs"][lay])
        assert len(temps) == 8 and all(0 <= t < 256 for t in temps)  # temporaries are VGPRs
        assert set(np.flatnonzero(~marched[lay])) == temps  # a layout leaves out its own temporaries and nothing else
    assert (marched[0] | marched[1]).all()  # the union is all 512
    assert not set(layout["temp_regs"][0]) & set(layout["temp_regs"][1])


def test_ring_holds_at_least_496_registers_once_each(layout):
    n = int(layout["ring_regs"])
    ring = layout["ring"][:n]
    assert n >= 496 and len(set(ring.tolist())) == n and ring.min() >= 0 and ring.max() < 512
    assert not set(ring.tolist()) & set(layout["temp_regs"][0].tolist())  # the rotate keeps layout 0's temporaries


def test_plant_slots(layout):
    regs = layout["plant_regs"].tolist()
    assert tuple(regs) == ops.REGFILE_PLANT_REGS
    assert {0, 255, 256, 511} <= set(regs) and any(0 < r < 255 for r in regs) and any(256 < r < 511 for r in regs)
    ring = set(layout["ring"][:int(layout["ring_regs"])].tolist())
    ok = layout["plant_phase_ok"].astype(bool)
    for slot, reg in enumerate(regs):
        for phase in range(4):
            assert ok[slot, phase] == bool(layout["marched"][phase >> 1][reg])
        assert ok[slot, ops.REGFILE_ROTATE] == (reg in ring)
        assert ok[slot].any()
    for lay in range(2):  # each layout's temporaries hold a slot, which only the other layout verifies
        held = [r for r in regs if r in set(layout["temp_regs"][lay].tolist())]
        assert held and all(layout["marched"][1 - lay][r] for r in held)


@pytest.mark.parametrize("seed", SEEDS)
def test_pattern(layout, seed):
    for wave in (0, 7):
        p0, p1 = fill(seed, wave), fill(seed, wave, inverse=True)
        assert ((p0 ^ p1) == M32).all()  # across the two passes every bit of every cell holds 0 and 1
        assert all(len(set(p0[:, lane].tolist())) == 512 for lane in range(64))  # no two registers of a lane are equal
        assert all(len(set(p0[reg].tolist())) == 64 for reg in range(512))  # no two lanes of a register
        for phase in range(4):
            want = np.where(layout["marched"][phase >> 1].astype(bool)[:, None], p1 if phase & 1 else p0, 0)
            assert (ops.regfile_expected(wave, phase, seed=seed) == want).all()
    assert (fill(seed, 0) != fill(seed, 1)).any()


def test_rotation_and_a_plants_journey(layout):
    n = int(layout["ring_regs"])
    ring = layout["ring"][:n]
    filled = fill(0x5EED, 3)
    ok = layout["plant_phase_ok"].astype(bool)
    slot = max(s for s in range(8) if ok[s, ops.REGFILE_ROTATE])
    reg, lane, mask = int(layout["plant_regs"][slot]), 31, 0x80000001
    at = ring.tolist().index(reg)
    for sweeps in (1, n - 1, n, n + 1):
        got = ops.regfile_expected(3, ops.REGFILE_ROTATE, sweeps=sweeps, seed=0x5EED)
        assert (got[ring] == filled[np.roll(ring, -(sweeps % n))]).all()  # ring index i holds the fill of index i + sweeps
        assert (got[layout["temp_regs"][0]] == 0).all()
        planted = ops.regfile_expected(3, ops.REGFILE_ROTATE, sweeps=sweeps, plants=[(3, ops.REGFILE_ROTATE, slot, lane, mask)], seed=0x5EED)
        diff = planted ^ got
        where = int(ring[(at - sweeps) % n])  # the planted word has moved `sweeps` places down the ring
        assert diff[where, lane] == mask and np.count_nonzero(diff) == 1
    # a plant of another wave, or of another phase, is not this wave's
    clean = ops.regfile_expected(3, 0, seed=0x5EED)
    assert (ops.regfile_expected(3, 0, plants=[(2, 0, slot, lane, mask), (3, 1, slot, lane, mask)], seed=0x5EED) == clean).all()
    every = ops.regfile_expected(3, 0, plants=[(ops.ALL_WAVES, 0, slot, lane, mask)], seed=0x5EED)
    assert (every ^ clean)[reg, lane] == mask and np.count_nonzero(every ^ clean) == 1
